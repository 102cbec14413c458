"""The distributed 1-D transform behind the C ABI (include/fftw3_amd.h, fftw3_amd/csrc/slab1d.c): the reference's
fftw_mpi_local_size_1d / fftw_mpi_plan_dft_1d with the communicator replaced by a list of devices of one process.
The one-GPU box runs it with the same device named several times (devs = {0, 0, ...}): the local plans, the twiddle
kernel, the peer-to-peer exchanges and the event ordering are the same, only the copies stay on one card."""
import numpy as np
import pytest

import fftw3_amd as fa
from util import TOL, aerror, crand, oracle_dft

SIN, SOUT = fa.SLAB_SCRAMBLED_IN, fa.SLAB_SCRAMBLED_OUT


# ---- CPU tier ------------------------------------------------------------------------------------------------------

def test_local_size_1d_blocks_cover_the_transform():
    for n, ndev in [(4096, 1), (4096, 2), (4096, 4), (1296, 3), (3 << 20, 4), (1 << 31, 2), (13, 1), (36, 2)]:
        for sign in (fa.FORWARD, fa.BACKWARD):
            for flags in (0, SIN, SOUT, SIN | SOUT):
                ci = co = 0
                for g in range(ndev):
                    tot, ni, i0, no, o0 = fa.slab_local_size_1d(n, ndev, g, sign, flags)
                    assert (ni, no) == (n // ndev, n // ndev) and tot == n // ndev
                    assert (i0, o0) == (ci, co)
                    ci += ni
                    co += no
                assert ci == co == n


def test_local_size_1d_rejects_impossible_splits():
    assert fa.slab_local_size_1d(7, 2, 0, fa.FORWARD)[0] == -1          # a prime over two devices
    assert fa.slab_local_size_1d(24, 4, 0, fa.FORWARD)[0] == -1         # 16 does not divide 24
    assert fa.slab_local_size_1d(4096, 2, 2, fa.FORWARD)[0] == -1       # no device 2 of 2
    assert fa.slab_local_size_1d(0, 1, 0, fa.FORWARD)[0] == -1
    for n in (1, 2, 7, 13, 97, 1000003):                                  # one device: every n has a split
        assert fa.slab_local_size_1d(n, 1, 0, fa.FORWARD)[0] == n
        n0, n1 = fa.slab_split_1d(n, 1, fa.FORWARD)
        assert n0 * n1 == n
    with pytest.raises(ValueError):
        fa.SlabPlan1dC(24, [0] * 4, [np.zeros(6, complex)] * 4, [np.zeros(6, complex)] * 4, fa.FORWARD)


def _batch(s):
    return int(s.split("batch=")[1].split()[0])


def test_backward_split_is_the_forward_split_swapped():
    for n, ndev in [(4096, 4), (1296, 3), (3 << 20, 2), (1 << 20, 4), (1 << 31, 2)]:
        f = fa.slab_split_1d(n, ndev, fa.FORWARD)
        b = fa.slab_split_1d(n, ndev, fa.BACKWARD)
        assert f is not None and b == (f[1], f[0]) and f[0] % ndev == 0 and f[1] % ndev == 0
        assert fa.slab_split_1d(n, ndev, fa.FORWARD) == f                 # deterministic
        if n > 1 << 22:
            continue
        bufs = [np.zeros(n // ndev, dtype=complex) for _ in range(ndev)]
        pf = fa.SlabPlan1dC(n, [0] * ndev, bufs, bufs, fa.FORWARD)
        pb = fa.SlabPlan1dC(n, [0] * ndev, bufs, bufs, fa.BACKWARD)
        assert fa.lib.fftw_amd_slab_num_devices(pf.handle) == ndev
        for g in range(ndev):
            # column plan: w = n1 / P transforms of length n0; row plan: h = n0 / P transforms of length n1
            assert _batch(pf.local_plan_sprint(g, 1)) == f[1] // ndev
            assert _batch(pf.local_plan_sprint(g, 0)) == f[0] // ndev
            assert _batch(pb.local_plan_sprint(g, 1)) == f[0] // ndev
            assert _batch(pb.local_plan_sprint(g, 0)) == f[1] // ndev
        assert pf.local_plan_sprint(ndev, 0) is None
        pf.destroy()
        pb.destroy()


def test_split_prefers_balanced_lengths_with_register_kernels():
    assert fa.slab_split_1d(4096, 4, fa.FORWARD) == (64, 64)
    assert fa.slab_split_1d(1 << 26, 4, fa.FORWARD) == (8192, 8192)
    n0, n1 = fa.slab_split_1d(3 << 20, 4, fa.FORWARD)
    assert n0 * n1 == 3 << 20 and max(n0, n1) <= 4 * min(n0, n1)


def test_1d_plan_rejects_bad_arguments_and_is_built_without_a_device():
    bufs = [np.zeros(1024, dtype=complex) for _ in range(4)]
    assert fa.slab_local_size_1d(4096, 0, 0, fa.FORWARD)[0] == -1
    assert fa.slab_local_size_1d(4096 * 33 * 33, 33, 0, fa.FORWARD)[0] == -1
    for n, devs in [(4096, []), (4096 * 33 * 33, [0] * 33), (0, [0, 0]), (-4096, [0, 0]), (4096, [0, -1])]:
        arrs = [np.zeros(8, dtype=complex)] * max(1, len(devs))
        with pytest.raises(ValueError):
            fa.SlabPlan1dC(n, devs, arrs, arrs, fa.FORWARD)
    with pytest.raises(ValueError):
        fa.SlabPlan1dC(4096, [0, 0], bufs[:2], bufs[:2], 0)                    # no such sign
    with pytest.raises(ValueError):
        fa.SlabPlanC([4096], [0], bufs[:1], bufs[:1], fa.FORWARD)             # the rank-2/3 planner keeps rejecting rank 1
    for flags in (0, SIN, SOUT, SIN | SOUT):
        sp = fa.SlabPlan1dC(4096, [0] * 4, bufs, bufs, fa.FORWARD, fa.ESTIMATE | flags)
        assert sp.local_plan_sprint(3, 0) is not None and sp.local_plan_sprint(3, 1) is not None
        if fa.device_count() == 0:
            with pytest.raises(RuntimeError):
                sp.execute()
        sp.destroy()


def _dft(a, axis, sign):
    return np.fft.fft(a, axis=axis) if sign == fa.FORWARD else np.fft.ifft(a, axis=axis) * a.shape[axis]


def _six_steps(ins, n, ndev, sign, flags):
    """numpy model of slab1d.c with the planner's split: per-device inputs in the plan's layout -> per-device outputs"""
    n0, n1 = fa.slab_split_1d(n, ndev, sign)
    h, w = n0 // ndev, n1 // ndev
    W = []
    for r in range(ndev):
        if flags & SIN:
            Wr = ins[r].reshape(w, n0).T
        else:
            Wr = np.concatenate([ins[g].reshape(h, n1)[:, r * w:(r + 1) * w] for g in range(ndev)], axis=0)
        Wr = _dft(Wr, 0, sign)
        m = (np.arange(n0)[:, None] * (r * w + np.arange(w))[None, :]) % n
        W.append(Wr * np.exp(sign * 2j * np.pi * m / n))
    outs = [_dft(np.concatenate([W[r][g * h:(g + 1) * h] for r in range(ndev)], axis=1), 1, sign) for g in range(ndev)]
    if flags & SOUT:
        return [o.reshape(-1) for o in outs]
    return [np.concatenate([outs[d].T[g * w:(g + 1) * w] for d in range(ndev)], axis=1).reshape(-1) for g in range(ndev)]


def _scramble_in(x, n, ndev, sign):
    """device inputs of a SCRAMBLED_IN plan: [j1 in block g of n1][j0], element x[n1 j0 + j1]"""
    n0, n1 = fa.slab_split_1d(n, ndev, sign)
    w = n1 // ndev
    return [np.ascontiguousarray(x.reshape(n0, n1)[:, g * w:(g + 1) * w].T).reshape(-1) for g in range(ndev)]


def _scrambled_out(X, n, ndev, sign):
    """device outputs of a SCRAMBLED_OUT plan: [k0 in block g of n0][k1], element X[k0 + n0 k1]"""
    n0, n1 = fa.slab_split_1d(n, ndev, sign)
    h = n0 // ndev
    return [np.ascontiguousarray(X.reshape(n1, n0)[:, g * h:(g + 1) * h].T).reshape(-1) for g in range(ndev)]


@pytest.mark.parametrize("n,ndev", [(4096, 1), (4096, 4), (1296, 3), (3 << 12, 2), (1 << 12, 2)])
def test_numpy_model_of_the_six_steps_pins_the_layouts(n, ndev):
    rng = np.random.default_rng(n + ndev)
    x = crand(rng, n)
    b = n // ndev
    for sign in (fa.FORWARD, fa.BACKWARD):
        X = _dft(x, 0, sign)
        blocks = [x[g * b:(g + 1) * b] for g in range(ndev)]
        got = np.concatenate(_six_steps(blocks, n, ndev, sign, 0))
        assert aerror(got, X) < TOL
        got = _six_steps(blocks, n, ndev, sign, SOUT)
        for o, want in zip(got, _scrambled_out(X, n, ndev, sign)):
            assert aerror(o, want) < TOL
        got = np.concatenate(_six_steps(_scramble_in(x, n, ndev, sign), n, ndev, sign, SIN))
        assert aerror(got, X) < TOL
    # FORWARD SCRAMBLED_OUT, then BACKWARD SCRAMBLED_IN: n x in normal order
    mid = _six_steps([x[g * b:(g + 1) * b] for g in range(ndev)], n, ndev, fa.FORWARD, SOUT)
    back = np.concatenate(_six_steps(mid, n, ndev, fa.BACKWARD, SIN))
    assert aerror(back, n * x) < TOL


# ---- GPU tier (one card, the same device named ndev times) ----------------------------------------------------------

def _taerror(a, b):
    """aerror of util on two device tensors"""
    import torch
    d = torch.view_as_real(a - b).abs().amax()
    na = torch.view_as_real(a).abs().amax(-1)
    nb = torch.view_as_real(b).abs().amax(-1)
    return float(d / torch.minimum(na, nb).amax())


def _run(n, ndev, blocks, sign, flags=0, inplace=False, twice=False):
    """device inputs -> device outputs of one 1-D slab plan over [0] * ndev"""
    import torch
    ins = [b.clone() for b in blocks]
    outs = ins if inplace else [torch.zeros_like(b) for b in ins]
    torch.cuda.synchronize()
    sp = fa.SlabPlan1dC(n, [0] * ndev, ins, outs, sign, fa.ESTIMATE | flags)
    sp.execute()
    if twice and not inplace:
        sp.execute()                                                      # a second run right behind the first
    sp.sync()
    sp.destroy()
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("n,ndev", [(4096, 1), (4096, 2), (4096, 4), (1296, 3)])
def test_slab1d_matches_the_oracle(n, ndev):
    import torch
    rng = np.random.default_rng(n * 7 + ndev)
    x = crand(rng, n)
    b = n // ndev
    blocks = [torch.from_numpy(x[g * b:(g + 1) * b].copy()).cuda() for g in range(ndev)]
    for sign in (fa.FORWARD, fa.BACKWARD):
        want = oracle_dft(x, (n,), 1, sign)
        for inplace in (False, True):
            outs = _run(n, ndev, blocks, sign, inplace=inplace, twice=True)
            got = np.concatenate([o.cpu().numpy() for o in outs])
            assert aerror(got, want) < TOL, (n, ndev, sign, inplace)
        # in place, executed twice back-to-back: the second run transforms the first one's output
        ins = [t.clone() for t in blocks]
        torch.cuda.synchronize()
        sp = fa.SlabPlan1dC(n, [0] * ndev, ins, ins, sign)
        sp.execute()
        sp.execute()
        sp.sync()
        sp.destroy()
        got = np.concatenate([o.cpu().numpy() for o in ins])
        assert aerror(got, oracle_dft(want, (n,), 1, sign)) < TOL, (n, ndev, sign, "in place twice")


@pytest.mark.gpu
@pytest.mark.parametrize("n,ndev", [(3 << 20, 2), (3 << 20, 4), (1 << 26, 4)])
def test_slab1d_matches_the_single_device_plan(n, ndev):
    import torch
    g_ = torch.Generator(device="cuda").manual_seed(n + ndev)
    x = torch.complex(torch.rand(n, dtype=torch.float64, device="cuda", generator=g_) - 0.5,
                      torch.rand(n, dtype=torch.float64, device="cuda", generator=g_) - 0.5)
    b = n // ndev
    for sign in (fa.FORWARD, fa.BACKWARD):
        want = torch.zeros_like(x)
        p = fa.plan_dft_1d(n, x, want, sign)
        p.execute()
        torch.cuda.synchronize()
        del p
        for inplace in (False, True):
            outs = _run(n, ndev, [x[g * b:(g + 1) * b] for g in range(ndev)], sign, inplace=inplace, twice=True)
            assert _taerror(torch.cat(outs), want) < TOL, (n, ndev, sign, inplace)
            del outs
        del want
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_slab1d_scrambled_layouts():
    import torch
    n, ndev = 1 << 20, 4
    b = n // ndev
    g_ = torch.Generator(device="cuda").manual_seed(5)
    x = torch.complex(torch.rand(n, dtype=torch.float64, device="cuda", generator=g_) - 0.5,
                      torch.rand(n, dtype=torch.float64, device="cuda", generator=g_) - 0.5)
    blocks = [x[g * b:(g + 1) * b] for g in range(ndev)]
    X = torch.cat(_run(n, ndev, blocks, fa.FORWARD))
    n0, n1 = fa.slab_split_1d(n, ndev, fa.FORWARD)
    h = n0 // ndev
    # SCRAMBLED_OUT: device g holds [k0 in block g of n0][k1], element X[k0 + n0 k1]
    for inplace in (False, True):
        so = _run(n, ndev, blocks, fa.FORWARD, SOUT, inplace=inplace, twice=True)
        for g in range(ndev):
            want = X.reshape(n1, n0)[:, g * h:(g + 1) * h].t().reshape(-1)
            assert _taerror(so[g], want) < TOL, (g, inplace)
    # FORWARD SCRAMBLED_OUT, then BACKWARD SCRAMBLED_IN: n x in normal order
    back = _run(n, ndev, so, fa.BACKWARD, SIN)
    assert _taerror(torch.cat(back), n * x) < TOL
    back = _run(n, ndev, so, fa.BACKWARD, SIN, inplace=True)
    assert _taerror(torch.cat(back), n * x) < TOL


def _tones(lo, cnt, n, tones):
    """sum of a exp(2 pi i ((f j) mod n) / n) over the tones (f, a), j in [lo, lo + cnt), generated on the device"""
    import torch
    j = torch.arange(lo, lo + cnt, dtype=torch.int64, device="cuda")
    out = torch.zeros(cnt, dtype=torch.complex128, device="cuda")
    for f, a in tones:
        ph = ((j * f) % n).to(torch.float64) * (2.0 * np.pi / n)
        out += torch.polar(torch.full_like(ph, a), ph)
        del ph
    return out


@pytest.mark.gpu
def test_slab1d_known_answer_beyond_the_int_api():
    """n = 2^31 over two devices, in place: a 32 GiB transform no fftw_plan_dft_1d call can express"""
    import torch
    n, ndev = 1 << 31, 2
    b = n // ndev
    tones = [(123456789, 1.0), (1987654321, 0.25)]
    bound = 1e-10 * n
    n0, n1 = fa.slab_split_1d(n, ndev, fa.FORWARD)
    step = 1 << 27
    for flags in (0, SOUT):
        data = [torch.empty(b, dtype=torch.complex128, device="cuda") for _ in range(ndev)]
        for g in range(ndev):
            for lo in range(0, b, step):
                data[g][lo:lo + step] = _tones(g * b + lo, step, n, tones)
        torch.cuda.synchronize()
        sp = fa.SlabPlan1dC(n, [0] * ndev, data, data, fa.FORWARD, fa.ESTIMATE | flags)
        sp.execute()
        sp.sync()
        sp.destroy()
        del sp
        torch.cuda.empty_cache()
        where = {}
        for f, a in tones:
            if flags & SOUT:
                k0, k1 = f % n0, f // n0
                g, off = k0 // (n0 // ndev), (k0 % (n0 // ndev)) * n1 + k1
            else:
                g, off = f // b, f % b
            where[(g, off)] = a * n
        for (g, off), want in where.items():
            v = complex(data[g][off].item())
            assert abs(v.real - want) < bound and abs(v.imag) < bound, (flags, g, off, v, want)
            data[g][off] = 0
        for g in range(ndev):
            for lo in range(0, b, step):
                assert float(torch.view_as_real(data[g][lo:lo + step]).abs().amax()) < bound, (flags, g, lo)
        del data
        torch.cuda.empty_cache()


C_SLAB1D = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <fftw3.h>
#include <fftw3_amd.h>
/* a C caller spreads one 4096-point transform over "two devices" (device 0 twice on this box) and checks one tone */
int main(void) {
    const long long n = 4096, f = 1234;
    const int ndev = 2, devs[2] = {0, 0};
    fftw_complex *h = (fftw_complex *)malloc((size_t)n * sizeof(fftw_complex));
    fftw_complex *in[2], *out[2];
    long long ni, i0, no, o0, i;
    int g;
    if (fftw_amd_device_count() < 1) { printf("no device\n"); return 2; }
    for (i = 0; i < n; ++i) { h[i][0] = cos(2 * M_PI * (double)((f * i) % n) / n); h[i][1] = sin(2 * M_PI * (double)((f * i) % n) / n); }
    for (g = 0; g < ndev; ++g) {
        long long elems = fftw_amd_slab_local_size_1d(n, ndev, g, FFTW_FORWARD, 0, &ni, &i0, &no, &o0);
        if (elems != n / ndev) { printf("local size %lld\n", elems); return 3; }
        in[g] = (fftw_complex *)fftw_amd_malloc_device((size_t)elems * sizeof(fftw_complex));
        out[g] = (fftw_complex *)fftw_amd_malloc_device((size_t)elems * sizeof(fftw_complex));
        fftw_amd_memcpy_to_device(in[g], h + i0, (size_t)ni * sizeof(fftw_complex));
    }
    fftw_amd_slab_plan sp = fftw_amd_slab_plan_dft_1d(n, ndev, devs, in, out, FFTW_FORWARD, FFTW_ESTIMATE);
    if (!sp) { printf("1-d slab planner returned NULL\n"); return 4; }
    fftw_amd_slab_execute(sp);
    fftw_amd_slab_sync(sp);
    for (g = 0; g < ndev; ++g) {
        fftw_amd_slab_local_size_1d(n, ndev, g, FFTW_FORWARD, 0, &ni, &i0, &no, &o0);
        fftw_amd_memcpy_to_host(h + o0, out[g], (size_t)no * sizeof(fftw_complex));
    }
    for (i = 0; i < n; ++i) {
        double re = h[i][0] - (i == f ? (double)n : 0.0), im = h[i][1];
        if (fabs(re) > 1e-10 * n || fabs(im) > 1e-10 * n) { printf("bin %lld: %g %g\n", i, h[i][0], h[i][1]); return 5; }
    }
    fftw_amd_destroy_slab_plan(sp);
    for (g = 0; g < ndev; ++g) { fftw_amd_free_device(in[g]); fftw_amd_free_device(out[g]); }
    free(h);
    printf("slab1d client ok\n");
    return 0;
}
"""


@pytest.mark.gpu
def test_c_client_spreads_one_1d_transform_over_two_streams_of_one_device(tmp_path):
    import os
    import subprocess
    from util import ROOT
    src = tmp_path / "slab1dc.c"
    exe = tmp_path / "slab1dc"
    src.write_text(C_SLAB1D)
    libdir = os.path.join(ROOT, "fftw3_amd", "lib")
    subprocess.run(["gcc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir,
                    "-lfftw3", "-Wl,-rpath," + libdir, "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "slab1d client ok" in r.stdout, r.stdout
