"""Real data and the TRANSPOSED layouts of the slab plans behind the C ABI (include/fftw3_amd.h,
fftw3_amd/csrc/slab.c, the transposing exchange of kernels_slab.hip): fftw_mpi_local_size_*_transposed,
fftw_mpi_plan_dft_r2c / _c2r_2d / _3d and FFTW_MPI_TRANSPOSED_IN / _OUT of the reference's fftw3-mpi.h with a list of
devices of one process in the place of the communicator.  Without a GPU: sizes, plan shapes, and a numpy replay of
every pipeline from the plan's own exchange list.  On the one-GPU box the device is named P times."""
import numpy as np
import pytest

import fftw3_amd as fa
from fftw3_amd import slab
from slab_layouts import KIND_FLAGS, T_IN, T_OUT, Geo, replay
from util import TOL, aerror, crand, oracle_c2r, oracle_dft, oracle_r2c, rrand


def test_local_size_transposed_matches_the_reference_block_rule():
    for n in ([7, 5], [64, 64], [100, 3], [5, 4, 3], [4096, 2049]):
        rest = int(np.prod(n[2:]))
        for ndev in (1, 2, 3, 8):
            cover0 = cover1 = 0
            for g in range(ndev):
                got = fa.slab_local_size_transposed(n, ndev, g)
                want = slab.local_size_2d_transposed(*n, ndev, g) if len(n) == 2 else slab.local_size_3d_transposed(*n, ndev, g)
                assert got == tuple(want), (n, ndev, g)
                tot, ln0, lo0, ln1, lo1 = got
                assert tot == max(ln0 * n[1] * rest, ln1 * n[0] * rest)
                assert (lo0 == cover0 or ln0 == 0) and (lo1 == cover1 or ln1 == 0)
                cover0 += ln0
                cover1 += ln1
            assert (cover0, cover1) == (n[0], n[1])


def _host_arrays(geo, flags):
    return [np.zeros(geo.elems(g, flags), dtype=complex) for g in range(geo.P)]


def test_every_kind_and_flag_combination_is_planned_without_a_device():
    for shape in ((96, 80), (40, 24, 16), (7, 5)):
        for kind, allowed in KIND_FLAGS.items():
            for flags in allowed:
                geo = Geo(kind, shape, 3)
                ins, outs = _host_arrays(geo, flags), _host_arrays(geo, flags)
                sp = geo.make_plan([0, 0, 0], ins, outs, fa.FORWARD, flags)
                assert fa.lib.fftw_amd_slab_num_devices(sp.handle) == 3
                assert sp.local_plan_sprint(0, 0) is not None and sp.local_plan_sprint(0, 1) is not None
                if fa.device_count() == 0:
                    with pytest.raises(RuntimeError):
                        sp.execute()
                sp.destroy()
    geo = Geo("r2c", (96, 80), 2)
    a = _host_arrays(geo, T_OUT)
    with pytest.raises(ValueError):
        fa.SlabPlanR2cC([96, 80], [0, 0], a, a, fa.ESTIMATE | T_IN)          # r2c starts from the normal layout
    with pytest.raises(ValueError):
        fa.SlabPlanC2rC([96, 80], [0, 0], a, a, fa.ESTIMATE | T_OUT)         # c2r ends in it
    with pytest.raises(ValueError):
        fa.SlabPlanR2cC([96], [0], a[:1], a[:1])                             # rank 1
    with pytest.raises(ValueError):
        fa.SlabPlanC2rC([96, 0], [0], a[:1], a[:1])                          # a zero extent
    with pytest.raises(ValueError):
        fa.SlabPlanC([0, 80], [0], a[:1], a[:1], fa.FORWARD, fa.ESTIMATE | T_OUT)
    with pytest.raises(ValueError):
        fa.SlabPlanR2cC([96, 80], [0, 0], [a[0], None], a, fa.ESTIMATE | T_OUT)   # NULL array of a non-empty block
    with pytest.raises(ValueError):
        fa.SlabPlanC([96, 80], [0, 0], a, [a[0], None], fa.FORWARD, fa.ESTIMATE | T_IN)
    # (5, 5) on 4 devices: device 3 owns nothing in either layout and may pass NULL
    geo = Geo("c2c", (5, 5), 4)
    b = _host_arrays(geo, T_OUT)
    assert geo.cuts[3][1] == 0 and geo.cuts[3][3] == 0
    fa.SlabPlanC([5, 5], [0] * 4, b[:3] + [None], b[:3] + [None], fa.FORWARD, fa.ESTIMATE | T_OUT).destroy()


@pytest.mark.parametrize("n0", [1024, 4096])
def test_transposed_out_runs_the_first_dimension_along_contiguous_rows(n0):
    """the point of the transposing exchange: for rank 2 the length-n0 plan is a plan over contiguous interleaved
    rows, and for a length with a one-trip rows kernel exactly one step"""
    for kind, n1 in (("c2c", 512), ("r2c", 1026)):
        geo = Geo(kind, (n0, n1), 2)
        ins, outs = _host_arrays(geo, T_OUT), _host_arrays(geo, T_OUT)
        sp = geo.make_plan([0, 0], ins, outs, fa.FORWARD, T_OUT)
        for g in range(2):
            steps = sp.local_plan_steps(g, 1)
            assert len(steps) == 1, sp.local_plan_sprint(g, 1)
            d = steps[0]
            assert d.kind == 1 and d.L == n0 and d.is_l == 2 and d.os_l == 2       # FFTW_AMD_STEP_PASS over unit-stride rows
            assert "batch=%d" % geo.cuts[g][3] in sp.local_plan_sprint(g, 1)
        sp.destroy()
    # the normal-order plan of the same problem runs the same transforms DOWN its column block instead
    geo = Geo("c2c", (n0, 512), 2)
    ins = _host_arrays(geo, 0)
    sp = geo.make_plan([0, 0], ins, ins, fa.FORWARD, 0)
    assert all(d.is_l == 2 * 256 for d in sp.local_plan_steps(0, 1) if d.kind == 1 and d.L == n0)
    sp.destroy()


def _global_input(geo, rng):
    if geo.kind == "c2c":
        return crand(rng, *geo.shape)
    x = rrand(rng, *geo.shape)
    return x if geo.kind == "r2c" else np.fft.rfftn(x)


def _cut_input(geo, x, g, flags):
    """device g's input as a flat complex array (real rows viewed as complex)"""
    if geo.kind == "r2c":
        part = geo.cut_real(x, g).view(np.complex128)
    else:
        part = geo.cut(x, g, bool(flags & T_IN))
    out = np.zeros(geo.elems(g, flags), dtype=complex)
    out[:part.size] = part
    return out


def _join_output(geo, outs, flags):
    if geo.kind == "c2r":
        return geo.join_real([np.asarray(o).view(np.float64) for o in outs])
    return geo.join(outs, bool(flags & T_OUT))


REPLAY_SHAPES = [(7, 5), (12, 10), (9, 11), (6, 5, 4), (5, 6, 7), (16, 24)]


@pytest.mark.parametrize("kind", ["c2c", "r2c", "c2r"])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_numpy_replay_of_the_pipelines(kind, P):
    """local plans from numpy.fft, exchanges from fftw_amd_slab_exchange_ops (what the executor iterates): the replayed
    pipeline gives numpy's fftn / rfftn / irfftn * N in the documented layouts; uneven blocks, an empty block
    ((7, 5) on 4), odd nc ((12, 10): 6, (6, 5, 4): 3; (9, 11) and (5, 6, 7): odd last dimension)"""
    rng = np.random.default_rng(P)
    for shape in REPLAY_SHAPES:
        for flags in KIND_FLAGS[kind]:
            for sign in ((-1, 1) if kind == "c2c" else (-1 if kind == "r2c" else 1,)):
                geo = Geo(kind, shape, P)
                x = _global_input(geo, rng)
                ins = [_cut_input(geo, x, g, flags) for g in range(P)]
                outs = _host_arrays(geo, flags)
                sp = geo.make_plan([0] * P, ins, outs, sign, flags)
                got = _join_output(geo, replay(geo, sp, ins, sign, flags), flags)
                want = geo.expected(x, sign)
                assert aerror(got.reshape(1, -1), want.reshape(1, -1)) < 1e-12, (kind, shape, P, flags, sign)
                sp.destroy()


# ---------------------------------------------------------------------------------------------------------- GPU tier

GPU_CASES = [((96, 80), 3), ((7, 5), 4), ((1024, 512), 2), ((64, 64), 1), ((40, 24, 16), 2), ((128, 128, 128), 2),
             ((4096, 4096), 2), ((96, 81), 3), ((40, 24, 15), 4)]


def _single_device(kind, shape, x, sign):
    """the whole transform by ONE ordinary plan of the library"""
    import torch
    dev = torch.device("cuda:0")
    n = int(np.prod(shape))
    nc = shape[-1] // 2 + 1
    nh = n // shape[-1] * nc
    if kind == "c2c":
        xd = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dev)
        yd = torch.zeros_like(xd)
        fa.plan_many_dft(len(shape), list(shape), 1, xd, None, 1, n, yd, None, 1, n, sign).execute()
    elif kind == "r2c":
        xd = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dev)
        yd = torch.zeros(nh, dtype=torch.complex128, device=dev)
        fa.plan_many_dft_r2c(len(shape), list(shape), 1, xd, None, 1, n, yd, None, 1, nh).execute()
    else:
        xd = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dev)
        yd = torch.zeros(n, dtype=torch.float64, device=dev)
        fa.plan_many_dft_c2r(len(shape), list(shape), 1, xd, None, 1, nh, yd, None, 1, n).execute()
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _oracle(kind, shape, x, sign):
    if kind == "c2c":
        return oracle_dft(x.reshape(1, -1), shape, 1, sign)
    if kind == "r2c":
        return oracle_r2c(x.reshape(1, -1), shape, 1)
    return oracle_c2r(x.reshape(1, -1), shape, 1)


def _run_on_gpu(geo, x, sign, flags, inplace, twice):
    import torch
    dev = torch.device("cuda:0")
    P = geo.P
    ins = [torch.from_numpy(_cut_input(geo, x, g, flags)).to(dev) for g in range(P)]
    outs = ins if inplace else [torch.full_like(t, float("nan")) for t in ins]
    sp = geo.make_plan([0] * P, ins, outs, sign, flags)
    sp.execute()
    if twice:
        assert not inplace
        sp.execute()                                                  # a second run right behind the first
    sp.sync()
    torch.cuda.synchronize()
    got = _join_output(geo, [o.cpu().numpy() for o in outs], flags)
    sp.destroy()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["c2c", "r2c", "c2r"])
@pytest.mark.parametrize("shape,ndev", GPU_CASES)
def test_slab_plans_match_the_single_device_plan(kind, shape, ndev):
    rng = np.random.default_rng(sum(shape) + ndev)
    n = int(np.prod(shape))
    geo = Geo(kind, shape, ndev)
    for sign in ((-1, 1) if kind == "c2c" else (-1 if kind == "r2c" else 1,)):
        x = crand(rng, *shape) if kind == "c2c" else rrand(rng, *shape)
        if kind == "c2r":
            x = _single_device("r2c", shape, x, -1).reshape(geo.cdims)     # a Hermitian-consistent half spectrum
        want = _single_device(kind, shape, x, sign).reshape(1, -1)
        if n <= 1 << 16:
            assert aerror(want, np.asarray(_oracle(kind, shape, x, sign)).reshape(1, -1)) < TOL
        for flags in KIND_FLAGS[kind]:
            if kind == "c2c" and flags == 0:
                continue                                              # tests/test_slab_cabi.py
            for inplace, twice in ((False, True), (True, False)):
                got = _run_on_gpu(geo, x, sign, flags, inplace, twice)
                e = aerror(got.reshape(1, -1), want)
                print("slab %s %s P=%d sign=%d flags=%#x inplace=%d: %.3e" % (kind, shape, ndev, sign, flags, inplace, e))
                assert e < TOL, (kind, shape, ndev, sign, hex(flags), inplace)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,ndev", [((96, 80), 3), ((7, 5), 4), ((1024, 512), 2), ((40, 24, 15), 4), ((128, 128, 128), 2)])
def test_round_trips_through_the_transposed_layout(shape, ndev):
    """forward TRANSPOSED_OUT, then backward TRANSPOSED_IN on the arrays the first plan left: N x, two exchanges"""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7 + ndev)
    n = int(np.prod(shape))
    for fwd, bwd in (("r2c", "c2r"), ("c2c", "c2c")):
        gf, gb = Geo(fwd, shape, ndev), Geo(bwd, shape, ndev)
        x = rrand(rng, *shape) if fwd == "r2c" else crand(rng, *shape)
        a = [torch.from_numpy(_cut_input(gf, x, g, T_OUT)).to(dev) for g in range(ndev)]
        b = [torch.zeros_like(t) for t in a]
        c = [torch.zeros_like(t) for t in a]
        pf = gf.make_plan([0] * ndev, a, b, -1, T_OUT)
        pb = gb.make_plan([0] * ndev, b, c, 1, T_IN)
        pf.execute()
        pf.sync()
        pb.execute()
        pb.sync()
        torch.cuda.synchronize()
        got = _join_output(gb, [t.cpu().numpy() for t in c], T_IN)
        e = aerror(got.reshape(1, -1), (n * x).reshape(1, -1))
        print("round trip %s %s P=%d: %.3e" % (fwd, shape, ndev, e))
        assert e < TOL, (fwd, shape, ndev)
        pf.destroy()
        pb.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [-1, 0, 1])
@pytest.mark.parametrize("rest", [1, 2, 3, 4, 5, 6, 7, 8, 9, 513])
def test_transposing_exchange_kernel_is_an_exact_permutation(rest, nt):
    """the kernel by itself, both regimes (every LDS tile instantiation rest = 1 ... 7, direct runs from 8 on), plain
    and nontemporal accesses and the launcher's own choice, three sources with extents that are no multiples of the
    tile, padded strides on both sides: bit for bit the numpy permutation"""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(rest)
    B = 37 if rest < 100 else 5
    As = [45, 1, 19] if rest < 100 else [3, 1, 2]
    atot = sum(As)
    da, db = rest + (2 if rest > 1 else 0), (atot + 3) * (rest + 2)      # destination [B][atot + 3][da]
    dst = torch.full((B * db + 5,), float("nan"), dtype=torch.complex128, device=dev)
    want = dst.cpu().numpy().copy()
    blocks, keep, a0 = [], [], 0
    for A in As:
        sb = rest + 1
        sa = B * sb + 7
        src = crand(rng, A * sa)
        for a in range(A):
            for b in range(B):
                o = 5 + b * db + (a0 + a) * da
                want[o:o + rest] = src[a * sa + b * sb:a * sa + b * sb + rest]
        t = torch.from_numpy(src).to(dev)
        keep.append(t)
        blocks.append((t, 5 + a0 * da, A, B, sa, sb))
        a0 += A
    assert fa.slab_block_transpose(dst, da, db, rest, blocks, nt=nt) == 0
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))      # NaN padding untouched, payload identical
    # arguments the launcher cannot run are refused, not launched
    assert fa.slab_block_transpose(dst, 0, db, rest, blocks) == 1
    assert fa.slab_block_transpose(dst, da, db, rest, [(keep[0], 0, -1, B, 1, 1)]) == 1


C_SLAB_REAL = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <fftw3.h>
#include <fftw3_amd.h>
/* the loop of a distributed spectral code on "three devices" (device 0 three times on this box): r2c TRANSPOSED_OUT,
   pointwise scaling of the spectrum in the transposed layout, c2r TRANSPOSED_IN; x must come back */
int main(void) {
    const long long n[2] = {192, 150}, nc = 150 / 2 + 1, cn[2] = {192, 150 / 2 + 1};
    const int ndev = 3, devs[3] = {0, 0, 0};
    const double scale = 1.0 / (double)(n[0] * n[1]);
    double *x = (double *)malloc((size_t)(n[0] * n[1]) * sizeof(double));
    double *re[3];
    fftw_complex *sp[3];
    long long elems[3], ln0[3], lo0[3], ln1[3], lo1[3], i, j;
    double worst = 0.0;
    int g;
    if (fftw_amd_device_count() < 1) { printf("no device\n"); return 2; }
    srand48(3);
    for (i = 0; i < n[0] * n[1]; ++i) x[i] = drand48() - 0.5;
    for (g = 0; g < ndev; ++g) {
        elems[g] = fftw_amd_slab_local_size_transposed(2, cn, ndev, g, &ln0[g], &lo0[g], &ln1[g], &lo1[g]);
        double *h = (double *)calloc((size_t)(2 * elems[g] + 2), sizeof(double));
        re[g] = (double *)fftw_amd_malloc_device((size_t)(2 * elems[g] + 2) * sizeof(double));
        sp[g] = (fftw_complex *)fftw_amd_malloc_device((size_t)(elems[g] + 1) * sizeof(fftw_complex));
        for (i = 0; i < ln0[g]; ++i)
            for (j = 0; j < n[1]; ++j) h[i * 2 * nc + j] = x[(lo0[g] + i) * n[1] + j];      /* rows padded to 2 nc */
        fftw_amd_memcpy_to_device(re[g], h, (size_t)(2 * elems[g]) * sizeof(double));
        free(h);
    }
    fftw_amd_slab_plan fw = fftw_amd_slab_plan_dft_r2c(2, n, ndev, devs, re, sp, FFTW_ESTIMATE | FFTW_AMD_SLAB_TRANSPOSED_OUT);
    fftw_amd_slab_plan bw = fftw_amd_slab_plan_dft_c2r(2, n, ndev, devs, sp, re, FFTW_ESTIMATE | FFTW_AMD_SLAB_TRANSPOSED_IN);
    if (!fw || !bw) { printf("slab planner returned NULL\n"); return 3; }
    if (fftw_amd_slab_plan_dft_r2c(2, n, ndev, devs, re, sp, FFTW_AMD_SLAB_TRANSPOSED_IN)) { printf("r2c took TRANSPOSED_IN\n"); return 4; }
    fftw_amd_slab_execute(fw);
    fftw_amd_slab_sync(fw);
    for (g = 0; g < ndev; ++g) {
        /* the spectrum of device g: [local_n1][n0] complex; scale it on the host (the pointwise work of the loop) */
        size_t cnt = (size_t)(ln1[g] * n[0]);
        fftw_complex *h = (fftw_complex *)malloc((cnt + 1) * sizeof(fftw_complex));
        fftw_amd_memcpy_to_host(h, sp[g], cnt * sizeof(fftw_complex));
        for (i = 0; i < (long long)cnt; ++i) { h[i][0] *= scale; h[i][1] *= scale; }
        fftw_amd_memcpy_to_device(sp[g], h, cnt * sizeof(fftw_complex));
        free(h);
    }
    fftw_amd_slab_execute(bw);
    fftw_amd_slab_sync(bw);
    for (g = 0; g < ndev; ++g) {
        double *h = (double *)malloc((size_t)(2 * elems[g] + 2) * sizeof(double));
        fftw_amd_memcpy_to_host(h, re[g], (size_t)(2 * elems[g]) * sizeof(double));
        for (i = 0; i < ln0[g]; ++i)
            for (j = 0; j < n[1]; ++j) {
                double d = fabs(h[i * 2 * nc + j] - x[(lo0[g] + i) * n[1] + j]);
                if (d > worst) worst = d;
            }
        free(h);
    }
    if (!(worst <= 1e-12)) { printf("round trip differs: %g\n", worst); return 5; }
    fftw_amd_destroy_slab_plan(fw);
    fftw_amd_destroy_slab_plan(bw);
    for (g = 0; g < ndev; ++g) { fftw_amd_free_device(re[g]); fftw_amd_free_device(sp[g]); }
    free(x);
    printf("slab real client ok\n");
    return 0;
}
"""


@pytest.mark.gpu
def test_c_client_round_trips_real_data_through_the_transposed_layout(tmp_path):
    import os
    import subprocess
    from util import ROOT
    src = tmp_path / "slabr.c"
    exe = tmp_path / "slabr"
    src.write_text(C_SLAB_REAL)
    libdir = os.path.join(ROOT, "fftw3_amd", "lib")
    subprocess.run(["gcc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir,
                    "-lfftw3", "-Wl,-rpath," + libdir, "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "slab real client ok" in r.stdout, r.stdout
