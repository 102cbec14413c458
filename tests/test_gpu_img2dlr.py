"""The one-trip real-image kernels for extents above 32 on the GPU (pass2dlr.hpp, FFTW_AMD_K_IMG2DLR), reached through
FFTW_AMD_REAL_IMGL=1.

Every pair of img2dlr_menu.inc runs r2c and c2r out of place on 2T + 3 images (two full tiles and a partial one), the
device arrays inside the NaN-patterned arenas of tests/footprint.py: no guard violations, the input preserved bit for
bit, relative L-infinity error at most util.TOL against the oracle (the c2r from random complex half spectra, which
are not Hermitian) and the rms gate of tests/accuracy.py against the long-double DFT of the real images -- for the c2r
gate the input is the r2c spectrum of real images, whose c2r is n0 n1 times those images.  The eight pairs of the CPU
tier also run in place with padded rows, on a single image, twice (bit-identical), out of place with padded real rows,
and through the FFTW_UNALIGNED twin on arrays 8 bytes off.  One batch above the 384 MiB rule runs the nontemporal
forms, and one FFTW_MEASURE plan runs whichever candidate wins and round-trips through wisdom."""
import numpy as np
import pytest

import accuracy as A
import fftw3_amd as fa
import footprint as F
from accuracy_cases import knobs
from test_img2dlr_plans import MENU, ON, PAIRS, tile
from util import TOL, aerror, crand, oracle_c2r, oracle_r2c, rrand

A.require_longdouble()
pytestmark = pytest.mark.gpu

EIGHT = list(PAIRS)


def _label(n0, n1, fwd):
    return "pass-%d/img2dl-%s-%dx%d tile=%d" % (n1, "r2c" if fwd else "c2r", n0, n1, tile(n0, n1, fwd))


@pytest.fixture(scope="module")
def dev():
    import torch
    assert fa.device_count() > 0
    return torch.device("cuda:0")


def _problem(n0, n1, hm, fwd, layout):
    """layout: "dense", "padded" (out of place, real rows of n1 + 2 doubles) or "inplace" (padded rows, one array)"""
    h = n1 // 2 + 1
    real = F.Layout() if layout == "dense" else F.Layout((n0, 2 * h), 1, n0 * 2 * h)
    cplx = F.Layout() if layout == "dense" else F.Layout((n0, h), 1, n0 * h)
    lin, lout = (real, cplx) if fwd else (cplx, real)
    return F.Problem("r2c" if fwd else "c2r", (n0, n1), hm, lin, lout, inplace=layout == "inplace")


def _run(dev, n0, n1, hm, fwd, layout, x, twice=False):
    """the plan on device arenas; returns (result, violations, input kept, bit-identical repeat)"""
    import torch
    prob = _problem(n0, n1, hm, fwd, layout)
    AR = prob.arenas()
    prob.scatter(AR, x)
    full = [a.to_device(dev) for a in AR]
    ref = [t.clone() for t in full]
    with knobs(ON):
        p = prob.plan(fa, [t[a.lo:] for t, a in zip(full, AR)])
    assert _label(n0, n1, fwd) in p.sprint() and len(p.steps()) == 1, p.sprint()
    p.execute()
    p.sync()
    torch.cuda.synchronize()
    viol = [F.check(r, t, w) for r, t, w in zip(ref, full, prob.written(AR))]
    kept = None if prob.inplace else F.same_bits(full[0], ref[0])
    first = [t.clone() for t in full]
    repeat = None
    if twice:
        for t, r in zip(full, ref):
            t.copy_(r)
        p.execute()
        p.sync()
        torch.cuda.synchronize()
        repeat = all(F.same_bits(t, f) for t, f in zip(full, first))
    out = first[-1][AR[-1].lo:AR[-1].lo + AR[-1].span].cpu().numpy()
    return prob.gather([out]), viol, kept, repeat


def _inputs(n0, n1, hm, fwd):
    rng = np.random.default_rng(100 * n0 + n1 + (0 if fwd else 5))
    h = n1 // 2 + 1
    return rrand(rng, hm, n0, n1) if fwd else crand(rng, hm, n0, h)


def _oracle(n0, n1, hm, fwd, x):
    h = n1 // 2 + 1
    if fwd:
        return oracle_r2c(x.reshape(-1), (n0, n1), hm).reshape(hm, n0, h)
    return oracle_c2r(x.reshape(-1), (n0, n1), hm).reshape(hm, n0, n1)


def _check_against_oracle(n0, n1, hm, fwd, x, got, viol, kept, what):
    assert not any(viol), (n0, n1, fwd, what, viol)
    assert kept is not False, (n0, n1, fwd, what, "the input of an out-of-place plan changed")
    e = aerror(got, _oracle(n0, n1, hm, fwd, x))
    assert e <= TOL, (n0, n1, fwd, what, e)
    return e


@pytest.mark.parametrize("n0,n1", MENU, ids=["%dx%d" % p for p in MENU])
def test_every_menu_pair_both_directions(dev, n0, n1):
    h = n1 // 2 + 1
    # r2c: oracle, then the rms gate against the long-double DFT cut to h columns
    hm = 2 * tile(n0, n1, True) + 3
    x = _inputs(n0, n1, hm, True)
    got, viol, kept, _ = _run(dev, n0, n1, hm, True, "dense", x)
    e = _check_against_oracle(n0, n1, hm, True, x, got, viol, kept, "r2c")
    ld = A.ld_dft(x, (n0, n1), hm)[:, :, :h]
    eg, eo, en = (A.rms_err(v, ld) for v in (got, _oracle(n0, n1, hm, True, x), np.fft.rfft2(x, axes=(1, 2))))
    print("%dx%d r2c hm %d: Linf %.3g gpu %.3f u oracle %.3f u numpy %.3f u" % (n0, n1, hm, e, eg / A.U, eo / A.U, en / A.U))
    assert A.passes(eg, eo, en), (n0, n1, "r2c", eg / A.U, eo / A.U, en / A.U)
    # c2r: random complex half spectra against the oracle
    hm = 2 * tile(n0, n1, False) + 3
    y = _inputs(n0, n1, hm, False)
    got, viol, kept, _ = _run(dev, n0, n1, hm, False, "dense", y)
    e = _check_against_oracle(n0, n1, hm, False, y, got, viol, kept, "c2r")
    # ... and for the rms gate the c2r of r2c spectra: n0 n1 times the real images they came from
    xr = _inputs(n0, n1, hm, True)
    ldy = A.ld_dft(xr, (n0, n1), hm)
    yr = np.ascontiguousarray(ldy[:, :, :h]).astype(np.complex128)
    got, viol, kept, _ = _run(dev, n0, n1, hm, False, "dense", yr)
    assert not any(viol) and kept is not False
    # long-double reference of exactly this input: backward columns, Hermitian expansion row-wise, backward rows
    z = np.moveaxis(A.ld_dft(np.moveaxis(yr, 1, 2).reshape(-1, n0), (n0,), hm * h, +1).reshape(hm, h, n0), 2, 1)
    ld = A.ld_c2r(z.reshape(-1, h), n1, hm * n0).reshape(hm, n0, n1)
    eg, eo, en = (A.rms_err(v, ld) for v in (got, _oracle(n0, n1, hm, False, yr),
                                             np.fft.irfft2(yr, s=(n0, n1), axes=(1, 2), norm="forward")))
    print("%dx%d c2r hm %d: Linf %.3g gpu %.3f u oracle %.3f u numpy %.3f u" % (n0, n1, hm, e, eg / A.U, eo / A.U, en / A.U))
    assert A.passes(eg, eo, en), (n0, n1, "c2r", eg / A.U, eo / A.U, en / A.U)


@pytest.mark.parametrize("layout", ["dense", "padded", "inplace"])
@pytest.mark.parametrize("fwd", [True, False], ids=["r2c", "c2r"])
@pytest.mark.parametrize("n0,n1", EIGHT, ids=["%dx%d" % p for p in EIGHT])
def test_eight_pairs_every_form(dev, n0, n1, fwd, layout):
    T = tile(n0, n1, fwd)
    for hm in (1, 2 * T + 3):
        x = _inputs(n0, n1, hm, fwd)
        got, viol, kept, repeat = _run(dev, n0, n1, hm, fwd, layout, x, twice=True)
        _check_against_oracle(n0, n1, hm, fwd, x, got, viol, kept, (layout, hm))
        assert repeat, (n0, n1, fwd, layout, hm, "the second execution differs from the first")


@pytest.mark.parametrize("fwd", [True, False], ids=["r2c", "c2r"])
@pytest.mark.parametrize("n0,n1", EIGHT, ids=["%dx%d" % p for p in EIGHT])
def test_new_array_execute_8_bytes_off_goes_through_the_twin(dev, n0, n1, fwd):
    import torch
    hm = 2 * tile(n0, n1, fwd) + 3
    h = n1 // 2 + 1
    x = _inputs(n0, n1, hm, fwd)
    want = _oracle(n0, n1, hm, fwd, x).reshape(-1)
    nin, nout = (hm * n0 * n1, 2 * hm * n0 * h) if fwd else (2 * hm * n0 * h, hm * n0 * n1)
    al = torch.zeros(nin + 8, dtype=torch.float64, device=dev)
    ao = torch.zeros(nout + 8, dtype=torch.float64, device=dev)
    with knobs(ON):
        if fwd:
            p = fa.plan_many_dft_r2c(2, [n0, n1], hm, al, None, 1, n0 * n1, ao, None, 1, n0 * h)
        else:
            p = fa.plan_many_dft_c2r(2, [n0, n1], hm, al, None, 1, n0 * h, ao, None, 1, n0 * n1)
    assert _label(n0, n1, fwd) in p.sprint(), p.sprint()
    xin, xout = al[1:1 + nin], ao[1:1 + nout]
    assert xin.data_ptr() % 16 == 8 and xout.data_ptr() % 16 == 8
    flat = torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.float64))

    def result(t):
        r = t.cpu().numpy()
        return r.view(np.complex128) if fwd else r

    xin.copy_(flat)
    with knobs(ON):
        (p.execute_dft_r2c if fwd else p.execute_dft_c2r)(xin, xout)
    torch.cuda.synchronize()
    assert aerror(result(xout), want) <= TOL
    # the plan's own arrays still take the one-trip step
    al[:nin].copy_(flat)
    p.execute()
    torch.cuda.synchronize()
    assert aerror(result(ao[:nout]), want) <= TOL


@pytest.mark.parametrize("fwd", [True, False], ids=["r2c", "c2r"])
def test_large_batch_runs_the_nontemporal_forms(dev, fwd):
    """64 x 64 at the smallest batch above the 384 MiB rule of FFTW_AMD_NT = 1 (input plus output bytes) that is a
    multiple of a block of 256 distinct images.  The input repeats the block, so the output of every tile is compared
    against that block's transform."""
    import torch
    n0 = n1 = 64
    assert (n0, n1) in MENU
    blk, h = 256, 33
    per_block = blk * 8 * (n0 * n1 + 2 * n0 * h)
    hm = blk * -(-(384 << 20) // per_block)
    assert hm == 6144 and hm * per_block // blk >= 384 << 20 > (hm - blk) * per_block // blk
    x = _inputs(n0, n1, blk, fwd)
    want = torch.from_numpy(_oracle(n0, n1, blk, fwd, x).reshape(blk, -1)).to(dev)
    xd = torch.from_numpy(x.reshape(blk, -1)).to(dev).repeat(hm // blk, 1)
    yd = torch.zeros(hm, n0 * (h if fwd else n1), dtype=torch.complex128 if fwd else torch.float64, device=dev)
    with knobs(ON):
        if fwd:
            p = fa.plan_many_dft_r2c(2, [n0, n1], hm, xd, None, 1, n0 * n1, yd, None, 1, n0 * h)
        else:
            p = fa.plan_many_dft_c2r(2, [n0, n1], hm, xd, None, 1, n0 * h, yd, None, 1, n0 * n1)
    st = p.steps()
    assert len(st) == 1 and st[0].variant == fa.K_IMG2DLR, p.sprint()
    assert (st[0].flags & fa.F_NT_IN) and (st[0].flags & fa.F_NT_OUT), p.sprint()
    p.execute()
    p.sync()
    torch.cuda.synchronize()
    d = yd.reshape(hm // blk, blk, -1) - want[None]
    if fwd:
        err = float(torch.maximum(d.real.abs(), d.imag.abs()).max())
        mag = float(torch.maximum(want.real.abs(), want.imag.abs()).max())
    else:
        err, mag = float(d.abs().max()), float(want.abs().max())
    print("64x64 x %d %s: Linf %.3g" % (hm, "r2c" if fwd else "c2r", err / mag))
    assert err / mag <= TOL
    assert torch.equal(xd[:blk].cpu(), torch.from_numpy(x.reshape(blk, -1)))


def test_measure_times_the_one_trip_plan_and_wisdom_round_trips(dev):
    import torch
    n0 = n1 = 64
    hm, h = 1024, 33
    fa.forget_wisdom()
    try:
        x = _inputs(n0, n1, hm, True)
        want = _oracle(n0, n1, hm, True, x).reshape(hm, -1)
        xd = torch.from_numpy(x.reshape(hm, -1)).to(dev)
        yd = torch.zeros(hm, n0 * h, dtype=torch.complex128, device=dev)
        p = fa.plan_many_dft_r2c(2, [n0, n1], hm, xd, None, 1, n0 * n1, yd, None, 1, n0 * h, fa.MEASURE)
        text = fa.export_wisdom_to_string()
        assert "t1 s" in text and "64:64:66" in text, text
        xd.copy_(torch.from_numpy(x.reshape(hm, -1)))
        yd.zero_()
        p.execute()
        torch.cuda.synchronize()
        assert aerror(yd.cpu().numpy(), want) <= TOL, p.sprint()
        fa.forget_wisdom()
        assert fa.import_wisdom_from_string(text) == 1
        assert fa.export_wisdom_to_string() == text
        p2 = fa.plan_many_dft_r2c(2, [n0, n1], hm, xd, None, 1, n0 * n1, yd, None, 1, n0 * h, fa.ESTIMATE | fa.WISDOM_ONLY)
        assert p2.sprint() == p.sprint(), (p.sprint(), p2.sprint(), text)
        yd.zero_()
        p2.execute()
        torch.cuda.synchronize()
        assert aerror(yd.cpu().numpy(), want) <= TOL
        print("FFTW_MEASURE picked: %s" % p.sprint())
    finally:
        fa.forget_wisdom()
