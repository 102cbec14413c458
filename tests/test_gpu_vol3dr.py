"""The one-trip small real-volume kernels on the GPU (pass3dr.hpp, FFTW_AMD_K_VOL3DR), reached through
FFTW_AMD_REAL_VOL=1.

Every triple of vol3dr_menu.inc runs r2c and c2r out of place on 2T + 3 volumes (two full tiles and a partial one), the
device arrays inside the NaN-patterned arenas of tests/footprint.py: no guard violations, the input preserved bit for
bit, relative L-infinity error at most 1e-10 against the oracle (the c2r from random complex half spectra, which are
not Hermitian) and the rms gate of tests/accuracy.py against the long-double DFT of the real volumes -- for the c2r
gate the input is the r2c spectrum of real volumes, whose c2r is n0 n1 n2 times those volumes.  The triples of the CPU
tier also run in place with padded rows, on a single volume, twice (bit-identical), out of place with padded real
rows, and through the FFTW_UNALIGNED twin on arrays 8 bytes off.  One batch above the 384 MiB rule runs the
nontemporal forms, and one FFTW_MEASURE plan runs whichever candidate wins and round-trips through wisdom."""
import numpy as np
import pytest

import accuracy as A
import fftw3_amd as fa
import footprint as F
from accuracy_cases import knobs
from test_vol3dr_plans import MENU, ON, TRIPLES, tile
from util import TOL, aerror, crand, oracle_c2r, oracle_r2c, rrand

A.require_longdouble()
pytestmark = pytest.mark.gpu


def _id(t):
    return "%dx%dx%d" % t


def _label(t, fwd):
    return "pass-%d/vol3d-%s-%dx%dx%d tile=%d" % (t[2], "r2c" if fwd else "c2r", t[0], t[1], t[2], tile(t, fwd))


@pytest.fixture(scope="module")
def dev():
    import torch
    assert fa.device_count() > 0
    return torch.device("cuda:0")


def _problem(t, hm, fwd, layout):
    """layout: "dense", "padded" (out of place, real rows of n2 + 2 doubles) or "inplace" (padded rows, one array)"""
    n0, n1, n2 = t
    h = n2 // 2 + 1
    real = F.Layout() if layout == "dense" else F.Layout((n0, n1, 2 * h), 1, n0 * n1 * 2 * h)
    cplx = F.Layout() if layout == "dense" else F.Layout((n0, n1, h), 1, n0 * n1 * h)
    lin, lout = (real, cplx) if fwd else (cplx, real)
    return F.Problem("r2c" if fwd else "c2r", t, hm, lin, lout, inplace=layout == "inplace")


def _run(dev, t, hm, fwd, layout, x, twice=False):
    """the plan on device arenas; returns (result, violations, input kept, bit-identical repeat)"""
    import torch
    prob = _problem(t, hm, fwd, layout)
    AR = prob.arenas()
    prob.scatter(AR, x)
    full = [a.to_device(dev) for a in AR]
    ref = [v.clone() for v in full]
    with knobs(ON):
        p = prob.plan(fa, [v[a.lo:] for v, a in zip(full, AR)])
    assert _label(t, fwd) in p.sprint() and len(p.steps()) == 1, p.sprint()
    p.execute()
    p.sync()
    torch.cuda.synchronize()
    viol = [F.check(r, v, w) for r, v, w in zip(ref, full, prob.written(AR))]
    kept = None if prob.inplace else F.same_bits(full[0], ref[0])
    first = [v.clone() for v in full]
    repeat = None
    if twice:
        for v, r in zip(full, ref):
            v.copy_(r)
        p.execute()
        p.sync()
        torch.cuda.synchronize()
        repeat = all(F.same_bits(v, f) for v, f in zip(full, first))
    out = first[-1][AR[-1].lo:AR[-1].lo + AR[-1].span].cpu().numpy()
    return prob.gather([out]), viol, kept, repeat


def _inputs(t, hm, fwd):
    n0, n1, n2 = t
    rng = np.random.default_rng(10000 * n0 + 100 * n1 + n2 + (0 if fwd else 5))
    return rrand(rng, hm, n0, n1, n2) if fwd else crand(rng, hm, n0, n1, n2 // 2 + 1)


def _oracle(t, hm, fwd, x):
    n0, n1, n2 = t
    if fwd:
        return oracle_r2c(x.reshape(-1), t, hm).reshape(hm, n0, n1, n2 // 2 + 1)
    return oracle_c2r(x.reshape(-1), t, hm).reshape(hm, n0, n1, n2)


def _check_against_oracle(t, hm, fwd, x, got, viol, kept, what):
    assert not any(viol), (t, fwd, what, viol)
    assert kept is not False, (t, fwd, what, "the input of an out-of-place plan changed")
    e = aerror(np.asarray(got).reshape(-1), _oracle(t, hm, fwd, x).reshape(-1))
    assert e <= TOL, (t, fwd, what, e)
    return e


@pytest.mark.parametrize("t", MENU, ids=[_id(t) for t in MENU])
def test_every_menu_triple_both_directions(dev, t):
    n0, n1, n2 = t
    h = n2 // 2 + 1
    # r2c: oracle, then the rms gate against the long-double DFT cut to h columns
    hm = 2 * tile(t, True) + 3
    x = _inputs(t, hm, True)
    got, viol, kept, _ = _run(dev, t, hm, True, "dense", x)
    e = _check_against_oracle(t, hm, True, x, got, viol, kept, "r2c")
    ld = A.ld_dft(x, t, hm)[..., :h]
    eg, eo, en = (A.rms_err(v, ld) for v in (got, _oracle(t, hm, True, x), np.fft.rfftn(x, axes=(1, 2, 3))))
    print("%s r2c hm %d: Linf %.3g gpu %.3f u oracle %.3f u numpy %.3f u" % (_id(t), hm, e, eg / A.U, eo / A.U, en / A.U))
    assert A.passes(eg, eo, en), (t, "r2c", eg / A.U, eo / A.U, en / A.U)
    # c2r: random complex half spectra against the oracle
    hm = 2 * tile(t, False) + 3
    y = _inputs(t, hm, False)
    got, viol, kept, _ = _run(dev, t, hm, False, "dense", y)
    e = _check_against_oracle(t, hm, False, y, got, viol, kept, "c2r")
    # ... and for the rms gate the c2r of r2c spectra: n0 n1 n2 times the real volumes they came from
    xr = _inputs(t, hm, True)
    yr = np.ascontiguousarray(A.ld_dft(xr, t, hm)[..., :h]).astype(np.complex128)
    got, viol, kept, _ = _run(dev, t, hm, False, "dense", yr)
    assert not any(viol) and kept is not False
    # long-double reference of exactly this input: backward over the two leading axes of every column, then the
    # Hermitian expansion and the backward transform row by row
    z = np.moveaxis(A.ld_dft(np.moveaxis(yr, 3, 1).reshape(-1), (n0, n1), hm * h, +1).reshape(hm, h, n0, n1), 1, 3)
    ld = A.ld_c2r(np.ascontiguousarray(z).reshape(-1, h), n2, hm * n0 * n1).reshape(hm, n0, n1, n2)
    eg, eo, en = (A.rms_err(v, ld) for v in (got, _oracle(t, hm, False, yr),
                                             np.fft.irfftn(yr, s=t, axes=(1, 2, 3), norm="forward")))
    print("%s c2r hm %d: Linf %.3g gpu %.3f u oracle %.3f u numpy %.3f u" % (_id(t), hm, e, eg / A.U, eo / A.U, en / A.U))
    assert A.passes(eg, eo, en), (t, "c2r", eg / A.U, eo / A.U, en / A.U)


@pytest.mark.parametrize("layout", ["dense", "padded", "inplace"])
@pytest.mark.parametrize("fwd", [True, False], ids=["r2c", "c2r"])
@pytest.mark.parametrize("t", TRIPLES, ids=[_id(t) for t in TRIPLES])
def test_fixed_triples_every_form(dev, t, fwd, layout):
    T = tile(t, fwd)
    for hm in (1, 2 * T + 3):
        x = _inputs(t, hm, fwd)
        got, viol, kept, repeat = _run(dev, t, hm, fwd, layout, x, twice=True)
        _check_against_oracle(t, hm, fwd, x, got, viol, kept, (layout, hm))
        assert repeat, (t, fwd, layout, hm, "the second execution differs from the first")


@pytest.mark.parametrize("fwd", [True, False], ids=["r2c", "c2r"])
@pytest.mark.parametrize("t", TRIPLES, ids=[_id(t) for t in TRIPLES])
def test_new_array_execute_8_bytes_off_goes_through_the_twin(dev, t, fwd):
    import torch
    n0, n1, n2 = t
    hm = 2 * tile(t, fwd) + 3
    h = n2 // 2 + 1
    nr, nc = n0 * n1 * n2, n0 * n1 * h
    x = _inputs(t, hm, fwd)
    want = _oracle(t, hm, fwd, x).reshape(-1)
    nin, nout = (hm * nr, 2 * hm * nc) if fwd else (2 * hm * nc, hm * nr)
    al = torch.zeros(nin + 8, dtype=torch.float64, device=dev)
    ao = torch.zeros(nout + 8, dtype=torch.float64, device=dev)
    with knobs(ON):
        if fwd:
            p = fa.plan_many_dft_r2c(3, list(t), hm, al, None, 1, nr, ao, None, 1, nc)
        else:
            p = fa.plan_many_dft_c2r(3, list(t), hm, al, None, 1, nc, ao, None, 1, nr)
    assert _label(t, fwd) in p.sprint(), p.sprint()
    xin, xout = al[1:1 + nin], ao[1:1 + nout]
    assert xin.data_ptr() % 16 == 8 and xout.data_ptr() % 16 == 8
    flat = torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.float64))

    def result(v):
        r = v.cpu().numpy()
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
    """16 x 16 x 16 with 16384 volumes: 512 MiB of real data and 576 MiB of half spectra, above the 384 MiB rule of
    FFTW_AMD_NT = 1.  The input repeats a block of 512 distinct volumes, so the output of every tile is compared
    against that block's transform on the device."""
    import torch
    t = (16, 16, 16)
    assert t in MENU
    n0, n1, n2 = t
    hm, blk, h = 16384, 512, 9
    nr, nc = n0 * n1 * n2, n0 * n1 * h
    x = _inputs(t, blk, fwd)
    want = torch.from_numpy(_oracle(t, blk, fwd, x).reshape(blk, -1)).to(dev)
    xd = torch.from_numpy(x.reshape(blk, -1)).to(dev).repeat(hm // blk, 1)
    yd = torch.zeros(hm, nc if fwd else nr, dtype=torch.complex128 if fwd else torch.float64, device=dev)
    with knobs(ON):
        if fwd:
            p = fa.plan_many_dft_r2c(3, list(t), hm, xd, None, 1, nr, yd, None, 1, nc)
        else:
            p = fa.plan_many_dft_c2r(3, list(t), hm, xd, None, 1, nc, yd, None, 1, nr)
    st = p.steps()
    assert len(st) == 1 and st[0].variant == fa.K_VOL3DR, p.sprint()
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
    print("16x16x16 x %d %s: Linf %.3g" % (hm, "r2c" if fwd else "c2r", err / mag))
    assert err / mag <= TOL
    assert torch.equal(xd[:blk].cpu(), torch.from_numpy(x.reshape(blk, -1)))


def test_measure_times_the_one_trip_plan_and_wisdom_round_trips(dev):
    import torch
    t = (16, 16, 16)
    n0, n1, n2 = t
    hm, h = 1024, 9
    nr, nc = n0 * n1 * n2, n0 * n1 * h
    fa.forget_wisdom()
    try:
        x = _inputs(t, hm, True)
        want = _oracle(t, hm, True, x).reshape(hm, -1)
        xd = torch.from_numpy(x.reshape(hm, -1)).to(dev)
        yd = torch.zeros(hm, nc, dtype=torch.complex128, device=dev)
        p = fa.plan_many_dft_r2c(3, list(t), hm, xd, None, 1, nr, yd, None, 1, nc, fa.MEASURE)
        text = fa.export_wisdom_to_string()
        assert "t1 s" in text and "r3 16:256:288 16:16:18 16:1:2" in text, text
        xd.copy_(torch.from_numpy(x.reshape(hm, -1)))
        yd.zero_()
        p.execute()
        torch.cuda.synchronize()
        assert aerror(yd.cpu().numpy(), want) <= TOL, p.sprint()
        fa.forget_wisdom()
        assert fa.import_wisdom_from_string(text) == 1
        assert fa.export_wisdom_to_string() == text
        p2 = fa.plan_many_dft_r2c(3, list(t), hm, xd, None, 1, nr, yd, None, 1, nc, fa.ESTIMATE | fa.WISDOM_ONLY)
        assert p2.sprint() == p.sprint(), (p.sprint(), p2.sprint(), text)
        yd.zero_()
        p2.execute()
        torch.cuda.synchronize()
        assert aerror(yd.cpu().numpy(), want) <= TOL
        print("FFTW_MEASURE picked: %s" % p.sprint())
    finally:
        fa.forget_wisdom()
