"""The one-trip small-volume kernel on the GPU (pass3d.hpp, FFTW_AMD_K_VOL3D), reached through FFTW_AMD_VOL3D=1.

Every triple of vol3d_menu.inc runs forward, out of place, on 2T + 3 volumes (two full tiles and a partial one), the
device arrays inside the NaN-patterned arenas of tests/footprint.py: no guard violation, the input preserved bit for
bit, relative L-infinity error at most 1e-10 against the oracle and the rms gate of tests/accuracy.py against the
long-double reference.  The ten triples of the CPU tier also run backward, in place, on a single volume, twice
(bit-identical), and through the FFTW_UNALIGNED twin on arrays 8 bytes off.  One batch above the 384 MiB rule runs the
nontemporal forms, and one FFTW_MEASURE plan runs whichever candidate wins and round-trips through wisdom."""
import numpy as np
import pytest

import accuracy as A
import accuracy_cases as AC
import fftw3_amd as fa
import footprint as F
from accuracy_cases import knobs
from test_vol3d_plans import IDS, MENU, ON, TEN, TEN_IDS, label, tile
from util import TOL, aerror, crand, oracle_dft

A.require_longdouble()
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert fa.device_count() > 0
    return torch.device("cuda:0")


def _gates(case, x, got, what=""):
    e = aerror(got, AC.ref_oracle(case, x))
    m = AC.measure(case, got, x)
    print("%s%s Linf %.3g gpu %.3f u oracle %.3f u numpy %.3f u" % (case.id, what, e, m["gpu"] / A.U, m["oracle"] / A.U,
                                                                     m["numpy"] / A.U))
    assert e <= TOL, (case.id, what, e)
    assert A.passes(m["gpu"], m["oracle"], m["numpy"]), (case.id, what, m["gpu"] / A.U, m["oracle"] / A.U, m["numpy"] / A.U)
    if "per" in m:
        eg, eo, en = m["per"]
        for b in range(case.hm):
            assert A.passes(eg[b], eo[b], en[b]), (case.id, "entry %d" % b, eg[b] / A.U, eo[b] / A.U, en[b] / A.U)


@pytest.mark.parametrize("shape", MENU, ids=IDS)
def test_every_menu_triple_forward(shape):
    T = tile(*shape)
    case = AC.Case("vol3d", "c2c", shape, 2 * T + 3, labels=[label(*shape)], env=ON)
    x = AC.make_input(case)
    got, sprint, guards = AC.run_gpu(case, x)
    AC.check_labels(case, sprint)
    assert not any(guards.violations), (case.id, guards.violations)
    assert guards.preserved is True, (case.id, "the input of an out-of-place plan changed")
    _gates(case, x, got)


def _run_in_arenas(dev, shape, hm, sign, inplace):
    """the plan on device arenas, executed twice; returns (case, input, result, bit-identical repeat, violations, input
    kept)"""
    import torch
    case = AC.Case("vol3d", "c2c", shape, hm, sign, env=ON)
    x = AC.make_input(case)
    prob = F.Problem("c2c", shape, hm, F.Layout(), F.Layout(), sign=sign, inplace=inplace)
    AR = prob.arenas()
    prob.scatter(AR, x)
    full = [a.to_device(dev) for a in AR]
    ref = [t.clone() for t in full]
    with knobs(ON):
        p = prob.plan(fa, [t[a.lo:] for t, a in zip(full, AR)])
    assert label(*shape) in p.sprint() and len(p.steps()) == 1, p.sprint()
    p.execute()
    p.sync()
    torch.cuda.synchronize()
    first = [t.clone() for t in full]
    viol = [F.check(r, t, w) for r, t, w in zip(ref, full, prob.written(AR))]
    kept = None if inplace else F.same_bits(full[0], ref[0])
    for t, r in zip(full, ref):
        t.copy_(r)
    p.execute()
    p.sync()
    torch.cuda.synchronize()
    repeat = all(F.same_bits(t, f) for t, f in zip(full, first))
    out = first[-1][AR[-1].lo:AR[-1].lo + AR[-1].span].cpu().numpy()
    return case, x, prob.gather([out]).reshape(x.shape), repeat, viol, kept


@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "inplace"])
@pytest.mark.parametrize("sign", [-1, +1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("shape", TEN, ids=TEN_IDS)
def test_ten_triples_every_form(dev, shape, sign, inplace):
    T = tile(*shape)
    for hm in (1, 2 * T + 3):
        case, x, got, repeat, viol, kept = _run_in_arenas(dev, shape, hm, sign, inplace)
        assert not any(viol), (case.id, viol)
        assert kept is not False, (case.id, "the input of an out-of-place plan changed")
        assert repeat, (case.id, "the second execution differs from the first")
        _gates(case, x, got, " in place" if inplace else "")


@pytest.mark.parametrize("shape", TEN, ids=TEN_IDS)
def test_new_array_execute_8_bytes_off_goes_through_the_twin(dev, shape):
    import torch
    hm = 2 * tile(*shape) + 3
    n = int(np.prod(shape))
    x = crand(np.random.default_rng(10000 * shape[0] + 100 * shape[1] + shape[2]), hm, n)
    want = oracle_dft(x, shape, hm).reshape(hm, n)
    al = torch.zeros(hm * n * 2 + 8, dtype=torch.float64, device=dev)
    ao = torch.zeros(hm * n * 2 + 8, dtype=torch.float64, device=dev)
    with knobs(ON):
        p = fa.plan_many_dft(3, list(shape), hm, al, None, 1, n, ao, None, 1, n, fa.FORWARD)
    assert label(*shape) in p.sprint(), p.sprint()
    xin, xout = al[1:1 + 2 * hm * n], ao[1:1 + 2 * hm * n]
    assert xin.data_ptr() % 16 == 8 and xout.data_ptr() % 16 == 8
    xin.copy_(torch.from_numpy(x.view(np.float64).reshape(-1)))
    with knobs(ON):
        p.execute_dft(xin, xout)
    torch.cuda.synchronize()
    assert aerror(xout.cpu().numpy().view(np.complex128).reshape(hm, n), want) <= TOL
    # the plan's own arrays still take the one-trip step
    al[:2 * hm * n].copy_(torch.from_numpy(x.view(np.float64).reshape(-1)))
    ao.zero_()
    p.execute()
    torch.cuda.synchronize()
    assert label(*shape) in p.sprint(), p.sprint()
    assert aerror(ao[:2 * hm * n].cpu().numpy().view(np.complex128).reshape(hm, n), want) <= TOL


def test_large_batch_runs_the_nontemporal_forms(dev):
    """16 x 16 x 16 with 8192 volumes: 512 MiB per side, above the 384 MiB rule of FFTW_AMD_NT = 1.  The input repeats
    a block of 512 distinct volumes, so the whole output is compared on the device against that block's transform."""
    import torch
    shape = (16, 16, 16)
    assert shape in MENU
    hm, blk, n = 8192, 512, 4096
    x = crand(np.random.default_rng(16), blk, n)
    want = torch.from_numpy(oracle_dft(x, shape, blk).reshape(blk, n)).to(dev)
    xd = torch.from_numpy(x).to(dev).repeat(hm // blk, 1)
    yd = torch.zeros_like(xd)
    with knobs(ON):
        p = fa.plan_many_dft(3, list(shape), hm, xd, None, 1, n, yd, None, 1, n, fa.FORWARD)
    st = p.steps()
    assert len(st) == 1 and st[0].variant == fa.K_VOL3D, p.sprint()
    assert (st[0].flags & fa.F_NT_IN) and (st[0].flags & fa.F_NT_OUT), p.sprint()
    p.execute()
    p.sync()
    torch.cuda.synchronize()
    d = yd.reshape(hm // blk, blk, n) - want[None]
    err = float(torch.maximum(d.real.abs(), d.imag.abs()).max())
    mag = float(torch.maximum(want.real.abs(), want.imag.abs()).max())
    print("16x16x16 x %d: Linf %.3g" % (hm, err / mag))
    assert err / mag <= TOL
    assert torch.equal(xd.reshape(hm // blk, blk, n), torch.from_numpy(x).to(dev)[None].expand(hm // blk, blk, n))


def test_measure_times_the_one_trip_plan_and_wisdom_round_trips(dev):
    import torch
    shape = (16, 16, 16)
    hm, n = 4096, 4096
    fa.forget_wisdom()
    try:
        x = crand(np.random.default_rng(17), hm, n)
        want = oracle_dft(x, shape, hm).reshape(hm, n)
        xd = torch.from_numpy(x).to(dev)
        yd = torch.zeros_like(xd)
        p = fa.plan_many_dft(3, list(shape), hm, xd, None, 1, n, yd, None, 1, n, fa.FORWARD, fa.MEASURE)
        text = fa.export_wisdom_to_string()
        assert "t0 s-1 r3 16:512:512 16:32:32 16:2:2" in text, text
        xd.copy_(torch.from_numpy(x))
        yd.zero_()
        p.execute()
        torch.cuda.synchronize()
        assert aerror(yd.cpu().numpy(), want) <= TOL, p.sprint()
        fa.forget_wisdom()
        assert fa.import_wisdom_from_string(text) == 1
        assert fa.export_wisdom_to_string() == text
        p2 = fa.plan_many_dft(3, list(shape), hm, xd, None, 1, n, yd, None, 1, n, fa.FORWARD, fa.ESTIMATE | fa.WISDOM_ONLY)
        assert p2.sprint() == p.sprint(), (p.sprint(), p2.sprint(), text)
        yd.zero_()
        p2.execute()
        torch.cuda.synchronize()
        assert aerror(yd.cpu().numpy(), want) <= TOL
        print("FFTW_MEASURE picked: %s" % p.sprint())
    finally:
        fa.forget_wisdom()
