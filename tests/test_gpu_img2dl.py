"""The one-trip image kernel for extents above 32 on the GPU (pass2dl.hpp, FFTW_AMD_K_IMG2DL).

Every pair of img2dl_menu.inc runs forward, out of place, on 2T + 3 images (two full tiles and a partial one): relative
L-infinity error at most 1e-10 against the oracle and the rms gate of tests/accuracy.py, the device arrays inside the
NaN-patterned arenas of tests/footprint.py.  Seven pairs -- the largest, non-square ones in both orientations, a
one-stage and a two-stage axis on either side, a radix-5 split -- also run backward, in place, on a single image, twice
(bit-identical), and through the FFTW_UNALIGNED twin on arrays 8 bytes off.  One batch above the 384 MiB rule runs the
nontemporal forms."""
import numpy as np
import pytest

import accuracy as A
import accuracy_cases as AC
import fftw3_amd as fa
import footprint as F
from test_img2dl_plans import MENU, PAIRS, tile
from util import TOL, aerror, crand, oracle_dft

A.require_longdouble()
pytestmark = pytest.mark.gpu

SEVEN = [p for p in PAIRS if p in MENU]


def _label(n0, n1):
    return "pass-%d/img2dl-%dx%d tile=%d" % (n1, n0, n1, tile(n0, n1))


@pytest.fixture(scope="module")
def dev():
    import torch
    assert fa.device_count() > 0
    return torch.device("cuda:0")


@pytest.mark.parametrize("n0,n1", MENU, ids=["%dx%d" % p for p in MENU])
def test_every_menu_pair_forward(n0, n1):
    case = AC.Case("img2dl", "c2c", (n0, n1), 2 * tile(n0, n1) + 3, labels=[_label(n0, n1)])
    x = AC.make_input(case)
    got, sprint, guards = AC.run_gpu(case, x)
    AC.check_labels(case, sprint)
    assert not any(guards.violations), (case.id, guards.violations)
    assert guards.preserved is not False, (case.id, "the input of an out-of-place plan changed")
    e = aerror(got, AC.ref_oracle(case, x))
    m = AC.measure(case, got, x)
    print("%s Linf %.3g gpu %.3f u oracle %.3f u numpy %.3f u" % (case.id, e, m["gpu"] / A.U, m["oracle"] / A.U,
                                                                   m["numpy"] / A.U))
    assert e <= TOL, (case.id, e)
    assert A.passes(m["gpu"], m["oracle"], m["numpy"]), (case.id, m["gpu"] / A.U, m["oracle"] / A.U, m["numpy"] / A.U)
    if "per" in m:
        eg, eo, en = m["per"]
        for b in range(case.hm):
            assert A.passes(eg[b], eo[b], en[b]), (case.id, "entry %d" % b, eg[b] / A.U, eo[b] / A.U, en[b] / A.U)


def _run_in_arenas(dev, n0, n1, hm, sign, inplace):
    """the plan on device arenas, executed twice; returns (result, bit-identical repeat, violations, input kept)"""
    import torch
    case = AC.Case("img2dl", "c2c", (n0, n1), hm, sign)
    x = AC.make_input(case)
    prob = F.Problem("c2c", (n0, n1), hm, F.Layout(), F.Layout(), sign=sign, inplace=inplace)
    AR = prob.arenas()
    prob.scatter(AR, x)
    full = [a.to_device(dev) for a in AR]
    ref = [t.clone() for t in full]
    p = prob.plan(fa, [t[a.lo:] for t, a in zip(full, AR)])
    assert _label(n0, n1) in p.sprint() and len(p.steps()) == 1, p.sprint()
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
@pytest.mark.parametrize("n0,n1", SEVEN, ids=["%dx%d" % p for p in SEVEN])
def test_seven_pairs_every_form(dev, n0, n1, sign, inplace):
    T = tile(n0, n1)
    for hm in (1, 2 * T + 3):
        case, x, got, repeat, viol, kept = _run_in_arenas(dev, n0, n1, hm, sign, inplace)
        assert not any(viol), (case.id, viol)
        assert kept is not False, (case.id, "the input of an out-of-place plan changed")
        assert repeat, (case.id, "the second execution differs from the first")
        e = aerror(got, AC.ref_oracle(case, x))
        m = AC.measure(case, got, x)
        print("%s%s Linf %.3g gpu %.3f u oracle %.3f u numpy %.3f u" % (case.id, " in place" if inplace else "", e,
                                                                          m["gpu"] / A.U, m["oracle"] / A.U, m["numpy"] / A.U))
        assert e <= TOL, (case.id, e)
        assert A.passes(m["gpu"], m["oracle"], m["numpy"]), (case.id, m["gpu"] / A.U, m["oracle"] / A.U, m["numpy"] / A.U)


@pytest.mark.parametrize("n0,n1", SEVEN, ids=["%dx%d" % p for p in SEVEN])
def test_new_array_execute_8_bytes_off_goes_through_the_twin(dev, n0, n1):
    import torch
    hm = 2 * tile(n0, n1) + 3
    n = n0 * n1
    x = crand(np.random.default_rng(n0 * 100 + n1), hm, n)
    want = oracle_dft(x, (n0, n1), hm).reshape(hm, n)
    al = torch.zeros(hm * n * 2 + 8, dtype=torch.float64, device=dev)
    ao = torch.zeros(hm * n * 2 + 8, dtype=torch.float64, device=dev)
    p = fa.plan_many_dft(2, [n0, n1], hm, al, None, 1, n, ao, None, 1, n, fa.FORWARD)
    assert _label(n0, n1) in p.sprint(), p.sprint()
    xin, xout = al[1:1 + 2 * hm * n], ao[1:1 + 2 * hm * n]
    assert xin.data_ptr() % 16 == 8 and xout.data_ptr() % 16 == 8
    xin.copy_(torch.from_numpy(x.view(np.float64).reshape(-1)))
    p.execute_dft(xin, xout)
    torch.cuda.synchronize()
    assert aerror(xout.cpu().numpy().view(np.complex128).reshape(hm, n), want) <= TOL
    # the plan's own arrays still take the one-trip step
    al[:2 * hm * n].copy_(torch.from_numpy(x.view(np.float64).reshape(-1)))
    p.execute()
    torch.cuda.synchronize()
    assert aerror(ao[:2 * hm * n].cpu().numpy().view(np.complex128).reshape(hm, n), want) <= TOL


def test_large_batch_runs_the_nontemporal_forms(dev):
    """64 x 64 with 8192 images: 512 MiB in all, above the 384 MiB rule of FFTW_AMD_NT = 1.  The input repeats a block
    of 256 distinct images, so the whole output is compared against the oracle's transform of that block."""
    import torch
    n0 = n1 = 64
    assert (n0, n1) in MENU
    hm, blk, n = 8192, 256, 4096
    x = crand(np.random.default_rng(64), blk, n)
    want = torch.from_numpy(oracle_dft(x, (n0, n1), blk).reshape(blk, n)).to(dev)
    xd = torch.from_numpy(x).to(dev).repeat(hm // blk, 1)
    yd = torch.zeros_like(xd)
    p = fa.plan_many_dft(2, [n0, n1], hm, xd, None, 1, n, yd, None, 1, n, fa.FORWARD)
    st = p.steps()
    assert len(st) == 1 and st[0].variant == fa.K_IMG2DL, p.sprint()
    assert (st[0].flags & fa.F_NT_IN) and (st[0].flags & fa.F_NT_OUT), p.sprint()
    p.execute()
    p.sync()
    torch.cuda.synchronize()
    y = yd.reshape(hm // blk, blk, n)
    d = y - want[None]
    err = float(torch.maximum(d.real.abs(), d.imag.abs()).max())
    mag = float(torch.maximum(want.real.abs(), want.imag.abs()).max())
    print("64x64 x %d: Linf %.3g" % (hm, err / mag))
    assert err / mag <= TOL
    assert torch.equal(xd[:blk].cpu(), torch.from_numpy(x))
