"""The two-trip planes plan of rank-3 c2c problems on the GPU (planner.c emit_vol_planes), reached through
FFTW_AMD_VOL_PLANES=1: the (n1, n2) planes of the volumes as one image step (img2d, img2dl or img2dw), then the first
axis as one pass in place on the output.

Seven volumes, one for every image family and for full and partial tiles of the planes, run forward out of place and
backward in place, the device arrays inside the NaN-patterned arenas of tests/footprint.py: the plan is the two steps, no
guard violation, the input preserved out of place, a second execution bit-identical, relative L-infinity error at most
1e-10 against the oracle and the rms gate of tests/accuracy.py against the long-double reference.  New-array execution on
arrays 8 bytes off goes through the FFTW_UNALIGNED twin, one batch above the 384 MiB rule runs the nontemporal forms,
and one FFTW_MEASURE plan runs whichever candidate wins and round-trips through wisdom."""
import numpy as np
import pytest

import accuracy as A
import fftw3_amd as fa
from accuracy_cases import knobs
from test_vol_planes_plans import ON, check_planes_plan, vid
from util import TOL, aerror, crand, oracle_dft
from volplanes_gpu import every_condition

A.require_longdouble()
pytestmark = pytest.mark.gpu

# (shape, howmany, family of the plane step); 5 x 64 x 128: five planes are two full tiles and a partial one
SEVEN = [((5, 128, 128), 1, fa.K_IMG2DW), ((5, 64, 128), 1, fa.K_IMG2DW), ((3, 128, 64), 3, fa.K_IMG2DW),
         ((8, 64, 64), 2, fa.K_IMG2DL), ((16, 48, 40), 3, fa.K_IMG2DL), ((6, 32, 32), 3, fa.K_IMG2D),
         ((128, 128, 128), 2, fa.K_IMG2DW)]


@pytest.fixture(scope="module")
def dev():
    import torch
    assert fa.device_count() > 0
    return torch.device("cuda:0")


def _both_forms(dev, case, forms):
    shape, hm, variant = case
    for form in forms:
        sign, inplace = (-1, False) if form == "fwd-oop" else (+1, True)
        every_condition(dev, ON, shape, hm, sign, inplace,
                        lambda p: check_planes_plan(p, shape, hm, variant, fa.FORWARD if sign < 0 else fa.BACKWARD))


@pytest.mark.parametrize("case", SEVEN[:-1], ids=vid)
def test_six_volumes_forward_out_of_place_and_backward_in_place(dev, case):
    _both_forms(dev, case, ("fwd-oop", "bwd-inplace"))


@pytest.mark.parametrize("form", ["fwd-oop", "bwd-inplace"])
def test_one_128_cubed_with_two_volumes(dev, form):
    """a test per form: the long-double reference of 2 x 128^3 points takes seconds, and each direction has its own"""
    assert SEVEN[-1][:2] == ((128, 128, 128), 2)
    _both_forms(dev, SEVEN[-1], (form,))


def test_new_array_execute_8_bytes_off_goes_through_the_twin(dev):
    import torch
    shape, hm, variant = (3, 128, 64), 3, fa.K_IMG2DW
    n = int(np.prod(shape))
    x = crand(np.random.default_rng(312864), hm, n)
    want = oracle_dft(x, shape, hm).reshape(hm, n)
    al = torch.zeros(hm * n * 2 + 8, dtype=torch.float64, device=dev)
    ao = torch.zeros(hm * n * 2 + 8, dtype=torch.float64, device=dev)
    with knobs(ON):
        p = fa.plan_many_dft(3, list(shape), hm, al, None, 1, n, ao, None, 1, n, fa.FORWARD)
    check_planes_plan(p, shape, hm, variant, fa.FORWARD)
    xin, xout = al[1:1 + 2 * hm * n], ao[1:1 + 2 * hm * n]
    assert xin.data_ptr() % 16 == 8 and xout.data_ptr() % 16 == 8
    xin.copy_(torch.from_numpy(x.view(np.float64).reshape(-1)))
    with knobs(ON):
        p.execute_dft(xin, xout)
    torch.cuda.synchronize()
    assert aerror(xout.cpu().numpy().view(np.complex128).reshape(hm, n), want) <= TOL
    # the plan's own arrays still take the two steps
    al[:2 * hm * n].copy_(torch.from_numpy(x.view(np.float64).reshape(-1)))
    ao.zero_()
    p.execute()
    torch.cuda.synchronize()
    check_planes_plan(p, shape, hm, variant, fa.FORWARD)
    assert aerror(ao[:2 * hm * n].cpu().numpy().view(np.complex128).reshape(hm, n), want) <= TOL


def test_large_batch_runs_the_nontemporal_forms(dev):
    """128 x 128 x 128 with 13 volumes: 416 MiB per side, above the 384 MiB rule of FFTW_AMD_NT = 1.  Every volume is the
    same one, so the whole output is compared on the device against that volume's transform."""
    import torch
    shape, hm = (128, 128, 128), 13
    n = int(np.prod(shape))
    x = crand(np.random.default_rng(13), 1, n)
    want = torch.from_numpy(oracle_dft(x, shape, 1).reshape(1, n)).to(dev)
    xd = torch.from_numpy(x).to(dev).repeat(hm, 1)
    yd = torch.zeros_like(xd)
    with knobs(ON):
        p = fa.plan_many_dft(3, list(shape), hm, xd, None, 1, n, yd, None, 1, n, fa.FORWARD)
    check_planes_plan(p, shape, hm, fa.K_IMG2DW, fa.FORWARD)
    a, b = p.steps()
    assert (a.flags & fa.F_NT_IN) and (b.flags & fa.F_NT_OUT), p.sprint()
    p.execute()
    p.sync()
    torch.cuda.synchronize()
    d = yd - want
    err = float(torch.maximum(d.real.abs(), d.imag.abs()).max())
    mag = float(torch.maximum(want.real.abs(), want.imag.abs()).max())
    print("128x128x128 x %d: Linf %.3g" % (hm, err / mag))
    assert err / mag <= TOL
    assert torch.equal(xd, torch.from_numpy(x).to(dev).expand(hm, n))


def test_measure_runs_whichever_candidate_wins_and_wisdom_round_trips(dev):
    import torch
    shape, hm = (8, 64, 64), 4
    n = int(np.prod(shape))
    fa.forget_wisdom()
    try:
        x = crand(np.random.default_rng(86464), hm, n)
        want = oracle_dft(x, shape, hm).reshape(hm, n)
        xd = torch.from_numpy(x).to(dev)
        yd = torch.zeros_like(xd)
        p = fa.plan_many_dft(3, list(shape), hm, xd, None, 1, n, yd, None, 1, n, fa.FORWARD, fa.MEASURE)
        text = fa.export_wisdom_to_string()
        assert "t0 s-1 r3 8:8192:8192 64:128:128 64:2:2" in text, text
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
