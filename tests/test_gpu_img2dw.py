"""The one-trip image kernel for an extent of 128 on the GPU (pass2dw.hpp, FFTW_AMD_K_IMG2DW), reached through
FFTW_AMD_IMG_WIDE=1.

Each of 128 x 128, 64 x 128 and 128 x 64 runs forward, out of place, on 2T + 1 images (two full tiles and, where T = 2, a
partial one), and backward, in place, on a single image, the device arrays inside the NaN-patterned arenas of
tests/footprint.py: the label is in the plan, no guard violation, the input preserved out of place, a second execution
bit-identical, relative L-infinity error at most 1e-10 against the oracle and the rms gate of tests/accuracy.py against
the long-double reference.  New-array execution on arrays 8 bytes off goes through the FFTW_UNALIGNED twin, and one
FFTW_MEASURE plan runs whichever candidate wins and round-trips through wisdom."""
import numpy as np
import pytest

import accuracy as A
import fftw3_amd as fa
from accuracy_cases import knobs
from test_vol_planes_plans import WIDE, WIDE_ON, wide_label
from util import TOL, aerror, crand, oracle_dft
from volplanes_gpu import every_condition

A.require_longdouble()
pytestmark = pytest.mark.gpu
IDS = ["%dx%d" % p for p in WIDE]


@pytest.fixture(scope="module")
def dev():
    import torch
    assert fa.device_count() > 0
    return torch.device("cuda:0")


def _is_the_wide_step(n0, n1):
    def check(p):
        assert wide_label(n0, n1) in p.sprint() and len(p.steps()) == 1, p.sprint()
    return check


@pytest.mark.parametrize("n0,n1", WIDE, ids=IDS)
def test_tiles_forward_and_a_single_image_backward_in_place(dev, n0, n1):
    """2T + 1 images forward out of place (two full tiles and, where T = 2, a partial one), then one image backward in
    place; every condition of the module's docstring holds for both"""
    T = fa.img2dw_tile(n0, n1)
    every_condition(dev, WIDE_ON, (n0, n1), 2 * T + 1, -1, False, _is_the_wide_step(n0, n1))
    every_condition(dev, WIDE_ON, (n0, n1), 1, +1, True, _is_the_wide_step(n0, n1))


def test_new_array_execute_8_bytes_off_goes_through_the_twin(dev):
    for n0, n1 in WIDE:
        _twin(dev, n0, n1)


def _twin(dev, n0, n1):
    import torch
    hm = 2 * fa.img2dw_tile(n0, n1) + 1
    n = n0 * n1
    x = crand(np.random.default_rng(n0 * 1000 + n1), hm, n)
    want = oracle_dft(x, (n0, n1), hm).reshape(hm, n)
    al = torch.zeros(hm * n * 2 + 8, dtype=torch.float64, device=dev)
    ao = torch.zeros(hm * n * 2 + 8, dtype=torch.float64, device=dev)
    with knobs(WIDE_ON):
        p = fa.plan_many_dft(2, [n0, n1], hm, al, None, 1, n, ao, None, 1, n, fa.FORWARD)
    assert wide_label(n0, n1) in p.sprint(), p.sprint()
    xin, xout = al[1:1 + 2 * hm * n], ao[1:1 + 2 * hm * n]
    assert xin.data_ptr() % 16 == 8 and xout.data_ptr() % 16 == 8
    xin.copy_(torch.from_numpy(x.view(np.float64).reshape(-1)))
    with knobs(WIDE_ON):
        p.execute_dft(xin, xout)
    torch.cuda.synchronize()
    assert aerror(xout.cpu().numpy().view(np.complex128).reshape(hm, n), want) <= TOL
    # the plan's own arrays still take the one-trip step
    al[:2 * hm * n].copy_(torch.from_numpy(x.view(np.float64).reshape(-1)))
    ao.zero_()
    p.execute()
    torch.cuda.synchronize()
    assert wide_label(n0, n1) in p.sprint(), p.sprint()
    assert aerror(ao[:2 * hm * n].cpu().numpy().view(np.complex128).reshape(hm, n), want) <= TOL


def test_measure_runs_whichever_candidate_wins_and_wisdom_round_trips(dev):
    import torch
    shape, hm, n = (128, 128), 5, 128 * 128
    fa.forget_wisdom()
    try:
        x = crand(np.random.default_rng(128), hm, n)
        want = oracle_dft(x, shape, hm).reshape(hm, n)
        xd = torch.from_numpy(x).to(dev)
        yd = torch.zeros_like(xd)
        p = fa.plan_many_dft(2, list(shape), hm, xd, None, 1, n, yd, None, 1, n, fa.FORWARD, fa.MEASURE)
        text = fa.export_wisdom_to_string()
        assert "t0 s-1 r2 128:256:256 128:2:2" in text, text
        xd.copy_(torch.from_numpy(x))
        yd.zero_()
        p.execute()
        torch.cuda.synchronize()
        assert aerror(yd.cpu().numpy(), want) <= TOL, p.sprint()
        fa.forget_wisdom()
        assert fa.import_wisdom_from_string(text) == 1
        assert fa.export_wisdom_to_string() == text
        p2 = fa.plan_many_dft(2, list(shape), hm, xd, None, 1, n, yd, None, 1, n, fa.FORWARD, fa.ESTIMATE | fa.WISDOM_ONLY)
        assert p2.sprint() == p.sprint(), (p.sprint(), p2.sprint(), text)
        yd.zero_()
        p2.execute()
        torch.cuda.synchronize()
        assert aerror(yd.cpu().numpy(), want) <= TOL
        print("FFTW_MEASURE picked: %s" % p.sprint())
    finally:
        fa.forget_wisdom()
