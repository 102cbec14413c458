"""The two-trip c2r plan on the GPU (emit_c2r_decimated, FFTW_AMD_F_REAL_DEC_C2R, pass3t_kernel RD = 2): a long c2r
transform n = L1 x 2048 as the rows trip over the half spectrum (mirror and conjugation on the load side, the rows
k1 and L1 - k1 of the scratch image stored from one result) plus the backward complex pass of length L1 -- where the
other plans take three trips.  Off under FFTW_ESTIMATE (FFTW_AMD_REAL_DEC=1 here), a FFTW_MEASURE candidate."""
import numpy as np
import pytest

import fftw3_amd as fa
from util import oracle_c2r, aerror, crand, rrand, TOL

pytestmark = pytest.mark.gpu
B = 3


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert fa.device_count() > 0, "no HIP device: the GPU tier cannot run"
    return torch, torch.device("cuda:0")


def _spectra(rng, b, n):
    """half spectra of real rows, so that a round trip has something to return to"""
    xr = rrand(rng, b, n)
    return xr, np.fft.rfft(xr, axis=-1)


# 2048 x 256: the smallest admissible n, 129 rows, the last tile holds the self-mirror row alone; 2048 x 1000: 501
# rows, 5 ordinary rows in the last tile, mixed-radix column pass; 2048 x 1920; 2^21 (1024-point columns); 2^22
@pytest.mark.parametrize("n", [2048 * 256, 2048 * 1000, 2048 * 1920, 1 << 21, 1 << 22])
def test_c2r_in_two_trips(torch_dev, n, monkeypatch):
    torch, dev = torch_dev
    monkeypatch.setenv("FFTW_AMD_REAL_DEC", "1")
    rng = np.random.default_rng(n)
    xr, y = _spectra(rng, B, n)
    y[:, 0] += 0.25j                       # ignored, as by the oracle
    y[:, n // 2] -= 0.5j
    want = oracle_c2r(y, (n,), B).reshape(B, n)
    yd = torch.from_numpy(y).to(dev)
    keep = yd.clone()
    zd = torch.zeros(B, n, dtype=torch.float64, device=dev)
    p = fa.plan_many_dft_c2r(1, [n], B, yd, None, 1, n // 2 + 1, zd, None, 1, n)
    assert len(p.steps()) == 2 and "reg3+c2r-decimated" in p.sprint(), p.sprint()
    p.execute()
    torch.cuda.synchronize()
    e = aerror(zd.cpu().numpy(), want)
    print("n %d out of place %.3g" % (n, e))
    assert e < TOL
    assert torch.equal(torch.view_as_real(yd), torch.view_as_real(keep))      # the input is bit-identical
    # in place: rows of n + 2 reals
    pd = torch.view_as_real(keep.clone()).reshape(B, n + 2)
    q = fa.plan_many_dft_c2r(1, [n], B, pd, None, 1, n // 2 + 1, pd, None, 1, n + 2)
    assert len(q.steps()) == 2 and "reg3+c2r-decimated" in q.sprint(), q.sprint()
    q.execute()
    torch.cuda.synchronize()
    e = aerror(pd[:, :n].cpu().numpy(), want)
    print("n %d in place %.3g" % (n, e))
    assert e < TOL
    # r2c two-trip -> c2r two-trip returns n x
    xd = torch.from_numpy(xr).to(dev)
    sd = torch.zeros(B, n // 2 + 1, dtype=torch.complex128, device=dev)
    f = fa.plan_many_dft_r2c(1, [n], B, xd, None, 1, n, sd, None, 1, n // 2 + 1)
    g = fa.plan_many_dft_c2r(1, [n], B, sd, None, 1, n // 2 + 1, zd, None, 1, n)
    assert "real-decimated" in f.sprint() and "c2r-decimated" in g.sprint()
    zd.zero_()
    f.execute()
    g.execute()
    torch.cuda.synchronize()
    e = aerror(zd.cpu().numpy(), n * xr)
    print("n %d round trip %.3g" % (n, e))
    assert e < TOL
    # the three-trip plan of the same transform agrees to rounding
    monkeypatch.delenv("FFTW_AMD_REAL_DEC")
    z3 = torch.zeros_like(zd)
    y3 = keep.clone()
    p3 = fa.plan_many_dft_c2r(1, [n], B, y3, None, 1, n // 2 + 1, z3, None, 1, n)
    assert "c2r-decimated" not in p3.sprint()
    p3.execute()
    torch.cuda.synchronize()
    assert aerror(z3.cpu().numpy(), want) < TOL


def test_c2r_in_two_trips_as_the_last_axis_of_a_2d_transform(torch_dev, monkeypatch):
    torch, dev = torch_dev
    monkeypatch.setenv("FFTW_AMD_REAL_DEC", "1")
    n0, n1 = 4, 2048 * 256
    rng = np.random.default_rng(5)
    y = np.fft.rfft2(rrand(rng, n0, n1))
    want = oracle_c2r(y, (n0, n1), 1).reshape(n0, n1)
    yd = torch.from_numpy(y).to(dev)
    zd = torch.zeros(n0, n1, dtype=torch.float64, device=dev)
    p = fa.plan_dft_c2r_2d(n0, n1, yd, zd)
    assert "reg3+c2r-decimated" in p.sprint(), p.sprint()
    p.execute()
    torch.cuda.synchronize()
    assert aerror(zd.cpu().numpy(), want) < TOL


def test_measure_mode_times_the_two_trip_c2r_plan_too(torch_dev):
    """for c2r problems FFTW_MEASURE also times the two-trip plan (cfg.real_dec); whichever wins, a wisdom entry exists,
    round-trips, and both plans compute the oracle's answer"""
    torch, dev = torch_dev
    fa.forget_wisdom()
    try:
        n, b = 1 << 20, 24
        rng = np.random.default_rng(22)
        y = crand(rng, b, n // 2 + 1)
        want = oracle_c2r(y, (n,), b).reshape(b, n)
        yd = torch.from_numpy(y).to(dev)
        zd = torch.zeros(b, n, dtype=torch.float64, device=dev)
        p = fa.plan_many_dft_c2r(1, [n], b, yd, None, 1, n // 2 + 1, zd, None, 1, n, fa.MEASURE)
        text = fa.export_wisdom_to_string()
        assert "t2 s" in text and "%d:2:1" % n in text, text
        picked = "c2r-decimated" in p.sprint()
        yd.copy_(torch.from_numpy(y))
        p.execute()
        torch.cuda.synchronize()
        assert aerror(zd.cpu().numpy(), want) < TOL
        fa.forget_wisdom()
        assert fa.import_wisdom_from_string(text) == 1
        yd.copy_(torch.from_numpy(y))
        p2 = fa.plan_many_dft_c2r(1, [n], b, yd, None, 1, n // 2 + 1, zd, None, 1, n, fa.ESTIMATE | fa.WISDOM_ONLY)
        assert ("c2r-decimated" in p2.sprint()) == picked, (p.sprint(), p2.sprint(), text)
        zd.zero_()
        p2.execute()
        torch.cuda.synchronize()
        assert aerror(zd.cpu().numpy(), want) < TOL
    finally:
        fa.forget_wisdom()
