"""The two forms of the register-resident 1024-point pass (pass1024.hpp): the full-tile kernel
(pass1024_full_kernel: every tile of the launch holds 8 sequences, no re / im swap, no output twiddle, fixed
cache policy, 32-bit element offsets on a scalar base) and the general kernel that takes everything else.  Every case
is compared with the CPU oracle under the reference's error metric and bound (util.aerror, TOL = 1e-10), forward
and backward, and asserts WHICH form ran from the library's launch counters (fa.p1024_launches()).

Backward transforms swap re / im on load and store (FFTW_AMD_F_SWAP_IN / OUT), so every sign = +1 case here is a
"flags request SWAP" case: it must take the general kernel whatever the tile count, and still match.

n = 2^21 = 2048 x 1024 is planned with its 1024-point pass carrying the input twiddle (2048 rows per transform),
so it is a second user of the full-tile form with the input twiddle, with another table (tw = 2^21) and twiddle
positions up to 2047."""
import functools

import numpy as np
import pytest

import fftw3_amd as fa
from util import TOL, aerror, crand, oracle_dft, rrand

pytestmark = pytest.mark.gpu
K_P1024 = 1            # FFTW_AMD_K_P1024


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert fa.device_count() > 0, "no HIP device: the GPU tier cannot run"
    return torch, torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def problem(n, b, sign):
    """(input, oracle's answer) of b transforms of length n; computed once, never written to"""
    x = crand(np.random.default_rng(n + 7 * b), b, n)
    want = oracle_dft(x, (n,), b, sign).reshape(b, n)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def counted(torch, plan):
    """execute once; (full-tile launches, general launches) of the 1024-point pass it made"""
    f0, g0 = fa.p1024_launches()
    plan.execute()
    torch.cuda.synchronize()
    f1, g1 = fa.p1024_launches()
    return f1 - f0, g1 - g0


def n_p1024_steps(plan):
    return sum(1 for s in plan.steps() if s.variant == K_P1024 and s.L == 1024)


@pytest.mark.parametrize("howmany", [1, 5, 8, 9, 16])
@pytest.mark.parametrize("sign", [-1, 1])
def test_rows_of_1024_full_and_partial_tiles(torch_dev, howmany, sign):
    """contiguous rows in, contiguous rows out, one step: 8 and 16 rows are whole tiles, 1 / 5 / 9 are not"""
    torch, dev = torch_dev
    x, want = problem(1024, howmany, sign)
    xd = torch.from_numpy(x.copy()).to(dev)
    yd = torch.zeros_like(xd)
    p = fa.plan_many_dft(1, [1024], howmany, xd, None, 1, 1024, yd, None, 1, 1024, sign)
    assert n_p1024_steps(p) == 1, p.sprint()
    full, general = counted(torch, p)
    e = aerror(yd.cpu().numpy(), want)
    print("rows howmany=%d sign=%+d: error %.3e, full %d, general %d" % (howmany, sign, e, full, general))
    assert e < TOL
    if howmany % 8 == 0 and sign < 0:
        assert (full, general) == (1, 0)
    else:
        assert (full, general) == (0, 1)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("sign", [-1, 1])
def test_two_pass_2_20_both_kernels_of_the_benchmark_plan(torch_dev, inplace, sign):
    """n = 2^20, howmany = 2: the column pass without twiddle and the row pass with the input twiddle, the two
    kernels of the benchmark's plan.  Forward: both on the full-tile form; backward: both general."""
    torch, dev = torch_dev
    n, b = 1 << 20, 2
    x, want = problem(n, b, sign)
    xd = torch.from_numpy(x.copy()).to(dev)
    yd = xd if inplace else torch.zeros_like(xd)
    p = fa.plan_many_dft(1, [n], b, xd, None, 1, n, yd, None, 1, n, sign)
    assert n_p1024_steps(p) == 2 and p.steps()[1].flags & fa.F_TW_IN, p.sprint()
    full, general = counted(torch, p)
    e = aerror(yd.cpu().numpy(), want)
    print("2^20 inplace=%d sign=%+d: error %.3e, full %d, general %d" % (inplace, sign, e, full, general))
    assert e < TOL
    assert (full, general) == ((2, 0) if sign < 0 else (0, 2))


@pytest.mark.parametrize("sign", [-1, 1])
def test_2_21_input_twiddle_with_another_table(torch_dev, sign):
    """n = 2^21, howmany = 3: a 2048-point column pass, then 2048 rows of 1024 per transform with the input twiddle
    of w_(2^21): the full-tile form with twiddle positions up to 2047"""
    torch, dev = torch_dev
    n, b = 1 << 21, 3
    x, want = problem(n, b, sign)
    xd = torch.from_numpy(x.copy()).to(dev)
    yd = torch.zeros_like(xd)
    p = fa.plan_many_dft(1, [n], b, xd, None, 1, n, yd, None, 1, n, sign)
    st = p.steps()
    assert n_p1024_steps(p) == 1 and st[1].L == 1024 and st[1].flags & fa.F_TW_IN and st[1].tw_n == n, p.sprint()
    full, general = counted(torch, p)
    e = aerror(yd.cpu().numpy(), want)
    print("2^21 sign=%+d: error %.3e, full %d, general %d" % (sign, e, full, general))
    assert e < TOL
    assert (full, general) == ((1, 0) if sign < 0 else (0, 1))


def test_split_arrays_keep_off_the_register_pass(torch_dev):
    """n = 2^20 on split re / im arrays: not an interleaved layout, so the plan has no register-pass step at all and
    neither form is launched (the fallback from the full-tile form to the general one is what the sign = +1 cases
    of the other tests cover)"""
    torch, dev = torch_dev
    n = 1 << 20
    rng = np.random.default_rng(11)
    planes = rrand(rng, 2, n)
    pd = torch.from_numpy(planes).to(dev)
    od = torch.zeros_like(pd)
    p = fa.plan_guru64_split_dft([(n, 1, 1)], [], pd[0], pd[1], od[0], od[1])
    assert n_p1024_steps(p) == 0 and [s.L for s in p.steps()] == [1024, 1024], p.sprint()
    full, general = counted(torch, p)
    o = od.cpu().numpy()
    e = aerror(o[0] + 1j * o[1], oracle_dft(planes[0] + 1j * planes[1], (n,), 1))
    print("split 2^20: error %.3e, full %d, general %d" % (e, full, general))
    assert e < TOL
    assert (full, general) == (0, 0)


@pytest.mark.parametrize("shape", [(1024, 12), (12, 1024)])
@pytest.mark.parametrize("sign", [-1, 1])
def test_2d_with_a_partial_last_tile(torch_dev, shape, sign):
    """1024 x 12: twelve columns side by side (one whole tile and half a tile); 12 x 1024: twelve rows"""
    torch, dev = torch_dev
    rng = np.random.default_rng(shape[0])
    x = crand(rng, *shape)
    xd = torch.from_numpy(x.copy()).to(dev)
    yd = torch.zeros_like(xd)
    p = fa.plan_dft_2d(shape[0], shape[1], xd, yd, sign)
    assert n_p1024_steps(p) == 1, p.sprint()
    full, general = counted(torch, p)
    e = aerror(yd.cpu().numpy(), oracle_dft(x, shape, 1, sign).reshape(shape))
    print("2-D %dx%d sign=%+d: error %.3e, full %d, general %d" % (shape[0], shape[1], sign, e, full, general))
    assert e < TOL
    assert (full, general) == (0, 1)


def test_one_lane_pair_launches_keep_the_general_tile(torch_dev, monkeypatch):
    """FFTW_AMD_LANES=1: the pair kernel (pass 2 of chunk c - 1 and pass 1 of chunk c in one launch) is built on the
    general tile; chunks of 1 transform, 3 transforms -> 4 pair launches, none of the full-tile form"""
    torch, dev = torch_dev
    monkeypatch.setenv("FFTW_AMD_LANES", "1")
    n, b = 1 << 20, 3
    x, want = problem(n, b, -1)
    fa.set_chunk_bytes(16 << 20)
    try:
        xd = torch.from_numpy(x.copy()).to(dev)
        yd = torch.zeros_like(xd)
        p = fa.plan_many_dft(1, [n], b, xd, None, 1, n, yd, None, 1, n, fa.FORWARD)
        assert p.chunk == 1 and p.batch == 3
        full, general = counted(torch, p)
        assert p.paired, "the pair launch did not engage"
        e = aerror(yd.cpu().numpy(), want)
        print("pair launches: error %.3e, full %d, general %d" % (e, full, general))
        assert e < TOL
        assert (full, general) == (0, 4)
    finally:
        fa.set_chunk_bytes(0)


def test_rows_full_and_general_forms_agree_bit_for_bit(torch_dev):
    """the same 8 rows of 1024 points as a batch of 8 (full-tile form) and as the first 8 of a batch of 9 (general
    form): the products whose rounding a compiler could choose are written with explicit FMAs in pass1024.hpp, so
    the two forms must give the same bits, not merely the same answer to 1e-10"""
    torch, dev = torch_dev
    x, _ = problem(1024, 9, -1)
    xd = torch.from_numpy(x.copy()).to(dev)
    y9, y8 = torch.zeros_like(xd), torch.zeros_like(xd[:8])
    p9 = fa.plan_many_dft(1, [1024], 9, xd, None, 1, 1024, y9, None, 1, 1024, fa.FORWARD)
    p8 = fa.plan_many_dft(1, [1024], 8, xd, None, 1, 1024, y8, None, 1, 1024, fa.FORWARD)
    assert counted(torch, p9) == (0, 1) and counted(torch, p8) == (1, 0)
    a, b = y9[:8].cpu().numpy(), y8.cpu().numpy()
    print("rows 8 of 9 against 8: max |diff| %.3e" % float(np.abs(a - b).max()))
    assert np.array_equal(a.view(np.float64), b.view(np.float64))


def test_two_pass_full_and_general_forms_agree_bit_for_bit(torch_dev, monkeypatch):
    """n = 2^20, 3 transforms: both kernels of the benchmark's plan on the full-tile form (default lanes) against
    the pair kernel, which is built on the general tile (FFTW_AMD_LANES=1, chunks of one transform): same bits"""
    torch, dev = torch_dev
    n, b = 1 << 20, 3
    x, _ = problem(n, b, -1)
    xd = torch.from_numpy(x.copy()).to(dev)
    yf, yg = torch.zeros_like(xd), torch.zeros_like(xd)
    pf = fa.plan_many_dft(1, [n], b, xd, None, 1, n, yf, None, 1, n, fa.FORWARD)
    assert counted(torch, pf) == (2, 0)
    monkeypatch.setenv("FFTW_AMD_LANES", "1")
    fa.set_chunk_bytes(16 << 20)
    try:
        pg = fa.plan_many_dft(1, [n], b, xd, None, 1, n, yg, None, 1, n, fa.FORWARD)
        assert counted(torch, pg) == (0, 4) and pg.paired
    finally:
        fa.set_chunk_bytes(0)
    a, g = yf.cpu().numpy(), yg.cpu().numpy()
    print("2^20 full against pair (general): max |diff| %.3e" % float(np.abs(a - g).max()))
    assert np.array_equal(a.view(np.float64), g.view(np.float64))
