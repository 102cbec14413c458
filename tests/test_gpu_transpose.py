"""GPU tier of the transposition path (transpose.hpp, kernels_tr.hip): the rank-0 guru plans of
tests/transpose_cases.py on the device, at the tile edge (31, 32, 33), one past it, several tiles with a ragged border
in both directions (65, 100 x 100, 257 x 129) and the degenerate shapes (1 x 40, 64 x 3).

The user arrays sit in the NaN arenas of tests/footprint.py ([guard | span | guard], every word that is no input
element a distinct quiet NaN).  A transposition moves data and computes nothing, so the WHOLE arena is compared bit
for bit with the image the definition gives: the output elements, and with them the guards, the leading-dimension
gaps and the input of an out-of-place plan, which must come back unchanged.  Every plan runs twice on re-initialised
arenas; both images must be that one."""
import numpy as np
import pytest

import fftw3_amd as fa
from footprint import Arena
from transpose_cases import GPU_EXTRA, NONSQUARE, SQUARE_N, Case, is_transpose_step

pytestmark = pytest.mark.gpu

SHAPES = NONSQUARE + GPU_EXTRA + tuple((n, n) for n in SQUARE_N)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert fa.device_count() > 0, "no HIP device: the GPU tier cannot run"
    return torch, torch.device("cuda:0")


def _images(case, seed, offset=0):
    """arenas with the input scattered, and the images they must hold after the plan ran (uint64 words)"""
    rng = np.random.default_rng(seed)
    iw, ow = case.in_words(), case.out_words()
    x = rng.random(iw.shape) - 0.5
    if case.inplace:
        arenas = [Arena(max(case.span_in(), case.span_out()), offset=offset)]
    else:
        arenas = [Arena(case.span_in(), offset=offset), Arena(case.span_out(), offset=offset)]
    arenas[0].put(iw.reshape(-1), x.reshape(-1))
    want = [a.snapshot() for a in arenas]
    want[-1].view(np.float64)[arenas[-1].lo + ow.reshape(-1)] = x.reshape(-1)
    return arenas, want


def _device(torch_dev, arenas):
    torch, dev = torch_dev
    full = [a.to_device(dev) for a in arenas]
    return full, [t[a.lo:] for t, a in zip(full, arenas)]


def _same(full, want):
    return all(np.array_equal(t.cpu().numpy().view(np.uint64), w) for t, w in zip(full, want))


def _run(torch_dev, case, seed, expect_steps=None):
    torch, _ = torch_dev
    arenas, want = _images(case, seed)
    full, user = _device(torch_dev, arenas)
    p = case.plan(user[0], user[-1])
    if expect_steps is not None:
        expect_steps(p)
    p.execute()
    torch.cuda.synchronize()
    assert _same(full, want), (case, p.sprint())
    for t, a in zip(full, arenas):                       # the arenas re-initialised, the same plan again
        t.copy_(torch.from_numpy(a.f64))
    p.execute()
    torch.cuda.synchronize()
    assert _same(full, want), (case, "second execution", p.sprint())
    return p


def _one_tiled_step(p):
    st = p.steps()
    assert len(st) == 1 and is_transpose_step(st[0]), p.sprint()


@pytest.mark.parametrize("kind", ["r2r", "c2c"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_out_of_place(torch_dev, kind, shape):
    n0, n1 = shape
    for k, (pad, batch, vl) in enumerate(((0, 1, 1), (3, 3, 3), (3, 3, 1), (0, 1, 3))):
        _run(torch_dev, Case(kind, n0, n1, n1 + pad, n0 + pad, batch, vl), 100 * n0 + n1 + k, _one_tiled_step)


@pytest.mark.parametrize("kind", ["r2r", "c2c"])
@pytest.mark.parametrize("n", SQUARE_N + (100,))
def test_in_place_square(torch_dev, kind, n):
    def check(p):
        _one_tiled_step(p)
        assert p.steps()[0].flags & fa.F_PAIR_SWAP and p.workspace_bytes == 0

    for k, (pad, batch, vl) in enumerate(((0, 1, 1), (3, 1, 1), (0, 3, 1), (3, 3, 1), (3, 3, 3))):
        _run(torch_dev, Case(kind, n, n, n + pad, n + pad, batch, vl, inplace=True), 7 * n + k, check)


@pytest.mark.parametrize("kind", ["r2r", "c2c"])
@pytest.mark.parametrize("shape", NONSQUARE + ((257, 129),), ids=lambda s: "%dx%d" % s)
def test_in_place_nonsquare_through_scratch(torch_dev, kind, shape):
    n0, n1 = shape
    for k, (batch, vl) in enumerate(((1, 1), (3, 1), (3, 3))):
        p = _run(torch_dev, Case(kind, n0, n1, batch=batch, vl=vl, inplace=True), 31 * n0 + n1 + k)
        assert p.batch == p.chunk


@pytest.mark.parametrize("kind", ["r2r", "c2c"])
def test_new_array_execution_on_a_second_in_place_buffer(torch_dev, kind):
    """execute_r2r / execute_dft on another array; for reals one that is 8 bytes off 16-byte alignment (reals are only
    guaranteed 8-byte alignment: the launcher then moves 8-byte elements)"""
    torch, _ = torch_dev
    for n, pad, batch, vl in ((33, 0, 1, 1), (100, 3, 3, 1), (65, 3, 3, 2), (32, 0, 2, 3)):
        case = Case(kind, n, n, n + pad, n + pad, batch, vl, inplace=True)
        arenas, _ = _images(case, n)
        _, user = _device(torch_dev, arenas)
        p = case.plan(user[0], user[0])
        arenas2, want2 = _images(case, n + 1, offset=1 if kind == "r2r" else 0)
        full2, user2 = _device(torch_dev, arenas2)
        assert user2[0].data_ptr() % 16 == (8 if kind == "r2r" else 0)
        if kind == "r2r":
            p.execute_r2r(user2[0], user2[0])
        else:
            p.execute_dft(user2[0], user2[0])
        torch.cuda.synchronize()
        assert _same(full2, want2), (case, p.sprint())
    # out of place on two other arrays, the real ones off alignment
    case = Case(kind, 257, 129, 129 + 3, 257 + 3, 2, 1)
    arenas, _ = _images(case, 5)
    _, user = _device(torch_dev, arenas)
    p = case.plan(user[0], user[1])
    arenas2, want2 = _images(case, 6, offset=1 if kind == "r2r" else 0)
    full2, user2 = _device(torch_dev, arenas2)
    if kind == "r2r":
        p.execute_r2r(user2[0], user2[1])
    else:
        p.execute_dft(user2[0], user2[1])
    torch.cuda.synchronize()
    assert _same(full2, want2), (case, p.sprint())


def test_in_place_nonsquare_real_transpose_is_exact(torch_dev):
    """1200 x 2000 reals in place (the shape of the complex case of test_gpu_parity): the parent planned ONE
    element-wise copy of the array onto itself -- thousands of workgroups reading and writing the same words in a
    permuted order.  (That plan usually, not certainly, gives a wrong result; the deterministic checks of the rule
    are in tests/test_transpose_plans.py.)"""
    torch, dev = torch_dev
    n0, n1 = 1200, 2000
    x = np.random.default_rng(172).random(n0 * n1) - 0.5
    xd = torch.from_numpy(x).to(dev)
    p = fa.plan_guru64_r2r([], [(n0, n1, 1), (n1, 1, n0)], xd, xd, [])
    assert p.batch == p.chunk and p.steps()[0].dst_buf >= 2
    p.execute()
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy().reshape(n1, n0), x.reshape(n0, n1).T)
