"""CPU tier of the one-trip image plans for extents above 32 (planner.c emit_img2dl, FFTW_AMD_K_IMG2DL, pass2dl.hpp):
batches of dense contiguous 2-D transforms n0 x n1 with both extents in {16, 32, 40, 48, 64} and at least one above 32
plan as ONE step that is the 2-D DFT of every tile, and the numpy step interpreter (which already knows
FFTW_AMD_F_LO_DFT) computes what the oracle computes.  Every layout the rule excludes keeps a plan without that step and
still matches.  The pairs cover non-square shapes in both orientations, a one-stage and a two-stage axis on either side
and a radix-5 split."""
import os
import re

import numpy as np
import pytest

import fftw3_amd as fa
from accuracy_cases import knobs
from step_interp import Interp, run_plan_on_host, scratch_reals
from util import ROOT, TOL, aerror, crand, oracle_dft, rrand

PAIRS = [(64, 64), (40, 40), (48, 64), (64, 48), (64, 32), (32, 64), (16, 40)]
EXTENTS = (16, 32, 40, 48, 64)
MUST_STAY = [(64, 64)]


def menu():
    """the (n0, n1) pairs of img2dl_menu.inc (an entry whose kernel spilled, or whose plan measured no faster than the
    two-trip plan, was dropped from it)"""
    with open(os.path.join(ROOT, "fftw3_amd", "csrc", "img2dl_menu.inc")) as f:
        return [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"X\((\d+), (\d+)\)", f.read())]


MENU = menu()


def tile(n0, n1):
    return fa.img2dl_tile(n0, n1)


def _cases():
    out = []
    for n0, n1 in PAIRS:
        for which in ("one", "T", "2T+3"):
            out.append((n0, n1, which))
    return out


def _howmany(n0, n1, which):
    T = tile(n0, n1)
    return {"one": 1, "T": T, "2T+3": 2 * T + 3}[which]


def _skip_dropped(n0, n1):
    if (n0, n1) not in MENU:
        pytest.skip("%d x %d was dropped from img2dl_menu.inc" % (n0, n1))


_INPUT = {}


def _input(n0, n1, hm):
    """the same input and oracle results for every test of one case"""
    key = (n0, n1, hm)
    if key not in _INPUT:
        rng = np.random.default_rng(1000 * n0 + n1)
        x = crand(rng, hm * n0 * n1)
        _INPUT[key] = (x, {s: oracle_dft(x, (n0, n1), hm, s) for s in (-1, +1)})
        for v in _INPUT[key][1].values():
            v.setflags(write=False)
        x.setflags(write=False)
    return _INPUT[key]


def _table_bytes(n0, n1):
    """the stage tables of the two-stage axes, all a plan with the step owns: no scratch buffer"""
    return 16 * sum(set(n for n in (n0, n1) if n > 32))


def _has_img2dl(p):
    return any(s.variant == fa.K_IMG2DL for s in p.steps())


def test_menu_and_tile_query_agree():
    want = [(a, b) for a in EXTENTS for b in EXTENTS if a > 32 or b > 32]
    assert len(want) == 21
    assert set(MENU) <= set(want) and len(set(MENU)) == len(MENU)
    assert set(MUST_STAY) <= set(MENU), sorted(set(MUST_STAY) - set(MENU))
    for n0 in range(0, 67):
        for n1 in range(0, 67):
            T = tile(n0, n1)
            if (n0 <= 32 and n1 <= 32) or n0 in (33, 63, 65) or n1 in (33, 63, 65):
                assert T == 0, (n0, n1, T)
            if (n0, n1) in MENU:
                assert T >= 1 and T * n0 * n1 <= 8192, (n0, n1, T)
            else:
                assert T == 0, (n0, n1, T)


@pytest.mark.parametrize("n0,n1,which", _cases())
def test_one_step_with_the_documented_fields(n0, n1, which):
    _skip_dropped(n0, n1)
    hm = _howmany(n0, n1, which)
    x, _ = _input(n0, n1, hm)
    y = np.zeros_like(x)
    for sign in (fa.FORWARD, fa.BACKWARD):
        p = fa.plan_many_dft(2, [n0, n1], hm, x, None, 1, n0 * n1, y, None, 1, n0 * n1, sign)
        st = p.steps()
        assert len(st) == 1, p.sprint()
        s = st[0]
        assert s.kind == fa.STEP_PASS and s.variant == fa.K_IMG2DL, p.sprint()
        assert s.flags & fa.F_LO_DFT
        swaps = s.flags & (fa.F_SWAP_IN | fa.F_SWAP_OUT)
        assert swaps == ((fa.F_SWAP_IN | fa.F_SWAP_OUT) if sign == fa.BACKWARD else 0)
        assert (s.L, s.is_l, s.os_l) == (n1, 2, 2)
        assert (s.tile_lo_n, s.tile_lo_is, s.tile_lo_os) == (n0, 2 * n1, 2 * n1)
        assert s.ndims == 1 and (s.dim_n[0], s.dim_is[0], s.dim_os[0]) == (hm, 2 * n0 * n1, 2 * n0 * n1)
        assert s.tile == tile(n0, n1)
        assert s.tw_n == 0 and s.src_im == 1 and s.dst_im == 1
        # the intra-axis twiddles of a two-stage axis: stage tables in slots that no pass without tw_n reads
        assert (s.table >= 0) == (n1 > 32) and (s.table2 >= 0) == (n0 > 32)
        assert s.nradices >= 1 and int(np.prod([s.radices[i] for i in range(s.nradices)])) == n1
        assert (s.src_buf, s.dst_buf) == (0, 1)
        # no scratch: the plan owns nothing but those tables (n entries of 16 bytes, one table for equal extents)
        assert p.workspace_bytes == _table_bytes(n0, n1)
        assert p.batch == p.chunk == hm
        assert "pass-%d/img2dl-%dx%d tile=%d" % (n1, n0, n1, s.tile) in p.sprint(), p.sprint()


@pytest.mark.parametrize("n0,n1,which", _cases())
def test_interpreter_matches_the_oracle(n0, n1, which):
    _skip_dropped(n0, n1)
    hm = _howmany(n0, n1, which)
    x, want = _input(n0, n1, hm)
    for sign in (fa.FORWARD, fa.BACKWARD):
        y = np.zeros_like(x)
        p = fa.plan_many_dft(2, [n0, n1], hm, x, None, 1, n0 * n1, y, None, 1, n0 * n1, sign)
        assert _has_img2dl(p)
        run_plan_on_host(p, x, y)
        assert aerror(y, want[sign]) < TOL, (n0, n1, hm, sign)
        z = x.copy()                                   # in place
        p = fa.plan_many_dft(2, [n0, n1], hm, z, None, 1, n0 * n1, z, None, 1, n0 * n1, sign)
        assert _has_img2dl(p) and len(p.steps()) == 1 and p.workspace_bytes == _table_bytes(n0, n1)
        run_plan_on_host(p, z, z)
        assert aerror(z, want[sign]) < TOL, (n0, n1, hm, sign, "in place")


def _misaligned(words):
    w = rrand(np.random.default_rng(5), words + 2)
    w = w[1:] if w.ctypes.data % 16 == 0 else w[:-1]
    assert w.ctypes.data % 16 == 8
    return w[:words]


@pytest.mark.parametrize("n0,n1,which", _cases())
def test_excluded_layouts_keep_a_plan_without_the_step(n0, n1, which):
    _skip_dropped(n0, n1)
    hm = _howmany(n0, n1, which)
    x, want = _input(n0, n1, hm)
    n = n0 * n1
    w = want[-1].reshape(hm, n0, n1)
    # the knob restores the two-trip plan
    with knobs({"FFTW_AMD_NO_IMG2D": "1"}):
        y = np.zeros_like(x)
        p = fa.plan_many_dft(2, [n0, n1], hm, x, None, 1, n, y, None, 1, n, fa.FORWARD)
        assert not _has_img2dl(p) and "img2dl" not in p.sprint()
        run_plan_on_host(p, x, y)
        assert aerror(y, w) < TOL
    with knobs({"FFTW_AMD_NO_TUNED": "1"}):
        y = np.zeros_like(x)
        p = fa.plan_many_dft(2, [n0, n1], hm, x, None, 1, n, y, None, 1, n, fa.FORWARD)
        assert not _has_img2dl(p) and "img2dl" not in p.sprint()
        run_plan_on_host(p, x, y)
        assert aerror(y, w) < TOL
    # FFTW_UNALIGNED, on arrays 8 bytes off
    xu = _misaligned(2 * hm * n)
    yu = np.zeros(hm * n, dtype=np.complex128)
    p = fa.plan_many_dft(2, [n0, n1], hm, xu, None, 1, n, yu, None, 1, n, fa.FORWARD, fa.ESTIMATE | fa.UNALIGNED)
    assert not _has_img2dl(p), p.sprint()
    run_plan_on_host(p, xu, yu)
    assert aerror(yu, oracle_dft(xu.view(np.complex128), (n0, n1), hm)) < TOL
    # a gapped dist (with one image there is no loop, so no dist: FFTW's extent-1 loops carry nothing, and the
    # single dense image keeps the step)
    dist = n + 3
    xg = np.zeros(hm * dist, dtype=np.complex128)
    xg.reshape(hm, dist)[:, :n] = x.reshape(hm, n)
    yg = np.zeros_like(xg)
    p = fa.plan_many_dft(2, [n0, n1], hm, xg, None, 1, dist, yg, None, 1, dist, fa.FORWARD)
    assert _has_img2dl(p) == (hm == 1), p.sprint()
    run_plan_on_host(p, xg, yg)
    assert aerror(yg.reshape(hm, dist)[:, :n], w) < TOL
    if hm > 1:
        # ... on one side only
        yd = np.zeros_like(x)
        p = fa.plan_many_dft(2, [n0, n1], hm, xg, None, 1, dist, yd, None, 1, n, fa.FORWARD)
        assert not _has_img2dl(p), p.sprint()
        run_plan_on_host(p, xg, yd)
        assert aerror(yd, w) < TOL
    # inembed with a pitch
    pitch = n1 + 2
    xp = np.zeros(hm * n0 * pitch, dtype=np.complex128)
    xp.reshape(hm, n0, pitch)[:, :, :n1] = x.reshape(hm, n0, n1)
    yp = np.zeros_like(x)
    p = fa.plan_many_dft(2, [n0, n1], hm, xp, [n0, pitch], 1, n0 * pitch, yp, None, 1, n, fa.FORWARD)
    assert not _has_img2dl(p), p.sprint()
    run_plan_on_host(p, xp, yp)
    assert aerror(yp, w) < TOL
    # split arrays through the guru interface (one allocation: the interpreter addresses the imaginary plane
    # from the real one)
    N = hm * n
    s = np.zeros(4 * N)
    s[0:N], s[N:2 * N] = x.real, x.imag
    p = fa.plan_guru64_split_dft([(n0, n1, n1), (n1, 1, 1)], [(hm, n, n)], s[0:N], s[N:2 * N], s[2 * N:3 * N], s[3 * N:],
                                 fa.ESTIMATE)
    assert not _has_img2dl(p), p.sprint()

    class _At(object):
        def __init__(self, a, base):
            self.a, self.base = a, base

        def __getitem__(self, i):
            return self.a[np.asarray(i) + self.base]

        def __setitem__(self, i, v):
            self.a[np.asarray(i) + self.base] = v

    Interp(p).run(s, _At(s, 2 * N), scratch_reals(p))
    assert aerror(s[2 * N:3 * N] + 1j * s[3 * N:], w) < TOL
    # the same dense images through the guru interface do get the step
    y = np.zeros_like(x)
    p = fa.plan_guru64_dft([(n0, n1, n1), (n1, 1, 1)], [(hm, n, n)], x, y, fa.FORWARD)
    assert _has_img2dl(p), p.sprint()


@pytest.mark.parametrize("n0,n1", PAIRS)
def test_two_howmany_loops_keep_a_plan_without_the_step(n0, n1):
    """2 T images as one loop of 2 T get the step, as two loops (T, 2) they do not: every pair, 64 x 64 and the radix-5
    pair included"""
    _skip_dropped(n0, n1)
    T = tile(n0, n1)
    hm, n = 2 * T, n0 * n1
    x, want = _input(n0, n1, hm)
    y = np.zeros_like(x)
    p = fa.plan_guru64_dft([(n0, n1, n1), (n1, 1, 1)], [(hm, n, n)], x, y, fa.FORWARD)
    assert _has_img2dl(p), p.sprint()
    p = fa.plan_guru64_dft([(n0, n1, n1), (n1, 1, 1)], [(T, 2 * n, 2 * n), (2, n, n)], x, y, fa.FORWARD)
    assert not _has_img2dl(p), p.sprint()
    run_plan_on_host(p, x, y)
    assert aerror(y, want[-1]) < TOL


@pytest.mark.parametrize("shape", [(2, 64, 64), (3, 16, 40)])
def test_rank_3_is_outside_the_rule(shape):
    rng = np.random.default_rng(9)
    n = int(np.prod(shape))
    hm = 3
    x = crand(rng, hm * n)
    y = np.zeros_like(x)
    p = fa.plan_many_dft(3, list(shape), hm, x, None, 1, n, y, None, 1, n, fa.FORWARD)
    assert not _has_img2dl(p), p.sprint()
    run_plan_on_host(p, x, y)
    assert aerror(y, oracle_dft(x, shape, hm)) < TOL


@pytest.mark.parametrize("shape", [(32, 32), (16, 16), (33, 64), (64, 63), (65, 64), (64, 24), (128, 64)])
def test_extents_outside_the_menu_are_outside_the_rule(shape):
    rng = np.random.default_rng(10)
    n = int(np.prod(shape))
    hm = 5
    x = crand(rng, hm * n)
    y = np.zeros_like(x)
    p = fa.plan_many_dft(2, list(shape), hm, x, None, 1, n, y, None, 1, n, fa.FORWARD)
    assert tile(*shape) == 0
    assert not _has_img2dl(p), p.sprint()
    run_plan_on_host(p, x, y)
    assert aerror(y, oracle_dft(x, shape, hm)) < TOL
