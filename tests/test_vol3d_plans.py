"""CPU tier of the one-trip small-volume plans (planner.c emit_vol3d, FFTW_AMD_K_VOL3D, pass3d.hpp): with
FFTW_AMD_VOL3D=1 (or a wisdom record with bit 64) batches of dense 3-D c2c transforms n0 x n1 x n2 of vol3d_menu.inc
plan as ONE step with exactly the documented fields, and the extended numpy interpreter (tests/step_interp_vol3d.py)
computes what the oracle computes.  Without the knob, and for every layout the rule excludes, the plans are the
axis-by-axis ones.

The ten triples: T > 1, ragged butterfly counts, T = 1 at full size, extent 32, odd and prime-factor radices, and three
distinct extents (6 x 10 x 12 tells an axis mix-up from a correct kernel off the powers of two)."""
import os
import re

import numpy as np
import pytest

import fftw3_amd as fa
import step_interp
from accuracy_cases import knobs
from step_interp_vol3d import run_plan_on_host
from util import ROOT, TOL, aerror, crand, oracle_dft

TEN = [(4, 4, 4), (4, 8, 16), (16, 8, 4), (8, 8, 8), (16, 16, 16), (16, 16, 32), (32, 8, 32), (5, 5, 5), (15, 15, 15),
       (6, 10, 12)]
ON = {"FFTW_AMD_VOL3D": "1"}


def menu():
    """the (n0, n1, n2) triples of vol3d_menu.inc (an entry whose kernel spilled, or whose plan did not measure faster
    than the axis-by-axis plan, was dropped from it)"""
    with open(os.path.join(ROOT, "fftw3_amd", "csrc", "vol3d_menu.inc")) as f:
        return [tuple(int(v) for v in m.groups()) for m in re.finditer(r"X\((\d+), (\d+), (\d+)\)", f.read())]


MENU = menu()
IDS = ["%dx%dx%d" % t for t in MENU]
TEN_IDS = ["%dx%dx%d" % t for t in TEN]


def tile(n0, n1, n2):
    return fa.vol3d_tile(n0, n1, n2)


def label(n0, n1, n2):
    return "pass-%d/vol3d-%dx%dx%d tile=%d" % (n2, n0, n1, n2, tile(n0, n1, n2))


_INPUT = {}


def _input(shape, hm):
    """the same input and oracle results (forward, backward) for every test of one case"""
    key = (shape, hm)
    if key not in _INPUT:
        rng = np.random.default_rng(10000 * shape[0] + 100 * shape[1] + shape[2])
        x = crand(rng, hm * int(np.prod(shape)))
        _INPUT[key] = (x, {s: oracle_dft(x, shape, hm, s) for s in (-1, +1)})
        for v in _INPUT[key][1].values():
            v.setflags(write=False)
        x.setflags(write=False)
    return _INPUT[key]


def _has(p):
    return any(s.variant == fa.K_VOL3D for s in p.steps())


def _plan(shape, hm, x, y, sign=fa.FORWARD, flags=fa.ESTIMATE):
    n = int(np.prod(shape))
    return fa.plan_many_dft(3, list(shape), hm, x, None, 1, n, y, None, 1, n, sign, flags)


def test_menu_and_tile_query_agree():
    assert len(set(MENU)) == len(MENU)
    assert set(TEN) <= set(MENU), sorted(set(TEN) - set(MENU))
    for t in MENU:
        T = tile(*t)
        assert T >= 1 and T * t[0] * t[1] * t[2] <= 8192, (t, T)
    for t in [(7, 8, 8), (32, 32, 32), (32, 32, 16), (0, 4, 4), (4, 4, 33), (4, 4, 64), (3, 3, 3)]:
        assert t not in MENU and tile(*t) == 0, t


@pytest.mark.parametrize("shape", MENU, ids=IDS)
def test_one_step_with_the_documented_fields(shape):
    n0, n1, n2 = shape
    T = tile(*shape)
    hm = 2 * T + 3
    n = n0 * n1 * n2
    x = np.zeros(hm * n, dtype=np.complex128)
    y = np.zeros_like(x)
    for sign in (fa.FORWARD, fa.BACKWARD):
        for out in (y, x):
            with knobs(ON):
                p = _plan(shape, hm, x, out, sign)
            st = p.steps()
            assert len(st) == 1, p.sprint()
            s = st[0]
            assert s.kind == fa.STEP_PASS and s.variant == fa.K_VOL3D, p.sprint()
            want = fa.F_LO_DFT | fa.F_VOL3D | ((fa.F_SWAP_IN | fa.F_SWAP_OUT) if sign == fa.BACKWARD else 0)
            assert s.flags & ~(fa.F_NT_IN | fa.F_NT_OUT) == want, hex(s.flags)
            assert (s.L, s.is_l, s.os_l) == (n2, 2, 2)
            assert (s.tile_lo_n, s.tile_lo_is, s.tile_lo_os) == (n1, 2 * n2, 2 * n2)
            assert s.aux_n == n0
            assert s.ndims == 1 and (s.dim_n[0], s.dim_is[0], s.dim_os[0]) == (hm, 2 * n, 2 * n)
            assert s.tile == T
            assert s.tw_n == 0 and s.table == -1 and s.table2 == -1 and s.src_im == 1 and s.dst_im == 1
            assert (s.src_buf, s.dst_buf) == (0, 1)
            assert p.workspace_bytes == 0
            assert p.batch == p.chunk == hm
            assert label(*shape) in p.sprint(), p.sprint()


@pytest.mark.parametrize("which", ["one", "2T+3"])
@pytest.mark.parametrize("shape", TEN, ids=TEN_IDS)
def test_interpreter_matches_the_oracle(shape, which):
    hm = 1 if which == "one" else 2 * tile(*shape) + 3
    x, want = _input(shape, hm)
    for sign in (fa.FORWARD, fa.BACKWARD):
        y = np.zeros_like(x)
        with knobs(ON):
            p = _plan(shape, hm, x, y, sign)
        assert _has(p) and len(p.steps()) == 1, p.sprint()
        run_plan_on_host(p, x, y)
        assert aerror(y, want[sign]) < TOL, (shape, hm, sign)
        z = x.copy()                                   # in place
        with knobs(ON):
            p = _plan(shape, hm, z, z, sign)
        assert _has(p) and len(p.steps()) == 1 and p.workspace_bytes == 0
        run_plan_on_host(p, z, z)
        assert aerror(z, want[sign]) < TOL, (shape, hm, sign, "in place")


@pytest.mark.parametrize("shape", TEN, ids=TEN_IDS)
def test_without_the_knob_the_plans_are_the_axis_by_axis_ones(shape):
    for hm in (1, 2 * tile(*shape) + 3):
        x, want = _input(shape, hm)
        for sign in (fa.FORWARD, fa.BACKWARD):
            for inplace in (False, True):
                a = x.copy()
                b = a if inplace else np.zeros_like(a)
                off = _plan(shape, hm, a, b, sign)
                assert not _has(off) and "vol3d" not in off.sprint(), off.sprint()
                with knobs(ON):
                    with knobs({"FFTW_AMD_NO_IMG2D": "1"}):
                        no = _plan(shape, hm, a, b, sign)
                assert no.sprint() == off.sprint(), (no.sprint(), off.sprint())
                step_interp.run_plan_on_host(off, a, b)
                assert aerror(b, want[sign]) < TOL, (shape, hm, sign, inplace)


def _misaligned(words):
    w = np.zeros(words + 2)
    w = w[1:] if w.ctypes.data % 16 == 0 else w[:-1]
    assert w.ctypes.data % 16 == 8
    return w[:words]


@pytest.mark.parametrize("shape", TEN, ids=TEN_IDS)
def test_excluded_layouts_keep_a_plan_without_the_step(shape):
    n0, n1, n2 = shape
    T = tile(*shape)
    hm = 2 * T + 3 + (2 * T + 3) % 2                   # even, for the two howmany loops
    n = n0 * n1 * n2
    x, want = _input(shape, hm)
    w = want[-1]

    def check(p, a, b, why, got=None):
        assert not _has(p) and "vol3d" not in p.sprint(), (why, p.sprint())
        step_interp.run_plan_on_host(p, a, b)
        assert aerror(b if got is None else got(), w) < TOL, (shape, why)

    with knobs(ON):
        y = np.zeros_like(x)
        assert _has(_plan(shape, hm, x, y))
        # FFTW_AMD_NO_TUNED
        with knobs({"FFTW_AMD_NO_TUNED": "1"}):
            p = _plan(shape, hm, x, y)
        check(p, x, y, "FFTW_AMD_NO_TUNED")
        # FFTW_UNALIGNED on aligned arrays, and a pointer 8 bytes off (which needs FFTW_UNALIGNED)
        y = np.zeros_like(x)
        check(_plan(shape, hm, x, y, flags=fa.ESTIMATE | fa.UNALIGNED), x, y, "FFTW_UNALIGNED")
        xu, yu = _misaligned(2 * hm * n), _misaligned(2 * hm * n)
        xu[:] = x.view(np.float64)
        p = _plan(shape, hm, xu, yu, flags=fa.ESTIMATE | fa.UNALIGNED)
        check(p, xu, yu, "8 bytes off", lambda: yu.view(np.complex128))
        # a howmany distance larger than a volume, on both sides and on one
        dist = n + 3
        xg = np.zeros(hm * dist, dtype=np.complex128)
        xg.reshape(hm, dist)[:, :n] = x.reshape(hm, n)
        yg = np.zeros_like(xg)
        p = fa.plan_many_dft(3, list(shape), hm, xg, None, 1, dist, yg, None, 1, dist, fa.FORWARD)
        check(p, xg, yg, "dist", lambda: yg.reshape(hm, dist)[:, :n])
        yd = np.zeros_like(x)
        p = fa.plan_many_dft(3, list(shape), hm, xg, None, 1, dist, yd, None, 1, n, fa.FORWARD)
        check(p, xg, yd, "dist on the input only")
        # padded rows
        pitch = n2 + 2
        xp = np.zeros(hm * n0 * n1 * pitch, dtype=np.complex128)
        xp.reshape(hm, n0, n1, pitch)[:, :, :, :n2] = x.reshape(hm, n0, n1, n2)
        yp = np.zeros_like(x)
        p = fa.plan_many_dft(3, list(shape), hm, xp, [n0, n1, pitch], 1, n0 * n1 * pitch, yp, None, 1, n, fa.FORWARD)
        check(p, xp, yp, "padded rows")
        # split arrays through the guru interface
        N = hm * n
        s = np.zeros(4 * N)
        s[0:N], s[N:2 * N] = x.real, x.imag
        dims = [(n0, n1 * n2, n1 * n2), (n1, n2, n2), (n2, 1, 1)]
        p = fa.plan_guru64_split_dft(dims, [(hm, n, n)], s[0:N], s[N:2 * N], s[2 * N:3 * N], s[3 * N:], fa.ESTIMATE)
        assert not _has(p) and "vol3d" not in p.sprint(), p.sprint()
        # the same dense volumes through the interleaved guru interface do get the step; two howmany loops do not
        y = np.zeros_like(x)
        p = fa.plan_guru64_dft(dims, [(hm, n, n)], x, y, fa.FORWARD)
        assert _has(p), p.sprint()
        p = fa.plan_guru64_dft(dims, [(hm // 2, 2 * n, 2 * n), (2, n, n)], x, y, fa.FORWARD)
        check(p, x, y, "two howmany loops")


@pytest.mark.parametrize("shape", [(7, 8, 8), (32, 32, 32), (16, 16), (4, 4, 4, 4)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_triples_outside_the_menu_and_other_ranks_are_outside_the_rule(shape):
    rng = np.random.default_rng(12)
    n = int(np.prod(shape))
    hm = 3
    x = crand(rng, hm * n)
    y = np.zeros_like(x)
    if len(shape) == 3:
        assert tile(*shape) == 0
    with knobs(ON):
        p = fa.plan_many_dft(len(shape), list(shape), hm, x, None, 1, n, y, None, 1, n, fa.FORWARD)
    assert not _has(p) and "vol3d" not in p.sprint(), p.sprint()
    step_interp.run_plan_on_host(p, x, y)
    assert aerror(y, oracle_dft(x, shape, hm)) < TOL


def test_wisdom_bit_64_switches_the_step_on():
    shape, hm = (6, 10, 12), 5
    n0, n1, n2 = shape
    n = n0 * n1 * n2
    x, want = _input(shape, hm)
    y = np.zeros_like(x)
    fa.forget_wisdom()
    try:
        key = "t0 s-1 r3 %d:%d:%d %d:%d:%d %d:2:2 h1 %d:%d:%d i1 o1 p0" % (n0, 2 * n1 * n2, 2 * n1 * n2, n1, 2 * n2, 2 * n2,
                                                                           n2, hm, 2 * n, 2 * n)
        for bits, on in ((64 | 4, True), (4, False), (32 | 16 | 4, False)):
            rec = "(fftw3_amd_wisdom-1\n  (%s) 134217728 0 1024 %d 0.250000\n)\n" % (key, bits)
            assert fa.import_wisdom_from_string(rec) == 1
            assert fa.export_wisdom_to_string() == rec
            p = _plan(shape, hm, x, y, flags=fa.ESTIMATE | fa.WISDOM_ONLY)   # the key is the problem's
            assert _has(p) == on, (bits, p.sprint())
            y[:] = 0
            run_plan_on_host(p, x, y)
            assert aerror(y, want[-1]) < TOL
            fa.forget_wisdom()
    finally:
        fa.forget_wisdom()
