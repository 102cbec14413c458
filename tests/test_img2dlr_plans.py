"""CPU tier of the one-trip real-image plans for extents above 32 (planner.c emit_real_image, FFTW_AMD_K_IMG2DLR,
pass2dlr.hpp): with FFTW_AMD_REAL_IMGL=1 (or a wisdom record with bit 256) batches of dense 2-D r2c / c2r transforms
n0 x n1 with both extents in {16, 32, 40, 48, 64} and at least one above 32 plan as ONE step with exactly the
documented fields, and the extended numpy interpreter (tests/step_interp_img2dlr.py) computes what the oracle
computes -- the c2r from random complex half spectra that are not Hermitian.  Without the knob, with
FFTW_AMD_REAL_IMG=1 alone, and for every layout the rule excludes, the plans are the axis-by-axis ones and match
through the base interpreter.

The pairs: one-stage and two-stage columns, radix-5 and radix-6 second stages, H = n1 / 2 = 8, 20, 24, 32, both
orientations."""
import os
import re

import numpy as np
import pytest

import fftw3_amd as fa
import step_interp
from accuracy_cases import knobs
from step_interp import Interp, scratch_reals
from step_interp_img2dlr import run_plan_on_host
from util import ROOT, TOL, aerror, crand, oracle_c2r, oracle_r2c, rrand

PAIRS = [(64, 64), (16, 40), (40, 16), (48, 64), (64, 48), (32, 64), (40, 40), (64, 16)]
EXTENTS = (16, 32, 40, 48, 64)
ON = {"FFTW_AMD_REAL_IMGL": "1"}
LDS_DOUBLES = 9216


def menu():
    """the (n0, n1) pairs of img2dlr_menu.inc (an entry whose kernel spilled, or whose plan did not measure faster than
    the axis-by-axis plan, was dropped from it)"""
    with open(os.path.join(ROOT, "fftw3_amd", "csrc", "img2dlr_menu.inc")) as f:
        return [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"X\((\d+), (\d+)\)", f.read())]


MENU = menu()


def tile(n0, n1, fwd):
    return fa.img2dlr_tile(n0, n1, fwd)


def _cases():
    return [(n0, n1, which) for n0, n1 in PAIRS for which in ("one", "T", "2T+3")]


def _howmany(n0, n1, which, fwd):
    T = tile(n0, n1, fwd)
    return {"one": 1, "T": T, "2T+3": 2 * T + 3}[which]


_INPUT = {}


def _input(n0, n1, hm, fwd):
    """the same input and oracle result for every test of one case: (logical input, logical output), (hm, n0, .)"""
    key = (n0, n1, hm, fwd)
    if key not in _INPUT:
        rng = np.random.default_rng(1000 * n0 + n1 + (0 if fwd else 7))
        h = n1 // 2 + 1
        if fwd:
            x = rrand(rng, hm, n0, n1)
            y = oracle_r2c(x.reshape(-1), (n0, n1), hm).reshape(hm, n0, h)
        else:
            x = crand(rng, hm, n0, h)                     # not Hermitian
            y = oracle_c2r(x.reshape(-1), (n0, n1), hm).reshape(hm, n0, n1)
        x.setflags(write=False)
        y.setflags(write=False)
        _INPUT[key] = (x, y)
    return _INPUT[key]


def _has(p):
    return any(s.variant == fa.K_IMG2DLR for s in p.steps())


def _plan(n0, n1, hm, fwd, a, b, pitch, flags=fa.ESTIMATE):
    """the plan on flat float64 arrays a -> b (the same object in place): real rows `pitch` doubles apart"""
    h = n1 // 2 + 1
    if fwd:
        return fa.plan_many_dft_r2c(2, [n0, n1], hm, a, [n0, pitch], 1, n0 * pitch, b, [n0, h], 1, n0 * h, flags)
    return fa.plan_many_dft_c2r(2, [n0, n1], hm, a, [n0, h], 1, n0 * h, b, [n0, pitch], 1, n0 * pitch, flags)


def _arrays(n0, n1, hm, fwd, x, pitch, inplace):
    """flat float64 input and output arrays of the layout, the input filled from the logical x"""
    h = n1 // 2 + 1
    rwords, cwords = hm * n0 * pitch, hm * n0 * 2 * h
    a = np.zeros(max(rwords, cwords) if inplace else (rwords if fwd else cwords))
    if fwd:
        a[:rwords].reshape(hm, n0, pitch)[:, :, :n1] = x
    else:
        a[:cwords].view(np.complex128).reshape(hm, n0, h)[:] = x
    b = a if inplace else np.zeros(cwords if fwd else rwords)
    return a, b


def _result(n0, n1, hm, fwd, b, pitch):
    h = n1 // 2 + 1
    if fwd:
        return b[:hm * n0 * 2 * h].view(np.complex128).reshape(hm, n0, h)
    return b[:hm * n0 * pitch].reshape(hm, n0, pitch)[:, :, :n1]


def _layouts(n1):
    return [("dense", n1, False), ("padded", n1 + 2, False), ("inplace", n1 + 2, True)]


def _table_bytes(n0, n1):
    """the stage tables, all a plan with the step owns (no scratch buffer): the row axis always, the column axis when it
    has two stages; one table for equal extents, 16 bytes per entry"""
    return 16 * sum(set([n1] + ([n0] if n0 > 32 else [])))


def test_menu_and_tile_query_agree():
    want = [(a, b) for a in EXTENTS for b in EXTENTS if a > 32 or b > 32]
    assert len(want) == 21
    assert set(MENU) <= set(want) and len(set(MENU)) == len(MENU)
    assert set(PAIRS) <= set(MENU), sorted(set(PAIRS) - set(MENU))
    for n0 in range(0, 67):
        for n1 in range(0, 67):
            for fwd in (True, False):
                T = tile(n0, n1, fwd)
                if (n0, n1) in MENU:
                    assert T >= 1, (n0, n1, fwd, T)
                    # every use of the plane of a workgroup fits a CU twice (72 KiB): the exchanges (rows of W | 1
                    # doubles, W = n1 / 2 complex columns r2c, n1 / 2 + 1 c2r), both parts of Z2 at once (r2c), the
                    # real tile (c2r)
                    H = n1 // 2
                    if fwd:
                        assert 2 * T * n0 * (H | 1) <= LDS_DOUBLES, (n0, n1, fwd, T)
                    else:
                        assert T * n0 * ((H + 1) | 1) <= LDS_DOUBLES and T * n0 * (n1 | 1) <= LDS_DOUBLES, (n0, n1, fwd, T)
                else:
                    assert T == 0, (n0, n1, fwd, T)
                if n1 % 2 or (n0 <= 32 and n1 <= 32):
                    assert T == 0


@pytest.mark.parametrize("n0,n1,which", _cases())
def test_one_step_with_the_documented_fields(n0, n1, which):
    h = n1 // 2 + 1
    for fwd in (True, False):
        hm = _howmany(n0, n1, which, fwd)
        x, _ = _input(n0, n1, hm, fwd)
        for name, pitch, inplace in _layouts(n1):
            a, b = _arrays(n0, n1, hm, fwd, x, pitch, inplace)
            with knobs(ON):
                p = _plan(n0, n1, hm, fwd, a, b, pitch)
            st = p.steps()
            assert len(st) == 1, p.sprint()
            s = st[0]
            assert s.kind == fa.STEP_PASS and s.variant == fa.K_IMG2DLR, p.sprint()
            want = fa.F_REAL_IMG | (fa.F_REAL_IN if fwd else fa.F_REAL_OUT)
            assert s.flags & ~(fa.F_NT_IN | fa.F_NT_OUT) == want, (name, hex(s.flags))
            rside = (0, 1, pitch, n0 * pitch)
            cside = (1, 2, n1 + 2, n0 * (n1 + 2))
            assert (s.L, s.tile_lo_n) == (n1, n0)
            assert (s.src_im, s.is_l, s.tile_lo_is, s.dim_is[0]) == (rside if fwd else cside), name
            assert (s.dst_im, s.os_l, s.tile_lo_os, s.dim_os[0]) == (cside if fwd else rside), name
            assert s.ndims == 1 and s.dim_n[0] == hm
            assert s.tile == tile(n0, n1, fwd) and s.tw_n == 0
            # the stage tables: the row axis always (the untangle / tangle twiddles), the column axis when it has two stages
            assert s.table >= 0 and (s.table2 >= 0) == (n0 > 32)
            assert (s.src_buf, s.dst_buf) == (0, 1)
            # no scratch buffer: the plan owns nothing but those tables
            assert p.workspace_bytes == _table_bytes(n0, n1)
            assert p.batch == p.chunk == hm
            label = "pass-%d/img2dl-%s-%dx%d tile=%d" % (n1, "r2c" if fwd else "c2r", n0, n1, s.tile)
            assert label in p.sprint(), p.sprint()
    assert h == n1 // 2 + 1


@pytest.mark.parametrize("n0,n1,which", _cases())
def test_interpreter_matches_the_oracle(n0, n1, which):
    for fwd in (True, False):
        hm = _howmany(n0, n1, which, fwd)
        x, want = _input(n0, n1, hm, fwd)
        for name, pitch, inplace in _layouts(n1):
            a, b = _arrays(n0, n1, hm, fwd, x, pitch, inplace)
            with knobs(ON):
                p = _plan(n0, n1, hm, fwd, a, b, pitch)
            assert _has(p) and len(p.steps()) == 1
            run_plan_on_host(p, a, b)
            assert aerror(_result(n0, n1, hm, fwd, b, pitch), want) < TOL, (n0, n1, hm, fwd, name)


@pytest.mark.parametrize("env", [{}, {"FFTW_AMD_REAL_IMG": "1"}], ids=["unset", "REAL_IMG"])
@pytest.mark.parametrize("n0,n1,which", _cases())
def test_without_the_knob_the_plans_are_todays(n0, n1, which, env):
    """also with FFTW_AMD_REAL_IMG=1 alone: the knob of the images up to 32 does not switch this step on"""
    for fwd in (True, False):
        hm = _howmany(n0, n1, which, fwd)
        x, want = _input(n0, n1, hm, fwd)
        for name, pitch, inplace in _layouts(n1):
            a, b = _arrays(n0, n1, hm, fwd, x, pitch, inplace)
            with knobs(env):
                p = _plan(n0, n1, hm, fwd, a, b, pitch)
            assert not _has(p) and "img2d" not in p.sprint(), p.sprint()
            step_interp.run_plan_on_host(p, a, b)
            assert aerror(_result(n0, n1, hm, fwd, b, pitch), want) < TOL, (n0, n1, hm, fwd, name)


def _misaligned(words):
    w = np.zeros(words + 2)
    w = w[1:] if w.ctypes.data % 16 == 0 else w[:-1]
    assert w.ctypes.data % 16 == 8
    return w[:words]


class _At(object):
    """an array addressed from `base` words into it"""
    def __init__(self, a, base):
        self.a, self.base = a, base

    def __getitem__(self, i):
        return self.a[np.asarray(i) + self.base]

    def __setitem__(self, i, v):
        self.a[np.asarray(i) + self.base] = v


@pytest.mark.parametrize("fwd", [True, False], ids=["r2c", "c2r"])
@pytest.mark.parametrize("n0,n1,which", _cases())
def test_excluded_layouts_keep_a_plan_without_the_step(n0, n1, which, fwd):
    hm = _howmany(n0, n1, which, fwd)
    x, want = _input(n0, n1, hm, fwd)
    h = n1 // 2 + 1

    def check(p, a, b, pitch, why):
        assert not _has(p) and "img2d" not in p.sprint(), (why, p.sprint())
        step_interp.run_plan_on_host(p, a, b)
        assert aerror(_result(n0, n1, hm, fwd, b, pitch), want) < TOL, (n0, n1, hm, fwd, why)

    with knobs(ON):
        for knob in ("FFTW_AMD_NO_IMG2D", "FFTW_AMD_NO_TUNED"):
            a, b = _arrays(n0, n1, hm, fwd, x, n1, False)
            with knobs({knob: "1"}):
                p = _plan(n0, n1, hm, fwd, a, b, n1)
            check(p, a, b, n1, knob)
        # FFTW_UNALIGNED, on arrays 8 bytes off
        a, b = _arrays(n0, n1, hm, fwd, x, n1, False)
        au, bu = _misaligned(a.size), _misaligned(b.size)
        au[:] = a
        p = _plan(n0, n1, hm, fwd, au, bu, n1, fa.ESTIMATE | fa.UNALIGNED)
        check(p, au, bu, n1, "unaligned")
        # a gapped dist on both sides and on one side (with one image there is no loop, so no dist)
        if hm > 1:
            rd, cd = n0 * n1 + 6, n0 * h + 3
            for gap_r, gap_c in ((True, True), (True, False), (False, True)):
                rdist, cdist = (rd if gap_r else n0 * n1), (cd if gap_c else n0 * h)
                ra, ca = np.zeros(hm * rdist), np.zeros(2 * hm * cdist)
                if fwd:
                    ra.reshape(hm, rdist)[:, :n0 * n1] = x.reshape(hm, -1)
                    p = fa.plan_many_dft_r2c(2, [n0, n1], hm, ra, None, 1, rdist, ca, None, 1, cdist)
                    assert not _has(p), p.sprint()
                    step_interp.run_plan_on_host(p, ra, ca)
                    got = ca.view(np.complex128).reshape(hm, cdist)[:, :n0 * h]
                else:
                    ca.view(np.complex128).reshape(hm, cdist)[:, :n0 * h] = x.reshape(hm, -1)
                    p = fa.plan_many_dft_c2r(2, [n0, n1], hm, ca, None, 1, cdist, ra, None, 1, rdist)
                    assert not _has(p), p.sprint()
                    step_interp.run_plan_on_host(p, ca, ra)
                    got = ra.reshape(hm, rdist)[:, :n0 * n1]
                assert aerror(got, want.reshape(hm, -1)) < TOL, (gap_r, gap_c)
        # a real pitch that is neither n1 nor n1 + 2
        a, b = _arrays(n0, n1, hm, fwd, x, n1 + 4, False)
        check(_plan(n0, n1, hm, fwd, a, b, n1 + 4), a, b, n1 + 4, "real pitch n1 + 4")
        # a complex pitch above n1 + 2
        hp = h + 1
        ca, ra = np.zeros(2 * hm * n0 * hp), np.zeros(hm * n0 * n1)
        if fwd:
            ra[:] = x.reshape(-1)
            p = fa.plan_many_dft_r2c(2, [n0, n1], hm, ra, None, 1, n0 * n1, ca, [n0, hp], 1, n0 * hp)
            assert not _has(p), p.sprint()
            step_interp.run_plan_on_host(p, ra, ca)
            got = ca.view(np.complex128).reshape(hm, n0, hp)[:, :, :h]
        else:
            ca.view(np.complex128).reshape(hm, n0, hp)[:, :, :h] = x
            p = fa.plan_many_dft_c2r(2, [n0, n1], hm, ca, [n0, hp], 1, n0 * hp, ra, None, 1, n0 * n1)
            assert not _has(p), p.sprint()
            step_interp.run_plan_on_host(p, ca, ra)
            got = ra.reshape(hm, n0, n1)
        assert aerror(got, want) < TOL, "complex pitch"
        # a split complex side through the guru interface (one allocation: the interpreter addresses the imaginary
        # plane from the real one)
        R, Cn = hm * n0 * n1, hm * n0 * h
        s = np.zeros(R + 2 * Cn)
        dims_r = [(n0, n1, h), (n1, 1, 1)]
        if fwd:
            s[:R] = x.reshape(-1)
            p = fa.plan_guru64_split_dft_r2c(dims_r, [(hm, n0 * n1, n0 * h)], s[:R], s[R:R + Cn], s[R + Cn:])
            assert not _has(p), p.sprint()
            Interp(p).run(s, _At(s, R), scratch_reals(p))
            got = (s[R:R + Cn] + 1j * s[R + Cn:]).reshape(hm, n0, h)
        else:
            s[R:R + Cn], s[R + Cn:] = x.real.reshape(-1), x.imag.reshape(-1)
            p = fa.plan_guru64_split_dft_c2r([(n0, h, n1), (n1, 1, 1)], [(hm, n0 * h, n0 * n1)], s[R:R + Cn], s[R + Cn:],
                                             s[:R])
            assert not _has(p), p.sprint()
            Interp(p).run(_At(s, R), s, scratch_reals(p))
            got = s[:R].reshape(hm, n0, n1)
        assert aerror(got, want) < TOL, "split"
        # the same dense images through the interleaved guru interface do get the step; two howmany loops do not
        a, b = _arrays(n0, n1, hm, fwd, x, n1, False)
        if fwd:
            p = fa.plan_guru64_dft_r2c(dims_r, [(hm, n0 * n1, n0 * h)], a, b)
        else:
            p = fa.plan_guru64_dft_c2r([(n0, h, n1), (n1, 1, 1)], [(hm, n0 * h, n0 * n1)], a, b)
        assert _has(p), p.sprint()
        if hm % 2 == 0 and hm > 2:
            if fwd:
                p = fa.plan_guru64_dft_r2c(dims_r, [(hm // 2, 2 * n0 * n1, 2 * n0 * h), (2, n0 * n1, n0 * h)], a, b)
            else:
                p = fa.plan_guru64_dft_c2r([(n0, h, n1), (n1, 1, 1)],
                                           [(hm // 2, 2 * n0 * h, 2 * n0 * n1), (2, n0 * h, n0 * n1)], a, b)
            check(p, a, b, n1, "two howmany loops")


@pytest.mark.parametrize("fwd", [True, False], ids=["r2c", "c2r"])
@pytest.mark.parametrize("shape", [(32, 32), (16, 16), (33, 64), (64, 62), (64, 63), (40, 65), (64, 24), (128, 64), (2, 64, 64),
                                   (3, 16, 40)], ids=lambda s: "x".join(str(v) for v in s))
def test_other_extents_odd_rows_and_rank_3_are_outside_the_rule(shape, fwd):
    rng = np.random.default_rng(11)
    hm = 5
    n, nl = int(np.prod(shape)), shape[-1]
    hn = n // nl * (nl // 2 + 1)
    if len(shape) == 2:
        assert tile(shape[0], shape[1], fwd) == 0
    with knobs(ON):
        if fwd:
            x = rrand(rng, hm * n)
            y = np.zeros(hm * hn, dtype=np.complex128)
            p = fa.plan_many_dft_r2c(len(shape), list(shape), hm, x, None, 1, n, y, None, 1, hn)
            want = oracle_r2c(x, shape, hm)
        else:
            x = crand(rng, hm * hn)
            y = np.zeros(hm * n)
            p = fa.plan_many_dft_c2r(len(shape), list(shape), hm, x.copy(), None, 1, hn, y, None, 1, n)
            want = oracle_c2r(x, shape, hm)
        assert not _has(p), p.sprint()
        xin = x.copy()
        step_interp.run_plan_on_host(p, xin, y)
        assert aerror(y, want) < TOL


def test_wisdom_bit_256_switches_the_step_on():
    """bits 32 (real_img) and 128 (real_vol) alone do not; export equals import"""
    n0, n1, hm = 40, 16, 7
    h = n1 // 2 + 1
    x, want = _input(n0, n1, hm, True)
    a, b = _arrays(n0, n1, hm, True, x, n1, False)
    fa.forget_wisdom()
    try:
        key = "t1 s-1 r2 %d:%d:%d %d:1:2 h1 %d:%d:%d i0 o1 p0" % (n0, n1, 2 * h, n1, hm, n0 * n1, 2 * n0 * h)
        for bits, on in ((256 | 4, True), (4, False), (32 | 4, False), (128 | 4, False), (32 | 128 | 4, False),
                         (256 | 32 | 4, True)):
            rec = "(fftw3_amd_wisdom-1\n  (%s) 134217728 0 1024 %d 0.250000\n)\n" % (key, bits)
            assert fa.import_wisdom_from_string(rec) == 1
            assert fa.export_wisdom_to_string() == rec
            p = _plan(n0, n1, hm, True, a, b, n1, fa.ESTIMATE | fa.WISDOM_ONLY)   # the key is the problem's
            assert _has(p) == on, (bits, p.sprint())
            b[:] = 0
            run_plan_on_host(p, a, b)
            assert aerror(_result(n0, n1, hm, True, b, n1), want) < TOL
            fa.forget_wisdom()
    finally:
        fa.forget_wisdom()
