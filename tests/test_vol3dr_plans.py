"""CPU tier of the one-trip small real-volume plans (planner.c emit_real_volume, FFTW_AMD_K_VOL3DR, pass3dr.hpp): with
FFTW_AMD_REAL_VOL=1 (or a wisdom record with bit 128) batches of 3-D r2c / c2r transforms n0 x n1 x n2, every extent at
most 32 and n2 even, plan as ONE step with exactly the documented fields, and the extended numpy interpreter
(tests/step_interp_vol3dr.py) computes what the oracle computes -- the c2r from random complex half spectra that are
not Hermitian.  Without the knob, and for every layout the rule excludes, the plans are the axis-by-axis ones and match
through the base interpreter.

The triples: tiles of many volumes and of one, an extent of 32 on every axis, three distinct extents with odd radices,
and odd leading extents (no self-paired plane n0 / 2, an odd number of row pairs)."""
import os
import re

import numpy as np
import pytest

import fftw3_amd as fa
import step_interp
from accuracy_cases import knobs
from step_interp import Interp, scratch_reals
from step_interp_vol3dr import run_plan_on_host
from util import ROOT, TOL, aerror, crand, oracle_c2r, oracle_r2c, rrand

TRIPLES = [(4, 4, 4), (4, 8, 16), (16, 8, 4), (8, 8, 8), (16, 16, 16), (16, 16, 32), (32, 8, 32), (6, 10, 12), (10, 12, 6),
           (5, 5, 10), (15, 15, 6)]
ON = {"FFTW_AMD_REAL_VOL": "1"}


def menu():
    """the (n0, n1, n2) triples of vol3dr_menu.inc"""
    with open(os.path.join(ROOT, "fftw3_amd", "csrc", "vol3dr_menu.inc")) as f:
        return [tuple(int(v) for v in m.groups()) for m in re.finditer(r"X\((\d+), (\d+), (\d+)\)", f.read())]


MENU = menu()


def tile(t, fwd):
    return fa.vol3dr_tile(t[0], t[1], t[2], fwd)


def _cases():
    return [(t, which) for t in TRIPLES for which in ("one", "2T+3")]


def _ids(v):
    return "x".join(str(k) for k in v) if isinstance(v, tuple) else str(v)


def _howmany(t, which, fwd):
    return {"one": 1, "2T+3": 2 * tile(t, fwd) + 3}[which]


_INPUT = {}


def _input(t, hm, fwd):
    """the same input and oracle result for every test of one case: (logical input, logical output)"""
    key = (t, hm, fwd)
    if key not in _INPUT:
        n0, n1, n2 = t
        rng = np.random.default_rng(10000 * n0 + 100 * n1 + n2 + (0 if fwd else 7))
        h = n2 // 2 + 1
        if fwd:
            x = rrand(rng, hm, n0, n1, n2)
            y = oracle_r2c(x.reshape(-1), t, hm).reshape(hm, n0, n1, h)
        else:
            x = crand(rng, hm, n0, n1, h)                 # not Hermitian
            y = oracle_c2r(x.reshape(-1), t, hm).reshape(hm, n0, n1, n2)
        x.setflags(write=False)
        y.setflags(write=False)
        _INPUT[key] = (x, y)
    return _INPUT[key]


def _has(p):
    return any(s.variant == fa.K_VOL3DR for s in p.steps())


def _plan(t, hm, fwd, a, b, pitch, flags=fa.ESTIMATE):
    """the plan on flat float64 arrays a -> b (the same object in place): real rows `pitch` doubles apart"""
    n0, n1, n2 = t
    h = n2 // 2 + 1
    if fwd:
        return fa.plan_many_dft_r2c(3, list(t), hm, a, [n0, n1, pitch], 1, n0 * n1 * pitch, b, [n0, n1, h], 1, n0 * n1 * h, flags)
    return fa.plan_many_dft_c2r(3, list(t), hm, a, [n0, n1, h], 1, n0 * n1 * h, b, [n0, n1, pitch], 1, n0 * n1 * pitch, flags)


def _arrays(t, hm, fwd, x, pitch, inplace):
    """flat float64 input and output arrays of the layout, the input filled from the logical x"""
    n0, n1, n2 = t
    h = n2 // 2 + 1
    rwords, cwords = hm * n0 * n1 * pitch, hm * n0 * n1 * 2 * h
    a = np.zeros(max(rwords, cwords) if inplace else (rwords if fwd else cwords))
    if fwd:
        a[:rwords].reshape(hm, n0, n1, pitch)[..., :n2] = x
    else:
        a[:cwords].view(np.complex128).reshape(hm, n0, n1, h)[:] = x
    b = a if inplace else np.zeros(cwords if fwd else rwords)
    return a, b


def _result(t, hm, fwd, b, pitch):
    n0, n1, n2 = t
    h = n2 // 2 + 1
    if fwd:
        return b[:hm * n0 * n1 * 2 * h].view(np.complex128).reshape(hm, n0, n1, h)
    return b[:hm * n0 * n1 * pitch].reshape(hm, n0, n1, pitch)[..., :n2]


def _layouts(n2):
    return [("dense", n2, False), ("padded", n2 + 2, False), ("inplace", n2 + 2, True)]


def test_menu_and_tile_query_agree():
    assert len(set(MENU)) == len(MENU) and MENU
    assert set(TRIPLES) <= set(MENU), sorted(set(TRIPLES) - set(MENU))
    # the categories of the fixed set
    assert any(min(tile(t, True), tile(t, False)) > 1 for t in TRIPLES)
    assert any(tile(t, True) == 1 and tile(t, False) == 1 for t in TRIPLES)
    for n0 in (0, 1, 3, 4, 5, 6, 8, 10, 12, 15, 16, 32, 33):
        for n1 in (0, 1, 4, 5, 6, 7, 8, 10, 12, 15, 16, 32, 33):
            for n2 in range(0, 35):
                for fwd in (True, False):
                    T = tile((n0, n1, n2), fwd)
                    if (n0, n1, n2) in MENU:
                        h = n2 // 2 + 1
                        assert T >= 1, (n0, n1, n2, fwd, T)
                        # the plane of a workgroup fits a CU twice in each of its uses (unpadded lower bounds), and no
                        # item holds more than 32 run-order values
                        words = (n2 // 2, h) if fwd else (h, n2)
                        assert T * n0 * n1 * max(words) <= 9216, (n0, n1, n2, fwd, T)
                        assert T * n0 * n1 * (h if fwd else n2 // 2) <= 32 * 256, (n0, n1, n2, fwd, T)
                    else:
                        assert T == 0, (n0, n1, n2, fwd, T)
                    if n2 % 2:
                        assert T == 0
    for t in ((16, 32, 32), (32, 16, 32), (32, 32, 16), (33, 4, 4), (4, 4, 34), (5, 5, 5), (4, 4, 5)):
        assert tile(t, True) == 0 and tile(t, False) == 0


@pytest.mark.parametrize("t,which", _cases(), ids=_ids)
def test_one_step_with_the_documented_fields(t, which):
    n0, n1, n2 = t
    for fwd in (True, False):
        hm = _howmany(t, which, fwd)
        x, _ = _input(t, hm, fwd)
        for name, pitch, inplace in _layouts(n2):
            a, b = _arrays(t, hm, fwd, x, pitch, inplace)
            with knobs(ON):
                p = _plan(t, hm, fwd, a, b, pitch)
            st = p.steps()
            assert len(st) == 1, p.sprint()
            s = st[0]
            assert s.kind == fa.STEP_PASS and s.variant == fa.K_VOL3DR, p.sprint()
            want = fa.F_REAL_VOL | (fa.F_REAL_IN if fwd else fa.F_REAL_OUT)
            assert s.flags & ~(fa.F_NT_IN | fa.F_NT_OUT) == want, (name, hex(s.flags))
            rside = (0, 1, pitch, n0 * n1 * pitch)
            cside = (1, 2, n2 + 2, n0 * n1 * (n2 + 2))
            assert (s.L, s.tile_lo_n, s.aux_n) == (n2, n1, n0)
            assert (s.src_im, s.is_l, s.tile_lo_is, s.dim_is[0]) == (rside if fwd else cside), name
            assert (s.dst_im, s.os_l, s.tile_lo_os, s.dim_os[0]) == (cside if fwd else rside), name
            assert s.ndims == 1 and s.dim_n[0] == hm
            assert s.tile == tile(t, fwd) and s.tw_n == 0 and s.table == -1 and s.table2 == -1
            assert (s.src_buf, s.dst_buf) == (0, 1)
            assert p.workspace_bytes == 0
            assert p.batch == p.chunk == hm
            label = "pass-%d/vol3d-%s-%dx%dx%d tile=%d" % (n2, "r2c" if fwd else "c2r", n0, n1, n2, s.tile)
            assert label in p.sprint(), p.sprint()


@pytest.mark.parametrize("t,which", _cases(), ids=_ids)
def test_interpreter_matches_the_oracle(t, which):
    for fwd in (True, False):
        hm = _howmany(t, which, fwd)
        x, want = _input(t, hm, fwd)
        for name, pitch, inplace in _layouts(t[2]):
            a, b = _arrays(t, hm, fwd, x, pitch, inplace)
            with knobs(ON):
                p = _plan(t, hm, fwd, a, b, pitch)
            assert _has(p) and len(p.steps()) == 1
            run_plan_on_host(p, a, b)
            assert aerror(_result(t, hm, fwd, b, pitch), want) < TOL, (t, hm, fwd, name)


@pytest.mark.parametrize("t,which", _cases(), ids=_ids)
def test_without_the_knob_the_plans_are_todays(t, which):
    for fwd in (True, False):
        hm = _howmany(t, which, fwd)
        x, want = _input(t, hm, fwd)
        for name, pitch, inplace in _layouts(t[2]):
            a, b = _arrays(t, hm, fwd, x, pitch, inplace)
            p = _plan(t, hm, fwd, a, b, pitch)
            assert not _has(p) and "vol3d" not in p.sprint(), p.sprint()
            # the sibling knobs do not imply this one, and NO_IMG2D / NO_TUNED aside the plan is the same text
            with knobs({"FFTW_AMD_REAL_IMG": "1", "FFTW_AMD_VOL3D": "1"}):
                q = _plan(t, hm, fwd, a, b, pitch)
            assert q.sprint() == p.sprint()
            step_interp.run_plan_on_host(p, a, b)
            assert aerror(_result(t, hm, fwd, b, pitch), want) < TOL, (t, hm, fwd, name)


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
@pytest.mark.parametrize("t,which", _cases(), ids=_ids)
def test_excluded_layouts_keep_a_plan_without_the_step(t, which, fwd):
    n0, n1, n2 = t
    hm = _howmany(t, which, fwd)
    x, want = _input(t, hm, fwd)
    h = n2 // 2 + 1
    nr, nc = n0 * n1 * n2, n0 * n1 * h

    def check(p, a, b, pitch, why):
        assert not _has(p) and "vol3d" not in p.sprint(), (why, p.sprint())
        step_interp.run_plan_on_host(p, a, b)
        assert aerror(_result(t, hm, fwd, b, pitch), want) < TOL, (t, hm, fwd, why)

    with knobs(ON):
        for knob in ("FFTW_AMD_NO_IMG2D", "FFTW_AMD_NO_TUNED"):
            a, b = _arrays(t, hm, fwd, x, n2, False)
            with knobs({knob: "1"}):
                p = _plan(t, hm, fwd, a, b, n2)
            check(p, a, b, n2, knob)
        # arrays 8 bytes off, with and without FFTW_UNALIGNED; FFTW_UNALIGNED on aligned arrays
        a, b = _arrays(t, hm, fwd, x, n2, False)
        au, bu = _misaligned(a.size), _misaligned(b.size)
        au[:] = a
        check(_plan(t, hm, fwd, au, bu, n2, fa.ESTIMATE | fa.UNALIGNED), au, bu, n2, "8-byte offset, unaligned flag")
        bu[:] = 0
        check(_plan(t, hm, fwd, au, bu, n2), au, bu, n2, "8-byte offset")
        check(_plan(t, hm, fwd, a, b, n2, fa.ESTIMATE | fa.UNALIGNED), a, b, n2, "unaligned flag")
        # in place with dense rows (the c2r then has rows of n2 + 2 doubles on the complex side only)
        a, _ = _arrays(t, hm, fwd, x, n2, True)
        if fwd:
            pass                                            # r2c in place needs the padded rows: not a valid dense problem
        else:
            check(_plan(t, hm, fwd, a, a, n2), a, a, n2, "in place, dense rows")
        # a gapped volume pitch on both sides and on one side (with one volume there is no loop, so no dist)
        if hm > 1:
            rd, cd = nr + 6, nc + 3
            for gap_r, gap_c in ((True, True), (True, False), (False, True)):
                rdist, cdist = (rd if gap_r else nr), (cd if gap_c else nc)
                ra, ca = np.zeros(hm * rdist), np.zeros(2 * hm * cdist)
                if fwd:
                    ra.reshape(hm, rdist)[:, :nr] = x.reshape(hm, -1)
                    p = fa.plan_many_dft_r2c(3, list(t), hm, ra, None, 1, rdist, ca, None, 1, cdist)
                    assert not _has(p), p.sprint()
                    step_interp.run_plan_on_host(p, ra, ca)
                    got = ca.view(np.complex128).reshape(hm, cdist)[:, :nc]
                else:
                    ca.view(np.complex128).reshape(hm, cdist)[:, :nc] = x.reshape(hm, -1)
                    p = fa.plan_many_dft_c2r(3, list(t), hm, ca, None, 1, cdist, ra, None, 1, rdist)
                    assert not _has(p), p.sprint()
                    step_interp.run_plan_on_host(p, ca, ra)
                    got = ra.reshape(hm, rdist)[:, :nr]
                assert aerror(got, want.reshape(hm, -1)) < TOL, (gap_r, gap_c)
        # a real row pitch that is neither n2 nor n2 + 2, and a gapped plane pitch (one row more per plane)
        a, b = _arrays(t, hm, fwd, x, n2 + 4, False)
        check(_plan(t, hm, fwd, a, b, n2 + 4), a, b, n2 + 4, "real pitch n2 + 4")
        ra, ca = np.zeros(hm * n0 * (n1 + 1) * n2), np.zeros(2 * hm * nc)
        if fwd:
            ra.reshape(hm, n0, n1 + 1, n2)[:, :, :n1] = x
            p = fa.plan_many_dft_r2c(3, list(t), hm, ra, [n0, n1 + 1, n2], 1, n0 * (n1 + 1) * n2, ca, None, 1, nc)
            assert not _has(p), p.sprint()
            step_interp.run_plan_on_host(p, ra, ca)
            got = ca.view(np.complex128).reshape(hm, n0, n1, h)
        else:
            ca.view(np.complex128)[:] = x.reshape(-1)
            p = fa.plan_many_dft_c2r(3, list(t), hm, ca, None, 1, nc, ra, [n0, n1 + 1, n2], 1, n0 * (n1 + 1) * n2)
            assert not _has(p), p.sprint()
            step_interp.run_plan_on_host(p, ca, ra)
            got = ra.reshape(hm, n0, n1 + 1, n2)[:, :, :n1]
        assert aerror(got, want) < TOL, "plane pitch"
        # a complex row pitch other than n2 / 2 + 1
        hp = h + 1
        ca, ra = np.zeros(2 * hm * n0 * n1 * hp), np.zeros(hm * nr)
        if fwd:
            ra[:] = x.reshape(-1)
            p = fa.plan_many_dft_r2c(3, list(t), hm, ra, None, 1, nr, ca, [n0, n1, hp], 1, n0 * n1 * hp)
            assert not _has(p), p.sprint()
            step_interp.run_plan_on_host(p, ra, ca)
            got = ca.view(np.complex128).reshape(hm, n0, n1, hp)[..., :h]
        else:
            ca.view(np.complex128).reshape(hm, n0, n1, hp)[..., :h] = x
            p = fa.plan_many_dft_c2r(3, list(t), hm, ca, [n0, n1, hp], 1, n0 * n1 * hp, ra, None, 1, nr)
            assert not _has(p), p.sprint()
            step_interp.run_plan_on_host(p, ca, ra)
            got = ra.reshape(hm, n0, n1, n2)
        assert aerror(got, want) < TOL, "complex pitch"
        # a split complex side through the guru interface (one allocation: the interpreter addresses the imaginary
        # plane from the real one)
        R, Cn = hm * nr, hm * nc
        s = np.zeros(R + 2 * Cn)
        dims_r = [(n0, n1 * n2, n1 * h), (n1, n2, h), (n2, 1, 1)]
        dims_c = [(n0, n1 * h, n1 * n2), (n1, h, n2), (n2, 1, 1)]
        if fwd:
            s[:R] = x.reshape(-1)
            p = fa.plan_guru64_split_dft_r2c(dims_r, [(hm, nr, nc)], s[:R], s[R:R + Cn], s[R + Cn:])
            assert not _has(p), p.sprint()
            Interp(p).run(s, _At(s, R), scratch_reals(p))
            got = (s[R:R + Cn] + 1j * s[R + Cn:]).reshape(hm, n0, n1, h)
        else:
            s[R:R + Cn], s[R + Cn:] = x.real.reshape(-1), x.imag.reshape(-1)
            p = fa.plan_guru64_split_dft_c2r(dims_c, [(hm, nc, nr)], s[R:R + Cn], s[R + Cn:], s[:R])
            assert not _has(p), p.sprint()
            Interp(p).run(_At(s, R), s, scratch_reals(p))
            got = s[:R].reshape(hm, n0, n1, n2)
        assert aerror(got, want) < TOL, "split"
        # the same dense volumes through the interleaved guru interface do get the step; two howmany loops do not
        a, b = _arrays(t, hm, fwd, x, n2, False)
        if fwd:
            p = fa.plan_guru64_dft_r2c(dims_r, [(hm, nr, nc)], a, b)
        else:
            p = fa.plan_guru64_dft_c2r(dims_c, [(hm, nc, nr)], a, b)
        assert _has(p), p.sprint()
    if hm > 1:
        # two howmany loops: 2 x (hm + 1) / 2 volumes of a batch extended by one
        hm2 = hm + 1
        x2, want2 = _input(t, hm2, fwd)
        a, b = _arrays(t, hm2, fwd, x2, n2, False)
        with knobs(ON):
            if fwd:
                p = fa.plan_guru64_dft_r2c(dims_r, [(hm2 // 2, 2 * nr, 2 * nc), (2, nr, nc)], a, b)
            else:
                p = fa.plan_guru64_dft_c2r(dims_c, [(hm2 // 2, 2 * nc, 2 * nr), (2, nc, nr)], a, b)
        assert not _has(p) and "vol3d" not in p.sprint(), p.sprint()
        step_interp.run_plan_on_host(p, a, b)
        assert aerror(_result(t, hm2, fwd, b, n2), want2) < TOL, "two howmany loops"


@pytest.mark.parametrize("fwd", [True, False], ids=["r2c", "c2r"])
@pytest.mark.parametrize("shape", [(4, 4, 5), (8, 8, 15), (33, 4, 4), (4, 33, 8), (4, 4, 34), (16, 32, 32), (8, 16), (32, 32),
                                   (2, 4, 4, 4), (3, 8, 8, 8)], ids=_ids)
def test_odd_rows_other_extents_and_other_ranks_are_outside_the_rule(shape, fwd):
    rng = np.random.default_rng(11)
    hm = 3
    n, nl = int(np.prod(shape)), shape[-1]
    hn = n // nl * (nl // 2 + 1)
    if len(shape) == 3:
        assert tile(shape, fwd) == 0
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


def test_wisdom_bit_128_switches_the_step_on():
    t, hm = (4, 8, 16), 7
    n0, n1, n2 = t
    h = n2 // 2 + 1
    x, want = _input(t, hm, True)
    a, b = _arrays(t, hm, True, x, n2, False)
    fa.forget_wisdom()
    try:
        key = "t1 s-1 r3 %d:%d:%d %d:%d:%d %d:1:2 h1 %d:%d:%d i0 o1 p0" % (n0, n1 * n2, 2 * n1 * h, n1, n2, 2 * h, n2, hm,
                                                                          n0 * n1 * n2, 2 * n0 * n1 * h)
        for bits, on in ((128 | 4, True), (4, False), (64 | 32 | 4, False)):
            rec = "(fftw3_amd_wisdom-1\n  (%s) 134217728 0 1024 %d 0.250000\n)\n" % (key, bits)
            assert fa.import_wisdom_from_string(rec) == 1
            assert fa.export_wisdom_to_string() == rec
            p = _plan(t, hm, True, a, b, n2, fa.ESTIMATE | fa.WISDOM_ONLY)   # the key is the problem's
            assert _has(p) == on, (bits, p.sprint())
            b[:] = 0
            run_plan_on_host(p, a, b)
            assert aerror(_result(t, hm, True, b, n2), want) < TOL
            fa.forget_wisdom()
    finally:
        fa.forget_wisdom()
