"""CPU tier of the two-trip planes plan of rank-3 c2c problems (planner.c emit_vol_planes) and of the one-trip image
step for an extent of 128 (FFTW_AMD_K_IMG2DW, pass2dw.hpp).

With FFTW_AMD_VOL_PLANES=1 (or a wisdom record with bit 512) a dense volume, or a dense batch of volumes, plans as exactly
two steps: one image step over the chunk's n0 planes per volume (the family whose tile query takes (n1, n2)), then one
pass of n0 in place on the output; no scratch buffer.  With FFTW_AMD_IMG_WIDE=1 (bit 1024) batches of 128 x 128, 64 x 128
and 128 x 64 images are the single img2dw step.  The extended numpy interpreter (tests/step_interp_volplanes.py)
computes what the oracle computes, and with neither knob set, or for a layout the rule excludes, the plan is the one
built without the knobs, step description for step description."""
import ctypes

import numpy as np
import pytest

import fftw3_amd as fa
import step_interp
from accuracy_cases import knobs
from step_interp_volplanes import is_planes_step, run_plan_on_host, tile_of
from util import TOL, aerror, crand, oracle_dft

ON = {"FFTW_AMD_VOL_PLANES": "1"}
WIDE_ON = {"FFTW_AMD_IMG_WIDE": "1"}
NAMES = {fa.K_IMG2D: "img2d", fa.K_IMG2DL: "img2dl", fa.K_IMG2DW: "img2dw"}
# (shape, howmany, family of the plane step)
VOLUMES = [((5, 128, 128), 1, fa.K_IMG2DW), ((3, 64, 128), 1, fa.K_IMG2DW), ((3, 128, 64), 3, fa.K_IMG2DW),
           ((8, 64, 64), 2, fa.K_IMG2DL), ((16, 48, 40), 3, fa.K_IMG2DL), ((6, 32, 32), 3, fa.K_IMG2D)]
BIG = [((128, 128, 128), 1, fa.K_IMG2DW), ((128, 128, 128), 3, fa.K_IMG2DW)]
WIDE = [(128, 128), (64, 128), (128, 64)]


def vid(v):
    return "%s-hm%d" % ("x".join(str(n) for n in v[0]), v[1])


def image_label(variant, n0, n1):
    return "pass-%d/%s-%dx%d tile=%d" % (n1, NAMES[variant], n0, n1, tile_of(variant, n0, n1))


def wide_label(n0, n1):
    return image_label(fa.K_IMG2DW, n0, n1)


def descs(p):
    """every field of every step description, as bytes"""
    return [ctypes.string_at(ctypes.addressof(s), ctypes.sizeof(s)) for s in p.steps()]


def same_plan(p, q):
    return p.sprint() == q.sprint() and descs(p) == descs(q) and p.workspace_bytes == q.workspace_bytes


_INPUT = {}


def _input(shape, hm):
    """the same input and oracle results (forward, backward) for every test of one case"""
    key = (shape, hm)
    if key not in _INPUT:
        rng = np.random.default_rng(sum(1000 ** i * n for i, n in enumerate(shape)) + hm)
        x = crand(rng, hm * int(np.prod(shape)))
        _INPUT[key] = (x, {s: oracle_dft(x, shape, hm, s) for s in (-1, +1)})
        for v in _INPUT[key][1].values():
            v.setflags(write=False)
        x.setflags(write=False)
    return _INPUT[key]


def _plan(shape, hm, x, y, sign=fa.FORWARD, flags=fa.ESTIMATE):
    n = int(np.prod(shape))
    return fa.plan_many_dft(len(shape), list(shape), hm, x, None, 1, n, y, None, 1, n, sign, flags)


def _table_bytes(p):
    """what the plan owns besides scratch buffers: 16 bytes per entry of its tables"""
    ids = set()
    for s in p.steps():
        ids |= {t for t in (s.table, s.table2) if t >= 0}
    return sum(16 * (p.table(t).size // 2) for t in ids)


def check_planes_plan(p, shape, hm, variant, sign):
    n0, n1, n2 = shape
    st = p.steps()
    assert len(st) == 2, p.sprint()
    a, b = st
    assert is_planes_step(a) and a.variant == variant, p.sprint()
    assert image_label(variant, n1, n2) in p.sprint(), p.sprint()
    swaps = (fa.F_SWAP_IN | fa.F_SWAP_OUT) if sign == fa.BACKWARD else 0
    assert a.flags & ~(fa.F_NT_IN | fa.F_NT_OUT) == fa.F_LO_DFT | swaps, hex(a.flags)
    assert (a.L, a.is_l, a.os_l, a.tile_lo_n, a.tile_lo_is, a.tile_lo_os) == (n2, 2, 2, n1, 2 * n2, 2 * n2)
    assert a.ndims == 1 and (a.dim_n[0], a.dim_is[0], a.dim_os[0]) == (p.chunk * n0, 2 * n1 * n2, 2 * n1 * n2)
    assert p.batch == p.chunk == hm and a.tile == tile_of(variant, n1, n2) and a.tw_n == 0
    assert (a.src_buf, a.dst_buf, a.src_im, a.dst_im) == (0, 1, 1, 1)
    # one pass of n0, in place on the output, over the n1 n2 contiguous columns and the batch
    assert b.kind == fa.STEP_PASS and b.L == n0 and (b.src_buf, b.dst_buf) == (1, 1), p.sprint()
    assert (b.is_l, b.os_l) == (2 * n1 * n2, 2 * n1 * n2) and b.tw_n == 0 and not (b.flags & fa.F_LO_DFT)
    assert b.flags & (fa.F_SWAP_IN | fa.F_SWAP_OUT) == swaps
    loops = sorted((b.dim_n[i], b.dim_is[i], b.dim_os[i]) for i in range(b.ndims))
    want = [(n1 * n2, 2, 2)] + ([(hm, 2 * n0 * n1 * n2, 2 * n0 * n1 * n2)] if hm > 1 else [])
    assert loops == sorted(want), p.sprint()
    assert "pass-%d/" % n0 in p.sprint().split("\n")[2], p.sprint()
    # no scratch buffer: only the caller's two arrays, and the workspace is the tables
    assert all(s.src_buf < 2 and s.dst_buf < 2 and s.aux_buf < 2 for s in st), p.sprint()
    assert p.workspace_bytes == _table_bytes(p)


@pytest.mark.parametrize("case", VOLUMES + BIG, ids=vid)
def test_planes_plan_is_two_steps_with_the_documented_fields(case):
    shape, hm, variant = case
    n = int(np.prod(shape))
    x = np.zeros(hm * n, dtype=np.complex128)
    y = np.zeros_like(x)
    for sign in (fa.FORWARD, fa.BACKWARD):
        for out in (y, x):
            with knobs(ON):
                p = _plan(shape, hm, x, out, sign)
            check_planes_plan(p, shape, hm, variant, sign)
            off = _plan(shape, hm, x, out, sign)
            assert len(off.steps()) == 3 and not any(is_planes_step(s) for s in off.steps()), off.sprint()


def test_a_large_batch_marks_the_first_read_and_the_last_write_nontemporal():
    shape, hm = (128, 128, 128), 13                    # 416 MiB per side: above the 384 MiB rule
    n = int(np.prod(shape))
    x = np.zeros(hm * n, dtype=np.complex128)
    y = np.zeros_like(x)
    with knobs(ON):
        p = _plan(shape, hm, x, y)
    a, b = p.steps()
    assert (a.flags & fa.F_NT_IN) and not (a.flags & fa.F_NT_OUT), hex(a.flags)
    assert (b.flags & fa.F_NT_OUT) and not (b.flags & fa.F_NT_IN), hex(b.flags)


@pytest.mark.parametrize("case", VOLUMES, ids=vid)
def test_interpreter_matches_the_oracle(case):
    shape, hm, variant = case
    x, want = _input(shape, hm)
    for sign in (fa.FORWARD, fa.BACKWARD):
        y = np.zeros_like(x)
        with knobs(ON):
            p = _plan(shape, hm, x, y, sign)
        check_planes_plan(p, shape, hm, variant, sign)
        run_plan_on_host(p, x, y)
        assert aerror(y, want[sign]) < TOL, (shape, hm, sign)
        z = x.copy()                                   # in place
        with knobs(ON):
            p = _plan(shape, hm, z, z, sign)
        check_planes_plan(p, shape, hm, variant, sign)
        run_plan_on_host(p, z, z)
        assert aerror(z, want[sign]) < TOL, (shape, hm, sign, "in place")


def _misaligned(words):
    w = np.zeros(words + 2)
    w = w[1:] if w.ctypes.data % 16 == 0 else w[:-1]
    assert w.ctypes.data % 16 == 8
    return w[:words]


def _declined(make, why):
    """the plan built with the knob on equals the plan built with it unset"""
    off = make()
    with knobs(ON):
        on = make()
    assert same_plan(on, off), (why, on.sprint(), off.sprint())
    assert not any(is_planes_step(s) for s in on.steps()), (why, on.sprint())
    return on


def test_declined_layouts_keep_the_plan_of_the_axis_loop():
    shape, hm = (8, 64, 64), 4
    n0, n1, n2 = shape
    n = n0 * n1 * n2
    x, want = _input(shape, hm)
    y = np.zeros_like(x)
    with knobs(ON):
        assert is_planes_step(_plan(shape, hm, x, y).steps()[0])

    # a gap between planes
    pl = n1 * n2 + 8
    xg = np.zeros(hm * n0 * pl, dtype=np.complex128)
    xg.reshape(hm, n0, pl)[:, :, :n1 * n2] = x.reshape(hm, n0, n1 * n2)
    yg = np.zeros_like(xg)
    dims = [(n0, pl, pl), (n1, n2, n2), (n2, 1, 1)]
    p = _declined(lambda: fa.plan_guru64_dft(dims, [(hm, n0 * pl, n0 * pl)], xg, yg, fa.FORWARD), "a gap between planes")
    step_interp.run_plan_on_host(p, xg, yg)
    assert aerror(yg.reshape(hm, n0, pl)[:, :, :n1 * n2].reshape(-1), want[-1]) < TOL
    # a gap between volumes
    dist = n + 3
    xv = np.zeros(hm * dist, dtype=np.complex128)
    xv.reshape(hm, dist)[:, :n] = x.reshape(hm, n)
    yv = np.zeros_like(xv)
    p = _declined(lambda: fa.plan_many_dft(3, list(shape), hm, xv, None, 1, dist, yv, None, 1, dist, fa.FORWARD),
                  "a gap between volumes")
    step_interp.run_plan_on_host(p, xv, yv)
    assert aerror(yv.reshape(hm, dist)[:, :n].reshape(-1), want[-1]) < TOL
    # split arrays
    N = hm * n
    s = np.zeros(4 * N)
    s[0:N], s[N:2 * N] = x.real, x.imag
    dense = [(n0, n1 * n2, n1 * n2), (n1, n2, n2), (n2, 1, 1)]
    _declined(lambda: fa.plan_guru64_split_dft(dense, [(hm, n, n)], s[0:N], s[N:2 * N], s[2 * N:3 * N], s[3 * N:],
                                               fa.ESTIMATE), "split arrays")
    # a two-level howmany loop (the same dense volumes through one loop do get the plan)
    with knobs(ON):
        assert is_planes_step(fa.plan_guru64_dft(dense, [(hm, n, n)], x, y, fa.FORWARD).steps()[0])
    p = _declined(lambda: fa.plan_guru64_dft(dense, [(hm // 2, 2 * n, 2 * n), (2, n, n)], x, y, fa.FORWARD),
                  "two howmany loops")
    step_interp.run_plan_on_host(p, x, y)
    assert aerror(y, want[-1]) < TOL
    # FFTW_UNALIGNED, on aligned arrays and on arrays 8 bytes off
    _declined(lambda: _plan(shape, hm, x, y, flags=fa.ESTIMATE | fa.UNALIGNED), "FFTW_UNALIGNED")
    xu, yu = _misaligned(2 * N), _misaligned(2 * N)
    xu[:] = x.view(np.float64)
    p = _declined(lambda: _plan(shape, hm, xu, yu, flags=fa.ESTIMATE | fa.UNALIGNED), "8 bytes off")
    step_interp.run_plan_on_host(p, xu, yu)
    assert aerror(yu.view(np.complex128), want[-1]) < TOL
    # FFTW_AMD_NO_IMG2D and FFTW_AMD_NO_TUNED
    for knob in ("FFTW_AMD_NO_IMG2D", "FFTW_AMD_NO_TUNED"):
        with knobs({knob: "1"}):
            _declined(lambda: _plan(shape, hm, x, y), knob)


@pytest.mark.parametrize("shape", [(1 << 20, 4, 4), (4096, 16, 16), (3000, 16, 16), (4, 96, 96), (4, 128, 32), (4, 256, 128)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_declined_extents_keep_the_plan_of_the_axis_loop(shape):
    """an n0 that needs more than one pass (the planes do have a kernel), and plane pairs without a kernel"""
    x = np.zeros(int(np.prod(shape)), dtype=np.complex128)      # planning touches no element
    if shape[1] <= 32:
        assert tile_of(fa.K_IMG2D, shape[1], shape[2]) > 0
    p = _declined(lambda: _plan(shape, 1, x, x), shape)
    if shape[1] <= 32:
        assert len(p.steps()) > 3, p.sprint()


def test_other_ranks_and_real_problems_are_outside_the_rule():
    x = np.zeros(3 * 64 * 64, dtype=np.complex128)
    y = np.zeros_like(x)
    _declined(lambda: _plan((64, 64), 3, x, y), "rank 2")
    _declined(lambda: _plan((3, 4, 16, 64), 1, x, y), "rank 4")
    r = np.zeros(4 * 32 * 32)
    c = np.zeros(4 * 32 * 17, dtype=np.complex128)
    _declined(lambda: fa.plan_many_dft_r2c(3, [4, 32, 32], 1, r, None, 1, r.size, c, None, 1, c.size, fa.ESTIMATE), "r2c")


def test_tile_queries():
    assert [fa.img2dw_tile(*t) for t in WIDE] == [1, 2, 2]
    for t in [(64, 64), (128, 32), (256, 128), (128, 256), (0, 128), (128, 96), (32, 128)]:
        assert fa.img2dw_tile(*t) == 0, t
    # the three families do not overlap
    for n0 in (16, 32, 64, 128):
        for n1 in (16, 32, 64, 128):
            assert sum(tile_of(v, n0, n1) > 0 for v in NAMES) <= 1, (n0, n1)


@pytest.mark.parametrize("shape", WIDE, ids=lambda s: "%dx%d" % s)
def test_wide_images_are_one_step_and_the_interpreter_matches_the_oracle(shape):
    n0, n1 = shape
    T = fa.img2dw_tile(n0, n1)
    hm = 2 * T + 1
    n = n0 * n1
    x, want = _input(shape, hm)
    for sign in (fa.FORWARD, fa.BACKWARD):
        for inplace in (False, True):
            a = x.copy()
            b = a if inplace else np.zeros_like(a)
            with knobs(WIDE_ON):
                p = _plan(shape, hm, a, b, sign)
            st = p.steps()
            assert len(st) == 1 and wide_label(n0, n1) in p.sprint(), p.sprint()
            assert "img2dw-%dx%d" % shape in p.sprint()
            s = st[0]
            assert s.kind == fa.STEP_PASS and s.variant == fa.K_IMG2DW and s.tile == T and s.batch_dim == 0
            swaps = (fa.F_SWAP_IN | fa.F_SWAP_OUT) if sign == fa.BACKWARD else 0
            assert s.flags & ~(fa.F_NT_IN | fa.F_NT_OUT) == fa.F_LO_DFT | swaps, hex(s.flags)
            assert (s.L, s.is_l, s.os_l, s.tile_lo_n, s.tile_lo_is, s.tile_lo_os) == (n1, 2, 2, n0, 2 * n1, 2 * n1)
            assert s.ndims == 1 and (s.dim_n[0], s.dim_is[0], s.dim_os[0]) == (hm, 2 * n, 2 * n)
            assert s.table >= 0 and s.table2 >= 0 and s.tw_n == 0 and (s.src_buf, s.dst_buf) == (0, 1)
            assert p.workspace_bytes == _table_bytes(p) == 16 * (n0 + n1 if n0 != n1 else n0)
            run_plan_on_host(p, a, b)
            assert aerror(b, want[sign]) < TOL, (shape, sign, inplace)
            # with the knob off -- and with the planes knob on -- the plan is the two-trip one
            off = _plan(shape, hm, a, b, sign)
            assert "img2dw" not in off.sprint() and len(off.steps()) == 2, off.sprint()
            with knobs(ON):
                assert same_plan(_plan(shape, hm, a, b, sign), off)
            off_unaligned = _plan(shape, hm, a, b, sign, flags=fa.ESTIMATE | fa.UNALIGNED)
            with knobs(WIDE_ON):
                for knob in ("FFTW_AMD_NO_IMG2D", "FFTW_AMD_NO_TUNED"):
                    with knobs({knob: "1"}):
                        q = _plan(shape, hm, a, b, sign)
                    assert "img2dw" not in q.sprint(), q.sprint()
                assert same_plan(_plan(shape, hm, a, b, sign, flags=fa.ESTIMATE | fa.UNALIGNED), off_unaligned)


def test_volume_planes_need_only_their_own_knob():
    """FFTW_AMD_VOL_PLANES alone is enough for a volume whose planes need the wide kernel, and FFTW_AMD_IMG_WIDE alone
    changes no rank-3 plan"""
    shape, hm = (3, 64, 128), 1
    x = np.zeros(int(np.prod(shape)), dtype=np.complex128)
    y = np.zeros_like(x)
    off = _plan(shape, hm, x, y)
    with knobs(WIDE_ON):
        assert same_plan(_plan(shape, hm, x, y), off)
    with knobs(ON):
        assert _plan(shape, hm, x, y).steps()[0].variant == fa.K_IMG2DW


def test_wisdom_bits_512_and_1024_switch_the_plans_on():
    fa.forget_wisdom()
    try:
        shape, hm = (8, 64, 64), 2
        n0, n1, n2 = shape
        n = n0 * n1 * n2
        x, want = _input(shape, hm)
        y = np.zeros_like(x)
        key = "t0 s-1 r3 %d:%d:%d %d:%d:%d %d:2:2 h1 %d:%d:%d i1 o1 p0" % (n0, 2 * n1 * n2, 2 * n1 * n2, n1, 2 * n2, 2 * n2,
                                                                           n2, hm, 2 * n, 2 * n)
        for bits, on in ((512 | 4, True), (4, False), (1024 | 64 | 4, False)):
            rec = "(fftw3_amd_wisdom-1\n  (%s) 134217728 0 1024 %d 0.250000\n)\n" % (key, bits)
            assert fa.import_wisdom_from_string(rec) == 1
            assert fa.export_wisdom_to_string() == rec
            p = _plan(shape, hm, x, y, flags=fa.ESTIMATE | fa.WISDOM_ONLY)
            assert is_planes_step(p.steps()[0]) == on, (bits, p.sprint())
            y[:] = 0
            run_plan_on_host(p, x, y)
            assert aerror(y, want[-1]) < TOL
            fa.forget_wisdom()
        shape, hm = (128, 64), 5
        n0, n1 = shape
        n = n0 * n1
        x, want = _input(shape, hm)
        y = np.zeros_like(x)
        key = "t0 s-1 r2 %d:%d:%d %d:2:2 h1 %d:%d:%d i1 o1 p0" % (n0, 2 * n1, 2 * n1, n1, hm, 2 * n, 2 * n)
        for bits, on in ((1024 | 4, True), (4, False), (512 | 4, False)):
            rec = "(fftw3_amd_wisdom-1\n  (%s) 134217728 0 1024 %d 0.250000\n)\n" % (key, bits)
            assert fa.import_wisdom_from_string(rec) == 1
            assert fa.export_wisdom_to_string() == rec
            p = _plan(shape, hm, x, y, flags=fa.ESTIMATE | fa.WISDOM_ONLY)
            assert ("img2dw" in p.sprint()) == on, (bits, p.sprint())
            y[:] = 0
            run_plan_on_host(p, x, y)
            assert aerror(y, want[-1]) < TOL
            fa.forget_wisdom()
    finally:
        fa.forget_wisdom()
