"""CPU tier of the transposition path of the plan layer: rank-0 guru plans with exchanged strides (how FFTW callers
transpose) and in-place transforms with transposed output.  The planner's step lists are checked for the kernel they
name (FFTW_AMD_STEP_COPY of variant FFTW_AMD_K_TRANSPOSE, transpose.hpp), for their scratch, and run under the numpy
step interpreter, whose COPY gathers everything before it stores anything -- exactly what the in-place kernel
guarantees.  Transpositions move data and compute nothing: every comparison is np.array_equal."""
import numpy as np
import pytest

import fftw3_amd as fa
from step_interp import Interp, run_plan_on_host, scratch_reals
from transpose_cases import NONSQUARE, SQUARE_N, Case, is_transpose_step
from util import TOL, aerror, crand, oracle_dft, rrand

rng = np.random.default_rng(23)


def _fill(case, span):
    """an array of `span` words of random data (gaps included, so that a gap that moves shows)"""
    return rrand(rng, span)


def _want(case, x):
    """the output words the definition gives, as [b][r][c][t][word]"""
    return x[case.in_words()]


def test_r2r_inplace_with_different_locations_is_rejected():
    """fftw_mkproblem_rdft: an in-place problem must address the same locations on both sides
    (fftw_tensor_inplace_locations); the c2c constructor had the rule, the r2r one did not"""
    x = np.zeros(16)
    with pytest.raises(ValueError):
        fa.plan_guru64_r2r([], [(8, 1, 2)], x, x, [])
    with pytest.raises(ValueError):
        fa.plan_guru64_r2r([], [(4, 1, 3), (3, 1, 4)], x, x, [])
    # identical strides on both sides are never asked the question, mirrored ones included (as before)
    p = fa.plan_guru64_r2r([], [(8, -1, -1)], fa.ptr(x) + 8 * 7, fa.ptr(x) + 8 * 7, [])
    p._keep = (x,)
    assert len(p.steps()) == 1 and p.steps()[0].variant != fa.K_TRANSPOSE
    # the same loops on two arrays stay legal
    fa.plan_guru64_r2r([], [(8, 1, 2)], x, np.zeros(16), [])


@pytest.mark.parametrize("kind", ["r2r", "c2c"])
@pytest.mark.parametrize("n", SQUARE_N)
def test_inplace_square_is_one_step_without_scratch(kind, n):
    for ld in (n, n + 3):
        for batch in (1, 3):
            c = Case(kind, n, n, ld, ld, batch, inplace=True)
            x = _fill(c, c.span_in())
            x0 = x.copy()
            p = c.plan(x, x)
            st = p.steps()
            assert len(st) == 1, (c, p.sprint())
            assert st[0].kind == fa.STEP_COPY and st[0].variant == fa.K_TRANSPOSE, (c, p.sprint())
            assert st[0].flags & fa.F_PAIR_SWAP
            assert p.workspace_bytes == 0, c
            assert "transpose-inplace" in p.sprint()
            run_plan_on_host(p, x, x)
            want = x0.copy()
            want[c.out_words()] = _want(c, x0)
            assert np.array_equal(x, want), c            # the transpose, and the leading-dimension gaps untouched
            v = x[:batch * n * ld * c.words].reshape(batch, n, ld, c.words)[:, :, :n]
            v0 = x0[:batch * n * ld * c.words].reshape(batch, n, ld, c.words)[:, :, :n]
            assert np.array_equal(v, v0.transpose(0, 2, 1, 3)), c
            run_plan_on_host(p, x, x)
            assert np.array_equal(x, x0), c              # twice = identity


@pytest.mark.parametrize("shape", NONSQUARE)
def test_inplace_nonsquare_r2r_goes_through_scratch_in_one_chunk(shape):
    """the parent planned these as ONE element-wise copy of the array onto itself: a data race between workgroups
    that the gather-then-store interpreter cannot see.  Now: dense scratch image, one chunk, like via_scratch of c2c"""
    n0, n1 = shape
    for batch in (1, 3):
        c = Case("r2r", n0, n1, batch=batch, inplace=True)
        x = _fill(c, c.span_in())
        x0 = x.copy()
        p = c.plan(x, x)
        st = p.steps()
        assert p.batch == p.chunk, c
        assert st[0].dst_buf >= 2 and st[-1].src_buf >= 2 and st[-1].dst_buf == 1, (c, p.sprint())
        assert all(s.dst_buf != 1 for s in st[:-1])
        if min(n0, n1) > 1:
            assert sum(is_transpose_step(s) for s in st) == 1, (c, p.sprint())   # the transposing half is tiled
        if min(n0, n1) > 1 or batch > 1:
            # the plain half carries the contiguous run as the copy's OWN index (aux_n elements of unit stride on both
            # sides, a workgroup of copy_kernel then takes 256 neighbours), the rest as loops: whole rows at least,
            # and index times loops is every element once.  (A lone loop is the plan's batch loop and stays a loop.)
            plain = [s for s in st if not is_transpose_step(s)]
            assert len(plain) == len(st) - (1 if min(n0, n1) > 1 else 0)
            for s in plain:
                assert s.kind == fa.STEP_COPY and not s.flags & fa.F_PAIR_SWAP, (c, p.sprint())
                assert s.is_l == 1 and s.os_l == 1 and s.aux_n == s.aux_valid, (c, p.sprint())
                assert s.aux_n >= max(n1, 2) and s.aux_n % n1 == 0, (c, p.sprint())
                assert s.aux_n * int(np.prod(list(s.dim_n[:s.ndims]))) == batch * n0 * n1, (c, p.sprint())
                assert list(s.dim_is[:s.ndims]) == list(s.dim_os[:s.ndims]), (c, p.sprint())
        run_plan_on_host(p, x, x)
        assert np.array_equal(x.reshape(batch, n1, n0), x0.reshape(batch, n0, n1).transpose(0, 2, 1)), c


@pytest.mark.parametrize("kind", ["r2r", "c2c"])
@pytest.mark.parametrize("shape", NONSQUARE + ((32, 32), (65, 65)))
def test_out_of_place_is_one_tiled_step(kind, shape):
    n0, n1 = shape
    for vl, batch, pad in ((1, 1, 0), (3, 1, 0), (3, 3, 3), (1, 3, 3), (2, 2, 1)):
        c = Case(kind, n0, n1, n1 + pad, n0 + pad, batch, vl)
        x = _fill(c, c.span_in())
        x0 = x.copy()
        y = _fill(c, c.span_out())
        y0 = y.copy()
        p = c.plan(x, y)
        st = p.steps()
        assert len(st) == 1 and is_transpose_step(st[0]) and not (st[0].flags & fa.F_PAIR_SWAP), (c, p.sprint())
        assert p.workspace_bytes == 0
        assert "(transpose " in p.sprint()
        run_plan_on_host(p, x, y)
        want = y0.copy()
        want[c.out_words()] = _want(c, x0)
        assert np.array_equal(y, want), c
        assert np.array_equal(x, x0)


def test_c2c_inplace_nonsquare_keeps_scratch_with_a_tiled_half():
    for n0, n1 in NONSQUARE:
        x = crand(rng, n0 * n1)
        x0 = x.copy()
        p = fa.plan_guru64_dft([], [(n0, n1, 1), (n1, 1, n0)], x, x, fa.FORWARD)
        st = p.steps()
        assert p.batch == p.chunk
        if min(n0, n1) > 1:       # (a 1 x 40 matrix has the same strides on both sides once its extent-1 loop is gone)
            assert st[0].dst_buf >= 2 and st[-1].dst_buf == 1
            assert sum(is_transpose_step(s) for s in st) == 1, p.sprint()
        run_plan_on_host(p, x, x)
        assert np.array_equal(x.reshape(n1, n0), x0.reshape(n0, n1).T)


@pytest.mark.parametrize("n", [64, 1024])
def test_square_transposed_output_inplace_transform_needs_no_extra_scratch(n):
    """[(n, 1, v)], [(v, n, 1)] with n == v (the reference's dft-ct-dif + q1 case): the ordinary in-place rows plan
    in one chunk, then the in-place square step"""
    v = n
    x = crand(rng, n * v)
    x0 = x.copy()
    p = fa.plan_guru64_dft([(n, 1, v)], [(v, n, 1)], x, x, fa.FORWARD)
    rows = fa.plan_many_dft(1, [n], v, x, None, 1, n, x, None, 1, n, fa.FORWARD)
    st = p.steps()
    assert p.batch == p.chunk
    assert is_transpose_step(st[-1]) and (st[-1].flags & fa.F_PAIR_SWAP), p.sprint()
    assert not any(is_transpose_step(s) for s in st[:-1])
    assert len(st) == len(rows.steps()) + 1
    assert p.workspace_bytes <= rows.workspace_bytes, (p.workspace_bytes, rows.workspace_bytes)
    run_plan_on_host(p, x, x)
    want = oracle_dft(x0.reshape(1, -1), (n,), v).reshape(v, n).T.reshape(-1)
    assert aerror(x, want) < TOL


class _At(object):
    """a flat float64 array addressed from word `base` (the pointer the planner was given), for layouts with
    negative strides"""

    def __init__(self, a, base):
        self.a, self.base = a, base

    def __getitem__(self, i):
        return self.a[np.asarray(i) + self.base]

    def __setitem__(self, i, v):
        self.a[np.asarray(i) + self.base] = v


def test_excluded_layouts_plan_as_before():
    n0, n1 = 12, 20
    # negative stride: the columns of the source are read backwards
    x = rrand(rng, n0 * n1)
    y = np.zeros(n0 * n1)
    p = fa.plan_guru64_r2r([], [(n0, n1, 1), (n1, -1, n0)], fa.ptr(x) + 8 * (n1 - 1), y, [])
    p._keep = (x, y)
    assert not any(is_transpose_step(s) for s in p.steps()), p.sprint()
    Interp(p).run(_At(x, n1 - 1), y, scratch_reals(p))
    assert np.array_equal(y.reshape(n1, n0), x.reshape(n0, n1)[:, ::-1].T)
    xc = crand(rng, n0 * n1)
    yc = np.zeros(n0 * n1, dtype=np.complex128)
    p = fa.plan_guru64_dft([], [(n0, n1, 1), (n1, -1, n0)], fa.ptr(xc) + 16 * (n1 - 1), yc, fa.FORWARD)
    p._keep = (xc, yc)
    assert not any(is_transpose_step(s) for s in p.steps()), p.sprint()
    Interp(p).run(_At(xc.view(np.float64), 2 * (n1 - 1)), yc.view(np.float64), scratch_reals(p))
    assert np.array_equal(yc.reshape(n1, n0), xc.reshape(n0, n1)[:, ::-1].T)
    # split-complex planes (one allocation: the interpreter addresses the imaginary plane from the real one)
    N = n0 * n1
    s = rrand(rng, 4 * N)
    s0 = s.copy()
    p = fa.plan_guru64_split_dft([], [(n0, n1, 1), (n1, 1, n0)], s[0:N], s[N:2 * N], s[2 * N:3 * N], s[3 * N:], fa.ESTIMATE)
    assert not any(is_transpose_step(t) for t in p.steps()), p.sprint()
    it = Interp(p)
    it.run(s, _At(s, 2 * N), scratch_reals(p))
    assert np.array_equal(s[2 * N:3 * N].reshape(n1, n0), s0[0:N].reshape(n0, n1).T)
    assert np.array_equal(s[3 * N:].reshape(n1, n0), s0[N:2 * N].reshape(n0, n1).T)
    # a complex array 8 bytes off 16-byte alignment under FFTW_UNALIGNED
    w = rrand(rng, 2 * N + 2)
    w = w[1:] if w.ctypes.data % 16 == 0 else w[:-1]
    assert w.ctypes.data % 16 == 8
    w = w[:2 * N]
    yc = np.zeros(N, dtype=np.complex128)
    p = fa.plan_guru64_dft([], [(n0, n1, 1), (n1, 1, n0)], w, yc, fa.FORWARD, fa.ESTIMATE | fa.UNALIGNED)
    assert not any(is_transpose_step(t) for t in p.steps()), p.sprint()
    run_plan_on_host(p, w, yc)
    assert np.array_equal(yc.reshape(n1, n0), w.view(np.complex128).reshape(n0, n1).T)
    # more than two permuted loops
    a, b, c = 4, 5, 6
    x = rrand(rng, a * b * c)
    y = np.zeros(a * b * c)
    p = fa.plan_guru64_r2r([], [(a, b * c, 1), (b, c, a), (c, 1, a * b)], x, y, [])
    assert not any(is_transpose_step(t) for t in p.steps()), p.sprint()
    run_plan_on_host(p, x, y)
    assert np.array_equal(y.reshape(c, b, a), x.reshape(a, b, c).transpose(2, 1, 0))
