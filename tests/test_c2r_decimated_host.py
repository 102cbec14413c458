"""Host logic of the two-trip c2r plan (emit_c2r_decimated in fftw3_amd/csrc/planner.c): the step list, the plan's
arithmetic under the numpy interpreter (tests/step_interp_c2r.py), where it is NOT planned, and wisdom."""
import numpy as np
import pytest

import fftw3_amd as fa
from step_interp_c2r import run_plan_on_host
from util import oracle_r2c, oracle_c2r, aerror, rrand, TOL

N, B = 2048 * 256, 3


@pytest.fixture(scope="module")
def problem():
    """real rows, their half spectra and the c2r of those (= n x), computed once"""
    rng = np.random.default_rng(17)
    xr = rrand(rng, B, N)
    spec = oracle_r2c(xr, (N,), B).reshape(B, N // 2 + 1)
    back = oracle_c2r(spec, (N,), B).reshape(B, N)
    for a in (xr, spec, back):
        a.setflags(write=False)
    return xr, spec, back


def _plan(y, z, n=N, b=B, flags=fa.ESTIMATE):
    return fa.plan_many_dft_c2r(1, [n], b, y, None, 1, n // 2 + 1, z, None, 1, n, flags)


def test_two_steps_and_their_description(monkeypatch):
    y, z = np.zeros((B, N // 2 + 1), dtype=complex), np.zeros((B, N))
    monkeypatch.setenv("FFTW_AMD_REAL_DEC", "1")
    p = _plan(y, z)
    st = p.steps()
    assert len(st) == 2 and "reg3+c2r-decimated" in p.sprint(), p.sprint()
    assert "real-decimated" not in p.sprint()
    s0, s1 = st
    assert s0.kind == fa.STEP_PASS and (s0.flags & fa.F_REAL_DEC_C2R) and not (s0.flags & (fa.F_REAL_DEC | fa.F_TW_IN))
    assert s0.L == 2048 and s0.dim_n[0] == 256 // 2 + 1 and s0.dim_tw[0] == 1 and s0.tile == 8 and s0.tw_n == N
    assert s0.src_buf == 0 and s0.dst_buf >= 2 and s0.dim_is[0] == 2 and s0.is_l == 2 * 256
    assert s1.kind == fa.STEP_PASS and s1.L == 256 and s1.tw_n == 0 and s1.variant != 0          # a register kernel
    assert not (s1.flags & (fa.F_REAL_DEC | fa.F_REAL_DEC_C2R)) and s1.src_buf == s0.dst_buf and s1.dst_buf == 1


def test_interpreted_plan_out_of_place(problem, monkeypatch):
    xr, spec, back = problem
    monkeypatch.setenv("FFTW_AMD_REAL_DEC", "1")
    y = spec.copy()
    y[:, 0] += 0.25j                       # the imaginary parts of X[0] and X[n / 2] are ignored
    y[:, N // 2] -= 0.5j
    keep = y.copy()
    z = np.zeros((B, N))
    p = _plan(y, z)
    assert "c2r-decimated" in p.sprint()
    run_plan_on_host(p, y, z)
    assert aerror(z, back) < TOL
    assert np.array_equal(y, keep)         # the plan never writes its input


def test_interpreted_plan_in_place_padded(problem, monkeypatch):
    xr, spec, back = problem
    monkeypatch.setenv("FFTW_AMD_REAL_DEC", "1")
    pad = np.zeros((B, N + 2))
    pad.reshape(B, N // 2 + 1, 2)[..., 0] = spec.real
    pad.reshape(B, N // 2 + 1, 2)[..., 1] = spec.imag
    q = fa.plan_many_dft_c2r(1, [N], B, pad, None, 1, N // 2 + 1, pad, None, 1, N + 2)
    assert len(q.steps()) == 2 and "c2r-decimated" in q.sprint(), q.sprint()
    run_plan_on_host(q, pad, pad)
    assert aerror(pad[:, :N], back) < TOL


def test_not_planned_by_default_unaligned_other_lengths_or_r2r(monkeypatch):
    y, z = np.zeros((B, N // 2 + 1), dtype=complex), np.zeros((B, N))
    assert "c2r-decimated" not in _plan(y, z).sprint()
    monkeypatch.setenv("FFTW_AMD_REAL_DEC", "1")
    assert "c2r-decimated" in _plan(y, z).sprint()
    assert "c2r-decimated" not in _plan(y, z, flags=fa.ESTIMATE | fa.UNALIGNED).sprint()
    m = 2000 * 300
    assert "c2r-decimated" not in _plan(np.zeros((B, m // 2 + 1), dtype=complex), np.zeros((B, m)), n=m).sprint()
    # an r2r problem whose inner transform is a c2r keeps its plan
    h = np.zeros((B, N))
    r = fa.plan_many_r2r(1, [N], B, h, None, 1, N, z, None, 1, N, [fa.HC2R])
    assert "decimated" not in r.sprint(), r.sprint()


def test_r2c_plan_of_the_same_length_is_unchanged(monkeypatch):
    xr, y = np.zeros((B, N)), np.zeros((B, N // 2 + 1), dtype=complex)
    monkeypatch.setenv("FFTW_AMD_REAL_DEC", "1")
    p = fa.plan_many_dft_r2c(1, [N], B, xr, None, 1, N, y, None, 1, N // 2 + 1)
    st = p.steps()
    assert len(st) == 2 and "reg3+real-decimated" in p.sprint() and "c2r-decimated" not in p.sprint(), p.sprint()
    assert st[0].L == 256 and st[0].flags & (fa.F_REAL_DEC | fa.F_REAL_DEC_C2R) == 0
    assert (st[1].flags & fa.F_REAL_DEC) and (st[1].flags & fa.F_TW_IN) and not (st[1].flags & fa.F_REAL_DEC_C2R)
    assert st[1].L == 2048 and st[1].dim_n[0] == 129 and st[1].tile == 8


def test_round_trip_r2c_then_c2r_decimated(problem, monkeypatch):
    xr, spec, back = problem
    monkeypatch.setenv("FFTW_AMD_REAL_DEC", "1")
    x = xr.copy()
    y = np.zeros((B, N // 2 + 1), dtype=complex)
    z = np.zeros((B, N))
    f = fa.plan_many_dft_r2c(1, [N], B, x, None, 1, N, y, None, 1, N // 2 + 1)
    g = _plan(y, z)
    assert "real-decimated" in f.sprint() and "c2r-decimated" in g.sprint()
    run_plan_on_host(f, x, y)
    run_plan_on_host(g, y, z)
    assert aerror(z, N * xr) < TOL


def test_wisdom_remembers_the_two_trip_c2r_plan():
    """bit 16 of the flags word of a c2r entry: export -> forget -> import reproduces the two-step plan"""
    fa.forget_wisdom()
    try:
        y, z = np.zeros((B, N // 2 + 1), dtype=complex), np.zeros((B, N))
        key = "t2 s1 r1 %d:2:1 h1 %d:%d:%d i1 o0 p0" % (N, B, N + 2, N)
        rec = "(fftw3_amd_wisdom-1\n  (%s) 134217728 0 1024 21 0.500000\n)\n" % key      # 21 = small tiles, 2 lanes, real_dec
        assert fa.import_wisdom_from_string(rec) == 1
        p = _plan(y, z, flags=fa.ESTIMATE | fa.WISDOM_ONLY)
        assert len(p.steps()) == 2 and "reg3+c2r-decimated" in p.sprint(), p.sprint()
        text = fa.export_wisdom_to_string()
        assert key in text and "134217728 0 1024 21" in text
        fa.forget_wisdom()
        with pytest.raises(ValueError):
            _plan(y, z, flags=fa.ESTIMATE | fa.WISDOM_ONLY)
        assert "c2r-decimated" not in _plan(y, z).sprint()
        assert fa.import_wisdom_from_string(text) == 1
        q = _plan(y, z, flags=fa.ESTIMATE | fa.WISDOM_ONLY)
        assert len(q.steps()) == 2 and "reg3+c2r-decimated" in q.sprint(), q.sprint()
    finally:
        fa.forget_wisdom()
