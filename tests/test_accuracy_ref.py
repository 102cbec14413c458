"""CPU tier of the rms accuracy gate (tests/accuracy.py), no device needed:

- the long-double reference is exact enough: against the committed 80-bit fixtures, a long-double direct sum and
  its own Bluestein path;
- the two double references (the oracle and numpy.fft) pass the gate with the other as the only comparator, for the
  inputs of every case of the GPU matrix (tests/accuracy_cases.py); a case above 2^18 points is replaced by the same
  family at a smaller batch and n (even lengths halved, the 2-D shapes along their longest axis), and the r2r cases
  keep one row of their batch;
- the gate fails wrong code: a double radix-2 FFT whose twiddle table is off by 10 ulp rms fails it at every power of
  two from 1024 to 2^20, and passes it with the exact table, the two-level lo * hi table and the binary-power product;
- the planner's own host tables (twiddle, two-level, chirp, Rader) pass the gate through the step interpreter
  (tests/step_interp.py, numpy.fft for the butterflies) at 2^20, 2^22, 15 375 360, 1031 (Bluestein, step by step
  and as rows), 8191, 65537 and 12289 (Rader: the planner takes Rader for 8191, whose 8190 is 13-smooth), r2c and
  c2r 2^22 and 4096 x 4096.  The interpreter supports all of them.
"""
import os

import numpy as np
import pytest

import accuracy as A
import accuracy_cases as AC
import fftw3_amd as fa
from util import ROOT, crand, oracle_c2r, oracle_dft, oracle_r2c, rrand

A.require_longdouble()

GOLD = os.path.join(ROOT, "tests", "golden")
LD = np.longdouble


def _ulp_check(got, want):
    """every element within 1 ulp of the fixture's largest magnitude"""
    want = np.asarray(want)
    got = np.asarray(got).reshape(want.shape)
    big = max(np.abs(want.real).max(), np.abs(want.imag).max() if np.iscomplexobj(want) else 0.0)
    tol = np.spacing(big)
    d = got.astype(np.clongdouble) - want.astype(np.clongdouble)
    e = max(float(np.abs(d.real).max()), float(np.abs(d.imag).max()))
    assert e <= tol, (e, tol)


def test_against_the_1d_and_2d_fixtures():
    z = np.load(os.path.join(GOLD, "c2c_1d.npz"))
    for k in z.files:
        if k.endswith("_in"):
            x = z[k]
            shape = x.shape[-1:]
            hm = x.size // shape[0]
            for suf, sign in (("_fwd", -1), ("_bwd", +1)):
                if k[:-3] + suf in z.files:
                    _ulp_check(A.ld_dft(x, shape, hm, sign).reshape(z[k[:-3] + suf].shape), z[k[:-3] + suf])
    z = np.load(os.path.join(GOLD, "nd.npz"))
    for k in z.files:
        if k.startswith("c") and k.endswith("_in"):
            x = z[k]
            _ulp_check(A.ld_dft(x, x.shape, 1, -1)[0], z[k[:-3] + "_fwd"])
        if k.startswith("r") and k.endswith("_in"):
            x = z[k]
            y = A.ld_dft(x, x.shape, 1, -1)[0][:, :x.shape[1] // 2 + 1]
            _ulp_check(y, z[k[:-3] + "_out"])


def test_against_the_second_fixture_set():
    z = np.load(os.path.join(GOLD, "pins2.npz"))
    for n in (65537, 12289, 8191, 60060):
        x, bins = z["c%d_in" % n], z["c%d_bins" % n]
        _ulp_check(A.ld_dft(x, (n,), 1, -1)[0][bins], z["c%d_fwd" % n])
        _ulp_check(A.ld_dft(x, (n,), 1, +1)[0][bins], z["c%d_bwd" % n])
    for n in (77, 1001):
        _ulp_check(A.ld_r2c(z["r%d_in" % n], n)[0], z["r%d_out" % n])
    for shape in ((6, 10, 8), (5, 6, 7)):
        key = "x".join(str(s) for s in shape)
        _ulp_check(A.ld_dft(z["c3_%s_in" % key], shape, 1, -1)[0], z["c3_%s_fwd" % key])
        _ulp_check(A.ld_dft(z["r3_%s_in" % key], shape, 1, -1)[0][:, :, :shape[2] // 2 + 1], z["r3_%s_out" % key])
    for n in (16, 15, 1000, 243):
        for kind in range(11):
            _ulp_check(A.ld_r2r(z["k%d_n%d_in" % (kind, n)], kind), z["k%d_n%d_out" % (kind, n)])


def _direct(x, sign):
    n = x.shape[0]
    j = np.arange(n, dtype=np.int64)
    m = (j[:, None] * j[None, :]) % n
    ang = (2 * A.PI) * m.astype(LD) / LD(n)
    W = np.cos(ang) + (1j * sign) * np.sin(ang).astype(np.clongdouble)
    return np.sum(W * x.astype(np.clongdouble)[None, :], axis=1)


@pytest.mark.parametrize("sign", [-1, +1])
def test_against_a_long_double_direct_sum(sign):
    rng = np.random.default_rng(7)
    for n in list(range(1, 70)) + [97, 127, 128, 131, 143, 169, 191, 210, 211, 241, 251, 256]:
        x = crand(rng, n)
        e = A.rms_err(A.ld_dft(x, (n,), 1, sign)[0], _direct(x, sign))
        assert e <= 1e-17, (n, e)


def test_bluestein_against_stockham():
    rng = np.random.default_rng(8)
    for n in (2, 16, 256, 1024, 1 << 14, 1 << 16):
        x = crand(rng, 3, n)
        for sign in (-1, +1):
            e = A.rms_err(A.ld_dft(x, (n,), 3, sign, force_bluestein=True), A.ld_dft(x, (n,), 3, sign))
            assert e <= 1e-17, (n, sign, e)


def test_real_references_are_the_complex_transform():
    rng = np.random.default_rng(9)
    for n in (1, 2, 7, 16, 77, 1000):
        x = rrand(rng, 2, n)
        assert A.rms_err(A.ld_r2c(x, n, 2), A.ld_dft(x, (n,), 2, -1)[:, :n // 2 + 1]) <= 1e-18
        y = A.ld_c2r(A.ld_r2c(x, n, 2), n, 2)
        assert A.rms_err(y, x.astype(LD) * n) <= 1e-17, n
        # c2r ignores the imaginary parts of Y[0] and, for even n, of Y[n / 2]
        Y = A.ld_r2c(x, n, 2).astype(np.clongdouble)
        Y[:, 0] += 0.25j
        if n % 2 == 0:
            Y[:, n // 2] -= 0.5j
        assert A.rms_err(A.ld_c2r(Y, n, 2), x.astype(LD) * n) <= 1e-17, n


def test_the_metric():
    a = np.array([3.0 + 4.0j, 0.0])
    assert A.rms_err(a, a) == 0.0
    assert abs(A.rms_err(a * (1 + 1e-10), a) - 1e-10) < 1e-16      # the double rounding of 1 + 1e-10
    per = A.rms_err_per_transform(np.array([[1.0, 1.0], [2.0, 2.0 + 2e-8]]), np.array([[1.0, 1.0], [2.0, 2.0]]), 2)
    assert per[0] == 0.0 and abs(per[1] - np.sqrt(0.5) * 1e-8) < 1e-16
    assert A.passes(3 * A.U, A.U) and not A.passes(3.01 * A.U, A.U, 0.5 * A.U)
    assert A.passes(1.5 * A.U, 0.0, 0.0) and not A.passes(1.6 * A.U, 0.0)


# ---- the two references against each other, on every case of the GPU matrix

CPU_POINTS = 1 << 18


def _standin(case):
    """the case itself when small enough, else the same family at a smaller n"""
    shape, hm = list(case.shape), case.hm
    while int(np.prod(shape)) * hm > CPU_POINTS and hm > 1:
        hm = max(1, hm // 2) if hm > 2 else 1
    while int(np.prod(shape)) * hm > CPU_POINTS:
        i = int(np.argmax(shape))
        if shape[i] % 2:
            break
        shape[i] //= 2
    if case.kind == "r2r":
        hm = 1                                  # direct O(n^2) sums: one row is enough for the references
    if tuple(shape) == case.shape and hm == case.hm:
        return case
    return AC.Case(case.fam, case.kind, shape, hm, case.sign, r2r=case.r2r)


def _ref_groups():
    seen, out = set(), []
    for c in AC.cases():
        s = _standin(c)
        key = (s.kind, s.shape, s.hm, s.sign, s.r2r)
        if key not in seen:
            seen.add(key)
            out.append(s)
    return out


REF = _ref_groups()


@pytest.mark.parametrize("fam", sorted(set(c.fam for c in REF)))
def test_oracle_and_numpy_pass_the_gate_against_each_other(fam):
    for case in (c for c in REF if c.fam == fam):
        x = AC.make_input(case)
        ld = AC.ref_ld(case, x)
        eo = A.rms_err(AC.ref_oracle(case, x), ld)
        en = A.rms_err(AC.ref_numpy(case, x), ld)
        assert A.passes(eo, en) and A.passes(en, eo), (case.id, eo / A.U, en / A.U)
        assert max(eo, en) < 30 * A.U, (case.id, eo / A.U, en / A.U)


def test_every_r2r_rows_case_plans_as_its_one_step():
    """the 45 (half length, kind) pairs of the one-trip r2r rows kernels: each host plan is the one pinned step"""
    rows = [c for c in AC.cases() if c.fam == "r2r-rows"]
    assert len(set((c.shape, c.r2r) for c in rows)) == len(rows) == 5 * 9
    for c in rows:
        prob = AC._problem(c)
        p = prob.plan(fa, [a.user() for a in prob.arenas()])
        AC.check_plan(c, p)
        AC.check_labels(c, p.sprint())


# ---- the gate separates correct twiddle schemes from subtly wrong ones

def _fft_radix2(x, tw):
    """double radix-2 decimation-in-time FFT of x (n,), twiddles tw[j] ~ exp(-2 pi i j / n), j < n / 2"""
    def rec(v, N):
        B, n = v.shape
        if n == 1:
            return v
        m = n // 2
        S = rec(np.ascontiguousarray(v.reshape(B, m, 2).transpose(0, 2, 1)).reshape(2 * B, m), N).reshape(B, 2, m)
        t = S[:, 1] * tw[np.arange(m) * (N // n)]
        return np.concatenate([S[:, 0] + t, S[:, 0] - t], axis=1)
    return rec(x.reshape(1, -1), x.size)[0]


def _tables(n, rng):
    j = np.arange(n // 2, dtype=np.int64)
    exact_ld = A._roots(n, -1)
    exact = exact_ld[:n // 2].astype(np.complex128)
    s = (n.bit_length() - 1) // 2
    lo = exact_ld[np.arange(1 << s)].astype(np.complex128)
    hi = exact_ld[(np.arange(n >> s) << s) % n].astype(np.complex128)
    two_level = lo[j & ((1 << s) - 1)] * hi[j >> s]
    prod = np.ones(n // 2, dtype=np.complex128)
    for b in range(n.bit_length() - 1):
        wb = exact_ld[(1 << b) % n].astype(np.complex128)
        prod = np.where(j & (1 << b), prod * wb, prod)
    noisy = exact * (1 + 10 * A.U * rng.standard_normal(n // 2))
    return {"exact": exact, "two-level": two_level, "binary-powers": prod, "10u": noisy}


@pytest.mark.parametrize("k", list(range(10, 21)))
def test_gate_fails_a_10_ulp_twiddle_table_and_passes_correct_ones(k):
    n = 1 << k
    rng = np.random.default_rng(k)
    x = crand(rng, n)
    ld = A.ld_dft(x, (n,), 1, -1)[0]
    eo = A.rms_err(oracle_dft(x, (n,)), ld)
    en = A.rms_err(np.fft.fft(x), ld)
    for name, tw in _tables(n, rng).items():
        e = A.rms_err(_fft_radix2(x, tw), ld)
        print(n, name, e / max(eo, en))
        if name == "10u":
            assert not A.passes(e, eo, en), (n, name, e / A.U, eo / A.U, en / A.U)
        else:
            assert A.passes(e, eo, en), (n, name, e / A.U, eo / A.U, en / A.U)


# ---- the planner's host tables through the step interpreter

def _interp_c2c(shape, hm=1, sign=-1):
    from step_interp import Interp, scratch_reals
    n = int(np.prod(shape))
    x = crand(np.random.default_rng(n), hm * n)
    y = np.zeros_like(x)
    p = fa.plan_many_dft(len(shape), list(shape), hm, x, None, 1, n, y, None, 1, n, sign)
    Interp(p).run(x.view(np.float64), y.view(np.float64), scratch_reals(p))
    ld = A.ld_dft(x, shape, hm, sign)
    return p.sprint(), A.rms_err(y, ld), A.rms_err(oracle_dft(x, shape, hm, sign), ld), \
        A.rms_err(AC.ref_numpy(AC.Case("", "c2c", shape, hm, sign), x.reshape((hm,) + tuple(shape))), ld)


# 1031 alone runs the step-by-step Bluestein (chirp multiplies in copy steps), a batch of it the one-kernel rows form;
# 8191 is planned as Rader (8190 = 2 3^2 5 7 13), not Bluestein, and is kept as a third Rader length
@pytest.mark.parametrize("shape,hm,label", [((1 << 20,), 1, "reg32x32"), ((1 << 22,), 1, "reg2"),
                                            ((15375360,), 1, "pass-520"), ((1031,), 1, "copy n=2100"),
                                            ((1031,), 5, "bluestein-rows n=1031"), ((8191,), 1, "rader-mul n=8190"),
                                            ((65537,), 1, "rader-mul"), ((12289,), 1, "rader-mul"),
                                            ((4096, 4096), 1, "dft4-across-rows")],
                         ids=["2^20", "2^22", "15375360", "1031", "1031x5", "8191", "65537", "12289", "4096x4096"])
def test_host_tables_through_the_step_interpreter(shape, hm, label):
    s, e, eo, en = _interp_c2c(shape, hm)
    assert label in s, s
    assert A.passes(e, eo, en), (shape, e / A.U, eo / A.U, en / A.U, s)


def test_host_tables_of_the_real_plans_through_the_step_interpreter():
    from step_interp import Interp, scratch_reals
    n, h = 1 << 22, (1 << 21) + 1
    x = rrand(np.random.default_rng(5), n)
    y = np.zeros(h, dtype=np.complex128)
    p = fa.plan_many_dft_r2c(1, [n], 1, x, None, 1, n, y, None, 1, h)
    assert "r2c-untangle4" in p.sprint(), p.sprint()
    Interp(p).run(x, y.view(np.float64), scratch_reals(p))
    ld = A.ld_r2c(x, n)
    e, eo, en = A.rms_err(y, ld), A.rms_err(oracle_r2c(x, (n,)), ld), A.rms_err(np.fft.rfft(x), ld)
    assert A.passes(e, eo, en), ("r2c", e / A.U, eo / A.U, en / A.U)
    Y = crand(np.random.default_rng(6), h)
    z = np.zeros(n)
    q = fa.plan_many_dft_c2r(1, [n], 1, Y, None, 1, h, z, None, 1, n)
    assert "c2r-tangle4" in q.sprint(), q.sprint()
    Interp(q).run(Y.copy().view(np.float64), z, scratch_reals(q))
    ld = A.ld_c2r(Y, n)
    e = A.rms_err(z, ld)
    eo = A.rms_err(oracle_c2r(Y.copy(), (n,)), ld)
    en = A.rms_err(np.fft.irfft(Y, n, norm="forward"), ld)
    assert A.passes(e, eo, en), ("c2r", e / A.U, eo / A.U, en / A.U)
