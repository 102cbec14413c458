"""CPU tier of the footprint harness (tests/footprint.py): the checker fails on every planted
violation, footprint() equals what the oracle writes for every layout of the GPU matrix, and the planner's step
lists, run by the step interpreter on NaN-patterned arenas, write only the footprint, preserve the input out of
place and read nothing but the input."""
import numpy as np
import pytest

import fftw3_amd as fa
import accuracy as A
import accuracy_cases as AC
import footprint as F
import footprint_cases as FC
from step_interp import Interp, scratch_reals
from util import TOL, aerror

CASES = FC.cases()


# ---- the checker against planted violations

def _numpy_executor(prob, AR, plant=None):
    """a correct strided c2c transform on the arenas (numpy.fft on the gathered input, scattered to the output
    footprint), then one planted fault"""
    x = prob.gather_in([a.user() for a in prob.in_arenas(AR)])
    y = np.fft.fft(x, axis=1)
    out = prob.out_arenas(AR)[0]
    w = F.word_offsets(prob.out_elems, prob.out_side)
    out.put(w[..., 0].reshape(-1), y.real.reshape(-1))
    out.put(w[..., 1].reshape(-1), y.imag.reshape(-1))
    if plant:
        plant(AR)


def _self_test_problem(layout):
    c = FC.FCase("self", "c2c", (12,), 5, layout)
    return c, c.problem()


def _run_planted(layout, plant):
    c, prob = _self_test_problem(layout)
    AR = prob.arenas()
    x = AC.make_input(c)
    prob.scatter(AR, x)
    before = [a.snapshot() for a in AR]
    _numpy_executor(prob, AR, plant)
    viol = [F.check(b, a.words, w) for b, a, w in zip(before, AR, prob.written(AR))]
    got = prob.gather([a.user() for a in prob.out_arenas(AR)])
    return prob, AR, viol, got, np.fft.fft(x, axis=1)


@pytest.mark.parametrize("layout", ["dense", "gapped", "strided", "sparecol", "rows2cols", "gapped-inplace"])
def test_checker_is_clean_on_a_correct_executor(layout):
    prob, AR, viol, got, want = _run_planted(layout, None)
    assert not any(viol), viol
    assert aerror(got, want) < TOL


def test_checker_reports_each_planted_violation_at_its_offset():
    def expect(layout, plant, arena, offset):
        prob, AR, viol, got, want = _run_planted(layout, plant)
        assert [v.count for v in viol] == [1 if i == arena else 0 for i in range(len(AR))], (layout, viol)
        assert viol[arena].first == [offset], (viol, offset)

    # one extra element after the last row (dense: the first word past the span)
    c, prob = _self_test_problem("dense")
    end = int(prob.out_fp.max()) + 1
    lo = prob.arenas()[1].lo
    expect("dense", lambda AR: AR[1].put([end], [1.0]), 1, lo + end)
    # one into a stride gap of the output (strided: ostride 2, complex word 2 is in the gap)
    expect("strided", lambda AR: AR[1].put([2], [1.0]), 1, lo + 2)
    # one into the spare interleaved column (sparecol: stride hm + 2, columns hm and hm + 1 are spare)
    expect("sparecol", lambda AR: AR[1].put([2 * 5 + 1], [0.5]), 1, lo + 11)
    # one into the lower guard
    expect("dense", lambda AR: AR[1].put([-3], [0.0]), 1, lo - 3)
    # one input word changed, out of place
    expect("gapped", lambda AR: AR[0].put([4], [AR[0].get([4])[0] + 1.0]), 0, lo + 4)
    # a guard word overwritten with another guard word's pattern
    def copy_guard(AR):
        AR[1].words[7] = AR[1].words[8]
    expect("dense", copy_guard, 1, 7)


def test_an_output_taken_from_a_gap_fails_the_value_check():
    def plant(AR):                      # output element 3 of row 1 <- a word of the input's gap
        gap = AR[0].get([2 * 12 + 1])   # gapped: idist = n + 3, complex element 12 of row 0 is a gap
        AR[1].put([2 * ((12 + 5) + 3)], gap)
    prob, AR, viol, got, want = _run_planted("gapped", plant)
    assert not any(viol)                # the write itself is inside the footprint
    assert np.isnan(got[1, 3].real) and np.isnan(got).sum() == 1
    with pytest.raises(AssertionError):
        A.rms_err(got, want)


# ---- footprint() against the oracle

def _oracle_cases():
    seen, out = set(), []
    for c in CASES:
        key = (c.kind, c.shape, c.hm, c.layout, c.r2r, tuple(c.kinds or ()))
        if c.layout.startswith("split") or c.sign > 0 or key in seen:
            continue
        seen.add(key)
        out.append(c)
    return out


def test_footprint_equals_what_the_oracle_writes():
    """every layout of the GPU matrix (split planes excepted: the oracle has no split interface): the words the
    oracle changes in a NaN-patterned arena are exactly footprint()"""
    cases = _oracle_cases()
    assert len(cases) > 150
    for c in cases:
        prob = c.problem()
        AR = prob.arenas()
        prob.scatter(AR, FC.make_input(c))
        before = [a.snapshot() for a in AR]
        prob.oracle(AR)
        out = prob.out_arenas(AR)[0]
        changed = np.flatnonzero(out.words != before[-1]) - out.lo
        if prob.inplace:
            union = np.union1d(prob.in_fp, prob.out_fp)
            assert np.all(np.isin(prob.out_fp, changed)) and np.all(np.isin(changed, union)), c.id
        else:
            assert np.array_equal(changed, prob.out_fp), (c.id, changed[:8], prob.out_fp[:8])
        assert not np.isnan(prob.gather([out.user()])).any(), c.id


# ---- the c2c families stay reached by a non-dense layout

def _plan_on_host(c):
    prob = c.problem()
    with AC.knobs(c.env):
        return prob.plan(fa, [a.user() for a in prob.arenas()]).sprint()


def test_every_c2c_family_is_reached_by_a_non_dense_case():
    reached = FC.family_labels(_plan_on_host)
    for f, cid in sorted(reached.items()):
        print("%-24s %s" % (f, cid))
    assert sorted(reached) == sorted(FC.FAMILIES), sorted(set(FC.FAMILIES) - set(reached))


def test_every_r2r_rows_step_is_reached_by_a_non_dense_case():
    reached = FC.r2r_rows_steps(_plan_on_host)
    for lab, cid in sorted(reached.items()):
        print("%-32s %s" % (lab, cid))
    assert sorted(reached) == sorted(FC.R2R_ROWS_STEPS), sorted(set(FC.R2R_ROWS_STEPS) - set(reached))


def test_case_ids_are_unique_and_references_are_shared():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids)) and len(ids) >= 300
    # cases of one (kind, shape, hm, sign, r2r) are adjacent: the long-double reference cache holds 5 entries
    keys = [(c.kind, c.shape, c.hm, c.sign, c.r2r) for c in CASES]
    runs = 1 + sum(1 for a, b in zip(keys, keys[1:]) if a != b)
    assert runs == len(set(keys)), (runs, len(set(keys)))


# ---- the planner's step lists on arenas

def _interp(plan, prob, arrays, AR, store):
    it = Interp(plan)
    if prob.split:
        f = store.view(np.float64)
        ins, outs = prob.in_arenas(AR), prob.out_arenas(AR)
        it.run(f[ins[0].base + ins[0].lo:], f[outs[0].base + outs[0].lo:], scratch_reals(plan))
    elif prob.inplace:
        it.run(arrays[0], arrays[0], scratch_reals(plan))
    else:
        it.run(arrays[0], arrays[1], scratch_reals(plan))


def _sweep():
    """a seeded sweep of small problems: ranks 1 ... 3, prime factors up to 31 plus Bluestein and Rader lengths, the
    four kinds, the layouts of the GPU matrix, in and out of place"""
    rng = np.random.default_rng(20260501)
    smooth = [n for n in range(2, 400) if max(A._factors(n)) <= 31]
    hard = [37, 41, 67, 74, 97, 101, 131, 257, 331]          # Rader / Bluestein
    c2c_l = ["dense", "gapped", "strided", "sparecol", "rows2cols", "dense-inplace", "gapped-inplace",
             "sparecol-inplace", "split1", "split2", "split-gapped", "unaligned"]
    real_l = ["dense", "padded-inplace", "gapped", "realstride2", "cplxstride3", "sparecol"]
    r2r_l = ["gapped", "strided", "sparecol", "gapped-inplace", "dense"]
    out = []
    for i in range(340):
        kind = ("c2c", "r2c", "c2r", "r2r")[i % 4]
        rank = 1 if i % 5 else int(rng.integers(2, 4))
        hm = int(rng.integers(1, 8))
        if rank == 1:
            n = int(rng.choice(hard)) if i % 9 == 0 else int(rng.choice(smooth))
            lay = {"c2c": c2c_l, "r2r": r2r_l}.get(kind, real_l)
            name = lay[int(rng.integers(len(lay)))]
            kw = {}
            if kind == "r2r":
                kw["r2r"] = int(rng.integers(11))
                if kw["r2r"] == 3 and n < 2:
                    n = 2
            if name == "unaligned":
                kw["flags"] = FC.UNALIGNED
            if kind == "c2c" and not name.startswith("split") and rng.integers(2):
                kw["sign"] = +1
            out.append(FC.FCase("sweep", kind, (n,), hm, name, **kw))
        else:
            shape = tuple(int(rng.choice([2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 16, 17, 20, 31])) for _ in range(rank))
            kw = {}
            if kind == "r2r":
                kw["kinds"] = [int(rng.integers(11)) for _ in range(rank)]
                shape = tuple(max(s, 2) for s in shape)
            out.append(FC.FCase("sweep", kind, shape, hm, "embedded" if rng.integers(2) else "dense", **kw))
    return out


def _oracle_result(c, x):
    """the oracle on the same layout, into arenas of its own"""
    prob = c.problem()
    if prob.split:
        return np.fft.fft(x, axis=1)
    AR = prob.arenas()
    prob.scatter(AR, x)
    prob.oracle(AR)
    return prob.gather([prob.out_arenas(AR)[0].user()])


def _sweep_input(c):
    rng = np.random.default_rng(AC._seed(c.id))
    prob = c.problem()
    shape = prob.in_elems.shape
    if prob.in_side in ("real", "r2r"):
        return rng.random(shape) - 0.5
    return (rng.random(shape) - 0.5) + 1j * (rng.random(shape) - 0.5)


def test_step_lists_write_only_the_footprint_and_preserve_the_input():
    sweep = _sweep()
    assert len(sweep) >= 300
    seen = set()
    for c in sweep:
        x = _sweep_input(c)
        r = FC.run(c, x, execute=_interp)
        seen.add((c.kind, len(c.shape), c.layout))
        assert not any(r.violations), (c.id, r.violations, r.sprint)
        assert aerror(r.got, _oracle_result(c, x)) < TOL, (c.id, r.sprint)
        if not c.problem().inplace:
            assert r.preserved, (c.id, r.sprint)
            assert all(dst != 0 for _, dst in r.plan_steps), (c.id, r.sprint)
        assert r.repeat, c.id
    assert {k for k, _, _ in seen} == {"c2c", "r2c", "c2r", "r2r"} and {r for _, r, _ in seen} == {1, 2, 3}


def test_r2r_rows_cases_write_only_the_footprint_through_the_step_interpreter():
    """the r2r-rows cases of the GPU matrix, pinned steps and tiles included, through the step interpreter"""
    rows = [c for c in CASES if c.fam.startswith("r2r-rows")]
    assert len(rows) == 2 * 8 * 6 + 2
    for c in rows:
        x = FC.make_input(c)
        r = FC.run(c, x, execute=_interp)
        AC.check_labels(c, r.sprint)
        assert not any(r.violations), (c.id, r.violations, r.sprint)
        assert aerror(r.got, _oracle_result(c, x)) < TOL, (c.id, r.sprint)
        if not c.problem().inplace:
            assert r.preserved, (c.id, r.sprint)
        assert r.repeat, c.id


def test_arena_layout():
    a = F.Arena(1000, np.float64, 100)
    assert a.guard == F.GUARD_MIN and a.lo == a.guard and a.size == 1000 + 2 * a.guard
    b = F.Arena(10, np.complex128, 70000, offset=1)
    assert b.guard == 70144 and b.guard % 512 == 0 and b.lo == b.guard + 1
    assert np.isnan(b.f64).all() and len(np.unique(b.words)) == b.size
    assert int(b.words[5]) == 0x7FF8000000000005
