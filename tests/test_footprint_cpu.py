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
from step_interp_c2r import InterpC2R
from step_interp_img2dr import InterpImg2DR
from step_interp_vol3d import InterpVol3D
from step_interp_vol3dr import InterpVol3DR
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
        if c.layout.startswith("split") or c.layout in FC.GURU_ONLY or c.sign > 0 or key in seen:
            continue
        seen.add(key)
        out.append(c)
    return out


def test_footprint_equals_what_the_oracle_writes():
    """every layout of the GPU matrix (split planes and the guru-only layouts excepted: the oracle has neither
    interface; test_guru_footprints_equal_a_nested_loop_enumeration has those): the words the oracle changes in a
    NaN-patterned arena are exactly footprint()"""
    cases = _oracle_cases()
    assert len(cases) > 450
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


def _loop_words(dims, hdims, words, last_half):
    """sorted word offsets of a guru vector of transforms, by the definition: one plain loop per howmany dimension
    and per dimension, [(n, stride in elements)]; `words` per element; last_half: n_last / 2 + 1 entries"""
    loops = list(hdims) + list(dims)
    if last_half:
        loops[-1] = (loops[-1][0] // 2 + 1, loops[-1][1])
    out = []

    def walk(level, base):
        n, st = loops[level]
        if level == len(loops) - 1:
            for j in range(n):
                for w in range(words):
                    out.append(words * (base + j * st) + w)
            return
        for j in range(n):
            walk(level + 1, base + j * st)
    walk(0, 0)
    return np.array(sorted(set(out)), dtype=np.int64)


def test_guru_footprints_equal_a_nested_loop_enumeration():
    """the layouts the oracle cannot run (split planes, transposed output, a two-level howmany loop): footprint()
    and the scatter / gather offsets against an independent enumeration, a plain loop nest over the guru lists"""
    seen, count = set(), 0
    for c in CASES:
        key = (c.kind, c.shape, c.hm, c.layout)
        if not (c.layout.startswith("split") or c.layout in FC.GURU_ONLY) or key in seen or c.n * c.hm > (1 << 19):
            continue
        seen.add(key)
        count += 1
        prob = c.problem()
        assert prob.guru
        for which, side, fp, elems in (("in", prob.in_side, prob.in_fp, prob.in_elems),
                                       ("out", prob.out_side, prob.out_fp, prob.out_elems)):
            k = 1 if which == "in" else 2
            dims = [(d[0], d[k]) for d in prob.dims]
            hdims = [(d[0], d[k]) for d in prob.hdims]
            words = 2 if side in ("complex", "halfcomplex") else 1
            want = _loop_words(dims, hdims, words, side.endswith("halfcomplex"))
            assert np.array_equal(fp, want), (c.id, which, fp[:8], want[:8])
            assert elems.shape == (c.hm,) + F.logical_shape(c.shape, side), (c.id, which, elems.shape)
            assert np.array_equal(np.unique(F.word_offsets(elems, side)), want), (c.id, which)
        # every arena of a split side has the side's footprint; the planes never share an arena
        sides = [prob.in_side] if prob.inplace else [prob.in_side, prob.out_side]
        assert len(prob.arenas()) == sum(2 if sd.startswith("split") else 1 for sd in sides), c.id
    assert count >= 60, count


def test_embed_dims_is_the_advanced_interface():
    """the embed constructor against the manual's formula, element (b, j0, j1, j2) of a 3-D sub-array"""
    dims, hdims = F.embed_dims((3, 4, 6), 5, (7, 8, 9), 2, 1111, (4, 5, 4), 3, 999, "real", "halfcomplex")
    assert dims == [(3, 2 * 72, 3 * 20), (4, 2 * 9, 3 * 4), (6, 2, 3)] and hdims == [(5, 1111, 999)]
    e = F.elem_offsets(*F.side_dims(dims, hdims, "halfcomplex", "out"))
    assert e.shape == (5, 3, 4, 4) and e[4, 2, 3, 3] == 4 * 999 + 3 * ((2 * 5 + 3) * 4 + 3)
    e = F.elem_offsets(*F.side_dims(dims, hdims, "real", "in"))
    assert e.shape == (5, 3, 4, 6) and e[1, 2, 1, 5] == 1111 + 2 * ((2 * 8 + 1) * 9 + 5)


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


def test_every_nd_family_is_reached_by_a_non_dense_case():
    reached = FC.nd_family_labels(_plan_on_host)
    for f, cid in sorted(reached.items()):
        print("%-24s %s" % (f, cid))
    assert sorted(reached) == sorted(FC.ND_FAMILIES), sorted(set(FC.ND_FAMILIES) - set(reached))


def test_nd_cases_cover_every_layout_of_every_kind():
    """every (kind, layout) pair of ND_LAYOUTS is a case of rank >= 2, on a shape of rank 2 and on one of rank 3 or
    more; c2r has every out-of-place device layout with and without FFTW_PRESERVE_INPUT; the pinned labels of every
    nd case hold for the plan made on host arrays"""
    nd = FC.nd_cases()
    have = set((c.kind, c.layout + ("@host" if c.host else ""), min(len(c.shape), 3)) for c in nd)
    want = set((k, name, r) for k, names in FC.ND_LAYOUTS.items() for name in names for r in (2, 3))
    assert not want - have, sorted(want - have)
    keep = set((c.layout, bool(c.flags & FC.PRESERVE_INPUT)) for c in nd if c.kind == "c2r" and not c.host)
    for name in FC.ND_LAYOUTS["c2r"]:
        if not name.endswith("@host"):
            assert (name, False) in keep and ((name, True) in keep or "inplace" in name), name
    for c in nd + FC.no_transpose_cases():
        if c.labels or c.absent or c.tile:
            prob = c.problem()
            with AC.knobs(c.env):
                plan = prob.plan(fa, [a.user() for a in prob.arenas()])
                AC.check_plan(c, plan)
                AC.check_labels(c, plan.sprint())


def test_case_ids_are_unique_and_references_are_shared():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids)) and len(ids) >= 1300
    # cases of one (kind, shape, hm, sign, r2r) are adjacent: the long-double reference cache holds 5 entries
    keys = [(c.kind, c.shape, c.hm, c.sign, c.r2r) for c in CASES]
    runs = 1 + sum(1 for a, b in zip(keys, keys[1:]) if a != b)
    assert runs == len(set(keys)), (runs, len(set(keys)))


# ---- the planner's step lists on arenas

class InterpAll(InterpImg2DR, InterpVol3D, InterpVol3DR, InterpC2R):
    """the base interpreter plus every step form that has an interpreter of its own: an instance of each of those
    classes, so each class's step() runs on an object of its own kind; it hands every other step to Interp"""

    def step(self, s, bufs, cs, cn):
        if s.kind == fa.STEP_PASS:
            for cls, mine in ((InterpImg2DR, s.variant == fa.K_IMG2DR), (InterpVol3D, s.variant == fa.K_VOL3D),
                              (InterpVol3DR, s.variant == fa.K_VOL3DR), (InterpC2R, s.flags & fa.F_REAL_DEC_C2R)):
                if mine:
                    return cls.step(self, s, bufs, cs, cn)
        return Interp.step(self, s, bufs, cs, cn)


def _interp(plan, prob, arrays, AR, store):
    it = InterpAll(plan)
    if prob.split:
        f = store.view(np.float64)
        ins, outs = prob.in_arenas(AR), prob.out_arenas(AR)
        it.run(f[ins[0].base + ins[0].lo:], f[outs[0].base + outs[0].lo:], scratch_reals(plan))
    elif prob.inplace:
        it.run(arrays[0], arrays[0], scratch_reals(plan))
    else:
        it.run(arrays[0], arrays[1], scratch_reals(plan))


def _sweep():
    """a seeded sweep of small problems: ranks 1 ... 4, prime factors up to 31 plus Bluestein and Rader lengths, the
    four kinds, the layouts of the GPU matrix (rank >= 2: those of ND_LAYOUTS, on extents that include the one-trip
    kernels' with their knobs set), in and out of place"""
    rng = np.random.default_rng(20260501)
    smooth = [n for n in range(2, 400) if max(A._factors(n)) <= 31]
    hard = [37, 41, 67, 74, 97, 101, 131, 257, 331]          # Rader / Bluestein
    c2c_l = ["dense", "gapped", "strided", "sparecol", "rows2cols", "dense-inplace", "gapped-inplace",
             "sparecol-inplace", "split1", "split2", "split-gapped", "unaligned"]
    real_l = ["dense", "padded-inplace", "gapped", "realstride2", "cplxstride3", "sparecol"]
    r2r_l = ["gapped", "strided", "sparecol", "gapped-inplace", "dense"]
    out, turn = [], dict.fromkeys(FC.ND_LAYOUTS, 0)
    for i in range(480):
        kind = ("c2c", "r2c", "c2r", "r2r")[i % 4]
        rank = 1 if i % 5 not in (0, 3) else int(rng.integers(2, 5 if i % 5 == 3 else 4))
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
            ext = [2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 16, 17, 20, 31] if rank < 4 else [2, 3, 4, 5, 7]
            if i % 5 == 3 and rank < 4:                 # the one-trip kernels' extents, knobs on
                ext = [8, 16, 32]
            shape = tuple(int(rng.choice(ext)) for _ in range(rank))
            kw = {}
            if kind == "r2r":
                kw["kinds"] = [int(rng.integers(11)) for _ in range(rank)]
                shape = tuple(max(s, 2) for s in shape)
            if i % 5 == 3:
                names = [nm for nm in FC.ND_LAYOUTS[kind] if not nm.endswith("@host")]
                name = names[turn[kind] % len(names)]   # in turn: every layout of every kind is drawn
                turn[kind] += 1
                kw["env"] = {"FFTW_AMD_VOL3D": "1", "FFTW_AMD_REAL_IMG": "1", "FFTW_AMD_REAL_VOL": "1"}
                if name == "unaligned":
                    kw["flags"] = FC.UNALIGNED
                if name == "howmany2":
                    hm *= 2
                if kind == "c2r" and "inplace" not in name and rng.integers(2):
                    kw["flags"] = kw.get("flags", 0) | FC.PRESERVE_INPUT
            else:
                name = "embedded" if rng.integers(2) else "dense"
            out.append(FC.FCase("sweep", kind, shape, hm, name, **kw))
    return out


def _oracle_result(c, x):
    """the oracle on the same layout, into arenas of its own"""
    prob = c.problem()
    if prob.guru:                       # the oracle has no guru interface: the same transform on dense arrays
        c = FC.FCase("sweep", c.kind, c.shape, c.hm, "dense" if len(c.shape) > 1 else "gapped", c.sign, r2r=c.r2r,
                     kinds=c.kinds)
        prob = c.problem()
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
    assert len(sweep) >= 480
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
    assert {k for k, _, _ in seen} == {"c2c", "r2c", "c2r", "r2r"} and {r for _, r, _ in seen} == {1, 2, 3, 4}
    for kind, names in FC.ND_LAYOUTS.items():
        drawn = {name for k, r, name in seen if k == kind and r > 1}
        assert drawn == {nm for nm in names if not nm.endswith("@host")}, (kind, drawn)


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


def test_transposition_cases_write_only_the_footprint_through_the_step_interpreter():
    """the exchanged-stride cases of the GPU matrix, whose plans end in a transposition step (in place without
    scratch when square), and two smaller ones, through the step interpreter"""
    rows = [c for c in CASES if c.layout in ("transposed-inplace", "transposed-out") and c.n <= (1 << 16)]
    rows += [FC.FCase("sweep", "c2c", shape, hm, "transposed-inplace") for shape, hm in (((24, 24), 3), ((12, 20), 2))]
    kinds = set()
    for c in rows:
        x = FC.make_input(c)
        r = FC.run(c, x, execute=_interp)
        kinds.update(w for w in ("(transpose-inplace n=1", "(transpose n=1") if w in r.sprint)
        assert not any(r.violations), (c.id, r.violations, r.sprint)
        assert aerror(r.got, _oracle_result(c, x)) < TOL, (c.id, r.sprint)
        if not c.problem().inplace:
            assert r.preserved, (c.id, r.sprint)
        assert r.repeat, c.id
    assert len(kinds) == 2, kinds


def test_arena_layout():
    a = F.Arena(1000, np.float64, 100)
    assert a.guard == F.GUARD_MIN and a.lo == a.guard and a.size == 1000 + 2 * a.guard
    b = F.Arena(10, np.complex128, 70000, offset=1)
    assert b.guard == 70144 and b.guard % 512 == 0 and b.lo == b.guard + 1
    assert np.isnan(b.f64).all() and len(np.unique(b.words)) == b.size
    assert int(b.words[5]) == 0x7FF8000000000005
