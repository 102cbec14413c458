"""CPU tier of the opt-in plan families (fa_family_table, planner.c): the list of configurations the FFTW_MEASURE
search times, the bits of a wisdom record, and that a family's environment variable and its wisdom bit mean the same
plan.

The table and the loop nest below restate what the search has always done; they are written out here and not derived
from the C code."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fftw3_amd as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2C, R2C, C2R, R2R = 0, 1, 2, 3
# (field, variable, wisdom bit, problem types, rank or None), in the order the search tries them
FAMILIES = [
    ("real_dec", "FFTW_AMD_REAL_DEC", 16, (R2C, C2R), None),
    ("real_img", "FFTW_AMD_REAL_IMG", 32, (R2C, C2R), None),
    ("real_vol", "FFTW_AMD_REAL_VOL", 128, (R2C, C2R), 3),
    ("real_imgl", "FFTW_AMD_REAL_IMGL", 256, (R2C, C2R), 2),
    ("vol3d", "FFTW_AMD_VOL3D", 64, (C2C,), 3),
    ("vol_planes", "FFTW_AMD_VOL_PLANES", 512, (C2C,), 3),
    ("img_wide", "FFTW_AMD_IMG_WIDE", 1024, (C2C,), 2),
]
CHUNKS = (64 << 20, 128 << 20, 256 << 20, 1 << 30, 4 << 30)
PROBLEMS = [(C2C, 1), (C2C, 2), (C2C, 3), (C2C, 4), (R2C, 1), (R2C, 2), (R2C, 3), (C2R, 1), (C2R, 2), (C2R, 3), (R2R, 1)]
FLAGS = [("MEASURE", fa.MEASURE), ("PATIENT", fa.PATIENT)]
COMBOS = [(t, r, name, f) for t, r in PROBLEMS for name, f in FLAGS]


def expected(ptype, rank, flags):
    nl = 2 if flags & (fa.PATIENT | fa.EXHAUSTIVE) else 1
    out = []
    for ci in range(5):
        for pi in range(2):
            for li in range(nl):
                for st in range(nl):
                    for lf in range(2):
                        lanes = 1 if pi else (2 if ci < 3 else 1)
                        bits = (1 if st else 0) | (2 if lf else 0) | ((lanes - 1) << 2)
                        out.append("%d %d %d %d" % (CHUNKS[ci], pi, 512 if li else 1024, bits))
    for _, _, bit, types, frank in FAMILIES:
        if ptype in types and frank in (None, rank):
            out.append("%d 0 1024 %d" % (128 << 20, (1 << 2) | bit))
    return out


def _run_child(call, env):
    code = "import sys; sys.path[:0] = %r\nimport test_measure_candidates as T\nT.%s\n" % (
        [ROOT, os.path.join(ROOT, "tests")], call)
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FFTW_AMD_")}
    env.update(extra)
    return env


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "t%d-r%d-%s" % c[:3])
def test_candidate_list_is_the_loop_nest_then_the_families(combo, monkeypatch):
    ptype, rank, _, flags = combo
    for _, var, _, _, _ in FAMILIES:
        monkeypatch.delenv(var, raising=False)
    got = fa.measure_candidates(ptype, rank, flags)
    assert got == expected(ptype, rank, flags)
    assert got[0] == "67108864 0 1024 4"
    assert len(got) == len(set(got))                    # no configuration is timed twice


def test_candidate_list_spot_values(monkeypatch):
    for _, var, _, _, _ in FAMILIES:
        monkeypatch.delenv(var, raising=False)

    def tail_bits(lines, k):
        assert all(l.startswith("134217728 0 1024 ") for l in lines[-k:])
        return [int(l.split()[3]) for l in lines[-k:]]

    c = fa.measure_candidates(C2C, 1, fa.MEASURE)
    assert len(c) == 20 and not any(int(l.split()[3]) >> 4 for l in c)
    c = fa.measure_candidates(C2C, 3, fa.MEASURE)
    assert len(c) == 22 and c[-2:] == ["134217728 0 1024 68", "134217728 0 1024 516"]
    c = fa.measure_candidates(C2C, 2, fa.MEASURE)
    assert len(c) == 21 and c[-1] == "134217728 0 1024 1028"
    c = fa.measure_candidates(R2C, 3, fa.PATIENT)
    assert len(c) == 83 and tail_bits(c, 3) == [20, 36, 132]
    c = fa.measure_candidates(C2R, 2, fa.MEASURE)
    assert len(c) == 23 and tail_bits(c, 3) == [20, 36, 260]
    c = fa.measure_candidates(R2C, 1, fa.MEASURE)
    assert len(c) == 22 and tail_bits(c, 2) == [20, 36]
    # the base candidates carry no family bit, plain MEASURE never tries small tiles, EXHAUSTIVE is PATIENT
    for ptype, rank, _, flags in COMBOS:
        base = fa.measure_candidates(ptype, rank, flags)[:80 if flags else 20]
        assert not any(int(l.split()[3]) >> 4 for l in base)
        assert flags or not any(int(l.split()[3]) & 1 for l in base)
        assert fa.measure_candidates(ptype, rank, flags | fa.EXHAUSTIVE) == fa.measure_candidates(ptype, rank, fa.PATIENT)


def child_lists():
    print(json.dumps([fa.measure_candidates(t, r, f) for t, r, _, f in COMBOS]))


def test_the_search_overrides_the_family_variables():
    """with every family switched on in the environment the search still times each family alone, after base
    candidates that have none"""
    got = _run_child("child_lists()", _clean_env(**{var: "1" for _, var, _, _, _ in FAMILIES}))
    assert got == [expected(t, r, f) for t, r, _, f in COMBOS]


def test_wisdom_bits_round_trip():
    """every value of the bits field comes back as it went in"""
    fa.forget_wisdom()
    try:
        for b in range(2048):
            rec = "(fftw3_amd_wisdom-1\n  (t0 s-1 r1 4096:2:2 h0 i1 o1 p0) 134217728 0 1024 %d 0.250000\n)\n" % b
            assert fa.import_wisdom_from_string(rec) == 1
            assert fa.export_wisdom_to_string() == rec, b
    finally:
        fa.forget_wisdom()


# one problem per family on which its emitter accepts: (type, shape, howmany)
ACCEPTED = {
    "real_dec": (R2C, (2048 * 256,), 3),
    "real_img": (R2C, (16, 16), 3),
    "real_vol": (R2C, (16, 16, 16), 3),
    "real_imgl": (R2C, (64, 64), 3),
    "vol3d": (C2C, (16, 16, 16), 3),
    "vol_planes": (C2C, (64, 64, 64), 3),
    "img_wide": (C2C, (128, 128), 3),
}


def _problem(ptype, shape, hm, flags):
    """(plan, wisdom key) of hm dense transforms, out of place, on zero arrays (planning touches no element)"""
    n = int(np.prod(shape))
    if ptype == C2C:
        x, y = np.zeros(hm * n, dtype=np.complex128), np.zeros(hm * n, dtype=np.complex128)
        mul_i, mul_o, idist, odist, last_o = 2, 2, n, n, shape[-1]
        make = lambda: fa.plan_many_dft(len(shape), list(shape), hm, x, None, 1, n, y, None, 1, n, fa.FORWARD, flags)
    else:
        h = shape[-1] // 2 + 1
        nc = n // shape[-1] * h
        x, y = np.zeros(hm * n), np.zeros(hm * nc, dtype=np.complex128)
        mul_i, mul_o, idist, odist, last_o = 1, 2, n, nc, h
        make = lambda: fa.plan_many_dft_r2c(len(shape), list(shape), hm, x, None, 1, n, y, None, 1, nc, flags)
    assert x.ctypes.data % 16 == 0 and y.ctypes.data % 16 == 0
    dims, si, so = [], mul_i, mul_o                     # row-major strides in doubles, as the key has them
    for k in reversed(range(len(shape))):
        dims.insert(0, "%d:%d:%d" % (shape[k], si, so))
        si, so = si * shape[k], so * (last_o if k == len(shape) - 1 else shape[k])
    key = "t%d s-1 r%d %s h1 %d:%d:%d i%d o1 p0" % (ptype, len(shape), " ".join(dims), hm, mul_i * idist, mul_o * odist,
                                                    1 if ptype == C2C else 0)
    return make, key


def child_plans(field):
    """the plan of ACCEPTED[field] three times: under the environment the parent gave this process (the family's variable
    set), with the variable gone, and with it gone under a wisdom record that carries the family's bit alone"""
    ptype, shape, hm = ACCEPTED[field]
    var, bit = [f[1:3] for f in FAMILIES if f[0] == field][0]
    assert os.environ[var] == "1"
    make, key = _problem(ptype, shape, hm, fa.ESTIMATE)
    by_env = make().sprint()
    del os.environ[var]                                 # read per plan: the next plan does not see it
    default = make().sprint()
    make, key = _problem(ptype, shape, hm, fa.ESTIMATE | fa.WISDOM_ONLY)
    assert fa.import_wisdom_from_string("(fftw3_amd_wisdom-1\n  (%s) 134217728 0 1024 %d 0.250000\n)\n" % (key, bit)) == 1
    by_bit = make().sprint()                            # raises under WISDOM_ONLY when the key is not the problem's
    print(json.dumps({"env": by_env, "default": default, "bit": by_bit}))


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f[0])
def test_variable_and_wisdom_bit_switch_on_the_same_plan(family):
    """in a child: neither the variable nor the record may outlive the case"""
    field, var = family[:2]
    got = _run_child("child_plans(%r)" % field, _clean_env(**{var: "1"}))
    assert got["env"] == got["bit"]
    assert got["env"] != got["default"] and got["bit"] != got["default"]
