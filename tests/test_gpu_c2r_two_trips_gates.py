"""The two-trip c2r plan (FFTW_AMD_F_REAL_DEC_C2R) under the two project gates, with the machinery of
tests/accuracy_cases.py and tests/footprint_cases.py: the rms gate against the long-double reference and the
NaN-patterned footprint arenas (nothing outside the output footprint changes, the input of the out-of-place plan comes
back bit for bit, a second execution repeats the first)."""
import numpy as np
import pytest

import accuracy as A
import accuracy_cases as AC
import footprint_cases as FC

A.require_longdouble()
pytestmark = pytest.mark.gpu

ENV = {"FFTW_AMD_REAL_DEC": "1"}
LABELS = ["reg3+c2r-decimated"]
RMS = [AC.Case("real-dec", "c2r", (1 << 22,), 1, labels=LABELS, env=ENV),
       AC.Case("real-dec", "c2r", (2048 * 256,), 3, labels=LABELS, env=ENV)]
FOOT = [FC.FCase("real-dec", "c2r", (2048 * 256,), 3, "dense", labels=LABELS, env=ENV),
        FC.FCase("real-dec", "c2r", (2048 * 256,), 3, "padded-inplace", labels=LABELS, env=ENV)]


def _gate(case, m):
    print("%s gpu %.3f u oracle %.3f u numpy %.3f u" % (case.id, m["gpu"] / A.U, m["oracle"] / A.U, m["numpy"] / A.U))
    assert A.passes(m["gpu"], m["oracle"], m["numpy"]), (case.id, m["gpu"] / A.U, m["oracle"] / A.U, m["numpy"] / A.U)
    if "per" in m:
        eg, eo, en = m["per"]
        for b in range(case.hm):
            assert A.passes(eg[b], eo[b], en[b]), (case.id, "entry %d" % b, eg[b] / A.U, eo[b] / A.U, en[b] / A.U)


@pytest.mark.parametrize("case", RMS, ids=[c.id for c in RMS])
def test_rms_error_within_three_times_the_references(case):
    x = AC.make_input(case)
    got, sprint, guards = AC.run_gpu(case, x)
    AC.check_labels(case, sprint)
    assert not any(guards.violations), (case.id, guards.violations, sprint)
    assert guards.preserved is not False, (case.id, "the input of an out-of-place plan changed", sprint)
    _gate(case, AC.measure(case, got, x))


@pytest.mark.parametrize("case", FOOT, ids=[c.id for c in FOOT])
def test_plan_writes_only_its_footprint(case):
    x = FC.make_input(case)
    r = FC.run(case, x)
    print("%s :: %s" % (case.id, " | ".join(ln.strip() for ln in r.sprint.strip().split("\n")[1:])))
    AC.check_labels(case, r.sprint)
    assert len(r.plan_steps) == 2, r.sprint
    assert not any(r.violations), (case.id, r.violations, r.sprint)
    _gate(case, FC.measure(case, r.got, x))
    assert r.repeat, (case.id, "the second execution of the plan differs from the first", r.sprint)
    assert r.preserved is not False, (case.id, "the input of an out-of-place plan changed", r.sprint)
