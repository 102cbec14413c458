"""The footprint contract on the GPU (tests/footprint.py): every case of tests/footprint_cases.py
executes its plan twice on arenas whose every non-input word is a distinct quiet NaN, and

  1. no word outside FFTW's output footprint changes (guards, stride gaps, padding, spare columns, the input),
  2. the values inside it pass the rms gate of tests/accuracy.py against the long-double reference -- the gaps are
     NaN, so one over-read that reaches the result fails it,
  3. a second execute() of the same plan, the arenas re-initialised, leaves bit-identical output arenas,
  4. the input arenas of an out-of-place plan are bit-identical after both, for every kind and whatever the flags.

Every case prints the kernels its plan's sprint() shows; dense cases assert the labels the accuracy matrix pins.
Plans of rank 2 and more run in the layouts of footprint_cases.ND_LAYOUTS; the one-trip image and volume steps run in
their exact layouts, and every other layout must show the step gone (the fallback paths)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import accuracy as A
import accuracy_cases as AC
import footprint_cases as FC

A.require_longdouble()
pytestmark = pytest.mark.gpu

CASES = FC.cases()


PASSED = {}          # id -> sprint of the cases that ran and met the whole pass condition in this session


def _run_and_check(case):
    x = FC.make_input(case)
    r = FC.run(case, x)
    print("%s :: %s" % (case.id, " | ".join(ln.strip() for ln in r.sprint.strip().split("\n")[1:])))
    AC.check_labels(case, r.sprint)
    assert not any(r.violations), (case.id, r.violations, r.sprint)
    m = FC.measure(case, r.got, x)
    print("  gpu %.3f u oracle %.3f u numpy %.3f u" % (m["gpu"] / A.U, m["oracle"] / A.U, m["numpy"] / A.U))
    assert A.passes(m["gpu"], m["oracle"], m["numpy"]), (case.id, m["gpu"] / A.U, m["oracle"] / A.U,
                                                        m["numpy"] / A.U, r.sprint)
    if "per" in m:
        eg, eo, en = m["per"]
        for b in range(case.hm):
            assert A.passes(eg[b], eo[b], en[b]), (case.id, "entry %d" % b, eg[b] / A.U, eo[b] / A.U, en[b] / A.U)
    assert r.repeat, (case.id, "the second execution of the plan differs from the first", r.sprint)
    assert r.preserved is not False, (case.id, "the input of an out-of-place plan changed", r.sprint)
    PASSED[case.id] = r.sprint


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_plan_writes_only_its_footprint(case):
    _run_and_check(case)


def test_every_c2c_family_is_reached_by_a_non_dense_case_that_passed():
    """every kernel family of the c2c table shows in the sprint() of a non-dense case that executed and met the pass
    condition.  After the parametrised test above that is a lookup; selected on its own, this test runs the gapped
    and in-place cases itself."""
    def sprint_of(c):
        if c.id not in PASSED and not PASSED_ANY[0] and c.layout in ("gapped", "dense-inplace") and c.sign < 0:
            _run_and_check(c)
        return PASSED.get(c.id)

    PASSED_ANY = [bool(PASSED)]
    reached = FC.family_labels(sprint_of)
    for f, cid in sorted(reached.items()):
        print("%-24s %s" % (f, cid))
    assert sorted(reached) == sorted(FC.FAMILIES), sorted(set(FC.FAMILIES) - set(reached))


def test_every_r2r_rows_step_is_reached_by_a_non_dense_case_that_passed():
    """each of the three one-trip r2r rows steps is the whole plan of a non-dense case that executed and met the pass
    condition (a lookup after the parametrised test; selected on its own, this test runs the in-place cases)"""
    def sprint_of(c):
        if c.id not in PASSED and not PASSED_ANY[0] and c.layout == "dense-inplace":
            _run_and_check(c)
        return PASSED.get(c.id)

    PASSED_ANY = [bool(PASSED)]
    reached = FC.r2r_rows_steps(sprint_of)
    for lab, cid in sorted(reached.items()):
        print("%-32s %s" % (lab, cid))
    assert sorted(reached) == sorted(FC.R2R_ROWS_STEPS), sorted(set(FC.R2R_ROWS_STEPS) - set(reached))


def test_every_nd_family_is_reached_by_a_non_dense_case_that_passed():
    """every kernel family of the nd table shows in the sprint() of a case of rank >= 2 in a layout whose strides
    differ from dense (the in-place twin for the steps that exist on dense arrays only: footprint_cases.ND_DENSE_ONLY),
    that executed and that met the whole pass condition (a lookup after the parametrised test; selected on its own,
    this test runs the embedded and in-place cases of the nd table itself)"""
    def sprint_of(c):
        if c.id not in PASSED and not PASSED_ANY[0] and c.sign < 0 and c.hm <= 3 and not c.host and \
                (c.layout == "embedded" or c.layout.endswith("-inplace")):
            _run_and_check(c)
        return PASSED.get(c.id)

    PASSED_ANY = [bool(PASSED)]
    reached = FC.nd_family_labels(sprint_of)
    for f, cid in sorted(reached.items()):
        print("%-24s %s" % (f, cid))
    assert sorted(reached) == sorted(FC.ND_FAMILIES), sorted(set(FC.ND_FAMILIES) - set(reached))


def test_exchanged_strides_in_place_without_transposition_steps():
    """FFTW_AMD_NO_TRANSPOSE=1 is read once per process, so its cases run in a child: the in-place plans whose output
    strides are the input's exchanged, on the element-wise copies, under the same four-part pass condition"""
    code = ("import sys; sys.path[:0] = %r\n"
            "import footprint_cases as FC, test_gpu_footprint as T\n"
            "for c in FC.no_transpose_cases():\n"
            "    T._run_and_check(c)\n"
            "    assert 'transpose' not in T.PASSED[c.id], T.PASSED[c.id]\n"
            "print('checked', len(T.PASSED))\n") % ([FC.AC.ROOT, os.path.join(FC.AC.ROOT, "tests")],)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FFTW_AMD_NO_TRANSPOSE="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "checked %d" % len(FC.no_transpose_cases()) in r.stdout, r.stdout
