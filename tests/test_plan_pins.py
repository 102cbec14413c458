"""The planner's output for the corpus of tools/plan_dump.py, pinned: tests/golden/plan_pins.txt holds, per case, the
step count and the SHA-256 of the canonical dump of its plan (every step field, the tables' descriptors, batch, chunk,
lanes, workspace, flop estimate).  Planning needs no device.  A change that is meant to alter plans regenerates the
file with `python tools/plan_dump.py --write`; its diff then shows which cases moved."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("plan_dump", os.path.join(ROOT, "tools", "plan_dump.py"))
plan_dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plan_dump)

CASES = plan_dump.corpus()


def _pins():
    with open(plan_dump.PINS) as f:
        return dict((line.split()[0], line.strip()) for line in f if line.strip())


def test_pins_file_lists_exactly_the_corpus():
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids)
    assert sorted(_pins()) == sorted(ids), "tools/plan_dump.py --write regenerates tests/golden/plan_pins.txt"


KNOBS = ["FFTW_AMD_" + k for k in (
    "NO_TUNED", "NO_3S", "NO_R1", "NO_BLUE_ROWS", "NO_NARROW", "NO_SPLIT_COSTS", "NO_LO_DFT", "NO_IMG2D", "NO_R2CROWS",
    "R2R_UNFUSED", "NO_RADIX4", "FORCE_RADIX4", "FORCE_LENS")]


def _plan_text(cid):
    """the dump of a pinned case without its two header lines (the id and the environment, which always differ)"""
    case = [c for c in CASES if c[0] == cid]
    assert len(case) == 1 and cid in _pins(), "%s is not a pinned case" % cid
    return plan_dump.dump_case(case[0])[0].split("\n", 2)[2]


@pytest.mark.parametrize("knob", KNOBS)
def test_each_knob_flips_a_pinned_plan(knob):
    """a condition on the corpus, not on the planner: the pins protect a switch only if some pinned case reaches it.
    The hash of a dump covers the line that names the environment, so the plans themselves are compared."""
    env = dict((c[0], c[1]) for c in CASES)
    with_knob, without = plan_dump.KNOB_TWINS[knob]
    assert knob in env[with_knob] and dict((k, v) for k, v in env[with_knob].items() if k != knob) == env[without]
    assert _pins()[with_knob].split()[2] != _pins()[without].split()[2]
    assert _plan_text(with_knob) != _plan_text(without), "%s changes nothing in the plan of %s" % (knob, without)


@pytest.mark.parametrize("cid,same_as", plan_dump.KNOB_SAME, ids=[c[0] for c in plan_dump.KNOB_SAME])
def test_knob_truth_rules(cid, same_as):
    """presence-tested hooks (=0 still switches the feature off); a malformed or non-matching FORCE_LENS is void"""
    assert _plan_text(cid) == _plan_text(same_as)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_is_the_pinned_one(case):
    want = _pins().get(case[0])
    got = plan_dump.pin_line(case)
    assert got == want, (
        "the plan of case %s differs from the pinned one (id, steps, sha256: got %r, pinned %r): run "
        "`python tools/plan_dump.py --case %s` on this commit and on the one the pins were written from and diff "
        "the two dumps; if the change is intended, `python tools/plan_dump.py --write`" % (case[0], got, want, case[0]))
