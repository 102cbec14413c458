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


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_is_the_pinned_one(case):
    want = _pins().get(case[0])
    got = plan_dump.pin_line(case)
    assert got == want, (
        "the plan of case %s differs from the pinned one (id, steps, sha256: got %r, pinned %r): run "
        "`python tools/plan_dump.py --case %s` on this commit and on the one the pins were written from and diff "
        "the two dumps; if the change is intended, `python tools/plan_dump.py --write`" % (case[0], got, want, case[0]))
