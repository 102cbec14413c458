"""The rms accuracy gate on the GPU (tests/accuracy.py): for every case of the matrix in tests/accuracy_cases.py the
plan, the oracle and numpy.fft transform the same input, all three are measured against the same long-double
reference, and

    e_gpu <= 3 * max(e_oracle, e_numpy, u / 2)

for the whole batch and, for n >= 1024, for every batch entry on its own (an error confined to a ragged last tile or
one chunk is not diluted by the rest).  Every case also asserts the kernel its plan's sprint() shows, and its device
arrays sit in the NaN-patterned arenas of tests/footprint.py: no word outside the output footprint may change and the
input of an out-of-place plan must come back bit for bit.  A case that names its tile also asserts that its plan is
that one step with two full tiles and a ragged one, and a case with linf set the 1e-10 bar as well.  This is in
addition to the 1e-10 checks of the other modules, which only see indexing bugs: a twiddle off by a few ulp passes
those and fails this.  The slowest cases carry "slow" in their ids (-k slow selects them)."""
import numpy as np
import pytest

import accuracy as A
import accuracy_cases as AC

A.require_longdouble()
pytestmark = pytest.mark.gpu

CASES = AC.cases()


@pytest.mark.parametrize("case", CASES, ids=[("slow-" if c.slow else "") + c.id for c in CASES])
def test_rms_error_within_three_times_the_references(case):
    x = AC.make_input(case)
    got, sprint, guards = AC.run_gpu(case, x)
    AC.check_labels(case, sprint)
    assert not any(guards.violations), (case.id, guards.violations, sprint)
    assert guards.preserved is not False, (case.id, "the input of an out-of-place plan changed", sprint)
    m = AC.measure(case, got, x)
    ratio = m["gpu"] / max(m["oracle"], m["numpy"], A.U / 2)
    print("%s gpu %.3f u oracle %.3f u numpy %.3f u ratio %.2f" % (case.id, m["gpu"] / A.U, m["oracle"] / A.U,
                                                                   m["numpy"] / A.U, ratio))
    AC.check_linf(case, got, x)
    assert A.passes(m["gpu"], m["oracle"], m["numpy"]), (case.id, m["gpu"] / A.U, m["oracle"] / A.U,
                                                        m["numpy"] / A.U, sprint)
    if "per" in m:
        eg, eo, en = m["per"]
        worst = int(np.argmax(eg / np.maximum(np.maximum(eo, en), A.U / 2)))
        for b in range(case.hm):
            assert A.passes(eg[b], eo[b], en[b]), (case.id, "entry %d" % b, eg[b] / A.U, eo[b] / A.U, en[b] / A.U)
        print("  worst entry %d: gpu %.3f u oracle %.3f u numpy %.3f u" % (worst, eg[worst] / A.U, eo[worst] / A.U,
                                                                           en[worst] / A.U))
