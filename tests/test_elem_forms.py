"""Which kernel form every element-wise step takes (fa_hip_elem_form, kernels_elem.hip), pinned: the cases of
elem_form_cases.py are planned on host arrays (planning and the probe need no device) and the form of every step that
is not a pass is compared with tests/golden/elem_forms.txt.  A wrong term in a form's predicate moves a step to the
general kernel, where every parity test stays green and only the speed is gone; here it moves a line."""
import pytest

import fftw3_amd as fa
import elem_form_cases as E

CASES = E.cases()


def test_fixture_lists_exactly_the_cases():
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids)
    assert sorted(E.golden()) == sorted(ids)


def test_fixture_holds_every_form_and_every_fast_form_refused():
    gold = E.golden()
    forms = set(f for steps in gold.values() for _, _, f in steps)
    assert forms == set(fa.ELEM_FORMS) - {"TRANSPOSE", "NONE"}
    # a case and its 8-bytes-off twin have the same steps; where the twin's form differs a fast form was refused.
    # The 16-byte side of the two DCT tangle forms is scratch, which no user offset reaches: see the test below
    refused = set()
    for cid, steps in gold.items():
        base = cid.replace("-inplace-off8", "").replace("-off8", "")
        if base != cid:
            assert [s[:2] for s in steps] == [s[:2] for s in gold[base]]
            refused |= set(b[2] for s, b in zip(steps, gold[base]) if s[2] != b[2])
    assert refused == set(E.FAST_FORMS) - {"POST2_DCT", "PRE2_DCT"}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forms_are_the_pinned_ones(case):
    p = E.make_plan(case)
    got = E.plan_forms(p)
    p.destroy()
    assert got == E.golden()[case[0]]


@pytest.mark.parametrize("cid, form, general, side", [
    ("r2r-redft10-128x256-norows", "POST2_DCT", "POST2", 0),     # reads 16-byte pairs from its source only
    ("r2r-redft01-128x256-norows", "PRE2_DCT", "PRE2", 1)])     # writes them to its destination only
def test_dct_tangle_forms_test_their_pair_side_only(cid, form, general, side):
    """the source of the DCT-II untangle and the destination of the DCT-III tangle are scratch, so the probe is asked
    directly: 8 bytes off on the side of the 16-byte accesses refuses the form, on the side of the reals it does not"""
    p = E.make_plan([c for c in CASES if c[0] == cid][0])
    step = [s for s in p.steps() if s.kind in (fa.STEP_R2C_POST, fa.STEP_C2R_PRE)][0]
    cn = p.batch
    p.destroy()
    assert fa.elem_form(step, 0, 0, cn) == form
    assert fa.elem_form(step, *((8, 0) if side == 0 else (0, 8)), cn) == general
    assert fa.elem_form(step, *((0, 8) if side == 0 else (8, 0)), cn) == form


def test_a_pass_is_no_element_wise_step():
    p = E.make_plan(CASES[0])
    forms = [fa.elem_form(s, 0, 0, p.batch) for s in p.steps() if s.kind == fa.STEP_PASS]
    p.destroy()
    assert forms and set(forms) == {"NONE"}
