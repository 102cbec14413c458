"""The cases of tests/test_elem_forms.py and tests/test_gpu_elem_forms.py: problems of the plan corpus
(tools/plan_dump.py) whose element-wise steps reach every kernel form of kernels_elem.hip, each fast case once more
with its arrays 8 bytes off a 16-byte boundary, where the streaming forms must not be taken.

tests/golden/elem_forms.txt pins the form of every element-wise step, one line per step: `case step kind form`.  It
is a record of the kernels these cases launch on the device, so it does not depend on fa_hip_elem_form, the function
it checks."""
import importlib.util
import os

import fftw3_amd as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("plan_dump", os.path.join(ROOT, "tools", "plan_dump.py"))
plan_dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plan_dump)

GOLDEN = os.path.join(ROOT, "tests", "golden", "elem_forms.txt")
FAST_FORMS = ("POST2_DCT", "PRE2_DCT", "POST2_FAST", "PRE2_FAST", "POST4_FAST", "PRE4_FAST", "R2R_SHUFFLE", "R2R_UNSHUFFLE")


def cases():
    """[(case id, environment, plan_dump function, arguments, keywords)]"""
    P = plan_dump
    out = []

    def add(cid, env, fn, *a, **k):
        out.append((cid, dict(env), fn, a, k))

    for d, fwd in (("r2c", True), ("c2r", False)):
        add(d + "-512x8-norows", P.NOROWS, P.real_many, fwd, [512], 8)
        add(d + "-512x8-norows-off8", P.NOROWS, P.real_many, fwd, [512], 8, roff=8, coff=8)
        add(d + "-64x4-force4", P.FORCE4, P.real_many, fwd, [64], 4)
        add(d + "-64x4-force4-off8", P.FORCE4, P.real_many, fwd, [64], 4, roff=8, coff=8)
        add(d + "-24x3-force4-strided", P.FORCE4, P.real_many, fwd, [24], 3, rstride=3, rdist=1, cstride=3, cdist=1)
        add(d + "-77", {}, P.real_many, fwd, [77])
    for name, kind in (("redft10", fa.REDFT10), ("redft01", fa.REDFT01)):
        add("r2r-%s-128x256-norows" % name, P.NOROWS, P.r2r_many, [128], [kind], 256)
        add("r2r-%s-128x256-norows-inplace-off8" % name, P.NOROWS, P.r2r_many, [128], [kind], 256, inplace=True, off=8)
        add("r2r-%s-64x4-force4" % name, P.FORCE4, P.r2r_many, [64], [kind], 4)
        add("r2r-%s-64x4-force4-inplace-off8" % name, P.FORCE4, P.r2r_many, [64], [kind], 4, inplace=True, off=8)
        # h = n / 2 odd: the DCT streaming forms are refused, the general untangle / tangle runs the r2r hooks
        add("r2r-%s-10x256-norows" % name, P.NOROWS, P.r2r_many, [10], [kind], 256)
    for name, kind in P.R2R_KINDS:
        add("r2r-%s-128x256-unfused" % name, P.UNFUSED, P.r2r_many, [128], [kind], 256)
    add("c2c-rader-61x8", {}, P.c2c_many, [61], 8)
    return out


def make_plan(case, doubles=plan_dump.doubles):
    """the plan of a case on arrays from `doubles`; the caller destroys it"""
    cid, env, fn, a, k = case
    with plan_dump.environment(env):
        return fn(*a, doubles=doubles, **k)


def plan_forms(plan):
    """[(step index, step kind, form name)] of the element-wise steps of a plan that runs in one chunk.  The
    misalignments are those of the arrays the plan was made on; scratch buffers (ids >= 2) are device allocations."""
    base = [fa.ptr(x) for x in plan._keep]
    cn = min(plan.batch, plan.chunk)
    assert cn == plan.batch

    def mis(buf, off):
        return ((base[buf] if buf < 2 else 0) + 8 * off) % 16

    return [(i, s.kind, fa.elem_form(s, mis(s.src_buf, s.src_base), mis(s.dst_buf, s.dst_base), cn))
            for i, s in enumerate(plan.steps()) if s.kind != fa.STEP_PASS]


def golden():
    """{case id: [(step index, step kind, form name)]}"""
    out = {}
    with open(GOLDEN) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                cid, step, kind, form = line.split()
                out.setdefault(cid, []).append((int(step), int(kind), form))
    return out
