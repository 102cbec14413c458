"""The footprint case matrix and its runner (tests/footprint.py), in the style of
tests/accuracy_cases.py whose Case, knobs, make_input, ref_ld, measure and check_labels it reuses.

One FCase is one plan on arenas: a transform, a named layout, device or host arrays, flags and knobs.  run() executes
it twice on re-initialised arenas and returns what the four parts of the pass condition need.  Cases that share
(kind, shape, hm, sign) are adjacent, so that the cached long-double reference serves all their layouts.
"""
import numpy as np

import accuracy as A
import accuracy_cases as AC
import footprint as F
from footprint import Layout as L
import fftw3_amd as fa
from util import crand, oracle_c2r, oracle_r2c, oracle_r2r, rrand

UNALIGNED, PRESERVE_INPUT = fa.UNALIGNED, fa.PRESERVE_INPUT

# the kernel families of the c2c table: (label substrings of sprint(), all of which one non-dense case must show)
FAMILIES = {
    "pass1r": ["/reg1"],
    "reg2": ["pass-120/reg2"],
    "reg3": ["pass-1000/reg3"],
    "row-per-workgroup-8192": ["pass-8192/reg3"],
    "row-per-workgroup-10000": ["pass-10000/reg3"],
    "lds": ["pass-299/lds:23x13"],
    "bluestein-rows": ["bluestein-rows n=1031"],
    "bluestein-steps": ["copy n=2100", "pass-2100/reg3"],
    "rader": ["rader-mul n=12288"],
    "two-pass": ["pass-184/reg2", "tw=33856"],
    "pass1024": ["pass-1024/reg32x32"],
    "pass-2048x1024": ["pass-2048/reg3", "pass-1024/reg32x32"],
}
# the three one-trip r2r rows steps (accuracy_cases.R2R_ROWS); the tile follows, so that "pre" is not "pre+post"
R2R_ROWS_STEPS = ["r2c-rows+r2r-post tile=", "c2r-rows+r2r-pre tile=", "c2r-rows+r2r-pre+post tile="]


class FCase(AC.Case):
    def __init__(self, fam, kind, shape, hm, layout, sign=-1, labels=(), env=None, r2r=None, host=False, flags=0,
                 absent=(), kinds=None, tile=None):
        AC.Case.__init__(self, fam, kind, shape, hm, sign, labels, env, r2r=r2r, absent=absent, tile=tile)
        self.layout, self.host, self.flags, self.kinds = layout, host, flags, kinds

    @property
    def id(self):
        s = AC.Case.id.fget(self) + "-" + self.layout
        if self.kinds:
            s += "-k" + "x".join(str(k) for k in self.kinds)
        if self.host:
            s += "-host"
        if self.flags & PRESERVE_INPUT:
            s += "-preserve"
        return s

    @property
    def dense(self):
        return self.layout == "dense" and not self.host

    def problem(self):
        return problem(self)


def _plus2(shape):
    return tuple(v + 2 for v in shape)


def problem(c):
    """the Problem of a case: its layout name spelt out in FFTW's embed / stride / dist"""
    kind, shape, h, name = c.kind, c.shape, c.hm, c.layout
    kw = dict(sign=c.sign, flags=c.flags)
    if kind == "r2r":
        kw["r2r"] = c.kinds or [c.r2r]
    if len(shape) > 1:
        hs = F.logical_shape(shape, "halfcomplex")
        si = hs if kind == "c2r" else shape
        so = hs if kind == "r2c" else shape
        if name == "dense":
            return F.Problem(kind, shape, h, L(), L(), **kw)
        if name == "dense-inplace":
            assert kind in ("c2c", "r2r")
            return F.Problem(kind, shape, h, L(), L(), inplace=True, **kw)
        if name == "embedded":
            ei, eo = _plus2(si), _plus2(so)
        else:
            assert name == "embedded-70x100-66x99"
            ei, eo = (70, 100), (66, 99)
        return F.Problem(kind, shape, h, L(ei, 1, int(np.prod(ei))), L(eo, 1, int(np.prod(eo))), **kw)
    n = shape[0]
    if kind in ("c2c", "r2r"):
        table = {
            "dense": (L(), L(), {}),
            "gapped": (L(None, 1, n + 3), L(None, 1, n + 5), {}),
            "strided": (L(None, 3, 3 * n + 1), L(None, 2, 2 * n + 7), {}),
            "sparecol": (L(None, h + 2, 1), L(None, h + 2, 1), {}),
            "rows2cols": (L(None, 1, n), L(None, h + 1, 1), {}),
            "dense-inplace": (L(), L(), dict(inplace=True)),
            "gapped-inplace": (L(None, 1, n + 3), L(None, 1, n + 3), dict(inplace=True)),
            "sparecol-inplace": (L(None, h + 2, 1), L(None, h + 2, 1), dict(inplace=True)),
            "split1": (L(None, 1, n), L(None, 1, n), dict(split=True)),
            "split2": (L(None, 2, 2 * n + 1), L(None, 1, n), dict(split=True)),
            "split-gapped": (L(None, 1, n + 3), L(None, 1, n + 5), dict(split=True)),
            "unaligned": (L(), L(), dict(offset=1)),
        }
        li, lo, extra = table[name]
        kw.update(extra)
        return F.Problem(kind, shape, h, li, lo, **kw)
    # 1-D r2c / c2r: the real side and the half-complex side (nh elements)
    nh = n // 2 + 1
    table = {
        "dense": (L(), L(), {}),
        "padded-inplace": (L((2 * nh,), 1, 2 * nh), L(None, 1, nh), dict(inplace=True)),
        "gapped": (L(None, 1, n + 3), L(None, 1, nh + 5), {}),
        "realstride2": (L(None, 2, 2 * n + 1), L(), {}),
        "cplxstride3": (L(), L(None, 3, 3 * nh + 1), {}),
        "sparecol": (L(None, h + 1, 1), L(None, h + 1, 1), {}),
    }
    lr, lc, extra = table[name]
    kw.update(extra)
    li, lo = (lr, lc) if kind == "r2c" else (lc, lr)
    return F.Problem(kind, shape, h, li, lo, **kw)


def _p1tile(n):
    return 256 * (6 if n == 4 else min(8, 32 // n))


def cases():
    C = []

    def c2c(fam, n, hm, layouts, labels=(), env=None, absent=(), signs=(-1,)):
        """layouts of one (n, hm), grouped by direction so that each reference is computed once"""
        for sign in signs:
            for name in layouts:
                host = name.endswith("@host")
                name = name.replace("@host", "")
                if sign > 0 and name not in ("dense", "gapped"):
                    continue
                if sign > 0 and host:
                    continue
                pinned = name == "dense" and not host
                C.append(FCase(fam, "c2c", (n,), hm, name, sign, labels=labels if pinned else (), env=env,
                               absent=absent if pinned else (), host=host,
                               flags=UNALIGNED if name == "unaligned" else 0))

    ALL = ["dense", "gapped", "strided", "sparecol", "rows2cols", "dense-inplace", "gapped-inplace",
           "sparecol-inplace", "split1", "split2", "gapped@host", "sparecol@host", "split-gapped@host", "unaligned"]
    both = (-1, +1)
    for n in (4, 7, 32):
        for hm in (2 * _p1tile(n) + 257, _p1tile(n) + 3):
            c2c("pass1r", n, hm, ALL, ["pass-%d/reg1" % n], signs=both)
    c2c("reg2", 120, 67, ALL, ["pass-120/reg2"], signs=both)
    c2c("reg2", 512, 67, ALL, ["pass-512/reg"], signs=both)
    c2c("reg3", 1000, 67, ALL, ["pass-1000/reg3"], signs=both)
    c2c("reg3", 2048, 67, ALL, ["pass-2048/reg3"], signs=both)
    c2c("reg3", 4096, 17, ALL, ["pass-4096/reg3"], signs=both)
    c2c("row-per-workgroup", 8192, 5, ALL, ["pass-8192/reg3"], signs=both)
    c2c("row-per-workgroup", 10000, 5, ALL, ["pass-10000/reg3"], signs=both)
    c2c("lds", 299, 20, ALL, ["pass-299/lds:23x13"], signs=both)
    for sign in both:                   # the two Bluestein forms share each direction's reference
        c2c("bluestein", 1031, 5, ALL, ["bluestein-rows n=1031"], signs=(sign,))
        c2c("bluestein-steps", 1031, 5, ALL, ["copy n=2100", "pass-2100/reg3"], env={"FFTW_AMD_NO_BLUE_ROWS": "1"},
            absent=["bluestein-rows"], signs=(sign,))
    c2c("rader", 12289, 3, ALL, ["rader-mul n=12288"], signs=both)
    c2c("two-pass", 184 * 184, 3, ALL, ["pass-184/reg2", "tw=%d" % (184 * 184)],
        env={"FFTW_AMD_FORCE_LENS": "184,184"}, signs=both)
    c2c("pass1024", 1 << 20, 2, ["dense", "gapped", "dense-inplace", "gapped-inplace"],
        ["pass-1024/reg32x32 tile=8 buf0", "pass-1024/reg32x32 tile=8 tw=1048576"], signs=both)
    c2c("pass-2048x1024", 1 << 21, 1, ["dense", "dense-inplace"])       # a lone transform: the planner's own split
    c2c("pass-2048x1024", 1 << 21, 2, ["dense", "dense-inplace"],
        ["pass-2048/reg3", "pass-1024/reg32x32 tile=8 tw=2097152"])
    # c2c in more dimensions, embedded in larger arrays
    C.append(FCase("nd", "c2c", (64, 96), 2, "embedded-70x100-66x99"))
    C.append(FCase("nd", "c2c", (3, 5, 7), 2, "embedded"))
    # real transforms; c2r with and without FFTW_PRESERVE_INPUT
    RL = ["dense", "padded-inplace", "gapped", "realstride2", "cplxstride3", "sparecol", "gapped@host"]
    for n, hm in ((64, 131), (256, 35), (2000, 11), (8192, 11), (1009, 5), (1 << 20, 1)):
        for kind in ("r2c", "c2r"):
            for name in RL:
                host = name.endswith("@host")
                name = name.replace("@host", "")
                labels = ()
                if name == "dense" and not host:
                    labels = {8192: ["pass-4096/%s-rows" % kind],
                              1 << 20: ["r2c-untangle n=1048576" if kind == "r2c" else "c2r-tangle n=1048576"],
                              1009: ["rader-mul n=1008"] + (["herm-expand n=1009"] if kind == "c2r" else [])
                              }.get(n, ())
                C.append(FCase("real", kind, (n,), hm, name, labels=labels, host=host))
                if kind == "c2r" and not host and "inplace" not in name:
                    C.append(FCase("real", kind, (n,), hm, name, labels=labels, flags=PRESERVE_INPUT))
    for shape in ((16, 9), (128, 1024)):
        for kind in ("r2c", "c2r"):
            for name in ("dense", "embedded"):
                C.append(FCase("real-nd", kind, shape, 2, name))
                if kind == "c2r":
                    C.append(FCase("real-nd", kind, shape, 2, name, flags=PRESERVE_INPUT))
    for kind in ("r2c", "c2r"):
        C.append(FCase("real-nd", kind, (5, 6, 8), 2, "embedded"))
    C.append(FCase("real-nd", "c2r", (5, 6, 8), 2, "embedded", flags=PRESERVE_INPUT))
    # r2r: the eleven kinds
    for n in (1000, 243):
        for k in range(11):
            for name in ("gapped", "strided", "sparecol", "gapped-inplace"):
                C.append(FCase("r2r", "r2r", (n,), 3, name, r2r=k, labels=["r2r-" + AC.R2R_TAG[k]]))
    C.append(FCase("r2r-nd", "r2r", (12, 1000), 2, "embedded", kinds=[5, 8]))
    # r2r-rows: the one-trip real-rows kernels with r2r hooks at half lengths 128 and 1024 (tiles of 32 and 4 rows),
    # the ragged batches of the accuracy matrix.  Only the dense case pins the step; which other layouts keep it is
    # r2r_rows_steps' business
    for half in (128, 1024):
        for k in (0, 5, 9, 1, 4, 8, 3, 7):
            n, hm, T, lab = AC.r2r_rows(half, k)
            for name in ("dense", "gapped", "strided", "sparecol", "dense-inplace", "gapped-inplace"):
                pin = dict(labels=[lab], absent=AC.R2R_ROWS_ABSENT, tile=T) if name == "dense" else {}
                C.append(FCase("r2r-rows", "r2r", (n,), hm, name, r2r=k, **pin))
    # the rows step as the last axis of a plan that another axis shares, embedded and in place
    C.append(FCase("r2r-rows-nd", "r2r", (24, 256), 2, "embedded", kinds=[4, 5],
                   labels=["pass-128/r2c-rows+r2r-post tile=32"]))
    C.append(FCase("r2r-rows-nd", "r2r", (20, 256), 2, "dense-inplace", kinds=[9, 8],
                   labels=["pass-128/c2r-rows+r2r-pre+post tile=32"]))
    return C


# ---- inputs and references (1-D and c2c: those of accuracy_cases; real and r2r in more dimensions: here)

def _nd_real(case):
    return len(case.shape) > 1 and case.kind != "c2c"


def make_input(case):
    if not _nd_real(case):
        return AC.make_input(case)
    rng = np.random.default_rng(AC._seed("%s-%s-%d" % (case.kind, case.shape, case.hm)))
    if case.kind == "c2r":
        return crand(rng, case.hm, *F.logical_shape(case.shape, "halfcomplex"))
    return rrand(rng, case.hm, *case.shape)


def _rows(fn, y, ax):
    """fn on the 1-D rows of y along axis ax"""
    z = np.moveaxis(y, ax, -1)
    zs = z.shape
    out = fn(np.ascontiguousarray(z).reshape(-1, zs[-1]))
    return np.moveaxis(out.reshape(zs[:-1] + (out.shape[-1],)), -1, ax)


_LD = {}


def _ld_nd(case, x):
    """long-double reference of a real or r2r transform in more dimensions: the 1-D references of
    tests/accuracy.py axis by axis (FFTW: c2r transforms the leading dimensions first, the halved one last)"""
    key = (case.kind, case.shape, case.hm, tuple(case.kinds or ()))
    if key in _LD:
        return _LD[key]
    _LD.clear()
    shape, hm, r = case.shape, case.hm, len(case.shape)
    if case.kind == "r2c":
        y = A.ld_dft(x, shape, hm, -1)[..., :shape[-1] // 2 + 1]
    elif case.kind == "c2r":
        y = np.asarray(x, dtype=A.CLD)
        for ax in range(1, r):
            y = _rows(lambda v: A._fft_rows(v, +1), y, ax)
        y = _rows(lambda v: A.ld_c2r(v, shape[-1], v.shape[0]), y, r)
    else:
        y = np.asarray(x, dtype=A.LD)
        for ax in range(r):
            y = _rows(lambda v, k=case.kinds[ax]: A.ld_r2r(v, k), y, ax + 1)
    _LD[key] = np.ascontiguousarray(y)
    return _LD[key]


def ref_oracle(case, x):
    if not _nd_real(case):
        return AC.ref_oracle(case, x)
    if case.kind == "r2c":
        return oracle_r2c(x, case.shape, case.hm).reshape((case.hm,) + F.logical_shape(case.shape, "halfcomplex"))
    if case.kind == "c2r":
        return oracle_c2r(x.reshape(-1), case.shape, case.hm).reshape((case.hm,) + case.shape)
    return oracle_r2r(x.reshape(-1), list(case.shape), case.kinds, howmany=case.hm).reshape(x.shape)


def ref_numpy(case, x):
    if not _nd_real(case):
        return AC.ref_numpy(case, x)
    axes = tuple(range(1, len(case.shape) + 1))
    if case.kind == "r2c":
        return np.fft.rfftn(x, axes=axes)
    if case.kind == "c2r":
        return np.fft.irfftn(x, s=case.shape, axes=axes, norm="forward")
    y = x
    for ax, k in enumerate(case.kinds):
        y = _rows(lambda v, k=k: AC._np_r2r(v, k), y, ax + 1)
    return y


def measure(case, got, x):
    """accuracy_cases.measure, extended to real and r2r transforms in more dimensions"""
    if not _nd_real(case):
        return AC.measure(case, got, x)
    ld = _ld_nd(case, x)
    orc, nmp = ref_oracle(case, x), ref_numpy(case, x)
    out = {"gpu": A.rms_err(got, ld), "oracle": A.rms_err(orc, ld), "numpy": A.rms_err(nmp, ld)}
    if case.n >= 1024 and case.hm > 1:
        out["per"] = tuple(A.rms_err_per_transform(v, ld, case.hm) for v in (got, orc, nmp))
    return out


# ---- the runner

class Result(object):
    """violations: per arena, after the first execution; got: the logical output of the first execution; repeat: a
    second execute() of the same plan on the re-initialised arenas left bit-identical output arenas; preserved: the
    input arenas are bit-identical after both executions (None in place)"""
    pass


class _DeviceWords(object):
    """payload-based indexing of a device arena that returns numpy (what Problem.gather needs)"""

    def __init__(self, t, lo):
        self.t, self.lo = t, lo

    def __getitem__(self, idx):
        import torch
        return self.t[torch.from_numpy(np.asarray(idx, dtype=np.int64) + self.lo).to(self.t.device)].cpu().numpy()


def run(case, x, execute=None):
    """plan the case once on fresh arenas and execute that plan twice, the arenas re-initialised in between.  Device
    cases upload the arenas and compare on the device; host cases hand the numpy arenas to the library.
    `execute(plan, prob, arrays, arenas, store)` replaces plan.execute() + sync (the CPU tier passes the step
    interpreter)."""
    prob = case.problem()
    AR = prob.arenas()
    store = F.colocate(AR) if (prob.split and execute is not None) else None
    prob.scatter(AR, x)
    before = [a.snapshot() for a in AR]
    written = prob.written(AR)
    device = not case.host and execute is None
    ins = [i for i, a in enumerate(AR) if any(a is o for o in prob.in_arenas(AR))]
    outs = [i for i, a in enumerate(AR) if any(a is o for o in prob.out_arenas(AR))]
    res = Result()
    if device:
        import torch
        ref = [a.to_device() for a in AR]
        full = [t.clone() for t in ref]
        arrays = [t[a.lo:] for t, a in zip(full, AR)]
    else:
        ref, full = before, [a.words for a in AR]
        arrays = [a.user() for a in AR]
    with AC.knobs(case.env):
        plan = prob.plan(fa, arrays)
        AC.check_plan(case, plan)
        res.sprint = plan.sprint()
        res.plan_steps = [(s.src_buf, s.dst_buf) for s in plan.steps()]
        res.preserved = None if prob.inplace else True
        first = None
        for trip in range(2):
            if trip:                    # the same arrays back to the images they had before the first execution
                for f, r in zip(full, ref):
                    if device:
                        f.copy_(r)
                    else:
                        f[:] = r
            if execute is None:
                plan.execute()
                plan.sync()
                if device:
                    torch.cuda.synchronize()
            else:
                execute(plan, prob, arrays, AR, store)
            if not prob.inplace:
                res.preserved = res.preserved and all(F.same_bits(full[i], ref[i]) for i in ins)
            if trip == 0:
                res.violations = [F.check(r, f, w) for r, f, w in zip(ref, full, written)]
                views = [_DeviceWords(full[i], AR[i].lo) if device else AR[i].user() for i in outs]
                res.got = prob.gather(views)
                first = [full[i].clone() if device else full[i].copy() for i in outs]
            else:
                res.repeat = all(F.same_bits(full[i], f) for i, f in zip(outs, first))
        plan.destroy()
    return res


def family_labels(sprint_of):
    """{family of FAMILIES: id of the first non-dense 1-D c2c case whose sprint shows all the family's labels};
    sprint_of(case) -> the case's sprint(), or None to pass the case over"""
    reached = {}
    for c in cases():
        if c.kind != "c2c" or len(c.shape) > 1 or c.dense or c.layout == "unaligned":
            continue
        s = sprint_of(c)
        for f in FAMILIES:
            if s and f not in reached and all(lab in s for lab in FAMILIES[f]):
                reached[f] = c.id
    return reached


def r2r_rows_steps(sprint_of):
    """{step of R2R_ROWS_STEPS: id of the first non-dense r2r-rows case whose plan is that one step};
    sprint_of(case) -> the case's sprint(), or None to pass the case over"""
    reached = {}
    for c in cases():
        if c.fam != "r2r-rows" or c.dense:
            continue
        s = sprint_of(c)
        for lab in R2R_ROWS_STEPS:
            if s and lab not in reached and lab in s and len(s.strip().split("\n")) == 2:
                reached[lab] = c.id
    return reached
