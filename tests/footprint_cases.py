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
        return _nd_problem(c, kw)
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


# the layouts an nd case can name, per kind ("@host": the same layout on host arrays)
ND_LAYOUTS = {
    "c2c": ["dense", "dense-inplace", "embedded", "embedded-inplace", "unaligned", "interleaved", "strided",
            "rows2cols", "split", "split-gapped", "transposed-out", "howmany2", "embedded@host", "split-gapped@host"],
    "r2c": ["dense", "embedded", "unaligned", "interleaved", "strided", "rows2cols", "padded-inplace", "split",
            "split-gapped", "howmany2", "embedded@host", "split-gapped@host"],
    "r2r": ["dense", "dense-inplace", "embedded", "embedded-inplace", "unaligned", "interleaved", "strided",
            "rows2cols", "transposed-out", "howmany2", "embedded@host"],
}
ND_LAYOUTS["c2r"] = ND_LAYOUTS["r2c"]
# `transposed-inplace` (c2c: the transposed output over the input) is named by the transposition cases only
GURU_ONLY = ("split", "split-gapped", "transposed-out", "transposed-inplace", "howmany2")


def _nd_problem(c, kw):
    """rank >= 2: the layout names of ND_LAYOUTS.  P_in / P_out are the element counts of one dense transform on
    each side (the half-complex side counts n_last / 2 + 1 in its last dimension)"""
    kind, shape, h, name = c.kind, c.shape, c.hm, c.layout
    assert name in ND_LAYOUTS[kind] or name in ("embedded-70x100-66x99", "transposed-inplace"), (kind, name)
    hs = F.logical_shape(shape, "halfcomplex")
    si = hs if kind == "c2r" else shape
    so = hs if kind == "r2c" else shape
    pi, po = int(np.prod(si)), int(np.prod(so))
    P = lambda li, lo, **extra: F.Problem(kind, shape, h, li, lo, **dict(kw, **extra))
    if name == "dense":
        return P(L(), L())
    if name == "dense-inplace":
        return P(L(), L(), inplace=True)
    if name == "unaligned":
        return P(L(), L(), offset=1)
    if name == "embedded":
        ei, eo = _plus2(si), _plus2(so)
        return P(L(ei, 1, int(np.prod(ei))), L(eo, 1, int(np.prod(eo))))
    if name == "embedded-70x100-66x99":
        return P(L((70, 100), 1, 7000), L((66, 99), 1, 66 * 99))
    if name == "embedded-inplace":
        e = _plus2(shape)
        return P(L(e, 1, int(np.prod(e))), L(e, 1, int(np.prod(e))), inplace=True)
    if name == "interleaved":           # the batch interleaved, two spare columns
        return P(L(None, h + 2, 1), L(None, h + 2, 1))
    if name == "strided":               # element strides 3 and 2, an odd gap after every transform
        return P(L(None, 3, 3 * pi + 1), L(None, 2, 2 * po + 7))
    if name == "rows2cols":
        return P(L(None, 1, pi), L(None, h + 1, 1))
    if name == "padded-inplace":        # the real rows padded to 2 (n_last / 2 + 1) reals, over the half spectra
        er = shape[:-1] + (2 * hs[-1],)
        lr, lc = L(er, 1, int(np.prod(er))), L(hs, 1, int(np.prod(hs)))
        return P(lr, lc, inplace=True) if kind == "r2c" else P(lc, lr, inplace=True)
    if name == "split":
        return P(L(None, 1, pi), L(None, 1, po), split=True)
    if name == "split-gapped":
        return P(L(None, 1, pi + 3), L(None, 1, po + 5), split=True)
    if name == "transposed-out":        # row-major in, column-major out: the output strides in reverse order
        so_t = [int(np.prod(shape[:k])) for k in range(len(shape))]
        return P(L(None, 1, pi), F.Guru(so_t, [(h, po)]))
    if name == "transposed-inplace":    # the output over the input, its strides in reverse order (c2c)
        so_t = [int(np.prod(shape[:k])) for k in range(len(shape))]
        return P(L(None, 1, pi), F.Guru(so_t, [(h, po)]), inplace=True)
    assert name == "howmany2" and h % 2 == 0
    # pairs of dense transforms, the pairs an odd gap further apart than two transforms: no single loop says that
    gi, go = F.embed_strides(si, None, 1), F.embed_strides(so, None, 1)
    return P(F.Guru(gi, [(h // 2, 2 * pi + 3), (2, pi)]), F.Guru(go, [(h // 2, 2 * po + 5), (2, po)]))


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
    C.extend(nd_cases())
    return C


def _nd(C, fam, kind, shape, hm, layouts, labels=(), env=None, absent=(), gone=(), kinds=None, signs=(-1,),
        tile=None, envs=None, bwd=("dense", "strided")):
    """the nd layouts of one (kind, shape, hm): `dense` pins labels / absent / tile, every other layout asserts that
    the labels `gone` are absent.  c2c: both directions in the layouts `bwd` (dense and a non-dense one), forward
    elsewhere; c2r: every out-of-place device layout also with FFTW_PRESERVE_INPUT; howmany2 has 2 hm transforms and
    comes last, so that every (kind, shape, hm, sign) stays one run of the table; envs: every layout under each of
    these knob sets"""
    order = [n for n in layouts if n != "howmany2"] + [n for n in layouts if n == "howmany2"]
    knobs = list(envs) if envs else [env]
    for sign in signs:
        for name, knob in [(n, e) for n in order for e in knobs]:
            host = name.endswith("@host")
            name = name.replace("@host", "")
            if sign > 0 and (host or name not in bwd):
                continue
            pinned = name == "dense" and not host
            kw = dict(sign=sign, env=knob, host=host, kinds=kinds, labels=labels if pinned else (),
                      absent=absent if pinned else gone, tile=tile if pinned else None)
            fl = UNALIGNED if name == "unaligned" else 0
            h = 2 * hm if name == "howmany2" else hm
            C.append(FCase(fam, kind, shape, h, name, flags=fl, **kw))
            if kind == "c2r" and not host and "inplace" not in name:
                C.append(FCase(fam, kind, shape, h, name, flags=fl | PRESERVE_INPUT, **kw))


def _one_trip(C, fam, kind, shape, T, label, env=None, exact=("dense",)):
    """a one-trip step: its exact layouts at hm = 2 T + 3 (the step and its tile pinned; check_plan), at hm = 1 and
    at hm = T - 1, a batch smaller than one tile (the step pinned), then at hm = 3 in every layout of the kind: the
    exact ones keep the step (and lose it without the knob `env` of an opt-in step), every other one must show that
    the label is gone -- the fallback paths.  c2c: the backward direction (the steps' swap flags) in every exact
    layout at the three batches, and at hm = 3 in dense (the step pinned) and strided (the step gone)"""
    signs = (-1, +1) if kind == "c2c" else (-1,)
    ragged = 2 * T + 3 if (2 * T + 3) % T else 2 * T + 1                 # T = 3: 2 T + 3 would be three full tiles
    for hm in sorted(set((ragged, 1, T - 1)) - set((0, 3))):             # 3 is the batch of the sweep below
        for sign in signs:
            for name in exact:
                C.append(FCase(fam, kind, shape, hm, name, sign, env=env, labels=[label],
                               tile=T if hm > 2 * T else None))
    step = label.split(" tile=")[0]
    order = [n for n in ND_LAYOUTS[kind] if n != "howmany2"] + ["howmany2"]
    for sign in signs:
        for name in order:
            keeps = name in exact
            one = []
            _nd(one, fam, kind, shape, 3, [name], env=env, gone=() if keeps else [step], signs=(sign,))
            for c in one:
                if keeps:
                    c.labels, c.absent = (label,), ()
            if keeps and env:           # an opt-in step: the same layout without the knob is the general path
                _nd(one, fam + "-off", kind, shape, 3, [name], absent=[step], gone=[step], signs=(sign,))
            C.extend(one)


# kernel families of the nd table: label substrings of sprint(), all of which one passing case of rank >= 2 that is
# not `dense` must show (nd_family_labels)
ND_FAMILIES = {
    "column-reg3": ["pass-1000/reg3", "pass-12/"],
    "column-reg2": ["pass-600/reg2", "pass-6/"],
    "rows-2048-short-columns": ["pass-2048/reg3", "pass-5/lds:5"],
    "two-pass-axis-4096": ["pass-64/lds:8x8 tile=3 tw=4096", "pass-3/"],
    "bluestein-axis-1031": ["copy n=2100", "pass-2100/reg3", "copy n=1031", "pass-6/"],
    "bluestein-axis-1030": ["copy n=2100", "pass-2100/reg3", "copy n=1030", "pass-4/"],
    "lds-axis": ["pass-299/lds:23x13", "pass-8/"],
    "rader-axis": ["rader-mul n=12288", "pass-3/"],
    "two-pass-axis-184x184": ["pass-184/lds:23x8", "tw=33856", "pass-3/"],
    "transpose-inplace": ["pass-256/reg2", "(transpose-inplace n=1"],
    "transpose": ["pass-160/reg2", "(transpose n=1"],
    "dft2-across-rows": ["pass-4096/reg3+dft2-across-rows"],
    "dft4-across-rows": ["pass-2048/reg3+dft4-across-rows"],
    "rank3": ["pass-12/", "pass-20/lds:5x4", "pass-30/"],
    "rank4": ["pass-5/lds:5", "pass-4/lds:4", "pass-3/lds:3", "pass-2/lds:2"],
    "img2d": ["img2d-32x32 tile=8"],
    "img2dl": ["img2dl-64x48 tile=2"],
    "vol3d": ["vol3d-16x16x16 tile=2"],
    "img2d-r2c": ["img2d-r2c-32x32"],
    "img2d-c2r": ["img2d-c2r-32x32"],
    "vol3d-r2c": ["vol3d-r2c-16x16x16", ],
    "vol3d-c2r": ["vol3d-c2r-16x16x16"],
    "vol3d-r2c-8x8x32": ["vol3d-r2c-8x8x32"],
    "vol3d-c2r-8x8x32": ["vol3d-c2r-8x8x32"],
    "real-rows-nd": ["pass-512/r2c-rows"],
    "real-rows-nd-c2r": ["pass-512/c2r-rows"],
    "r2r-rows-nd": ["pass-128/r2c-rows+r2r-post tile=32", "r2r-post-e01 n=24"],
}


def nd_cases():
    """the nd share of the matrix: every layout of ND_LAYOUTS on the paths rank >= 2 plans take"""
    C = []
    CL, RL, QL = ND_LAYOUTS["c2c"], ND_LAYOUTS["r2c"], ND_LAYOUTS["r2r"]
    both = (-1, +1)
    blue = ["copy n=2100", "pass-2100/reg3"]
    # column-form register passes; tuned rows under a short column axis; hard lengths off the last axis
    _nd(C, "nd-col", "c2c", (1000, 12), 3, CL, ["pass-12/reg1", "pass-1000/reg3 tile=8"], signs=both)
    _nd(C, "nd-col", "c2c", (600, 6), 1, CL, ["pass-6/reg1", "pass-600/reg2"], signs=both)
    _nd(C, "nd-rows", "c2c", (5, 2048), 3, CL, ["pass-2048/reg3", "pass-5/lds:5"], signs=both)
    _nd(C, "nd-rows", "c2c", (4096, 3), 3, CL, ["pass-3/reg1", "pass-64/lds:8x8 tile=3 tw=4096"], signs=both)
    # the column form has one Bluestein form: with and without the knob, the same steps
    _nd(C, "nd-bluestein", "c2c", (1031, 6), 3, CL, blue + ["copy n=1031"], absent=["bluestein-rows"], signs=both,
        envs=[None, {"FFTW_AMD_NO_BLUE_ROWS": "1"}])
    _nd(C, "nd-lds", "c2c", (299, 8), 3, CL, ["pass-8/reg1", "pass-299/lds:23x13"], signs=both)
    _nd(C, "nd-rader", "c2c", (12289, 3), 1, CL, ["pass-3/reg1", "rader-mul n=12288"], signs=both)
    _nd(C, "nd-bluestein", "c2c", (1030, 4), 3, CL, blue + ["copy n=1030"], signs=both)
    # the two-pass split as one axis (FFTW_AMD_FORCE_LENS applies to an axis; 184 x 184 is also the planner's own)
    _nd(C, "nd-two-pass", "c2c", (184 * 184, 3), 1, CL, ["pass-3/reg1", "pass-184/lds:23x8 tile=3 tw=33856"],
        env={"FFTW_AMD_FORCE_LENS": "184,184"}, signs=both)
    # tiled transposes behind a transform: in place with exchanged strides, square (no scratch) and not
    _nd(C, "nd-transpose", "c2c", (256, 256), 3, CL + ["transposed-inplace"], ["pass-256/reg2"],
        absent=["transpose"], signs=both)
    _nd(C, "nd-transpose", "c2c", (96, 160), 3, CL + ["transposed-inplace"], ["pass-160/reg2", "pass-96/reg2"],
        absent=["transpose"], signs=both)
    # a DFT across the rows of a tile: four rows at about 2^21 points; two rows need 4096-point rows and more than
    # 1024 of them, so that case is slow.  Backward: dense and embedded keep the step, strided is the fallback
    x4 = ["pass-260/reg2", "pass-2048/reg3+dft4-across-rows"]
    x2 = ["pass-513/reg2", "pass-4096/reg3+dft2-across-rows"]
    for sign in both:
        for name in ("dense", "dense-inplace", "embedded", "strided"):
            if sign < 0 or name != "dense-inplace":
                keeps = name != "strided"
                C.append(FCase("nd-xrow", "c2c", (1040, 2048), 1, name, sign, labels=x4 if keeps else (),
                               absent=() if keeps else ["across-rows"]))
    for sign in both:
        C.append(FCase("slow-nd-xrow", "c2c", (1026, 4096), 1, "dense-inplace", sign, labels=x2))
    # ranks 3 and 4
    _nd(C, "nd-rank3", "c2c", (30, 20, 12), 3, CL, ["pass-12/reg1", "pass-20/lds:5x4", "pass-30/reg2"], signs=both)
    _nd(C, "nd-rank3", "c2c", (3, 5, 7), 3, CL, ["pass-7/lds:7", "pass-5/lds:5", "pass-3/lds:3"], signs=both)
    _nd(C, "nd-rank4", "c2c", (2, 3, 4, 5), 1, CL, ["pass-5/lds:5", "pass-4/lds:4", "pass-3/lds:3", "pass-2/lds:2"],
        signs=both)
    # one-trip steps in their exact layouts, and every other layout on the fallback path
    inpl = ("dense", "dense-inplace")
    pad = ("dense", "padded-inplace")
    _one_trip(C, "nd-img2d", "c2c", (32, 32), int(fa.lib.fa_hip_img2d_tile(32, 32)), "img2d-32x32 tile=%d"
              % fa.lib.fa_hip_img2d_tile(32, 32), exact=inpl)
    _one_trip(C, "nd-img2dl", "c2c", (64, 48), fa.img2dl_tile(64, 48), "img2dl-64x48 tile=%d" % fa.img2dl_tile(64, 48),
              exact=inpl)
    _one_trip(C, "nd-vol3d", "c2c", (16, 16, 16), fa.vol3d_tile(16, 16, 16), "vol3d-16x16x16 tile=%d"
              % fa.vol3d_tile(16, 16, 16), env={"FFTW_AMD_VOL3D": "1"}, exact=inpl)
    for kind, fwd in (("r2c", True), ("c2r", False)):
        T = fa.img2dr_tile(32, 32, fwd)
        _one_trip(C, "nd-img2dr", kind, (32, 32), T, "img2d-%s-32x32 tile=%d" % (kind, T),
                  env={"FFTW_AMD_REAL_IMG": "1"}, exact=pad)
        _nd(C, "nd-real", kind, (64, 48), 3, RL, ["pass-24/reg2", "pass-64/reg2"], gone=["img2d"])
        for shape in ((16, 16, 16), (8, 8, 32)):
            T = fa.vol3dr_tile(shape[0], shape[1], shape[2], fwd)
            _one_trip(C, "nd-vol3dr", kind, shape, T, "vol3d-%s-%s tile=%d" % (kind, "x".join(map(str, shape)), T),
                      env={"FFTW_AMD_REAL_VOL": "1"}, exact=pad)
    # real transforms in more dimensions
    for shape, lays in (((16, 9), RL), ((13, 11), RL), ((64, 64), RL), ((5, 6, 8), RL),
                        ((128, 1024), ["dense", "padded-inplace", "interleaved", "strided", "split", "split-gapped"])):
        for kind in ("r2c", "c2r"):
            lab = ["pass-512/%s-rows" % kind, "pass-128/reg2"] if shape == (128, 1024) else ()
            _nd(C, "nd-real", kind, shape, 3, lays, lab)
    # r2r in more dimensions
    _nd(C, "nd-r2r", "r2r", (12, 1000), 3, QL, ["r2r-pre-o01 n=1000", "r2r-pre-e10 n=12"], kinds=[5, 8])
    _nd(C, "nd-r2r", "r2r", (24, 256), 3, QL, ["pass-128/r2c-rows+r2r-post tile=32", "r2r-post-e01 n=24"],
        kinds=[4, 5])
    _nd(C, "nd-r2r", "r2r", (7, 9, 10), 3, QL, ["r2r-post-e00", "r2r-post-o00", "r2r-post-dht"], kinds=[3, 7, 2])
    return C


def no_transpose_cases():
    """FFTW_AMD_NO_TRANSPOSE=1 is read once per process, so these run in a process of their own
    (tests/test_gpu_footprint.py): the exchanged-stride in-place plans on the element-wise copies"""
    env = {"FFTW_AMD_NO_TRANSPOSE": "1"}
    return [FCase("nd-no-transpose", "c2c", (96, 160), 3, "transposed-inplace", env=env),
            FCase("nd-no-transpose", "c2c", (24, 24), 3, "transposed-inplace", env=env)]


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


# families whose step exists in dense arrays only: the in-place twin is the non-dense layout there is.  Every other
# family must be reached in a layout whose strides differ from the dense ones
ND_DENSE_ONLY = ("img2d", "img2dl", "vol3d", "dft2-across-rows")
ND_DENSE_LIKE = ("dense", "dense-inplace", "unaligned")


def nd_family_labels(sprint_of):
    """{family of ND_FAMILIES: id of the first case of rank >= 2 whose sprint shows all the family's labels}: a
    case in a layout whose strides differ from dense (not dense, dense-inplace or unaligned), for the families of
    ND_DENSE_ONLY the dense-inplace one; sprint_of(case) -> the case's sprint(), or None to pass the case over"""
    reached = {}
    for c in nd_cases():
        if len(c.shape) < 2 or c.dense or c.layout == "unaligned" or all(f in reached for f in ND_FAMILIES):
            continue
        open_f = [f for f in ND_FAMILIES if f not in reached and
                  (c.layout not in ND_DENSE_LIKE or f in ND_DENSE_ONLY)]
        s = sprint_of(c) if open_f else None
        for f in open_f:
            if s and all(lab in s for lab in ND_FAMILIES[f]):
                reached[f] = c.id
    return reached
