"""The GPU accuracy case matrix and its runners (tests/accuracy.py).

One Case is one plan: a kernel family, a transform and layout, the forcing knobs, and the substrings its sprint() must
show so that a planner change cannot move a case off its family.  run_gpu() executes it on the GPU and measure() rates the
plan, the oracle and numpy.fft against the same long-double reference.  The matrix is shared by
tests/test_gpu_accuracy.py (the gate), tests/test_accuracy_ref.py (the references against each other, on the CPU)
and tools/perf/accuracy_table.py (the recorded table).
"""
import os
import re
from contextlib import contextmanager

import numpy as np

import accuracy as A
from util import ROOT, crand, oracle_c2r, oracle_dft, oracle_r2c, oracle_r2r, rrand

CSRC = os.path.join(ROOT, "fftw3_amd", "csrc")
R2R_TAG = ["post-r2hc", "pre-hc2r", "post-dht", "post-e00", "post-e01", "post-e10", "post-e11",
           "post-o00", "post-o01", "post-o10", "post-o11"]
# the one-trip real-rows kernels with r2r hooks (r2crows.hpp with r2r_epi.hpp): rows per workgroup R2CRGeom<R1, R2>::T
# for each half length L, and per r2r kind the step's label and the r2r length n whose inner real DFT has 2L points
R2R_ROWS_TILE = {64: 64, 128: 32, 256: 16, 512: 8, 1024: 4}
R2R_ROWS = {0: ("r2c-rows+r2r-post", 2, 0), 2: ("r2c-rows+r2r-post", 2, 0), 5: ("r2c-rows+r2r-post", 2, 0),
            9: ("r2c-rows+r2r-post", 2, 0), 3: ("r2c-rows+r2r-post", 1, 1), 7: ("r2c-rows+r2r-post", 1, -1),
            1: ("c2r-rows+r2r-pre", 2, 0), 4: ("c2r-rows+r2r-pre+post", 2, 0), 8: ("c2r-rows+r2r-pre+post", 2, 0)}
R2R_ROWS_ABSENT = ["(r2r-", "untangle", "tangle", "(copy"]


def r2r_rows(L, k):
    """(n, hm, tile, label) of r2r kind k on the one-trip rows kernel of half length L: two full tiles and a ragged
    one; the label ends in the tile so that "r2r-pre" cannot match a "r2r-pre+post" step"""
    name, mul, add = R2R_ROWS[k]
    T = R2R_ROWS_TILE[L]
    return mul * L + add, 2 * T + 3, T, "pass-%d/%s tile=%d" % (L, name, T)


def _menu(name, nfields):
    pat = r"X\(" + ", ".join([r"(\d+)"] * nfields) + r"\)"
    with open(os.path.join(CSRC, name)) as f:
        return [int(m.group(1)) for m in re.finditer(pat, f.read())]


def _largest_fitting_hard_length(nb, lo):
    """largest n with 2n - 1 <= nb, above lo, whose largest prime factor exceeds 31 (so the planner needs
    Bluestein); the rule of tests/test_gpu_menu.py"""
    def lpf(v):
        p, best = 2, 1
        while p * p <= v:
            while v % p == 0:
                best, v = p, v // p
            p += 1
        return max(best, v) if v > 1 else best
    n = (nb + 1) // 2
    while n > lo and lpf(n) <= 31:
        n -= 1
    return n if n > lo else 0


class Case(object):
    def __init__(self, fam, kind, shape, hm=1, sign=-1, labels=(), env=None, col=False, r2r=None, padded=False,
                 slow=False, absent=(), tile=None, linf=False):
        self.fam, self.kind, self.shape, self.hm, self.sign = fam, kind, tuple(shape), hm, sign
        self.labels, self.absent, self.env = tuple(labels), tuple(absent), dict(env or {})
        self.col, self.r2r, self.padded, self.slow = col, r2r, padded, slow
        # tile: the plan is one step of this tile, the batch two full tiles and a ragged one (check_plan);
        # linf: the result also meets the relative L-infinity bound of util.TOL against the oracle (check_linf)
        self.tile, self.linf = tile, linf

    @property
    def n(self):
        return int(np.prod(self.shape))

    @property
    def id(self):
        s = "%s-%s-%s-hm%d" % (self.fam, self.kind, "x".join(str(v) for v in self.shape), self.hm)
        if self.kind in ("c2c", "slab"):
            s += "-fwd" if self.sign < 0 else "-bwd"
        if self.r2r is not None:
            s += "-k%d" % self.r2r
        if self.col:
            s += "-col"
        if self.padded:
            s += "-inplace"
        for k, v in sorted(self.env.items()):
            s += "-%s=%s" % (k.replace("FFTW_AMD_", "").lower(), v)
        return s

    def __repr__(self):
        return self.id


def cases():
    C = []
    # pass1r: dense rows of 2 ... 32, the batch shapes of test_one_stage_rows_kernel
    for L in range(2, 33):
        tile = 256 * (6 if L == 4 else min(8, 32 // L))
        C.append(Case("pass1r", "c2c", (L,), 2 * tile + 257, labels=["pass-%d/reg1" % L]))
        C.append(Case("pass1r", "c2c", (L,), tile + 3, +1, labels=["pass-%d/reg1" % L]))
    # passrr: every rr_menu.inc length as contiguous rows (a three-stage rows kernel may take 525 ... 648)
    rr = _menu("rr_menu.inc", 3)
    r3 = _menu("r3_menu.inc", 4)
    for L in rr:
        env = {"FFTW_AMD_NO_R1": "1"} if L <= 32 else {}
        lab = "pass-%d/reg3" % L if L in r3 else "pass-%d/reg2" % L
        C.append(Case("passrr", "c2c", (L,), 67, labels=[lab], env=env))
    C.append(Case("passrr", "c2c", (120,), 67, +1, labels=["pass-120/reg2"]))
    # passrr: two-pass L x L (input twiddle, two-level table), forced split
    for L in (16, 32, 64, 128, 256, 512, 36, 100, 136, 152, 184, 360):
        kern = "lds:" if L == 16 else "reg2"                    # 16 x 16 runs on the LDS kernel
        C.append(Case("passrr-2pass", "c2c", (L * L,), 3, labels=["pass-%d/%s" % (L, kern), "tw=%d" % (L * L)],
                      env={"FFTW_AMD_FORCE_LENS": "%d,%d" % (L, L)}))
    C.append(Case("passrr-2pass", "c2c", (184 * 184,), 3, +1, labels=["pass-184/reg2", "tw=%d" % (184 * 184)],
                  env={"FFTW_AMD_FORCE_LENS": "184,184"}))
    # pass3g / pass3s / pass3w: every r3 / r3w menu length as rows, rows of 2048 ... 16384
    for L in r3 + _menu("r3w_menu.inc", 4) + [2048, 4096, 8192, 16384]:
        hm = max(3, (1 << 16) // L) | 1
        C.append(Case("pass3", "c2c", (L,), hm, labels=["pass-%d/reg3" % L]))
    C.append(Case("pass3", "c2c", (4096,), 17, +1, labels=["pass-4096/reg3"]))
    C.append(Case("pass3", "c2c", (10000,), 5, +1, labels=["pass-10000/reg3"]))
    # pass3t: every r3t_menu length in its single column form (interleaved batch, stride = howmany)
    for L in _menu("r3t_menu.inc", 4):
        C.append(Case("pass3t", "c2c", (L,), 300 if L <= 1024 else 67, col=True, labels=["pass-%d/reg3" % L]))
    C.append(Case("pass3t", "c2c", (1000,), 300, +1, col=True, labels=["pass-1000/reg3"]))
    # pass1024: the benchmark's plan, a batch over the 8-transform chunk on both lanes, and on one lane
    p1024 = ["pass-1024/reg32x32 tile=8 buf0", "pass-1024/reg32x32 tile=8 tw=1048576"]
    C.append(Case("pass1024", "c2c", (1 << 20,), 9, labels=p1024, slow=True))
    C.append(Case("pass1024", "c2c", (1 << 20,), 9, labels=p1024, env={"FFTW_AMD_LANES": "1"}, slow=True))
    C.append(Case("pass1024", "c2c", (1 << 20,), 2, +1, labels=p1024))
    # wide and long plans
    C.append(Case("wide", "c2c", (1 << 21,), 3, labels=["pass-2048/reg3", "pass-1024/reg32x32 tile=8 tw=2097152"],
                  slow=True))
    C.append(Case("wide", "c2c", (1 << 22,), 2, labels=["pass-2048/reg3 tile=8 buf0", "pass-2048/reg3 tile=8 tw=4194304"],
                  slow=True))
    C.append(Case("wide", "c2c", (1 << 22,), 2, +1, labels=["pass-2048/reg3 tile=8 tw=4194304"], slow=True))
    C.append(Case("three-pass", "c2c", (1 << 23,), 1, labels=["tw=8388608", "tw=65536", "pass-512/reg2"], slow=True))
    C.append(Case("three-pass", "c2c", (15375360,), 1, labels=["pass-192/reg2", "pass-520/reg2", "pass-154/reg2"],
                  slow=True))
    # pass3q / XROW: rows with a DFT across the rows of a tile
    C.append(Case("xrow", "c2c", (2048, 4096), 1, labels=["pass-4096/reg3+dft2-across-rows"], slow=True))
    C.append(Case("xrow", "c2c", (4096, 4096), 1, labels=["pass-4096/reg3+dft4-across-rows"], slow=True))
    C.append(Case("xrow", "c2c", (2048, 4096), 1, +1, labels=["pass-4096/reg3+dft2-across-rows"], slow=True))
    # LDS kernel: radices 11 and 13, in-LDS prime stages 17 ... 31
    for L, rad in ((55, "11x5"), (363, "11x11x3"), (65, "13x5"), (169, "13x13"), (299, "23x13"), (544, "17x8x4"),
                   (928, "29x8x4"), (992, "31x8x4")):
        C.append(Case("lds", "c2c", (L,), 20, labels=["pass-%d/lds:%s" % (L, rad)]))
    C.append(Case("lds", "c2c", (299,), 20, +1, labels=["pass-299/lds:23x13"]))
    # Bluestein rows: the length each padded size of blue_menu.inc / bluew_menu.inc is picked for
    blue = _menu("blue_menu.inc", 4) + _menu("bluew_menu.inc", 4)
    for i, nb in enumerate(blue):
        n = _largest_fitting_hard_length(nb, (blue[i - 1] + 1) // 2 if i else 200)
        if n:
            C.append(Case("bluestein", "c2c", (n,), 2 * max(1, 8192 // nb) + 1,
                          labels=["pass-%d/bluestein-rows n=%d" % (nb, n)]))
    C.append(Case("bluestein", "c2c", (1031,), 5, +1, labels=["bluestein-rows n=1031"]))
    C.append(Case("bluestein-steps", "c2c", (1031,), 5, labels=["copy n=2100", "pass-2100/reg3"],
                  absent=["bluestein-rows"], env={"FFTW_AMD_NO_BLUE_ROWS": "1"}))
    C.append(Case("rader", "c2c", (65537,), 1, labels=["rader-mul n=65536"]))
    C.append(Case("rader", "c2c", (65537,), 1, +1, labels=["rader-mul n=65536"]))
    C.append(Case("rader", "c2c", (12289,), 3, labels=["rader-mul n=12288"]))
    # real transforms
    C.append(Case("real-untangle4", "r2c", (1 << 22,), 1, labels=["r2c-untangle4"], slow=True))
    C.append(Case("real-untangle4", "c2r", (1 << 22,), 1, labels=["c2r-tangle4"], slow=True))
    C.append(Case("real-untangle", "r2c", (1 << 20,), 1, labels=["r2c-untangle n=1048576"]))
    C.append(Case("real-untangle", "c2r", (1 << 20,), 1, labels=["c2r-tangle n=1048576"]))
    C.append(Case("real-dec", "r2c", (1 << 22,), 1, labels=["reg3+real-decimated"], env={"FFTW_AMD_REAL_DEC": "1"},
                  slow=True))
    for L in _menu("r2cr_menu.inc", 3) + _menu("r3rw_menu.inc", 4) + [2048, 4096, 8192, 16384]:
        hm = 11 if L > 648 else 4096 // L * 2 + 3
        C.append(Case("real-rows", "r2c", (2 * L,), hm, labels=["pass-%d/r2c-rows" % L]))
        C.append(Case("real-rows", "c2r", (2 * L,), hm, labels=["pass-%d/c2r-rows" % L]))
    C.append(Case("real-rows", "r2c", (8192,), 11, labels=["pass-4096/r2c-rows"], padded=True))
    C.append(Case("real-odd", "r2c", (1009,), 5, labels=["rader-mul n=1008"]))
    C.append(Case("real-odd", "c2r", (1009,), 5, labels=["herm-expand n=1009", "rader-mul n=1008"]))
    # r2r: the eleven kinds
    for n in (16, 15, 1000, 243, 4096):
        for k in range(11):
            C.append(Case("r2r", "r2r", (n,), 3, r2r=k, labels=["r2r-" + R2R_TAG[k]]))
    # r2r-rows: the nine kinds whose whole axis is one launch of the fused real-rows kernel (in-row gather of the
    # Makhoul / padded sequence, real DFT, epilogue or prologue with the modulus-4n twiddle, DCT-III / DST-III store
    # shuffle), every half length of the kernel, two full tiles and a ragged one
    for L in sorted(R2R_ROWS_TILE):
        for k in sorted(R2R_ROWS):
            n, hm, T, lab = r2r_rows(L, k)
            C.append(Case("r2r-rows", "r2r", (n,), hm, r2r=k, labels=[lab], absent=R2R_ROWS_ABSENT, tile=T, linf=True))
    # the single-device 1-D slab plan: slab_twiddle_kernel's global-position twiddles
    C.append(Case("slab1d", "slab", (1 << 22,), 1, labels=["pass-2048/reg3"], slow=True))
    return C


@contextmanager
def knobs(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_input(case):
    """logical input, (hm,) + shape (c2r: the half spectra); a fixed function of kind, shape and batch, so that
    cases which differ only in knobs or direction share it (and their long-double reference)"""
    rng = np.random.default_rng(_seed("%s-%s-%d" % (case.kind, case.shape, case.hm)))
    n, hm = case.n, case.hm
    if case.kind in ("r2c", "r2r"):
        return rrand(rng, hm, n)
    if case.kind == "c2r":
        return crand(rng, hm, n // 2 + 1)
    return crand(rng, hm, n).reshape((hm,) + case.shape)


def _seed(s):
    h = 0
    for ch in s.encode():
        h = (h * 131 + ch) % (1 << 31)
    return h


_LD = {}


def ref_ld(case, x):
    """long-double reference, cached per session (several cases share one input and transform)"""
    key = (case.kind, case.shape, case.hm, case.sign, case.r2r, x.shape, x.reshape(-1)[:4].tobytes())
    if key in _LD:
        return _LD[key]
    if len(_LD) > 4:
        _LD.clear()
    n, hm = case.n, case.hm
    if case.kind in ("c2c", "slab"):
        y = A.ld_dft(x, case.shape, hm, case.sign)
    elif case.kind == "r2c":
        y = A.ld_r2c(x, n, hm)
    elif case.kind == "c2r":
        y = A.ld_c2r(x, n, hm)
    else:
        y = A.ld_r2r(x, case.r2r)
    _LD[key] = y
    return y


def ref_oracle(case, x):
    n, hm = case.n, case.hm
    if case.kind in ("c2c", "slab"):
        return oracle_dft(x.reshape(-1), case.shape, hm, case.sign).reshape(x.shape)
    if case.kind == "r2c":
        return oracle_r2c(x, (n,), hm).reshape(hm, n // 2 + 1)
    if case.kind == "c2r":
        return oracle_c2r(x.reshape(-1), (n,), hm).reshape(hm, n)
    return oracle_r2r(x.reshape(-1), [n], [case.r2r], howmany=hm).reshape(hm, n)


def _np_r2r(x, kind):
    """the r2r kinds through numpy.fft of a zero-padded embedding (unnormalised, rows of x)"""
    hm, n = x.shape
    F = np.fft.fft
    if kind == 0:
        X = np.fft.rfft(x, axis=1)
        y = np.empty_like(x)
        y[:, :n // 2 + 1] = X.real
        q = np.arange(1, (n + 1) // 2)
        y[:, n - q] = X[:, q].imag
        return y
    if kind == 1:
        X = x[:, :n // 2 + 1] + 0j
        q = np.arange(1, (n + 1) // 2)
        X[:, q] += 1j * x[:, n - q]
        return np.fft.irfft(X, n, axis=1, norm="forward")
    if kind == 2:
        X = F(x, axis=1)
        return X.real - X.imag
    if kind == 3:
        e = np.concatenate([x, x[:, -2:0:-1]], axis=1)
        return F(e, axis=1).real[:, :n]
    if kind == 7:
        z = np.zeros((hm, 2 * (n + 1)))
        z[:, 1:n + 1] = x
        z[:, n + 2:] = -x[:, ::-1]
        return -F(z, axis=1).imag[:, 1:n + 1]
    k = np.arange(n)
    if kind in (5, 9):
        z = np.zeros((hm, 4 * n))
        z[:, 2 * k + 1] = 2 * x
        Y = F(z, axis=1)
        return Y.real[:, k] if kind == 5 else -Y.imag[:, k + 1]
    if kind == 4:
        z = np.zeros((hm, 4 * n))
        z[:, 0] = x[:, 0]
        z[:, 1:n] = 2 * x[:, 1:]
        return F(z, axis=1).real[:, 2 * k + 1]
    if kind == 8:
        z = np.zeros((hm, 4 * n))
        z[:, 1:n] = 2 * x[:, :n - 1]
        z[:, n] = x[:, n - 1]
        return -F(z, axis=1).imag[:, 2 * k + 1]
    z = np.zeros((hm, 8 * n))
    z[:, 2 * k + 1] = 2 * x
    Y = F(z, axis=1)
    return Y.real[:, 2 * k + 1] if kind == 6 else -Y.imag[:, 2 * k + 1]


def ref_numpy(case, x):
    n = case.n
    axes = tuple(range(1, len(case.shape) + 1))
    if case.kind in ("c2c", "slab"):
        if case.sign < 0:
            return np.fft.fftn(x, axes=axes)
        return np.fft.ifftn(x, axes=axes, norm="forward")
    if case.kind == "r2c":
        return np.fft.rfft(x, axis=1)
    if case.kind == "c2r":
        return np.fft.irfft(x, n, axis=1, norm="forward")
    return _np_r2r(x, case.r2r)


class Guards(object):
    """what the arenas around run_gpu's device arrays saw (tests/footprint.py): violations, one entry per arena, of
    "every word outside the output footprint is bit-identical", and whether the input of an out-of-place plan came
    back bit for bit (None: in place, or a slab plan, which has its own tests)"""
    def __init__(self, violations=(), preserved=None):
        self.violations, self.preserved = list(violations), preserved


def _problem(case):
    import footprint as F
    n, hm = case.n, case.hm
    kw = dict(sign=case.sign)
    if case.kind == "c2c":
        lay = F.Layout(None, hm, 1) if case.col else F.Layout()
        return F.Problem("c2c", case.shape, hm, lay, lay, **kw)
    if case.kind == "r2c" and case.padded:
        h = n // 2 + 1
        return F.Problem("r2c", (n,), hm, F.Layout((2 * h,), 1, 2 * h), F.Layout(None, 1, h), inplace=True)
    if case.kind == "r2r":
        kw["r2r"] = [case.r2r]
    return F.Problem(case.kind, (n,), hm, F.Layout(), F.Layout(), **kw)


def run_gpu(case, x):
    """execute the case's plan on cuda:0, its device arrays inside NaN-patterned arenas (tests/footprint.py);
    returns (output in the logical layout of the reference, sprint, Guards)"""
    import torch
    import fftw3_amd as fa
    import footprint as F
    n, hm, dev = case.n, case.hm, torch.device("cuda:0")
    with knobs(case.env):
        if case.kind != "slab":
            prob = _problem(case)
            AR = prob.arenas()
            prob.scatter(AR, x)
            full = [a.to_device(dev) for a in AR]
            ref = [t.clone() for t in full]
            p = prob.plan(fa, [t[a.lo:] for t, a in zip(full, AR)])
            check_plan(case, p)
            p.execute()
            p.sync()
            torch.cuda.synchronize()
            viol = [F.check(r, t, w) for r, t, w in zip(ref, full, prob.written(AR))]
            kept = None if prob.inplace else F.same_bits(full[0], ref[0])
            out = full[-1][AR[-1].lo:AR[-1].lo + AR[-1].span].cpu().numpy()
            y = prob.gather([out])
            if case.kind == "c2c":
                y = y.reshape(x.shape)
            return y, p.sprint(), Guards(viol, kept)
        assert case.kind == "slab" and hm == 1
        xd = torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).to(dev)
        yd = torch.zeros_like(xd)
        torch.cuda.synchronize()
        sp = fa.SlabPlan1dC(n, [0], [xd], [yd], case.sign)
        s = sp.local_plan_sprint(0, 0) + "\n" + sp.local_plan_sprint(0, 1)
        sp.execute()
        sp.sync()
        y = yd.cpu().numpy().reshape(x.shape)
        sp.destroy()
        return y, s, Guards()


def measure(case, got, x):
    """rms errors of the GPU result and of both references against the long-double one, whole batch and per
    batch entry: {"gpu": e, "oracle": e, "numpy": e, "per": (e_gpu[], e_oracle[], e_numpy[])}"""
    ld = ref_ld(case, x)
    orc = ref_oracle(case, x)
    nmp = ref_numpy(case, x)
    out = {"gpu": A.rms_err(got, ld), "oracle": A.rms_err(orc, ld), "numpy": A.rms_err(nmp, ld)}
    if case.n >= 1024 and case.hm > 1:
        out["per"] = tuple(A.rms_err_per_transform(v, ld, case.hm) for v in (got, orc, nmp))
    return out


def check_labels(case, sprint):
    for lab in case.labels:
        assert lab in sprint, (case.id, lab, sprint)
    for lab in case.absent:
        assert lab not in sprint, (case.id, lab, sprint)


def check_plan(case, plan):
    """a case that names its tile: the plan is that one step, and the batch has two full tiles and a ragged one"""
    if case.tile is None:
        return
    st, T = plan.steps(), case.tile
    assert len(st) == 1, (case.id, plan.sprint())
    assert st[0].tile == T and case.hm > 2 * T and case.hm % T != 0, (case.id, st[0].tile, T, case.hm)


def check_linf(case, got, x):
    """for a case with linf set: the 1e-10 bar of the other modules, relative L-infinity against the oracle, which no
    rms dilutes (one wrong element of any row, the ragged tile's included, fails it); returns the error"""
    if not case.linf:
        return None
    from util import TOL, aerror
    e = aerror(got, ref_oracle(case, x))
    assert e <= TOL, (case.id, "relative L-infinity error against the oracle", e)
    return e
