#!/usr/bin/env python3
"""Canonical text dump of the plans of a fixed corpus of problems (planning needs no device).

Two commits plan alike exactly when their dumps are byte-identical:

    python tools/plan_dump.py > dump.txt          # every case
    python tools/plan_dump.py --case ID           # one case
    python tools/plan_dump.py --list              # the case ids
    python tools/plan_dump.py --write             # regenerate tests/golden/plan_pins.txt

A dump holds every field of every step descriptor, every table's descriptor (its reported length, or the table it is
the DFT of -- not its contents), batch, chunk, lanes, the workspace size, the flop estimate and the plan's own
description.  No pointers, no addresses.  The planner reads the alignment of the arrays it is given, so every array
is allocated 64-byte aligned here, a few cases offset by 8 bytes on purpose; it reads its FFTW_AMD_* switches at plan
time, so they are set and restored around each case.  tests/test_plan_pins.py compares the hashes of the dumps
with tests/golden/plan_pins.txt.
"""
import argparse
import contextlib
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import fftw3_amd as fa  # noqa: E402

PINS = os.path.join(ROOT, "tests", "golden", "plan_pins.txt")


def doubles(count, off=0):
    """`count` uninitialised doubles at a 64-byte aligned address plus `off` bytes (nothing reads them)"""
    raw = np.empty(8 * int(count) + 64 + off, dtype=np.uint8)
    start = (-raw.ctypes.data) % 64 + off
    return raw[start:start + 8 * int(count)].view(np.float64)


@contextlib.contextmanager
def environment(env):
    """exactly the FFTW_AMD_* switches of `env`: the caller's own are taken out for the duration and put back"""
    old = {k: v for k, v in os.environ.items() if k.startswith("FFTW_AMD_")}
    for k in old:
        del os.environ[k]
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(old)


# ------------------------------------------------------------------ problems

def real_many(fwd, n, hm=1, rstride=1, rdist=None, cstride=1, cdist=None, inplace=False, roff=0, coff=0, flags=fa.ESTIMATE,
              doubles=doubles):
    """r2c (fwd) or c2r of the real shape n, howmany hm; strides / dists in elements of their own side;
    doubles: the allocator (a GPU test passes one that returns device memory)"""
    n = list(n)
    total, half = int(np.prod(n)), int(np.prod(n[:-1])) * (n[-1] // 2 + 1)
    if inplace:                                  # FFTW's padded layout: rows of 2 (n / 2 + 1) doubles on both sides
        rdist = 2 * half if rdist is None else rdist
        cdist = half if cdist is None else cdist
        c = doubles(2 * cdist * hm, coff)
        r = c
        inembed = n[:-1] + [2 * (n[-1] // 2 + 1)]
    else:
        rdist = total if rdist is None else rdist
        cdist = half if cdist is None else cdist
        r = doubles(rstride * total + rdist * hm, roff)
        c = doubles(2 * (cstride * half + cdist * hm), coff)
        inembed = None
    if fwd:
        return fa.plan_many_dft_r2c(len(n), n, hm, r, inembed, rstride, rdist, c, None, cstride, cdist, flags)
    return fa.plan_many_dft_c2r(len(n), n, hm, c, None, cstride, cdist, r, inembed, rstride, rdist, flags)


def real_split(fwd, n, hm):
    """guru split interface: the half spectrum as two planes of reals (cut from one array: a step holds their distance)"""
    h = n // 2 + 1
    r, planes = doubles(n * hm), doubles(2 * h * hm)
    re, im = planes[:h * hm], planes[h * hm:]
    if fwd:
        return fa.plan_guru64_split_dft_r2c([(n, 1, 1)], [(hm, n, h)], r, re, im)
    return fa.plan_guru64_split_dft_c2r([(n, 1, 1)], [(hm, h, n)], re, im, r)


def r2r_many(n, kinds, hm=1, inplace=False, off=0, doubles=doubles):
    n = list(n)
    total = int(np.prod(n))
    x = doubles(total * hm, off)
    y = x if inplace else doubles(total * hm)
    return fa.plan_many_r2r(len(n), n, hm, x, None, 1, total, y, None, 1, total, list(kinds))


def c2c_many(n, hm=1, sign=fa.FORWARD, inplace=False, doubles=doubles):
    n = list(n)
    total = int(np.prod(n))
    x = doubles(2 * total * hm)
    y = x if inplace else doubles(2 * total * hm)
    return fa.plan_many_dft(len(n), n, hm, x, None, 1, total, y, None, 1, total, sign)


R2R_KINDS = [("r2hc", fa.R2HC), ("hc2r", fa.HC2R), ("dht", fa.DHT), ("redft00", fa.REDFT00), ("redft01", fa.REDFT01),
             ("redft10", fa.REDFT10), ("redft11", fa.REDFT11), ("rodft00", fa.RODFT00), ("rodft01", fa.RODFT01),
             ("rodft10", fa.RODFT10), ("rodft11", fa.RODFT11)]

DEC = {"FFTW_AMD_REAL_DEC": "1"}
NOROWS = {"FFTW_AMD_NO_R2CROWS": "1"}
FORCE4 = {"FFTW_AMD_FORCE_RADIX4": "1"}
UNFUSED = {"FFTW_AMD_R2R_UNFUSED": "1"}


def corpus():
    """[(case id, environment, function that returns the plan)], the smallest sizes that reach each planner branch"""
    cases = []

    def add(cid, env, fn, *a, **k):
        cases.append((cid, dict(env), lambda: fn(*a, **k)))

    for d, fwd in (("r2c", True), ("c2r", False)):
        # odd lengths: the full complex transform of the real sequence
        add(d + "-15", {}, real_many, fwd, [15])
        add(d + "-15x4", {}, real_many, fwd, [15], 4)
        # even lengths on the general untangle / tangle path
        add(d + "-10000", {}, real_many, fwd, [10000])
        add(d + "-10000x4-norows", NOROWS, real_many, fwd, [10000], 4)
        add(d + "-512x8-norows", NOROWS, real_many, fwd, [512], 8)
        add(d + "-512x8-split", {}, real_split, fwd, 512, 8)
        add(d + "-512x8-unaligned-flag", {}, real_many, fwd, [512], 8, flags=fa.ESTIMATE | fa.UNALIGNED)
        # one-trip rows: short rows (dense, padded in place), two-stage power of two, mixed two-stage, three-stage
        add(d + "-16x256", {}, real_many, fwd, [16], 256)
        add(d + "-16x256-inplace", {}, real_many, fwd, [16], 256, inplace=True)
        add(d + "-16x255", {}, real_many, fwd, [16], 255)
        add(d + "-16x256-no-r1", {"FFTW_AMD_NO_R1": "1"}, real_many, fwd, [16], 256)
        add(d + "-512x8", {}, real_many, fwd, [512], 8)
        add(d + "-512x8-inplace", {}, real_many, fwd, [512], 8, inplace=True)
        add(d + "-200x8", {}, real_many, fwd, [200], 8)
        add(d + "-4096x4", {}, real_many, fwd, [4096], 4)
        add(d + "-4096x4-no3s", {"FFTW_AMD_NO_3S": "1"}, real_many, fwd, [4096], 4)
        add(d + "-2560x4", {}, real_many, fwd, [2560], 4)
        add(d + "-32768x2", {}, real_many, fwd, [32768], 2)
        # arrays offset by 8 bytes: the rows kernels need 16-byte alignment
        add(d + "-512x8-real-off8", {}, real_many, fwd, [512], 8, roff=8)
        add(d + "-512x8-cplx-off8", {}, real_many, fwd, [512], 8, coff=8)
        add(d + "-16x256-real-off8", {}, real_many, fwd, [16], 256, roff=8)
        # howmany with a non-unit dist, a strided last dim
        add(d + "-512x8-dist", {}, real_many, fwd, [512], 8, rdist=520, cdist=260)
        add(d + "-512x8-odd-dist", {}, real_many, fwd, [512], 8, rdist=513, cdist=257)
        add(d + "-512x4-strided", {}, real_many, fwd, [512], 4, rstride=2, rdist=1024, cstride=3, cdist=3 * 257)
        add(d + "-15x4-strided", {}, real_many, fwd, [15], 4, rstride=4, rdist=1, cstride=4, cdist=1)
        # a batch in several chunks
        add(d + "-65536x64-chunked", {"FFTW_AMD_CHUNK_BYTES": str(1 << 22)}, real_many, fwd, [65536], 64)
        add(d + "-2^20x16-chunked", {"FFTW_AMD_CHUNK_BYTES": str(1 << 25)}, real_many, fwd, [1 << 20], 16)
        # radix 4
        add(d + "-2^22", {}, real_many, fwd, [1 << 22])
        add(d + "-2^22-no-radix4", {"FFTW_AMD_NO_RADIX4": "1"}, real_many, fwd, [1 << 22])
        add(d + "-2^21x2", {}, real_many, fwd, [1 << 21], 2)
        add(d + "-64x4-force4", FORCE4, real_many, fwd, [64], 4)
        add(d + "-24x3-force4-strided", FORCE4, real_many, fwd, [24], 3, rstride=3, rdist=1, cstride=3, cdist=1)
        add(d + "-3932160", {}, real_many, fwd, [3932160])
        # decimated over the real data: three eligible lengths, the ways to fall through
        add(d + "-dec-256x2048x3", DEC, real_many, fwd, [256 * 2048], 3)
        add(d + "-dec-256x2048x3-inplace", DEC, real_many, fwd, [256 * 2048], 3, inplace=True)
        add(d + "-dec-1024x2048", DEC, real_many, fwd, [1024 * 2048])
        add(d + "-dec-2048x2048", DEC, real_many, fwd, [2048 * 2048])
        add(d + "-dec-255x2048", DEC, real_many, fwd, [255 * 2048])
        add(d + "-dec-128x2048", DEC, real_many, fwd, [128 * 2048], 2)
        add(d + "-dec-256x2048-unaligned-flag", DEC, real_many, fwd, [256 * 2048], flags=fa.ESTIMATE | fa.UNALIGNED)
        add(d + "-dec-256x2048-real-off8", DEC, real_many, fwd, [256 * 2048], roff=8)
        add(d + "-dec-256x2048-cplx-off8", DEC, real_many, fwd, [256 * 2048], coff=8)
        add(d + "-dec-256x2048x3-odd-dist", DEC, real_many, fwd, [256 * 2048], 3, rdist=256 * 2048 + 1, cdist=128 * 2048 + 1)
        add(d + "-dec-off-256x2048x3", {}, real_many, fwd, [256 * 2048], 3)
        add(d + "-dec-4x256x2048", DEC, real_many, fwd, [4, 256 * 2048])
        # two and three dimensions
        add(d + "-8x512", {}, real_many, fwd, [8, 512])
        add(d + "-8x512-inplace", {}, real_many, fwd, [8, 512], inplace=True)
        add(d + "-6x15", {}, real_many, fwd, [6, 15])
        add(d + "-300x16", {}, real_many, fwd, [300, 16])
        add(d + "-4x10000x2", {}, real_many, fwd, [4, 10000], 2)
        add(d + "-4x6x64", {}, real_many, fwd, [4, 6, 64])
        add(d + "-3x5x7x2", {}, real_many, fwd, [3, 5, 7], 2)
        add(d + "-4x6x64-force4", FORCE4, real_many, fwd, [4, 6, 64])

    # r2r: every kind at an even and an odd length, fused and not, 256 rows (the fused rows kernel), and a short batch
    for name, kind in R2R_KINDS:
        for n in (128, 65):
            add("r2r-%s-%dx256" % (name, n), {}, r2r_many, [n], [kind], 256)
            add("r2r-%s-%dx256-unfused" % (name, n), UNFUSED, r2r_many, [n], [kind], 256)
        add("r2r-%s-15x3" % name, {}, r2r_many, [15], [kind], 3)
        add("r2r-%s-3000x4" % name, {}, r2r_many, [3000], [kind], 4)
    add("r2r-rodft00-63x256", {}, r2r_many, [63], [fa.RODFT00], 256)
    add("r2r-redft10-128x256-inplace", {}, r2r_many, [128], [fa.REDFT10], 256, inplace=True)
    add("r2r-redft01-128x256-inplace", {}, r2r_many, [128], [fa.REDFT01], 256, inplace=True)
    add("r2r-redft10-128x256-off8", {}, r2r_many, [128], [fa.REDFT10], 256, off=8)
    add("r2r-redft01-128x256-off8", {}, r2r_many, [128], [fa.REDFT01], 256, off=8)
    add("r2r-redft10-128x256-norows", NOROWS, r2r_many, [128], [fa.REDFT10], 256)
    add("r2r-redft01-128x256-norows", NOROWS, r2r_many, [128], [fa.REDFT01], 256)
    add("r2r-redft10-64x4-force4", FORCE4, r2r_many, [64], [fa.REDFT10], 4)
    add("r2r-redft01-64x4-force4", FORCE4, r2r_many, [64], [fa.REDFT01], 4)
    add("r2r-r2hc-2^22", {}, r2r_many, [1 << 22], [fa.R2HC])
    add("r2r-hc2r-dec-256x2048", DEC, r2r_many, [256 * 2048], [fa.HC2R], 3)
    add("r2r-redft10-rodft01-8x128", {}, r2r_many, [8, 128], [fa.REDFT10, fa.RODFT01])
    add("r2r-redft00-dht-rodft11-4x6x10", {}, r2r_many, [4, 6, 10], [fa.REDFT00, fa.DHT, fa.RODFT11])

    # c2c: one, two and three passes, Rader, Bluestein step by step and as rows; their emitters share the helpers
    add("c2c-4096x8", {}, c2c_many, [4096], 8)
    add("c2c-3000x4", {}, c2c_many, [3000], 4)
    add("c2c-65536x2", {}, c2c_many, [65536], 2)
    add("c2c-65536x2-backward-inplace", {}, c2c_many, [65536], 2, fa.BACKWARD, True)
    add("c2c-1000000", {}, c2c_many, [1000000])
    add("c2c-2^22", {}, c2c_many, [1 << 22])
    add("c2c-2^22-no-tuned", {"FFTW_AMD_NO_TUNED": "1"}, c2c_many, [1 << 22])
    add("c2c-rader-97x8", {}, c2c_many, [97], 8)
    add("c2c-rader-97", {}, c2c_many, [97])
    add("c2c-bluestein-1031", {}, c2c_many, [1031])
    add("c2c-bluestein-rows-1031x8", {}, c2c_many, [1031], 8)
    add("c2c-bluestein-1031x8-no-rows", {"FFTW_AMD_NO_BLUE_ROWS": "1"}, c2c_many, [1031], 8, fa.BACKWARD)
    add("c2c-64x97", {}, c2c_many, [64, 97])
    add("c2c-8x16x32x2", {}, c2c_many, [8, 16, 32], 2)

    # every test switch the planner reads while it builds the steps flips at least one plan (KNOB_TWINS), and the
    # traps of their truth rules: the NO_* hooks are presence-tested (=0 still switches the feature off);
    # FORCE_LENS is void when malformed or when its product is not the length, and is read up to four entries only
    add("c2c-2^22-no-tuned-0", {"FFTW_AMD_NO_TUNED": "0"}, c2c_many, [1 << 22])
    add("c2c-bluestein-1031x8-no-blue-rows", {"FFTW_AMD_NO_BLUE_ROWS": "1"}, c2c_many, [1031], 8)
    add("c2c-2^21x2", {}, c2c_many, [1 << 21], 2)
    add("c2c-2^21x2-no-narrow", {"FFTW_AMD_NO_NARROW": "1"}, c2c_many, [1 << 21], 2)
    add("c2c-65536x2-no-split-costs", {"FFTW_AMD_NO_SPLIT_COSTS": "1"}, c2c_many, [65536], 2)
    add("c2c-4096x8-no-3s", {"FFTW_AMD_NO_3S": "1"}, c2c_many, [4096], 8)
    add("c2c-2048x2048", {}, c2c_many, [2048, 2048])
    add("c2c-2048x2048-no-lo-dft", {"FFTW_AMD_NO_LO_DFT": "1"}, c2c_many, [2048, 2048])
    add("c2c-16x16x64", {}, c2c_many, [16, 16], 64)
    add("c2c-16x16x64-no-img2d", {"FFTW_AMD_NO_IMG2D": "1"}, c2c_many, [16, 16], 64)
    add("c2c-4096x8-force-64x64", {"FFTW_AMD_FORCE_LENS": "64,64"}, c2c_many, [4096], 8)
    add("c2c-4096x8-force-malformed", {"FFTW_AMD_FORCE_LENS": "32,x"}, c2c_many, [4096], 8)
    add("c2c-4096x8-force-other-product", {"FFTW_AMD_FORCE_LENS": "64,32"}, c2c_many, [4096], 8)
    add("c2c-4096x8-force-five-entries", {"FFTW_AMD_FORCE_LENS": "8,8,8,8,2"}, c2c_many, [4096], 8)
    return cases


# knob -> (a case planned with it, the same problem's case without it): their plans differ (tests/test_plan_pins.py)
KNOB_TWINS = {
    "FFTW_AMD_NO_TUNED": ("c2c-2^22-no-tuned", "c2c-2^22"),
    "FFTW_AMD_NO_3S": ("c2c-4096x8-no-3s", "c2c-4096x8"),
    "FFTW_AMD_NO_R1": ("r2c-16x256-no-r1", "r2c-16x256"),
    "FFTW_AMD_NO_BLUE_ROWS": ("c2c-bluestein-1031x8-no-blue-rows", "c2c-bluestein-rows-1031x8"),
    "FFTW_AMD_NO_NARROW": ("c2c-2^21x2-no-narrow", "c2c-2^21x2"),
    "FFTW_AMD_NO_SPLIT_COSTS": ("c2c-65536x2-no-split-costs", "c2c-65536x2"),
    "FFTW_AMD_NO_LO_DFT": ("c2c-2048x2048-no-lo-dft", "c2c-2048x2048"),
    "FFTW_AMD_NO_IMG2D": ("c2c-16x16x64-no-img2d", "c2c-16x16x64"),
    "FFTW_AMD_NO_R2CROWS": ("r2c-512x8-norows", "r2c-512x8"),
    "FFTW_AMD_R2R_UNFUSED": ("r2r-redft10-128x256-unfused", "r2r-redft10-128x256"),
    "FFTW_AMD_NO_RADIX4": ("r2c-2^22-no-radix4", "r2c-2^22"),
    "FFTW_AMD_FORCE_RADIX4": ("r2c-4x6x64-force4", "r2c-4x6x64"),
    "FFTW_AMD_FORCE_LENS": ("c2c-4096x8-force-64x64", "c2c-4096x8"),
}

# (case, the case whose plan it must equal): what the truth rules make of a switch's value
KNOB_SAME = [
    ("c2c-2^22-no-tuned-0", "c2c-2^22-no-tuned"),
    ("c2c-4096x8-force-malformed", "c2c-4096x8"),
    ("c2c-4096x8-force-other-product", "c2c-4096x8"),
]


# ---------------------------------------------------------------------- dump

def _value(v):
    return ",".join(str(x) for x in v) if hasattr(v, "__len__") else str(v)


def dump_plan(p):
    """(text, number of steps)"""
    out = ["batch=%d chunk=%d lanes=%d workspace_bytes=%d" % (p.batch, p.chunk, p.lanes, p.workspace_bytes),
           "flops=%s" % ",".join(repr(x) for x in p.flops()), "sprint:", p.sprint()]
    probe, tid = (ctypes.c_double * 1)(), 0
    while True:
        n = fa.lib.fftw_amd_plan_table(p.handle, tid, probe, 1)
        if n < 0:
            break
        # 0 = a table the device has yet to compute, its source in probe[0] (as Plan.table() reads it; an empty
        # permutation table would report 0 too, which no plan holds)
        out.append("table %d: doubles=%d" % (tid, n) if n else "table %d: dft_of %d" % (tid, int(probe[0])))
        tid += 1
    steps = p.steps()
    for i, s in enumerate(steps):
        out.append("step %d: " % i + " ".join("%s=%s" % (f[0], _value(getattr(s, f[0]))) for f in fa.StepDesc._fields_))
    return "\n".join(out) + "\n", len(steps)


def dump_case(case):
    cid, env, make = case
    with environment(env):
        p = make()
        text, nsteps = dump_plan(p)
        p.destroy()
    head = "case %s\nenv %s\n" % (cid, " ".join("%s=%s" % kv for kv in sorted(env.items())) or "-")
    return head + text, nsteps


def pin_line(case):
    text, nsteps = dump_case(case)
    return "%s %d %s" % (case[0], nsteps, hashlib.sha256(text.encode()).hexdigest())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", help="dump this case only")
    ap.add_argument("--list", action="store_true", help="print the case ids")
    ap.add_argument("--pins", action="store_true", help="print one line per case: id, step count, SHA-256 of its dump")
    ap.add_argument("--write", action="store_true", help="write those lines to tests/golden/plan_pins.txt")
    a = ap.parse_args()
    cases = corpus()
    if a.case:
        cases = [c for c in cases if c[0] == a.case]
        if not cases:
            sys.exit("no such case: %s" % a.case)
    if a.list:
        print("\n".join(c[0] for c in cases))
    elif a.pins or a.write:
        lines = [pin_line(c) for c in cases]
        if a.write:
            with open(PINS, "w") as f:
                f.write("\n".join(lines) + "\n")
        else:
            print("\n".join(lines))
    else:
        nsteps = 0
        for c in cases:
            text, k = dump_case(c)
            nsteps += k
            sys.stdout.write(text + "\n")
        sys.stderr.write("%d cases, %d steps\n" % (len(cases), nsteps))


if __name__ == "__main__":
    main()
