"""Registers, spills, LDS and private-segment size of every vol3dr_kernel / vol3dc_kernel instantiation (pass3dr.hpp),
from the compiler's own resource-usage remarks (the figures it writes into the code object's metadata; the instruction
stream is not looked at): compiles fftw3_amd/csrc/kernels_volr.hip for gfx950 once more (no GPU needed) and writes
profiles/vol3dr_codeobj.txt.  An entry that spills, has a private segment or an LDS access pattern above two-way is to
be dropped from vol3dr_menu.inc.

The column `way` is the LDS bank-conflict degree of every access pattern of the kernel, counted here by enumeration and
not read from a hardware counter: for every group of 32 consecutive work-items of the tile, ragged groups included
(items beyond a stage's butterfly count redo the last one; a predicated store counts its active lanes only), the largest
number of distinct 64-bit words that fall on one of the 32 banks.  The patterns, in the order of the column:
    r2c   layout X: A stores of stage 1, B loads / stores of stage 2, C loads of stage 3 (own row), Cm (row -k);
          layout O: S stores of stage 3 (own row), Sm (row -k, predicated), D loads in the order of the run
    c2r   layout C: A stores of stage A, B loads / stores of stage B, C loads of stage C (row r), Cm (row r');
          layout R: S stores of stage C (row r), Sm (row r', predicated), D / D1 loads of the words 2c / 2c + 1 in run order

    python tools/perf/vol3dr_codeobj.py [--log remarks.txt]     (--log: parse a saved compiler output instead)
    python tools/perf/vol3dr_codeobj.py --search                rewrite fftw3_amd/csrc/vol3dr_pad.inc

--search needs no library: it repeats the tile rule of pass3dr.hpp (fa_vol3dr_tile) in Python and, per menu triple and
direction, looks for the largest T and the smallest paddings (ds, dp) of the two layouts for which every pattern is at
most two-way and the C++ rule arrives at the same T.  The table mode then re-counts every entry from the strides and
the tile that the built library reports."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LDS_DOUBLES = 9216          # FA_IMG2D_LDS_DOUBLES
RUN_LIM = 32                # FA_IMG2DR_RUN_LIM


def menu():
    with open(os.path.join(ROOT, "fftw3_amd", "csrc", "vol3dr_menu.inc")) as f:
        return [tuple(int(v) for v in m.groups()) for m in re.finditer(r"X\((\d+), (\d+), (\d+)\)", f.read())]


def worst(n, f, mask=None):
    """largest number of distinct words on one bank over the 32-item groups of n butterflies"""
    idx = np.minimum(np.arange(-(-n // 256) * 256), n - 1)
    a = np.asarray(f(idx)).reshape(-1, 32)
    if mask is not None:
        a = np.where(np.asarray(mask(idx)).reshape(-1, 32), a, -1)
    a = np.sort(a, axis=1)
    first = np.ones(a.shape, dtype=bool)
    first[:, 1:] = a[:, 1:] != a[:, :-1]
    first &= a >= 0
    key = (np.arange(a.shape[0])[:, None] * 32 + (a % 32))[first]
    return int(np.bincount(key, minlength=1).max()) if key.size else 0


def ways_layout(R0, R1, R2, T, lay, S, SP):
    """conflict degrees of the patterns of layout `lay` (0 X, 1 O, 2 C, 3 R) of pass3dr.hpp"""
    H, M0, NR = R2 // 2, R0 // 2 + 1, R0 * R1
    P = (NR + 1) // 2

    def addr(t, a0, a1, a2):
        return (t * R0 + a0) * SP + a1 * S + a2

    if lay == 0 or lay == 2:
        W = H if lay == 0 else H + 1
        out = [worst(T * R1 * W, lambda g: addr(g // (R1 * W), 0, (g % (R1 * W)) // W, g % W)),
               worst(T * R0 * W, lambda h: (h // W) * SP + h % W)]
    if lay == 0 or lay == 1:
        def own(q):
            return addr(q // (M0 * R1), (q % (M0 * R1)) // R1, q % R1, 0)

        def mirror(q):
            k0, k1 = (q % (M0 * R1)) // R1, q % R1
            return addr(q // (M0 * R1), (R0 - k0) % R0, (R1 - k1) % R1, 0)

        def has_mirror(q):
            k0 = (q % (M0 * R1)) // R1
            return (k0 > 0) & (2 * k0 != R0)
        n3 = T * M0 * R1
        if lay == 0:
            return out + [worst(n3, own), worst(n3, mirror)]
        W, V = H + 1, NR * (H + 1)
        return [worst(n3, own), worst(n3, mirror, has_mirror),
                worst(T * V, lambda e: e + (e // W) * (S - W) + (e // (R1 * W)) * (SP - R1 * S))]

    def row_r(q):
        r = 2 * (q % P)
        return addr(q // P, r // R1, r % R1, 0)

    def row_rr(q):
        r = np.minimum(2 * (q % P) + 1, NR - 1)
        return addr(q // P, r // R1, r % R1, 0)

    def two(q):
        return 2 * (q % P) + 1 < NR
    if lay == 2:
        return out + [worst(T * P, row_r), worst(T * P, row_rr)]

    def run(e):
        row, c = e // H, e % H
        return (row // R1) * SP + (row % R1) * S + 2 * c
    return [worst(T * P, row_r), worst(T * P, row_rr, two), worst(T * NR * H, run), worst(T * NR * H, lambda e: run(e) + 1)]


def cdiv(a):
    return (a + 255) // 256


def lim(R, first):
    """fa_img2dr_lim"""
    base = 32 if R & (R - 1) == 0 else (32 if R == 32 else (15 if R == 15 else (30 if first else 28)))
    return max(base, R)


def regs_ok(R0, R1, R2, T, fwd):
    """the per-item and run-order limits of fa_vol3dr_fwd_ok / fa_vol3dr_bwd_ok (not the plane)"""
    H, M0, P = R2 // 2, R0 // 2 + 1, (R0 * R1 + 1) // 2
    if fwd:
        return (cdiv(T * R1 * H) * R0 <= lim(R0, True) and cdiv(T * R0 * H) * R1 <= lim(R1, False) and
                cdiv(T * M0 * R1) * R2 <= lim(R2, False) and cdiv(T * R0 * R1 * (H + 1)) <= RUN_LIM)
    return (cdiv(T * R1 * (H + 1)) * R0 <= lim(R0, True) and cdiv(T * R0 * (H + 1)) * R1 <= lim(R1, False) and
            cdiv(T * P) * R2 <= lim(R2, False) and cdiv(T * R0 * R1 * H) <= RUN_LIM)


def width(R2, lay):
    return R2 // 2 if lay == 0 else (R2 if lay == 3 else R2 // 2 + 1)


def search_one(R0, R1, R2, fwd):
    """(T, (ds, dp) of the first layout, (ds, dp) of the second) or None"""
    lays = (0, 1) if fwd else (2, 3)
    cands = sorted(((R1 * ds + dp, ds, dp) for ds in range(4) for dp in range(41)))
    treg = [T for T in range(1, 16384 // (R0 * R1 * R2) + 1) if regs_ok(R0, R1, R2, T, fwd)]

    def fits(T, lay, ds, dp):
        return T * R0 * (R1 * (width(R2, lay) + ds) + dp) <= LDS_DOUBLES

    def cpp_tile(pads):
        T = 16384 // (R0 * R1 * R2)
        while T > 0 and not (regs_ok(R0, R1, R2, T, fwd) and all(fits(T, l, *p) for l, p in zip(lays, pads))):
            T -= 1
        return T

    for T in reversed(treg):
        good = []
        for lay in lays:
            g = []
            for _, ds, dp in cands:
                if fits(T, lay, ds, dp) and max(ways_layout(R0, R1, R2, T, lay, width(R2, lay) + ds, R1 * (width(R2, lay) + ds) + dp)) <= 2:
                    g.append((ds, dp))
                    if len(g) >= 6:
                        break
            good.append(g)
        for pa in good[0]:
            for pb in good[1]:
                if cpp_tile((pa, pb)) == T:
                    return T, pa, pb
    return None


def search():
    lines = ["/* vol3dr_pad.inc -- LDS paddings of the kernels of pass3dr.hpp: P(n0, n1, n2, layout, ds, dp), layout 0 X / 1 O (r2c),",
             "   2 C / 3 R (c2r); row stride = row width + ds, plane stride = n1 x row stride + dp (doubles).  Written by",
             "   tools/perf/vol3dr_codeobj.py --search: the smallest paddings at the largest tile for which every access pattern",
             "   of the kernel is at most two-way on the 32 banks, counted by enumeration.  A triple without its entries has no",
             "   such padding and a tile of 0. */"]
    none = []
    for t in menu():
        row = []
        for fwd in (True, False):
            r = search_one(*t, fwd)
            if r is None:
                none.append(t + ("r2c" if fwd else "c2r",))
                continue
            T, pa, pb = r
            lays = (0, 1) if fwd else (2, 3)
            row += ["P(%d, %d, %d, %d, %d, %d)" % (t + (lays[0],) + pa), "P(%d, %d, %d, %d, %d, %d)" % (t + (lays[1],) + pb)]
            print("%dx%dx%d %s T=%d" % (t + ("r2c" if fwd else "c2r", T)), pa, pb, flush=True)
        if row:
            lines.append(" ".join(row))
    with open(os.path.join(ROOT, "fftw3_amd", "csrc", "vol3dr_pad.inc"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("no two-way padding:", none)


def remarks():
    if "--log" in sys.argv:
        with open(sys.argv[sys.argv.index("--log") + 1]) as f:
            return f.read()
    cmd = [HIPCC, "-O3", "-fPIC", "--offload-arch=gfx950", "-Iinclude", "-Ifftw3_amd/csrc", "-std=c++17", "-Wall",
           "-Rpass-analysis=kernel-resource-usage", "-c", "fftw3_amd/csrc/kernels_volr.hip", "-o", os.devnull]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout)
        raise SystemExit("compilation failed")
    return r.stdout


def main():
    if "--search" in sys.argv:
        search()
        return
    import fftw3_amd as fa
    rows = []
    for blk in remarks().split("Function Name: ")[1:]:
        # _Z13vol3dr_kernelILi4ELi8ELi16EEv10Vol3DRArgs
        m = re.match(r"_Z13vol3d([rc])_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", blk)
        if not m:
            continue
        fwd = m.group(1) == "r"
        n0, n1, n2 = (int(v) for v in m.groups()[1:])

        def g(key):
            return int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
        T = fa.vol3dr_tile(n0, n1, n2, fwd)
        st = (C.c_int * 4)()
        lds = int(fa.lib.fa_hip_vol3dr_lds(n0, n1, n2, 1 if fwd else 0, st))
        la, lb = (0, 1) if fwd else (2, 3)
        w = ways_layout(n0, n1, n2, T, la, st[0], st[1]) + ways_layout(n0, n1, n2, T, lb, st[2], st[3])
        rows.append((n0, n1, n2, "r2c" if fwd else "c2r", T, g("VGPRs"), g("AGPRs"), g("VGPRs Spill"), g("SGPRs Spill"),
                     g("ScratchSize [bytes/lane]"), lds, "%d/%d" % (st[0], st[1]), "%d/%d" % (st[2], st[3]),
                     "/".join(str(v) for v in w), g("Occupancy [waves/SIMD]")))
    rows.sort()
    out = ["# vol3dr_kernel<n0, n1, n2> (r2c) and vol3dc_kernel<n0, n1, n2> (c2r) (fftw3_amd/csrc/pass3dr.hpp), hipcc -O3",
           "# --offload-arch=gfx950, 256 work-items, __launch_bounds__(256, 2).  From -Rpass-analysis=kernel-resource-usage",
           "# (tools/perf/vol3dr_codeobj.py).  T = volumes per tile, lds = dynamic LDS bytes per workgroup (the plane), S/SP =",
           "# row and plane stride in doubles of the kernel's first layout (X for r2c, C for c2r) and of its second (O, R),",
           "# way = bank-conflict degree of the access patterns (r2c: A/B/C/Cm of X, S/Sm/D of O; c2r: A/B/C/Cm of C,",
           "# S/Sm/D/D1 of R) counted by enumeration of the addresses (no hardware counter), private = private segment",
           "# (scratch) bytes per lane.  A row with a spill, a private segment or a degree above two leaves vol3dr_menu.inc.",
           "# %3s %3s %3s %4s %4s %6s %6s %9s %9s %8s %6s %9s %9s %16s %5s" % (
               "n0", "n1", "n2", "dir", "T", "vgprs", "agprs", "vgprspill", "sgprspill", "private", "lds", "S/SP 1", "S/SP 2",
               "way", "waves")]
    for r in rows:
        out.append("  %3d %3d %3d %4s %4d %6d %6d %9d %9d %8d %6d %9s %9s %16s %5d" % r)
    bad = [r for r in rows if r[7] or r[8] or r[9]]
    over = [r for r in rows if max(int(v) for v in r[13].split("/")) > 2]
    out.append("# %d kernels (%d sizes x r2c / c2r), %d with a spill or a private segment, %d above two-way" %
               (len(rows), len(rows) // 2, len(bad), len(over)))
    for r in bad + over:
        out.append("#   leaves the menu: %d x %d x %d (%s)" % r[:4])
    with open(os.path.join(ROOT, "profiles", "vol3dr_codeobj.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out[-1 - len(bad + over):]))


if __name__ == "__main__":
    main()
