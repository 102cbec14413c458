"""Registers, spills, LDS and private-segment size of every vol3d_kernel instantiation (pass3d.hpp), from the compiler's
own resource-usage remarks: compiles fftw3_amd/csrc/kernels_vol.hip for gfx950 once more (no GPU needed) and writes
profiles/vol3d_codeobj.txt.  An entry that spills is to be dropped from vol3d_menu.inc.

The column `way` is the LDS bank-conflict degree of the kernel's layout, counted here by enumeration and not read from
a hardware counter: for each of the four lane patterns of pass3d.hpp (A: stores of stage 1, B: loads and stores of
stage 2, C: loads and stores of stage 3, D: loads of the transposition) and every group of 32 consecutive work-items of
the tile, ragged groups included, the largest number of distinct 64-bit words that fall on one of the 32 banks.

    python tools/perf/vol3d_codeobj.py [--log remarks.txt]     (--log: parse a saved compiler output instead)
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def remarks():
    if "--log" in sys.argv:
        with open(sys.argv[sys.argv.index("--log") + 1]) as f:
            return f.read()
    cmd = [HIPCC, "-O3", "-fPIC", "--offload-arch=gfx950", "-Iinclude", "-Ifftw3_amd/csrc", "-std=c++17", "-Wall",
           "-Rpass-analysis=kernel-resource-usage", "-c", "fftw3_amd/csrc/kernels_vol.hip", "-o", os.devnull]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout)
        raise SystemExit("compilation failed")
    return r.stdout


def ways(R0, R1, R2, T, S, SP):
    """"A/B/C/D" conflict degrees of the layout (t R0 + a0) SP + a1 S + a2"""
    P, V = R1 * R2, R0 * R1 * R2

    def addr(t, a0, a1, a2):
        return (t * R0 + a0) * SP + a1 * S + a2

    def worst(n, f):
        idx = np.minimum(np.arange(-(-n // 256) * 256), n - 1)     # items beyond the count redo the last one
        return max(int(np.bincount(np.unique(row) % 32, minlength=32).max()) for row in f(idx).reshape(-1, 32))

    return (worst(T * P, lambda g: addr(g // P, 0, (g % P) // R2, g % R2)),
            worst(T * R0 * R2, lambda h: addr(h // (R0 * R2), (h % (R0 * R2)) // R2, 0, h % R2)),
            worst(T * R0 * R1, lambda q: addr(q // (R0 * R1), (q % (R0 * R1)) // R1, q % R1, 0)),
            worst(T * V, lambda e: addr(e // V, (e % V) // P, (e % P) // R2, e % R2)))


def main():
    import fftw3_amd as fa
    rows = []
    for blk in remarks().split("Function Name: ")[1:]:
        # _Z12vol3d_kernelILi4ELi8ELi16ELb0EEv9Vol3DArgs
        m = re.match(r"_Z12vol3d_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E", blk)
        if not m:
            continue
        n0, n1, n2, bwd = (int(v) for v in m.groups())

        def g(key):
            return int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
        T = fa.vol3d_tile(n0, n1, n2)
        s, sp = C.c_int(), C.c_int()
        lds = int(fa.lib.fa_hip_vol3d_lds(n0, n1, n2, C.byref(s), C.byref(sp)))
        w = ways(n0, n1, n2, T, s.value, sp.value)
        rows.append((n0, n1, n2, bwd, T, T * n0 * n1 * n2, g("VGPRs"), g("AGPRs"), g("VGPRs Spill"), g("SGPRs Spill"),
                     g("ScratchSize [bytes/lane]"), lds, s.value, sp.value, "%d/%d/%d/%d" % w,
                     g("Occupancy [waves/SIMD]")))
    rows.sort()
    out = ["# vol3d_kernel<n0, n1, n2, BWD> (fftw3_amd/csrc/pass3d.hpp), hipcc -O3 --offload-arch=gfx950, 256 work-items,",
           "# __launch_bounds__(256, 2).  From -Rpass-analysis=kernel-resource-usage (tools/perf/vol3d_codeobj.py).",
           "# T = volumes per tile, elems = T n0 n1 n2, lds = dynamic LDS bytes per workgroup (the plane), S / SP = row and",
           "# plane stride of the LDS layout in doubles, way = bank-conflict degree of the lane patterns A/B/C/D of pass3d.hpp",
           "# counted by enumeration of the addresses (no hardware counter), private = private segment (scratch) bytes per",
           "# lane.  A row with a spill or a private segment leaves vol3d_menu.inc.",
           "# %3s %3s %3s %3s %4s %6s %6s %6s %9s %9s %8s %6s %3s %5s %8s %5s" % (
               "n0", "n1", "n2", "bwd", "T", "elems", "vgprs", "agprs", "vgprspill", "sgprspill", "private", "lds", "S",
               "SP", "way", "waves")]
    for r in rows:
        out.append("  %3d %3d %3d %3d %4d %6d %6d %6d %9d %9d %8d %6d %3d %5d %8s %5d" % r)
    bad = [r for r in rows if r[8] or r[9] or r[10]]
    over = [r for r in rows if max(int(v) for v in r[14].split("/")) > 2]
    out.append("# %d kernels (%d sizes x forward / backward), %d with a spill or a private segment, %d above two-way" %
               (len(rows), len(rows) // 2, len(bad), len(over)))
    with open(os.path.join(ROOT, "profiles", "vol3d_codeobj.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    print(out[-1])


if __name__ == "__main__":
    main()
