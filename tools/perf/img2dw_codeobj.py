"""Registers, spills, LDS and private-segment size of every img2dw_kernel instantiation (pass2dw.hpp), from the compiler's
own resource-usage remarks: compiles fftw3_amd/csrc/kernels_imgw.hip for gfx950 (no GPU needed), once per split of the
128-point axis (FA_IMG2DW_A128 = 16: 16 x 8, the one that is built; 8: 8 x 16), and writes profiles/img2dw_codeobj.txt.
An entry that spills is to be dropped from img2dw_menu.inc.

    python tools/perf/img2dw_codeobj.py
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def remarks(a128):
    cmd = [HIPCC, "-O3", "-fPIC", "--offload-arch=gfx950", "-Iinclude", "-Ifftw3_amd/csrc", "-std=c++17", "-Wall",
           "-DFA_IMG2DW_A128=%d" % a128, "-Rpass-analysis=kernel-resource-usage", "-c", "fftw3_amd/csrc/kernels_imgw.hip",
           "-o", os.devnull]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout)
        raise SystemExit("compilation failed")
    return r.stdout


def main():
    rows = []
    for a128 in (16, 8):
        for blk in remarks(a128).split("Function Name: ")[1:]:
            # _Z13img2dw_kernelILi64ELi128ELb0ELb1EEv10Img2DLArgs
            m = re.match(r"_Z13img2dw_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E", blk)
            if not m:
                continue
            n0, n1, bwd, nt = (int(v) for v in m.groups())

            def g(key):
                return int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
            T = 16384 // (n0 * n1)
            lds = (n0 * T * (n1 | 1) + 16) * 8
            rows.append((a128, n0, n1, bwd, nt, T, g("VGPRs"), g("AGPRs"), g("VGPRs Spill"), g("SGPRs Spill"),
                         g("ScratchSize [bytes/lane]"), lds, g("Occupancy [waves/SIMD]")))
    rows.sort(key=lambda r: (-r[0],) + r[1:])
    out = ["# img2dw_kernel<n0, n1, BWD, NT_OUT> (fftw3_amd/csrc/pass2dw.hpp), hipcc -O3 --offload-arch=gfx950, 512 work-items,",
           "# __launch_bounds__(512, 1), a tile of 16384 elements.  From -Rpass-analysis=kernel-resource-usage",
           "# (tools/perf/img2dw_codeobj.py).  a128 = first-stage radix of a 128-point axis (16: 128 = 16 x 8, what the library",
           "# builds; 8: 128 = 8 x 16, compiled for comparison only), T = images per tile, lds = dynamic LDS bytes per",
           "# workgroup (the plane), private = private segment (scratch) bytes per lane.  A row with a spill or a private",
           "# segment leaves img2dw_menu.inc.",
           "# %4s %3s %3s %3s %2s %2s %6s %6s %9s %9s %8s %7s %5s" % ("a128", "n0", "n1", "bwd", "nt", "T", "vgprs", "agprs",
                                                                     "vgprspill", "sgprspill", "private", "lds", "waves")]
    for r in rows:
        out.append("  %4d %3d %3d %3d %2d %2d %6d %6d %9d %9d %8d %7d %5d" % r)
    bad = [r for r in rows if r[8] or r[9] or r[10]]
    out.append("# %d kernels (3 sizes x forward / backward x plain / nontemporal store x 2 splits), %d with a spill or a private segment" %
               (len(rows), len(bad)))
    with open(os.path.join(ROOT, "profiles", "img2dw_codeobj.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    print(out[-1])


if __name__ == "__main__":
    main()
