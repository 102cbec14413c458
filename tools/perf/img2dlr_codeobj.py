"""Registers, spills, LDS and private-segment size of every img2dlr_kernel (r2c) and img2dlc_kernel (c2r) instantiation
(pass2dlr.hpp), from the compiler's own resource-usage remarks: compiles fftw3_amd/csrc/kernels_imglr.hip for gfx950 once
more (no GPU needed) and writes profiles/img2dlr_codeobj.txt.  A pair that spills or has a private segment in either direction is to be dropped
from img2dlr_menu.inc.

    python tools/perf/img2dlr_codeobj.py [--log remarks.txt]     (--log: parse a saved compiler output instead)
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def remarks():
    if "--log" in sys.argv:
        with open(sys.argv[sys.argv.index("--log") + 1]) as f:
            return f.read()
    cmd = [HIPCC, "-O3", "-fPIC", "--offload-arch=gfx950", "-Iinclude", "-Ifftw3_amd/csrc", "-std=c++17", "-Wall",
           "-Rpass-analysis=kernel-resource-usage", "-c", "fftw3_amd/csrc/kernels_imglr.hip", "-o", os.devnull]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout)
        raise SystemExit("compilation failed")
    return r.stdout


def main():
    import fftw3_amd as fa
    rows = []
    for blk in remarks().split("Function Name: ")[1:]:
        # _Z14img2dlr_kernelILi16ELi40EEv11Img2DLRArgs / _Z14img2dlc_kernelILi16ELi40EEv11Img2DLRArgs
        m = re.match(r"_Z14img2dl([rc])_kernelILi(\d+)ELi(\d+)EE", blk)
        if not m:
            continue
        fwd, n0, n1 = m.group(1) == "r", int(m.group(2)), int(m.group(3))

        def g(key):
            return int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
        T = fa.img2dlr_tile(n0, n1, fwd)
        if fwd:
            lds = (2 * T * n0 * ((n1 // 2) | 1) + 16) * 8
        else:
            lds = (T * n0 * (n1 | 1) + 16) * 8
        rows.append((n0, n1, "r2c" if fwd else "c2r", T, T * n0 * n1, g("VGPRs"), g("AGPRs"), g("VGPRs Spill"), g("SGPRs Spill"),
                     g("ScratchSize [bytes/lane]"), lds, g("Occupancy [waves/SIMD]")))
    rows.sort()
    out = ["# img2dlr_kernel<n0, n1> (r2c) and img2dlc_kernel<n0, n1> (c2r) (fftw3_amd/csrc/pass2dlr.hpp), hipcc -O3",
           "# --offload-arch=gfx950, 256 work-items, __launch_bounds__(256, 2).  From -Rpass-analysis=kernel-resource-usage",
           "# (tools/perf/img2dlr_codeobj.py).  T = images per tile, reals = T n0 n1, lds = dynamic LDS bytes per workgroup (the",
           "# plane), private = private segment (scratch) bytes per lane.  A row with a spill or a private segment leaves",
           "# img2dlr_menu.inc.",
           "# %3s %3s %3s %5s %6s %6s %6s %9s %9s %8s %6s %5s" % ("n0", "n1", "dir", "T", "reals", "vgprs", "agprs",
                                                                  "vgprspill", "sgprspill", "private", "lds", "waves")]
    for r in rows:
        out.append("  %3d %3d %3s %5d %6d %6d %6d %9d %9d %8d %6d %5d" % r)
    bad = [r for r in rows if r[7] or r[8] or r[9]]
    out.append("# %d kernels (%d sizes x r2c / c2r), %d with a spill or a private segment" % (len(rows), len(rows) // 2, len(bad)))
    with open(os.path.join(ROOT, "profiles", "img2dlr_codeobj.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    print(out[-1])


if __name__ == "__main__":
    main()
