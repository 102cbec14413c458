"""Instruction-class counts per kernel from a gfx950 assembly listing (hipcc -S --cuda-device-only).

    python tools/perf/isa_classes.py kernels.s pass1024
prints, for every kernel whose (mangled) name contains the filter: total, FP64 VALU, other VALU, LDS, global
(vector memory), SALU, waits, plus the VGPR count and scratch size from the kernel's metadata.  "SALU" is every s_*
instruction except s_waitcnt, s_barrier and s_nop, which are counted apart as "wait"."""
import re
import sys


def classify(op):
    if op.startswith("v_") and ("_f64" in op):
        return "fp64"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "global"
    if op in ("s_waitcnt", "s_barrier", "s_nop"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main():
    path, flt = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "")
    cur, counts, meta = None, {}, {}
    for line in open(path):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L") and m.group(1).startswith("_Z"):
            cur = m.group(1)
            counts[cur] = {}
            continue
        if cur is None:
            continue
        s = line.strip()
        if s.startswith(".end_amdhsa_kernel") or s.startswith(".Lfunc_end"):
            if s.startswith(".Lfunc_end"):
                cur = None
            continue
        if not s or s[0] in ".;" or s.endswith(":"):
            continue
        op = s.split()[0]
        c = classify(op)
        counts[cur][c] = counts[cur].get(c, 0) + 1
    # the register and scratch figures are comments behind the kernel's code: keyed by the preceding kernel name
    name = None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s*; (NumVgprs|ScratchSize|NumSgprs): (\d+)", line)
        if m and name:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
    cols = ["fp64", "valu", "lds", "global", "salu", "wait", "other"]
    print("%-90s %6s " % ("kernel", "total") + " ".join("%6s" % c for c in cols) + "   vgpr scratch")
    for k, c in counts.items():
        if flt not in k or not c:
            continue
        print("%-90s %6d " % (k[:90], sum(c.values())) + " ".join("%6d" % c.get(x, 0) for x in cols)
              + "  %5s %7s" % (meta.get(k, {}).get("NumVgprs", "?"), meta.get(k, {}).get("ScratchSize", "?")))


if __name__ == "__main__":
    main()
