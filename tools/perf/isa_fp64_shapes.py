"""Which FP64 expressions differ between two kernels of one gfx950 assembly listing (hipcc -S --cuda-device-only).

    python tools/perf/isa_fp64_shapes.py kernels.s KERNEL_A KERNEL_B [depth]

Walks each kernel's code in text order and keeps, for every vector register, the expression that produced it:
global loads are the leaf LD, LDS reads LDS, scalars and literals K, selects LD, other integer results I.  Every
FP64 add / mul / fma is then printed as its expression cut at `depth` levels (default 4), commutative operands
sorted, and the shapes whose counts differ between the two kernels are listed as "count in A, count in B, shape".
Two instantiations of one source that the compiler contracted to FMAs differently show up as pairs such as
fma(a, w, mul(b, w)) against fma(b, w, mul(a, w)); no output below the totals means no difference at that depth.
Branches are not followed, so this suits the straight-line tile kernels only."""
import collections
import re
import sys


def kernel_lines(path, name):
    """instructions of kernel `name`, comments and labels dropped"""
    inside = False
    for line in open(path):
        if line.startswith(name + ":"):
            inside = True
            continue
        if not inside:
            continue
        s = line.split(";")[0].strip()
        if s.startswith("s_endpgm"):
            return
        if s and s[0] != "." and not s.endswith(":"):
            yield s


def operand(tok):
    """(negated, (file, first register)) of an operand; file is "v", "a", "s" or "lit" """
    tok = tok.strip()
    neg = tok.startswith("-")
    tok = tok.lstrip("-").strip("|")
    m = re.match(r"^([vsa])\[(\d+):\d+\]$", tok) or re.match(r"^([vsa])(\d+)$", tok)
    if m:
        return neg, (m.group(1), int(m.group(2)))
    return neg, ("lit", tok)


def shape(e, depth):
    if not isinstance(e, tuple):
        return e
    if depth == 0:
        return "."
    op, parts = e[0], [shape(a, depth - 1) for a in e[1:]]
    if op in ("mul", "add"):
        parts.sort()
    elif op == "fma":
        parts = sorted(parts[:2]) + parts[2:]
    return op + "(" + ",".join(parts) + ")"


def shapes(path, name, depth):
    val = {}
    out = collections.Counter()

    def get(tok):
        neg, r = operand(tok)
        e = val.get(r, "?") if r[0] in ("v", "a") else "K"
        return ("neg", e) if neg else e

    def put(dst, e):
        val[operand(dst)[1]] = e
        out[shape(e, depth)] += 1

    for s in kernel_lines(path, name):
        op, _, rest = s.partition(" ")
        t = [x.strip() for x in rest.split(",")]
        if op.startswith("global_load") or op.startswith("ds_read"):
            f, r = operand(t[0])[1]
            for k in range(4):
                val[(f, r + k)] = "LD" if op[0] == "g" else "LDS"
        elif op.startswith("v_mul_f64"):
            put(t[0], ("mul", get(t[1]), get(t[2])))
        elif op.startswith("v_add_f64"):
            put(t[0], ("add", get(t[1]), get(t[2])))
        elif op.startswith("v_fma_f64"):
            put(t[0], ("fma", get(t[1]), get(t[2]), get(t[3])))
        elif op.startswith("v_fmac_f64"):
            put(t[0], ("fma", get(t[1]), get(t[2]), get(t[0])))
        elif op.startswith(("v_mov_b64", "v_mov_b32", "v_accvgpr", "v_pk_mov")):
            src = operand(t[1])[1]
            val[operand(t[0])[1]] = val.get(src, "?") if src[0] in ("v", "a") else "K"
        elif op.startswith("v_cndmask"):
            val[operand(t[0])[1]] = "LD"
        elif op.startswith("v_") and t and t[0].startswith("v"):
            val[operand(t[0])[1]] = "I"
    return out


def main():
    if len(sys.argv) not in (4, 5):
        sys.exit(__doc__)
    path, ka, kb = sys.argv[1:4]
    depth = int(sys.argv[4]) if len(sys.argv) == 5 else 4
    a, b = shapes(path, ka, depth), shapes(path, kb, depth)
    print("FP64 instructions: %d in A, %d in B; depth %d" % (sum(a.values()), sum(b.values()), depth))
    for k in sorted(set(a) | set(b)):
        if a[k] != b[k]:
            print(a[k], b[k], k)


if __name__ == "__main__":
    main()
