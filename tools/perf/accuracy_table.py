"""Run the GPU accuracy case matrix (tests/accuracy_cases.py) and print one line per case: family, n, direction,
e_gpu / u, e_oracle / u, e_numpy / u and the ratio e_gpu / max(e_oracle, e_numpy, u / 2) that the gate of
tests/test_gpu_accuracy.py holds to <= 3; then the largest ratio per family.  u = 2^-53.

    python tools/perf/accuracy_table.py [--family F] [--skip-slow]      (output kept as profiles/r05_accuracy.txt)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import accuracy as A  # noqa: E402
import accuracy_cases as AC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", default=None)
    ap.add_argument("--skip-slow", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.ensure_built()
    if A.LD_REASON:
        sys.exit(A.LD_REASON)
    worst = {}
    print("%-16s %-30s %-4s %9s %9s %9s %6s  %s" % ("family", "n (x howmany)", "dir", "gpu/u", "oracle/u", "numpy/u",
                                                   "ratio", "case"))
    for c in AC.cases():
        if (a.family and c.fam != a.family) or (a.skip_slow and c.slow):
            continue
        x = AC.make_input(c)
        got, s, _ = AC.run_gpu(c, x)
        AC.check_labels(c, s)
        m = AC.measure(c, got, x)
        r = m["gpu"] / max(m["oracle"], m["numpy"], A.U / 2)
        if "per" in m:
            eg, eo, en = m["per"]
            r = max(r, max(eg[b] / max(eo[b], en[b], A.U / 2) for b in range(c.hm)))
        d = {"c2c": "fwd" if c.sign < 0 else "bwd", "slab": "fwd" if c.sign < 0 else "bwd"}.get(c.kind, c.kind)
        if c.kind == "r2r":
            d = "k%d" % c.r2r
        print("%-16s %-30s %-4s %9.3f %9.3f %9.3f %6.2f  %s" % (
            c.fam, "x".join(str(v) for v in c.shape) + " x%d" % c.hm, d, m["gpu"] / A.U, m["oracle"] / A.U,
            m["numpy"] / A.U, r, c.id))
        sys.stdout.flush()
        if r > worst.get(c.fam, (0, ""))[0]:
            worst[c.fam] = (r, c.id)
    print()
    print("largest ratio per family (whole batch or worst single entry for n >= 1024)")
    for f, (r, cid) in sorted(worst.items()):
        print("  %-16s %6.2f  %s" % (f, r, cid))


if __name__ == "__main__":
    main()
