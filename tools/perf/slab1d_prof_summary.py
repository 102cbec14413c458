"""Per-configuration kernel statistics of a rocprofv3 --kernel-trace database of tools/perf/slab1d_time.py: kernel
time per execution split into local plans, exchanges (hipMemcpy2DAsync blits) and the twiddle, and the rate of
slab_twiddle_kernel against the 6.29 TB/s copy rate.  Configurations are told apart by their twiddle launches.

  rocprofv3 --kernel-trace --stats -d OUT -o slab1d -- python tools/perf/slab1d_time.py --ndev 2,4 --reps 3 \
      --warmup 1 --no-single
  python tools/perf/slab1d_prof_summary.py OUT/slab1d_results.db "P=2,P=2 SCRAMBLED_OUT,P=4,P=4 SCRAMBLED_OUT" \
      8,8,16,16 4 30          # names, twiddle launches per configuration, executions per configuration, log2 n
"""
import sqlite3, sys
from collections import defaultdict
c = sqlite3.connect(sys.argv[1])
names = sys.argv[2].split(",")            # e.g. P=2,P=2 SCRAMBLED_OUT,P=4,P=4 SCRAMBLED_OUT
ntw = [int(v) for v in sys.argv[3].split(",")]   # twiddle dispatches per config
runs = int(sys.argv[4])
n = 1 << int(sys.argv[5])
rows = [r for r in c.execute("select name, start, end, grid_x from kernels order by start") if "at::native" not in r[0]]
tw_idx = [i for i, r in enumerate(rows) if r[0].startswith("slab_twiddle")]
bounds, k = [0], 0
for j in range(len(ntw) - 1):
    k += ntw[j]
    a, b = tw_idx[k - 1], tw_idx[k]           # last twiddle of config j, first of config j + 1
    gaps = [(rows[i + 1][1] - rows[i][2], i + 1) for i in range(a, b)]
    bounds.append(max(gaps)[1])
bounds.append(len(rows))
def cat(name):
    if name.startswith("slab_twiddle"): return "twiddle"
    if "copyBufferRect" in name: return "exchanges (hipMemcpy2DAsync)"
    if "copyBuffer" in name: return "table upload"
    return "local plans"
for j, nm in enumerate(names):
    g = rows[bounds[j]:bounds[j + 1]]
    tot = defaultdict(float)
    for r in g:
        tot[cat(r[0])] += (r[2] - r[1]) / 1e6
    s = sum(v for k_, v in tot.items() if k_ != "table upload")
    P = int(nm.split("=")[1].split()[0])
    tw = [(r[2] - r[1]) / 1e9 for r in g if r[0].startswith("slab_twiddle")]
    bytes_ = 2 * 16 * n / P
    print("%s: %d dispatches over %d executions; kernel time per execution %.2f ms" % (nm, len(g), runs, s / runs))
    for k_ in ("local plans", "exchanges (hipMemcpy2DAsync)", "twiddle"):
        print("    %-30s %8.2f ms per execution  %5.1f %%" % (k_, tot[k_] / runs, 100 * tot[k_] / s))
    print("    slab_twiddle_kernel: %d launches of %d elements, median %.3f ms -> %.2f TB/s (read + write) = %.0f %% of 6.29 TB/s"
          % (len(tw), n // P, sorted(tw)[len(tw) // 2] * 1e3, bytes_ / sorted(tw)[len(tw) // 2] / 1e12,
             100 * bytes_ / sorted(tw)[len(tw) // 2] / 1e12 / 6.29))
