"""measurement (not a test): rank-0 guru transposes, out of place and in place, real and complex.

    timeout -k 10 600 python tools/perf/perf_transpose.py [label]

One process, under the outer `timeout` of the command line above; every plan is checked for an exact result at the
size it is timed at, warmed up, then executed REPS times between device events on the stream it runs on; the line gives the median, the spread and the rate on the algorithmic
bytes (every element read once and written once).  The same script runs on any commit (it uses no name the package
gained later), so the parent's column of profiles/transpose.txt comes from the same command on the parent's build.
FFTW_AMD_NO_TRANSPOSE=1 keeps the copies of this build on the element-wise kernels."""
import os
import statistics
import sys

sys.path.insert(0, os.environ.get("FFTW_AMD_PKG_ROOT") or
                os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import fftw3_amd as fa

WARM, REPS = 3, 15
dev = torch.device("cuda:0")

# (name, kind, n0, n1, in place)
CASES = [
    ("oop  c2c  8192 x 8192", "c2c", 8192, 8192, False),
    ("oop  r2r 16384 x 16384", "r2r", 16384, 16384, False),
    ("inpl c2c  8192 x 8192", "c2c", 8192, 8192, True),
    ("inpl r2r 16384 x 16384", "r2r", 16384, 16384, True),
    ("inpl c2c  6000 x 10000", "c2c", 6000, 10000, True),
    ("inpl r2r  6000 x 10000", "r2r", 6000, 10000, True),
    ("oop  c2c  6000 x 10000", "c2c", 6000, 10000, False),
    # skinny matrices: fewer rows (columns) than a tile has
    ("oop  c2c skinny 4 x 8388608", "c2c", 4, 8388608, False),
    ("oop  c2c skinny 8388608 x 4", "c2c", 8388608, 4, False),
    ("oop  r2r skinny 3 x 16777216", "r2r", 3, 16777216, False),
    ("inpl c2c skinny 4 x 8388608", "c2c", 4, 8388608, True),
]
# in-place transform with transposed output, square: [(n, 1, v)], [(v, n, 1)]
DFT_CASES = [1024, 4096]


def timed(p):
    for _ in range(WARM):
        p.execute()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        p.execute()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def route(p):
    return " | ".join(l.strip().lstrip("(").split(" x")[0] for l in p.sprint().splitlines()[1:])


label = sys.argv[1] if len(sys.argv) > 1 else "run"
only = sys.argv[2:]
print("# %s: median of %d executions after %d warm-ups, device events; GB/s on 2 x the array bytes" % (label, REPS, WARM))
for name, kind, n0, n1, inplace in CASES:
    if only and not any(o in name for o in only):
        continue
    dt = torch.float64 if kind == "r2r" else torch.complex128
    x = torch.rand(n0 * n1, dtype=torch.float64, device=dev).to(dt) if kind == "r2r" else \
        torch.view_as_complex(torch.rand(n0 * n1, 2, dtype=torch.float64, device=dev))
    y = x if inplace else torch.zeros_like(x)
    want = x.reshape(n0, n1).t().contiguous().reshape(-1)
    loops = [(n0, n1, 1), (n1, 1, n0)]
    if kind == "r2r":
        p = fa.plan_guru64_r2r([], loops, x, y, [], fa.ESTIMATE)
    else:
        p = fa.plan_guru64_dft([], loops, x, y, fa.FORWARD, fa.ESTIMATE)
    p.execute()
    torch.cuda.synchronize()
    exact = bool(torch.equal(y, want))
    del want
    med, lo, hi = timed(p)
    nbytes = 2.0 * n0 * n1 * (8 if kind == "r2r" else 16)
    print("%-29s %9.3f ms  (min %8.3f max %8.3f)  %7.1f GB/s  scratch %5d MiB  %s  [%s]" % (
        name, med, lo, hi, nbytes / med / 1e6, p.workspace_bytes >> 20, "exact" if exact else "WRONG RESULT", route(p)),
        flush=True)
    del p, x, y
    torch.cuda.empty_cache()
for n in DFT_CASES:
    name = "inpl dft %d rows -> T" % n
    if only and not any(o in name for o in only):
        continue
    x = torch.view_as_complex(torch.rand(n * n, 2, dtype=torch.float64, device=dev))
    want = torch.fft.fft(x.reshape(n, n), dim=1).t().contiguous().reshape(-1)
    p = fa.plan_guru64_dft([(n, 1, n)], [(n, n, 1)], x, x, fa.FORWARD, fa.ESTIMATE)
    p.execute()
    torch.cuda.synchronize()
    err = float((x - want).abs().max() / want.abs().max())
    del want
    med, lo, hi = timed(p)
    print("%-29s %9.3f ms  (min %8.3f max %8.3f)  %7.1f GB/s  scratch %5d MiB  err %.1e  [%s]" % (
        name, med, lo, hi, 2.0 * n * n * 16 / med / 1e6, p.workspace_bytes >> 20, err, route(p)),
        flush=True)
    del p, x
    torch.cuda.empty_cache()
