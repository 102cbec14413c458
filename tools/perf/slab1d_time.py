"""Wall time of the distributed 1-D transform (fftw_amd_slab_plan_dft_1d) at n = 2^30 over P = 1, 2, 4 entries of
one device list (devs = {0, ...}: on a one-GPU box every exchange is a copy on the same card), beside the
single-device fftw_plan_dft_1d of the same n.  Host clock around execute + synchronise, after a warm-up; prints
median / min / max over the repetitions and the effective rate 2 n 16 B / t.

  python tools/perf/slab1d_time.py [--log2n 30] [--ndev 1,2,4] [--reps 10] [--warmup 2] [--no-single]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import fftw3_amd as fa  # noqa: E402


def timed(run, sync, reps, warmup):
    for _ in range(warmup):
        run()
        sync()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def report(name, n, ts):
    med = statistics.median(ts)
    print("%-34s median %9.2f ms  min %9.2f  max %9.2f  (%d reps)  %6.2f TB/s effective"
          % (name, med, min(ts), max(ts), len(ts), 2 * n * 16 / (med * 1e-3) / 1e12), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--ndev", default="1,2,4")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-single", action="store_true")
    args = ap.parse_args()
    n = 1 << args.log2n
    torch.manual_seed(0)
    x = torch.view_as_complex(torch.rand((n, 2), dtype=torch.float64, device="cuda") - 0.5)
    y = torch.zeros_like(x)
    print("n = 2^%d (%.1f GiB per array), device %s" % (args.log2n, n * 16 / 2**30, torch.cuda.get_device_name(0)))
    if not args.no_single:
        p = fa.plan_dft_1d(n, x, y, fa.FORWARD)
        report("fftw_plan_dft_1d (one device)", n, timed(p.execute, p.sync, args.reps, args.warmup))
        p.destroy()
    for ndev in [int(v) for v in args.ndev.split(",")]:
        b = n // ndev
        ins = [x[g * b:(g + 1) * b] for g in range(ndev)]
        outs = [y[g * b:(g + 1) * b] for g in range(ndev)]
        for flags, tag in ((0, ""), (fa.SLAB_SCRAMBLED_OUT, " SCRAMBLED_OUT")):
            sp = fa.SlabPlan1dC(n, [0] * ndev, ins, outs, fa.FORWARD, fa.ESTIMATE | flags)
            n0, n1 = fa.slab_split_1d(n, ndev, fa.FORWARD)
            report("slab 1-d P=%d (%d x %d)%s" % (ndev, n0, n1, tag), n, timed(sp.execute, sp.sync, args.reps, args.warmup))
            if not flags:
                print("    columns: %s" % sp.local_plan_sprint(0, 1).replace("\n", " "))
                print("    rows:    %s" % sp.local_plan_sprint(0, 0).replace("\n", " "))
            sp.destroy()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
