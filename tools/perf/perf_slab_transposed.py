"""Slab plans of the C ABI with TRANSPOSED layouts against the normal-order slab plan of the same problem, and the
transposing exchange against the 2-D-copy exchange.  One MI355X, the device named P = 1, 2, 4 times.

    python tools/perf/perf_slab_transposed.py [--baseline-lib PATH] [--reps 9] [--out FILE]

--baseline-lib: libfftw3_amd.so built from the parent commit (into a side directory); it is loaded next to this
tree's library and supplies the parent's normal-order c2c plan.  Real plans have no parent: their baseline is this
tree's normal-order plan.

Timing.  Per comparison: 2 warm-up executions per side, then `reps` timed ones per side, the sides ALTERNATING
(baseline, transposed, baseline, ...).  Plans of this tree are timed by fftw_amd_slab_execute_timed: device events on
every stream of the plan around one execution that ends in a synchronise ("dev ms"); next to it the host clock from
the enqueue to the end of the synchronise ("host ms").  The parent's library has no such entry and keeps its streams
to itself, so the parent plan has the host clock only; this tree's normal-order c2c plan (the same local plans and
copies) stands beside it with both clocks.  Reported: median and (max - min) / median.  The
condition of a row: the transposed plan is not slower than the baseline by more than the baseline's own spread, on
device time against this tree's normal-order plan, and for c2c also on host time against the parent's plan.

Exchanges alone: the block moves are taken from fftw_amd_slab_exchange_ops of a TRANSPOSED_OUT and of a normal-order
plan of the same problem (what the executors iterate) and issued on the null stream between device events -- one
launch of the transposing kernel per receiving device, or P * P hipMemcpy2DAsync copies."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch         # noqa: E402

import fftw3_amd as fa                              # noqa: E402
from slab_layouts import T_IN, T_OUT, Geo           # noqa: E402


class ParentC2c(object):
    """the normal-order c2c slab plan of another build of the library"""

    def __init__(self, lib, n, devs, ins, outs, sign):
        self.lib = lib
        nn = (C.c_longlong * len(n))(*n)
        dv = (C.c_int * len(devs))(*devs)
        pp = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])   # noqa: E731
        lib.fftw_amd_slab_plan_dft.restype = C.c_void_p
        lib.fftw_amd_slab_plan_dft.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint]
        for f in ("fftw_amd_slab_execute", "fftw_amd_slab_sync", "fftw_amd_destroy_slab_plan"):
            getattr(lib, f).restype = None
            getattr(lib, f).argtypes = [C.c_void_p]
        self.handle = lib.fftw_amd_slab_plan_dft(len(n), nn, len(devs), dv, pp(ins), pp(outs), sign, fa.ESTIMATE)
        assert self.handle, "parent library returned NULL"

    def execute(self):
        self.lib.fftw_amd_slab_execute(self.handle)

    def sync(self):
        self.lib.fftw_amd_slab_sync(self.handle)

    def destroy(self):
        self.lib.fftw_amd_destroy_slab_plan(self.handle)


def timed(plan):
    """(device ms or None, host ms) of one execution"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if hasattr(plan, "execute_timed"):
        dev_ms = plan.execute_timed()
    else:
        dev_ms = None
        plan.execute()
        plan.sync()
    return dev_ms, (time.perf_counter() - t0) * 1e3


def med(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m


def compare(sides, reps):
    for _, p in sides:
        for _ in range(2):
            timed(p)
    got = [[] for _ in sides]
    for _ in range(reps):
        for k, (_, p) in enumerate(sides):
            got[k].append(timed(p))
    out = []
    for (name, _), v in zip(sides, got):
        dev = med([d for d, _ in v]) if v[0][0] is not None else None
        out.append((name, dev, med([h for _, h in v])))
    return out


def arrays(geo, flags, dev):
    return [torch.view_as_complex(torch.rand(geo.elems(g, flags), 2, dtype=torch.float64, device=dev) - 0.5)
            for g in range(geo.P)]


def event_ms(fn, reps):
    ms = []
    for it in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(torch.cuda.default_stream())
        fn()
        e1.record(torch.cuda.default_stream())
        torch.cuda.synchronize()
        if it >= 2:
            ms.append(e0.elapsed_time(e1))
    return med(ms)


def exchanges(kind, shape, P, reps, dev, say):
    """the transposing exchange of the TRANSPOSED_OUT plan and the first 2-D-copy exchange of the normal-order plan of
    the same problem, replayed from the plans' own lists on buffers of this tool"""
    geo = Geo(kind, shape, P)
    n0, n1, rest = geo.c3
    src = arrays(geo, T_OUT, dev)
    dst = [torch.zeros_like(t) for t in src]
    wbuf = [torch.zeros(max(1, n0 * geo.cuts[g][3] * rest), dtype=torch.complex128, device=dev) for g in range(P)]
    pt = geo.make_plan([0] * P, src, dst, -1, T_OUT)
    pn = geo.make_plan([0] * P, src, dst, -1, 0)
    tops, nops = pt.exchange_ops(0), pn.exchange_ops(0)
    stream = torch.cuda.default_stream().cuda_stream
    moved = 2.0 * 16 * sum(o["A"] * o["B"] * o["I"] for o in tops)
    assert moved == 2.0 * 16 * sum(o["A"] * o["B"] * o["I"] for o in nops)

    def kernel(nt):
        for r in range(P):
            mine = [o for o in tops if o["ddev"] == r]
            if mine:
                blocks = [(src[o["sdev"]].data_ptr() + 16 * o["soff"], o["doff"], o["A"], o["B"], o["ssa"], o["ssb"]) for o in mine]
                assert fa.slab_block_transpose(dst[r], mine[0]["dsa"], mine[0]["dsb"], mine[0]["I"], blocks, stream, nt) == 0

    cp = fa.lib.fa_hip_memcpy2d_peer
    cp.restype = None
    cp.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p]

    def copies():
        for o in nops:
            cp(wbuf[o["ddev"]].data_ptr() + 16 * o["doff"], 16 * o["dsa"], src[o["sdev"]].data_ptr() + 16 * o["soff"], 16 * o["ssa"],
               16 * o["I"], o["A"], stream)

    row = "%-4s %-12s %2d %5d %9.0f |" % (kind, "x".join(map(str, shape)), P, tops[0]["I"], moved / 2 ** 20)
    for fn in (lambda: kernel(-1), lambda: kernel(0), lambda: kernel(1), copies):
        m, s = event_ms(fn, reps)
        row += " %8.3f %6.2f %5.1f%% |" % (m, moved / (m * 1e-3) / 1e12, 100 * s)
    say(row)
    pt.destroy()
    pn.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    parent = None
    if a.baseline_lib:
        parent = C.CDLL(a.baseline_lib, mode=os.RTLD_NOW | os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    say("# slab plans, TRANSPOSED layouts against normal order; one MI355X, device 0 named P times; medians of %d alternating "
        "timed executions, spread = (max - min) / median" % a.reps)
    say("# dev ms: device events on the plan's streams around execute .. sync; host ms: host clock over the same")
    say("# c2c also against %s" % ("the parent commit's library (normal order; host clock only, it has no event entry)"
                                   if parent else "nothing else (no --baseline-lib)"))
    say("# execution on several DISTINCT devices is unverified: every number below is one card")
    say("%-4s %-12s %2s  %-20s %9s %7s %9s %7s   %s" % ("kind", "shape", "P", "plan", "dev ms", "spread", "host ms", "spread", "verdict"))
    cases = [("c2c", (4096, 4096)), ("c2c", (8192, 8192)), ("r2c", (8192, 8192)), ("c2r", (8192, 8192)),
             ("r2c", (512, 512, 512)), ("c2r", (512, 512, 512))]
    for kind, shape in cases:
        for P in (1, 2, 4):
            geo = Geo(kind, shape, P)
            tflag = T_IN if kind == "c2r" else T_OUT
            sign = 1 if kind == "c2r" else -1
            i0, o0 = arrays(geo, 0, dev), arrays(geo, 0, dev)
            i1, o1 = arrays(geo, tflag, dev), arrays(geo, tflag, dev)
            sides = [("normal (this tree)", geo.make_plan([0] * P, i0, o0, sign, 0)),
                     ("TRANSPOSED_%s" % ("IN" if kind == "c2r" else "OUT"), geo.make_plan([0] * P, i1, o1, sign, tflag))]
            if kind == "c2c" and parent is not None:
                i2, o2 = arrays(geo, 0, dev), arrays(geo, 0, dev)
                sides.append(("normal (parent)", ParentC2c(parent, list(shape), [0] * P, i2, o2, sign)))
            r = compare(sides, a.reps)
            (_, bd, bh), (_, td, th) = r[0], r[1]
            verdict = "dev: " + ("not slower" if td[0] <= bd[0] * (1 + bd[1]) else "SLOWER than normal + its spread")
            if len(r) > 2:
                ph = r[2][2]
                verdict += "; host vs parent: " + ("not slower" if th[0] <= ph[0] * (1 + ph[1]) else "SLOWER than parent + its spread")
            for k, (name, d, h) in enumerate(r):
                ds = "%9.3f %6.1f%%" % (d[0], 100 * d[1]) if d else "%9s %7s" % ("-", "-")
                say("%-4s %-12s %2d  %-20s %s %9.3f %6.1f%%   %s" % (kind, "x".join(map(str, shape)), P, name, ds, h[0], 100 * h[1],
                                                                  verdict if k == 1 else ""))
            for _, p in sides:
                p.destroy()
            del i0, o0, i1, o1, sides
            torch.cuda.empty_cache()
    say("")
    say("# exchanges alone, null stream, device events; TB/s = bytes moved (read + write) / time; the card's linear copy rate is "
        "6.25 TB/s (profiles/r03_mall_probe.txt)")
    say("# kernel: one launch of the transposing kernel per receiving device (I < 8: LDS tiles, I >= 8: direct), nontemporal "
        "policy by the launcher's rule / off / on; copies: the P * P hipMemcpy2DAsync of the normal-order plan's first exchange")
    say("%-4s %-12s %2s %5s %9s | %24s | %24s | %24s | %24s |" % ("kind", "shape", "P", "I", "MiB moved", "kernel, rule: ms TB/s spread",
                                                              "kernel, nt off", "kernel, nt on", "2-D copies"))
    for kind, shape in (("c2c", (4096, 4096)), ("c2c", (8192, 8192)), ("r2c", (8192, 8192)), ("c2c", (2048, 2048, 4)), ("r2c", (512, 512, 512))):
        for P in (1, 2, 4):
            exchanges(kind, shape, P, a.reps, dev, say)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
