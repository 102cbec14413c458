"""measurement (not a test): the two-trip planes plan of rank-3 c2c problems (FFTW_AMD_VOL_PLANES=1, planner.c
emit_vol_planes) and the one-trip image step for an extent of 128 (FFTW_AMD_IMG_WIDE=1, pass2dw.hpp) against the plans
built with the knobs unset, which are the parent commit's plans (tests/test_vol_planes_plans.py proves that).

    timeout -k 10 900 python tools/perf/perf_vol_planes.py [--rounds R] [--bytes B] [--out profiles/vol_planes.txt] [case ...]

One process, one session.  Per case a batch of about 4 GiB (one read + one write of it per execution), forward, out of
place, on device arrays: both plans are made on the same arrays, each is warmed up 3 times, then R rounds (default 4)
alternate "new" and "old", 5 executions of each per round, every execution timed between device events on the stream
the plan runs on.  A plan's figure is the median of its timed executions and its range their minimum and maximum: the
run-to-run spread the comparison has to beat.  The new plan counts as faster when its median is the lower one and its
range lies below the old plan's without overlap.  Both results are compared on the device with torch.fft.fftn on the
first and the last transform of the batch, at the size they are timed at.  Rates are algorithmic: one read and one
write of the batch over the median; the share of the roofline is that rate over 8 TB/s.  `case` arguments (64x64x64,
128x128 ...) restrict the list."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WARM, REPS = 3, 5
CASES = [(64, 64, 64), (128, 128, 128), (64, 128, 128), (256, 64, 64), (128, 128), (64, 128), (128, 64)]
PEAK_TBS = 8.0


def take(args, name):
    if name not in args:
        return None
    i = args.index(name)
    v = args[i + 1]
    del args[i:i + 2]
    return v


def plan_with(fa, env, shape, hm, x, y):
    old = {k: os.environ.get(k) for k in ("FFTW_AMD_VOL_PLANES", "FFTW_AMD_IMG_WIDE")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        n = 1
        for v in shape:
            n *= v
        return fa.plan_many_dft(len(shape), list(shape), hm, x, None, 1, n, y, None, 1, n, fa.FORWARD, fa.ESTIMATE)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def route(p):
    return " | ".join(ln.strip().lstrip("(").split(" buf")[0] for ln in p.sprint().splitlines()[1:])


def timed(torch, p, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        p.execute()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def main():
    args = sys.argv[1:]
    rounds = int(take(args, "--rounds") or 4)
    nbytes = int(take(args, "--bytes") or (4 << 30))
    out = take(args, "--out")
    cases = [tuple(int(v) for v in a.split("x")) for a in args] or CASES
    import torch
    import fftw3_amd as fa
    if fa.device_count() <= 0:
        raise SystemExit("perf_vol_planes: no HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    xall = torch.view_as_complex(torch.rand(nbytes // 16, 2, dtype=torch.float64, device=dev, generator=g) - 0.5)
    yall = torch.zeros_like(xall)
    lines = ["# two-trip planes plans (rank 3, FFTW_AMD_VOL_PLANES=1) and one-trip images with an extent of 128 (rank 2,",
             "# FFTW_AMD_IMG_WIDE=1), \"new\", against the plans built with the knobs unset, \"old\" (the parent commit's plans), MI355X.",
             "# Per case a batch of %.2f GiB (hm transforms), forward, out of place, device arrays, one process: %d warm-ups of" % (nbytes / 2.0 ** 30, WARM),
             "# each plan, then %d rounds alternating new and old, %d executions of each per round, timed between device events." % (rounds, REPS),
             "# ms: median (min ... max) of a plan's %d timed executions; the range is the run-to-run spread.  TB/s: one read +" % (rounds * REPS),
             "# one write of the batch over the median; roof: that rate over %.0f TB/s.  faster: the new median is the lower one" % PEAK_TBS,
             "# and the new range lies below the old range without overlap.  (tools/perf/perf_vol_planes.py)"]
    no_faster = []
    for shape in cases:
        n = 1
        for v in shape:
            n *= v
        hm = nbytes // (16 * n)
        x, y = xall[:hm * n], yall[:hm * n]
        env = {"FFTW_AMD_VOL_PLANES": "1"} if len(shape) == 3 else {"FFTW_AMD_IMG_WIDE": "1"}
        plans = {"new": plan_with(fa, env, shape, hm, x, y), "old": plan_with(fa, {}, shape, hm, x, y)}
        want_steps = 2 if len(shape) == 3 else 1
        assert len(plans["new"].steps()) == want_steps and "img2d" in route(plans["new"]), plans["new"].sprint()
        assert "img2d" not in route(plans["old"]), plans["old"].sprint()
        ts = {"new": [], "old": []}
        axes = tuple(range(1, len(shape) + 1))
        ends = torch.cat([x[:n], x[-n:]]).reshape((2,) + shape)
        want = torch.fft.fftn(ends, dim=axes).reshape(-1)
        for name in ("new", "old"):
            for _ in range(WARM):
                plans[name].execute()
            plans[name].sync()
            torch.cuda.synchronize()
            got = torch.cat([y[:n], y[-n:]])
            err = float((got - want).abs().max() / want.abs().max())
            if err > 1e-10:
                raise SystemExit("%s %s: result differs from the reference by %g" % ("x".join(map(str, shape)), name, err))
            y.zero_()
        for _ in range(rounds):
            for name in ("new", "old"):
                ts[name] += timed(torch, plans[name], REPS)
        stat = {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}
        faster = stat["new"][0] < stat["old"][0] and stat["new"][2] < stat["old"][1]
        if not faster:
            no_faster.append(shape)
        tb = 2.0 * 16 * n * hm / 1e12
        cols = ["%-11s hm %6d" % ("x".join(map(str, shape)), hm)]
        for name in ("new", "old"):
            m, lo, hi = stat[name]
            rate = tb / (m * 1e-3)
            cols.append("%s %8.4f ms (%8.4f ... %8.4f) %5.2f TB/s roof %4.1f %%" % (name, m, lo, hi, rate, 100.0 * rate / PEAK_TBS))
        cols.append("ratio %5.2f" % (stat["old"][0] / stat["new"][0]))
        cols.append("faster %s" % ("yes" if faster else "NO"))
        cols.append("new: " + route(plans["new"]))
        cols.append("old: " + route(plans["old"]))
        lines.append(" | ".join(cols))
        print(lines[-1], flush=True)
        for p in plans.values():
            p.destroy()
    lines.append("# %d cases, %d no faster than the old plan%s" % (
        len(cases), len(no_faster), (": " + " ".join("x".join(map(str, s)) for s in no_faster)) if no_faster else ""))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        path = out if os.path.isabs(out) else os.path.join(os.getcwd(), out)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
