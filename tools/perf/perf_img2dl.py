"""measurement (not a test): one-trip image plans for extents above 32 (FFTW_AMD_K_IMG2DL, pass2dl.hpp) against the
axis-by-axis plans they replace, for every pair of img2dl_menu.inc.

    timeout -k 10 1100 python tools/perf/perf_img2dl.py [--rounds R] [--parent DIR] [--out profiles/img2dl.txt] [pair ...]

The driver starts fresh worker processes, each under a `timeout` of its own, alternating this build as it is
("one-trip") with FFTW_AMD_NO_IMG2D=1 ("two-trip": the same binary without whole images in one trip; its sprint() goes
in the output) and, with --parent DIR, the package built from the parent commit in DIR ("parent"), R rounds of each
(default 2).  A worker goes through every pair once: a batch of 1 GiB of images on device arrays (1 GiB read + 1 GiB
written per execution), forward, out of place, 3 warm-ups, then 15 executions timed between device events on the stream
the plan runs on.  Every configuration's result is compared on the device with torch.fft.fft2 at the size it is timed
at.  A configuration's figure is the median of all its timed executions (rounds pooled) and its range their minimum
and maximum.  Rates are algorithmic: one read and one write of the batch over the time.  A pair counts as faster when
the one-trip median is below the others' and its range lies below their ranges without overlap (the tie rule of
profiles/r04_c2r_two_trip.txt).  A worker that fails ends the run.  `pair` arguments (e.g. 64x64) restrict the menu."""
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.environ.get("FFTW_AMD_PKG_ROOT") or ROOT
sys.path.insert(0, PKG)

WARM, REPS = 3, 15
BYTES = 1 << 30
WORKER_SECONDS = 240


def menu():
    with open(os.path.join(ROOT, "fftw3_amd", "csrc", "img2dl_menu.inc")) as f:
        return [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"X\((\d+), (\d+)\)", f.read())]


def worker(pairs):
    import torch
    import fftw3_amd as fa
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    xall = torch.view_as_complex(torch.rand(BYTES // 16, 2, dtype=torch.float64, device=dev, generator=g) - 0.5)
    yall = torch.zeros_like(xall)
    for n0, n1 in pairs:
        n = n0 * n1
        hm = BYTES // (16 * n)
        x, y = xall[:hm * n], yall[:hm * n]
        p = fa.plan_many_dft(2, [n0, n1], hm, x, None, 1, n, y, None, 1, n, fa.FORWARD, fa.ESTIMATE)
        for _ in range(WARM):
            p.execute()
        p.sync()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            p.execute()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        # the first and the last 64 images against torch's transform of the same input
        head = torch.cat([y[:64 * n], y[-64 * n:]])
        want = torch.fft.fft2(torch.cat([x[:64 * n], x[-64 * n:]]).reshape(-1, n0, n1)).reshape(-1)
        err = float((head - want).abs().max() / want.abs().max())
        route = " | ".join(ln.strip().lstrip("(").split(" buf")[0] for ln in p.sprint().splitlines()[1:])
        print(json.dumps({"n0": n0, "n1": n1, "hm": hm, "ts": ts, "err": err, "route": route}), flush=True)
        p.destroy()


def run_worker(pkg, env_extra, pairs):
    env = dict(os.environ)
    env.pop("FFTW_AMD_NO_IMG2D", None)
    env.update(env_extra)
    env["FFTW_AMD_PKG_ROOT"] = pkg
    cmd = ["timeout", "-k", "10", str(WORKER_SECONDS), sys.executable, os.path.abspath(__file__), "--worker"]
    r = subprocess.run(cmd + ["%dx%d" % p for p in pairs], env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit("worker %s %s failed with status %d" % (pkg, env_extra, r.returncode))
    return {(d["n0"], d["n1"]): d for d in (json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{"))}


def take(args, name):
    if name not in args:
        return None
    i = args.index(name)
    v = args[i + 1]
    del args[i:i + 2]
    return v


def main():
    args = sys.argv[1:]
    rounds = int(take(args, "--rounds") or 2)
    out = take(args, "--out")
    parent = take(args, "--parent")
    is_worker = "--worker" in args
    args = [a for a in args if a != "--worker"]
    pairs = [tuple(int(v) for v in a.split("x")) for a in args] or menu()
    if is_worker:
        worker(pairs)
        return
    configs = [("1trip", ROOT, {}), ("2trip", ROOT, {"FFTW_AMD_NO_IMG2D": "1"})]
    if parent:
        configs.append(("parent", os.path.abspath(parent), {}))
    runs = {name: [] for name, _, _ in configs}
    for _ in range(rounds):
        for name, pkg, env in configs:
            runs[name].append(run_worker(pkg, env, pairs))
    lines = ["# one-trip image plans for extents above 32 against the axis-by-axis plans, MI355X: \"1trip\" this build,",
             "# \"2trip\" the same binary with FFTW_AMD_NO_IMG2D=1" + (", \"parent\" the parent commit's build." if parent else "."),
             "# Per pair a batch of 1 GiB of images (hm = 2^30 / (16 n0 n1)), forward, out of place, device arrays; %d timed" % REPS,
             "# executions between device events after %d warm-ups, %d rounds of each configuration in alternating fresh" % (WARM, rounds),
             "# processes.  ms: median (min ... max) of the pooled executions.  GB/s: one read + one write of the batch over",
             "# the median.  faster: the one-trip median is the lowest and its range lies below the other ranges without",
             "# overlap.  (tools/perf/perf_img2dl.py)"]
    not_faster = []
    gb = 2.0 * BYTES / 1e9
    for pr in pairs:
        stat = {}
        for name, _, _ in configs:
            ts = [t for r in runs[name] for t in r[pr]["ts"]]
            err = max(r[pr]["err"] for r in runs[name])
            if err > 1e-10:
                raise SystemExit("%dx%d %s: result differs from the reference by %g" % (pr[0], pr[1], name, err))
            stat[name] = (statistics.median(ts), min(ts), max(ts))
        assert "img2dl" in runs["1trip"][0][pr]["route"], runs["1trip"][0][pr]["route"]
        for name in stat:
            if name != "1trip":
                assert "img2d" not in runs[name][0][pr]["route"], runs[name][0][pr]["route"]
        others = [stat[k] for k in stat if k != "1trip"]
        faster = all(stat["1trip"][0] < o[0] and stat["1trip"][2] < o[1] for o in others)
        if not faster:
            not_faster.append(pr)
        cols = ["%3dx%-3d hm %6d" % (pr[0], pr[1], runs["1trip"][0][pr]["hm"])]
        for name, _, _ in configs:
            m, lo, hi = stat[name]
            cols.append("%s %7.4f ms (%7.4f ... %7.4f) %5.0f GB/s" % (name, m, lo, hi, gb / (m * 1e-3)))
        cols.append("ratio %5.2f" % (min(o[0] for o in others) / stat["1trip"][0]))
        cols.append("faster %s" % ("yes" if faster else "NO"))
        cols.append(runs["2trip"][0][pr]["route"])
        lines.append(" | ".join(cols))
    lines.append("# %d pairs, %d not faster than their axis-by-axis plans%s" % (
        len(pairs), len(not_faster), (": " + " ".join("%dx%d" % p for p in not_faster)) if not_faster else ""))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out if os.path.isabs(out) else os.path.join(os.getcwd(), out), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
