"""measurement (not a test): one-trip small-image plans (FFTW_AMD_K_IMG2D, pass2d.hpp) against the two-trip plans they
replace, for every pair of img2d_menu.inc.

    timeout -k 10 1100 python tools/perf/perf_img2d.py [--rounds R] [--out profiles/img2d.txt] [pair ...]

The driver starts fresh worker processes, alternating this build as it is ("one-trip") with FFTW_AMD_NO_IMG2D=1
("two-trip": the parent's plan, its sprint() goes in the output), R rounds of each (default 2).  A worker goes through
every pair once: a batch of 1 GiB of images on device arrays (1 GiB read + 1 GiB written per execution), forward, out
of place, 3 warm-ups, then the median of 15 executions between device events on the stream the plan runs on.  Both
configurations' results are compared on the device at the size they are timed at.  Rates are algorithmic: one read and
one write of the batch over the time.  The run-to-run spread of a pair is the largest relative difference between the
rounds of one configuration; a pair counts as faster when the one-trip median is below the two-trip median by more
than that spread.  A worker that fails ends the run.  `pair` arguments (e.g. 16x16) restrict the menu."""
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.environ.get("FFTW_AMD_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WARM, REPS = 3, 15
BYTES = 1 << 30


def menu():
    with open(os.path.join(ROOT, "fftw3_amd", "csrc", "img2d_menu.inc")) as f:
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
        # a checksum of the result the other configuration must reproduce: the first and the last 64 images
        head = torch.cat([y[:64 * n], y[-64 * n:]])
        want = torch.fft.fft2(torch.cat([x[:64 * n], x[-64 * n:]]).reshape(-1, n0, n1)).reshape(-1)
        err = float((head - want).abs().max() / want.abs().max())
        route = " | ".join(ln.strip().lstrip("(").split(" buf")[0] for ln in p.sprint().splitlines()[1:])
        print(json.dumps({"n0": n0, "n1": n1, "hm": hm, "ms": statistics.median(ts), "lo": min(ts), "hi": max(ts),
                          "err": err, "route": route}), flush=True)
        p.destroy()


def run_worker(env_extra, pairs):
    env = dict(os.environ)
    env.pop("FFTW_AMD_NO_IMG2D", None)
    env.update(env_extra)
    env["FFTW_AMD_PKG_ROOT"] = ROOT
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"] + ["%dx%d" % p for p in pairs]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=480)
    if r.returncode != 0:
        raise SystemExit("worker %s failed with status %d" % (env_extra, r.returncode))
    return {(d["n0"], d["n1"]): d for d in (json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{"))}


def main():
    args = sys.argv[1:]
    rounds, out = 2, None
    if "--rounds" in args:
        i = args.index("--rounds")
        rounds = int(args[i + 1])
        del args[i:i + 2]
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    is_worker = "--worker" in args
    args = [a for a in args if a != "--worker"]
    pairs = [tuple(int(v) for v in a.split("x")) for a in args] or menu()
    if is_worker:
        worker(pairs)
        return
    one, two = [], []
    for _ in range(rounds):
        one.append(run_worker({}, pairs))
        two.append(run_worker({"FFTW_AMD_NO_IMG2D": "1"}, pairs))
    lines = ["# one-trip small-image plans against the two-trip plans of FFTW_AMD_NO_IMG2D=1 (the parent's plans), MI355X.",
             "# Per pair a batch of 1 GiB of images (hm = 2^30 / (16 n0 n1)), forward, out of place, device arrays; median of",
             "# %d executions between device events after %d warm-ups, %d rounds of each configuration in alternating fresh" % (REPS, WARM, rounds),
             "# processes (the figure is the median of the rounds' medians).  GB/s: one read + one write of the batch over",
             "# the time.  spread: largest relative difference between the rounds of one configuration.  faster: the one-trip",
             "# time is below the two-trip time by more than the spread.  (tools/perf/perf_img2d.py)",
             "# %3s %3s %8s %9s %8s %9s %8s %6s %7s %7s  %s" % ("n0", "n1", "hm", "1trip ms", "GB/s", "2trip ms", "GB/s",
                                                                "ratio", "spread", "faster", "two-trip plan")]
    not_faster = []
    for pr in pairs:
        a = [r[pr]["ms"] for r in one]
        b = [r[pr]["ms"] for r in two]
        ma, mb = statistics.median(a), statistics.median(b)
        spread = max((max(a) - min(a)) / min(a), (max(b) - min(b)) / min(b))
        faster = ma < mb * (1.0 - spread) if spread < 1 else False
        err = max(r[pr]["err"] for r in one + two)
        if err > 1e-10:
            raise SystemExit("%dx%d: result differs from the reference by %g" % (pr[0], pr[1], err))
        assert "img2d" in one[0][pr]["route"] and "img2d" not in two[0][pr]["route"], (one[0][pr]["route"], two[0][pr]["route"])
        if not faster:
            not_faster.append(pr)
        gb = 2.0 * BYTES / 1e9
        lines.append("  %3d %3d %8d %9.4f %8.0f %9.4f %8.0f %6.2f %6.1f%% %7s  %s" % (
            pr[0], pr[1], one[0][pr]["hm"], ma, gb / (ma * 1e-3), mb, gb / (mb * 1e-3), mb / ma, 100 * spread,
            "yes" if faster else "NO", two[0][pr]["route"]))
    lines.append("# %d pairs, %d not faster than their two-trip plan by more than the spread%s" % (
        len(pairs), len(not_faster), (": " + " ".join("%dx%d" % p for p in not_faster)) if not_faster else ""))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out if os.path.isabs(out) else os.path.join(os.getcwd(), out), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
