"""measurement (not a test): one-trip real-image plans for extents above 32 (FFTW_AMD_K_IMG2DLR, pass2dlr.hpp) against
the axis-by-axis plans they replace, r2c and c2r, for every pair of img2dlr_menu.inc.

    timeout -k 10 1100 python tools/perf/perf_img2dlr.py [--rounds R] [--out profiles/img2dlr.txt] [pair ...]

The driver starts fresh worker processes, alternating this build with FFTW_AMD_REAL_IMGL=1 ("one-trip") and without it
("axis by axis": the parent's plan, its sprint() goes in the output), R rounds of each (default 2).  A worker goes through
every pair once, r2c then c2r: a batch of 1 GiB of real data on device arrays, out of place, dense rows, 3 warm-ups,
then the median of 15 executions between device events on the stream the plan runs on.  Both configurations' results
are compared on the device at the size they are timed at.  Rates are algorithmic: one read of the input and one write
of the output (1 GiB of reals plus the half spectra, (n1 + 2) / n1 GiB) over the time.  The run-to-run spread of a pair
is the largest relative difference between the rounds of one configuration; a direction counts as faster when the
one-trip median is below the axis-by-axis median by more than that spread, and a pair stays in the menu when both
directions are.  A worker that fails ends the run.  `pair` arguments (e.g. 64x64) restrict the menu."""
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
    with open(os.path.join(ROOT, "fftw3_amd", "csrc", "img2dlr_menu.inc")) as f:
        return [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"X\((\d+), (\d+)\)", f.read())]


def worker(pairs):
    import torch
    import fftw3_amd as fa
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    rall = torch.rand(BYTES // 8, dtype=torch.float64, device=dev, generator=g) - 0.5
    call = torch.view_as_complex(torch.rand(3 * BYTES // 32, 2, dtype=torch.float64, device=dev, generator=g) - 0.5)
    for n0, n1 in pairs:
        n, h = n0 * n1, n1 // 2 + 1
        hm = BYTES // (8 * n)
        for fwd in (True, False):
            r, c = rall[:hm * n], call[:hm * n0 * h]
            if fwd:
                p = fa.plan_many_dft_r2c(2, [n0, n1], hm, r, None, 1, n, c, None, 1, n0 * h, fa.ESTIMATE)
            else:
                p = fa.plan_many_dft_c2r(2, [n0, n1], hm, c, None, 1, n0 * h, r, None, 1, n, fa.ESTIMATE)
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
            # the first and the last 64 images against torch on the same device data
            rr = torch.cat([r[:64 * n], r[-64 * n:]]).reshape(-1, n0, n1)
            cc = torch.cat([c[:64 * n0 * h], c[-64 * n0 * h:]]).reshape(-1, n0, h)
            if fwd:
                got, want = cc, torch.fft.rfft2(rr)
            else:
                z = torch.fft.ifft(cc, dim=1, norm="forward")
                z[:, :, 0] = z[:, :, 0].real + 0j
                z[:, :, h - 1] = z[:, :, h - 1].real + 0j
                got, want = rr, torch.fft.irfft(z, n=n1, dim=2, norm="forward")
            err = float((got - want).abs().max() / want.abs().max())
            route = " | ".join(ln.strip().lstrip("(").split(" buf")[0] for ln in p.sprint().splitlines()[1:])
            print(json.dumps({"n0": n0, "n1": n1, "fwd": fwd, "hm": hm, "ms": statistics.median(ts), "lo": min(ts),
                              "hi": max(ts), "err": err, "route": route}), flush=True)
            p.destroy()
            if not fwd:
                # the c2r overwrote the reals and (as FFTW's c2r may) possibly its input: fresh data for the next pair
                rall.uniform_(-0.5, 0.5, generator=g)
                torch.view_as_real(call).uniform_(-0.5, 0.5, generator=g)


def run_worker(env_extra, pairs):
    env = dict(os.environ)
    for k in ("FFTW_AMD_REAL_IMGL", "FFTW_AMD_REAL_IMG", "FFTW_AMD_NO_IMG2D", "FFTW_AMD_NO_TUNED"):
        env.pop(k, None)
    env.update(env_extra)
    env["FFTW_AMD_PKG_ROOT"] = ROOT
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"] + ["%dx%d" % p for p in pairs]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=400)
    if r.returncode != 0:
        raise SystemExit("worker %s failed with status %d" % (env_extra, r.returncode))
    sys.stderr.write("worker %s done\n" % (env_extra,))
    sys.stderr.flush()
    return {(d["n0"], d["n1"], d["fwd"]): d for d in (json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{"))}


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
    one, three = [], []
    for _ in range(rounds):
        one.append(run_worker({"FFTW_AMD_REAL_IMGL": "1"}, pairs))
        three.append(run_worker({}, pairs))
    lines = ["# one-trip real-image plans, extents above 32 (FFTW_AMD_REAL_IMGL=1), against the plans without the knob (the parent's",
             "# plans), MI355X.  Per pair a batch of 1 GiB of real data (hm = 2^30 / (8 n0 n1)), out of place, dense rows, device",
             "# arrays; median of %d executions between device events after %d warm-ups, %d rounds of each configuration in" % (REPS, WARM, rounds),
             "# alternating fresh processes (the figure is the median of the rounds' medians).  GB/s: one read of the input + one",
             "# write of the output (the reals and the half spectra) over the time.  spread: largest relative difference between",
             "# the rounds of one configuration.  faster: the one-trip time is below the axis-by-axis time by more than the spread.",
             "# A pair stays in img2dlr_menu.inc when both directions are faster.  (tools/perf/perf_img2dlr.py)",
             "# %3s %3s %3s %8s %9s %8s %9s %8s %6s %7s %7s  %s" % ("n0", "n1", "dir", "hm", "1trip ms", "GB/s", "axes ms", "GB/s",
                                                                    "ratio", "spread", "faster", "axis-by-axis plan")]
    not_faster = []
    ratios = {True: [], False: []}
    rates = {True: [], False: []}
    for pr in pairs:
        for fwd in (True, False):
            k = pr + (fwd,)
            a = [r[k]["ms"] for r in one]
            b = [r[k]["ms"] for r in three]
            ma, mb = statistics.median(a), statistics.median(b)
            spread = max((max(a) - min(a)) / min(a), (max(b) - min(b)) / min(b))
            faster = ma < mb * (1.0 - spread) if spread < 1 else False
            err = max(r[k]["err"] for r in one + three)
            if err > 1e-10:
                raise SystemExit("%dx%d %s: result differs from the reference by %g" % (pr[0], pr[1], "r2c" if fwd else "c2r", err))
            assert "img2dl-" in one[0][k]["route"] and "img2d" not in three[0][k]["route"], (one[0][k]["route"], three[0][k]["route"])
            if not faster and pr not in not_faster:
                not_faster.append(pr)
            gb = BYTES * (1.0 + (pr[1] + 2.0) / pr[1]) / 1e9
            ratios[fwd].append(mb / ma)
            rates[fwd].append(gb / (ma * 1e-3))
            lines.append("  %3d %3d %3s %8d %9.4f %8.0f %9.4f %8.0f %6.2f %6.1f%% %7s  %s" % (
                pr[0], pr[1], "r2c" if fwd else "c2r", one[0][k]["hm"], ma, gb / (ma * 1e-3), mb, gb / (mb * 1e-3), mb / ma,
                100 * spread, "yes" if faster else "NO", three[0][k]["route"]))
    for fwd in (True, False):
        lines.append("# %s: one-trip %.0f ... %.0f GB/s, %.2f ... %.2f x the axis-by-axis plan" % (
            "r2c" if fwd else "c2r", min(rates[fwd]), max(rates[fwd]), min(ratios[fwd]), max(ratios[fwd])))
    lines.append("# %d pairs, %d not faster than their axis-by-axis plan by more than the spread in both directions%s" % (
        len(pairs), len(not_faster), (": " + " ".join("%dx%d" % p for p in not_faster)) if not_faster else ""))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out if os.path.isabs(out) else os.path.join(os.getcwd(), out), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
