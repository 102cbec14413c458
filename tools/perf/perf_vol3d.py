"""measurement (not a test): one-trip small-volume plans (FFTW_AMD_K_VOL3D, pass3d.hpp, FFTW_AMD_VOL3D=1) against the
axis-by-axis plans of the same build with the knob unset, for every triple of vol3d_menu.inc.

    timeout -k 10 1100 python tools/perf/perf_vol3d.py [--out profiles/vol3d.txt] [triple ...]

The plan with the knob unset is the parent commit's plan (tests/test_vol3d_plans.py pins that); it is the yardstick,
its sprint() goes in the output.  The driver starts one fresh worker process per configuration.  A worker goes through
every triple once: a batch of 2 GiB of volumes on device arrays (2 GiB read + 2 GiB written per execution), forward,
out of place, 3 warm-ups, then the median and the range of 9 executions between device events on the stream the plan
runs on.  Both configurations' results are compared on the device, at the size they are timed at, against torch's own
transform of the first and the last 16 volumes.  Rates are algorithmic: one read and one write of the batch over the
time.  A triple counts as faster when the one-trip median is below the axis-by-axis median by more than the two ranges
(max - min of the 9) together.  A worker that fails ends the run.  `triple` arguments (e.g. 16x16x16) restrict the
menu."""
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.environ.get("FFTW_AMD_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WARM, REPS = 3, 9
BYTES = 2 << 30


def menu():
    with open(os.path.join(ROOT, "fftw3_amd", "csrc", "vol3d_menu.inc")) as f:
        return [tuple(int(v) for v in m.groups()) for m in re.finditer(r"X\((\d+), (\d+), (\d+)\)", f.read())]


def worker(triples):
    import torch
    import fftw3_amd as fa
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    xall = torch.view_as_complex(torch.rand(BYTES // 16, 2, dtype=torch.float64, device=dev, generator=g) - 0.5)
    yall = torch.zeros_like(xall)
    for shape in triples:
        n = shape[0] * shape[1] * shape[2]
        hm = BYTES // (16 * n)
        x, y = xall[:hm * n], yall[:hm * n]
        p = fa.plan_many_dft(3, list(shape), hm, x, None, 1, n, y, None, 1, n, fa.FORWARD, fa.ESTIMATE)
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
        head = torch.cat([y[:16 * n], y[-16 * n:]])
        want = torch.fft.fftn(torch.cat([x[:16 * n], x[-16 * n:]]).reshape((-1,) + tuple(shape)), dim=(1, 2, 3)).reshape(-1)
        err = float((head - want).abs().max() / want.abs().max())
        route = " | ".join(ln.strip().lstrip("(").split(" buf")[0] for ln in p.sprint().splitlines()[1:])
        print(json.dumps({"shape": list(shape), "hm": hm, "ms": statistics.median(ts), "lo": min(ts), "hi": max(ts),
                          "err": err, "route": route}), flush=True)
        p.destroy()


def run_worker(env_extra, triples):
    env = dict(os.environ)
    for k in ("FFTW_AMD_VOL3D", "FFTW_AMD_NO_IMG2D", "FFTW_AMD_NO_TUNED"):
        env.pop(k, None)
    env.update(env_extra)
    env["FFTW_AMD_PKG_ROOT"] = ROOT
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"] + ["%dx%dx%d" % t for t in triples]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=480)
    if r.returncode != 0:
        raise SystemExit("worker %s failed with status %d" % (env_extra, r.returncode))
    return {tuple(d["shape"]): d for d in (json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{"))}


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    is_worker = "--worker" in args
    args = [a for a in args if a != "--worker"]
    triples = [tuple(int(v) for v in a.split("x")) for a in args] or menu()
    if is_worker:
        worker(triples)
        return
    one = run_worker({"FFTW_AMD_VOL3D": "1"}, triples)
    axes = run_worker({}, triples)
    lines = ["# one-trip small-volume plans (FFTW_AMD_VOL3D=1) against the axis-by-axis plans of the same build with the knob",
             "# unset (the parent's plans), MI355X.  Per triple a batch of 2 GiB of volumes (hm = 2^31 / (16 n0 n1 n2)), forward,",
             "# out of place, device arrays; median and range (max - min) of %d executions between device events after %d" % (REPS, WARM),
             "# warm-ups, one fresh process per configuration.  TB/s: one read + one write of the batch over the median.",
             "# faster: the one-trip median is below the axis-by-axis median by more than the two ranges together.",
             "# (tools/perf/perf_vol3d.py)",
             "# %3s %3s %3s %8s %9s %7s %6s %9s %7s %6s %6s %7s  %s" % ("n0", "n1", "n2", "hm", "1trip ms", "range", "TB/s",
                                                                        "axes ms", "range", "TB/s", "ratio", "faster",
                                                                        "axis-by-axis plan")]
    not_faster = []
    for t in triples:
        a, b = one[t], axes[t]
        for d in (a, b):
            if d["err"] > 1e-10:
                raise SystemExit("%dx%dx%d: result differs from the reference by %g" % (t + (d["err"],)))
        assert "vol3d" in a["route"] and "vol3d" not in b["route"], (a["route"], b["route"])
        ra, rb = a["hi"] - a["lo"], b["hi"] - b["lo"]
        faster = a["ms"] < b["ms"] - (ra + rb)
        if not faster:
            not_faster.append(t)
        tb = 2.0 * BYTES / 1e12
        lines.append("  %3d %3d %3d %8d %9.4f %7.4f %6.2f %9.4f %7.4f %6.2f %6.2f %7s  %s" % (
            t + (a["hm"], a["ms"], ra, tb / (a["ms"] * 1e-3), b["ms"], rb, tb / (b["ms"] * 1e-3), b["ms"] / a["ms"],
                 "yes" if faster else "NO", b["route"])))
    lines.append("# %d triples, %d not faster than their axis-by-axis plan by more than the two ranges%s" % (
        len(triples), len(not_faster), (": " + " ".join("%dx%dx%d" % t for t in not_faster)) if not_faster else ""))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out if os.path.isabs(out) else os.path.join(os.getcwd(), out), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
