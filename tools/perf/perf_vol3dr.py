"""measurement (not a test): one-trip small real-volume plans (FFTW_AMD_K_VOL3DR, pass3dr.hpp, FFTW_AMD_REAL_VOL=1)
against the axis-by-axis plans of the same build with the knob unset, r2c and c2r, for every triple of vol3dr_menu.inc.

    timeout -k 10 1100 python tools/perf/perf_vol3dr.py [--out profiles/vol3dr.txt] [--baseline-root DIR] [triple ...]

The plan with the knob unset is the parent commit's plan (tests/test_vol3dr_plans.py pins that); it is the yardstick,
its sprint() goes in the output.  The driver starts one fresh worker process per configuration.  A worker goes through
every triple once, r2c then c2r: a batch of about 1 GiB of real data on device arrays, out of place, dense rows, 3
warm-ups, then the median and the range of 9 executions between device events on the stream the plan runs on.  Both
configurations' results are compared, at the size they are timed at, against numpy's transform on the host of the
first and the last 16 volumes.  Rates are algorithmic: one read of the input and one write of the output (the reals
and the half spectra, (n2 + 2) / n2 times the reals) over the median.  A direction counts as faster when the one-trip
median is below the axis-by-axis median by more than the two ranges (max - min of the 9) together; a triple stays in
the menu when both directions are.  A worker that fails ends the run.  `triple` arguments (e.g. 16x16x16) restrict
the menu.  --baseline-root DIR runs the knob-off configuration from the package built in DIR (a build of the parent
commit) instead of this one."""
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.environ.get("FFTW_AMD_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, REPS = 3, 9
BYTES = 1 << 30


def menu():
    with open(os.path.join(HERE, "fftw3_amd", "csrc", "vol3dr_menu.inc")) as f:
        return [tuple(int(v) for v in m.groups()) for m in re.finditer(r"X\((\d+), (\d+), (\d+)\)", f.read())]


def worker(triples):
    import torch
    import fftw3_amd as fa
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    rall = torch.rand(BYTES // 8, dtype=torch.float64, device=dev, generator=g) - 0.5
    call = torch.view_as_complex(torch.rand(3 * BYTES // 32, 2, dtype=torch.float64, device=dev, generator=g) - 0.5)
    for t in triples:
        n0, n1, n2 = t
        n, h = n0 * n1 * n2, n2 // 2 + 1
        nc = n0 * n1 * h
        hm = BYTES // (8 * n)
        for fwd in (True, False):
            r, c = rall[:hm * n], call[:hm * nc]
            if fwd:
                p = fa.plan_many_dft_r2c(3, list(t), hm, r, None, 1, n, c, None, 1, nc, fa.ESTIMATE)
            else:
                p = fa.plan_many_dft_c2r(3, list(t), hm, c, None, 1, nc, r, None, 1, n, fa.ESTIMATE)
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
            # the first and the last 16 volumes against numpy's transform of the same device data
            rr = torch.cat([r[:16 * n], r[-16 * n:]]).reshape(-1, n0, n1, n2).cpu().numpy()
            cc = torch.cat([c[:16 * nc], c[-16 * nc:]]).reshape(-1, n0, n1, h).cpu().numpy()
            if fwd:
                got, want = cc, np.fft.rfftn(rr, axes=(1, 2, 3))
            else:
                z = np.fft.ifftn(cc, axes=(1, 2), norm="forward")
                z[..., 0] = z[..., 0].real
                z[..., h - 1] = z[..., h - 1].real
                got, want = rr, np.fft.irfft(z, n=n2, axis=3, norm="forward")
            err = float(np.abs(got - want).max() / np.abs(want).max())
            route = " | ".join(ln.strip().lstrip("(").split(" buf")[0] for ln in p.sprint().splitlines()[1:])
            print(json.dumps({"shape": list(t), "fwd": fwd, "hm": hm, "ms": statistics.median(ts), "lo": min(ts),
                              "hi": max(ts), "err": err, "route": route}), flush=True)
            p.destroy()
            if not fwd:
                # the c2r overwrote the reals and (as FFTW's c2r may) possibly its input: fresh data for the next triple
                rall.uniform_(-0.5, 0.5, generator=g)
                torch.view_as_real(call).uniform_(-0.5, 0.5, generator=g)
                torch.cuda.synchronize()


def run_worker(env_extra, triples, root):
    env = dict(os.environ)
    for k in ("FFTW_AMD_REAL_VOL", "FFTW_AMD_REAL_IMG", "FFTW_AMD_VOL3D", "FFTW_AMD_NO_IMG2D", "FFTW_AMD_NO_TUNED"):
        env.pop(k, None)
    env.update(env_extra)
    env["FFTW_AMD_PKG_ROOT"] = root
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"] + ["%dx%dx%d" % t for t in triples]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("worker %s failed with status %d" % (env_extra, r.returncode))
    sys.stderr.write("worker %s done\n" % (env_extra,))
    sys.stderr.flush()
    return {(tuple(d["shape"]), d["fwd"]): d for d in (json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{"))}


def main():
    args = sys.argv[1:]
    out, base_root = None, ROOT
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    if "--baseline-root" in args:
        i = args.index("--baseline-root")
        base_root = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    is_worker = "--worker" in args
    args = [a for a in args if a != "--worker"]
    triples = [tuple(int(v) for v in a.split("x")) for a in args] or menu()
    if is_worker:
        worker(triples)
        return
    one = run_worker({"FFTW_AMD_REAL_VOL": "1"}, triples, ROOT)
    axes = run_worker({}, triples, base_root)
    lines = ["# one-trip small real-volume plans (FFTW_AMD_REAL_VOL=1) against the axis-by-axis plans %s," % (
                 "of the same build with the knob unset (the parent's plans)" if base_root == ROOT else "of a build of the parent commit"),
             "# MI355X.  Per triple a batch of 1 GiB of real data (hm = 2^30 / (8 n0 n1 n2)), out of place, dense rows, device arrays;",
             "# median and range (max - min) of %d executions between device events after %d warm-ups, one fresh process per" % (REPS, WARM),
             "# configuration.  TB/s: one read of the input + one write of the output (the reals and the half spectra) over the",
             "# median.  faster: the one-trip median is below the axis-by-axis median by more than the two ranges together.  A",
             "# triple stays in vol3dr_menu.inc when both directions are faster.  (tools/perf/perf_vol3dr.py)",
             "# %3s %3s %3s %3s %8s %9s %7s %6s %9s %7s %6s %7s %7s  %s" % ("n0", "n1", "n2", "dir", "hm", "1trip ms", "range", "TB/s",
                                                                            "axes ms", "range", "TB/s", "ratio", "faster",
                                                                            "axis-by-axis plan")]
    not_faster = []
    rates, ratios = {True: [], False: []}, {True: [], False: []}
    for t in triples:
        for fwd in (True, False):
            a, b = one[(t, fwd)], axes[(t, fwd)]
            for name, d in (("one-trip", a), ("axis-by-axis", b)):
                if d["err"] > 1e-10:
                    raise SystemExit("%dx%dx%d %s, %s plan (%s): result differs from the reference by %g" % (
                        t + ("r2c" if fwd else "c2r", name, d["route"], d["err"])))
            assert "vol3d-" in a["route"] and "vol3d" not in b["route"], (a["route"], b["route"])
            ra, rb = a["hi"] - a["lo"], b["hi"] - b["lo"]
            faster = a["ms"] < b["ms"] - (ra + rb)
            if not faster and t not in not_faster:
                not_faster.append(t)
            tb = 8.0 * a["hm"] * t[0] * t[1] * (2 * t[2] + 2) / 1e12
            rates[fwd].append(tb / (a["ms"] * 1e-3))
            ratios[fwd].append(b["ms"] / a["ms"])
            lines.append("  %3d %3d %3d %3s %8d %9.4f %7.4f %6.2f %9.4f %7.4f %6.2f %7.2f %7s  %s" % (
                t + ("r2c" if fwd else "c2r", a["hm"], a["ms"], ra, tb / (a["ms"] * 1e-3), b["ms"], rb, tb / (b["ms"] * 1e-3),
                     b["ms"] / a["ms"], "yes" if faster else "NO", b["route"])))
    for fwd in (True, False):
        lines.append("# %s: one-trip %.2f ... %.2f TB/s, %.1f ... %.1f x the axis-by-axis plan" % (
            "r2c" if fwd else "c2r", min(rates[fwd]), max(rates[fwd]), min(ratios[fwd]), max(ratios[fwd])))
    lines.append("# %d triples, %d not faster than their axis-by-axis plan by more than the two ranges in both directions%s" % (
        len(triples), len(not_faster), (": " + " ".join("%dx%dx%d" % t for t in not_faster)) if not_faster else ""))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out if os.path.isabs(out) else os.path.join(os.getcwd(), out), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
