"""c2r of n = L1 x 2048 real points in two trips (FFTW_AMD_F_REAL_DEC_C2R, FFTW_AMD_REAL_DEC=1) against the three-trip
plan FFTW_ESTIMATE picks (the same binary with the variable unset): ms per batch of 4 GiB of real output -- after a
warm-up, the median (and min ... max) of PERF_REPS timed executions with the default two chunk lanes -- whole % of the
8 TB/s roofline on the algorithmic bytes (8 n in + 8 n out), error against torch.fft.irfft, and the per-step times of
fftw_amd_execute_profiled"""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import fftw3_amd as fa
reps = int(os.environ.get("PERF_REPS", "9"))
out = torch.zeros((4 << 30) // 8, dtype=torch.float64, device="cuda")
for n in ([int(v) for v in os.environ["PERF_N"].split(",")] if os.environ.get("PERF_N") else (1 << 22, 1 << 21, 1 << 20)):
    hm = out.numel() // n
    z = out[:hm * n].reshape(hm, n)
    y = torch.fft.rfft(torch.rand(hm, n, dtype=torch.float64, device="cuda") - 0.5, dim=1)
    ref = torch.fft.irfft(y[:2], n=n, dim=1) * n
    line = "%8d x %-5d" % (n, hm)
    for old in (0, 1):
        if old: os.environ.pop("FFTW_AMD_REAL_DEC", None)
        else: os.environ["FFTW_AMD_REAL_DEC"] = "1"
        p = fa.plan_many_dft_c2r(1, [n], hm, y, None, 1, n // 2 + 1, z, None, 1, n)
        for _ in range(2): p.execute(); p.sync()
        err = float((z[:2] - ref).abs().max() / ref.abs().max())
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter(); p.execute(); p.sync(); ts.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ts)
        prof = p.execute_profiled()
        line += " | %s %d trips %7.3f ms (%.3f ... %.3f) %5.1f %% err %.1e lanes %d steps [%s]" % (
            "old" if old else "new", len(p.steps()), med, min(ts), max(ts), 100 * 16.0 * n * hm / (med * 1e-3) / 8e12, err,
            p.lanes, ", ".join("%.3f" % ms for _, ms, _ in prof))
        del p
    os.environ.pop("FFTW_AMD_REAL_DEC", None)
    print(line, flush=True)
    del y, ref
