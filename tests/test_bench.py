"""bench.py's own contract: a plain run prints the headline only, --full adds the
roofline / legs / CPU baseline, and --dump-outputs writes what the last timed step
computed (float64, at most 64 MB, the same sample from run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import ROOT, TOL, aerror, oracle_dft

sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _dumped(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def _total_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_writes_small_arrays_whole(tmp_path):
    import torch
    z = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    c = torch.complex(torch.arange(5.0, dtype=torch.float64), -torch.arange(5.0, dtype=torch.float64))
    bench.dump_outputs(str(tmp_path), {"real": z, "cplx": c})
    got = _dumped(str(tmp_path))
    assert set(got) == {"real", "cplx"}
    assert got["real"].dtype == np.float64 and np.array_equal(got["real"], z.numpy())
    assert got["cplx"].shape == (5, 2) and np.array_equal(got["cplx"][:, 0] + 1j * got["cplx"][:, 1], c.numpy())


def test_dump_outputs_samples_a_large_array_within_the_cap(tmp_path):
    import torch
    g = torch.Generator().manual_seed(3)
    y = torch.complex(torch.rand((40, 1 << 17), dtype=torch.float64, generator=g),
                      torch.rand((40, 1 << 17), dtype=torch.float64, generator=g))   # 80 MiB
    bench.dump_outputs(str(tmp_path / "a"), {"out": y})
    bench.dump_outputs(str(tmp_path / "b"), {"out": y})
    a, b = _dumped(str(tmp_path / "a")), _dumped(str(tmp_path / "b"))
    assert set(a) == {"out_first", "out_sample"}
    assert _total_bytes(str(tmp_path / "a")) <= 64 * 10**6
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k])
    assert np.array_equal(a["out_first"][:, 0] + 1j * a["out_first"][:, 1], y[0].numpy())
    k = (bench.DUMP_BYTES - y.shape[1] * 16) // 16
    idx = np.unique(np.random.default_rng(0).integers(0, y.numel(), k, dtype=np.int64))
    s = a["out_sample"]
    assert np.array_equal(s[:, 0] + 1j * s[:, 1], y.reshape(-1).numpy()[idx])
    assert idx[-1] >= y.numel() - y.numel() // 100          # the sample reaches the end of the batch


def test_bench_rejects_zero_steps(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    import torch
    b, n = 4, 1 << 20
    line = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", str(b),
                   "--dump-outputs", str(tmp_path)])
    for k in HEADLINE_KEYS:
        assert k in line, k
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["dtype"] == "f64"
    assert "roofline" not in line and "cpu_baseline" not in line and "legs" not in line["config"]
    assert _total_bytes(str(tmp_path)) <= 64 * 10**6
    got = _dumped(str(tmp_path))
    assert set(got) == {"out_first", "out_sample"}
    # the input bench.py generates for the headline workload (one slab at this batch)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    x = (torch.rand((b, n, 2), dtype=torch.float64, device=dev, generator=gen) - 0.5).cpu().numpy()
    x = x[..., 0] + 1j * x[..., 1]
    want = oracle_dft(x, (n,), b).reshape(b, n)
    first = got["out_first"][:, 0] + 1j * got["out_first"][:, 1]
    assert aerror(first, want[0]) < TOL
    k = (bench.DUMP_BYTES - n * 16) // 16
    idx = np.unique(np.random.default_rng(0).integers(0, b * n, k, dtype=np.int64))
    s = got["out_sample"][:, 0] + 1j * got["out_sample"][:, 1]
    assert np.abs(s - want.reshape(-1)[idx]).max() < TOL * np.abs(want).max()


@pytest.mark.gpu
def test_full_adds_the_roofline():
    line = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4", "--full",
                   "--no-legs", "--no-cpu-baseline"])
    assert line["steps"] == 2 and line["roofline"]["per_launch"]["launches_per_step"] >= 1
