"""bench.py: the plain run's result line and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_and_sampled(gh, tmp_path, monkeypatch):
    """Up to DUMP_SAMPLE bytes the whole output is written; above it the bytes at a fixed
    seeded set of sorted positions, the same from call to call.  The histogram always
    covers the whole output.  (dump_outputs takes any torch uint8 tensor: a CPU one here.)"""
    import torch

    import bench

    data = gh.generate(5, 0.5, 5000)
    out = torch.from_numpy(data.copy())
    bench.dump_outputs(str(tmp_path / "whole"), out, data.size, 375, 0, 1)
    dec = np.load(tmp_path / "whole" / "decoded.npy")
    assert dec.dtype == np.float32 and np.array_equal(dec, data.astype(np.float32))
    hist = np.load(tmp_path / "whole" / "histogram.npy")
    assert hist.dtype == np.float64 and np.array_equal(hist, np.bincount(data, minlength=256))

    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, data.size, 375, 1, 2)
    a = np.load(tmp_path / "a" / "decoded_rank1.npy")
    idx = np.sort(np.random.default_rng(375).integers(0, data.size, size=1000, dtype=np.int64))
    assert a.dtype == np.float32 and np.array_equal(a, data[idx].astype(np.float32))
    assert np.array_equal(a, np.load(tmp_path / "b" / "decoded_rank1.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "histogram_rank1.npy"), hist)


@pytest.mark.gpu
def test_bench_plain_run_dumps_outputs(gpu, tmp_path):
    """A plain run: the contract keys, --steps timed steps, nothing of --full, and the last
    timed decode's output in DIR/decoded.npy == the generator's bytes."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--size", "3000000", "--dump-outputs", str(tmp_path / "o")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["metric"] == "decoded GB/s" and j["unit"] == "GB/s" and j["higher_is_better"] is True
    assert j["dtype"] == "u8" and j["steps"] == 3 and j["warmup"] == 1
    assert j["value"] > 0 and j["ms_per_step"] > 0
    # value = bytes per step / ms_per_step, up to the line's rounding (3 and 4 decimals)
    tol = j["value"] * 0.00005 / (j["ms_per_step"] - 0.00005) + 0.0006
    assert abs(j["value"] - 3000000 / (j["ms_per_step"] * 1e-3) / 1e9) <= tol
    assert j["full"] is False
    for k in ("bitexact", "sub", "sustained", "e2e"):
        assert j[k] is None
    assert "cpu_baseline" not in j and j["roofline"]["copy_gbps"] is None
    data = gpu.generate(375, 0.1, 3000000)
    dec = np.load(tmp_path / "o" / "decoded.npy")
    assert dec.dtype == np.float32 and np.array_equal(dec, data.astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "o" / "histogram.npy"), np.bincount(data, minlength=256))
