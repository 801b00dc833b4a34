"""bench.py's output contract on the GPU: one JSON line with the driver's keys; with --full the
roofline and cpu_baseline objects and the streaming figure's detail; a plain run the headline keys
alone and, with --dump-outputs, the last timed step's output (short runs: 3 timed steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", *args]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_line_contract():
    d = run_bench("--full", "--no-cpu-baseline", "--no-traffic", "--no-per-sample", "--side-steps", "0",
                  "--stream-blocks", "16")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"] == "f64"
    assert "workload" in d["config"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] in ("hbm", "mfma") and 0 < rf["frac"] < 1.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    st = d["streaming"]
    assert st["block"] == 1024 and st["us_per_block"] > 0
    assert st["kernels"] and st["roofline"]["bound"].startswith("latency")
    # 1024-sample calls of the stationary C2 bank take the streaming engine: one launch per block
    assert st["path"] == "stream" and st["launches_per_block"] == 1, st
    assert st["end_to_end_host_buffers"]["us_per_block"] > 0
    assert st["per_band_engine"]["path"] == "lti"


@pytest.mark.gpu
def test_bench_plain_line_and_dump(tmp_path):
    """A plain run: the headline keys and nothing that takes a run of its own; --dump-outputs leaves
    the last timed call's 480,000 output samples (float64, the C2 bank's mix of the seeded input)."""
    out = tmp_path / "dump"
    d = run_bench("--dump-outputs", str(out))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype"):
        assert k in d, k
    for k in ("roofline", "cpu_baseline", "streaming", "side", "per_sample"):
        assert k not in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["unit"] == "band-samples/s" and d["ms_per_step"] > 0
    # value is the timed steps' band-samples over their time
    assert abs(d["value"] - 4096 * 480000 / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    assert [p.name for p in out.iterdir()] == ["y.npy"]
    y = np.load(out / "y.npy")
    assert y.dtype == np.float64 and y.shape == (480000,)
    assert np.all(np.isfinite(y)) and np.max(np.abs(y)) > 0
