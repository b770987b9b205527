"""bench.py without --full: the headline alone (no calibration run, roofline, skips-off loops or CPU baseline), and
--dump-outputs: what the last timed step computed, the same in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "per_pass_ms", "measured_read_gbps", "ms_per_step_noskip", "ms_per_step_median", "cpu_baseline", "exchange_wait_ms")


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frame", "640x360",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, f"exactly one line on stdout, got {len(lines)}: {lines[:3]}"
    return json.loads(lines[0])


def test_plain_run_and_its_outputs(tmp_path):
    d = _bench(tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["unit"] == "Mpixels/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["config"]["frame"] == [640, 360]
    assert d["ms_per_step"] > 0 and abs(d["value"] - 640 * 360 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]
    assert not [k for k in FULL_ONLY if k in d], "a plain run measures the headline only"
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["ao.npy", "reflections.npy", "taa_output.npy"], names
    again = _bench(tmp_path / "b")
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        # smaller than the sample: written whole (the AO and the reflections at half resolution, the TAA output at full)
        assert a.dtype == np.float32 and a.shape[:2] == ((360, 640) if n == "taa_output.npy" else (180, 320)), (n, a.dtype, a.shape)
        assert np.array_equal(a, b, equal_nan=True), f"{n}: two runs with the same arguments computed different outputs"
        total += a.nbytes
    assert total <= 64 << 20
    assert np.isfinite(np.load(tmp_path / "a" / "taa_output.npy")).all() and again["steps"] == 3
