"""GPU: the plain benchmark command as it is run for every change -- `bench.py --steps K --warmup W --dump-outputs DIR` in a
fresh process: one JSON line with the headline fields only (the side metrics are --full's), and the last timed step's detections
on disk as a caller of the timed path receives them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["unit"] == "images/sec" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["steps"] == 3 and out["regions"]["count"] == 1 and out["ms_per_step"] > 0
    assert abs(out["value"] - 8 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]
    for k in ("roofline", "kernels_isolated", "energy_ledger", "cpu_baseline", "equivalence_ap", "configs1_r50_b8"):
        assert k not in out, k                       # --full only
    rows = np.load(d / "detections.npy")
    counts = np.load(d / "counts.npy")
    assert rows.dtype == np.float32 and counts.dtype == np.float32 and rows.shape[0] == 8 == counts.shape[0] and rows.shape[2] == 18
    assert abs(float(counts.mean()) - out["config"]["detections_per_image_mean"]) < 1e-6
    assert counts.min() > 0 and np.isfinite(rows).all()
    for i, k in enumerate(counts.astype(np.int64)):
        assert not rows[i, k:].any()
        assert (rows[i, :k, 8] > 0).all()            # scores of the kept detections
