"""bench.py's plain run: the headline line without the secondary measurements, exactly --steps timed steps,
and --dump-outputs writing the last timed step's loss and trained parameters as float32 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("young_run", "step_us", "roofline", "roofline_sparse", "dcnv2", "din", "uniform", "value_uniform",
             "parity_full_vocab", "reference_dataloader", "cpu_baseline")


def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--vocab-scale", "0.01", "--age-steps", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["unit"] == "samples/sec" and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] - 4096 * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    assert not [k for k in FULL_ONLY if k in d]
    files = sorted(os.listdir(out))
    assert "loss.npy" in files and len(files) > 1
    assert sum(os.path.getsize(os.path.join(out, f)) for f in files) <= 64 << 20
    loss = np.load(os.path.join(out, "loss.npy"))
    assert loss.shape == (1,) and np.isfinite(loss).all()
    for f in files:
        a = np.load(os.path.join(out, f))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    assert any(".embedding_layers." in f for f in files)
