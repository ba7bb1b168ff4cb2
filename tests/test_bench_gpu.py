"""bench.py on the MI355X: a plain run is the headline alone, and --dump-outputs writes what the
native timed step computed (small shape: the persistent LSTM kernels at 256 rows)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_dumps_last_step_outputs(tmp_path):
    B, H, F = 256, 512, 16
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "11", "--warmup", "2", "--batch", str(B),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 11 and rec["dtype"] == "bf16" and rec["persistent_fwd"] and rec["persistent_bwd"]
    # timed_s carries 4 decimals: 0.05 ms over 11 steps
    assert rec["ms_per_step"] == pytest.approx(1000.0 * rec["timed_s"] / 11, abs=0.006)
    assert rec["value"] == pytest.approx(B / (rec["ms_per_step"] / 1000.0), rel=1e-3)
    assert "secondary" not in rec and "parity" not in rec
    arrs = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert set(arrs) == {"params", "pred", "loss"}
    for k, a in arrs.items():
        assert a.dtype == np.float32 and a.ndim == 1 and np.isfinite(a).all(), k
    from wellflow.models.lstm import LstmLayout, init_lstm_flat

    assert arrs["pred"].size == B and arrs["params"].size == LstmLayout(F, H).numel
    assert arrs["loss"][0] == pytest.approx(rec["train_loss"], rel=1e-5, abs=1e-6)
    # trained, not the seeded initial weights: every timed step really updated them
    assert np.abs(arrs["params"] - init_lstm_flat(F, H, seed=0).numpy()).max() > 1e-3
    assert arrs["pred"].std() > 0
