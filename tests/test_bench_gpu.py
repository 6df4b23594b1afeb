"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run - the headline alone, timed over exactly K steps, and the
last timed step's results written by --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_k_steps_and_dumps_the_last_one(tmp_path):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "utt/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 3 and d["steps_timed_per_window"] == 3 and d["windows"] == 1
    # two eager steps + the capture pass of the hipGraph replay, W warm-up steps, K timed steps - nothing else
    assert d["steps_run_total"] == 3 + 2 + 3
    assert d["value"] == pytest.approx(64 * 1e3 / d["ms_per_step"], rel=2e-3)
    for key in ("windowed", "roofline", "configs", "cpu_baseline", "headline_repeat_at_end"):
        assert key not in d, key  # --full only
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sorted(got) == ["loss", "neg_scores", "state"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64_000_000
    assert got["loss"].shape == (1,) and round(float(got["loss"][0]), 5) == d["final_loss"]
    assert got["neg_scores"].shape == (64,)
    # ResNet-18 + OC-Softmax: 12,450,290 parameters + the 256-float loss centre + 7,232 BatchNorm running statistics
    assert got["state"].shape == (12_457_778,)
