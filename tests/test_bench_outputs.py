"""bench.py ``--dump-outputs`` and the plain / ``--full`` split.

CPU: the dump writer (dtypes, the seeded sample of an array over its byte share).
GPU: one plain bench run writes the state its last timed step produced, reports the
timed steps it was asked for, and measures nothing after them.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_dtypes_and_seeded_sample(tmp_path, monkeypatch):
    import bench
    big = torch.arange(1000, dtype=torch.float32)
    tensors = {"w": big, "h": torch.tensor([1.5, -2.0], dtype=torch.bfloat16),
               "step": torch.tensor([7], dtype=torch.int64)}
    bench.dump_outputs(str(tmp_path / "a"), tensors)
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in tensors}
    assert a["w"].dtype == np.float32 and np.array_equal(a["w"], big.numpy())
    assert a["h"].dtype == np.float32 and a["h"].tolist() == [1.5, -2.0]
    assert a["step"].dtype == np.float64 and a["step"].tolist() == [7.0]
    # 3 arrays share 1200 bytes: 400 bytes = 100 float32 each; only "w" is over its share
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 1200)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), tensors)
    b, c = (np.load(tmp_path / d / "w.npy") for d in ("b", "c"))
    assert b.shape == (100,) and np.array_equal(b, c)            # the same sample every time
    assert len(set(b.tolist())) == 100 and set(b.tolist()) <= set(big.tolist()) and np.all(np.diff(b) > 0)
    assert np.load(tmp_path / "b" / "h.npy").tolist() == [1.5, -2.0]
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) < 1200 + 3 * 256


@pytest.mark.gpu
def test_plain_bench_dumps_last_step_and_skips_extras(dev, tmp_path):
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--batch", "512", "--graph", "0", "--prewarm_steps", "5", "--prewarm_ms", "0",
                        "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["steps"] == 4 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["full"] is False
    assert out["unit"] == "images/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert abs(out["value"] - 512 / out["ms_per_step"] * 1e3) <= 1e-3 * out["value"]
    # the per-phase steps (--phases defaults to 3), like every other extra, are left to --full
    assert out["phase_ms_eager"] is None and out["comm"] is None and out["pg"] is None
    assert out["config"]["hip_graph"] is False and out["ms_per_step_eager"] == out["ms_per_step"]
    got = {f[:-4]: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
    assert sorted(got) == ["ema", "loss_ema", "mom", "params", "stats", "step"]
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    # the dump is the state right after the last timed step: W + K steps, nothing after them
    assert got["step"].tolist() == [6.0]
    assert got["params"].shape == got["mom"].shape == got["ema"].shape and np.abs(got["mom"]).max() > 0
    assert abs(float(got["stats"][4]) - out["final_train_loss"]) <= 1e-5
