"""Device summaries, the parts that need no GPU: histogram_proto_from_stats against
histogram_proto byte for byte, the boundary inputs of the GPU tests against the oracle (this pins
the test data, not the kernel), and the --monitor_device flag's fallback on a CPU executor."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from distributed_tensorflow_ibm_mnist_amd.obs import events
from distributed_tensorflow_ibm_mnist_amd.obs.events import BUCKET_LIMITS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("summary_oracle", os.path.join(ROOT, "tests", "summary_oracle.py"))
oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(oracle)

RNG = np.random.default_rng(5)
CASES = {
    "normals": RNG.standard_normal(4097).astype(np.float32),
    "single": np.array([0.37], np.float32),
    "zeros": np.zeros(33, np.float32),
    "negatives": -np.abs(RNG.standard_normal(1000)).astype(np.float32) - 1e-3,
}


@pytest.mark.parametrize("name", list(CASES))
def test_proto_from_stats_is_histogram_proto_bytewise(name):
    v = CASES[name].astype(np.float64)
    idx = np.searchsorted(BUCKET_LIMITS, v, side="left")
    counts = np.bincount(idx, minlength=len(BUCKET_LIMITS))
    got = events.histogram_proto_from_stats(v.min(), v.max(), v.size, v.sum(), (v * v).sum(), counts)
    assert got == events.histogram_proto(CASES[name])
    # the oracle's counts and moments are those six quantities
    c, s = oracle.reference(CASES[name], [(0, 1, v.size, v.size)], BUCKET_LIMITS)
    assert c[0, -1] == 0 and np.array_equal(c[0, :-1], counts)
    assert s[0, 0] == v.min() and s[0, 1] == v.max()
    assert events.histogram_proto_from_stats(s[0, 0], s[0, 1], c[0].sum(), v.sum(), (v * v).sum(), c[0, :-1]) == got


def test_table_has_at_most_8_limits_per_binade():
    pos = BUCKET_LIMITS[BUCKET_LIMITS > 0][:-1]
    assert len(BUCKET_LIMITS) == 1551 and np.bincount(np.frexp(pos)[1] - np.frexp(pos)[1].min()).max() <= 8


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_boundary_set_lands_where_it_is_meant_to(kind):
    vals, want = oracle.boundary_set(kind)
    nb = len(BUCKET_LIMITS)
    n_inner = nb - 2
    le, gt = vals[:n_inner].astype(np.float64), vals[n_inner:2 * n_inner].astype(np.float64)
    lim = BUCKET_LIMITS[1:-1]
    assert (le <= lim).all() and (gt > lim).all()
    if kind == "fp32":      # neighbours in fp32: nothing representable lies between them
        assert (np.nextafter(vals[:n_inner], np.float32(np.inf)) == vals[n_inner:2 * n_inner]).all()
    else:                   # exactly bf16, and neighbours there: one step of the 8-bit mantissa
        assert (vals.view(np.uint32) & 0xffff == 0).all()
        a, b = vals[:n_inner].view(np.uint32) >> 16, vals[n_inner:2 * n_inner].view(np.uint32) >> 16
        step = np.abs(a.astype(np.int64) - b.astype(np.int64))
        zero = lim == 0.0   # 0.0 -> the smallest positive bf16 (a denormal)
        assert (step[~zero] == 1).all() and le[zero][0] == 0.0 and b[zero][0] == 1
    idx = np.searchsorted(BUCKET_LIMITS, vals.astype(np.float64), side="left")
    assert np.array_equal(idx, want)
    # each inner bucket edge is hit from both sides, the zeros share the 0.0 limit's bucket
    zero_b = int(np.where(BUCKET_LIMITS == 0.0)[0][0])
    tail = dict(zip(vals[2 * n_inner:].tolist(), want[2 * n_inner:].tolist()))
    assert want[2 * n_inner] == zero_b and want[2 * n_inner + 1] == zero_b and np.signbit(vals[2 * n_inner + 1])
    big = float(vals[2 * n_inner + 2])
    assert tail[big] == nb - 1 and tail[-big] == 1
    if kind == "fp32":
        assert big == float(np.finfo(np.float32).max)
        assert BUCKET_LIMITS[zero_b + 1] == 1e-12 and BUCKET_LIMITS[zero_b - 1] == -1e-12
        for d in (1e-45, 1e-40, 1.1754942e-38):
            assert tail[float(np.float32(d))] == zero_b + 1 and tail[float(np.float32(-d))] == zero_b
    # the oracle agrees, as one segment, and counts NaN and both infinities in the last column
    ext = np.concatenate([vals, np.array([np.nan, np.inf, -np.inf], np.float32)])
    c, s = oracle.reference(ext, [(0, 1, ext.size, ext.size)], BUCKET_LIMITS)
    assert c[0, nb] == 3 and np.array_equal(c[0, :nb], np.bincount(want, minlength=nb))
    assert s[0, 0] == -big and s[0, 1] == big and np.isfinite(s[0]).all()


def test_oracle_padding_offset_and_divisor():
    v = np.full(100, 1e30, np.float32)
    v[7 + np.arange(5)[:, None] * 8 + np.arange(6)[None, :]] = np.arange(30, dtype=np.float32).reshape(5, 6)
    c, s = oracle.reference(v, [(7, 5, 6, 8), (0, 0, 0, 0)], BUCKET_LIMITS, divisor=3)
    d = (np.arange(30, dtype=np.float32) / 3).astype(np.float64)
    assert c[0].sum() == 30 and c[0, -1] == 0 and s[0, 1] == d.max() and s[0, 0] == 0.0
    assert abs(s[0, 2] - d.sum()) < 1e-12 and list(s[1]) == [np.inf, -np.inf, 0.0, 0.0] and c[1].sum() == 0
    nan = np.array([np.nan], np.float32)
    nan.view(np.uint32)[0] = 0x7fc12345
    assert oracle.divided(nan, 1).view(np.uint32)[0] == 0x7fc12345


def _tags(logdir):
    tags = set()
    for f in events.find_event_files(logdir):
        for ev in events.read_events(f):
            tags |= set(ev["values"])
    return tags


def test_monitor_device_flag_falls_back_on_cpu(tmp_path):
    """--impl=torch --cpu has no device tensors: --monitor_device=1 writes what =0 writes."""
    out = {}
    for flag in (0, 1):
        d = str(tmp_path / f"m{flag}")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--impl=torch", "--cpu", "--model=mlp",
                            "--in_channels=1", "--batch_size=16", "--max_steps=4", "--test_interval=2",
                            "--log_step_count_steps=0", "--train_data=synthetic://300",
                            "--test_data=synthetic://100?seed=1", "--eval_examples=100", f"--train_dir={d}",
                            f"--monitor_device={flag}"], cwd=ROOT, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, OMP_NUM_THREADS="2", PYTHONUNBUFFERED="1"))
        assert r.returncode == 0, r.stderr[-2000:]
        out[flag] = _tags(os.path.join(d, "log"))
    assert out[0] == out[1]
    for t in ("train loss", "train accuracy", "test loss", "test accuracy"):
        assert t in out[1], t
    assert any(t.startswith("gradient/") for t in out[1]) and any(t.startswith("gw_ratio/") for t in out[1])
