#!/usr/bin/env python3
"""Replica.evaluate with and without the evaluation metrics, and the metrics kernels alone.

    python bench/micro_eval_metrics.py [--batch 128] [--split 10000] [--reps 7] [--rows 65536]
                                       [--models lenet5,reference_cnn]

Per model: a few training steps, then ``evaluate()`` and ``evaluate(metrics=True)`` over a
``split``-image synthetic split alternating in one process, ``reps`` times each after one warm-up
of both (wall clock around a call that ends in a copy to the host).  With metrics the HIP head
runs layer by layer instead of fused, so the difference is that plus two launches per batch plus
one more small copy, not the kernels alone.
Then, once: the kernel pair (eval_metrics_k + eval_metrics_finish_k) on ``rows`` rows of fp32
[rows, 16] and bf16 logits with 10 classes, HIP events around ``reps`` back-to-back calls.  That
reads ``rows * 10`` values and 4 labels bytes per row; at 65536 rows it is about 2.9 MB (fp32),
microseconds of memory traffic: what is measured is launch and the per-block serial float64
summation.  Prints one JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref  # noqa: E402
from distributed_tensorflow_ibm_mnist_amd.obs.eval_metrics import EvalAccumulator  # noqa: E402
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig  # noqa: E402
from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica  # noqa: E402


def _stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def evaluate_pair(model: str, B: int, split: int, reps: int, dev) -> dict:
    spec = get_model(model, 1)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.integers(0, 256, (split, 784), dtype=np.uint8))
    y = torch.arange(split) % 10
    rep = Replica(spec, "hip", B, dev, torch_ref.init_params(spec, seed=0),
                  OptConfig(lr0=0.01, use_momentum=True, momentum=0.9), x, y, 1, x, y, seed=1, log=lambda *_: None)
    for _ in range(5):
        rep.step()
    ms = {False: [], True: []}
    for k in range(reps + 1):
        for flag in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep.evaluate(metrics=flag)
            torch.cuda.synchronize()
            if k:                                       # k = 0 warms both paths up
                ms[flag].append((time.perf_counter() - t0) * 1e3)
    out = {"what": "Replica.evaluate", "model": model, "batch": B, "split": split, "reps": reps,
           "batches": (split + B - 1) // B, "plain_ms": _stat(ms[False]), "metrics_ms": _stat(ms[True])}
    out["added_ms_median"] = round(out["metrics_ms"]["median"] - out["plain_ms"]["median"], 4)
    return out


def kernel_pair(rows: int, reps: int, bf16: bool, dev) -> dict:
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(rows, 16, device=dev, generator=g) * 3
    if bf16:
        logits = logits.bfloat16()
    labels = torch.randint(0, 10, (rows,), device=dev, generator=g, dtype=torch.int32)
    acc = EvalAccumulator(dev, 10)
    us = []
    for k in range(3):
        acc.zero()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            acc.add(logits, labels, rows)
        e1.record()
        torch.cuda.synchronize()
        if k:
            us.append(e0.elapsed_time(e1) * 1e3 / reps)
    bytes_read = rows * (10 * logits.element_size() + 4)
    return {"what": "eval_metrics kernel pair", "rows": rows, "dtype": "bf16" if bf16 else "fp32", "calls": reps,
            "us_per_call": [round(v, 2) for v in us], "bytes_read": bytes_read,
            "GBps_at_best": round(bytes_read / (min(us) * 1e-6) / 1e9, 1)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--split", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--models", default="lenet5,reference_cnn")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("micro_eval_metrics: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    for model in a.models.split(","):
        print(json.dumps(evaluate_pair(model, a.batch, a.split, a.reps, dev)), flush=True)
    for bf16 in (False, True):
        print(json.dumps(kernel_pair(a.rows, max(a.reps, 20), bf16, dev)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
