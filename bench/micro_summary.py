#!/usr/bin/env python3
"""One Monitor.write_train, host path against device path (obs/device_summary.py).

    python bench/micro_summary.py [--batch 128] [--reps 5] [--models lenet5,reference_cnn]

Per model: one training step, then write_train alternating host / device in one process,
``reps`` times each after one warm-up of both (wall clock around a call that ends synchronised:
both paths end in copies to the host), and the device path's launches alone (HIP events around
DeviceSummarizer's kernels, no copy).  Prints one JSON line per model.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref  # noqa: E402
from distributed_tensorflow_ibm_mnist_amd.obs.monitor import Monitor  # noqa: E402
from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet  # noqa: E402
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig  # noqa: E402


class _Replica:
    world = 1

    def __init__(self, net, spec):
        self.net, self.spec = net, spec

    def read_stats(self):
        return self.net.read_stats()


def measure(model: str, B: int, reps: int, dev) -> dict:
    spec = get_model(model, 1)
    net = HipNet(spec, B, dev, torch_ref.init_params(spec, seed=0), OptConfig(lr0=0.05, use_momentum=True, momentum=0.9))
    g = torch.Generator(device=dev).manual_seed(0)
    net.x0.copy_((torch.rand(B, 28, 28, 1, device=dev, generator=g) - 0.5).to(torch.bfloat16))
    net.labels.copy_(torch.randint(0, 10, (B,), device=dev, generator=g, dtype=torch.int32))
    net.train_step()
    torch.cuda.synchronize()
    rep = _Replica(net, spec)
    with tempfile.TemporaryDirectory() as tmp:
        mons = {}
        for name, flag in (("host", False), ("device", True)):
            mons[name] = Monitor(os.path.join(tmp, name), 1, 1, rep, device_summaries=flag)
            mons[name].register_reference_summaries()
        ms = {"host": [], "device": []}
        for k in range(reps + 1):
            for name in ("host", "device"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mons[name].write_train(k + 1)
                torch.cuda.synchronize()
                if k:                                   # k = 0 warms both paths up
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        # the launches alone, on the tensors write_train used
        m = mons["device"]
        _, _, _, jobs = m._device_jobs()
        S = m._summarizer
        nseg = sum(len(j[1]) for j in jobs)
        counts, stats = S._buffers(nseg)
        tables = [torch.tensor([list(map(int, s)) for s in j[1]], dtype=torch.int64).view(-1, 4) for j in jobs]
        kern = []
        for k in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            at = 0
            for (src, _, div), tab in zip(jobs, tables):
                n = tab.shape[0]
                S.K.summary_stats(src, tab, S.limits, counts[at:at + n], stats[at:at + n], S._scratch, float(div))
                at += n
            e1.record()
            torch.cuda.synchronize()
            if k:
                kern.append(e0.elapsed_time(e1))
        for mon in mons.values():
            mon.close()
    elems = sum(int(s[1]) * int(s[2]) for j in jobs for s in j[1])
    out = {"model": model, "batch": B, "reps": reps, "segments": nseg, "launch_sets": len(jobs), "elements": elems,
           "d2h_bytes_device_path": nseg * (32 + 4 * (S.nb + 1))}
    for name, v in (("host_ms", ms["host"]), ("device_ms", ms["device"]), ("device_kernels_ms", kern)):
        out[name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["speedup_median"] = round(out["host_ms"]["median"] / out["device_ms"]["median"], 2)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", default="lenet5,reference_cnn")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("micro_summary: needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    for model in a.models.split(","):
        print(json.dumps(measure(model, a.batch, a.reps, dev)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
