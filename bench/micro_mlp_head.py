#!/usr/bin/env python3
"""Times a fused head kernel alone (HIP events) at batch B: LeNet-5's mlp_head_k (default) or,
with --model reference_cnn, the reference CNN's ce_tail_k.
Usage: python bench/micro_mlp_head.py [B] [iters] [--model lenet5|reference_cnn]
                                      [--label_smoothing EPS] [--rounds N]
With --label_smoothing EPS > 0 the plain kernel (eps = 0) and the smoothed instantiation are timed
in the same process, alternating, `--rounds` windows of `iters` launches each: medians and ranges
of both, and one JSON line."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=None)
ap.add_argument("iters", nargs="?", type=int, default=50)
ap.add_argument("--model", default="lenet5", choices=["lenet5", "reference_cnn"])
ap.add_argument("--label_smoothing", type=float, default=0.0)
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()
B = args.B or (65536 if args.model == "lenet5" else 16384)
iters = args.iters
dev = torch.device("cuda:0")
spec = get_model(args.model, 1)
net = HipNet(spec, B, dev, torch_ref.init_params(spec, seed=0))
kind = {"mlp": "mlp_head", "tail": "ce_tail"}[net.head_kind]
src = net.layers[net.head - 1].out
src.copy_(torch.rand_like(src, dtype=torch.float32).to(torch.bfloat16))
net.labels.copy_(torch.randint(0, 10, (B,), device=dev, dtype=torch.int32))


def window(eps):
    """us per launch over one window of `iters` launches at this smoothing."""
    net.opt.label_smoothing = eps       # _run_head reads it per launch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        net._run_head(B, 1.0 / B, True, net.stats)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


variants = [0.0] + ([args.label_smoothing] if args.label_smoothing > 0 else [])
for eps in variants:                    # warm-up: both code objects loaded before any window
    for _ in range(5):
        net.opt.label_smoothing = eps
        net._run_head(B, 1.0 / B, True, net.stats)
torch.cuda.synchronize()
if len(variants) == 1:
    print(f"{kind} B={B}: {window(0.0):.1f} us")
    sys.exit(0)
times = {eps: [] for eps in variants}
for _ in range(args.rounds):
    for eps in variants:
        times[eps].append(window(eps))
out = {"kernel": kind, "B": B, "iters": iters, "rounds": args.rounds}
for eps in variants:
    t = times[eps]
    print(f"{kind} B={B} label_smoothing={eps}: median {statistics.median(t):.2f} us "
          f"(range {min(t):.2f} .. {max(t):.2f} over {len(t)} windows of {iters})")
    out[f"us_eps_{eps}"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
print(json.dumps(out))
