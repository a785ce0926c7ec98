#!/usr/bin/env python3
"""Times a fused head kernel alone (HIP events) at batch B: LeNet-5's mlp_head_k (default) or,
with --model reference_cnn, the reference CNN's ce_tail_k.
Usage: python bench/micro_mlp_head.py [B] [iters] [--model lenet5|reference_cnn]
                                      [--label_smoothing EPS] [--dropout P] [--mix] [--rounds N]
                                      [--distill_alpha A] [--distill_temperature T]
With --label_smoothing EPS > 0 the plain kernel (eps = 0) and the smoothed instantiation are timed
in the same process, alternating, `--rounds` windows of `iters` launches each: medians and ranges
of both, and one JSON line.  --dropout P > 0 (lenet5) does the same with the dropped instantiation
(with --label_smoothing too: plain against dropped + smoothed).  --mix does the same with the two-label
(mixup / CutMix) instantiation, on random second labels and weights in [0.5, 1]; it combines with the
other two.  --distill_alpha A > 0 (alone, with --distill_temperature T) does the same with the distilled
instantiation on random fp32 teacher logits [B, 16]: B x NC x 4 more bytes read per launch."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=None)
ap.add_argument("iters", nargs="?", type=int, default=50)
ap.add_argument("--model", default="lenet5", choices=["lenet5", "reference_cnn"])
ap.add_argument("--label_smoothing", type=float, default=0.0)
ap.add_argument("--dropout", type=float, default=0.0)
ap.add_argument("--mix", action="store_true")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--distill_alpha", type=float, default=0.0)
ap.add_argument("--distill_temperature", type=float, default=2.0)
args = ap.parse_args()
B = args.B or (65536 if args.model == "lenet5" else 16384)
iters = args.iters
dev = torch.device("cuda:0")
spec = get_model(args.model, 1)
net = HipNet(spec, B, dev, torch_ref.init_params(spec, seed=0), OptConfig(dropout=args.dropout, dropout_seed=1234, mix=args.mix))
if args.dropout > 0 and net.head_kind != "mlp":
    sys.exit("--dropout times the fused LeNet-5 head; the reference CNN's dropout is the stand-alone kernels")
if args.distill_alpha > 0 and (args.label_smoothing > 0 or args.dropout > 0 or args.mix):
    sys.exit("--distill_alpha is timed alone: the fused heads have no instantiation that joins it with another target")
kind = {"mlp": "mlp_head", "tail": "ce_tail"}[net.head_kind]
src = net.layers[net.head - 1].out
src.copy_(torch.rand_like(src, dtype=torch.float32).to(torch.bfloat16))
net.labels.copy_(torch.randint(0, 10, (B,), device=dev, dtype=torch.int32))
if args.mix:
    net.labels2.copy_(torch.randint(0, 10, (B,), device=dev, dtype=torch.int32))
    net.mix_lam.copy_(0.5 + 0.5 * torch.rand(B, device=dev))
    net.mix_lam[::4] = 1.0
if args.distill_alpha > 0:
    net.teacher_logits = torch.randn(B, 16, device=dev) * 5.0
    net.opt.distill_temperature = args.distill_temperature


def select(var):
    """(eps, dropped, mixed, distill_alpha): _run_head reads all four per launch."""
    net.opt.label_smoothing, net._drop_pass, net.opt.mix, net.opt.distill_alpha = var


def window(var):
    """us per launch over one window of `iters` launches of this variant."""
    select(var)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        net._run_head(B, 1.0 / B, True, net.stats)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


variants = [(0.0, False, False, 0.0)]
if args.label_smoothing > 0 or args.dropout > 0 or args.mix or args.distill_alpha > 0:
    variants.append((args.label_smoothing, args.dropout > 0, args.mix, args.distill_alpha))
for var in variants:                    # warm-up: both code objects loaded before any window
    select(var)
    for _ in range(5):
        net._run_head(B, 1.0 / B, True, net.stats)
torch.cuda.synchronize()
if len(variants) == 1:
    print(f"{kind} B={B}: {window(variants[0]):.1f} us")
    sys.exit(0)
times = {var: [] for var in variants}
for _ in range(args.rounds):
    for var in variants:
        times[var].append(window(var))
out = {"kernel": kind, "B": B, "iters": iters, "rounds": args.rounds}
for var in variants:
    t = times[var]
    eps, dropped, mixed, alpha = var
    tag = f"label_smoothing={eps}" + (f" dropout={args.dropout}" if dropped else "") + (" mix" if mixed else "")
    if args.distill_alpha > 0:
        tag = f"distill_alpha={alpha}" + (f" distill_temperature={args.distill_temperature}" if alpha > 0 else "")
    print(f"{kind} B={B} {tag}: median {statistics.median(t):.2f} us "
          f"(range {min(t):.2f} .. {max(t):.2f} over {len(t)} windows of {iters})")
    key = f"us_eps_{eps}" + (f"_dropout_{args.dropout}" if dropped else "") + ("_mix" if mixed else "")
    if args.distill_alpha > 0:
        key = f"us_distill_alpha_{alpha}"
        out["teacher_bytes"] = B * 10 * 4
    out[key] = {
        "median": statistics.median(t), "min": min(t), "max": max(t)}
print(json.dumps(out))
