#!/usr/bin/env python3
"""Times the augmentation kernel (augment.hip) against the plain input kernel it replaces, and a whole
LeNet-5 training step with augmentation on against the same step in the prep and bf16 input modes
(HIP events; one JSON line at the end).
Usage: python bench/micro_augment.py [--rounds 5] [--iters 100] [--batch 65536] [--step_iters 20]
                                     [--shift 2 --rotate 15 --scale 0.15] [--no_step]
                                     [--elastic_alpha 34 --elastic_sigma 4]
With --elastic_alpha > 0 the elastic form (augment_elastic.hip) is timed as a third kernel next to the
affine one, alternating in the same process, and a fourth Replica trains with affine + elastic.
* kernels: `augment_images` and `prep_images` on the same random rows of a 60000-image uint8 dataset,
  alternating windows of `iters` back-to-back launches in one process, at out [65536, 784, 1] bf16 and
  (1 -> 3 channels) [16384, 784, 3] bf16: median us of each, their ratio, achieved GB/s (both read one
  byte and write one bf16 per output element).
* step: Replica.step() (input kernel + the captured training step) of LeNet-5 at `--batch`:
  augmentation on (which trains in prep mode), --input_mode prep (the kernel swap alone), and the
  default --input_mode bf16 (which also shows the cost of leaving the fused gather); alternating
  windows of `step_iters` steps.  (`bench.py` has no key for augmentation, so the step is measured here.)"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributed_tensorflow_ibm_mnist_amd.data.augment import AugmentConfig, elastic_weights
from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.ops._ext import kernels
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--step_iters", type=int, default=20)
ap.add_argument("--shift", type=int, default=2)
ap.add_argument("--rotate", type=float, default=15.0)
ap.add_argument("--scale", type=float, default=0.15)
ap.add_argument("--elastic_alpha", type=float, default=0.0)
ap.add_argument("--elastic_sigma", type=float, default=4.0)
ap.add_argument("--no_step", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
K = kernels()
N = 60000
out = {"rounds": args.rounds, "augment": [args.shift, args.rotate, args.scale],
       "elastic": [args.elastic_alpha, args.elastic_sigma]}
table = torch.from_numpy(elastic_weights(args.elastic_sigma).copy()) if args.elastic_alpha > 0 else None


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters      # ms


g = torch.Generator(device="cpu").manual_seed(0)
src = torch.randint(0, 256, (N, 784), dtype=torch.uint8, generator=g).to(dev)
lab = torch.randint(0, 10, (N,), dtype=torch.int32, generator=g).to(dev)
for nb, cd in ((65536, 1), (16384, 3)):
    idx = torch.randint(0, N, (nb,), generator=g).to(dev)
    x = torch.empty(nb, 784, cd, dtype=torch.bfloat16, device=dev)
    lo = torch.empty(nb, dtype=torch.int32, device=dev)
    fns = {"prep_images": lambda: K.prep_images(src, idx, lab, x, lo, 784, 1, cd),
           "augment_images": lambda: K.augment_images(src, idx, lab, x, lo, 1, cd, 12345, 7, args.shift, args.rotate,
                                                      args.scale)}
    if table is not None:
        fns["augment_images_elastic"] = lambda: K.augment_images(src, idx, lab, x, lo, 1, cd, 12345, 7, args.shift,
                                                                 args.rotate, args.scale, elastic_alpha=args.elastic_alpha,
                                                                 elastic_weights=table)
    us = {k: [] for k in fns}
    for fn in fns.values():
        timed(fn, 10)
    for _ in range(args.rounds):
        for k, fn in fns.items():
            us[k].append(timed(fn, args.iters) * 1e3)
    res = {}
    for k, t in us.items():
        med = statistics.median(t)
        gbs = nb * 784 * (1 + 2 * cd) / (med * 1e-6) / 1e9
        print(f"{k} [{nb}, 784, {cd}] bf16: median {med:.2f} us (range {min(t):.2f} .. {max(t):.2f}), {gbs:.0f} GB/s")
        res[k] = {"us": med, "min": min(t), "max": max(t), "GBps": gbs}
    res["ratio"] = res["augment_images"]["us"] / res["prep_images"]["us"]
    print(f"  augment_images / prep_images = {res['ratio']:.2f}")
    if table is not None:
        res["elastic_ratio"] = res["augment_images_elastic"]["us"] / res["augment_images"]["us"]
        print(f"  augment_images with elastic / without = {res['elastic_ratio']:.2f}")
    out[f"{nb}x784x{cd}"] = res

if not args.no_step:
    spec = get_model("lenet5", 1)
    init = torch_ref.init_params(spec, seed=0)
    B = args.batch
    cfg = AugmentConfig(args.shift, args.rotate, args.scale, 7)
    reps = {}
    variants = [("augment", "bf16", cfg), ("prep", "prep", None), ("bf16", "bf16", None)]
    if table is not None:
        variants.insert(0, ("elastic", "bf16", AugmentConfig(args.shift, args.rotate, args.scale, 7, args.elastic_alpha,
                                                             args.elastic_sigma)))
    for name, mode, aug in variants:
        reps[name] = Replica(spec, "hip", B, dev, init, OptConfig(lr0=0.01, use_momentum=True, momentum=0.9), src.cpu(),
                             lab.cpu(), 1, seed=0, use_graph=True, fused_input=mode, augment=aug)
        timed(reps[name].step, 5)
    times = {k: [] for k in reps}
    for _ in range(args.rounds):
        for k, r in reps.items():
            times[k].append(timed(r.step, args.step_iters))
    for k, t in times.items():
        print(f"lenet5 B={B} {k}: median {statistics.median(t):.4f} ms/step "
              f"(range {min(t):.4f} .. {max(t):.4f} over {len(t)} windows of {args.step_iters} steps)")
        out[f"step_ms_{k}"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
        assert reps[k].read_stats()["nan"] == 0.0
    out["batch"] = B
print(json.dumps(out))
