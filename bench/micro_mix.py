#!/usr/bin/env python3
"""Times the mixing kernel (mix.hip) against the plain input kernel on the same buffer, and a whole
LeNet-5 training step with mixup / CutMix on against the same step without (HIP events; one JSON line
at the end).
Usage: python bench/micro_mix.py [--rounds 5] [--iters 100] [--batch 65536] [--step_iters 20]
                                 [--mixup_alpha 0.4 --cutmix_alpha 1.0 --mix_prob 1.0] [--no_step]
* kernels: `mix_images` (mixup alone, CutMix alone, and the two keys together) and `prep_images` on the
  same [65536, 784, 1] bf16 buffer, alternating windows of `iters` back-to-back launches in one process:
  median us of each and TB/s of bytes read + written.  `prep_images` reads one byte and writes one bf16
  per element; `mix_images` reads and writes one bf16 per element of every mixed entry (the buffer is
  mixed again and again, which changes its values and not its traffic).  The yardstick is `prep_images`'
  own rate on this machine: the ratio of the two rates is reported.
* step: Replica.step() (input kernel [+ mix] + the captured training step) of LeNet-5 at `--batch`: the
  keys on (which trains in prep mode), --input_mode prep (the mix launch and the two-label head alone),
  and the default --input_mode bf16.  (`bench.py` has no key for mixing, so the step is measured here.)"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributed_tensorflow_ibm_mnist_amd.data import mix as M
from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.ops._ext import kernels
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--step_iters", type=int, default=20)
ap.add_argument("--mixup_alpha", type=float, default=0.4)
ap.add_argument("--cutmix_alpha", type=float, default=1.0)
ap.add_argument("--mix_prob", type=float, default=1.0)
ap.add_argument("--no_step", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
K = kernels()
N = 60000
cfg = M.MixConfig(args.mixup_alpha, args.cutmix_alpha, args.mix_prob, 7)
out = {"rounds": args.rounds, "mix": [cfg.mixup_alpha, cfg.cutmix_alpha, cfg.prob]}


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
nb = 65536
idx = torch.randint(0, N, (nb,), generator=g).to(dev)
x = torch.empty(nb, 784, 1, dtype=torch.bfloat16, device=dev)
lo = torch.empty(nb, dtype=torch.int32, device=dev)
l2 = torch.empty(nb, dtype=torch.int32, device=dev)
lam = torch.empty(nb, dtype=torch.float32, device=dev)
T = torch.from_numpy(M.lam_table(cfg.mixup_alpha or 0.4)).to(dev)
S = torch.from_numpy(M.side_table(cfg.cutmix_alpha or 1.0)).to(dev)
thr = cfg.thr_p


def mixer(t, s):
    return lambda: K.mix_images(x, lo, l2, lam, nb, 1, 12345, 7, thr, lam_table=t, side_table=s)


fns = {"prep_images": lambda: K.prep_images(src, idx, lab, x, lo, 784, 1, 1), "mix_images mixup": mixer(T, None),
       "mix_images cutmix": mixer(None, S), "mix_images both": mixer(T, S)}
# bytes read + written per element of the buffer: prep 1 + 2; a mixed entry 2 + 2 (CutMix stores whole
# chunks of every mixed entry too)
mixed_share = {}
for k, (t, s) in (("mix_images mixup", (T, None)), ("mix_images cutmix", (None, S)), ("mix_images both", (T, S))):
    prm = torch.empty(nb, 6, dtype=torch.int32, device=dev)
    K.mix_params(prm, 12345, 7, thr, lam_table=t, side_table=s)
    mixed_share[k] = float((prm[:, 0] != 0).float().mean().item())
us = {k: [] for k in fns}
fns["prep_images"]()
for fn in fns.values():
    timed(fn, 10)
for _ in range(args.rounds):
    for k, fn in fns.items():
        us[k].append(timed(fn, args.iters) * 1e3)
res = {}
for k, t in us.items():
    med = statistics.median(t)
    per = 3.0 if k == "prep_images" else 4.0 * mixed_share[k]
    tbs = nb * 784 * per / (med * 1e-6) / 1e12
    print(f"{k} [{nb}, 784, 1] bf16: median {med:.2f} us (range {min(t):.2f} .. {max(t):.2f}), {tbs:.2f} TB/s")
    res[k] = {"us": med, "min": min(t), "max": max(t), "TBps": tbs}
for k in list(res):
    if k != "prep_images":
        res[k]["rate_ratio"] = res[k]["TBps"] / res["prep_images"]["TBps"]
        print(f"  {k}: rate / prep_images' rate = {res[k]['rate_ratio']:.2f}")
out["65536x784x1"] = res

if not args.no_step:
    spec = get_model("lenet5", 1)
    init = torch_ref.init_params(spec, seed=0)
    B = args.batch
    reps = {}
    for name, mode, mix in (("mix", "bf16", cfg), ("prep", "prep", None), ("bf16", "bf16", None)):
        reps[name] = Replica(spec, "hip", B, dev, init, OptConfig(lr0=0.01, use_momentum=True, momentum=0.9, mix=mix is not None),
                             src.cpu(), lab.cpu(), 1, seed=0, use_graph=True, fused_input=mode, mix=mix)
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
