#!/usr/bin/env python3
"""Times the stand-alone dropout kernels (dropout.hip) and a whole training step with and without
dropout (HIP events; one JSON line at the end).
Usage: python bench/micro_dropout.py [--p 0.5] [--rounds 5] [--iters 200]
                                     [--model reference_cnn] [--batch 16384] [--step_iters 20]
* kernels: dropout_fwd / dropout_bwd in place on [16384, 1024] and [16384, 192] bf16, windows of
  `iters` back-to-back launches: median us and achieved GB/s (every element read and written once).
* step: the captured training step of `--model` at `--batch`, a net with OptConfig(dropout=p) and one
  without, alternating windows of `step_iters` replays: median ms per step of each.  (`bench.py`
  builds its own OptConfig and has no dropout key, so the step is measured here.)"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.ops._ext import kernels
from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
from distributed_tensorflow_ibm_mnist_amd.runtime.graph import StepGraph
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig

ap = argparse.ArgumentParser()
ap.add_argument("--p", type=float, default=0.5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--model", default="reference_cnn", choices=["reference_cnn", "lenet5", "mlp"])
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--step_iters", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda:0")
K = kernels()
out = {"p": args.p, "rounds": args.rounds}


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters      # ms


step = torch.zeros(1, dtype=torch.int64, device=dev)
for nb, n in ((16384, 1024), (16384, 192)):
    x = torch.rand(nb, n, device=dev).to(torch.bfloat16)
    for name, kern in (("fwd", K.dropout_fwd), ("bwd", K.dropout_bwd)):
        fn = lambda: kern(x, nb, n, n, step, 1234, 3, args.p)
        timed(fn, 10)
        us = [timed(fn, args.iters) * 1e3 for _ in range(args.rounds)]
        med = statistics.median(us)
        gbs = 2 * nb * n * 2 / (med * 1e-6) / 1e9
        print(f"dropout_{name} [{nb}, {n}]: median {med:.2f} us (range {min(us):.2f} .. {max(us):.2f}), {gbs:.0f} GB/s")
        out[f"dropout_{name}_{nb}x{n}"] = {"us": med, "min": min(us), "max": max(us), "GBps": gbs}

spec = get_model(args.model, 1)
init = torch_ref.init_params(spec, seed=0)
B = args.batch
graphs = {}
for p in (0.0, args.p):
    net = HipNet(spec, B, dev, init, OptConfig(lr0=0.01, use_momentum=True, momentum=0.9, dropout=p, dropout_seed=1234))
    g = torch.Generator(device=dev).manual_seed(0)
    net.x0.copy_((torch.rand(B, 28, 28, 1, device=dev, generator=g) - 0.5).to(torch.bfloat16))
    net.labels.copy_(torch.randint(0, 10, (B,), device=dev, generator=g, dtype=torch.int32))
    graphs[p] = (net, StepGraph(net.train_step, warmup=3))
    timed(graphs[p][1].replay, 5)
times = {p: [] for p in graphs}
for _ in range(args.rounds):
    for p, (_, sg) in graphs.items():
        times[p].append(timed(sg.replay, args.step_iters))
for p, t in times.items():
    print(f"{args.model} B={B} dropout={p}: median {statistics.median(t):.4f} ms/step "
          f"(range {min(t):.4f} .. {max(t):.4f} over {len(t)} windows of {args.step_iters} replays)")
    out[f"step_ms_dropout_{p}"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    assert graphs[p][0].read_stats()["nan"] == 0.0
out.update(model=args.model, batch=B)
print(json.dumps(out))
