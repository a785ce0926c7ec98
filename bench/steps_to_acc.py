#!/usr/bin/env python3
"""Second BASELINE metric: steps to 99% train accuracy (MNIST LeNet-5).

Trains from random init on synthetic 28x28x1 data and, every ``--eval_every``
steps, measures top-1 accuracy on a fixed probe of ``--probe`` TRAINING images
(forward only, same kernels).  Reports the first global step at which the probe
accuracy reaches ``--target`` (default 0.99), plus wall time and images seen.

    python bench/steps_to_acc.py [--batch 128] [--lr 0.01] [--optimizer momentum|adam|...]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 \
        bench/steps_to_acc.py ...          (data parallel: global batch = N x batch)
    python bench/steps_to_acc.py --cpu --impl torch --model mlp     (CPU plumbing)

Defaults follow the reference's training hyperparameters where it has them
(batch 128) and BASELINE's model (LeNet-5).  Rank 0 prints one
JSON line; ``value`` is the step count (lower is better), null if the target
was not reached within ``--max_steps``.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LABEL = {"lenet5": "LeNet-5", "reference_cnn": "reference CNN (mnist_input.inference)", "mlp": "MLP 784-128-10"}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="lenet5", choices=sorted(LABEL))
    ap.add_argument("--in_channels", type=int, default=1)
    ap.add_argument("--batch", type=int, default=128, help="per-rank batch")
    ap.add_argument("--optimizer", default="momentum", choices=["sgd", "momentum", "nesterov", "adam", "rmsprop", "adagrad", "lars", "lamb"],
                    help="adam / rmsprop / adagrad: TF1 defaults (pass a matching --lr, e.g. 0.001 for adam)")
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--clip_norm", type=float, default=None, help="clip the gradients by this global norm")
    ap.add_argument("--lars_eta", type=float, default=0.001, help="lars: trust coefficient")
    ap.add_argument("--lr_schedule", default="staircase", choices=["staircase", "polynomial", "cosine"],
                    help="polynomial / cosine: decay from the end of the warmup to --lr_end at --lr_total_steps")
    ap.add_argument("--warmup_steps", type=int, default=0, help="linear warmup in front of any schedule")
    ap.add_argument("--lr_total_steps", type=int, default=None, help="polynomial / cosine (default: --max_steps)")
    ap.add_argument("--lr_end", type=float, default=0.0)
    ap.add_argument("--lr_power", type=float, default=1.0, help="polynomial: the exponent")
    ap.add_argument("--label_smoothing", type=float, default=0.0,
                    help="train against (1 - eps) * onehot + eps / 10; the accuracy probe is an eval and unaffected")
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="drop rate on the hidden dense layers, training only; the accuracy probe is an eval")
    ap.add_argument("--augment_shift", type=int, default=0,
                    help="random translation of the training images, pixels (0..8); the accuracy probe is an eval")
    ap.add_argument("--augment_rotate", type=float, default=0.0, help="random rotation, degrees (0..180)")
    ap.add_argument("--augment_scale", type=float, default=0.0, help="random zoom in [1 - z, 1 + z) (0..0.5)")
    ap.add_argument("--augment_elastic_alpha", type=float, default=0.0,
                    help="elastic distortion: displacement scale of the smoothed random field, pixels (0..64)")
    ap.add_argument("--augment_elastic_sigma", type=float, default=4.0,
                    help="elastic distortion: standard deviation of the smoothing Gaussian, pixels (0.5..8)")
    ap.add_argument("--mixup_alpha", type=float, default=0.0,
                    help="mixup of the training batches, the weight from Beta(a, a) (0.1..8); the accuracy probe is an eval")
    ap.add_argument("--cutmix_alpha", type=float, default=0.0, help="CutMix, the box area from Beta(a, a) (0.1..8)")
    ap.add_argument("--mix_prob", type=float, default=1.0, help="probability that a batch entry is mixed at all")
    ap.add_argument("--mix_seed", type=int, default=None, help="seed of the mixing draws (default: --seed)")
    ap.add_argument("--target", type=float, default=0.99)
    ap.add_argument("--eval_every", type=int, default=50)
    ap.add_argument("--probe", type=int, default=10000, help="training images in the accuracy probe")
    ap.add_argument("--max_steps", type=int, default=20000)
    ap.add_argument("--dataset_size", type=int, default=60000)
    ap.add_argument("--noise", type=float, default=0.25, help="synthetic-data noise amplitude")
    ap.add_argument("--style", default="hand", choices=["hand", "glyph"],
                    help="synthetic generator: hand = per-sample re-drawn strokes (default), glyph = shifted templates")
    ap.add_argument("--impl", default="hip", choices=["hip", "torch"])
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--graph", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fused_input", type=int, default=0, help="first conv reads the uint8 dataset directly")
    return ap.parse_args(argv)


def run(args) -> dict:
    import torch
    import torch.distributed as dist

    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceDataset, DeviceLoader, eval_batches
    from distributed_tensorflow_ibm_mnist_amd.data.synthetic import make_synthetic
    from distributed_tensorflow_ibm_mnist_amd.models import get_model
    from distributed_tensorflow_ibm_mnist_amd.models.torch_ref import init_params
    from distributed_tensorflow_ibm_mnist_amd.parallel.dp import DataParallel
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.cpu:
        dev = torch.device("cpu")
        if world > 1:
            dist.init_process_group("gloo")
    else:
        dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
        if world > 1:
            dist.init_process_group("nccl", device_id=dev)
    spec = get_model(args.model, args.in_channels)
    total = args.lr_total_steps if args.lr_total_steps is not None else args.max_steps
    sched = dict(schedule=args.lr_schedule, warmup_steps=args.warmup_steps, lr_end=args.lr_end, lr_power=args.lr_power,
                 total_steps=total if args.lr_schedule != "staircase" else 0)
    if args.optimizer in ("adam", "rmsprop", "adagrad", "lamb"):
        opt = OptConfig(lr0=args.lr, decay_rate=0.1, decay_steps=0, ema_max=0.9999, rule=args.optimizer,
                        clip_norm=args.clip_norm, **sched)
    elif args.optimizer == "lars":
        opt = OptConfig(lr0=args.lr, decay_rate=0.1, decay_steps=0, ema_max=0.9999, rule="lars", momentum=0.9,
                        lars_eta=args.lars_eta, **sched)
    else:
        opt = OptConfig(lr0=args.lr, decay_rate=0.1, decay_steps=0, momentum=0.9 if args.optimizer != "sgd" else 0.0,
                        nesterov=args.optimizer == "nesterov", use_momentum=args.optimizer != "sgd", ema_max=0.9999,
                        clip_norm=args.clip_norm, **sched)
    from distributed_tensorflow_ibm_mnist_amd.data.mix import MixConfig
    mix = MixConfig(args.mixup_alpha, args.cutmix_alpha, args.mix_prob, args.seed if args.mix_seed is None else args.mix_seed)
    opt = dataclasses.replace(opt, label_smoothing=args.label_smoothing, dropout=args.dropout,
                              dropout_seed=args.seed + rank, mix=mix.enabled)
    init = init_params(spec, seed=args.seed)
    if args.impl == "hip":
        from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
        net = HipNet(spec, args.batch, dev, init, opt)
    else:
        from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import TorchNet
        net = TorchNet(spec, args.batch, dev, init, opt)
    dp = DataParallel(net)
    dp.broadcast_state()

    imgs, labs = make_synthetic(args.dataset_size, seed=args.seed, channels=args.in_channels, noise=args.noise,
                                device=dev, style=args.style)
    ds = DeviceDataset(imgs, labs, dev, hw=784, channels=args.in_channels)
    n_probe = min(args.probe, args.dataset_size)
    probe = DeviceDataset(imgs[:n_probe], labs[:n_probe], dev, hw=784, channels=args.in_channels)
    # --fused_input: the first fused conv reads the uint8 dataset through the batch index
    # (K10 fused).  Off by default: measured ~25 us/step slower on LeNet-5 at 65536 than
    # prep_images + bf16 (profiles/r1_u8_input/).
    from distributed_tensorflow_ibm_mnist_amd.data.augment import AugmentConfig
    aug = AugmentConfig(args.augment_shift, args.augment_rotate, args.augment_scale, args.seed,
                        args.augment_elastic_alpha, args.augment_elastic_sigma)
    # augmentation writes the input buffer itself: no fused gather of un-augmented rows
    # (and so does mixing)
    fused_in = (args.impl == "hip" and args.fused_input and not aug.enabled and not mix.enabled
                and net.bind_u8_input(ds.images))
    loader = DeviceLoader(ds, net.x0, net.labels, rank=rank, world=world, seed=args.seed,
                          idx_out=net.idx_buf if fused_in else None, augment=aug, mix=mix, out_labels2=net.labels2,
                          out_lam=net.mix_lam)

    graph = None
    if args.graph and args.impl == "hip" and world == 1 and dev.type == "cuda":
        from distributed_tensorflow_ibm_mnist_amd.runtime.graph import StepGraph
        loader.next()                               # StepGraph's warmup replays train on a real batch
        graph = StepGraph(dp.train_step)

    def probe_accuracy() -> float:
        st = net.eval_stats
        st.zero_()
        n = 0
        for nb in eval_batches(probe, net.x0, net.labels):
            net.eval_batch(nb, st)
            n += nb
        return float(st[1].item()) / max(n, 1)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)

    sync()
    t0 = time.perf_counter()
    start_step = int(net.fp.step.item())
    reached, acc, step = None, 0.0, start_step
    history = []
    while step - start_step < args.max_steps:
        loader.next()
        if graph is not None:
            graph.replay()
        else:
            dp.train_step()
        step += 1
        if (step - start_step) % args.eval_every == 0:
            acc = probe_accuracy()
            history.append((step, round(acc, 5)))
            if acc >= args.target:
                reached = step
                break
    sync()
    el = time.perf_counter() - t0
    global_batch = args.batch * world
    out = {
        "metric": f"steps-to-{args.target * 100:g}%-train-acc MNIST {LABEL[args.model]}",
        "value": reached,
        "unit": "steps",
        "higher_is_better": False,
        "n_gpus": world if dev.type == "cuda" else 0,
        "seconds": round(el, 3),
        "images_seen": (reached or step) * global_batch,
        "final_probe_accuracy": round(acc, 5),
        "dtype": "bf16" if dev.type == "cuda" else "fp32",
        "data": f"synthetic 28x28x{args.in_channels} (style {args.style}, noise {args.noise}), random-init weights; "
                f"probe = first {n_probe} training images",
        "config": {"model": LABEL[args.model], "global_batch": global_batch, "optimizer": args.optimizer,
                   "lr": args.lr, "lr_schedule": opt.schedule, "warmup_steps": opt.warmup_steps,
                   "lr_total_steps": opt.total_steps, "lr_end": opt.lr_end, "lr_power": opt.lr_power,
                   "label_smoothing": opt.label_smoothing, "dropout": opt.dropout,
                   "augment": [aug.shift, aug.rotate, aug.scale],
                   "augment_elastic": [aug.elastic_alpha, aug.elastic_sigma],
                   "mix": [mix.mixup_alpha, mix.cutmix_alpha, mix.prob],
                   "eval_every": args.eval_every, "impl": args.impl, "hip_graph": graph is not None,
                   "parallelism": f"dp{world}"},
        "history": history[-20:],
    }
    if world > 1:
        dist.destroy_process_group()
    return out if rank == 0 else {}


def main() -> int:
    out = run(parse())
    if out:
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
