#!/usr/bin/env python3
"""Time the fused optimizer launch alone, per update rule, on the reference CNN's parameters
(3.46 M, with the bf16 / W^T copies the executor keeps): 200 launches between two device events
after a warm-up, one settled run per rule, rules interleaved over a few rounds in one process.

The launch is memory-bound.  Per element it reads params, grads, EMA and the rule's slots and
writes params, EMA, the slots and (weights) a bf16 copy:

    momentum          4 reads + 3 writes of 4 B + 2 B bf16 = 30 B
    adam / rmsprop    5 reads + 4 writes of 4 B + 2 B bf16 = 38 B     (expected 38 / 30 = 1.27 x momentum)
    adagrad           as momentum: one slot                = 30 B
    sgd               3 reads + 2 writes of 4 B + 2 B bf16 = 22 B

--clip_norm C times every rule a second time with clipping by global norm ("<rule>+clip": the
reduction launch, 8 B per element read, then the clipped optimizer launch), interleaved with the
plain launches; C is large by default so the updates themselves stay the same.

--rules also takes lars and lamb (the per-variable norm launch, 8 / 16 B per element read, the ratio
hand-off chosen by --handoff, then the optimizer launch).

    python bench/micro_opt.py [--launches 200] [--rounds 5] [--model reference_cnn] [--clip_norm 1e30]
                              [--rules momentum,lars,adam,lamb] [--handoff self|launch]
prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# lars / lamb: the per-variable norm launch reads params and grads (8 B), lamb's also both slots
# (16 B), in front of momentum's / adam's traffic
BYTES = {"sgd": 22, "momentum": 30, "adam": 38, "rmsprop": 38, "adagrad": 30, "lars": 38, "lamb": 54}
LAYERWISE = ("lars", "lamb")   # never timed with clip_norm (the combination is refused)
CLIP_BYTES = 8   # the reduction reads params and grads once more


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="reference_cnn")
    ap.add_argument("--in_channels", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rules", default="momentum,adam,rmsprop,adagrad")
    ap.add_argument("--clip_norm", type=float, default=None, help="also time each rule with this clip_norm")
    ap.add_argument("--lars_eta", type=float, default=0.001, help="lars: trust coefficient")
    ap.add_argument("--handoff", choices=["self", "launch"], default=None,
                    help="lars / lamb: every apply block sums its variable's partials itself, or a third one-block-"
                         "per-variable launch does (default: by the model's size)")
    ap.add_argument("--lr_schedule", default="staircase", choices=["staircase", "polynomial", "cosine"])
    ap.add_argument("--warmup_steps", type=int, default=0)
    ap.add_argument("--lr_total_steps", type=int, default=10000, help="polynomial / cosine")
    ap.add_argument("--lr_end", type=float, default=0.0)
    ap.add_argument("--lr_power", type=float, default=1.0)
    args = ap.parse_args()
    # a schedule or a warmup: every rule is timed a second time with it ("<rule>+sched"), at a global
    # step inside the decay, interleaved with the plain launches
    sched = {}
    if args.lr_schedule != "staircase" or args.warmup_steps > 0:
        sched = dict(schedule=args.lr_schedule, warmup_steps=args.warmup_steps, lr_end=args.lr_end,
                     lr_power=args.lr_power, total_steps=args.lr_total_steps if args.lr_schedule != "staircase" else 0)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("micro_opt.py times a GPU launch: no HIP device")   # no CPU fall-back: it would say nothing
    from distributed_tensorflow_ibm_mnist_amd.models import get_model
    from distributed_tensorflow_ibm_mnist_amd.models.torch_ref import init_params
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig

    dev = torch.device("cuda", 0)
    spec = get_model(args.model, args.in_channels)
    init = init_params(spec, seed=0)
    base_rules = [r for r in args.rules.split(",") if r]
    rules = base_rules + ([r + "+clip" for r in base_rules if r not in LAYERWISE] if args.clip_norm else [])
    rules += [r + "+sched" for r in base_rules] if sched else []
    if args.handoff:
        from distributed_tensorflow_ibm_mnist_amd.ops._ext import kernels
        kernels().set_layerwise_self_sum(int(args.handoff == "self"))
    nets = {}
    for key in rules:
        r, clip = key.split("+")[0], (args.clip_norm if key.endswith("+clip") else None)
        sk = sched if key.endswith("+sched") else {}
        if r in ("adam", "rmsprop", "adagrad", "lamb"):
            cfg = OptConfig(lr0=1e-3, ema_max=0.9999, rule=r, clip_norm=clip, **sk)
        elif r == "lars":
            cfg = OptConfig(lr0=1e-3, ema_max=0.9999, rule=r, momentum=0.9, lars_eta=args.lars_eta, **sk)
        else:
            cfg = OptConfig(lr0=1e-3, ema_max=0.9999, momentum=0.9 if r != "sgd" else 0.0, use_momentum=r != "sgd",
                            clip_norm=clip, **sk)
        net = HipNet(spec, 16, dev, init, cfg)      # the executor's own FlatParams layout (pads, W^T copies)
        if sk:
            net.fp.step.fill_(cfg.warmup_steps + max(1, (cfg.total_steps - cfg.warmup_steps) // 3))
        net.fp.grads.copy_(torch.randn(net.fp.total, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
                           * 1e-2)
        nets[key] = net
    n = nets[rules[0]].fp.total
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {r: [] for r in rules}
    for rnd in range(args.rounds):
        for r in rules:
            fp, cfg = nets[r].fp, nets[r].opt
            for _ in range(args.warmup):
                fp.apply(cfg)
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(args.launches):
                fp.apply(cfg)
            ev1.record()
            torch.cuda.synchronize()
            times[r].append(ev0.elapsed_time(ev1) * 1e3 / args.launches)     # us per launch
    for r in rules:
        assert torch.isfinite(nets[r].fp.params).all(), r
    out = {"metric": "fused optimizer launch, us (device events, back-to-back launches)", "model": args.model,
           "parameters": n, "launches": args.launches, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "rules": {}}
    for r in rules:
        med = statistics.median(times[r])
        nbytes = BYTES[r.split("+")[0]] + (CLIP_BYTES if r.endswith("+clip") else 0)
        out["rules"][r] = {"us_median": round(med, 2), "us_min": round(min(times[r]), 2),
                           "us_all": [round(t, 2) for t in times[r]], "bytes_per_element": nbytes,
                           "GBps": round(n * nbytes / med / 1e3, 1)}
    if "momentum" in out["rules"]:
        base = out["rules"]["momentum"]["us_median"]
        for r in rules:
            out["rules"][r]["ratio_to_momentum"] = round(out["rules"][r]["us_median"] / base, 3)
            out["rules"][r]["expected_ratio"] = round(out["rules"][r]["bytes_per_element"] / BYTES["momentum"], 3)
    if any(r in LAYERWISE for r in base_rules):
        from distributed_tensorflow_ibm_mnist_amd.ops._ext import kernels
        out["layerwise_handoff"] = {-1: "by size", 0: "launch", 1: "self"}[int(kernels().layerwise_self_sum_mode())]
        for r, plain in (("lars", "momentum"), ("lamb", "adam")):   # the norm pass's cost next to its byte ratio
            if r in out["rules"] and plain in out["rules"]:
                out["rules"][r]["ratio_to_" + plain] = round(out["rules"][r]["us_median"] /
                                                              out["rules"][plain]["us_median"], 3)
                out["rules"][r]["expected_ratio_to_" + plain] = round(BYTES[r] / BYTES[plain], 3)
    if args.clip_norm:
        from distributed_tensorflow_ibm_mnist_amd.ops._ext import kernels
        out["clip_norm"] = args.clip_norm
        out["grad_norm_blocks"] = int(kernels().grad_norm_max_blocks())
        for r in (r for r in base_rules if r not in LAYERWISE):   # clipped (two launches) over plain (one)
            c, p = out["rules"][r + "+clip"], out["rules"][r]
            c["ratio_to_unclipped"] = round(c["us_median"] / p["us_median"], 3)
            c["expected_ratio_to_unclipped"] = round(c["bytes_per_element"] / p["bytes_per_element"], 3)
    if sched:
        out["lr_schedule"] = sched
        for r in base_rules:   # the scheduled launch (the *_sched_k kernel) over the plain one
            out["rules"][r + "+sched"]["ratio_to_unscheduled"] = round(out["rules"][r + "+sched"]["us_median"] /
                                                                       out["rules"][r]["us_median"], 3)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
