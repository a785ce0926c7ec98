"""Learning-rate warmup with polynomial and cosine decay on the device (optimizer.hip sched_lr, the
*_sched_k optimizer kernels, lr_at_steps_k), on the GPU: the device's rate against the float64
oracle (tests/lr_schedule_oracle.py), every kernel family applying exactly that rate and following
the subclassed optimizer oracles across the warmup boundary, the defaults bit for bit, the
executors, hipGraph replay against eager (bitwise, with the rate moving under replay), the
binding's validation and the training CLI with a resume past the end of the decay.

Tolerances: the rate is measured as |lr - oracle| / lr0 and bounded by 4 times the worst such error
of the oracle module's numpy float32 transcription of the device function over the same inputs
(computed here, never from the kernel); tensors take the project's ``adaptive_oracle.close``
(max |out - ref| <= 1e-5 max |ref| + 1e-6)."""
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.runtime.params import FlatParams, OptConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lr_schedule_oracle",
                                               os.path.join(ROOT, "tests", "lr_schedule_oracle.py"))
oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(oracle)

pytestmark = pytest.mark.gpu

# the six-variable layout of test_adaptive_opt_gpu.py -- offsets 0 / 175 / 182 / 1502 / 1535 / 2195
SHAPES = [("a/weights", (5, 5, 1, 7), 0.0), ("a/biases", (7,), None), ("b/weights", (40, 33), 0.004),
          ("b/biases", (33,), None), ("c/weights", (33, 20), 0.002), ("c/biases", (20,), None)]
PADS = {"a/weights": (2, 8), "b/weights": (40, 40), "c/weights": (40, 24)}
WDS = {n: wd for n, _, wd in SHAPES}

KINDS = [("polynomial", 1.0), ("polynomial", 2.0), ("cosine", 1.0)]
SETS = [(0.05, 0.0, 3, 11), (0.05, 0.005, 0, 7), (0.5, 0.0, 500, 30000), (0.02, 0.0, 5, 2 ** 33)]


def np_of(t):
    return t.detach().cpu().numpy()


def sched_kw(sched):
    """The binding's keywords of an oracle schedule."""
    return {"lr_schedule": sched["kind"], "warmup_steps": sched["W"], "lr_total_steps": sched["T"],
            "lr_end": sched["lr_end"], "lr_power": sched["power"]}


def device_rate(K, dev, steps, lr0, sched, decay_rate=0.1, decay_steps=0):
    s = torch.as_tensor(np.asarray(steps, dtype=np.int64), device=dev)
    out = torch.full((s.numel(),), -1.0, dtype=torch.float32, device=dev)
    K.lr_at_steps(s, out, lr0, decay_rate, decay_steps, **sched_kw(sched))
    torch.cuda.synchronize()
    return np_of(out)


# ------------------------------------------------------------------ 1. the rate the device computes
def sweep(W, T):
    """0 .. T + 4 where T is small, else 20001 points over [0, T]; always T - 1, T, T + 1 and 2**40."""
    body = np.arange(0, T + 5, dtype=np.int64) if T <= 64 else \
        np.round(np.linspace(0.0, float(T), 20001)).astype(np.int64)
    edge = np.array([max(W - 1, 0), W, W + 1, T - 1, T, T + 1, 2 ** 40], dtype=np.int64)
    return np.unique(np.concatenate([body, edge]))


@functools.lru_cache(maxsize=None)
def reference(kind, power, lr0, lr_end, W, T):
    """(steps, float64 oracle, float32 transcription) of one case, computed once."""
    steps = sweep(W, T)
    sched = oracle.schedule(kind, W, T, lr_end, power)
    want = np.array([oracle.lr(int(t), lr0, **sched) for t in steps], dtype=np.float64)
    f32 = oracle.lr_f32(steps, lr0, **sched)
    return steps, want, f32


@functools.lru_cache(maxsize=None)
def transcription_worst():
    """The float32 transcription's worst |lr - oracle| / lr0 over every case of the test."""
    worst = 0.0
    for kind, power in KINDS:
        for lr0, lr_end, W, T in SETS:
            _, want, f32 = reference(kind, power, lr0, lr_end, W, T)
            worst = max(worst, float(np.abs(f32.astype(np.float64) - want).max() / lr0))
    return worst


@pytest.mark.parametrize("lr0,lr_end,W,T", SETS)
@pytest.mark.parametrize("kind,power", KINDS)
def test_lr_at_steps_matches_float64_oracle(dev, K, kind, power, lr0, lr_end, W, T):
    steps, want, f32 = reference(kind, power, lr0, lr_end, W, T)
    cpu_worst = transcription_worst()
    assert 0.0 < cpu_worst <= 1.5e-7, cpu_worst             # what single precision costs over these inputs
    sched = oracle.schedule(kind, W, T, lr_end, power)
    got = device_rate(K, dev, steps, lr0, sched)
    err = np.abs(got.astype(np.float64) - want) / lr0
    own = float(np.abs(f32.astype(np.float64) - want).max() / lr0)
    print(f"{kind} power {power} (lr0 {lr0}, lr_end {lr_end}, W {W}, T {T}): {len(steps)} steps, GPU worst "
          f"|lr - oracle| / lr0 = {err.max():.3e} at t = {int(steps[err.argmax()])}; float32 transcription "
          f"{own:.3e} here, {cpu_worst:.3e} over all cases; bound {4 * cpu_worst:.3e}")
    assert np.isfinite(got).all()
    assert err.max() <= 4 * cpu_worst, (err.max(), int(steps[err.argmax()]))
    late = steps >= T
    assert late.sum() >= 3 and (got[late].view(np.int32) == np.float32(lr_end).view(np.int32)).all()   # bitwise
    at = {int(t): g for t, g in zip(steps, got)}
    assert at[W] == np.float32(lr0) and (W == 0 or at[W - 1] == np.float32(lr0))   # no jump after the warmup
    if W > 1:
        assert at[0] < at[W - 1]


def apply_unit_gradient(dev, cfg, t):
    """p = 0, g = 1, grad_scale 1, plain SGD, EMA off, one apply at global step t: returns p."""
    fp = FlatParams.build(SHAPES, {n: torch.zeros(*s) for n, s, _ in SHAPES}, dev, pads=PADS)
    fp.init_slots(cfg)
    fp.grads.fill_(1.0)
    fp.step.fill_(t)
    fp.apply(cfg, grad_scale=1.0)
    torch.cuda.synchronize()
    return fp


def test_staircase_without_warmup_is_the_optimizers_own_rate_bitwise(dev, K):
    """lr_at_steps(staircase, W = 0) against what the unchanged launch (fused_opt_k) applies."""
    steps = [0, 1, 2, 3, 4, 7, 9, 2 ** 40]
    got = device_rate(K, dev, steps, 0.05, oracle.schedule(), decay_rate=0.5, decay_steps=2)
    cfg = OptConfig(lr0=0.05, decay_rate=0.5, decay_steps=2, ema_max=-1.0)
    for t, lr in zip(steps, got):
        p = np_of(apply_unit_gradient(dev, cfg, t).params)
        assert (p.view(np.int32) == (np.float32(0.0) - lr).view(np.int32)).all(), (t, lr, p[:4])     # 0 - lr * 1, bitwise
    assert got[0] == np.float32(0.05) and got[2] == np.float32(0.025) and got[-1] == 0.0
    flat = device_rate(K, dev, steps, 0.05, oracle.schedule(), decay_rate=0.5, decay_steps=0)
    assert (flat == np.float32(0.05)).all()


# ------------------------------------------------------------------ 2. the optimizer uses that rate
@pytest.mark.parametrize("kind,power,W", [("polynomial", 2.0, 3), ("cosine", 1.0, 3), ("staircase", 1.0, 4)])
def test_sgd_applies_exactly_the_rate_of_lr_at_steps(dev, K, kind, power, W):
    lr0, T = 0.05, 7 if kind != "staircase" else 0
    sched = oracle.schedule(kind, W, T, 0.1 * lr0 if kind != "staircase" else 0.0, power)
    decay = dict(decay_rate=0.5, decay_steps=2 if kind == "staircase" else 0)
    cfg = OptConfig(lr0=lr0, ema_max=-1.0, **decay, **oracle.opt_config_kwargs("sgd", sched))
    steps = sorted({0, W - 1, W, 5, 7, 8})                       # 0, W - 1, W, mid, T, T + 1
    rate = device_rate(K, dev, steps, lr0, sched, **decay)
    for t, lr in zip(steps, rate):
        want = oracle.lr(t, lr0, decay["decay_rate"], decay["decay_steps"], **sched)
        assert abs(float(lr) - want) <= 1e-6 * lr0, (t, lr, want)
        fp = apply_unit_gradient(dev, cfg, t)
        p = np_of(fp.params)
        assert (p.view(np.int32) == (np.float32(0.0) - lr).view(np.int32)).all(), (t, lr, p[:4])     # 0 - lr * 1, bitwise
        for n in PADS:                                             # the bf16 copies follow
            e = fp.by_name[n]
            assert torch.equal(fp.bf16_view(n)[..., :e.I, :e.J].reshape(-1),
                               fp.param_view(n).to(torch.bfloat16).reshape(-1)), n
    assert len(set(rate.tolist())) >= 4                            # the rate moves over these steps


LR0 = {"sgd": 0.05, "momentum": 0.05, "adam": 0.05, "rmsprop": 0.05, "adagrad": 0.05, "adam+clip": 0.05, "lars": 0.5,
       "lamb": 0.01}
ORACLE_KW = {"lars": {"eta": 0.02}}
CONFIG_KW = {"lars": {"lars_eta": 0.02}}
CASES = [(r, None) for r in oracle.RULES if r not in ("lars", "lamb")] + \
        [(r, h) for r in ("lars", "lamb") for h in (0, 1)]       # both hand-offs of the trust ratio


def check_state(fp, ref, rule, names):
    for n in names:
        s1, s2 = fp.slot_views(n)
        oracle.close(np_of(fp.param_view(n)), ref.p[n])
        oracle.close(np_of(fp.ema_view(n)), ref.ema[n])
        if rule != "sgd":
            oracle.close(np_of(s1), ref.s1[n])
        if rule in ("adam", "rmsprop", "adam+clip", "lamb"):
            oracle.close(np_of(s2), ref.s2[n])


@pytest.mark.parametrize("kind,power", [("polynomial", 2.0), ("cosine", 1.0)])
@pytest.mark.parametrize("rule,handoff", CASES)
def test_every_rule_follows_the_schedule_over_the_warmup_boundary(dev, K, rule, handoff, kind, power):
    lr0 = LR0[rule]
    sched = oracle.schedule(kind, 3, 7, 0.1 * lr0, power)
    prev = K.layerwise_self_sum_mode()
    if handoff is not None:
        K.set_layerwise_self_sum(handoff)
    try:
        torch.manual_seed(70)
        init = {n: torch.randn(*s) for n, s, _ in SHAPES}
        fp = FlatParams.build(SHAPES, init, dev, pads=PADS)
        fp.enable_transposed({"b/weights": (40, 48)})
        cfg = OptConfig(lr0=lr0, ema_max=0.9999, **oracle.opt_config_kwargs(rule, sched), **CONFIG_KW.get(rule, {}))
        fp.init_slots(cfg)
        ref = oracle.make(rule, {n: v.numpy() for n, v in init.items()}, WDS, lr0, 0.1, 0, 0.9999, sched,
                          grad_scale=0.5, **ORACLE_KW.get(rule, {}))
        rates = []
        for _ in range(8):
            g = {n: torch.randn_like(init[n]) for n in init}
            for n in g:
                fp.grad_view(n).copy_(g[n])
            rates.append(ref.lr())
            fp.apply(cfg, grad_scale=0.5)
            fp.step.add_(1)
            ref.step({n: v.numpy() for n, v in g.items()})
        torch.cuda.synchronize()
    finally:
        K.set_layerwise_self_sum(int(prev))
    assert rates[0] < rates[1] < rates[2] and rates[4] > rates[5] > rates[6] > rates[7] == 0.1 * lr0
    if rule == "adam+clip":
        assert any(ref.active), ref.scales                          # the clipping took part
    check_state(fp, ref, rule, list(init))
    for n in PADS:
        e = fp.by_name[n]
        c = fp.bf16_view(n)
        assert torch.equal(c[..., :e.I, :e.J], fp.param_view(n).to(torch.bfloat16).view(c.shape[:-2] + (e.I, e.J))), n
    assert torch.equal(fp.bf16t_view("b/weights")[:33, :40], fp.param_view("b/weights").to(torch.bfloat16).t())


# ------------------------------------------------------------------ 3. the defaults change nothing
@pytest.mark.parametrize("rule", ["momentum", "adam"])
def test_spelled_out_defaults_are_bitwise_the_old_launch(dev, K, rule):
    base = dict(lr0=0.05, decay_rate=0.5, decay_steps=2, ema_max=0.9999)
    base.update({"use_momentum": True, "momentum": 0.9} if rule == "momentum" else {"rule": "adam"})
    out = []
    for variant in ("omitted", "spelled", "positional"):
        cfg = OptConfig(**base) if variant != "spelled" else \
            OptConfig(schedule="staircase", warmup_steps=0, total_steps=0, lr_end=0.0, lr_power=1.0, **base)
        torch.manual_seed(71)
        init = {n: torch.randn(*s) for n, s, _ in SHAPES}
        fp = FlatParams.build(SHAPES, init, dev, pads=PADS)
        fp.init_slots(cfg)
        for _ in range(3):
            fp.grads.copy_(torch.randn(fp.total))
            if variant == "positional":      # the call as it was before the schedule's keywords existed
                extra = {} if rule == "momentum" else {"rule": "adam", "slot2": fp.slot2}
                K.fused_optimizer(fp.params, fp.grads, fp.mom, fp.ema, fp.bf16, fp.segs, fp.step, 0.05, 0.5, 2, 0.9,
                                  False, rule == "momentum", 0.5, 0.9999, fp.l2, **extra)
            else:
                fp.apply(cfg, grad_scale=0.5)
            fp.step.add_(1)
        torch.cuda.synchronize()
        out.append([t.clone() for t in (fp.params, fp.mom, fp.ema, fp.bf16, fp.l2)] +
                   ([fp.slot2.clone()] if rule == "adam" else []))
    for other in out[1:]:
        for a, b, name in zip(out[0], other, ("params", "slot 1", "ema", "bf16 copies", "l2", "slot 2")):
            assert torch.equal(a, b), name
    assert not torch.equal(out[0][0], torch.cat([init[n].reshape(-1) for n, _, _ in SHAPES]).to(dev))


# ------------------------------------------------------------------ 4. the executors
def _fill_batch(net, B, g, f32=False):
    x = torch.rand(B, 28, 28, 1, device=net.device, generator=g) - 0.5
    net.x0.copy_(x if f32 else x.to(torch.bfloat16))
    net.labels.copy_(torch.randint(0, 10, (B,), device=net.device, generator=g, dtype=torch.int32))


@pytest.mark.parametrize("rule,model,f32,kind", [("momentum", "lenet5", False, "cosine"),
                                                 ("adam", "mlp", True, "polynomial")])
def test_executor_update_follows_the_schedule(dev, K, rule, model, f32, kind):
    """Steps 0 and 1 inside the warmup (W = 2), step 2 at lr0, step 3 in the decay; the executor's own
    gradients go to the oracle, as in test_adaptive_opt_gpu.py."""
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor_f32 import HipNetF32
    B, lr0 = 128, 0.01
    spec = get_model(model, 1)
    sched = oracle.schedule(kind, 2, 5, 0.001, 2.0)
    cfg = OptConfig(lr0=lr0, ema_max=0.9999, **oracle.opt_config_kwargs(rule, sched))
    net = (HipNetF32 if f32 else HipNet)(spec, B, dev, torch_ref.init_params(spec, seed=3), cfg)
    fp = net.fp
    g = torch.Generator(device=dev).manual_seed(3)
    rates = []
    for _ in range(4):
        _fill_batch(net, B, g, f32)
        net.forward(defer_head=True)
        net.loss_and_grad()
        net.backward()
        torch.cuda.synchronize()
        step = int(fp.step.item())
        names = fp.names()
        ref = oracle.make(rule, {n: np_of(fp.param_view(n)) for n in names}, {e.name: e.wd for e in fp.entries}, lr0,
                          0.1, 0, 0.9999, sched, step0=step)
        for n in names:
            s1, s2 = fp.slot_views(n)
            ref.s1[n] = np_of(s1).astype(np.float64)
            if rule == "adam":
                ref.s2[n] = np_of(s2).astype(np.float64)
            ref.ema[n] = np_of(fp.ema_view(n)).astype(np.float64)
        grads = {n: np_of(fp.grad_view(n)).copy() for n in names}
        rates.append(ref.lr())
        net.update()
        torch.cuda.synchronize()
        ref.step(grads)
        check_state(fp, ref, rule, names)
        assert int(fp.step.item()) == step + 1
    # the oracle's lr_end + (lr0 - lr_end) * 1 is lr0 to an ulp of float64
    assert abs(rates[0] - lr0 / 2) < 1e-15 and abs(rates[1] - lr0) < 1e-15 and abs(rates[2] - lr0) < 1e-15
    assert 0.001 < rates[3] < 0.9 * lr0
    assert net.read_stats()["nan"] == 0.0


# ------------------------------------------------------------------ 5. hipGraph replay
def test_graph_replay_equals_eager_bitwise_and_the_rate_moves(dev, K):
    """W = 2, T = 5, 6 momentum steps: step 0 is the eager warm-up of the capture, steps 1 .. 5 are
    replays of one captured launch, across the end of the warmup and the end of the decay.  The
    rate a replayed step applied is rebuilt from the state around it -- p' = p - lr v', v' the new
    momentum -- as the least-squares lr = <p - p', v'> / <v', v'> in float64.  Rounding p' to fp32
    (|p| <= 1: 6e-8) against |lr v'| leaves that estimate far inside 1e-3 lr0, and the schedule's
    consecutive rates differ by 0.25 lr0 or more."""
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
    from distributed_tensorflow_ibm_mnist_amd.runtime.graph import StepGraph
    B, steps, lr0 = 128, 6, 0.02
    spec = get_model("lenet5", 1)
    sched = oracle.schedule("cosine", 2, 5, 0.0)
    g = torch.Generator(device=dev).manual_seed(8)
    xs = [(torch.rand(B, 28, 28, 1, device=dev, generator=g) - 0.5).to(torch.bfloat16) for _ in range(steps)]
    ys = [torch.randint(0, 10, (B,), device=dev, generator=g, dtype=torch.int32) for _ in range(steps)]
    rate = device_rate(K, dev, list(range(steps)), lr0, sched)
    assert rate.tolist() == [np.float32(lr0 / 2), np.float32(lr0), np.float32(lr0), rate[3], rate[4], 0.0]
    assert abs(rate[3] - 0.75 * lr0) < 1e-6 * lr0 and abs(rate[4] - 0.25 * lr0) < 1e-6 * lr0
    out, seen = [], []
    for graph in (False, True):
        net = HipNet(spec, B, dev, torch_ref.init_params(spec, seed=8),
                     OptConfig(lr0=lr0, ema_max=0.9999, **oracle.opt_config_kwargs("momentum", sched)))
        sg = None
        for k in range(steps):
            net.x0.copy_(xs[k])
            net.labels.copy_(ys[k])
            if not graph:
                net.train_step()
            elif sg is None:
                sg = StepGraph(net.train_step, warmup=1)    # the warm-up is step 0; capture executes nothing
            else:
                torch.cuda.synchronize()
                p0 = net.fp.params.double().clone()
                sg.replay()
                torch.cuda.synchronize()
                v1 = net.fp.mom.double()
                seen.append(float(((p0 - net.fp.params.double()) * v1).sum() / (v1 * v1).sum()))
        torch.cuda.synchronize()
        assert int(net.fp.step.item()) == steps
        out.append([t.clone() for t in (net.fp.params, net.fp.mom, net.fp.ema, net.stats)])
    for a, b, name in zip(out[0], out[1], ("params", "momentum", "ema", "stats")):
        assert torch.equal(a, b), name
    print("rates rebuilt from the replayed steps 1 .. 5:", seen, "device:", rate[1:].tolist())
    assert len(seen) == 5
    for k, est in enumerate(seen, start=1):
        assert abs(est - float(rate[k])) <= 1e-3 * lr0, (k, est, float(rate[k]))


# ------------------------------------------------------------------ 6. the binding validates
def test_binding_validates_the_schedule(dev, K):
    torch.manual_seed(72)
    init = {n: torch.randn(*s) for n, s, _ in SHAPES}
    fp = FlatParams.build(SHAPES, init, dev, pads=PADS)
    fp.grads.copy_(torch.randn(fp.total))
    args = (fp.params, fp.grads, fp.mom, fp.ema, fp.bf16, fp.segs, fp.step, 0.1, 0.1, 0, 0.9, False, True, 1.0,
            0.9999)
    ok = {"lr_schedule": "cosine", "warmup_steps": 2, "lr_total_steps": 9}
    with pytest.raises(RuntimeError, match="unknown lr_schedule 'linear'"):
        K.fused_optimizer(*args, lr_schedule="linear")
    for T in (2, 1, 0, -5):
        with pytest.raises(RuntimeError, match="lr_total_steps"):
            K.fused_optimizer(*args, **dict(ok, lr_total_steps=T))
    with pytest.raises(RuntimeError, match="lr_total_steps"):
        K.fused_optimizer(*args, lr_schedule="polynomial")                    # T defaults to 0
    with pytest.raises(RuntimeError, match="warmup_steps"):
        K.fused_optimizer(*args, warmup_steps=-1)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="lr_power"):
            K.fused_optimizer(*args, lr_power=bad, **dict(ok, lr_schedule="polynomial"))
    for bad in (-1e-3, float("inf"), float("-inf"), float("nan")):
        with pytest.raises(RuntimeError, match="lr_end"):
            K.fused_optimizer(*args, lr_end=bad, **ok)
    guard = torch.zeros(1, dtype=torch.int64, device=dev)
    guard_err = torch.zeros(1, dtype=torch.int32, device=dev)
    for kw in (ok, {"warmup_steps": 3}, {"lr_schedule": "polynomial", "lr_total_steps": 4}):
        with pytest.raises(RuntimeError, match="push guard"):
            K.fused_optimizer(*args, None, guard, 0, guard_err, 0, **kw)
    steps = torch.arange(4, device=dev)
    out = torch.zeros(4, device=dev)
    with pytest.raises(RuntimeError, match="unknown lr_schedule"):
        K.lr_at_steps(steps, out, 0.1, 0.1, 0, lr_schedule="exp")
    with pytest.raises(RuntimeError, match="lr_total_steps"):
        K.lr_at_steps(steps, out, 0.1, 0.1, 0, lr_schedule="cosine", warmup_steps=3, lr_total_steps=3)
    with pytest.raises(RuntimeError, match="out"):
        K.lr_at_steps(steps, out[:3], 0.1, 0.1, 0)
    with pytest.raises(RuntimeError, match="steps"):
        K.lr_at_steps(steps.int(), out, 0.1, 0.1, 0)
    with pytest.raises(RuntimeError, match="steps"):
        K.lr_at_steps(steps.cpu(), out, 0.1, 0.1, 0)
    with pytest.raises(ValueError, match="total_steps"):
        fp.apply(OptConfig(schedule="cosine", warmup_steps=4, total_steps=4))
    torch.cuda.synchronize()
    assert torch.equal(fp.params.cpu(), torch.cat([init[n].reshape(-1) for n, _, _ in SHAPES]))   # nothing ran
    assert fp.mom.abs().sum().item() == 0 and out.abs().sum().item() == 0 and int(guard_err.item()) == 0
    assert int(fp.step.item()) == 0
    K.fused_optimizer(*args, lr_schedule="COSINE", warmup_steps=2, lr_total_steps=9)     # case-insensitive; runs
    torch.cuda.synchronize()
    assert not torch.equal(fp.params.cpu(), torch.cat([init[n].reshape(-1) for n, _, _ in SHAPES]))


# ------------------------------------------------------------------ 7. the training CLI
def _learning_rates(d):
    from distributed_tensorflow_ibm_mnist_amd.obs.events import find_event_files, read_events
    out = {}
    for f in find_event_files(d):
        for ev in read_events(f):
            if "learning_rate" in ev["values"]:
                out[ev["step"]] = ev["values"]["learning_rate"]
    return out


def test_cli_lars_with_warmup_and_polynomial_decay_trains_and_resumes(tmp_path, dev):
    d = str(tmp_path / "lars_warmup")
    args = ["--model=lenet5", "--in_channels=1", "--optimizer=lars", "--base_lr=0.2", "--lars_eta=0.02",
            "--lr_schedule=polynomial", "--lr_power=2", "--warmup_steps=10", "--lr_end=0.002", "--batch_size=128",
            "--test_interval=1000", "--log_step_count_steps=0", "--save_summaries_steps=1",
            "--train_data=synthetic://4000", "--test_data=synthetic://512?seed=1", "--eval_examples=256",
            f"--train_dir={d}"]

    def run(extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args + extra, cwd=ROOT,
                           capture_output=True, text=True, timeout=180, env=dict(os.environ, PYTHONUNBUFFERED="1"))
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

    run(["--max_steps=40"])                                          # lr_total_steps: max_steps
    from distributed_tensorflow_ibm_mnist_amd.ckpt.saver import Saver
    t = Saver.restore(os.path.join(d, "model.ckpt-40"))
    assert int(t["global_step"]) == 40 and "conv1/weights/Momentum" in t
    assert not any(w in k.lower() for k in t for w in ("warmup", "schedule", "learning_rate")), sorted(t)   # no new state
    cfg = OptConfig(lr0=0.2, rule="lars", schedule="polynomial", lr_power=2.0, warmup_steps=10, total_steps=40,
                    lr_end=0.002)
    lr = _learning_rates(d)
    assert sorted(lr) == list(range(1, 41))
    for step, v in lr.items():
        assert np.float32(v) == np.float32(cfg.lr_at(step)), (step, v, cfg.lr_at(step))
    assert lr[1] < lr[5] < lr[9] and np.float32(lr[9]) == np.float32(lr[10]) == np.float32(0.2)
    assert lr[11] > lr[25] > lr[39] > lr[40] and np.float32(lr[40]) == np.float32(0.002)
    run(["--max_steps=60", "--lr_total_steps=40"])                   # resumed past the end of the decay
    lr = _learning_rates(d)
    assert sorted(lr) == list(range(1, 61))
    assert all(np.float32(lr[s]) == np.float32(0.002) for s in range(40, 61)), {s: lr[s] for s in range(38, 61)}
    u = Saver.restore(os.path.join(d, "model.ckpt-60"))
    assert int(u["global_step"]) == 60 and sorted(u) == sorted(t)
    assert all(np.isfinite(np.asarray(v)).all() for v in u.values())
    assert not np.array_equal(np.asarray(t["conv1/weights"]), np.asarray(u["conv1/weights"]))   # lr_end > 0: it trains on
