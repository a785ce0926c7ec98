"""Gradient clipping by global norm in the fused optimizer step (optimizer.hip grad_sqnorm_k +
clipped_opt_k), on the GPU: the reduction against float64, the clipped update of every rule against
the float64 oracle (tests/clip_oracle.py) on a layout that hits every access path, the exact
identity at a huge threshold, the binding's validation, the executors' wiring, hipGraph replay
against eager (bitwise) and a non-finite gradient."""
import importlib.util
import os
import struct

import numpy as np
import pytest
import torch

from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.runtime.params import FlatParams, OptConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("clip_oracle", os.path.join(ROOT, "tests", "clip_oracle.py"))
oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(oracle)

pytestmark = pytest.mark.gpu

# the layout of test_adaptive_opt_gpu.py -- offsets 0 / 175 / 182 / 1502 / 1535 / 2195: odd offsets
# (scalar path), odd counts (scalar tails), 8-byte pairs, segments of more than one 512-element chunk
SHAPES = [("a/weights", (5, 5, 1, 7), 0.0), ("a/biases", (7,), None), ("b/weights", (40, 33), 0.004),
          ("b/biases", (33,), None), ("c/weights", (33, 20), 0.002), ("c/biases", (20,), None)]
PADS = {"a/weights": (2, 8), "b/weights": (40, 40), "c/weights": (40, 24)}
ZERO_GRAD = "b/biases"
WDS = {n: wd for n, _, wd in SHAPES}
CLIP = 5.0
# randn over 2182 elements * grad_scale 0.5 has norm ~23 at amplitude 1: clipping at 5 is active at
# amplitudes 1 and 2, inactive at 0.1 and 0.05
AMPL = [1.0, 0.1, 2.0, 0.05, 1.0]


def np_of(t):
    return t.detach().cpu().numpy()


def build(dev, seed, transposed=True):
    torch.manual_seed(seed)
    init = {n: torch.randn(*s) for n, s, _ in SHAPES}
    fp = FlatParams.build(SHAPES, init, dev, pads=PADS)
    if transposed:
        fp.enable_transposed({"b/weights": (40, 48)})
    return init, fp


def ref_norm(params, grads, wds, grad_scale):
    """float64 sqrt(sum (g * grad_scale + wd * p)^2) over flat arrays."""
    g = grads.astype(np.float64) * grad_scale + wds.astype(np.float64) * params.astype(np.float64)
    return float(np.sqrt((g * g).sum()))


# ------------------------------------------------------------------ 1. the reduction alone
def test_grad_global_norm_six_tensor_layout(dev, K):
    init, fp = build(dev, 40, transposed=False)
    assert [int(r[0]) for r in fp.segs.tolist()] == [0, 175, 182, 1502, 1535, 2195]
    fp.grads.copy_(torch.randn(fp.total))
    gnorm = torch.full((2 + K.grad_norm_max_blocks(),), 7.0, device=dev)     # stale partials must not survive
    K.grad_global_norm(fp.params, fp.grads, fp.segs, 0.5, gnorm)
    first = gnorm[0].clone()
    wd = np.concatenate([np.full(e.n, e.wd or 0.0) for e in fp.entries])
    want = ref_norm(np_of(fp.params), np_of(fp.grads), wd, 0.5)
    got = float(first)
    print(f"six-tensor layout: global_norm {got:.7g}, float64 {want:.7g}, rel err {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-5 * want
    assert float(gnorm[1]) == 7.0                                             # the scale slot is the update's
    K.grad_global_norm(fp.params, fp.grads, fp.segs, 0.5, gnorm)
    assert torch.equal(gnorm[0], first)                                       # bitwise repeatable


def test_grad_global_norm_every_block_walks_several_chunks(dev, K):
    """One weight of 2 * 512 * grad_norm_max_blocks() + 777 elements: each block of the reduction
    walks several chunks and the last block's range is ragged (and ends in a partial chunk)."""
    nb = int(K.grad_norm_max_blocks())
    assert 1 <= nb <= 1024
    n = 2 * 512 * nb + 777
    wd = 0.003
    wd_bits = struct.unpack("<i", struct.pack("<f", wd))[0]
    segs = torch.tensor([[0, n, 1, 1, n, 1, n, -1, wd_bits, 0, -1, 0, 0, 0]], dtype=torch.int64)
    g = torch.Generator(device=dev).manual_seed(41)
    p = torch.randn(n, device=dev, generator=g)
    gr = torch.randn(n, device=dev, generator=g)
    gnorm = torch.zeros(2 + nb, device=dev)
    K.grad_global_norm(p, gr, segs, 0.5, gnorm)
    first = gnorm[0].clone()
    want = ref_norm(np_of(p), np_of(gr), np.full(n, np.float64(np.float32(wd))), 0.5)
    got = float(first)
    print(f"{n} elements, {nb} blocks: global_norm {got:.7g}, float64 {want:.7g}, rel err {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-5 * want
    # 3 chunks per block: the last used block is ragged and the blocks after it store 0
    used = -(-(2 * nb + 2) // 3)
    part = np_of(gnorm[2:])
    assert (part[:used] > 0).all() and (part[used:] == 0).all()
    K.grad_global_norm(p, gr, segs, 0.5, gnorm)
    assert torch.equal(gnorm[0], first)


# ------------------------------------------------------------------ 2. fp.apply against the oracle
def check_state(fp, ref, rule, names):
    for n in names:
        s1, s2 = fp.slot_views(n)
        oracle.close(np_of(fp.param_view(n)), ref.p[n])
        oracle.close(np_of(fp.ema_view(n)), ref.ema[n])
        if rule != "sgd":
            oracle.close(np_of(s1), ref.s1[n])
        if rule in ("adam", "rmsprop"):
            oracle.close(np_of(s2), ref.s2[n])


@pytest.mark.parametrize("rule", oracle.RULES)
def test_clipped_update_matches_float64_oracle(dev, K, rule):
    init, fp = build(dev, 42)
    cfg = OptConfig(lr0=0.05, decay_rate=0.5, decay_steps=2, ema_max=0.9999, clip_norm=CLIP,
                    **oracle.opt_config_kwargs(rule))
    fp.init_slots(cfg)
    assert fp.gnorm is not None and fp.gnorm.numel() == 2 + K.grad_norm_max_blocks()
    ref = oracle.ClipOracle(rule, {n: v.numpy() for n, v in init.items()}, WDS, 0.05, 0.5, 2, 0.9999, CLIP,
                            grad_scale=0.5)
    for k in range(5):
        g = {n: torch.randn_like(init[n]) * AMPL[k] for n in init}
        g[ZERO_GRAD].zero_()
        for n in g:
            fp.grad_view(n).copy_(g[n])
        fp.apply(cfg, grad_scale=0.5)
        fp.step.add_(1)
        ref.step({n: v.numpy() for n, v in g.items()})
        gn, s = fp.gnorm[:2].tolist()
        print(f"{rule} step {k}: global_norm {gn:.7g} (float64 {ref.norms[-1]:.7g}), s {s:.7g} ({ref.scales[-1]:.7g})")
        assert abs(gn - ref.norms[-1]) <= 1e-5 * ref.norms[-1]
        assert abs(s - ref.scales[-1]) <= 1e-5
        assert (s == 1.0) == (not ref.active[-1])          # at or below the threshold: exactly 1
    assert ref.active == [True, False, True, False, True]   # both branches ran
    check_state(fp, ref, rule, list(init))
    # bf16 copies: bf16(params) in the valid region, zero in the padding
    for n in PADS:
        e = fp.by_name[n]
        c = fp.bf16_view(n)
        want = fp.param_view(n).to(torch.bfloat16)
        assert torch.equal(c[..., :e.I, :e.J], want.view(c.shape[:-2] + (e.I, e.J))), n
        assert c[..., e.I:, :].float().abs().sum().item() == 0 and c[..., :, e.J:].float().abs().sum().item() == 0, n
    t = fp.bf16t_view("b/weights")
    assert torch.equal(t[:33, :40], fp.param_view("b/weights").to(torch.bfloat16).t())
    assert t[33:].float().abs().sum().item() == 0 and t[:, 40:].float().abs().sum().item() == 0


# ------------------------------------------------------------------ 3. a huge threshold changes no bit
@pytest.mark.parametrize("rule", oracle.RULES)
def test_huge_clip_norm_is_bitwise_no_clipping(dev, K, rule):
    out = []
    for clip in (None, 1e30):
        init, fp = build(dev, 43)
        cfg = OptConfig(lr0=0.05, decay_rate=0.5, decay_steps=2, ema_max=0.9999, clip_norm=clip,
                        **oracle.opt_config_kwargs(rule))
        fp.init_slots(cfg)
        torch.manual_seed(44)
        for _ in range(3):
            fp.grads.copy_(torch.randn(fp.total))
            fp.apply(cfg, grad_scale=0.5)
            fp.step.add_(1)
        torch.cuda.synchronize()
        out.append([t.clone() for t in (fp.params, fp.mom, fp.ema, fp.bf16)] +
                   ([fp.slot2.clone()] if rule in ("adam", "rmsprop") else []))
        if clip:
            assert float(fp.gnorm[1]) == 1.0 and float(fp.gnorm[0]) > 0
    for a, b, name in zip(out[0], out[1], ("params", "slot 1", "ema", "bf16 copies", "slot 2")):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------ 4. the binding validates
def test_binding_validates_clip_arguments(dev, K):
    init, fp = build(dev, 45, transposed=False)
    fp.grads.copy_(torch.randn(fp.total))
    args = (fp.params, fp.grads, fp.mom, fp.ema, fp.bf16, fp.segs, fp.step, 0.1, 0.1, 0, 0.0, False, False, 1.0,
            0.9999)
    gnorm = torch.zeros(2 + K.grad_norm_max_blocks(), device=dev)
    with pytest.raises(RuntimeError, match="needs gnorm"):
        K.fused_optimizer(*args, clip_norm=1.0)
    with pytest.raises(RuntimeError, match="gnorm"):
        K.fused_optimizer(*args, clip_norm=1.0, gnorm=gnorm[:-1])
    with pytest.raises(RuntimeError, match="gnorm"):
        K.fused_optimizer(*args, clip_norm=1.0, gnorm=gnorm.cpu())
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="clip_norm"):
            K.fused_optimizer(*args, clip_norm=bad, gnorm=gnorm)
    guard = torch.zeros(1, dtype=torch.int64, device=dev)
    guard_err = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="push guard"):
        K.fused_optimizer(*args, None, guard, 0, guard_err, 0, clip_norm=1.0, gnorm=gnorm)
    with pytest.raises(RuntimeError, match="init_slots"):
        fp.apply(OptConfig(clip_norm=1.0))
    with pytest.raises(RuntimeError, match="gnorm"):
        K.grad_global_norm(fp.params, fp.grads, fp.segs, 1.0, gnorm[:-1])
    torch.cuda.synchronize()
    assert torch.equal(fp.params.cpu(), torch.cat([init[n].reshape(-1) for n, _, _ in SHAPES]))   # nothing ran
    assert int(guard_err.item()) == 0 and gnorm.abs().sum().item() == 0


# ------------------------------------------------------------------ 5. the executors
def _fill_batch(net, B, g, f32=False):
    x = torch.rand(B, 28, 28, 1, device=net.device, generator=g) - 0.5
    net.x0.copy_(x if f32 else x.to(torch.bfloat16))
    net.labels.copy_(torch.randint(0, 10, (B,), device=net.device, generator=g, dtype=torch.int32))


@pytest.mark.parametrize("rule,model,f32", [("adam", "lenet5", False), ("momentum", "mlp", True)])
def test_executor_clipped_update_matches_oracle(dev, K, rule, model, f32):
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor_f32 import HipNetF32
    B = 128
    spec = get_model(model, 1)
    cfg = OptConfig(lr0=0.01, decay_rate=0.1, decay_steps=0, ema_max=0.9999, clip_norm=1.0,
                    **oracle.opt_config_kwargs(rule))
    net = (HipNetF32 if f32 else HipNet)(spec, B, dev, torch_ref.init_params(spec, seed=3), cfg)
    fp = net.fp
    names = fp.names()
    wds = {e.name: e.wd for e in fp.entries}
    g = torch.Generator(device=dev).manual_seed(3)
    for k in range(2):
        _fill_batch(net, B, g, f32)
        net.forward(defer_head=True)
        net.loss_and_grad()
        net.backward()
        torch.cuda.synchronize()
        step = int(fp.step.item())
        params = {n: np_of(fp.param_view(n)) for n in names}
        grads = {n: np_of(fp.grad_view(n)).copy() for n in names}
        if k == 0:
            # half of the first step's float64 norm: clipping is certainly active
            probe = oracle.ClipOracle(rule, params, wds, 0.01, 0.1, 0, 0.9999, None)
            probe.step(grads)
            net.opt.clip_norm = 0.5 * probe.norms[0]
        ref = oracle.ClipOracle(rule, params, wds, 0.01, 0.1, 0, 0.9999, net.opt.clip_norm, step0=step)
        for n in names:
            s1, s2 = fp.slot_views(n)
            ref.s1[n] = np_of(s1).astype(np.float64)
            if s2 is not None:
                ref.s2[n] = np_of(s2).astype(np.float64)
            ref.ema[n] = np_of(fp.ema_view(n)).astype(np.float64)
        net.update()
        torch.cuda.synchronize()
        ref.step(grads)
        check_state(fp, ref, rule, names)
        st = net.read_stats()
        print(f"{model} step {k}: global_norm {st['global_norm']:.7g} (float64 {ref.norms[0]:.7g}), "
              f"s {st['clip_scale']:.7g} ({ref.scales[0]:.7g})")
        assert abs(st["global_norm"] - ref.norms[0]) <= 1e-5 * ref.norms[0]
        assert abs(st["clip_scale"] - ref.scales[0]) <= 1e-5
        assert int(fp.step.item()) == step + 1
        if k == 0:
            assert ref.active[0] and st["clip_scale"] < 0.51
    assert net.read_stats()["nan"] == 0.0


# ------------------------------------------------------------------ 6. hipGraph replay
def test_graph_replay_equals_eager_bitwise(dev, K):
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
    from distributed_tensorflow_ibm_mnist_amd.runtime.graph import StepGraph
    B, steps = 128, 4
    spec = get_model("lenet5", 1)
    g = torch.Generator(device=dev).manual_seed(8)
    xs = [(torch.rand(B, 28, 28, 1, device=dev, generator=g) - 0.5).to(torch.bfloat16) for _ in range(steps)]
    ys = [torch.randint(0, 10, (B,), device=dev, generator=g, dtype=torch.int32) for _ in range(steps)]
    out = []
    for graph in (False, True):
        net = HipNet(spec, B, dev, torch_ref.init_params(spec, seed=8),
                     OptConfig(lr0=0.002, ema_max=0.9999, rule="adam", clip_norm=0.01))
        sg = None
        for k in range(steps):
            net.x0.copy_(xs[k])
            net.labels.copy_(ys[k])
            if not graph:
                net.train_step()
            elif sg is None:
                sg = StepGraph(net.train_step, warmup=1)    # the warm-up is step 0; capture executes nothing
            else:
                sg.replay()
        torch.cuda.synchronize()
        assert int(net.fp.step.item()) == steps
        out.append([t.clone() for t in (net.fp.params, net.fp.mom, net.fp.slot2, net.fp.ema, net.fp.gnorm[:2])])
    for a, b, name in zip(out[0], out[1], ("params", "m", "v", "ema", "gnorm[:2]")):
        assert torch.equal(a, b), name
    gn, s = out[0][4].tolist()
    assert gn > 0.01 and 0 < s < 1.0, (gn, s)               # clipping was active


# ------------------------------------------------------------------ 7. a non-finite gradient
def test_nonfinite_gradient_gives_nan_parameters(dev, K):
    init, fp = build(dev, 46)
    cfg = OptConfig(lr0=0.05, ema_max=0.9999, use_momentum=True, momentum=0.9, clip_norm=CLIP)
    fp.init_slots(cfg)
    fp.grads.copy_(torch.randn(fp.total))
    fp.grads[700] = float("inf")
    fp.apply(cfg, grad_scale=0.5)
    torch.cuda.synchronize()
    gn, s = fp.gnorm[:2].tolist()
    assert not np.isfinite(gn) and np.isnan(s), (gn, s)
    assert torch.isnan(fp.params).all()
