"""LARS and LAMB in the fused optimizer step (optimizer.hip var_sqnorm_k + var_ratio_k +
layerwise_opt_k), on the GPU: the per-variable reduction against float64, both rules against the
float64 oracle (tests/layerwise_oracle.py) on a layout that hits every access path, the exact
identity of lars at ratio 1 with momentum, the binding's validation, the executors' wiring,
hipGraph replay against eager (bitwise), a non-finite gradient and one whole step against the
plain-torch update.

Tolerances: the project's ``adaptive_oracle.close`` (max |out - ref| <= 1e-5 max |ref| + 1e-6) for
tensors, 1e-5 relative for norms and ratios."""
import importlib.util
import os
import struct

import numpy as np
import pytest
import torch

from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.runtime.params import FlatParams, OptConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("layerwise_oracle", os.path.join(ROOT, "tests", "layerwise_oracle.py"))
oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(oracle)

pytestmark = pytest.mark.gpu

# the layout of test_clip_norm_gpu.py -- offsets 0 / 175 / 182 / 1502 / 1535 / 2195: odd offsets
# (scalar path), odd counts (scalar tails), 8-byte pairs, segments of more than one 512-element chunk
SHAPES = [("a/weights", (5, 5, 1, 7), 0.0), ("a/biases", (7,), None), ("b/weights", (40, 33), 0.004),
          ("b/biases", (33,), None), ("c/weights", (33, 20), 0.002), ("c/biases", (20,), None)]
PADS = {"a/weights": (2, 8), "b/weights": (40, 40), "c/weights": (40, 24)}
WDS = {n: wd for n, _, wd in SHAPES}
AMPL = [1.0, 0.1, 2.0, 0.05, 1.0]
LR0 = {"lars": 0.5, "lamb": 0.01}


def np_of(t):
    return t.detach().cpu().numpy()


def build(dev, seed, transposed=True, zero_c=False):
    torch.manual_seed(seed)
    init = {n: torch.randn(*s) for n, s, _ in SHAPES}
    if zero_c:
        init["c/weights"].zero_()
    fp = FlatParams.build(SHAPES, init, dev, pads=PADS)
    if transposed:
        fp.enable_transposed({"b/weights": (40, 48)})
    return init, fp


def cfg_of(rule, lr0=None, **kw):
    return OptConfig(lr0=LR0[rule] if lr0 is None else lr0, ema_max=0.9999, rule=rule, momentum=0.9, **kw)


def partials(tnorm, nvar, nb):
    """[nvar][nb][2] view of the reduction's per-(variable, block) partial sums."""
    return np_of(tnorm[3 * nvar:3 * nvar + 2 * nvar * nb]).reshape(nvar, nb, 2)


def check_norms(rule, tnorm, segs, p, gr, grad_scale, m=None, v=None, t=1):
    """tnorm[3k], tnorm[3k + 1] against float64 per hand-built or FlatParams segment row; returns the
    float64 (pn, un) list."""
    head = np_of(tnorm[:3 * len(segs)]).reshape(-1, 3)
    want = []
    for k, row in enumerate(segs):
        off, n = int(row[0]), int(row[1])
        wd = np.float64(struct.unpack("<f", struct.pack("<i", int(row[8])))[0])
        sl = slice(off, off + n)
        g = gr[sl].astype(np.float64) * grad_scale + wd * p[sl].astype(np.float64)
        pn, un = oracle.var_norms(rule, p[sl], g, None if m is None else m[sl], None if v is None else v[sl], t=t)
        print(f"{rule} variable {k} ({n} elements): pn {head[k, 0]:.7g} (float64 {pn:.7g}), "
              f"un {head[k, 1]:.7g} ({un:.7g}), ratio {head[k, 2]:.7g}")
        oracle.close_scalar(head[k, 0], pn)
        oracle.close_scalar(head[k, 1], un)
        want.append((pn, un))
    return want


def lamb_state(total, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    mom = torch.randn(total, device=dev, generator=g) * 0.1
    slot2 = torch.rand(total, device=dev, generator=g) * 0.01
    step = torch.full((1,), 3, dtype=torch.int64, device=dev)
    return mom, slot2, step


# ------------------------------------------------------------------ 1. the reduction alone
@pytest.mark.parametrize("rule", oracle.RULES)
def test_var_norms_six_tensor_layout(dev, K, rule):
    init, fp = build(dev, 50, transposed=False)
    segs = fp.segs.tolist()
    assert [int(r[0]) for r in segs] == [0, 175, 182, 1502, 1535, 2195]
    assert [int(r[13]) for r in segs] == [1, 0, 1, 0, 1, 0]
    nvar, nb = len(segs), int(K.grad_norm_max_blocks())
    assert int(K.var_norm_buffer_size(nvar)) == nvar * (3 + 2 * nb)
    fp.grads.copy_(torch.randn(fp.total))
    tnorm = torch.full((int(K.var_norm_buffer_size(nvar)),), 7.0, device=dev)   # stale partials must not survive
    kw = {}
    m = v = None
    if rule == "lamb":
        mom, slot2, step = lamb_state(fp.total, dev, 51)
        kw = {"mom": mom, "slot2": slot2, "step": step}
        m, v = np_of(mom), np_of(slot2)
    K.var_norms(fp.params, fp.grads, fp.segs, 0.5, tnorm, rule=rule, **kw)
    first = tnorm.clone()
    want = check_norms(rule, tnorm, segs, np_of(fp.params), np_of(fp.grads), 0.5, m, v, t=4)
    head = np_of(tnorm[:3 * nvar]).reshape(-1, 3)
    for k, (pn, un) in enumerate(want):
        r = oracle.ratio(rule, bool(segs[k][13]), pn, un)
        oracle.close_scalar(head[k, 2], r)
        assert segs[k][13] or head[k, 2] == 1.0
    assert not (np_of(tnorm) == 7.0).any()
    # 9 chunks over nb blocks: one chunk per block; everything else stored 0
    part = partials(tnorm, nvar, nb)
    blk0 = np.cumsum([0] + [-(-int(r[1]) // 512) for r in segs])
    for k in range(nvar):
        own = np.zeros(nb, dtype=bool)
        own[blk0[k]:blk0[k + 1]] = True
        assert (part[k, own, 0] > 0).all() and (part[k, ~own] == 0).all(), k
    K.var_norms(fp.params, fp.grads, fp.segs, 0.5, tnorm, rule=rule, **kw)
    assert torch.equal(tnorm, first)                                          # bitwise repeatable


@pytest.mark.parametrize("extra", [0, 512])
@pytest.mark.parametrize("rule", oracle.RULES)
def test_var_norms_segment_boundary_inside_a_blocks_range(dev, K, rule, extra):
    """A weight of 2 * 512 * nb + 777 (+ extra) elements (wd 0.003), a weight of 1300 and a bias
    of 33: each reduction block walks several chunks.  extra = 0 is the layout as specified; at
    nb = 512 its first weight fills 1026 chunks = 342 blocks of 3 exactly, so the boundaries fall
    between blocks.  extra = 512 moves them inside: block 342 then holds the ragged tail of the
    first weight and two chunks of the second, block 343 the second's last chunk and the bias."""
    nb = int(K.grad_norm_max_blocks())
    assert 1 <= nb <= 1024
    ns = [2 * 512 * nb + 777 + extra, 1300, 33]
    wd_bits = struct.unpack("<i", struct.pack("<f", 0.003))[0]
    rows, off = [], 0
    for n, wb, adapt in zip(ns, (wd_bits, 0, 0), (1, 1, 0)):
        rows.append([off, n, 1, 1, n, 1, n, -1, wb, 0, -1, 0, 0, adapt])
        off += n
    segs = torch.tensor(rows, dtype=torch.int64)
    g = torch.Generator(device=dev).manual_seed(52)
    p = torch.randn(off, device=dev, generator=g)
    gr = torch.randn(off, device=dev, generator=g)
    kw = {}
    m = v = None
    if rule == "lamb":
        mom, slot2, step = lamb_state(off, dev, 53)
        kw = {"mom": mom, "slot2": slot2, "step": step}
        m, v = np_of(mom), np_of(slot2)
    tnorm = torch.full((int(K.var_norm_buffer_size(3)),), 7.0, device=dev)
    K.var_norms(p, gr, segs, 0.5, tnorm, rule=rule, **kw)
    first = tnorm.clone()
    check_norms(rule, tnorm, rows, np_of(p), np_of(gr), 0.5, m, v, t=4)
    assert float(tnorm[8]) == 1.0                                              # the bias: not adapted
    # which blocks hold a chunk of which variable; every other (variable, block) pair stored 0
    chunks = [-(-n // 512) for n in ns]
    per = max(1, -(-sum(chunks) // nb))
    part = partials(tnorm, 3, nb)
    c0 = 0
    crossing = set()
    for k, nc in enumerate(chunks):
        own = np.zeros(nb, dtype=bool)
        own[c0 // per:(c0 + nc - 1) // per + 1] = True
        assert (part[k, own, 0] > 0).all() and (part[k, ~own] == 0).all(), k
        if c0 % per:
            crossing.add(c0 // per)
        c0 += nc
    assert per >= 2 and (extra == 0 or len(crossing) == 2), (per, crossing)
    K.var_norms(p, gr, segs, 0.5, tnorm, rule=rule, **kw)
    assert torch.equal(tnorm, first)


# ------------------------------------------------------------------ 3. fp.apply against the oracle
def check_state(fp, ref, rule, names):
    for n in names:
        s1, s2 = fp.slot_views(n)
        oracle.close(np_of(fp.param_view(n)), ref.p[n])
        oracle.close(np_of(fp.ema_view(n)), ref.ema[n])
        oracle.close(np_of(s1), ref.s1[n])
        if rule == "lamb":
            oracle.close(np_of(s2), ref.s2[n])


def check_ratios(fp, ref, names, label):
    tr = fp.trust_ratios()
    for n in names:
        pn, un, r = tr[n]
        print(f"{label} {n}: pn {pn:.7g} ({ref.pn[-1][n]:.7g}), un {un:.7g} ({ref.un[-1][n]:.7g}), "
              f"ratio {r:.7g} ({ref.r[-1][n]:.7g})")
        for got, want in ((pn, ref.pn[-1][n]), (un, ref.un[-1][n]), (r, ref.r[-1][n])):
            assert np.isfinite(got) and abs(got - want) <= 1e-5 * abs(want), (label, n, got, want)
        if n.endswith("biases"):
            assert r == 1.0, (label, n, r)


@pytest.mark.parametrize("self_sum", [0, 1])
@pytest.mark.parametrize("rule", oracle.RULES)
def test_update_matches_float64_oracle(dev, K, rule, self_sum):
    """Both hand-offs of the ratio: the one-block-per-variable launch (0) and every apply block
    summing its variable's partials itself (1)."""
    prev = K.layerwise_self_sum_mode()                       # -1: chosen by the number of chunks
    K.set_layerwise_self_sum(self_sum)
    try:
        init, fp = build(dev, 54, zero_c=True)                # c/weights = 0: pn = 0, ratio 1 at step 1
        cfg = cfg_of(rule, decay_rate=0.5, decay_steps=2)
        fp.init_slots(cfg)
        assert fp.tnorm is not None and fp.tnorm.numel() == K.var_norm_buffer_size(len(SHAPES))
        ref = oracle.LayerwiseOracle(rule, {n: v.numpy() for n, v in init.items()}, WDS, LR0[rule], 0.5, 2, 0.9999,
                                     grad_scale=0.5)
        for k in range(5):
            g = {n: torch.randn_like(init[n]) * AMPL[k] for n in init}
            if k == 0:
                g["a/weights"].zero_()                        # wd 0: gn = un = 0, ratio 1 at step 1
            for n in g:
                fp.grad_view(n).copy_(g[n])
            fp.apply(cfg, grad_scale=0.5)
            fp.step.add_(1)
            ref.step({n: v.numpy() for n, v in g.items()})
            check_ratios(fp, ref, list(init), f"{rule} step {k}")
        assert ref.r[0]["a/weights"] == 1.0 and ref.r[0]["c/weights"] == 1.0 and ref.r[0]["b/weights"] != 1.0
        assert all(ref.r[k][n] != 1.0 for k in range(1, 5) for n in init if n.endswith("weights"))
        check_state(fp, ref, rule, list(init))
    finally:
        K.set_layerwise_self_sum(int(prev))
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


@pytest.mark.parametrize("rule", oracle.RULES)
def test_both_handoffs_above_the_size_threshold(dev, K, rule):
    """Up to 1024 chunks the apply blocks sum their variable's partials themselves, above that the
    one-block-per-variable launch does.  1030 chunks (the boundary layout + 512): the default takes
    the launch (bitwise the forced one), the forced self-sum gives the same update, and the ratios
    match float64 either way."""
    nb = int(K.grad_norm_max_blocks())
    ns = [2 * 512 * nb + 777 + 512, 1300, 33]
    assert sum(-(-n // 512) for n in ns) > 1024
    wd_bits = struct.unpack("<i", struct.pack("<f", 0.003))[0]
    rows, off = [], 0
    for n, wb, adapt in zip(ns, (wd_bits, 0, 0), (1, 1, 0)):
        rows.append([off, n, 1, 1, n, 1, n, -1, wb, 0, -1, 0, 0, adapt])
        off += n
    segs = torch.tensor(rows, dtype=torch.int64)
    g = torch.Generator(device=dev).manual_seed(59)
    p0 = torch.randn(off, device=dev, generator=g)
    gr = torch.randn(off, device=dev, generator=g)
    mom0, slot20, _ = lamb_state(off, dev, 60)
    bf = torch.zeros(1, dtype=torch.bfloat16, device=dev)
    step = torch.full((1,), 3, dtype=torch.int64, device=dev)
    prev = K.layerwise_self_sum_mode()
    out = {}
    try:
        for mode in (-1, 0, 1):
            K.set_layerwise_self_sum(mode)
            p, mom, slot2, ema = p0.clone(), mom0.clone(), slot20.clone(), p0.clone()
            tnorm = torch.full((int(K.var_norm_buffer_size(3)),), 7.0, device=dev)
            K.fused_optimizer(p, gr, mom, ema, bf, segs, step, 0.05, 0.1, 0, 0.9, False, True, 0.5, 0.9999,
                              rule=rule, slot2=slot2, tnorm=tnorm, lars_eta=0.01)
            torch.cuda.synchronize()
            out[mode] = (p, mom, slot2, ema, tnorm[:9].clone())
    finally:
        K.set_layerwise_self_sum(int(prev))
    for a, b, name in zip(out[-1], out[0], ("params", "slot 1", "slot 2", "ema", "norms and ratios")):
        assert torch.equal(a, b), name
    for a, b in zip(out[1][:4], out[0][:4]):
        oracle.close(np_of(a), np_of(b).astype(np.float64))
    m = np_of(mom0) if rule == "lamb" else None
    v = np_of(slot20) if rule == "lamb" else None
    for mode in (0, 1):
        want = check_norms(rule, out[mode][4], rows, np_of(p0), np_of(gr), 0.5, m, v, t=4)
        head = np_of(out[mode][4]).reshape(3, 3)
        for k, (pn, un) in enumerate(want):
            oracle.close_scalar(head[k, 2], oracle.ratio(rule, bool(rows[k][13]), pn, un, eta=0.01))
    assert not torch.equal(out[0][0], p0)


# ------------------------------------------------------------------ 4. lars at ratio 1 is momentum, bit for bit
def test_lars_without_adapted_rows_is_bitwise_momentum(dev, K):
    out = []
    for rule in ("lars", "momentum"):
        init, fp = build(dev, 55)
        fp.segs[:, 13] = 0                                     # no variable adapted: every ratio is 1
        if rule == "lars":
            cfg = cfg_of("lars", lr0=0.05, decay_rate=0.5, decay_steps=2)
        else:
            cfg = OptConfig(lr0=0.05, decay_rate=0.5, decay_steps=2, ema_max=0.9999, use_momentum=True, momentum=0.9)
        fp.init_slots(cfg)
        torch.manual_seed(56)
        for _ in range(3):
            fp.grads.copy_(torch.randn(fp.total))
            fp.apply(cfg, grad_scale=0.5)
            fp.step.add_(1)
        torch.cuda.synchronize()
        out.append([t.clone() for t in (fp.params, fp.mom, fp.ema, fp.bf16)])
        if rule == "lars":
            head = np_of(fp.tnorm[:18]).reshape(6, 3)
            assert (head[:, 2] == 1.0).all() and (head[:, :2] > 0).all()
    for a, b, name in zip(out[0], out[1], ("params", "mom", "ema", "bf16 copies")):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------ 5. the binding validates
def test_binding_validates_layerwise_arguments(dev, K):
    init, fp = build(dev, 57, transposed=False)
    fp.grads.copy_(torch.randn(fp.total))
    args = (fp.params, fp.grads, fp.mom, fp.ema, fp.bf16, fp.segs, fp.step, 0.1, 0.1, 0, 0.9, False, True, 1.0,
            0.9999)
    tnorm = torch.zeros(int(K.var_norm_buffer_size(len(SHAPES))), device=dev)
    slot2 = torch.zeros(fp.total, device=dev)
    gnorm = torch.zeros(2 + K.grad_norm_max_blocks(), device=dev)
    for rule, extra in (("lars", {}), ("lamb", {"slot2": slot2})):
        with pytest.raises(RuntimeError, match="needs tnorm"):
            K.fused_optimizer(*args, rule=rule, **extra)
        with pytest.raises(RuntimeError, match="tnorm"):
            K.fused_optimizer(*args, rule=rule, tnorm=tnorm[:-1], **extra)
        with pytest.raises(RuntimeError, match="tnorm"):
            K.fused_optimizer(*args, rule=rule, tnorm=tnorm.cpu(), **extra)
        with pytest.raises(RuntimeError, match="tnorm"):
            K.fused_optimizer(*args, rule=rule, tnorm=tnorm.double(), **extra)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(RuntimeError, match="lars_eta"):
                K.fused_optimizer(*args, rule=rule, tnorm=tnorm, lars_eta=bad, **extra)
        guard = torch.zeros(1, dtype=torch.int64, device=dev)
        guard_err = torch.zeros(1, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError, match="push guard"):
            K.fused_optimizer(*args, None, guard, 0, guard_err, 0, rule=rule, tnorm=tnorm, **extra)
        with pytest.raises(RuntimeError, match="clip_norm"):
            K.fused_optimizer(*args, rule=rule, tnorm=tnorm, clip_norm=1.0, gnorm=gnorm, **extra)
        with pytest.raises(RuntimeError, match="init_slots"):
            fp.apply(OptConfig(rule=rule))
        assert int(guard_err.item()) == 0
    with pytest.raises(RuntimeError, match="needs slot2"):
        K.fused_optimizer(*args, rule="lamb", tnorm=tnorm)
    with pytest.raises(RuntimeError, match=r"sgd\|momentum\|nesterov\|adam\|rmsprop\|adagrad\|lars\|lamb"):
        K.fused_optimizer(*args, rule="lion")
    with pytest.raises(RuntimeError, match="tnorm"):
        K.var_norms(fp.params, fp.grads, fp.segs, 1.0, tnorm[:-1])
    with pytest.raises(RuntimeError, match="lamb needs"):
        K.var_norms(fp.params, fp.grads, fp.segs, 1.0, tnorm, rule="lamb")
    torch.cuda.synchronize()
    assert torch.equal(fp.params.cpu(), torch.cat([init[n].reshape(-1) for n, _, _ in SHAPES]))   # nothing ran
    assert tnorm.abs().sum().item() == 0 and fp.mom.abs().sum().item() == 0 and slot2.abs().sum().item() == 0


# ------------------------------------------------------------------ 6. the executors
def _fill_batch(net, B, g, f32=False):
    x = torch.rand(B, 28, 28, 1, device=net.device, generator=g) - 0.5
    net.x0.copy_(x if f32 else x.to(torch.bfloat16))
    net.labels.copy_(torch.randint(0, 10, (B,), device=net.device, generator=g, dtype=torch.int32))


EXEC_LR = {"lars": 0.2, "lamb": 0.005}
LENET_WEIGHTS = ["conv1/weights", "conv2/weights", "local3/weights", "local4/weights", "softmax_linear/weights"]


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("rule", oracle.RULES)
def test_executors_run_the_layerwise_rules(dev, K, rule, f32):
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor_f32 import HipNetF32
    B = 128
    spec = get_model("lenet5", 1)
    cfg = cfg_of(rule, lr0=EXEC_LR[rule], lars_eta=0.02)
    net = (HipNetF32 if f32 else HipNet)(spec, B, dev, torch_ref.init_params(spec, seed=3), cfg)
    weights = [e.name for e in net.fp.entries if len(e.shape) >= 2]
    assert len(weights) == 5
    g = torch.Generator(device=dev).manual_seed(3)
    for _ in range(3):
        _fill_batch(net, B, g, f32)
        net.train_step()
    st = net.read_stats()
    print(f"{rule} f32={f32}: {st}")
    assert np.isfinite(st["total_loss"]) and np.isfinite(st["cross_entropy"]) and st["nan"] == 0.0
    assert sorted(k for k in st if k.startswith("trust_ratio/")) == sorted(f"trust_ratio/{n}" for n in weights)
    assert all(np.isfinite(st[f"trust_ratio/{n}"]) and 0 < st[f"trust_ratio/{n}"] != 1.0 for n in weights)
    assert all(r == 1.0 for n, (_, _, r) in net.fp.trust_ratios().items() if n not in weights)
    assert int(net.fp.step.item()) == 3 and torch.isfinite(net.fp.params).all()


@pytest.mark.parametrize("rule", oracle.RULES)
def test_graph_replay_equals_eager_bitwise(dev, K, rule):
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
    from distributed_tensorflow_ibm_mnist_amd.runtime.graph import StepGraph
    B, steps = 128, 4
    spec = get_model("lenet5", 1)
    g = torch.Generator(device=dev).manual_seed(8)
    xs = [(torch.rand(B, 28, 28, 1, device=dev, generator=g) - 0.5).to(torch.bfloat16) for _ in range(steps)]
    ys = [torch.randint(0, 10, (B,), device=dev, generator=g, dtype=torch.int32) for _ in range(steps)]
    out = []
    for graph in (False, True):
        net = HipNet(spec, B, dev, torch_ref.init_params(spec, seed=8), cfg_of(rule, lr0=EXEC_LR[rule], lars_eta=0.02))
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
        slot2 = net.fp.slot2 if rule == "lamb" else net.fp.mom
        out.append([t.clone() for t in (net.fp.params, net.fp.mom, slot2, net.fp.ema, net.fp.tnorm, net.stats)])
    for a, b, name in zip(out[0], out[1], ("params", "slot 1", "slot 2", "ema", "tnorm", "stats")):
        assert torch.equal(a, b), name
    head = np_of(out[0][4][:30]).reshape(10, 3)
    assert np.isfinite(head).all() and (head[0::2, 2] != 1.0).all() and (head[1::2, 2] == 1.0).all(), head


# ------------------------------------------------------------------ 7. a non-finite gradient
@pytest.mark.parametrize("rule", oracle.RULES)
def test_nonfinite_gradient_gives_nan_ratio_and_parameters(dev, K, rule):
    init, fp = build(dev, 58)
    cfg = cfg_of(rule, lr0=0.05)
    fp.init_slots(cfg)
    fp.grads.copy_(torch.randn(fp.total))
    fp.grads[700] = float("inf")                                  # inside b/weights
    fp.apply(cfg, grad_scale=0.5)
    torch.cuda.synchronize()
    tr = fp.trust_ratios()
    assert np.isnan(tr["b/weights"][2]) and not np.isfinite(tr["b/weights"][1]), tr["b/weights"]
    assert torch.isnan(fp.param_view("b/weights")).all()
    for n in ("a/weights", "a/biases", "b/biases", "c/weights", "c/biases"):
        assert np.isfinite(tr[n][2]) and torch.isfinite(fp.param_view(n)).all(), n


def test_nonfinite_gradient_raises_the_nan_flag_on_the_next_step(dev, K):
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
    B = 128
    spec = get_model("lenet5", 1)
    net = HipNet(spec, B, dev, torch_ref.init_params(spec, seed=4), cfg_of("lars", lr0=EXEC_LR["lars"], lars_eta=0.02))
    g = torch.Generator(device=dev).manual_seed(4)
    _fill_batch(net, B, g)
    net.forward(defer_head=True)
    net.loss_and_grad()
    net.backward()
    net.fp.grad_view("conv2/weights").view(-1)[11] = float("inf")
    net.update()
    st = net.read_stats()
    assert st["nan"] == 0.0 and np.isnan(st["trust_ratio/conv2/weights"]), st
    assert torch.isnan(net.fp.param_view("conv2/weights")).all()
    assert torch.isfinite(net.fp.param_view("conv1/weights")).all()
    net.train_step()
    assert net.read_stats()["nan"] == 1.0


# ------------------------------------------------------------------ 8. one whole step against plain torch
def test_lenet_lars_steps_match_the_plain_torch_update(dev, K):
    """LeNet-5, B = 128, 3 lars steps on HipNet; every step's update is repeated by TorchNet's
    torch_update from the same parameters, slots and gradients and compared with the whole-step
    measure the adaptive rules' executor tests use (adaptive_oracle.close).  The repository has no
    tolerance between the two executors' forward / backward passes (bf16 kernels against autocast),
    so the gradients are HipNet's."""
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import TorchNet, torch_update
    B = 128
    spec = get_model("lenet5", 1)
    init = torch_ref.init_params(spec, seed=5)
    cfg = cfg_of("lars", lr0=EXEC_LR["lars"], lars_eta=0.02)
    net = HipNet(spec, B, dev, init, cfg)
    tn = TorchNet(spec, B, dev, init, cfg_of("lars", lr0=EXEC_LR["lars"], lars_eta=0.02))
    assert tn.fp.names() == net.fp.names() and tn.fp.total == net.fp.total
    g = torch.Generator(device=dev).manual_seed(5)
    for k in range(3):
        _fill_batch(net, B, g)
        net.forward(defer_head=True)
        net.loss_and_grad()
        net.backward()
        for a, b in ((tn.fp.params, net.fp.params), (tn.fp.grads, net.fp.grads), (tn.fp.mom, net.fp.mom),
                     (tn.fp.ema, net.fp.ema), (tn.fp.step, net.fp.step)):
            a.copy_(b)
        net.update()
        torch_update(tn.fp, tn.opt)
        torch.cuda.synchronize()
        for n in net.fp.names():
            oracle.close(np_of(net.fp.param_view(n)), np_of(tn.fp.param_view(n)).astype(np.float64))
            oracle.close(np_of(net.fp.mom_view(n)), np_of(tn.fp.mom_view(n)).astype(np.float64))
            oracle.close(np_of(net.fp.ema_view(n)), np_of(tn.fp.ema_view(n)).astype(np.float64))
        a, b = net.fp.trust_ratios(), tn.fp.trust_ratios()
        for n in net.fp.names():
            for x, y in zip(a[n], b[n]):
                assert abs(x - y) <= 1e-5 * abs(y), (k, n, a[n], b[n])
    assert net.read_stats()["nan"] == 0.0
