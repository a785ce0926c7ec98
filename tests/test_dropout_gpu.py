"""Dropout on the device: the counter-based masks (csrc/kernels/dropout_rng.h) against the host
reference (ops/dropout.py) bit for bit, the stand-alone kernels (dropout.hip), the dropped
instantiations of the fused LeNet-5 head (mlp_head_drop.hip), the executors' training paths against
the oracle under the reference masks, rate 0 and the eval paths bitwise what they were, hipGraph
replay, the refusals and the library module."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.ops import dropout as D
from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED40 = (0xA5 << 32) | 0x1234567          # a 40-bit seed: both key words are used
SENT = 1e30


def rel_err(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _step_t(dev, t):
    return torch.tensor([t], dtype=torch.int64, device=dev)


def _mask(seed, t, layer, rows, n, p, dev):
    return torch.from_numpy(D.keep_mask(seed, t, layer, rows, n, p)).to(dev)


# ------------------------------------------------------------------ 1. device bits == host reference
@pytest.mark.parametrize("t", [0, 7, (1 << 32) + 5])
def test_device_mask_equals_host_reference(dev, K, t):
    step = _step_t(dev, t)
    for nb in (1, 33, 257):
        for n in (84, 120, 192, 1024):
            for layer, p in ((3, 0.5), (65535, 0.2)):
                out = torch.full((nb + 1, n), 7, dtype=torch.uint8, device=dev)
                K.dropout_mask(out, nb, n, step, SEED40, layer, p)
                want = D.keep_mask(SEED40, t, layer, nb, n, p)
                assert np.array_equal(out[:nb].cpu().numpy().astype(bool), want), (nb, n, layer, p)
                assert bool((out[nb] == 7).all()), "dropout_mask wrote a row >= nb"


def test_device_mask_known_rows(dev, K):
    """The issue's two rows, from the device."""
    out = torch.empty(256, 120, dtype=torch.uint8, device=dev)
    K.dropout_mask(out, 256, 120, _step_t(dev, 7), 1234, 3, 0.5)
    assert out[0, :16].tolist() == [1, 0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1]
    assert out[255, 104:120].tolist() == [0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0]


# ------------------------------------------------------------------ 2. stand-alone forward / backward
def _bf16_rne(v):
    """float64 array (finite) -> the nearest bf16 values, ties to even, as float64: ONE rounding of
    the 8-bit significand (numpy's rint rounds half to even; bf16's exponent range is fp32's)."""
    m, e = np.frexp(v)
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


def _standalone_ref(y, mask, inv_keep):
    """bf16_rne(float64(y) * float64(inv_keep)) where kept, +0 where dropped: the product of an 8-bit
    and a 24-bit significand is exact in float64, so the one rounding is the kernel's own."""
    kept = torch.where(mask, y, torch.zeros_like(y)).double().cpu().numpy()       # dropped: may be NaN / inf
    out = torch.from_numpy(_bf16_rne(kept * float(inv_keep))).to(torch.bfloat16)  # representable: exact
    return torch.where(mask, out.to(y.device), torch.zeros_like(y))


@pytest.mark.parametrize("p", [0.5, 0.2, 0.1])
@pytest.mark.parametrize("nb,n,ld", [(33, 84, 88), (257, 120, 120), (33, 192, 192), (5, 1024, 1024), (3, 2056, 2056)])
def test_standalone_forward_and_backward_are_exact(dev, K, nb, n, ld, p):
    t, layer = 7, 4
    step = _step_t(dev, t)
    thr, inv = D.threshold(p)
    mask = _mask(SEED40, t, layer, nb, n, p, dev)
    g = torch.Generator(device="cpu").manual_seed(nb * 1000 + n)
    rows = nb + 2
    for bwd in (False, True):
        v = torch.randn(rows, ld, generator=g)
        if not bwd:
            v = torch.relu(v)                          # an activation: zeros among the values
        else:
            v[:, ::5] = 0.0                            # a gradient: negative entries and zeros
        v = v.to(torch.bfloat16).to(dev)
        v[:, n:] = SENT                                # padded columns
        v[nb:] = SENT                                  # rows past nb
        dropped = (~mask).nonzero()
        r0, c0 = dropped[0].tolist()
        r1, c1 = dropped[-1].tolist()
        v[r0, c0] = float("nan")                       # a NaN and an infinity in dropped positions
        v[r1, c1] = float("-inf")
        want = v.clone()
        want[:nb, :n] = _standalone_ref(v[:nb, :n], mask, inv)
        (K.dropout_bwd if bwd else K.dropout_fwd)(v, nb, n, ld, step, SEED40, layer, p)
        torch.cuda.synchronize()
        assert torch.equal(v, want), ("bwd" if bwd else "fwd", nb, n, p)
        assert v[r0, c0].item() == 0.0 and v[r1, c1].item() == 0.0
        assert not torch.signbit(v[r0, c0]).item() and not torch.signbit(v[r1, c1]).item()    # +0
        assert bool((v[:nb, n:] == SENT).all()) and bool((v[nb:] == SENT).all())


@pytest.mark.parametrize("thr,bits", [(31335, 0x3FA4), (49195, 0x3F8F), (58969, 0x3FDC)])
def test_standalone_rounds_once_where_two_roundings_differ(dev, K, thr, bits):
    """Keep thresholds at which the fp32 product of one bf16 significand and inv_keep lands exactly on a
    bf16 tie although the exact product does not (found by enumerating all thresholds and
    significands): rounding the fp32 product would differ from the one rounding of the exact
    product.  All 256 sign / significand patterns of two binades, 64 rows each."""
    p = 1.0 - thr / 65536.0
    assert D.threshold(p)[0] == thr
    inv = D.threshold(p)[1]
    x1 = torch.tensor([bits << 16], dtype=torch.int32).view(torch.float32).double().item()
    two = float(np.float32(np.float32(x1) * np.float32(inv)))          # fp32 product, then bf16
    assert torch.tensor([two]).to(torch.bfloat16).double().item() != _bf16_rne(np.array([x1 * inv]))[0]
    pat = torch.cat([torch.arange(0x3F80, 0x4080), torch.arange(0xBF80, 0xC080)]).to(torch.int32)
    row = (pat << 16).view(torch.float32).to(torch.bfloat16)
    v = row.repeat(64, 1).contiguous().to(dev)
    mask = _mask(SEED40, 2, 1, 64, 512, p, dev)
    want = _standalone_ref(v, mask, inv)
    K.dropout_fwd(v, 64, 512, 512, _step_t(dev, 2), SEED40, 1, p)
    assert torch.equal(v, want)
    col = int((pat == bits).nonzero()[0])
    assert bool(mask[:, col].any())                                    # the tie case itself was kept somewhere


def test_standalone_rate_zero_launches_nothing(dev, K):
    v = torch.randn(9, 16, device=dev).to(torch.bfloat16)
    w = v.clone()
    K.dropout_fwd(v, 9, 16, 16, _step_t(dev, 3), 1, 0, 0.0)
    assert torch.equal(v, w)


# ------------------------------------------------------------------ 3. fused head, exact part
def _tr(w, rows, cols):
    t = torch.zeros(rows, cols, dtype=torch.bfloat16, device=w.device)
    t[:w.shape[1], :w.shape[0]] = w.t()
    return t


def _head_inputs(dev, B, seed):
    torch.manual_seed(seed)
    p = {"x": torch.relu(torch.randn(B, 400, device=dev)).to(torch.bfloat16),
         "w3": (torch.randn(400, 120, device=dev) * 0.07).to(torch.bfloat16),
         "w4": (torch.randn(120, 84, device=dev) * 0.13).to(torch.bfloat16),
         "w5": (torch.randn(84, 10, device=dev) * 0.3).to(torch.bfloat16),
         "y": torch.randint(0, 10, (B,), device=dev, dtype=torch.int32)}
    p["b3"], p["b4"], p["b5"] = (torch.randn(k, device=dev) * 0.1 for k in (120, 84, 10))
    return p


def _run_head(K, dev, p, nb, **kw):
    B = p["x"].shape[0]
    bf = dict(dtype=torch.bfloat16, device=dev)
    o = {"h3": torch.full((B, 120), SENT, **bf), "h4": torch.full((B, 88), SENT, **bf),
         "logits": torch.full((B, 16), SENT, device=dev), "dl": torch.full((B, 16), SENT, **bf),
         "dh4": torch.full((B, 88), SENT, **bf), "dh3": torch.full((B, 120), SENT, **bf),
         "dx": torch.full((B, 400), SENT, **bf)}
    stats, work = torch.zeros(8, device=dev), torch.zeros(4 * 1024 + 1, device=dev)
    dbias = torch.zeros(K.mlp_head_blocks(nb) * 16, device=dev)
    K.mlp_head(p["x"], _tr(p["w3"], 128, 416), p["b3"], 120, _tr(p["w4"], 96, 128), p["b4"], 84,
               _tr(p["w5"], 16, 96), p["b5"], 10, p["y"], nb, 1.0 / nb, o["h3"], o["h4"], o["logits"],
               dl=o["dl"], dh4=o["dh4"], dh3=o["dh3"], dx=o["dx"], stats=stats, work=work, dbias=dbias, **kw)
    torch.cuda.synchronize()
    o["stats"] = stats
    return o


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("p", [0.5, 0.75])
@pytest.mark.parametrize("nb", [31, 33, 257, 300])
def test_fused_head_stores_the_exactly_dropped_h3(dev, K, nb, p, eps):
    """inv_keep is 2 (p = 0.5) or 4 (0.75), and scaling by a power of two commutes with the bf16
    rounding: the stored h3 is bitwise inv_keep * h3_plain * mask, h3_plain from the plain launch on
    the same inputs.  Downstream of h3 the kernel's own outputs are chained with the layered
    formulas (tests/test_mlp_head_gpu.py's bounds: 1e-2 activations, 2e-2 gradients)."""
    B, t, l3, l4 = 512, 7, 5, 6
    inputs = _head_inputs(dev, B, 900 + nb)
    thr, inv = D.threshold(p)
    plain = _run_head(K, dev, inputs, nb, label_smoothing=eps)
    o = _run_head(K, dev, inputs, nb, label_smoothing=eps, dropout=p, drop_step=_step_t(dev, t), drop_seed=SEED40,
                  drop_layer3=l3, drop_layer4=l4)
    m3 = _mask(SEED40, t, l3, nb, 120, p, dev)
    m4 = _mask(SEED40, t, l4, nb, 84, p, dev)
    want3 = torch.where(m3, (plain["h3"][:nb].float() * inv).to(torch.bfloat16), torch.zeros_like(plain["h3"][:nb]))
    assert torch.equal(o["h3"][:nb], want3)
    # h4 from the kernel's own h3: dropped units are exactly 0, kept ones the layered formula
    w3, w4, w5 = inputs["w3"].float(), inputs["w4"].float(), inputs["w5"].float()
    h4 = torch.relu(o["h3"][:nb].float() @ w4 + inputs["b4"]) * inv * m4
    assert not o["h4"][:nb, :84][~m4].any()
    assert rel_err(o["h4"][:nb, :84], h4) < 1e-2
    assert not o["h4"][:nb, 84:].any()                              # padded columns are zero
    z = o["logits"][:nb, :10]
    assert rel_err(z, o["h4"][:nb, :84].float() @ w5 + inputs["b5"]) < 1e-2
    # backward: dy *= keep ? inv_keep : 0, the bit read off the stored activation
    k4, k3 = o["h4"][:nb, :84].float() > 0, o["h3"][:nb].float() > 0
    dh4 = ((o["dl"][:nb, :10].float() @ w5.t()) * k4 * inv).to(torch.bfloat16)
    dh3 = ((dh4.float() @ w4.t()) * k3 * inv).to(torch.bfloat16)
    dx = dh3.float() @ w3.t()
    for name, got, want in (("dh4", o["dh4"][:nb, :84], dh4), ("dh3", o["dh3"][:nb], dh3), ("dx", o["dx"][:nb], dx)):
        e = rel_err(got, want)
        print(f"nb={nb} p={p} eps={eps} {name}: rel err {e:.3e}")
        assert e < 2e-2, (name, e)
    assert not o["dh4"][:nb, :84][~m4].any() and not o["dh3"][:nb][~m3].any()
    assert o["stats"][2].item() == 0.0
    for k in ("h3", "h4", "logits", "dl", "dh4", "dh3", "dx"):    # rows past nb are untouched
        assert bool((o[k][nb:] == SENT).all()), f"mlp_head wrote {k} rows >= nb"


# ------------------------------------------------------------------ executors
def _opt(p, **kw):
    d = {} if p is None else {"dropout": p, "dropout_seed": SEED40}
    return OptConfig(**{**dict(lr0=0.05, decay_steps=0, use_momentum=False, ema_max=0.9999), **d, **kw})


def _batch(dev, n, cin=1, seed=21):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.rand(n, 28, 28, cin, generator=g) - 0.5).to(torch.bfloat16).to(dev)
    y = torch.randint(0, 10, (n,), generator=g, dtype=torch.int32).to(dev)
    return x, y


def _load(net, x, y):
    net.x0.copy_(x)
    net.labels.copy_(y)


def _grad_step(net):
    net.stats.zero_()
    net.forward(defer_head=True)
    net.loss_and_grad()
    net.backward()
    net.finalize(net.B, increment=False)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 4. fused == layered under the same masks
@pytest.mark.parametrize("B", [64, 300])
def test_fused_head_matches_layered_under_the_same_masks(dev, K, B):
    """tests/test_mlp_head_gpu.py::test_fused_head_matches_layered with dropout 0.5 on both nets, its
    bounds unchanged: 1e-2 on activations and dlogits, 2e-2 on data and parameter gradients."""
    p, t = 0.5, 3
    spec = get_model("lenet5", 1)
    init = torch_ref.init_params(spec, seed=B + 1)
    fused = HipNet(spec, B, dev, init, _opt(p))
    layered = HipNet(spec, B, dev, init, _opt(p), fuse_head=False)
    assert fused.head_kind == "mlp" and layered.head is None
    x, y = _batch(dev, B, seed=B)
    for net in (fused, layered):
        _load(net, x, y)
        net.fp.step.fill_(t)
        _grad_step(net)
    i = fused.head
    assert rel_err(fused.logits[:B, :10], layered.logits[:B, :10]) < 1e-2
    for j in (i, i + 1):
        a, b = fused.layers[j].out[:B], layered.layers[j].out[:B]
        assert rel_err(a, b) < 1e-2, j
        assert torch.all(a[:, fused.layers[j].spec.dout:] == 0)
        lay = fused.layers[j]
        m = _mask(SEED40, t, lay.idx, B, lay.spec.dout, p, dev)
        for net in (fused, layered):                       # no dropped unit survives on either path
            assert not net.layers[j].out[:B, :lay.spec.dout][~m].any()
    # h4's zero pattern equals the reference mask wherever the layered h4 is non-zero
    l4 = fused.layers[i + 1]
    m4 = _mask(SEED40, t, l4.idx, B, l4.spec.dout, p, dev)
    nz = layered.layers[i + 1].out[:B, :l4.spec.dout] != 0
    assert torch.equal((fused.layers[i + 1].out[:B, :l4.spec.dout] != 0)[nz], m4[nz])
    assert 0.3 < m4.float().mean().item() < 0.7 and bool(nz.any())
    assert rel_err(fused.dlogits[:B], layered.dlogits[:B]) < 1e-2
    for j in (i, i + 1, i + 2):
        e = rel_err(fused.dbuf[j][:B], layered.dbuf[j][:B])
        assert e < 2e-2, (j, e)
    for name in init:
        e = rel_err(fused.fp.grad_view(name), layered.fp.grad_view(name))
        assert e < 2e-2, (name, e)
    sf, sl = fused.stats.cpu(), layered.stats.cpu()
    assert abs(sf[4] - sl[4]) <= 1e-3 * abs(sl[4]) + 1e-3 / B
    assert sf[2] == 0


# ------------------------------------------------------------------ 5. gradients against the masked oracle
@pytest.mark.parametrize("model,B,fuse", [("lenet5", 200, True), ("lenet5", 200, False), ("mlp", 200, True),
                                          ("reference_cnn", 64, True)])
def test_executor_gradients_match_the_masked_oracle(dev, K, model, B, fuse):
    """forward(defer_head=True); loss_and_grad(); backward() under dropout 0.5 at step 7: every
    gradient against torch_ref given the host-reference multipliers (bf16-rounded weights), within
    max(3e-2, 3 x the bf16-autocast floor), the rule of test_fused_head_matches_oracle."""
    p, t = 0.5, 7
    spec = get_model(model, 1)
    init = torch_ref.init_params(spec, seed=1)
    net = HipNet(spec, B, dev, init, _opt(p), fuse_head=fuse)
    assert net.head_kind == ({"lenet5": "mlp", "reference_cnn": "tail", "mlp": None}[model] if fuse else None)
    x, y = _batch(dev, B)
    _load(net, x, y)
    net.fp.step.fill_(t)
    _grad_step(net)
    layers = D.dropout_layers(spec)
    assert len(layers) == (1 if model == "mlp" else 2)
    mult = {n: torch.from_numpy(D.multiplier(SEED40, t, i, B, spec.layers[i].dout, p)).to(dev)
            for n, i in layers.items()}
    prm = {k: v.to(dev).to(torch.bfloat16).float().requires_grad_(True) for k, v in init.items()}
    p16 = {k: v.detach().clone().requires_grad_(True) for k, v in prm.items()}
    lg, _ = torch_ref.forward(spec, prm, x.float(), dropout=mult)
    F.cross_entropy(lg, y.long()).backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        l16, _ = torch_ref.forward(spec, p16, x.float(), dropout=mult)
    F.cross_entropy(l16.float(), y.long()).backward()
    plain, _ = torch_ref.forward(spec, prm, x.float())
    assert rel_err(net.logits[:, :10], lg) < 3e-2
    print(f"{model}: dropped against plain logits: rel diff {rel_err(plain, lg):.3f}")
    assert rel_err(plain, lg) > 0.05, "the dropped and the plain logits must differ for this test to mean anything"
    for name in init:
        e = rel_err(net.fp.grad_view(name), prm[name].grad)
        floor = rel_err(p16[name].grad, prm[name].grad)
        print(f"{model} fuse={fuse} {name}: rel err {e:.3e} (bf16 floor {floor:.3e})")
        assert e < max(3e-2, 3.0 * floor), f"{name}: rel err {e:.3e} (bf16 floor {floor:.3e})"
    ce = F.cross_entropy(lg, y.long()).item()        # the training statistic: the loss of the dropped network
    assert abs(net.read_stats()["cross_entropy"] - ce) < 2e-2 * max(1.0, ce)


# ------------------------------------------------------------------ 6. rate 0 is bitwise the plain step
@pytest.mark.parametrize("fuse", [True, False])
def test_rate_zero_is_bitwise_the_net_without_the_key(dev, K, fuse):
    spec = get_model("lenet5", 1)
    init = torch_ref.init_params(spec, seed=2)
    out = []
    for p in (None, 0.0):
        net = HipNet(spec, 64, dev, init, _opt(p, use_momentum=True, momentum=0.9), fuse_head=fuse)
        for k in range(3):
            _load(net, *_batch(dev, 64, seed=40 + k))
            net.train_step()
        torch.cuda.synchronize()
        out.append((net.fp.params.clone(), net.fp.mom.clone(), net.stats.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 7. masks follow the step
@pytest.mark.parametrize("fuse", [True, False])
def test_masks_follow_the_device_step(dev, K, fuse):
    p, B = 0.5, 96
    spec = get_model("lenet5", 1)
    net = HipNet(spec, B, dev, torch_ref.init_params(spec, seed=4), _opt(p), fuse_head=fuse)
    _load(net, *_batch(dev, B, seed=5))
    l3 = net.layers[-3]
    pats = []
    for t in (0, 1):
        assert int(net.fp.step.item()) == t
        net.eval_batch(B, torch.zeros(8, device=dev))  # the undropped h3 of the current parameters
        alive = l3.out[:B].clone() > 0
        _grad_step(net)
        first = [v.clone() for v in (l3.out, net.layers[-2].out, net.logits, net.fp.grads, net.dbuf[-1])]
        _grad_step(net)                                # no update in between: identical outputs
        for a, b in zip(first, (l3.out, net.layers[-2].out, net.logits, net.fp.grads, net.dbuf[-1])):
            assert torch.equal(a, b)
        m = _mask(SEED40, t, l3.idx, B, 120, p, dev)
        assert torch.equal(l3.out[:B] != 0, alive & m)   # x 2 never flushes to zero: kept and past the ReLU
        pats.append(l3.out[:B] != 0)
        net.update()                                   # the optimizer increments the device step
        torch.cuda.synchronize()
    assert not torch.equal(pats[0], pats[1])
    assert not np.array_equal(D.keep_mask(SEED40, 0, l3.idx, B, 120, p), D.keep_mask(SEED40, 1, l3.idx, B, 120, p))


# ------------------------------------------------------------------ 8. hipGraph
@pytest.mark.parametrize("recipe", ["adam", "lamb_smooth"])
@pytest.mark.parametrize("model,fuse", [("lenet5", True), ("lenet5", False), ("reference_cnn", True)])
def test_graph_replay_equals_eager_bitwise(dev, K, model, fuse, recipe):
    """The step is read on the device: one eager warm-up plus 4 replays of the captured step are
    bitwise 5 eager steps (parameters, both slots, EMA, stats)."""
    from distributed_tensorflow_ibm_mnist_amd.runtime.graph import StepGraph
    if recipe == "adam":
        kw = dict(lr0=0.001, rule="adam", ema_max=0.9999, dropout=0.5, dropout_seed=SEED40)
    else:
        kw = dict(lr0=0.01, rule="lamb", ema_max=0.9999, label_smoothing=0.1, dropout=0.2, dropout_seed=SEED40)
    steps, B = 5, 64
    spec = get_model(model, 1)
    init = torch_ref.init_params(spec, seed=6)
    data = [_batch(dev, B, seed=60 + k) for k in range(steps)]
    out = []
    for graph in (False, True):
        net = HipNet(spec, B, dev, init, OptConfig(**kw), fuse_head=fuse)
        sg = None
        for k in range(steps):
            _load(net, *data[k])
            if not graph:
                net.train_step()
            elif sg is None:
                sg = StepGraph(net.train_step, warmup=1)    # the warm-up is step 0; capture executes nothing
            else:
                sg.replay()
        torch.cuda.synchronize()
        assert int(net.fp.step.item()) == steps
        out.append([t.clone() for t in (net.fp.params, net.fp.mom, net.fp.slot2, net.fp.ema, net.stats)])
        # the last step's masks are those of t = steps - 1
        lay = net.layers[-2]
        m = _mask(SEED40, steps - 1, lay.idx, B, lay.spec.dout, kw["dropout"], dev)
        assert not lay.out[:B, :lay.spec.dout][~m].any()
    for a, b, name in zip(out[0], out[1], ("params", "slot 1", "slot 2", "ema", "stats")):
        assert torch.equal(a, b), name
    assert out[0][4][2].item() == 0.0


# ------------------------------------------------------------------ 9. eval paths unchanged
@pytest.mark.parametrize("model,fuse", [("lenet5", True), ("lenet5", False), ("reference_cnn", True), ("mlp", True)])
def test_eval_paths_ignore_the_rate(dev, K, model, fuse):
    B = 64
    spec = get_model(model, 1)
    init = torch_ref.init_params(spec, seed=8)
    x, y = _batch(dev, B, seed=9)
    res = []
    for p in (0.0, 0.5):
        net = HipNet(spec, B, dev, init, _opt(p), fuse_head=fuse)
        _load(net, x, y)
        _grad_step(net)                                # a training pass first: eval must not inherit its state
        st = torch.zeros(8, device=dev)
        net.eval_batch(B, st)
        logits = net.logits.clone()
        pr = net.probs(B).clone()
        acts = [l.out.clone() for l in net.layers]
        torch.cuda.synchronize()
        res.append((st.clone(), logits, pr, acts))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    for a, b in zip(res[0][3], res[1][3]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 10. refusals
def test_bindings_refuse_invalid_arguments(dev, K):
    x = torch.zeros(8, 16, dtype=torch.bfloat16, device=dev)
    st = _step_t(dev, 0)
    ok = dict(nb=8, n=16, ld=16, step=st, seed=1, layer=0, p=0.5)
    K.dropout_fwd(x, **ok)
    for key, bad in (("p", 1.0), ("p", -0.1), ("p", float("nan")), ("p", float("inf")), ("seed", -1),
                     ("layer", 65536), ("layer", -1), ("n", 524289), ("nb", 1 << 31), ("ld", 12), ("n", 17)):
        for fn in (K.dropout_fwd, K.dropout_bwd):
            with pytest.raises(ValueError):
                fn(x, **{**ok, key: bad})
    out = torch.zeros(8, 16, dtype=torch.uint8, device=dev)
    for key, bad in (("p", 1.0), ("seed", -1), ("layer", 65536), ("n", 524289), ("nb", 1 << 31)):
        with pytest.raises(ValueError):
            K.dropout_mask(out, **{**dict(nb=8, n=16, step=st, seed=1, layer=0, p=0.5), key: bad})
    # every buffer is validated before the launch: too small, wrong dtype, wrong device, misaligned
    with pytest.raises(RuntimeError, match="needs"):
        K.dropout_fwd(x, **{**ok, "nb": 9})
    with pytest.raises(RuntimeError, match="dtype"):
        K.dropout_fwd(x.float(), **ok)
    with pytest.raises(RuntimeError, match="dtype"):
        K.dropout_fwd(x, **{**ok, "step": st.int()})
    with pytest.raises(RuntimeError, match="GPU"):
        K.dropout_fwd(x, **{**ok, "step": st.cpu()})
    with pytest.raises(RuntimeError, match="aligned"):
        K.dropout_fwd(torch.zeros(8 * 16 + 8, dtype=torch.bfloat16, device=dev)[4:], **ok)
    with pytest.raises(RuntimeError, match="needs"):
        K.dropout_mask(out, 9, 16, st, 1, 0, 0.5)
    # the fused head: the rate and the ids as above, and the gradient form only
    inputs = _head_inputs(dev, 32, 1)
    for kw in (dict(dropout=1.0), dict(dropout=0.5), dict(dropout=0.5, drop_step=st, drop_seed=-1),
               dict(dropout=0.5, drop_step=st, drop_layer3=65536), dict(dropout=0.5, drop_step=st, drop_layer4=65536)):
        with pytest.raises(ValueError, match="dropout"):
            _run_head(K, dev, inputs, 32, **kw)
    bf = dict(dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="dropout is a training quantity"):
        K.mlp_head(inputs["x"], _tr(inputs["w3"], 128, 416), inputs["b3"], 120, _tr(inputs["w4"], 96, 128),
                   inputs["b4"], 84, _tr(inputs["w5"], 16, 96), inputs["b5"], 10, inputs["y"], 32, 1.0,
                   torch.zeros(32, 120, **bf), torch.zeros(32, 88, **bf), torch.zeros(32, 16, device=dev),
                   stats=torch.zeros(8, device=dev), work=torch.zeros(4097, device=dev), dropout=0.5, drop_step=st)


def test_fp32_executor_refuses_dropout(dev, K):
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor_f32 import HipNetF32
    spec = get_model("lenet5", 1)
    with pytest.raises(ValueError, match="dropout"):
        HipNetF32(spec, 32, dev, torch_ref.init_params(spec, seed=0), _opt(0.5))
    HipNetF32(spec, 32, dev, torch_ref.init_params(spec, seed=0), _opt(0.0))


@pytest.mark.parametrize("job", ["ps", "worker"])
def test_ps_mode_refuses_dropout_at_start_up(job):
    """--job_name=ps|worker with dropout > 0: one line and exit code 2, before torch is imported or a
    socket opened (a fresh child process running the CLI)."""
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), f"--job_name={job}", "--ps_hosts=localhost:1",
                        "--worker_hosts=localhost:2", "--dropout=0.5"], cwd=ROOT, capture_output=True, text=True,
                       timeout=60, env=dict(os.environ, PYTHONUNBUFFERED="1"))
    dt = time.time() - t0
    out = r.stdout + r.stderr
    assert r.returncode == 2, out[-2000:]
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1 and "dropout" in lines[0] and "parameter-server mode" in lines[0], out[-2000:]
    assert "Traceback" not in out and dt < 5.0, (dt, out[-2000:])


# ------------------------------------------------------------------ 11. the module
def test_module_forward_backward_and_eval(dev, K):
    from distributed_tensorflow_ibm_mnist_amd.ops.nn import Dropout
    p, seed, layer, rows, n = 0.2, 99, 2, 37, 120
    thr, inv = D.threshold(p)
    mod = Dropout(p, seed, layer).to(dev)
    torch.manual_seed(3)
    for t in range(2):                                  # its own device step, one per training forward
        assert int(mod.step.item()) == t
        x = torch.randn(rows, n, device=dev).to(torch.bfloat16).requires_grad_(True)
        y = mod(x)
        dy = torch.randn(rows, n, device=dev).to(torch.bfloat16)
        y.backward(dy)
        m = _mask(seed, t, layer, rows, n, p, dev)
        assert torch.equal(y.detach(), _standalone_ref(x.detach(), m, inv))
        assert torch.equal(x.grad, _standalone_ref(dy, m, inv))
    assert int(mod.step.item()) == 2
    mod.eval()
    x = torch.randn(rows, n, device=dev).to(torch.bfloat16)
    assert mod(x) is x and int(mod.step.item()) == 2    # the identity, and no step
    with pytest.raises(ValueError, match="p"):
        Dropout(1.0)
    with pytest.raises(ValueError, match="multiple of 8"):
        Dropout(0.5).to(dev).train()(torch.zeros(4, 12, device=dev))
