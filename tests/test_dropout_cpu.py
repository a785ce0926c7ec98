"""Dropout, CPU side: the host reference of the counter-based masks (``ops/dropout.py``: Philox4x32-10
known answers, keep fraction, independence across keys), validation of the ``dropout`` /
``dropout_seed`` keys, and the plain-torch net, whose training step applies the reference masks."""
import math
import os

import numpy as np
import pytest
import torch

from distributed_tensorflow_ibm_mnist_amd.ops import dropout as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, T, L = 1234, 7, 3


@pytest.fixture
def pm():
    from distributed_tensorflow_ibm_mnist_amd.utils import parameter_mgr
    yield parameter_mgr
    parameter_mgr.configure({})


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


# ------------------------------------------------------------------ 1. known answers
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    """Philox4x32-10 with the Random123 constants: its published known-answer vectors."""
    assert _hex(D.philox4x32_10(counter, key)) == want


def test_keep_bits_known_rows():
    """The two 16-feature rows the issue fixes (seed 1234, t 7, L 3, p 0.5)."""
    assert D.keep_mask(SEED, T, L, 1, 16, 0.5)[0].astype(int).tolist() == [1, 0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1]
    m = D.keep_mask(SEED, T, L, 256, 120, 0.5)
    assert m[255, 104:120].astype(int).tolist() == [0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0]
    # a mask is a function of (row, feature) alone: fewer rows / features are a prefix
    assert np.array_equal(m[:33, :84], D.keep_mask(SEED, T, L, 33, 84, 0.5))


def test_draw_layout_matches_the_counter_definition():
    """draw(f) = (w[(f & 7) >> 1] >> (16 * (f & 1))) & 0xffff of counter (t lo, t hi, m, (L << 16) | f >> 3)."""
    t, seed = (1 << 32) + 5, (0xAB << 32) | 0x1234567
    d = D.draws(seed, t, L, 3, 20)
    for m, f in ((0, 0), (2, 7), (1, 8), (2, 19)):
        w = D.philox4x32_10((t & 0xFFFFFFFF, t >> 32, m, (L << 16) | (f >> 3)), (seed & 0xFFFFFFFF, seed >> 32))
        assert int(d[m, f]) == (int(w[(f & 7) >> 1]) >> (16 * (f & 1))) & 0xFFFF


# ------------------------------------------------------------------ 2. keep fraction
@pytest.mark.parametrize("n", [84, 120])
@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_keep_fraction_within_five_sigma(n, p):
    rows = 256
    thr, _ = D.threshold(p)
    q = thr / 65536.0
    frac = D.keep_mask(SEED, T, L, rows, n, p).mean()
    sigma = math.sqrt(q * (1 - q) / (rows * n))
    print(f"n={n} p={p}: keep fraction {frac:.5f}, expected {q:.5f}, {abs(frac - q) / sigma:.2f} sigma")
    assert abs(frac - q) <= 5 * sigma


# ------------------------------------------------------------------ 3. independence across keys
@pytest.mark.parametrize("what", ["t+1", "t+2^32", "L+1", "seed+1"])
def test_masks_of_neighbouring_keys_agree_on_half_the_bits(what):
    rows, n = 256, 120
    base = D.keep_mask(SEED, T, L, rows, n, 0.5)
    other = {"t+1": (SEED, T + 1, L), "t+2^32": (SEED, T + (1 << 32), L), "L+1": (SEED, T, L + 1),
             "seed+1": (SEED + 1, T, L)}[what]
    agree = (base == D.keep_mask(*other, rows, n, 0.5)).mean()
    sigma = 0.5 / math.sqrt(rows * n)
    print(f"{what}: agreement {agree:.5f}, {abs(agree - 0.5) / sigma:.2f} sigma on {rows * n} bits")
    assert abs(agree - 0.5) <= 5 * sigma


# ------------------------------------------------------------------ 4. validation
@pytest.mark.parametrize("bad", [1.0, -0.1, float("nan"), "x", 1.5, float("inf"), True, None])
def test_invalid_rates_raise_value_error_naming_key_and_value(pm, bad):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    for call in (lambda: D.threshold(bad), lambda: OptConfig(dropout=bad), lambda: D.keep_mask(0, 0, 0, 1, 8, bad)):
        with pytest.raises(ValueError, match="dropout") as e:
            call()
        assert str(bad) in str(e.value) or repr(bad) in str(e.value)
    if bad is not None:                       # (None in a config is "unset": the default)
        pm.configure({"dropout": bad})
        with pytest.raises(ValueError, match="dropout") as e:
            pm.getDropout()
        assert str(bad) in str(e.value) or repr(bad) in str(e.value)


@pytest.mark.parametrize("bad", [-1, 1 << 63, 1.5, "7", True])
def test_invalid_seeds_raise_value_error(pm, bad):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    with pytest.raises(ValueError, match="dropout_seed"):
        OptConfig(dropout=0.5, dropout_seed=bad)
    pm.configure({"dropout_seed": bad})
    with pytest.raises(ValueError, match="dropout_seed"):
        pm.getDropoutSeed(0)


def test_threshold_is_clamped_and_inv_keep_is_the_exact_reciprocal():
    assert D.threshold(0.0) == (65535, float(np.float32(65536.0 / 65535.0)))     # clamped from 65536
    assert D.threshold(0.99999999)[0] == 1                                        # clamped from 0
    assert D.threshold(0.5) == (32768, 2.0) and D.threshold(0.75) == (16384, 4.0)
    for p in (0.5, 0.75, 0.875):                 # powers of two: inv_keep * thr == 65536 exactly
        thr, inv = D.threshold(p)
        assert inv * thr == 65536.0
    # Otherwise 65536 / thr is no binary fraction, so no float32 inv_keep gives inv_keep * thr == 65536
    # in float64 (p = 0.2: 65535.999999046; p = 0.1: 65536.0016).  What can hold, and is asserted: it
    # is the float32 NEAREST to the reciprocal -- both float32 neighbours are farther from it -- and
    # so within half an ulp (2^-24 relative).
    for p in (0.1, 0.2, 0.5):
        thr, inv = D.threshold(p)
        assert thr == math.floor((1 - p) * 65536 + 0.5)
        assert inv == float(np.float32(65536.0 / thr))
        err = abs(inv * thr - 65536.0)
        for nb in (np.nextafter(np.float32(inv), np.float32(0)), np.nextafter(np.float32(inv), np.float32(4))):
            assert err <= abs(float(nb) * thr - 65536.0)
        assert err <= 65536.0 * 2.0 ** -24
        assert abs(thr / 65536.0 - (1 - p)) <= 2.0 ** -17                      # the documented quantisation


def test_key_flag_and_getter_round_trip(pm):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    assert {"dropout", "dropout_seed"} <= set(pm.FLAG_KEYS) and {"dropout", "dropout_seed"} <= set(pm.DEFAULTS)
    pm.configure({})
    assert pm.getDropout() == 0.0 and pm.getDropoutSeed(11) == 11 and OptConfig().dropout == 0.0
    pm.configure({"dropout": 0.25, "dropout_seed": 1 << 40})
    assert pm.getDropout() == 0.25 and pm.getDropoutSeed(11) == 1 << 40
    c = OptConfig.from_spec(pm.getOptimizer(0.01), 100, 0.1, dropout=pm.getDropout(), dropout_seed=pm.getDropoutSeed(0))
    assert (c.dropout, c.dropout_seed) == (0.25, 1 << 40)

    class Flags:        # the CLI: -1 is "unset", 0.0 a value
        config, dropout, dropout_seed = os.path.join(ROOT, "configs", "lenet5_dropout.yaml"), -1, -1
    pm.configure_from_flags(Flags)
    assert pm.getDropout() == 0.5 and pm.getDropoutSeed(3) == 3 and pm.getOptimizer(0.001).name == "adam"
    Flags.dropout, Flags.dropout_seed = 0.0, 9
    pm.configure_from_flags(Flags)
    assert pm.getDropout() == 0.0 and pm.getDropoutSeed(3) == 9


def test_ps_mode_refuses_dropout_at_start_up(pm):
    lines = []
    pm.configure({"dropout": 0.5})
    for job in ("ps", "worker"):
        with pytest.raises(SystemExit):
            pm.check_ps_dropout(job, lines.append)
    assert len(lines) == 2 and all("dropout" in ln and "parameter-server" in ln for ln in lines)
    pm.check_ps_dropout("", lines.append)               # single-process / data parallel: fine
    pm.configure({})
    pm.check_ps_dropout("worker", lines.append)         # rate 0: fine
    assert len(lines) == 2


def test_dropout_layers_are_the_hidden_relu_dense_layers():
    from distributed_tensorflow_ibm_mnist_amd.models import get_model
    assert list(D.dropout_layers(get_model("lenet5", 1))) == ["fc3", "fc4"]
    assert list(D.dropout_layers(get_model("reference_cnn", 1))) == ["local3", "local4"]
    assert list(D.dropout_layers(get_model("mlp", 1))) == ["hidden"]
    for name in ("lenet5", "reference_cnn", "mlp"):
        spec = get_model(name, 1)
        assert all(spec.layers[i].name == n for n, i in D.dropout_layers(spec).items())


# ------------------------------------------------------------------ 5. TorchNet
def _torchnet(p, B=32, seed=77):
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import TorchNet
    spec = get_model("mlp", 1)
    init = torch_ref.init_params(spec, seed=3)
    kw = {} if p is None else {"dropout": p, "dropout_seed": seed}
    return spec, init, TorchNet(spec, B, "cpu", init, OptConfig(lr0=0.1, ema_max=0.9999, **kw))


def _batch(B=32):
    g = torch.Generator().manual_seed(14)
    return torch.rand(B, 28, 28, 1, generator=g) - 0.5, torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)


def test_torchnet_step_matches_torch_ref_with_the_reference_masks():
    """Two CPU training steps at p = 0.5: the gradient of each equals autograd through
    torch_ref.forward(dropout=reference multipliers at that step), and differs from the undropped one."""
    from distributed_tensorflow_ibm_mnist_amd.models import torch_ref
    B, seed = 32, 77
    spec, _, net = _torchnet(0.5, B, seed)
    x, y = _batch(B)
    net.x0.copy_(x)
    net.labels.copy_(y)
    layers = D.dropout_layers(spec)
    assert list(layers) == ["hidden"]
    for t in range(2):
        assert int(net.fp.step.item()) == t
        params = {e.name: net.fp.params[e.off:e.off + e.n].view(e.shape).clone().requires_grad_(True)
                  for e in net.fp.entries}
        net.forward()
        net.loss_and_grad()
        net.backward()
        mult = {n: torch.from_numpy(D.multiplier(seed, t, i, B, spec.layers[i].dout, 0.5)) for n, i in layers.items()}
        logits, _ = torch_ref.forward(spec, params, x, dropout=mult)
        loss = torch.nn.functional.cross_entropy(logits, y.long())
        grads = torch.autograd.grad(loss, list(params.values()))
        plain = torch.autograd.grad(torch.nn.functional.cross_entropy(torch_ref.forward(spec, params, x)[0], y.long()),
                                    list(params.values()))
        for e, g, g0 in zip(net.fp.entries, grads, plain):
            got = net.fp.grads[e.off:e.off + e.n].view(e.shape)
            assert torch.allclose(got, g, rtol=1e-5, atol=1e-7), e.name
            assert not torch.allclose(got, g0, rtol=1e-3, atol=1e-5), e.name
        net.update()
    # the multipliers: 0 or inv_keep = 2, about half each
    m = mult["hidden"]
    assert set(m.unique().tolist()) == {0.0, 2.0}


def test_torchnet_rate_zero_is_bitwise_the_net_without_the_key_and_eval_ignores_the_rate():
    x, y = _batch()
    nets = [_torchnet(p)[2] for p in (None, 0.0, 0.5)]
    for net in nets:
        net.x0.copy_(x)
        net.labels.copy_(y)
    ev = [net.eval_batch(32).clone() for net in nets]
    pr = [net.probs(32) for net in nets]
    assert torch.equal(ev[0], ev[2]) and torch.equal(pr[0], pr[2])       # eval is unchanged by p
    for net in nets:
        for _ in range(3):
            net.train_step()
    assert torch.equal(nets[0].fp.params, nets[1].fp.params) and torch.equal(nets[0].stats, nets[1].stats)
    assert not torch.equal(nets[0].fp.params, nets[2].fp.params)
