"""Label smoothing, CPU side: the parameter manager's ``label_smoothing`` key and getter,
``OptConfig.label_smoothing``, the plain-torch net against a hand-written torch loop, and the
training CLI: its training ``cross_entropy`` scalar is the smoothed loss (float64 oracle,
tests/label_smoothing_oracle.py), its test-split loss line the plain one."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("label_smoothing_oracle",
                                               os.path.join(ROOT, "tests", "label_smoothing_oracle.py"))
lso = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lso)


@pytest.fixture
def pm():
    from distributed_tensorflow_ibm_mnist_amd.utils import parameter_mgr
    yield parameter_mgr
    parameter_mgr.configure({})


# ------------------------------------------------------------------ the oracle against torch
def test_oracle_equals_torch_float64():
    """The formulas of the oracle are torch's label_smoothing, loss and gradient, in float64."""
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(50, 10, generator=g, dtype=torch.float64) * 4).requires_grad_(True)
    y = torch.randint(0, 10, (50,), generator=g)
    for eps in (0.0, 0.1, 0.5):
        z.grad = None
        loss = F.cross_entropy(z, y, reduction="sum", label_smoothing=eps)
        (loss * 0.02).backward()
        assert abs(lso.ce_sum(z, y, eps) - loss.item()) <= 1e-12 * abs(loss.item())
        assert np.abs(lso.dlogits(z, y, 0.02, eps) - z.grad.numpy()).max() <= 1e-15


# ------------------------------------------------------------------ 13. key, flag, getter
def test_key_flag_and_getter_round_trip(pm, tmp_path):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    assert "label_smoothing" in pm.FLAG_KEYS and "label_smoothing" in pm.DEFAULTS
    pm.configure({})
    assert pm.getLabelSmoothing() == 0.0 and OptConfig().label_smoothing == 0.0
    assert pm.getOptimizer(0.1) == pm.OptimizerSpec("sgd", 0.1, 0.0, False)       # the spec does not carry it
    pm.configure({"label_smoothing": 0.1})
    assert pm.getLabelSmoothing() == 0.1
    assert pm.getOptimizer(0.1) == pm.OptimizerSpec("sgd", 0.1, 0.0, False)
    y = tmp_path / "p.yaml"
    y.write_text("optimizer: lamb\nlabel_smoothing: 0.2\n")
    pm.configure(str(y))
    assert pm.getLabelSmoothing() == 0.2
    pm.configure(str(y), label_smoothing=0.3)                                      # a keyword override wins
    assert pm.getLabelSmoothing() == 0.3
    c = OptConfig.from_spec(pm.getOptimizer(0.01), 100, 0.1, label_smoothing=pm.getLabelSmoothing())
    assert (c.rule, c.label_smoothing) == ("lamb", 0.3)
    assert OptConfig.from_spec(pm.getOptimizer(0.01), 100, 0.1).label_smoothing == 0.0

    class Flags:        # the CLI: -1 is "unset", 0.0 a value
        config, label_smoothing = str(y), -1
    pm.configure_from_flags(Flags)
    assert pm.getLabelSmoothing() == 0.2
    Flags.label_smoothing = 0.0
    pm.configure_from_flags(Flags)
    assert pm.getLabelSmoothing() == 0.0
    pm.configure(os.path.join(ROOT, "configs", "lenet5_lamb_smooth.yaml"))        # the example config loads
    assert pm.getLabelSmoothing() == 0.1 and pm.getOptimizer(0.03).name == "lamb"


@pytest.mark.parametrize("bad", [1.0, -0.1, float("nan"), "x", 1.5, float("inf")])
def test_invalid_values_raise_value_error_naming_the_key(pm, bad):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    pm.configure({"label_smoothing": bad})
    with pytest.raises(ValueError, match="label_smoothing") as e:
        pm.getLabelSmoothing()
    assert str(bad) in str(e.value) or repr(bad) in str(e.value)
    with pytest.raises(ValueError, match="label_smoothing") as e:
        OptConfig(label_smoothing=bad)
    assert str(bad) in str(e.value) or repr(bad) in str(e.value)


# ------------------------------------------------------------------ 14. TorchNet
def _torchnet(eps, B=32):
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import TorchNet
    spec = get_model("mlp", 1)
    init = torch_ref.init_params(spec, seed=3)
    kw = {} if eps is None else {"label_smoothing": eps}
    return spec, init, TorchNet(spec, B, "cpu", init, OptConfig(lr0=0.1, ema_max=0.9999, **kw))


def _batches(B=32, steps=5):
    g = torch.Generator().manual_seed(14)
    return [(torch.rand(B, 28, 28, 1, generator=g) - 0.5, torch.randint(0, 10, (B,), generator=g, dtype=torch.int32))
            for _ in range(steps)]


def test_torchnet_matches_hand_written_loop():
    """5 SGD steps of TorchNet(mlp, B = 32) with label_smoothing=0.1 == a hand-written torch loop
    w <- w - lr * (grad of F.cross_entropy(label_smoothing=0.1) + wd w); the cross_entropy
    statistic is the smoothed loss (float64 oracle), eval_batch the plain one."""
    from distributed_tensorflow_ibm_mnist_amd.models import torch_ref
    eps, lr = 0.1, 0.1
    spec, init, net = _torchnet(eps)
    p = {k: v.clone().float().requires_grad_(True) for k, v in init.items()}
    wd = {f"{L.name}/weights": float(L.wd or 0.0) for L in spec.weights()}
    for x, y in _batches():
        net.x0.copy_(x)
        net.labels.copy_(y)
        net.train_step()
        logits, _ = torch_ref.forward(spec, p, x)
        loss = F.cross_entropy(logits, y.long(), label_smoothing=eps)
        grads = torch.autograd.grad(loss, list(p.values()))
        ce = lso.ce_sum(logits, y, eps) / len(y)
        assert abs(net.read_stats()["cross_entropy"] - ce) <= 1e-5 * max(1.0, ce)
        with torch.no_grad():
            for (k, v), g in zip(p.items(), grads):
                v -= lr * (g + wd.get(k, 0.0) * v)
    for k, v in p.items():
        assert torch.allclose(net.fp.param_view(k), v.detach(), rtol=1e-5, atol=1e-7), k
    x, y = _batches()[0]
    net.x0.copy_(x)
    net.labels.copy_(y)
    st = net.eval_batch(32, torch.zeros(8))
    lso.check_ce(st[0].item(), lso.ce_sum(net.forward(32, grad=False), y, 0.0), "eval_batch")


def test_torchnet_zero_smoothing_is_bitwise_the_default():
    _, _, a = _torchnet(None)
    _, _, b = _torchnet(0.0)
    for x, y in _batches():
        for n in (a, b):
            n.x0.copy_(x)
            n.labels.copy_(y)
            n.train_step()
    assert torch.equal(a.fp.params, b.fp.params) and torch.equal(a.stats, b.stats)


def test_torch_ref_losses_take_label_smoothing():
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    spec = get_model("mlp", 1)
    p = torch_ref.init_params(spec, seed=0)
    x, y = _batches()[0]
    logits, _ = torch_ref.forward(spec, p, x)
    plain, smooth = torch_ref.losses(spec, p, logits, y), torch_ref.losses(spec, p, logits, y, label_smoothing=0.1)
    assert abs(plain["cross_entropy"].item() - lso.ce_sum(logits, y, 0.0) / 32) <= 1e-5
    assert abs(smooth["cross_entropy"].item() - lso.ce_sum(logits, y, 0.1) / 32) <= 1e-5


# ------------------------------------------------------------------ 15. the CLI
COMMON = ["--impl=torch", "--cpu", "--model=mlp", "--in_channels=1", "--batch_size=32", "--test_interval=10",
          "--log_step_count_steps=0", "--train_data=synthetic://1500", "--test_data=synthetic://300?seed=1",
          "--eval_examples=300", "--base_lr=0.05", "--optimizer=momentum", "--max_steps=20",
          "--save_summaries_steps=1"]


def run_main(args, timeout=300):
    e = dict(os.environ, OMP_NUM_THREADS="2", PYTHONUNBUFFERED="1")
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, env=e,
                          capture_output=True, text=True, timeout=timeout)


def scalars(d, key):
    from distributed_tensorflow_ibm_mnist_amd.obs.events import find_event_files, read_events
    out = {}
    for f in find_event_files(d):
        for ev in read_events(f):
            if key in ev["values"]:
                out[ev["step"]] = ev["values"][key]
    return out


def test_cli_trains_on_the_smoothed_loss_and_evaluates_the_plain_one(tmp_path):
    """main.py --label_smoothing=0.1: the events file's training cross_entropy of the first step
    is the float64 smoothed loss of the first batch (rebuilt here with the trainer's own loader
    and initial weights); the 'test loss' line after the last step is the plain cross-entropy
    of the test split under the checkpointed weights, not the smoothed one."""
    from distributed_tensorflow_ibm_mnist_amd.ckpt.saver import Saver
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica, load_state
    from distributed_tensorflow_ibm_mnist_amd.train.trainer import load_data
    eps = 0.1
    d = str(tmp_path / "smooth")
    r = run_main(COMMON + [f"--label_smoothing={eps}", f"--train_dir={d}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    ce = scalars(d, "cross_entropy")
    assert sorted(ce) == list(range(1, 21)), sorted(ce)
    spec = get_model("mlp", 1)
    x_tr, y_tr, c = load_data(["synthetic://1500"], 1)
    x_ev, y_ev, _ = load_data(["synthetic://300?seed=1"], 1)
    rep = Replica(spec, "torch", 32, "cpu", torch_ref.init_params(spec, seed=0), OptConfig(), x_tr, y_tr, c,
                  x_ev, y_ev, seed=0)
    rep.loader.next()
    logits = rep.net.forward(grad=False)
    want = lso.ce_sum(logits, rep.net.labels, eps) / 32
    plain = lso.ce_sum(logits, rep.net.labels, 0.0) / 32
    print(f"first step: cross_entropy {ce[1]!r}, float64 smoothed {want!r}, plain {plain!r}")
    tol = 1e-5 * max(1.0, want)
    assert abs(ce[1] - want) <= tol
    assert abs(want - plain) > 4 * tol       # near-zero initial logits: the two losses are close, yet apart
    # the test-split line after step 20 against the checkpoint of step 20
    m = re.findall(r"step 20: test loss ([0-9.]+)", r.stdout)
    assert len(m) == 1, r.stdout[-2000:]
    load_state(rep.net, Saver.restore(os.path.join(d, "model.ckpt-20")), strict=False)
    lg, lab = [], []
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import eval_batches
    for nb in eval_batches(rep.eval_ds, rep.net.x0, rep.net.labels):
        lg.append(rep.net.forward(nb, grad=False)[:nb].clone())
        lab.append(rep.net.labels[:nb].clone())
    lg, lab = torch.cat(lg), torch.cat(lab)
    assert len(lab) == 300
    t_plain, t_smooth = lso.ce_sum(lg, lab, 0.0) / 300, lso.ce_sum(lg, lab, eps) / 300
    print(f"test loss line {m[0]}, float64 plain {t_plain!r}, smoothed {t_smooth!r}")
    tol = 1e-4 + 1e-5 * t_plain              # the line prints four decimals
    assert abs(float(m[0]) - t_plain) <= tol
    assert abs(t_smooth - t_plain) > 10 * tol
    assert rep.evaluate(300)["loss"] == pytest.approx(t_plain, rel=1e-5)


def test_cli_rejects_an_invalid_value(tmp_path):
    r = run_main(COMMON + ["--label_smoothing=1.0", f"--train_dir={tmp_path / 'bad'}"], timeout=120)
    assert r.returncode != 0
    assert "label_smoothing" in (r.stdout + r.stderr) and "1.0" in (r.stdout + r.stderr)
