"""Adam / RMSProp / Adagrad, CPU side: the parameter manager's getOptimizer, the plain-torch
update against a float64 oracle, the checkpoint's TF1 slot names with a bitwise resume, and the
parameter-server refusal."""
import importlib.util
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("adaptive_oracle", os.path.join(ROOT, "tests", "adaptive_oracle.py"))
oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(oracle)

RULES = ["adam", "rmsprop", "adagrad"]


# ------------------------------------------------------------------ 1. getOptimizer
@pytest.fixture
def pm():
    from distributed_tensorflow_ibm_mnist_amd.utils import parameter_mgr
    yield parameter_mgr
    parameter_mgr.configure({})


def test_get_optimizer_defaults(pm):
    pm.configure({"optimizer": "Adam"})
    o = pm.getOptimizer(0.001)
    assert (o.name, o.learning_rate, o.beta1, o.beta2, o.epsilon) == ("adam", 0.001, 0.9, 0.999, None)
    pm.configure({"optimizer": "RMSProp"})
    o = pm.getOptimizer(0.01)
    # the manager's general momentum default (0.9) does not leak into RMSProp
    assert (o.name, o.rmsprop_decay, o.momentum, o.epsilon) == ("rmsprop", 0.9, 0.0, None)
    pm.configure({"optimizer": "ADAGRAD"})
    o = pm.getOptimizer(0.01)
    assert (o.name, o.adagrad_initial_accumulator) == ("adagrad", 0.1)
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    assert OptConfig(rule="adam").eps == 1e-8 and OptConfig(rule="rmsprop").eps == 1e-10
    pm.configure({"optimizer": "rmsprop"})
    c = OptConfig.from_spec(pm.getOptimizer(0.01), 100, 0.1)
    assert (c.rule, c.momentum, c.use_momentum, c.rmsprop_decay, c.slot_init()) == ("rmsprop", 0.0, False, 0.9, (0.0, 1.0))
    assert c.slot_names() == ("RMSProp_1", "RMSProp")


def test_get_optimizer_overrides_yaml_and_env(pm, tmp_path, monkeypatch):
    y = tmp_path / "p.yaml"
    y.write_text("optimizer: adam\nbeta1: 0.8\nbeta2: 0.99\nepsilon: 1.0e-6\n")
    pm.configure(str(y))
    o = pm.getOptimizer(0.5)
    assert (o.name, o.beta1, o.beta2, o.epsilon) == ("adam", 0.8, 0.99, 1e-6)
    y2 = tmp_path / "q.yaml"
    y2.write_text("optimizer: rmsprop\nrmsprop_decay: 0.95\nmomentum: 0.5\nepsilon: 1.0e-7\n")
    monkeypatch.setenv("MNISTX_PARAMS", str(y2))
    pm.configure()
    o = pm.getOptimizer(0.5)
    assert (o.name, o.rmsprop_decay, o.momentum, o.epsilon) == ("rmsprop", 0.95, 0.5, 1e-7)
    y3 = tmp_path / "r.yaml"
    y3.write_text("optimizer: adagrad\nadagrad_initial_accumulator: 0.5\n")
    monkeypatch.setenv("MNISTX_PARAMS", str(y3))
    pm.configure()
    assert pm.getOptimizer(0.5).adagrad_initial_accumulator == 0.5
    # a keyword override wins over the file
    pm.configure(str(y), beta1=0.7)
    assert pm.getOptimizer(0.5).beta1 == 0.7


def test_get_optimizer_unknown_name_raises(pm):
    pm.configure({"optimizer": "adadelta"})
    with pytest.raises(ValueError, match=r"sgd\|momentum\|nesterov\|adam\|rmsprop\|adagrad"):
        pm.getOptimizer(0.1)


# ------------------------------------------------------------------ 2. torch_update vs the float64 oracle
SHAPES = [("a/weights", (5, 5, 1, 7), 0.0), ("a/biases", (7,), None), ("b/weights", (40, 33), 0.004),
          ("b/biases", (33,), None)]
ZERO_GRAD = "b/biases"     # its gradient is zero on every step; no weight decay


@pytest.mark.parametrize("rule", RULES)
def test_torch_update_matches_float64_oracle(rule):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import FlatParams, OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import torch_update
    torch.manual_seed(20)
    init = {n: torch.randn(*s) for n, s, _ in SHAPES}
    fp = FlatParams.build(SHAPES, init, "cpu", pads={})
    cfg = OptConfig(lr0=0.05, decay_rate=0.5, decay_steps=3, ema_max=0.9999, rule=rule)   # the LR halves at step 3
    fp.init_slots(cfg)
    ref = oracle.Oracle(rule, {n: v.numpy() for n, v in init.items()}, {n: wd for n, _, wd in SHAPES},
                        0.05, 0.5, 3, 0.9999, grad_scale=0.5)
    for _ in range(6):
        g = {n: torch.randn_like(init[n]) for n in init}
        g[ZERO_GRAD].zero_()
        for n in g:
            fp.grad_view(n).copy_(g[n])
        torch_update(fp, cfg, grad_scale=0.5)
        fp.step += 1
        ref.step({n: v.numpy() for n, v in g.items()})
    assert ref.lr() == 0.0125     # steps 0-2 ran at 0.05, steps 3-5 at 0.025
    for n in init:
        s1, s2 = fp.slot_views(n)
        oracle.close(fp.param_view(n).numpy(), ref.p[n])
        oracle.close(fp.ema_view(n).numpy(), ref.ema[n])
        oracle.close(s1.numpy(), ref.s1[n])
        if rule == "adagrad":
            assert s2 is None
        else:
            oracle.close(s2.numpy(), ref.s2[n])
    # a gradient that was always zero: finite and unchanged
    assert torch.isfinite(fp.params).all()
    assert torch.equal(fp.param_view(ZERO_GRAD), init[ZERO_GRAD])


# ------------------------------------------------------------------ 3. CLI: checkpoint keys, bitwise resume
COMMON = ["--impl=torch", "--cpu", "--model=mlp", "--in_channels=1", "--batch_size=32", "--test_interval=1000",
          "--log_step_count_steps=0", "--train_data=synthetic://1500", "--test_data=synthetic://300?seed=1",
          "--eval_examples=300", "--base_lr=0.001"]


def run_main(args, timeout=300):
    e = dict(os.environ, OMP_NUM_THREADS="2", PYTHONUNBUFFERED="1")
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, env=e,
                          capture_output=True, text=True, timeout=timeout)


def restore(d, step):
    from distributed_tensorflow_ibm_mnist_amd.ckpt.saver import Saver
    return Saver.restore(os.path.join(d, f"model.ckpt-{step}"))


ADAM_KEYS = ("hidden/weights/Adam", "hidden/weights/Adam_1", "beta1_power", "beta2_power", "global_step")


def test_cli_adam_checkpoint_and_bitwise_resume(tmp_path):
    da, db = str(tmp_path / "straight"), str(tmp_path / "resumed")
    opt = ["--optimizer=adam", "--save_checkpoint_steps=20"]
    r = run_main(COMMON + opt + ["--max_steps=40", f"--train_dir={da}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    r = run_main(COMMON + opt + ["--max_steps=20", f"--train_dir={db}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    r = run_main(COMMON + opt + ["--max_steps=40", f"--train_dir={db}"])
    assert r.returncode == 0 and "model.ckpt-20" in r.stdout, (r.stdout + r.stderr)[-3000:]
    for d in (da, db):
        for step in (20, 40):
            t = restore(d, step)
            for k in ADAM_KEYS:
                assert k in t, (d, step, k)
            assert int(t["global_step"]) == step
            assert np.float32(t["beta1_power"]) == np.float32(0.9 ** (step + 1))
            assert np.float32(t["beta2_power"]) == np.float32(0.999 ** (step + 1))
    ta, tb = restore(da, 40), restore(db, 40)
    keys = [k for k in ta if k.endswith(("/weights", "/biases", "/Adam", "/Adam_1", "/ExponentialMovingAverage"))]
    assert len(keys) == 4 * 4
    for k in keys:
        assert np.array_equal(np.asarray(ta[k]), np.asarray(tb[k])), k
    assert np.abs(np.asarray(ta["hidden/weights/Adam_1"])).max() > 0


@pytest.mark.parametrize("rule,keys", [("rmsprop", ("hidden/weights/RMSProp", "hidden/weights/RMSProp_1")),
                                       ("adagrad", ("hidden/weights/Adagrad",))])
def test_cli_checkpoint_keys(tmp_path, rule, keys):
    d = str(tmp_path / rule)
    r = run_main(COMMON + [f"--optimizer={rule}", "--max_steps=5", f"--train_dir={d}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    t = restore(d, 5)
    for k in keys + ("global_step",):
        assert k in t, k
    assert "beta1_power" not in t and "hidden/weights/Momentum" not in t
    if rule == "rmsprop":      # ms starts at 1.0 and decays by 0.9 per step towards g^2; the momentum is 0
        ms = np.asarray(t["hidden/weights/RMSProp"])
        # five fp32 products: 0.9^5 to within 5 * 6e-8 relative
        assert 0.9 ** 5 * (1 - 1e-6) <= ms.min() and ms.max() < 1.5
    else:                      # the accumulator starts at 0.1 and only grows
        assert np.asarray(t["hidden/weights/Adagrad"]).min() >= np.float32(0.1)


# ------------------------------------------------------------------ 4. parameter-server mode refuses
def test_ps_mode_refuses_adaptive_optimizer():
    t0 = time.time()
    r = run_main(["--job_name=ps", "--ps_hosts=localhost:1", "--worker_hosts=localhost:2", "--optimizer=adam", "--cpu"],
                 timeout=60)
    dt = time.time() - t0
    out = r.stdout + r.stderr
    assert r.returncode != 0, out[-2000:]
    line = [l for l in out.splitlines() if "parameter-server mode" in l]
    assert len(line) == 1 and "'adam'" in line[0] and "sgd|momentum|nesterov" in line[0], out[-2000:]
    assert "Traceback" not in out, out[-2000:]
    assert dt < 2.0, dt    # start-up only: refused before torch is imported or any socket is opened
