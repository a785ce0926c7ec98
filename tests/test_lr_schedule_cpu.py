"""Learning-rate warmup with polynomial and cosine decay, CPU side: the parameter manager's keys and
flags with every refusal, ``OptConfig.lr_at`` against the float64 oracle
(tests/lr_schedule_oracle.py), the plain-torch update over the warmup boundary, the training CLI's
``learning_rate`` scalars and the parameter-server refusal."""
import importlib.util
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lr_schedule_oracle",
                                               os.path.join(ROOT, "tests", "lr_schedule_oracle.py"))
oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(oracle)


@pytest.fixture
def pm():
    from distributed_tensorflow_ibm_mnist_amd.utils import parameter_mgr
    yield parameter_mgr
    parameter_mgr.configure({})


# ------------------------------------------------------------------ 1. manager / config
def test_defaults_keys_and_flags(pm, tmp_path):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    for k in ("lr_schedule", "warmup_steps", "lr_total_steps", "lr_end", "lr_power"):
        assert k in pm.FLAG_KEYS and k in pm.DEFAULTS, k
    assert "warmup_steps" in pm.FLAG_KEYS
    pm.configure({})
    o = pm.getOptimizer(0.1)
    assert (o.lr_schedule, o.warmup_steps, o.lr_end, o.lr_power) == ("staircase", 0, 0.0, 1.0)
    c = OptConfig.from_spec(o, 100, 0.1)
    assert (c.schedule, c.warmup_steps, c.lr_end, c.lr_power, c.scheduled) == ("staircase", 0, 0.0, 1.0, False)
    assert c == OptConfig(lr0=0.1, decay_rate=0.1, decay_steps=100)           # the defaults spelled out are the defaults
    pm.configure({"lr_schedule": "Cosine", "warmup_steps": 5, "max_steps": 70})   # case-insensitive; T = max_steps
    o = pm.getOptimizer(0.1)
    assert (o.lr_schedule, o.warmup_steps, o.lr_total_steps) == ("cosine", 5, 70)
    assert pm.getLrSchedule() == "cosine" and pm.getWarmupSteps() == 5 and pm.getLrTotalSteps() == 70
    c = OptConfig.from_spec(o, 100, 0.1)
    assert (c.schedule, c.warmup_steps, c.total_steps, c.scheduled) == ("cosine", 5, 70, True)
    y = tmp_path / "p.yaml"
    y.write_text("optimizer: lamb\nlr_schedule: polynomial\nlr_power: 2.0\nwarmup_steps: 10\nlr_total_steps: 400\n"
                 "lr_end: 0.001\n")
    pm.configure(str(y))
    c = OptConfig.from_spec(pm.getOptimizer(0.1), 0, 0.1)
    assert (c.rule, c.schedule, c.lr_power, c.warmup_steps, c.total_steps, c.lr_end) == \
        ("lamb", "polynomial", 2.0, 10, 400, 0.001)
    pm.configure(str(y), warmup_steps=20, lr_schedule="cosine")                 # keyword overrides win
    o = pm.getOptimizer(0.1)
    assert (o.lr_schedule, o.warmup_steps, o.lr_total_steps) == ("cosine", 20, 400)

    class Flags:                                                               # the CLI's flags; '' and -1: unset
        config, lr_schedule, warmup_steps, lr_total_steps, lr_end, lr_power = "", "polynomial", 3, 9, -1, -1
    pm.configure_from_flags(Flags)
    o = pm.getOptimizer(0.1)
    assert (o.lr_schedule, o.warmup_steps, o.lr_total_steps, o.lr_end, o.lr_power) == ("polynomial", 3, 9, 0.0, 1.0)

    class Unset:
        config, lr_schedule, warmup_steps, lr_total_steps, lr_end, lr_power = "", "", -1, -1, -1, -1
    pm.configure_from_flags(Unset)
    assert pm.getOptimizer(0.1) == pm.OptimizerSpec("sgd", 0.1, 0.0, False)
    # warmup alone keeps the staircase and does not read lr_total_steps or lr_power
    pm.configure({"warmup_steps": 2000, "max_steps": 1000, "lr_power": -3})
    o = pm.getOptimizer(0.1)
    assert (o.lr_schedule, o.warmup_steps, o.lr_total_steps, o.lr_power) == ("staircase", 2000, 0, 1.0)
    assert OptConfig.from_spec(o, 100, 0.1).scheduled


def test_shipped_warmup_config_loads(pm):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    pm.configure(os.path.join(ROOT, "configs", "lenet5_lars_warmup.yaml"))
    o = pm.getOptimizer(pm.getBaseLearningRate())
    c = OptConfig.from_spec(o, 0, 0.1)
    assert (c.rule, c.schedule, c.lr_power, c.total_steps) == ("lars", "polynomial", 2.0, pm.getMaxSteps())
    assert 0 < c.warmup_steps < c.total_steps and pm.getTrainBatchSize() == 8192


BAD = [({"lr_schedule": "linear"}, "lr_schedule", "linear"),
       ({"warmup_steps": -1}, "warmup_steps", "-1"),
       ({"warmup_steps": 2.5}, "warmup_steps", "2.5"),
       ({"warmup_steps": "soon"}, "warmup_steps", "soon"),
       ({"lr_schedule": "cosine", "warmup_steps": 10, "lr_total_steps": 10}, "lr_total_steps", "10"),
       ({"lr_schedule": "polynomial", "lr_total_steps": 0}, "lr_total_steps", "0"),
       ({"lr_schedule": "polynomial", "warmup_steps": 50, "max_steps": 40}, "lr_total_steps", "40"),
       ({"lr_schedule": "cosine", "lr_total_steps": 7.5}, "lr_total_steps", "7.5"),
       ({"lr_end": -0.1}, "lr_end", "-0.1"),
       ({"lr_end": float("inf")}, "lr_end", "inf"),
       ({"lr_end": float("nan")}, "lr_end", "nan"),
       ({"lr_schedule": "polynomial", "lr_power": 0}, "lr_power", "0"),
       ({"lr_schedule": "polynomial", "lr_power": -1.0}, "lr_power", "-1.0"),
       ({"lr_schedule": "polynomial", "lr_power": float("inf")}, "lr_power", "inf"),
       ({"lr_schedule": "polynomial", "lr_power": float("nan")}, "lr_power", "nan")]


@pytest.mark.parametrize("cfg,key,value", BAD)
def test_manager_refuses_and_names_key_and_value(pm, cfg, key, value):
    pm.configure(dict({"max_steps": 100}, **cfg))
    with pytest.raises(ValueError, match=f"(?s){key}.*{value}"):
        pm.getOptimizer(0.1)


@pytest.mark.parametrize("kw,key", [({"schedule": "linear"}, "schedule"), ({"warmup_steps": -1}, "warmup_steps"),
                                    ({"warmup_steps": 1.5}, "warmup_steps"),
                                    ({"schedule": "cosine", "warmup_steps": 4, "total_steps": 4}, "total_steps"),
                                    ({"schedule": "polynomial"}, "total_steps"),
                                    ({"lr_end": -1e-3}, "lr_end"), ({"lr_end": float("nan")}, "lr_end"),
                                    ({"lr_end": float("inf")}, "lr_end"), ({"lr_power": 0.0}, "lr_power"),
                                    ({"lr_power": float("inf")}, "lr_power"), ({"lr_power": float("nan")}, "lr_power")])
def test_opt_config_validates(kw, key):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    with pytest.raises(ValueError, match=key):
        OptConfig(**kw)


# ------------------------------------------------------------------ 2. lr_at against the oracle
SETS = [(0.05, 0.0, 3, 11), (0.05, 0.005, 0, 7), (0.5, 0.0, 500, 30000), (0.02, 0.0, 5, 2 ** 33)]


def steps_of(W, T):
    return sorted({t for t in (0, W - 1, W, W + 1, (W + T) // 2, T - 1, T, T + 1, 2 ** 40) if t >= 0})


@pytest.mark.parametrize("kind,power", [("polynomial", 1.0), ("polynomial", 2.0), ("polynomial", 0.5), ("cosine", 1.0)])
@pytest.mark.parametrize("lr0,lr_end,W,T", SETS)
def test_lr_at_matches_the_oracle(kind, power, lr0, lr_end, W, T):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    c = OptConfig(lr0=lr0, schedule=kind, warmup_steps=W, total_steps=T, lr_end=lr_end, lr_power=power)
    sched = oracle.schedule(kind, W, T, lr_end, power)
    for t in steps_of(W, T):
        got, want = c.lr_at(t), oracle.lr(t, lr0, **sched)
        assert abs(got - want) <= 1e-14 * lr0, (t, got, want)       # both float64: a few ulp of lr0
        if t >= T:
            assert got == lr_end, (t, got)                          # exactly
    if W > 0:
        assert c.lr_at(W - 1) == lr0
        assert c.lr_at(0) < c.lr_at(W // 2) <= lr0
    assert c.lr_at(W) == lr0                                       # no jump at the end of the warmup
    assert c.lr_at(W + 1) <= lr0 and lr_end < c.lr_at((W + T) // 2) < lr0     # T = 2**33: 1 - cos(1e-10) rounds to 0


def test_staircase_is_unchanged_and_takes_a_warmup():
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    c = OptConfig(lr0=0.1, decay_rate=0.1, decay_steps=100)           # the values test_config_models.py pins
    assert c.lr_at(0) == 0.1 and c.lr_at(99) == 0.1 and abs(c.lr_at(100) - 0.01) < 1e-12
    assert abs(c.lr_at(250) - 0.001) < 1e-12
    for t in (0, 1, 99, 100, 101, 250, 2 ** 40):
        assert c.lr_at(t) == 0.1 * 0.1 ** (t // 100)
    w = OptConfig(lr0=0.1, decay_rate=0.1, decay_steps=100, warmup_steps=150)   # multiplies the unshifted staircase
    sched = oracle.schedule("staircase", W=150)
    for t in (0, 1, 99, 100, 148, 149, 150, 151, 250):
        assert abs(w.lr_at(t) - oracle.lr(t, 0.1, 0.1, 100, **sched)) <= 1e-15, t
    assert w.lr_at(149) == c.lr_at(149) and w.lr_at(150) == c.lr_at(150) and abs(w.lr_at(0) - 0.1 / 150) <= 1e-15
    assert abs(w.lr_at(100) - 101 / 150 * 0.01) <= 1e-15


# ------------------------------------------------------------------ 3. torch_update across the warmup boundary
SHAPES = [("a/weights", (5, 5, 1, 7), 0.0), ("a/biases", (7,), None), ("b/weights", (40, 33), 0.004),
          ("b/biases", (33,), None), ("c/weights", (33, 20), 0.002), ("c/biases", (20,), None)]
WDS = {n: wd for n, _, wd in SHAPES}


@pytest.mark.parametrize("kind", ["polynomial", "cosine"])
@pytest.mark.parametrize("rule", ["momentum", "adam"])
def test_torch_update_follows_the_schedule(rule, kind):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import FlatParams, OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import torch_update
    torch.manual_seed(61)
    init = {n: torch.randn(*s) for n, s, _ in SHAPES}
    fp = FlatParams.build(SHAPES, init, "cpu", pads={})
    sched = oracle.schedule(kind, W=3, T=7, lr_end=0.005, power=2.0)
    cfg = OptConfig(lr0=0.05, ema_max=0.9999, **oracle.opt_config_kwargs(rule, sched))
    fp.init_slots(cfg)
    ref = oracle.make(rule, {n: v.numpy() for n, v in init.items()}, WDS, 0.05, 0.1, 0, 0.9999, sched, grad_scale=0.5)
    rates = []
    for k in range(8):
        g = {n: torch.randn_like(init[n]) for n in init}
        for n in g:
            fp.grad_view(n).copy_(g[n])
        rates.append(ref.lr())
        torch_update(fp, cfg, grad_scale=0.5)
        fp.step += 1
        ref.step({n: v.numpy() for n, v in g.items()})
    assert abs(rates[0] - 0.05 / 3) < 1e-15 and rates[2] == 0.05 and rates[7] == 0.005
    assert abs(rates[3] - 0.05) < 1e-15 and rates[3] > rates[4] > rates[5] > rates[6] > rates[7]
    for n in init:
        s1, s2 = fp.slot_views(n)
        oracle.close(fp.param_view(n).numpy(), ref.p[n])
        oracle.close(fp.ema_view(n).numpy(), ref.ema[n])
        oracle.close(s1.numpy(), ref.s1[n])
        if rule == "adam":
            oracle.close(s2.numpy(), ref.s2[n])


# ------------------------------------------------------------------ 4. CLI, torch impl on the CPU
COMMON = ["--impl=torch", "--cpu", "--model=mlp", "--in_channels=1", "--batch_size=32", "--test_interval=1000",
          "--log_step_count_steps=0", "--train_data=synthetic://1500", "--test_data=synthetic://300?seed=1",
          "--eval_examples=300", "--save_summaries_steps=1"]


def run_main(args, timeout=300):
    e = dict(os.environ, OMP_NUM_THREADS="2", PYTHONUNBUFFERED="1")
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, env=e,
                          capture_output=True, text=True, timeout=timeout)


def scalars(d, tag):
    from distributed_tensorflow_ibm_mnist_amd.obs.events import find_event_files, read_events
    out = {}
    for f in find_event_files(d):
        for ev in read_events(f):
            if tag in ev["values"]:
                out[ev["step"]] = ev["values"][tag]
    return out


def test_cli_logs_the_scheduled_learning_rate(tmp_path):
    from distributed_tensorflow_ibm_mnist_amd.ckpt.saver import Saver
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    d = str(tmp_path / "cos")
    r = run_main(COMMON + ["--optimizer=momentum", "--base_lr=0.05", "--max_steps=12", "--warmup_steps=4",
                           "--lr_schedule=cosine", f"--train_dir={d}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    c = OptConfig(lr0=0.05, schedule="cosine", warmup_steps=4, total_steps=12)    # lr_total_steps: max_steps
    got = scalars(d, "learning_rate")
    assert sorted(got) == list(range(1, 13)), sorted(got)
    for step, v in got.items():                                                   # the events hold float32
        assert np.float32(v) == np.float32(c.lr_at(step)), (step, v, c.lr_at(step))
        assert abs(c.lr_at(step) - oracle.lr(step, 0.05, kind="cosine", W=4, T=12)) <= 1e-15
    assert np.float32(got[1]) == np.float32(0.025) and np.float32(got[3]) == np.float32(got[4]) == np.float32(0.05)
    assert got[4] > got[5] > got[11] > got[12] == 0.0
    t = Saver.restore(os.path.join(d, "model.ckpt-12"))          # a pure function of global_step: no new state
    assert int(np.asarray(t["global_step"])) == 12
    assert not any(w in k.lower() for k in t for w in ("warmup", "schedule", "learning_rate")), sorted(t)


# ------------------------------------------------------------------ 5. parameter-server mode refuses
@pytest.mark.parametrize("flags,what", [(["--lr_schedule=cosine", "--max_steps=10"], "'cosine'"),
                                        (["--lr_schedule=polynomial", "--max_steps=10"], "'polynomial'"),
                                        (["--warmup_steps=5"], "warmup_steps 5")])
@pytest.mark.parametrize("job", ["ps", "worker"])
def test_ps_mode_refuses_schedules_and_warmup(job, flags, what):
    t0 = time.time()
    r = run_main([f"--job_name={job}", "--ps_hosts=localhost:1", "--worker_hosts=localhost:2", "--cpu"] + flags,
                 timeout=60)
    dt = time.time() - t0
    out = r.stdout + r.stderr
    assert r.returncode == 2, out[-2000:]
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1 and what in lines[0] and "parameter-server mode" in lines[0], out[-2000:]
    assert "Traceback" not in out, out[-2000:]
    assert dt < 2.0, dt    # start-up only: refused before torch is imported or any socket is opened


def test_ps_check_passes_the_defaults(pm):
    pm.configure({})
    said = []
    pm.check_ps_lr_schedule("worker", said.append)
    pm.check_ps_lr_schedule("ps", said.append)
    pm.configure({"lr_schedule": "cosine", "warmup_steps": 3})
    pm.check_ps_lr_schedule("", said.append)                       # not a PS task: nothing to refuse
    assert said == []
    with pytest.raises(SystemExit) as e:
        pm.check_ps_lr_schedule("worker", said.append)
    assert e.value.code == 2 and len(said) == 1 and "parameter-server mode" in said[0]
