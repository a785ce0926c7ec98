"""LARS and LAMB, CPU side: the parameter manager's names and ``lars_eta`` key, the plain-torch
update against the float64 oracle (tests/layerwise_oracle.py), the training CLI with its
checkpoint slots and ``trust_ratio/*`` scalars, resuming across adam / lamb and momentum / lars,
the parameter-server refusal and two data-parallel gloo ranks."""
import importlib.util
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("layerwise_oracle", os.path.join(ROOT, "tests", "layerwise_oracle.py"))
oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(oracle)


# ------------------------------------------------------------------ 1. manager / config
@pytest.fixture
def pm():
    from distributed_tensorflow_ibm_mnist_amd.utils import parameter_mgr
    yield parameter_mgr
    parameter_mgr.configure({})


def test_names_defaults_and_overrides(pm, tmp_path, monkeypatch):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    pm.configure({"optimizer": "LARS"})                                                   # case-insensitive
    o = pm.getOptimizer(0.1)
    assert (o.name, o.lars_eta, o.momentum, o.epsilon, o.nesterov) == ("lars", 0.001, 0.9, None, False)
    c = OptConfig.from_spec(o, 100, 0.1)
    assert (c.rule, c.lars_eta, c.eps, c.use_momentum, c.momentum) == ("lars", 0.001, 0.0, True, 0.9)
    assert c.slot_names() == ("Momentum", None) and c.slot_init() == (0.0, 0.0)
    pm.configure({"optimizer": "Lamb"})
    o = pm.getOptimizer(0.1)
    assert (o.name, o.beta1, o.beta2, o.epsilon) == ("lamb", 0.9, 0.999, None)
    c = OptConfig.from_spec(o, 100, 0.1)
    assert (c.rule, c.eps) == ("lamb", 1e-6)
    assert c.slot_names() == ("Adam", "Adam_1") and c.slot_init() == (0.0, 0.0)
    assert "lars_eta" in pm.FLAG_KEYS
    pm.configure({"optimizer": "lars", "lars_eta": 0.02, "momentum": 0.8, "epsilon": 1e-9})  # a dict
    c = OptConfig.from_spec(pm.getOptimizer(0.1), 0, 0.1)
    assert (c.lars_eta, c.momentum, c.eps) == (0.02, 0.8, 1e-9)
    y = tmp_path / "p.yaml"
    y.write_text("optimizer: lamb\nbeta2: 0.99\nepsilon: 1.0e-5\n")
    pm.configure(str(y))                                                                   # YAML
    c = OptConfig.from_spec(pm.getOptimizer(0.1), 0, 0.1)
    assert (c.rule, c.beta2, c.eps) == ("lamb", 0.99, 1e-5)
    pm.configure(str(y), optimizer="lars", lars_eta=0.005)                                 # keyword overrides win
    o = pm.getOptimizer(0.1)
    assert (o.name, o.lars_eta) == ("lars", 0.005)
    y2 = tmp_path / "q.yaml"
    y2.write_text("optimizer: lars\nlars_eta: 0.003\n")
    monkeypatch.setenv("MNISTX_PARAMS", str(y2))
    pm.configure()                                                                         # MNISTX_PARAMS
    assert pm.getOptimizer(0.1).lars_eta == 0.003

    class Flags:                                                                           # the CLI's flags
        config, optimizer, lars_eta = "", "lars", 0.004
    pm.configure_from_flags(Flags)
    assert pm.getOptimizer(0.1).lars_eta == 0.004


@pytest.mark.parametrize("bad", [0, -1.0, float("inf"), float("nan")])
def test_lars_eta_must_be_positive(pm, bad):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    pm.configure({"optimizer": "lars", "lars_eta": bad})
    with pytest.raises(ValueError, match="lars_eta"):
        pm.getOptimizer(0.1)
    with pytest.raises(ValueError, match="lars_eta"):
        OptConfig(rule="lars", lars_eta=bad)


@pytest.mark.parametrize("rule", oracle.RULES)
def test_clip_norm_is_refused_with_the_layerwise_rules(pm, rule):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    pm.configure({"optimizer": rule, "clip_norm": 1.0})
    with pytest.raises(ValueError, match=f"(?s){rule}.*clip_norm"):
        pm.getOptimizer(0.1)
    with pytest.raises(ValueError, match=f"(?s){rule}.*clip_norm"):
        OptConfig(rule=rule, clip_norm=1.0)


def test_unknown_name_lists_the_new_rules(pm):
    pm.configure({"optimizer": "lion"})
    with pytest.raises(ValueError, match=r"sgd\|momentum\|nesterov\|adam\|rmsprop\|adagrad\|lars\|lamb"):
        pm.getOptimizer(0.1)


def test_shipped_lars_config_loads(pm):
    pm.configure(os.path.join(ROOT, "configs", "lenet5_lars.yaml"))
    o = pm.getOptimizer(pm.getBaseLearningRate())
    assert o.name == "lars" and o.lars_eta > 0 and pm.getMaxSteps() > 0 and pm.getTrainBatchSize() > 0


# ------------------------------------------------------------------ 2. torch_update vs the float64 oracle
# the six-tensor layout of the GPU tests: offsets 0 / 175 / 182 / 1502 / 1535 / 2195
SHAPES = [("a/weights", (5, 5, 1, 7), 0.0), ("a/biases", (7,), None), ("b/weights", (40, 33), 0.004),
          ("b/biases", (33,), None), ("c/weights", (33, 20), 0.002), ("c/biases", (20,), None)]
WDS = {n: wd for n, _, wd in SHAPES}
AMPL = [1.0, 0.1, 2.0, 0.05, 1.0]
LR0 = {"lars": 0.5, "lamb": 0.01}


def six_tensor_init(seed):
    torch.manual_seed(seed)
    init = {n: torch.randn(*s) for n, s, _ in SHAPES}
    init["c/weights"].zero_()          # pn = 0: ratio 1 at step 1
    return init


def step_grads(init, k):
    g = {n: torch.randn_like(init[n]) * AMPL[k] for n in init}
    if k == 0:
        g["a/weights"].zero_()         # wd 0: gn = un = 0, ratio 1 at step 1
    return g


@pytest.mark.parametrize("rule", oracle.RULES)
def test_torch_update_matches_float64_oracle(rule):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import FlatParams, OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import torch_update
    init = six_tensor_init(31)
    fp = FlatParams.build(SHAPES, init, "cpu", pads={})
    assert [int(r[0]) for r in fp.segs.tolist()] == [0, 175, 182, 1502, 1535, 2195]
    assert [int(r[13]) for r in fp.segs.tolist()] == [1, 0, 1, 0, 1, 0]            # the adapt column
    cfg = OptConfig(lr0=LR0[rule], decay_rate=0.5, decay_steps=2, ema_max=0.9999, rule=rule, momentum=0.9)
    fp.init_slots(cfg)
    assert fp.tnorm is not None and (rule == "lars" or fp.slot2 is not None)
    ref = oracle.LayerwiseOracle(rule, {n: v.numpy() for n, v in init.items()}, WDS, LR0[rule], 0.5, 2, 0.9999,
                                 grad_scale=0.5)
    for k in range(5):
        g = step_grads(init, k)
        for n in g:
            fp.grad_view(n).copy_(g[n])
        torch_update(fp, cfg, grad_scale=0.5)
        fp.step += 1
        ref.step({n: v.numpy() for n, v in g.items()})
        tr = fp.trust_ratios()
        for n in init:
            pn, un, r = tr[n]
            for got, want in ((pn, ref.pn[-1][n]), (un, ref.un[-1][n]), (r, ref.r[-1][n])):
                assert abs(got - want) <= 1e-5 * abs(want), (k, n, got, want)
            if n.endswith("biases"):
                assert r == 1.0
    assert ref.r[0]["c/weights"] == 1.0 and ref.r[0]["a/weights"] == 1.0 and ref.r[0]["b/weights"] != 1.0
    assert all(ref.r[1][n] != 1.0 for n in init if n.endswith("weights"))
    for n in init:
        s1, s2 = fp.slot_views(n)
        oracle.close(fp.param_view(n).numpy(), ref.p[n])
        oracle.close(fp.ema_view(n).numpy(), ref.ema[n])
        oracle.close(s1.numpy(), ref.s1[n])
        if rule == "lamb":
            oracle.close(s2.numpy(), ref.s2[n])


@pytest.mark.parametrize("rule", oracle.RULES)
def test_torch_update_nonfinite_norm_gives_nan_ratio(rule):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import FlatParams, OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import torch_update
    init = six_tensor_init(32)
    fp = FlatParams.build(SHAPES, init, "cpu", pads={})
    cfg = OptConfig(lr0=0.05, rule=rule, momentum=0.9)
    fp.init_slots(cfg)
    fp.grads.normal_()
    fp.grads[700] = float("inf")                                  # inside b/weights
    torch_update(fp, cfg)
    tr = fp.trust_ratios()
    assert np.isnan(tr["b/weights"][2]) and tr["a/weights"][2] > 0 and tr["b/biases"][2] == 1.0
    assert torch.isnan(fp.param_view("b/weights")).all()


def test_torch_update_needs_init_slots():
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import FlatParams, OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import torch_update
    fp = FlatParams.build(SHAPES, six_tensor_init(33), "cpu", pads={})
    for rule in oracle.RULES:
        with pytest.raises(RuntimeError, match="init_slots"):
            torch_update(fp, OptConfig(rule=rule))


# ------------------------------------------------------------------ 3. CLI, torch impl on the CPU
COMMON = ["--impl=torch", "--cpu", "--model=mlp", "--in_channels=1", "--batch_size=32", "--test_interval=1000",
          "--log_step_count_steps=0", "--train_data=synthetic://1500", "--test_data=synthetic://300?seed=1",
          "--eval_examples=300", "--save_summaries_steps=1"]
CLI = {"lars": ["--optimizer=lars", "--base_lr=1.0", "--lars_eta=0.02"], "lamb": ["--optimizer=lamb", "--base_lr=0.002"],
       "momentum": ["--optimizer=momentum", "--base_lr=0.05"], "adam": ["--optimizer=adam", "--base_lr=0.001"]}


def run_main(args, timeout=300):
    e = dict(os.environ, OMP_NUM_THREADS="2", PYTHONUNBUFFERED="1")
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, env=e,
                          capture_output=True, text=True, timeout=timeout)


def scalars(d, prefix):
    """tag -> {step: value} of the events whose tag starts with ``prefix``."""
    from distributed_tensorflow_ibm_mnist_amd.obs.events import find_event_files, read_events
    out = {}
    for f in find_event_files(d):
        for ev in read_events(f):
            for tag, v in ev["values"].items():
                if tag.startswith(prefix):
                    out.setdefault(tag, {})[ev["step"]] = v
    return out


def restore(d, step):
    from distributed_tensorflow_ibm_mnist_amd.ckpt.saver import Saver
    return Saver.restore(os.path.join(d, f"model.ckpt-{step}"))


@pytest.mark.parametrize("rule", oracle.RULES)
def test_cli_checkpoint_slots_resume_and_trust_ratio_tags(tmp_path, rule):
    da, db = str(tmp_path / "straight"), str(tmp_path / "resumed")
    r = run_main(COMMON + CLI[rule] + ["--max_steps=12", f"--train_dir={da}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    t = restore(da, 12)
    weights = sorted(k for k in t if k.endswith("/weights"))
    biases = sorted(k for k in t if k.endswith("/biases"))
    assert weights and biases
    if rule == "lars":
        assert all(f"{v}/Momentum" in t for v in weights + biases)
        assert not any(k.endswith(("/Adam", "/Adam_1")) for k in t) and "beta1_power" not in t
    else:
        assert all(f"{v}/Adam" in t and f"{v}/Adam_1" in t for v in weights + biases)
        assert "beta1_power" in t and "beta2_power" in t
        assert not any(k.endswith("/Momentum") for k in t)
    assert not any("trust" in k or "tnorm" in k for k in t)        # the ratios are not state
    tags = scalars(da, "trust_ratio/")
    assert sorted(tags) == [f"trust_ratio/{v}" for v in weights], sorted(tags)
    for tag, by_step in tags.items():
        assert sorted(by_step) == list(range(1, 13)), (tag, sorted(by_step))
        assert all(np.isfinite(v) and v > 0 for v in by_step.values()), (tag, by_step)
    # 6 steps, then 6 more from the checkpoint: bit for bit the 12 straight ones
    r = run_main(COMMON + CLI[rule] + ["--max_steps=6", f"--train_dir={db}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    r = run_main(COMMON + CLI[rule] + ["--max_steps=12", f"--train_dir={db}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    u = restore(db, 12)
    assert sorted(u) == sorted(t)
    for k in t:
        assert np.array_equal(np.asarray(t[k]), np.asarray(u[k])), k


@pytest.mark.parametrize("first,second", [("adam", "lamb"), ("lamb", "adam"), ("momentum", "lars"),
                                          ("lars", "momentum")])
def test_cli_resumes_from_the_sibling_rules_checkpoint(tmp_path, first, second):
    d = str(tmp_path / "train")
    r = run_main(COMMON + CLI[first] + ["--max_steps=4", f"--train_dir={d}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    t = restore(d, 4)
    r = run_main(COMMON + CLI[second] + ["--max_steps=8", f"--train_dir={d}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    u = restore(d, 8)
    assert sorted(u) == sorted(t) and int(np.asarray(u["global_step"])) == 8
    slot = "Adam" if "adam" in (first, second) else "Momentum"
    k = next(k for k in sorted(t) if k.endswith(f"/weights/{slot}"))
    assert np.abs(np.asarray(t[k])).max() > 0                       # the slot was carried over, then moved on
    assert not np.array_equal(np.asarray(t[k]), np.asarray(u[k]))
    assert all(np.isfinite(np.asarray(v)).all() for v in u.values())


# ------------------------------------------------------------------ 4. parameter-server mode refuses
@pytest.mark.parametrize("rule", oracle.RULES)
def test_ps_mode_refuses_the_layerwise_rules(rule):
    t0 = time.time()
    r = run_main(["--job_name=worker", "--ps_hosts=localhost:1", "--worker_hosts=localhost:2", f"--optimizer={rule}",
                  "--cpu"], timeout=60)
    dt = time.time() - t0
    out = r.stdout + r.stderr
    assert r.returncode != 0, out[-2000:]
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1 and f"'{rule}'" in lines[0] and "parameter-server mode" in lines[0], out[-2000:]
    assert "Traceback" not in out, out[-2000:]
    assert dt < 2.0, dt    # start-up only: refused before torch is imported or any socket is opened


# ------------------------------------------------------------------ 5. two data-parallel gloo ranks
def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, steps, B, rule, out_q):
    import torch.distributed as dist
    torch.set_num_threads(1)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.parallel.dp import DataParallel
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import TorchNet
    spec = get_model("mlp", 1)
    opt = OptConfig(lr0=LR0[rule], ema_max=0.9999, rule=rule, momentum=0.9, lars_eta=0.02)
    net = TorchNet(spec, B, "cpu", torch_ref.init_params(spec, seed=0), opt)
    dp = DataParallel(net, bucket_cap_mb=0.05)
    g = torch.Generator().manual_seed(321)
    ratios = []
    for _ in range(steps):
        x = torch.rand(world * B, 28, 28, 1, generator=g) - 0.5
        y = torch.randint(0, 10, (world * B,), generator=g, dtype=torch.int32)
        net.x0.copy_(x[rank * B:(rank + 1) * B])
        net.labels.copy_(y[rank * B:(rank + 1) * B])
        dp.train_step()
        st = net.read_stats()
        ratios.append(sorted((k, v) for k, v in st.items() if k.startswith("trust_ratio/")))
    slot2 = net.fp.slot2.clone() if net.fp.slot2 is not None else torch.zeros(1)
    out_q.put((rank, net.fp.params.clone(), net.fp.mom.clone(), slot2, ratios))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("rule", oracle.RULES)
def test_dp_two_gloo_ranks_report_identical_ratios(rule):
    """The norms are taken after the all-reduce, of the averaged gradient: both ranks derive the
    same ratios from bitwise-equal inputs and end with bitwise-equal parameters."""
    import torch.multiprocessing as mp
    world, B, steps = 2, 8, 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, steps, B, rule, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict((r[0], r[1:]) for r in (q.get(timeout=240) for _ in range(world)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for a, b, name in zip(got[0][:3], got[1][:3], ("params", "slot 1", "slot 2")):
        assert torch.equal(a, b), name
    assert got[0][3] == got[1][3]
    last = dict(got[0][3][-1])
    assert sorted(last) == ["trust_ratio/hidden/weights", "trust_ratio/softmax_linear/weights"] and all(np.isfinite(v) and v > 0 and v != 1.0 for v in last.values()), last
