"""Gradient clipping by global norm, CPU side: the parameter manager's ``clip_norm`` key, the
plain-torch update against the float64 oracle (tests/clip_oracle.py), the training CLI with its
``global_norm`` scalars, the parameter-server refusal and two data-parallel gloo ranks."""
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
_spec = importlib.util.spec_from_file_location("clip_oracle", os.path.join(ROOT, "tests", "clip_oracle.py"))
oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(oracle)


# ------------------------------------------------------------------ 1. manager / config
@pytest.fixture
def pm():
    from distributed_tensorflow_ibm_mnist_amd.utils import parameter_mgr
    yield parameter_mgr
    parameter_mgr.configure({})


def test_clip_norm_key_sources_and_default(pm, tmp_path, monkeypatch):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    pm.configure({})
    assert pm.getOptimizer(0.1).clip_norm is None and OptConfig().clip_norm is None       # the default: off
    assert "clip_norm" in pm.FLAG_KEYS
    for name in ("sgd", "momentum", "nesterov", "adam", "rmsprop", "adagrad"):
        pm.configure({"optimizer": name, "clip_norm": 2.5})                              # a dict
        o = pm.getOptimizer(0.1)
        assert o.clip_norm == 2.5, name
        assert OptConfig.from_spec(o, 100, 0.1).clip_norm == 2.5, name                   # from_spec carries it
    y = tmp_path / "p.yaml"
    y.write_text("optimizer: adam\nclip_norm: 1.5\n")
    pm.configure(str(y))                                                                   # YAML
    assert pm.getOptimizer(0.1).clip_norm == 1.5
    pm.configure(str(y), clip_norm=0.25)                                                   # a keyword override wins
    assert pm.getOptimizer(0.1).clip_norm == 0.25
    y2 = tmp_path / "q.yaml"
    y2.write_text("optimizer: momentum\nclip_norm: 3\n")
    monkeypatch.setenv("MNISTX_PARAMS", str(y2))
    pm.configure()                                                                         # MNISTX_PARAMS
    o = pm.getOptimizer(0.1)
    assert (o.name, o.clip_norm) == ("momentum", 3.0)
    assert OptConfig.from_spec(pm.getOptimizer(0.1), 0, 0.1).clip_norm == 3.0


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("inf"), float("nan")])
def test_clip_norm_must_be_positive(pm, bad):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    pm.configure({"clip_norm": bad})
    with pytest.raises(ValueError, match="clip_norm"):
        pm.getOptimizer(0.1)
    with pytest.raises(ValueError, match="clip_norm"):
        OptConfig(clip_norm=bad)


# ------------------------------------------------------------------ 2. torch_update vs the float64 oracle
SHAPES = [("a/weights", (5, 5, 1, 7), 0.0), ("a/biases", (7,), None), ("b/weights", (40, 33), 0.004),
          ("b/biases", (33,), None)]
ZERO_GRAD = "b/biases"
CLIP = 5.0
# per-step gradient amplitudes: randn over 1502 elements * grad_scale 0.5 has norm ~19.4 at amplitude 1,
# so clipping at 5 is active at amplitudes 1 and 2 and inactive at 0.1, 0.05 and 0.2
AMPL = [1.0, 0.1, 1.0, 0.05, 2.0, 0.2]


@pytest.mark.parametrize("rule", oracle.RULES)
def test_torch_update_matches_float64_oracle(rule):
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import FlatParams, OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import torch_update
    torch.manual_seed(21)
    init = {n: torch.randn(*s) for n, s, _ in SHAPES}
    fp = FlatParams.build(SHAPES, init, "cpu", pads={})
    cfg = OptConfig(lr0=0.05, decay_rate=0.5, decay_steps=3, ema_max=0.9999, clip_norm=CLIP,
                    **oracle.opt_config_kwargs(rule))
    fp.init_slots(cfg)
    ref = oracle.ClipOracle(rule, {n: v.numpy() for n, v in init.items()}, {n: wd for n, _, wd in SHAPES},
                            0.05, 0.5, 3, 0.9999, CLIP, grad_scale=0.5)
    for k in range(6):
        g = {n: torch.randn_like(init[n]) * AMPL[k] for n in init}
        g[ZERO_GRAD].zero_()
        for n in g:
            fp.grad_view(n).copy_(g[n])
        torch_update(fp, cfg, grad_scale=0.5)
        fp.step += 1
        ref.step({n: v.numpy() for n, v in g.items()})
        gn, s = fp.gnorm[:2].tolist()
        assert abs(gn - ref.norms[-1]) <= 1e-5 * ref.norms[-1], (k, gn, ref.norms[-1])
        assert abs(s - ref.scales[-1]) <= 1e-5, (k, s, ref.scales[-1])
        assert (s == 1.0) == (not ref.active[-1]), (k, s)          # inactive: exactly 1
    assert ref.active == [True, False, True, False, True, False]   # both branches ran
    for n in init:
        s1, s2 = fp.slot_views(n)
        oracle.close(fp.param_view(n).numpy(), ref.p[n])
        oracle.close(fp.ema_view(n).numpy(), ref.ema[n])
        if rule != "sgd":
            oracle.close(s1.numpy(), ref.s1[n])
        if rule in ("adam", "rmsprop"):
            oracle.close(s2.numpy(), ref.s2[n])
    assert torch.isfinite(fp.params).all()


def test_torch_update_nonfinite_norm_gives_nan():
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import FlatParams, OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import torch_update
    torch.manual_seed(22)
    init = {n: torch.randn(*s) for n, s, _ in SHAPES}
    fp = FlatParams.build(SHAPES, init, "cpu", pads={})
    cfg = OptConfig(lr0=0.05, clip_norm=1.0)
    fp.init_slots(cfg)
    fp.grads.normal_()
    fp.grads[300] = float("inf")
    torch_update(fp, cfg)
    assert not np.isfinite(float(fp.gnorm[0])) and np.isnan(float(fp.gnorm[1]))
    assert torch.isnan(fp.params).all()


def test_torch_update_needs_init_slots():
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import FlatParams, OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import torch_update
    init = {n: torch.randn(*s) for n, s, _ in SHAPES}
    fp = FlatParams.build(SHAPES, init, "cpu", pads={})
    with pytest.raises(RuntimeError, match="init_slots"):
        torch_update(fp, OptConfig(clip_norm=1.0))


# ------------------------------------------------------------------ 3. CLI, torch impl on the CPU
COMMON = ["--impl=torch", "--cpu", "--model=mlp", "--in_channels=1", "--batch_size=32", "--test_interval=1000",
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


def restore(d, step):
    from distributed_tensorflow_ibm_mnist_amd.ckpt.saver import Saver
    return Saver.restore(os.path.join(d, f"model.ckpt-{step}"))


def test_cli_writes_global_norm_and_clips(tmp_path):
    d = str(tmp_path / "clip")
    r = run_main(COMMON + ["--clip_norm=0.5", f"--train_dir={d}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    gn, sc = scalars(d, "global_norm"), scalars(d, "clip_scale")
    assert sorted(gn) == list(range(1, 21)) and sorted(sc) == sorted(gn), (sorted(gn), sorted(sc))
    print("global_norm by step:", [round(gn[k], 4) for k in sorted(gn)])
    for k in gn:
        assert gn[k] > 0 and sc[k] * gn[k] <= 0.5 * (1 + 1e-5), (k, gn[k], sc[k])
    assert any(sc[k] < 1.0 for k in sc)     # a fresh MLP's gradient norm is above 0.5: clipping ran
    assert "global_norm=" in r.stdout       # the result line


def test_cli_huge_clip_norm_is_bitwise_no_clipping(tmp_path):
    da, db = str(tmp_path / "plain"), str(tmp_path / "clip")
    r = run_main(COMMON + [f"--train_dir={da}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    r = run_main(COMMON + ["--clip_norm=1e30", f"--train_dir={db}"])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    ta, tb = restore(da, 20), restore(db, 20)
    assert sorted(ta) == sorted(tb)         # clipping adds nothing to a checkpoint
    assert len([k for k in ta if k.endswith("/Momentum")]) == 4
    for k in ta:
        assert np.array_equal(np.asarray(ta[k]), np.asarray(tb[k])), k
    assert not scalars(da, "global_norm") and len(scalars(db, "global_norm")) == 20


# ------------------------------------------------------------------ 4. parameter-server mode refuses
@pytest.mark.parametrize("job", ["ps", "worker"])
def test_ps_mode_refuses_clip_norm(job):
    t0 = time.time()
    r = run_main([f"--job_name={job}", "--ps_hosts=localhost:1", "--worker_hosts=localhost:2", "--clip_norm=1", "--cpu"],
                 timeout=60)
    dt = time.time() - t0
    out = r.stdout + r.stderr
    assert r.returncode != 0, out[-2000:]
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1 and "clip_norm" in lines[0] and "parameter-server mode" in lines[0], out[-2000:]
    assert "Traceback" not in out, out[-2000:]
    assert dt < 2.0, dt    # start-up only: refused before torch is imported or any socket is opened


# ------------------------------------------------------------------ 5. two data-parallel gloo ranks
def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, steps, B, out_q):
    import torch.distributed as dist
    torch.set_num_threads(1)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.parallel.dp import DataParallel
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import TorchNet
    spec = get_model("mlp", 1)
    opt = OptConfig(lr0=0.01, ema_max=0.9999, rule="adam", clip_norm=0.5)
    net = TorchNet(spec, B, "cpu", torch_ref.init_params(spec, seed=0), opt)
    dp = DataParallel(net, bucket_cap_mb=0.05)
    g = torch.Generator().manual_seed(321)
    scales = []
    for _ in range(steps):
        x = torch.rand(world * B, 28, 28, 1, generator=g) - 0.5
        y = torch.randint(0, 10, (world * B,), generator=g, dtype=torch.int32)
        net.x0.copy_(x[rank * B:(rank + 1) * B])
        net.labels.copy_(y[rank * B:(rank + 1) * B])
        dp.train_step()
        scales.append(net.read_stats()["clip_scale"])
    out_q.put((rank, net.fp.params.clone(), net.fp.mom.clone(), net.fp.gnorm[:2].clone(), scales))
    dist.barrier()
    dist.destroy_process_group()


def test_dp_two_gloo_ranks_stay_bitwise_equal():
    """The norm is taken after the all-reduce, of the averaged gradient: both ranks derive the
    same scale from bitwise-equal inputs and end with bitwise-equal parameters."""
    import torch.multiprocessing as mp
    world, B, steps = 2, 8, 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, steps, B, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict((r[0], r[1:]) for r in (q.get(timeout=240) for _ in range(world)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for a, b, name in zip(got[0][:3], got[1][:3], ("params", "adam m", "gnorm")):
        assert torch.equal(a, b), name
    assert got[0][3] == got[1][3] and any(s < 1.0 for s in got[0][3]), got[0][3]     # clipping was active


def test_dp_cli_chief_events_carry_global_norm(tmp_path):
    d = str(tmp_path / "train")
    env = dict(os.environ, OMP_NUM_THREADS="1", PYTHONUNBUFFERED="1", GLOO_SOCKET_IFNAME="lo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", os.path.join(ROOT, "main.py"),
           "--impl=torch", "--cpu", "--model=mlp", "--in_channels=1", "--batch_size=16", "--max_steps=6",
           "--test_interval=100", "--log_step_count_steps=0", "--save_summaries_steps=1",
           "--train_data=synthetic://1500", "--test_data=synthetic://300?seed=1", "--eval_examples=300",
           f"--train_dir={d}", "--collective_timeout=60", "--optimizer=adam", "--base_lr=0.001", "--clip_norm=0.5"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    gn, sc = scalars(d, "global_norm"), scalars(d, "clip_scale")
    assert sorted(gn) == list(range(1, 7)), sorted(gn)
    assert all(gn[k] > 0 and sc[k] * gn[k] <= 0.5 * (1 + 1e-5) for k in gn), (gn, sc)
    # both ranks print the same norm of the same averaged gradient
    results = [l for l in out.replace("result:", "\nresult:").splitlines() if l.startswith("result:")]
    norms = [tok for l in results for tok in l.split() if tok.startswith("global_norm=")]
    assert len(results) == 2 and len(norms) == 2 and norms[0] == norms[1], results
