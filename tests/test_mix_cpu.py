"""Mixup and CutMix, CPU side: validation of the four keys (parameter manager, ``MixConfig``, the
``main.py`` flags), the host tables and the sampler they feed, the host reference ``data/mix.py``
against the float64 oracle written from the formulas (tests/mix_oracle.py, which shares no code with the
package), the oracle's own proof that it tells a right kernel from a wrong one, the two-label loss of
``torch_ref`` and the CPU paths of the loader, ``TorchNet`` and the CLI."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_tensorflow_ibm_mnist_amd.data import mix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mix_oracle", os.path.join(ROOT, "tests", "mix_oracle.py"))
mo = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mo)

NAN, INF = float("nan"), float("inf")


@pytest.fixture
def pm():
    from distributed_tensorflow_ibm_mnist_amd.utils import parameter_mgr
    yield parameter_mgr
    parameter_mgr.configure({})


# ------------------------------------------------------------------ 1. validation
BAD = {
    "mixup_alpha": [-0.1, 0.05, 8.5, NAN, INF, True, "x", None],
    "cutmix_alpha": [-1, 0.0999, 9, NAN, -INF, False, "x", None],
    "mix_prob": [-0.01, 1.01, NAN, INF, True, "x", None],
    "mix_seed": [-1, 1 << 63, 2.5, True, "x"],
}
FIELD = {"mixup_alpha": "mixup_alpha", "cutmix_alpha": "cutmix_alpha", "mix_prob": "prob", "mix_seed": "seed"}


@pytest.mark.parametrize("key,bad", [(k, b) for k, vals in BAD.items() for b in vals])
def test_invalid_keys_raise_value_error(pm, key, bad):
    with pytest.raises(ValueError, match=key):
        M.MixConfig(**{FIELD[key]: bad})
    pm.configure({})
    pm.set_param(key, bad)
    getter = {"mixup_alpha": pm.getMixupAlpha, "cutmix_alpha": pm.getCutmixAlpha, "mix_prob": pm.getMixProb,
              "mix_seed": lambda: pm.getMixSeed(0)}[key]
    with pytest.raises(ValueError, match=key):
        getter()
    with pytest.raises(ValueError, match=key):
        pm.getMix(0)


def test_key_flag_and_getter_round_trip(pm):
    keys = set(BAD)
    assert keys <= set(pm.FLAG_KEYS) and keys <= set(pm.DEFAULTS)
    pm.configure({})
    cfg = pm.getMix(11)
    assert (cfg.mixup_alpha, cfg.cutmix_alpha, cfg.prob, cfg.seed) == (0.0, 0.0, 1.0, 11) and not cfg.enabled
    pm.configure({"mixup_alpha": 0.1, "cutmix_alpha": 8, "mix_prob": 0.5, "mix_seed": (1 << 63) - 1})
    cfg = pm.getMix(11)
    assert (cfg.mixup_alpha, cfg.cutmix_alpha, cfg.prob, cfg.seed) == (0.1, 8.0, 0.5, (1 << 63) - 1) and cfg.enabled
    # on needs a probability and an alpha
    assert not M.MixConfig(1.0, 1.0, 0.0).enabled and not M.MixConfig(0.0, 0.0, 1.0).enabled
    assert M.MixConfig(0.0, 0.2).enabled and M.MixConfig(0.2).enabled
    assert [M.prob_threshold(p) for p in (0.0, 0.25, 1.0, 1e-6)] == [0, 16384, 65536, 0]

    class Flags:        # the CLI: -1 is "unset", 0 a value
        config = os.path.join(ROOT, "configs", "lenet5_mix.yaml")
        mixup_alpha = cutmix_alpha = mix_prob = mix_seed = -1
    pm.configure_from_flags(Flags)
    cfg = pm.getMix(3)
    assert cfg.enabled and cfg.seed == 3 and cfg.mixup_alpha > 0 and cfg.cutmix_alpha > 0
    Flags.cutmix_alpha, Flags.mix_seed, Flags.mix_prob = 0.0, 9, 0.5
    pm.configure_from_flags(Flags)
    got = pm.getMix(3)
    assert (got.mixup_alpha, got.cutmix_alpha, got.prob, got.seed) == (cfg.mixup_alpha, 0.0, 0.5, 9)


CLI = ["--impl=torch", "--cpu", "--model=mlp", "--in_channels=1", "--batch_size=32", "--test_interval=1000",
       "--log_step_count_steps=0", "--train_data=synthetic://600", "--test_data=synthetic://100?seed=1",
       "--eval_examples=100"]
MIX_FLAGS = ["--mixup_alpha=0.4", "--cutmix_alpha=1.0", "--mix_prob=0.9", "--mix_seed=5"]


def _main(args, **kw):
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONUNBUFFERED="1")
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, **kw)


def test_cli_parses_the_flags_trains_and_refuses_bad_values(tmp_path):
    """main.py itself: the four flags go through flag parsing, the parameter manager and the trainer's
    start-up into a mixed run; a value outside the key's range ends the run naming the key."""
    r = _main(CLI + MIX_FLAGS + ["--max_steps=4", f"--train_dir={tmp_path / 'a'}"], timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "result: global_step=4" in r.stdout + r.stderr
    for bad, key in (("--mixup_alpha=9", "mixup_alpha"), ("--cutmix_alpha=0.05", "cutmix_alpha"),
                     ("--mix_prob=1.5", "mix_prob")):
        r = _main(CLI + [bad, "--max_steps=2", f"--train_dir={tmp_path / 'b'}"], timeout=120)
        assert r.returncode != 0 and key in r.stdout + r.stderr, (bad, (r.stdout + r.stderr)[-2000:])
    r = _main(CLI + ["--mix_seed=1.5", "--max_steps=2", f"--train_dir={tmp_path / 'c'}"], timeout=120)
    assert r.returncode != 0 and "mix_seed" in r.stdout + r.stderr     # an integer flag


def test_ps_worker_with_the_keys_is_not_refused(tmp_path):
    """--job_name=worker with the keys: one parameter server and one worker run to the end (a worker owns
    its loader and its loss, so nothing refuses the keys at start-up or later)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    base = s.getsockname()[1]
    s.close()
    common = CLI + MIX_FLAGS + ["--max_steps=6", "--optimizer=momentum", f"--train_dir={tmp_path / 'train'}",
                                f"--ps_hosts=localhost:{base}", f"--worker_hosts=localhost:{base + 100}"]
    env = dict(os.environ, OMP_NUM_THREADS="1", PYTHONUNBUFFERED="1")
    procs = []
    for job in ("ps", "worker"):
        log = open(tmp_path / f"{job}.log", "w")
        procs.append((job, subprocess.Popen([sys.executable, os.path.join(ROOT, "main.py")] + common +
                                            [f"--job_name={job}", "--task_id=0"], cwd=ROOT, env=env, stdout=log,
                                            stderr=subprocess.STDOUT)))
    for job, p in procs:
        try:
            p.wait(timeout=240)
        except subprocess.TimeoutExpired:
            for _, q in procs:
                q.kill()
            pytest.fail(f"{job} hung:\n" + open(tmp_path / f"{job}.log").read()[-3000:])
    logs = {job: open(tmp_path / f"{job}.log").read() for job, _ in procs}
    for job, p in procs:
        assert p.returncode == 0, logs[job][-3000:]
    assert "result: global_step=6" in logs["worker"] and "not supported" not in logs["worker"]


# ------------------------------------------------------------------ 2. the tables and the sampler
@pytest.mark.parametrize("alpha", mo.ALPHAS)
def test_table_shape_and_round_trip(alpha):
    T, S = M.lam_table(alpha), M.side_table(alpha)
    assert T.dtype == np.float32 and T.shape == (1025,) and S.dtype == np.int32 and S.shape == (1024,)
    assert T[0] == 0.5 and T[1024] == 1.0 and np.all(np.diff(T) >= 0)
    assert S.min() >= 0 and S.max() <= 19 and np.all(np.diff(S) <= 0)
    assert np.array_equal(T, mo.lam_table(alpha)) and np.array_equal(S, mo.side_table(alpha))
    lo, hi, q = mo.table_roundtrip(alpha)
    print(f"alpha={alpha}: widest round-trip bracket {np.max(hi - lo):.3e}")
    assert np.all(lo <= q) and np.all(q <= hi)
    with pytest.raises(ValueError, match="alpha"):
        M.lam_table(0.0)


@pytest.mark.parametrize("alpha", mo.ALPHAS)
def test_sampler_moments(alpha):
    """E[L (1 - L)] of Beta(a, a) is a / (2 (2 a + 1)); the table's interpolation bias is below 2e-5."""
    n = 65536
    prm = M.params(M.MixConfig(alpha, 0.0, 1.0, mo.SEED), 0, n)
    assert np.all(prm[:, 0] == M.MIXUP) and not prm[:, 2:].any()
    lam = prm[:, 1].copy().view(np.float32).astype(np.float64)
    assert lam.min() >= 0.5 and lam.max() <= 1.0
    v = lam * (1.0 - lam)
    err, se = abs(v.mean() - alpha / (2.0 * (2.0 * alpha + 1.0))), v.std(ddof=1) / np.sqrt(n)
    print(f"alpha={alpha}: |mean - exact| {err:.3e}, standard error {se:.3e}")
    assert err <= 5.0 * se


# ------------------------------------------------------------------ 3. params
CFGS = [(1.0, 0.0, 1.0), (0.0, 1.0, 1.0), (0.2, 4.0, 0.25), (4.0, 0.2, 1.0)]


@pytest.mark.parametrize("ma,ca,pr", CFGS)
def test_params_are_the_oracle_and_depend_on_the_position_alone(ma, ca, pr):
    cfg = M.MixConfig(ma, ca, pr, mo.SEED)
    for pos0, n in ((0, 300), ((1 << 32) - 3, 7), ((1 << 40) + 5, 300)):
        got = M.params(cfg, pos0, n)
        assert got.dtype == np.int32 and np.array_equal(got, mo.params(ma, ca, pr, mo.SEED, pos0, n))
        # the same entries at another pos0 / b split
        assert np.array_equal(got[3:], M.params(cfg, pos0 + 3, n - 3))
    assert not np.array_equal(M.params(cfg, 0, 64), M.params(cfg.with_seed(mo.SEED + 1), 0, 64))
    assert not np.array_equal(M.params(cfg, 0, 64), M.params(cfg, 1 << 32, 64))
    with pytest.raises(ValueError, match="pos0"):
        M.params(cfg, -1, 4)


def test_probability_and_the_switch():
    """mix_prob = 0.25 applies to 0.25 of the entries and, with both alphas set, half of the applied ones
    cut, both within 5 standard errors.  `apply` and the switch are bits of the first Philox word, read
    here off the oracle's own Philox: an applied CutMix entry whose box is empty comes out unmixed, which
    is a property of the box and not of the two probabilities."""
    n = 65536
    p = np.uint64(0) + np.arange(n, dtype=np.uint64)
    w0 = mo.philox(p & np.uint64(0xFFFFFFFF), p >> np.uint64(32), 0, M.TAG, 7, 0)[0]
    apply = (w0 >> np.uint64(16)).astype(np.int64) < M.prob_threshold(0.25)
    cutbit = (w0 & np.uint64(1)) == 1
    assert abs(apply.mean() - 0.25) <= 5.0 * np.sqrt(0.25 * 0.75 / n)
    assert abs(cutbit[apply].mean() - 0.5) <= 5.0 * np.sqrt(0.25 / apply.sum())
    # params follows exactly these bits: mixup alone is the apply bit, both keys split it by the switch
    one = M.params(M.MixConfig(1.0, 0.0, 0.25, 7), 0, n)
    assert np.array_equal(one[:, 0] != M.UNMIXED, apply)
    prm = M.params(M.MixConfig(1.0, 1.0, 0.25, 7), 0, n)
    assert np.array_equal(prm[:, 0] == M.MIXUP, apply & ~cutbit)
    cm = prm[:, 0] == M.CUTMIX
    assert not (cm & ~(apply & cutbit)).any() and (apply & cutbit & ~cm).sum() <= 1e-3 * n     # the empty boxes
    applied = prm[:, 0] != M.UNMIXED
    un = prm[~applied]
    assert np.all(un[:, 1].copy().view(np.float32) == 1.0) and not un[:, 2:].any()
    assert np.all(M.params(M.MixConfig(1.0, 0.0, 1.0, 7), 0, 4096)[:, 0] == M.MIXUP)
    # the tag: dropout's counter word of a layer no model has
    from distributed_tensorflow_ibm_mnist_amd.data import augment as A
    assert M.TAG == 0x41554702 == A.ELASTIC_TAG + 1 and M.TAG >> 16 == 16725


# ------------------------------------------------------------------ 4. mixed
@pytest.mark.parametrize("nb", [1, 2, 7, 77])
@pytest.mark.parametrize("ma,ca,pr", [(1.0, 0.0, 1.0), (0.0, 1.0, 1.0), (0.2, 4.0, 0.75)])
def test_mixed_is_the_oracle_and_has_its_properties(nb, ma, ca, pr):
    C = 3 if nb == 7 else 1
    x, y = mo.image_inputs(nb, C)
    cfg = M.MixConfig(ma, ca, pr, mo.SEED)
    out, l2, lam = M.mixed(x, y, cfg, mo.IMAGE_POS0)
    kind, wlam, box = mo.batch_draws(ma, ca, pr, mo.SEED, mo.IMAGE_POS0, nb)
    want, wl2, _ = mo.mixed(x, y, kind, wlam, box)
    assert out.dtype == np.float64 and np.array_equal(out, want) and np.array_equal(l2, wl2)
    assert lam.dtype == np.float32 and np.array_equal(lam, wlam)
    x64, xb = x.astype(np.float64).reshape(nb, 28, 28, C), x.astype(np.float64)[::-1].reshape(nb, 28, 28, C)
    o4 = out.reshape(nb, 28, 28, C)
    for b in range(nb):
        if kind[b] == mo.UNMIXED:
            assert np.array_equal(o4[b], x64[b]) and lam[b] == 1.0 and l2[b] == y[b]
        elif kind[b] == mo.CUTMIX:
            x0, x1, y0, y1 = box[b]
            inside = np.zeros((28, 28), bool)
            inside[y0:y1, x0:x1] = True
            assert np.array_equal(o4[b][inside], xb[b][inside]) and np.array_equal(o4[b][~inside], x64[b][~inside])
            area = (x1 - x0) * (y1 - y0)
            assert area > 0 and lam[b] == np.float32(784 - area) / np.float32(784) and l2[b] == y[nb - 1 - b]
        else:
            assert 0.5 <= lam[b] <= 1.0 and l2[b] == y[nb - 1 - b]
    if nb % 2:      # nb = 1 and the middle entry of an odd batch
        m = nb // 2
        assert np.array_equal(o4[m], x64[m]) and lam[m] == 1.0 and l2[m] == y[m]
    if nb > 1 and pr == 1.0:
        assert (kind != mo.UNMIXED).sum() >= nb - 2


def test_error_budget_and_wrong_kernels():
    """E32 of the mixup blend on the GPU tests' inputs, and the two wrong kernels of the issue: both
    exceed half a bf16 ulp + 4 * E32 by orders of magnitude."""
    E = mo.e32()
    print(f"E32 = {E:.3e}")
    assert 0.0 < E < 2.0 ** -23
    for bug, ratio in mo.self_check(E).items():
        assert ratio > 1e3, (bug, ratio)


# ------------------------------------------------------------------ 5. torch_ref.losses with two labels
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_torch_ref_two_label_loss(eps):
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    spec = get_model("mlp", 1)
    params = torch_ref.init_params(spec, seed=0)
    rng = np.random.default_rng(5)
    n = 64
    z = torch.randn(n, 10, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) * 3
    ya, yb = (torch.from_numpy(rng.integers(0, 10, n)) for _ in range(2))
    yb[:8] = ya[:8]
    lam = torch.from_numpy(mo.lam_vector(rng, n))
    got = torch_ref.losses(spec, params, z, ya, eps, labels2=yb, lam=lam)["cross_entropy"]
    rows = lam.double() * F.cross_entropy(z, ya, label_smoothing=eps, reduction="none") \
        + (1 - lam.double()) * F.cross_entropy(z, yb, label_smoothing=eps, reduction="none")
    assert abs(got.item() - rows.mean().item()) <= 1e-12
    assert abs(got.item() * n - mo.ce_sum(z, ya, yb, lam, eps)) <= 1e-9
    one = torch_ref.losses(spec, params, z, ya, eps, labels2=ya, lam=torch.ones(n))["cross_entropy"]
    assert abs(one.item() - torch_ref.losses(spec, params, z, ya, eps)["cross_entropy"].item()) <= 1e-12
    with pytest.raises(ValueError, match="labels2"):
        torch_ref.losses(spec, params, z, ya, eps, labels2=yb)


# ------------------------------------------------------------------ 6. the loader, CPU path
N_DS = 192


@pytest.fixture(scope="module")
def ds():
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceDataset
    rng = np.random.default_rng(9)
    return DeviceDataset(torch.from_numpy(rng.integers(0, 256, (N_DS, 784), dtype=np.uint8)), torch.arange(N_DS) % 10,
                         "cpu")


def _loader(ds, B, cfg, **kw):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceLoader
    return DeviceLoader(ds, torch.full((B, 28, 28, 1), 7.0), torch.full((B,), -77, dtype=torch.int32), mix=cfg,
                        out_labels2=torch.full((B,), -55, dtype=torch.int32), out_lam=torch.full((B,), -3.0), **kw)


def test_loader_mixes_the_gathered_batch_and_seek_resumes(ds):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import perm_positions
    cfg = M.MixConfig(0.4, 1.0, 0.9, 21)
    run = _loader(ds, 16, cfg, seed=4)
    assert run.lookahead_job() is None
    seen = []
    for k in range(3):
        assert run.next() == 16
        seen.append([t.clone() for t in (run.out_images, run.out_labels, run.out_labels2, run.out_lam)])
        rows = perm_positions(16 * k, 16, N_DS, 4)
        plain = (ds.images[rows].float() * (1.0 / 255.0) - 0.5).view(16, 784, 1).numpy()
        lab = (rows % 10).numpy().astype(np.int32)
        d = mo.batch_draws(0.4, 1.0, 0.9, 21, 16 * k, 16)
        want, l2, lam = mo.mixed(plain, lab, *d)
        got = run.out_images.double().numpy().reshape(16, 784, 1)
        assert np.all(np.abs(got - want) <= np.abs(want) * 2.0 ** -24 + 1e-45)       # one fp32 rounding
        assert np.array_equal(run.out_labels.numpy(), lab) and np.array_equal(run.out_labels2.numpy(), l2)
        assert np.array_equal(run.out_lam.numpy(), lam)
    other = _loader(ds, 16, cfg, seed=4)
    other.seek(2)
    other.next()
    for a, b in zip(seen[2], (other.out_images, other.out_labels, other.out_labels2, other.out_lam)):
        assert torch.equal(a, b)
    # a partial batch flips itself and leaves the rows past it alone
    run.out_images.fill_(7.0)
    run.out_lam.fill_(-3.0)
    assert run.next(5) == 5 and torch.all(run.out_images[5:] == 7.0) and torch.all(run.out_lam[5:] == -3.0)
    assert run.out_lam[2] == 1.0 and run.out_labels2[2] == run.out_labels[2]


def test_loader_refusals_and_the_plain_path(ds):
    cfg = M.MixConfig(1.0, 0.0, 1.0, 5)
    with pytest.raises(ValueError, match="idx_out"):
        _loader(ds, 16, cfg, idx_out=torch.zeros(16, dtype=torch.int64))
    off = _loader(ds, 16, M.MixConfig(seed=5), seed=4, idx_out=torch.zeros(16, dtype=torch.int64))
    assert off.mix is None
    plain, zero = _loader(ds, 16, None, seed=4), _loader(ds, 16, M.MixConfig(1.0, 1.0, 0.0), seed=4)
    assert zero.mix is None
    for ld in (plain, zero):
        ld.next()
    assert torch.equal(plain.out_images, zero.out_images) and torch.all(zero.out_lam == -3.0)
    # sharded ranks flip their own local batch and draw from global positions; unsharded ones offset the seed
    two = [_loader(ds, 8, cfg, seed=4, rank=r, world=2) for r in (0, 1)]
    assert two[0].mix.seed == two[1].mix.seed == 5
    for ld in two:
        ld.next()
    for r, ld in enumerate(two):
        assert np.array_equal(ld.out_lam.numpy(), mo.batch_draws(1.0, 0.0, 1.0, 5, 8 * r, 8)[1])
        assert torch.equal(ld.out_labels2, ld.out_labels.flip(0))
    solo = [_loader(ds, 8, cfg, seed=4, rank=r, world=2, shard=False) for r in (0, 1)]
    assert solo[0].mix.seed == 5 and solo[1].mix.seed == 5 + 7919
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceLoader
    with pytest.raises(ValueError, match="out_labels2"):
        DeviceLoader(ds, torch.zeros(8, 28, 28, 1), torch.zeros(8, dtype=torch.int32), mix=cfg)


# ------------------------------------------------------------------ 7. TorchNet, HipNetF32, the replica
def test_torchnet_takes_a_mixed_step_and_f32_refuses():
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor_f32 import HipNetF32
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import TorchNet
    spec = get_model("mlp", 1)
    init = torch_ref.init_params(spec, seed=0)
    B = 32
    net = TorchNet(spec, B, "cpu", init, OptConfig(lr0=0.05, mix=True, label_smoothing=0.1))
    plain = TorchNet(spec, B, "cpu", init, OptConfig(lr0=0.05, label_smoothing=0.1))
    assert plain.labels2 is None and plain.mix_lam is None
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 28, 28, 1, generator=g) - 0.5
    ya, yb = (torch.randint(0, 10, (B,), generator=g, dtype=torch.int32) for _ in range(2))
    lam = torch.from_numpy(mo.lam_vector(np.random.default_rng(2), B))
    for n in (net, plain):
        n.x0.copy_(x)
        n.labels.copy_(ya)
    net.labels2.copy_(yb)
    net.mix_lam.copy_(lam)
    net.forward()
    net.loss_and_grad()
    net.backward()
    p = {k: v.clone().requires_grad_(True) for k, v in init.items()}
    lg, _ = torch_ref.forward(spec, p, x)
    torch_ref.losses(spec, p, lg, ya, 0.1, labels2=yb, lam=lam)["cross_entropy"].backward()
    for name in init:
        assert torch.allclose(net.fp.grad_view(name), p[name].grad, rtol=1e-4, atol=1e-7), name
    assert abs(net.stats[0].item() - mo.ce_sum(lg.detach(), ya, yb, lam, 0.1)) <= 1e-3
    before = net.fp.params.clone()
    net.update()
    assert not torch.equal(before, net.fp.params) and int(net.fp.step.item()) == 1
    # eval stays hard-label: bitwise the plain net's on the same parameters
    plain.fp.params.copy_(net.fp.params)
    assert torch.equal(net.eval_batch(B)[:2], plain.eval_batch(B)[:2])
    with pytest.raises(ValueError, match="mixup_alpha"):
        HipNetF32(spec, B, "cpu", init, OptConfig(mix=True))
    with pytest.raises(ValueError, match="mix"):
        OptConfig(mix=1)


def test_replica_cpu_trains_mixed_and_evaluates_plain():
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica
    spec = get_model("mlp", 1)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.integers(0, 256, (N_DS, 784), dtype=np.uint8))
    y = torch.arange(N_DS) % 10
    cfg = M.MixConfig(0.4, 1.0, 1.0, 21)
    lines = []

    def make(mix, mode="prep"):
        return Replica(spec, "torch", 64, "cpu", torch_ref.init_params(spec, seed=0),
                       OptConfig(lr0=0.01, mix=mix is not None and mix.enabled), x, y, 1, x[:64], y[:64], seed=5,
                       use_graph=False, fused_input=mode, mix=mix, log=lines.append)
    a, b = make(cfg, "bf16"), make(None)
    assert len(lines) == 1 and "prep" in lines[0] and a.mix is cfg and b.mix is None
    assert a.evaluate() == b.evaluate()
    a.step()
    b.step()
    d = mo.batch_draws(0.4, 1.0, 1.0, 21, 0, 64)
    assert np.array_equal(a.net.mix_lam.numpy(), d[1]) and torch.equal(a.net.labels, b.net.labels)
    want, l2, _ = mo.mixed(b.net.x0.double().numpy().reshape(64, 784, 1), b.net.labels.numpy(), *d)
    got = a.net.x0.double().numpy().reshape(64, 784, 1)
    assert np.all(np.abs(got - want) <= np.abs(want) * 2.0 ** -23 + 1e-45)
    assert np.array_equal(a.net.labels2.numpy(), l2) and not torch.equal(a.net.fp.params, b.net.fp.params)
    with pytest.raises(ValueError, match="mix"):
        Replica(spec, "torch", 64, "cpu", torch_ref.init_params(spec, seed=0), OptConfig(lr0=0.01), x, y, 1, seed=5,
                use_graph=False, mix=cfg, log=lines.append)
