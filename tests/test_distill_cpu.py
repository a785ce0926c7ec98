"""Knowledge distillation without a GPU: the float64 oracle (tests/distill_oracle.py) against
``torch_ref`` and ``torch.nn.functional.kl_div``, the validation of the keys, ``TorchNet`` training with a
teacher, and the ``Teacher`` restoring a checkpoint written by the project's own ``Saver``."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_tensorflow_ibm_mnist_amd.ckpt.saver import Saver
from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
from distributed_tensorflow_ibm_mnist_amd.runtime.teacher import Teacher, TeacherSource
from distributed_tensorflow_ibm_mnist_amd.runtime.torchnet import TorchNet
from distributed_tensorflow_ibm_mnist_amd.train.replica import state_tensors
from distributed_tensorflow_ibm_mnist_amd.utils import parameter_mgr as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("distill_oracle", os.path.join(ROOT, "tests", "distill_oracle.py"))
do = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(do)

AT = [(1.0, 1.0), (0.5, 2.0), (0.25, 8.0), (0.5, 0.5)]


def _rows(nb, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nb, 10)) * scale, rng.standard_normal((nb, 10)) * scale,
            rng.integers(0, 10, nb).astype(np.int32))


@pytest.mark.parametrize("a,T", AT)
@pytest.mark.parametrize("nb", [1, 77, 300])
def test_oracle_matches_torch(nb, a, T):
    z, t, y = _rows(nb, nb)
    o = do.distill(z, t, y, a, T, 1.0 / nb)
    zt = torch.from_numpy(z).requires_grad_(True)
    tt, yt = torch.from_numpy(t), torch.from_numpy(y)
    rows = torch_ref.distillation_loss(zt, yt, tt, a, T)
    # the definition's torch form: T^2 kl_div(log_softmax(l / T), softmax(t / T), batchmean) + (1 - a) CE
    kl = F.kl_div(F.log_softmax(zt / T, 1), F.softmax(tt / T, 1), reduction="batchmean")
    whole = (1 - a) * F.cross_entropy(zt, yt.long()) + a * T * T * kl
    assert np.allclose(rows.detach().numpy(), o.rows, rtol=1e-12, atol=1e-12)
    assert abs(whole.item() * nb - o.loss) <= 1e-10 * max(1.0, abs(o.loss))
    assert abs(o.loss - (o.hard + o.ces - o.hq)) <= 1e-9 * (abs(o.hard) + abs(o.ces) + abs(o.hq))
    assert abs(o.soft - (o.ces - o.hq)) <= 1e-9 * (abs(o.ces) + abs(o.hq))
    (rows.sum() / nb).backward()
    assert np.allclose(zt.grad.numpy(), o.dl, rtol=1e-10, atol=1e-13)
    spec = get_model("mlp", 1)
    got = torch_ref.losses(spec, torch_ref.init_params(spec, seed=0), torch.from_numpy(z), yt, teacher_logits=tt,
                           distill_alpha=a, distill_temperature=T)
    assert abs(got["cross_entropy"].item() * nb - o.loss) <= 1e-9 * max(1.0, abs(o.loss))


def test_alpha_zero_is_the_plain_loss_exactly():
    z, t, y = _rows(77, 5)
    o = do.distill(z, t, y, 0.0, 4.0)
    plain = do.distill(z, z, y, 0.0, 1.0)
    assert o.loss == plain.loss and np.array_equal(o.dl, plain.dl) and o.soft == 0.0 and o.ces == 0.0
    spec = get_model("mlp", 1)
    params = torch_ref.init_params(spec, seed=0)
    zt, yt = torch.from_numpy(z).float(), torch.from_numpy(y)
    a = torch_ref.losses(spec, params, zt, yt, teacher_logits=torch.from_numpy(t).float(), distill_alpha=0.0,
                         distill_temperature=4.0)
    b = torch_ref.losses(spec, params, zt, yt)
    assert torch.equal(a["cross_entropy"], b["cross_entropy"]) and torch.equal(a["total_loss"], b["total_loss"])


@pytest.mark.parametrize("a,T", AT)
def test_identical_rows_have_no_soft_part(a, T):
    z, _, y = _rows(77, 9)
    o = do.distill(z, z, y, a, T)
    hard = do.distill(z, z, y, 0.0, 1.0)
    assert o.soft == 0.0 and abs(o.ces - o.hq) <= 1e-9 * abs(o.ces)
    assert np.array_equal(o.dl, (1.0 - a) * hard.dl)
    zt = torch.from_numpy(z)
    rows = torch_ref.distillation_loss(zt, torch.from_numpy(y), zt.clone(), a, T)
    assert torch.allclose(rows, (1.0 - a) * F.cross_entropy(zt, torch.from_numpy(y).long(), reduction="none"), rtol=0, atol=1e-14)


TEACHER_SCALE = 5.0      # tests/test_distill_gpu.py draws its teachers at this scale


@pytest.mark.parametrize("student_scale", [2.0, 3.0])
@pytest.mark.parametrize("nb", [33, 77, 300])
def test_the_bounds_discriminate_and_fp32_fits(nb, student_scale):
    """The logit scales of the GPU tests (students: standard normal times 3 in the layered kernels, about 2
    out of the fused heads; teachers: times 5): over several draws the loss bound and the bf16 dl bound tell
    a wrong temperature and the plain hard-label loss from the right ones by more than 10 x (at equal
    scales of 3 the margin of (0.25, 8) shrank to 3 x: T^2 KL came out near the hard loss).  A float32
    transcription of the definition uses a small share of the loss bound."""
    worst, margin = 0.0, np.inf
    for seed in range(6):
        rng = np.random.default_rng(1000 * seed + nb)
        z = (rng.standard_normal((nb, 10)) * student_scale).astype(np.float32).astype(np.float64)
        t = (rng.standard_normal((nb, 10)) * TEACHER_SCALE).astype(np.float32).astype(np.float64)
        y = rng.integers(0, 10, nb)
        for a, T in AT:
            o = do.distill(z, t, y, a, T, 1.0 / nb)
            tol = do.loss_tol(o)
            worst = max(worst, abs(do.distill_f32(z, t, y, a, T) - o.loss) / tol)
            others = [do.distill(z, t, y, 0.0, 1.0, 1.0 / nb)] + ([do.distill(z, t, y, a, 1.0, 1.0 / nb)] if T != 1.0 else [])
            for w in others:
                margin = min(margin, abs(w.loss - o.loss) / tol, np.abs(w.dl - o.dl).max() / (2.0 ** -8 * np.abs(o.dl).max()))
    print(f"nb={nb} scale={student_scale}: float32 transcription {100 * worst:.3f} % of the loss bound at worst; "
          f"smallest margin {margin:.1f} x the bound")
    assert margin > 20.0      # twice what the GPU tests ask for
    assert worst < 0.05


def test_edge_rows_in_the_oracle():
    z, _, y = _rows(8, 3)
    t = np.full((8, 10), -80.0)
    t[np.arange(8), np.arange(8)] = 80.0
    o = do.distill(z, t, y, 0.5, 0.5)
    assert np.isfinite(o.loss) and np.isfinite(o.dl).all()
    for v in (np.nan, np.inf):
        bad = t.copy()
        bad[3, 2] = v
        assert not np.isfinite(do.distill(z, bad, y, 0.5, 2.0).loss)
    zi = z.copy()
    zi[3, 2] = np.inf
    assert not np.isfinite(do.distill(zi, t, y, 0.5, 2.0).loss)


# ------------------------------------------------------------------ the keys
def test_optconfig_validates():
    assert OptConfig().distill_alpha == 0.0 and OptConfig().distill_temperature == 2.0
    ok = OptConfig(distill_alpha=1, distill_temperature=8)
    assert ok.distill_alpha == 1.0 and ok.distill_temperature == 8.0
    for kw, key in ((dict(distill_alpha=-0.1), "distill_alpha"), (dict(distill_alpha=1.01), "distill_alpha"),
                    (dict(distill_alpha=float("nan")), "distill_alpha"), (dict(distill_alpha="x"), "distill_alpha"),
                    (dict(distill_alpha=True), "distill_alpha"), (dict(distill_temperature=0), "distill_temperature"),
                    (dict(distill_temperature=-1.0), "distill_temperature"),
                    (dict(distill_temperature=float("inf")), "distill_temperature"),
                    (dict(distill_temperature=1e20), "distill_temperature"),
                    (dict(distill_temperature=float("nan")), "distill_temperature"),
                    (dict(distill_alpha=0.5, label_smoothing=0.1), "label_smoothing"),
                    (dict(distill_alpha=0.5, mix=True), "mix"), (dict(distill_alpha=0.5, dropout=0.2), "dropout")):
        with pytest.raises(ValueError, match=key) as e:
            OptConfig(**kw)
        assert "distill_" in str(e.value)
    # off: the other keys combine as before
    OptConfig(distill_alpha=0.0, label_smoothing=0.1, mix=True, dropout=0.2)


@pytest.fixture
def params_mgr():
    pm.configure({})
    yield pm
    pm.configure({})


def test_parameter_manager_keys(params_mgr, tmp_path):
    d = pm.getDistill()
    assert not d.enabled and d.alpha == 0.0 and d.temperature == 2.0 and d.ckpt_dir == "" and not d.use_ema
    pm.configure({"distill_from": str(tmp_path), "distill_model": "reference_cnn"})
    d = pm.getDistill()
    assert d.enabled and d.alpha == 0.5 and d.temperature == 2.0 and d.model == "reference_cnn"
    pm.configure({"distill_from": str(tmp_path), "distill_model": "mlp", "distill_alpha": 0.25, "distill_temperature": 4,
                  "distill_use_ema": 1})
    d = pm.getDistill()
    assert (d.alpha, d.temperature, d.use_ema) == (0.25, 4.0, True)
    pm.configure({"distill_from": str(tmp_path), "distill_model": "mlp", "distill_alpha": 0.0})
    assert not pm.getDistill().enabled
    bad = [({"distill_from": str(tmp_path)}, "distill_model"), ({"distill_model": "mlp"}, "distill_from"),
           ({"distill_alpha": 0.5}, "distill_from"),
           ({"distill_from": str(tmp_path), "distill_model": "mlp", "distill_alpha": 1.5}, "distill_alpha"),
           ({"distill_from": str(tmp_path), "distill_model": "mlp", "distill_temperature": 0}, "distill_temperature"),
           ({"distill_temperature": "hot"}, "distill_temperature"),
           ({"distill_from": str(tmp_path), "distill_model": "mlp", "distill_use_ema": 2}, "distill_use_ema"),
           ({"distill_from": 3, "distill_model": "mlp"}, "distill_from"),
           ({"distill_from": str(tmp_path), "distill_model": "mlp", "label_smoothing": 0.1}, "label_smoothing"),
           ({"distill_from": str(tmp_path), "distill_model": "mlp", "mixup_alpha": 0.4}, "mixup_alpha"),
           ({"distill_from": str(tmp_path), "distill_model": "mlp", "cutmix_alpha": 1.0}, "cutmix_alpha"),
           ({"distill_from": str(tmp_path), "distill_model": "mlp", "dropout": 0.5}, "dropout")]
    for cfg, key in bad:
        pm.configure(cfg)
        with pytest.raises(ValueError, match=key):
            pm.getDistill()
    with pytest.raises(ValueError, match="distill_typo"):
        pm.configure({"distill_typo": 1})
    for k in ("distill_from", "distill_model", "distill_alpha", "distill_temperature", "distill_use_ema"):
        assert k in pm.FLAG_KEYS and k in pm.DEFAULTS
    with pytest.raises(ValueError, match="distill_from"):
        TeacherSource(str(tmp_path / "missing"), "mlp")
    with pytest.raises(ValueError, match="distill_model"):
        TeacherSource(str(tmp_path), "")


# ------------------------------------------------------------------ TorchNet and the Teacher
B = 16


def _student(alpha=0.5, T=2.0, model="mlp"):
    spec = get_model(model, 1)
    init = torch_ref.init_params(spec, seed=2)
    net = TorchNet(spec, B, "cpu", init, OptConfig(lr0=0.05, distill_alpha=alpha, distill_temperature=T))
    g = torch.Generator().manual_seed(4)
    net.x0.copy_(torch.rand(B, 28, 28, 1, generator=g) - 0.5)
    net.labels.copy_(torch.randint(0, 10, (B,), generator=g, dtype=torch.int32))
    return spec, init, net


def test_torchnet_trains_against_a_teacher():
    spec, init, net = _student()
    with pytest.raises(RuntimeError, match="teacher_logits"):
        net.forward()
        net.loss_and_grad()
    tspec = get_model("lenet5", 1)
    teacher = Teacher(tspec, torch_ref.init_params(tspec, seed=7), net, "torch")
    assert teacher.net.x0 is net.x0 and net.teacher_logits is teacher.logits
    before = teacher.net.fp.params.clone()
    for step in range(2):
        t = teacher.forward().clone()
        want_t, _ = torch_ref.forward(tspec, {k: v for k, v in teacher.net._params(teacher.net.fp.params).items()},
                                      net.x0.float())
        assert torch.equal(t, want_t.float())
        net.forward()
        net.loss_and_grad()
        net.backward()
        # the oracle's dlogits pushed back through the reference forward
        p = {e.name: net.fp.params[e.off:e.off + e.n].view(e.shape).clone().requires_grad_(True) for e in net.fp.entries}
        lg, _ = torch_ref.forward(spec, p, net.x0.float())
        o = do.distill(lg.detach().numpy(), t.numpy(), net.labels.numpy(), 0.5, 2.0, 1.0 / B)
        lg.backward(torch.from_numpy(o.dl).float())
        for e in net.fp.entries:
            got, want = net.fp.grads[e.off:e.off + e.n].view(e.shape), p[e.name].grad
            assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item() + 1e-7, e.name
        assert abs(net.stats[0].item() - o.loss) <= do.loss_tol(o)
        net.update()
        assert net.read_stats()["nan"] == 0.0
    assert int(net.fp.step.item()) == 2 and torch.equal(before, teacher.net.fp.params)
    # eval stays the plain cross-entropy
    st = torch.zeros(8)
    net.eval_batch(B, st)
    lg = net.forward(B, grad=False)
    assert abs(st[0].item() - F.cross_entropy(lg, net.labels.long(), reduction="sum").item()) < 1e-4


@pytest.mark.parametrize("use_ema", [False, True])
def test_teacher_restores_a_saver_checkpoint(tmp_path, use_ema):
    tspec = get_model("lenet5", 1)
    src = TorchNet(tspec, B, "cpu", torch_ref.init_params(tspec, seed=11), OptConfig(lr0=0.1))
    g = torch.Generator().manual_seed(1)
    src.x0.copy_(torch.rand(B, 28, 28, 1, generator=g) - 0.5)
    src.labels.copy_(torch.randint(0, 10, (B,), generator=g, dtype=torch.int32))
    for _ in range(3):      # the EMA shadows leave the weights behind
        src.train_step()
    Saver().save(str(tmp_path), 3, state_tensors(src), meta={"model": "lenet5", "in_channels": 1})
    assert not torch.equal(src.fp.params, src.fp.ema)
    _, _, net = _student()
    teacher = TeacherSource(str(tmp_path), "lenet5", use_ema)(net, "torch")
    want = src.fp.ema if use_ema else src.fp.params
    assert torch.equal(teacher.net.fp.params, want)
    teacher.forward()
    ref, _ = torch_ref.forward(tspec, src._params(want), net.x0.float())
    assert torch.equal(teacher.logits, ref.float())
    os.mkdir(tmp_path / "empty")
    with pytest.raises(ValueError, match="no checkpoint"):
        TeacherSource(str(tmp_path / "empty"), "lenet5")(net, "torch")


def test_spec_mismatch_raises():
    _, _, net = _student()
    tspec = get_model("lenet5", 3)
    with pytest.raises(ValueError, match="lenet5.*mlp"):
        Teacher(tspec, torch_ref.init_params(tspec, seed=0), net, "torch")
    with pytest.raises(ValueError, match="x0"):
        TorchNet(get_model("mlp", 1), B, "cpu", torch_ref.init_params(get_model("mlp", 1), seed=0), x0=torch.zeros(3, 28, 28, 1))
