"""Elastic distortion, CPU side: the host reference (``data/augment.py``: the draws, the Gaussian table,
the float64 field and warp), validation of the two ``augment_elastic_*`` keys, the proof that the oracle
tells a right kernel from a wrong one, the error budget the GPU tests hold the device to, and the loader
on the CPU path (alpha = 0 untouched)."""
import math
import os

import numpy as np
import pytest
import torch

import augment_oracle as O
import elastic_oracle as E
from distributed_tensorflow_ibm_mnist_amd.data import augment as A
from distributed_tensorflow_ibm_mnist_amd.ops import dropout as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def pm():
    from distributed_tensorflow_ibm_mnist_amd.utils import parameter_mgr
    yield parameter_mgr
    parameter_mgr.configure({})


# ------------------------------------------------------------------ 1. draws and table
def test_draws_follow_the_indexing():
    """A plain-loop transcription of e -> (counter, word, half) for a handful of (p, e)."""
    seed = O.SEED                                        # 40 bits: the high key word is in use
    cfg = A.AugmentConfig(seed=seed, elastic_alpha=1.0)
    for p in (0, 5, (1 << 32) - 3, (1 << 40) + 5):
        got = A.elastic_draws(cfg, p, 1)
        assert got.dtype == np.uint16 and got.shape == (1, 2, 28, 28)
        for f, i, j in ((0, 0, 0), (0, 0, 7), (0, 0, 8), (0, 27, 27), (1, 0, 0), (1, 13, 5), (1, 27, 27), (0, 9, 22)):
            e = f * 784 + 28 * i + j
            w = D.philox4x32_10((p & 0xFFFFFFFF, p >> 32, e >> 3, 0x41554701), (seed & 0xFFFFFFFF, seed >> 32))
            want = (int(w[(e & 7) >> 1]) >> (16 * (e & 1))) & 0xFFFF
            assert int(got[0, f, i, j]) == want, (p, f, i, j)
    # a field belongs to the position: a batch is a window of the stream
    assert np.array_equal(A.elastic_draws(cfg, (1 << 32) - 3, 6)[3], A.elastic_draws(cfg, 1 << 32, 1)[0])
    assert A.ELASTIC_TAG == 0x41554701 and A.ELASTIC_TAG != A.TAG
    with pytest.raises(ValueError, match="pos0"):
        A.elastic_draws(cfg, -1, 1)


def test_draws_are_uniform_and_the_planes_independent():
    n = 64
    d = A.elastic_draws(A.AugmentConfig(seed=77, elastic_alpha=1.0), 12345, n).astype(np.float64)
    count = d[:, 0].size
    sd = 65536.0 / math.sqrt(12.0)                       # of one uniform 16-bit draw
    for f in (0, 1):
        assert abs(d[:, f].mean() - 32767.5) <= 5 * sd / math.sqrt(count)
    assert abs(np.corrcoef(d[:, 0].ravel(), d[:, 1].ravel())[0, 1]) <= 5 / math.sqrt(count)
    assert d.min() < 100 and d.max() > 65435


def test_r_is_exact_and_symmetric():
    d = np.arange(65536, dtype=np.uint16)
    r = (d.astype(np.float32) - np.float32(32767.5)) * np.float32(2.0 ** -15)
    assert np.array_equal(r.astype(np.float64), (d.astype(np.float64) - 32767.5) * 2.0 ** -15)   # exact in fp32
    assert np.array_equal(r, -r[::-1]) and r.min() > -1 and r.max() < 1 and not np.any(r == 0)


@pytest.mark.parametrize("sigma", [0.5, 1.0, 4.0, 8.0])
def test_weights(sigma):
    w = A.elastic_weights(sigma)
    K = math.ceil(3 * sigma)
    assert w.dtype == np.float32 and w.shape == (K + 1,) and 2 <= K <= 24
    assert abs(float(w[0]) + 2.0 * float(w[1:].astype(np.float64).sum()) - 1.0) < 1e-6
    assert np.all(np.diff(w) < 0) and w[-1] > 0
    k = np.arange(K + 1)
    assert np.allclose(w / w[0], np.exp(-k * k / (2.0 * sigma * sigma)), rtol=1e-6)


@pytest.mark.parametrize("sigma", [0.5, 4.0])
def test_field_of_one_draw_is_the_outer_product_of_the_table(sigma):
    """At the centre the whole kernel; at a corner the same cut off (zero extension, nothing reflected)."""
    w = A.elastic_weights(sigma).astype(np.float64)
    K = len(w) - 1
    full = np.concatenate([w[:0:-1], w])                 # w_K .. w_0 .. w_K
    for (ci, cj) in ((14, 13), (0, 0), (27, 2)):
        r = np.zeros((1, 2, 28, 28))
        r[0, 1, ci, cj] = 1.0
        d = A._smooth(r, w.astype(np.float32), 3.0, np.float64)
        want = np.zeros((28, 28))
        for i in range(28):
            for j in range(28):
                if abs(i - ci) <= K and abs(j - cj) <= K:
                    want[i, j] = 3.0 * full[K + i - ci] * full[K + j - cj]
        assert np.all(d[0, 0] == 0) and np.allclose(d[0, 1], want, rtol=0, atol=1e-15)


# ------------------------------------------------------------------ 2. the budget, right from wrong
def test_error_budget():
    for case in E.ELASTIC:
        ef, eo = E.e32_field(case), E.e32_out(case)
        print(f"{case}: E32_field = {ef:.3e}, E32_out = {eo:.3e}; max |D| = {np.abs(E.field(case)).max():.3f} px")
        assert 0 < ef < 1e-4 and 0 < eo < 1e-4
    er = E.e32_replica()
    print(f"Replica batches: E32_out = {er:.3e}")
    assert 0 < er < 1e-4
    ref = E.reference(E.ELASTIC[1], 1, 1, E.NB)
    assert np.all(E.bound(ref, False, 1e-6) == 4e-6) and E.bound(ref, True, 1e-6).max() == 4e-6 + 2.0 ** -9


@pytest.mark.parametrize("case", E.ELASTIC)
def test_the_oracle_tells_right_from_wrong(case):
    """Each transcription error moves some element of the GPU tests' inputs by more than 100 times the
    bound; the same matrix form without an error agrees with the oracle."""
    ref = E.field(case)
    assert np.abs(E.buggy_field(case, None) - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())
    fb = E.bound_field(case)
    for bug in E.FIELD_BUGS:
        d = float(np.abs(E.buggy_field(case, bug) - ref).max())
        print(f"{case} {bug}: max field deviation {d:.3e} px; bound {fb:.3e}")
        assert d > 100 * fb, (bug, d, fb)
    if case[0] != (0, 0.0, 0.0):          # under the identity the source pixel IS the output pixel
        img = E.reference(case, 1, 1, E.NB)
        d = float(np.abs(E.source_indexed_warp(case).reshape(img.shape) - img).max())
        ib = float(E.bound(img, True, E.e32_out(case)).max())
        print(f"{case} field indexed by the source pixel: max image deviation {d:.3e}; bound {ib:.3e}")
        assert d > 100 * ib


# ------------------------------------------------------------------ 3. the keys
BAD = {
    "augment_elastic_alpha": [-0.1, 64.5, float("nan"), float("inf"), True, "x", None],
    "augment_elastic_sigma": [0.0, 0.49, 8.5, -1.0, float("nan"), float("inf"), True, "x", None],
}


@pytest.mark.parametrize("key,bad", [(k, b) for k, vals in BAD.items() for b in vals])
def test_invalid_keys_raise_value_error(pm, key, bad):
    field = key[len("augment_"):]
    with pytest.raises(ValueError, match=key):
        A.AugmentConfig(**{field: bad})
    check = {"augment_elastic_alpha": A.check_elastic_alpha, "augment_elastic_sigma": A.check_elastic_sigma}[key]
    with pytest.raises(ValueError, match=key):
        check(bad)
    pm.configure({})
    pm.set_param(key, bad)
    getter = {"augment_elastic_alpha": pm.getAugmentElasticAlpha, "augment_elastic_sigma": pm.getAugmentElasticSigma}[key]
    with pytest.raises(ValueError, match=key):
        getter()
    with pytest.raises(ValueError, match=key):
        pm.getAugment(0)                                  # sigma is checked whatever alpha is


def test_config_keys_flags_and_getters(pm):
    old = A.AugmentConfig(2, 15.0, 0.15, 9)               # the positional use of before
    assert (old.shift, old.rotate, old.scale, old.seed, old.elastic_alpha, old.elastic_sigma) == (2, 15.0, 0.15, 9, 0.0, 4.0)
    assert not A.AugmentConfig().enabled and not A.AugmentConfig(elastic_sigma=2.0).enabled
    only = A.AugmentConfig(elastic_alpha=0.5)
    assert only.enabled and only.elastic and not old.elastic and old.enabled
    assert only.with_seed(3).elastic_alpha == 0.5
    assert A.check_elastic_alpha(64) == 64.0 and A.check_elastic_sigma(0.5) == 0.5 and A.check_elastic_sigma(8) == 8.0
    keys = {"augment_elastic_alpha", "augment_elastic_sigma"}
    assert keys <= set(pm.FLAG_KEYS) and keys <= set(pm.DEFAULTS)
    pm.configure({})
    assert (pm.getAugmentElasticAlpha(), pm.getAugmentElasticSigma()) == (0.0, 4.0) and not pm.getAugment(1).enabled
    pm.configure({"augment_elastic_alpha": 34, "augment_elastic_sigma": 6})
    cfg = pm.getAugment(11)
    assert (cfg.elastic_alpha, cfg.elastic_sigma, cfg.seed, cfg.shift) == (34.0, 6.0, 11, 0) and cfg.enabled

    class Flags:        # the CLI: -1 is "unset", 0 a value
        config = os.path.join(ROOT, "configs", "lenet5_elastic.yaml")
        augment_shift = augment_rotate = augment_scale = augment_seed = -1
        augment_elastic_alpha = augment_elastic_sigma = -1
    pm.configure_from_flags(Flags)
    cfg = pm.getAugment(3)
    assert (cfg.shift, cfg.rotate, cfg.scale, cfg.seed, cfg.elastic_alpha, cfg.elastic_sigma) == (2, 15.0, 0.15, 3, 34.0, 4.0)
    assert pm.getOptimizer(0.001).name == "adam"
    Flags.augment_elastic_alpha, Flags.augment_elastic_sigma = 0.0, 2.5
    pm.configure_from_flags(Flags)
    cfg = pm.getAugment(3)
    assert (cfg.elastic_alpha, cfg.elastic_sigma, cfg.shift) == (0.0, 2.5, 2) and not cfg.elastic
    with open(os.path.join(ROOT, "main.py")) as f:
        text = f.read()
    for k in keys:
        assert f'"{k}", -1' in text


# ------------------------------------------------------------------ 4. warp and the loader, CPU path
def test_alpha_zero_is_bitwise_todays_arrays():
    imgs = O.dataset(3)[O.indices(8)]
    old, new = O.config(O.AFFINE[0]), A.AugmentConfig(*O.AFFINE[0], O.SEED, 0.0, 2.0)
    assert np.array_equal(A.params(old, O.POS0, 8), A.params(new, O.POS0, 8))
    want = A.warp(imgs, A.params(old, O.POS0, 8), 3, 3)
    assert np.array_equal(A.warp(imgs, A.params(old, O.POS0, 8), 3, 3, np.float64, None), want)
    assert np.array_equal(A.augmented(imgs, new, O.POS0, 3, 3), want)
    assert np.array_equal(A.warp(imgs, A.params(old, O.POS0, 8), 3, 3, field=np.zeros((8, 2, 28, 28))), want)
    assert np.all(A.elastic_field(new, O.POS0, 8) == 0)
    with pytest.raises(ValueError, match="field"):
        A.warp(imgs, A.params(old, O.POS0, 8), 3, 3, field=np.zeros((8, 2, 784)))


def test_the_field_moves_the_image_by_whole_pixels():
    """D = (+2, -1) everywhere reads the source 2 to the right and 1 up: the image moves left and down."""
    img = np.zeros((1, 784), np.uint8)
    img[0, 10 * 28 + 5] = 255
    fld = np.zeros((1, 2, 28, 28))
    fld[:, 0], fld[:, 1] = 2.0, -1.0
    out = A.warp(img, np.array([[0, 0, 0, 1]], np.float32), 1, 1, field=fld).reshape(28, 28)
    assert out[11, 3] == 0.5 and np.count_nonzero(out + 0.5) == 1


def _loader(ds, B, cfg, **kw):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceLoader
    return DeviceLoader(ds, torch.full((B, 28, 28, 1), 7.0), torch.full((B,), -77, dtype=torch.int32), augment=cfg, **kw)


@pytest.fixture(scope="module")
def ds():
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceDataset
    return DeviceDataset(torch.from_numpy(O.replica_dataset(1).copy()), torch.arange(O.REPLICA_N) % 10, "cpu")


@pytest.mark.parametrize("case", [E.REPLICA_CASE, E.REPLICA_ONLY_ELASTIC])
def test_loader_writes_warp_with_the_field(ds, case):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import perm_positions
    cfg = E.config(case, 21)
    run = _loader(ds, 16, cfg, seed=4)
    assert run.augment is cfg and run.lookahead_job() is None
    for k in range(3):
        assert run.next() == 16
    rows = perm_positions(32, 16, O.REPLICA_N, 4).numpy()
    want = A.warp(O.replica_dataset(1)[rows], A.params(cfg, 32, 16), 1, 1, field=A.elastic_field(cfg, 32, 16))
    assert np.array_equal(run.out_images.numpy().reshape(16, 784, 1), want.astype(np.float32))
    assert np.array_equal(run.out_labels.numpy(), (rows % 10).astype(np.int32))
    plain = A.warp(O.replica_dataset(1)[rows], A.params(cfg, 32, 16), 1, 1)
    assert not np.array_equal(want, plain)
    other = _loader(ds, 16, cfg, seed=4)                  # seek resumes: nothing but the position is state
    other.seek(2)
    other.next()
    assert torch.equal(other.out_images, run.out_images)
    with pytest.raises(ValueError, match="idx_out"):
        _loader(ds, 16, cfg, idx_out=torch.zeros(16, dtype=torch.int64))
    solo = _loader(ds, 8, cfg, seed=4, rank=1, world=2, shard=False)
    assert solo.augment.seed == 21 + 7919 and solo.augment.elastic_alpha == cfg.elastic_alpha


def test_loader_with_alpha_zero_is_todays_loader(ds):
    a = _loader(ds, 16, O.config(O.REPLICA_CFG, 21), seed=4)
    b = _loader(ds, 16, A.AugmentConfig(*O.REPLICA_CFG, 21, 0.0, 1.5), seed=4)
    none = _loader(ds, 16, A.AugmentConfig(seed=21, elastic_sigma=1.5), seed=4)
    assert none.augment is None
    for _ in range(2):
        a.next()
        b.next()
        assert torch.equal(a.out_images, b.out_images) and torch.equal(a.out_labels, b.out_labels)


def test_replica_cpu_trains_in_prep_with_elastic_alone():
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica
    spec = get_model("mlp", 1)
    x = torch.from_numpy(O.replica_dataset(1).copy())
    y = torch.arange(O.REPLICA_N) % 10
    lines = []
    rep = Replica(spec, "torch", O.REPLICA_B, "cpu", torch_ref.init_params(spec, seed=0), OptConfig(lr0=0.01), x, y, 1,
                  x[:64], y[:64], seed=O.REPLICA_SEED, use_graph=False, fused_input="bf16",
                  augment=E.config(E.REPLICA_ONLY_ELASTIC, E.REPLICA_SEED), log=lines.append)
    assert len(lines) == 1 and "prep" in lines[0] and rep.augment is not None
    rep.step()
    want = E.replica_reference(1, 0, E.REPLICA_ONLY_ELASTIC)
    got = rep.net.x0.double().numpy().reshape(O.REPLICA_B, 784, 1)
    tol = 0.5 * O.bf16_ulp(want) if rep.net.x0.dtype == torch.bfloat16 else np.abs(want) * 2.0 ** -24 + 1e-45
    assert np.all(np.abs(got - want) <= tol)
