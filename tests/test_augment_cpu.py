"""Training augmentation, CPU side: the host reference (``data/augment.py``: the Philox draw, the
float64 warp), validation of the four ``augment_*`` keys, the proof that the oracle tells a right
kernel from a wrong one, the error budget the GPU tests hold the device to, and the loader on the
CPU path (seek, sharding, the un-augmented path untouched)."""
import math
import os

import numpy as np
import pytest
import torch

import augment_oracle as O
from distributed_tensorflow_ibm_mnist_amd.data import augment as A
from distributed_tensorflow_ibm_mnist_amd.ops import dropout as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def pm():
    from distributed_tensorflow_ibm_mnist_amd.utils import parameter_mgr
    yield parameter_mgr
    parameter_mgr.configure({})


# ------------------------------------------------------------------ 1. draws
@pytest.mark.parametrize("p,words,want", [
    (0, "4f4f9d82 cd592837 a56995a4 2677aabd", (-1.0, 2.0, 0.0765199363231659, 0.8950790166854858)),
    (5, "14a803d7 c1e88956 74dd44a1 bc91e1e7", (-3.0, 2.0, -0.022775894030928612, 1.0709803104400635)),
    ((1 << 32) + 5, "5cc3bea2 cb9d532c 43a56f0d 640ae21b", (-1.0, 2.0, -0.12344204634428024, 0.9672372937202454)),
])
def test_params_known_answers(p, words, want):
    """counter = (p lo, p hi, 0, 0x41554700), key = (seed lo, seed hi) through the Philox whose published
    vectors tests/test_dropout_cpu.py checks; (tx, ty, theta, s) derived by hand from the four words."""
    seed = O.SEED
    w = D.philox4x32_10((p & 0xFFFFFFFF, p >> 32, 0, 0x41554700), (seed & 0xFFFFFFFF, seed >> 32))
    assert " ".join("%08x" % int(x) for x in w) == words
    S, R, Z = 3, 15.0, 0.15
    f = np.float32
    u2, u3 = f(int(w[2]) >> 8) * f(2.0 ** -24), f(int(w[3]) >> 8) * f(2.0 ** -24)
    hand = [f((int(w[0]) * (2 * S + 1)) >> 32) - f(S), f((int(w[1]) * (2 * S + 1)) >> 32) - f(S),
            (f(R) * (f(2) * u2 - f(1))) * f(math.pi / 180), f(1) + f(Z) * (f(2) * u3 - f(1))]
    got = A.params(A.AugmentConfig(S, R, Z, seed), p, 1)
    assert got.dtype == np.float32 and got.shape == (1, 4)
    assert got[0].tolist() == [float(x) for x in hand] == list(want)
    # a draw is a function of the position alone: a batch is a window of the stream
    assert np.array_equal(A.params(A.AugmentConfig(S, R, Z, seed), max(p - 2, 0), 9)[p - max(p - 2, 0)], got[0])


@pytest.mark.parametrize("S", [1, 3, 8])
def test_shifts_are_uniform_integers(S):
    n = 1 << 16
    prm = A.params(A.AugmentConfig(S, 0.0, 0.0, 77), 12345, n)
    sigma = math.sqrt(n * (1 / (2 * S + 1)) * (1 - 1 / (2 * S + 1)))
    for k in (0, 1):
        t = prm[:, k]
        assert np.array_equal(t, np.round(t)) and t.min() == -S and t.max() == S
        counts = np.bincount((t + S).astype(np.int64), minlength=2 * S + 1)
        assert len(counts) == 2 * S + 1 and np.all(np.abs(counts - n / (2 * S + 1)) <= 5 * sigma), counts
    assert abs(np.corrcoef(prm[:, 0], prm[:, 1])[0, 1]) < 0.02          # x and y drawn independently
    assert np.all(prm[:, 2] == 0) and np.all(prm[:, 3] == 1)             # R = Z = 0: the identity, exactly


def test_theta_and_scale_stay_inside_their_half_open_ranges():
    for R, Z in ((15.0, 0.15), (180.0, 0.5), (0.0, 0.5), (180.0, 0.0)):
        prm = A.params(A.AugmentConfig(0, R, Z, 3), 0, 1 << 16)
        lim = np.float32(np.float32(R) * np.float32(math.pi / 180))
        assert np.all(prm[:, 2] >= -lim) and (np.all(prm[:, 2] < lim) if R else np.all(prm[:, 2] == 0))
        assert np.all(prm[:, 3] >= np.float32(1) - np.float32(Z))
        assert np.all(prm[:, 3] < np.float32(1) + np.float32(Z)) if Z else np.all(prm[:, 3] == 1)
        assert np.all(prm[:, 0] == 0) and np.all(prm[:, 1] == 0)
        if R:
            assert prm[:, 2].min() < -0.99 * lim and prm[:, 2].max() > 0.99 * lim
        if Z:
            assert prm[:, 3].min() < 1 - 0.99 * Z and prm[:, 3].max() > 1 + 0.99 * Z


def test_positions_2_pow_32_apart_and_seeds_differ():
    cfg = A.AugmentConfig(3, 15.0, 0.15, O.SEED)
    a, b = A.params(cfg, 7, 64), A.params(cfg, 7 + (1 << 32), 64)
    assert not np.any(np.all(a == b, axis=1))                            # the high position word is in the counter
    c = A.params(cfg.with_seed(O.SEED + (1 << 32)), 7, 64)               # and the high seed word in the key
    assert not np.any(np.all(a == c, axis=1))
    # dropout's counter word 3 is (layer index << 16) | feature group: the tag needs layer 0x4155, which no
    # model has, so equal seeds do not correlate the two features
    from distributed_tensorflow_ibm_mnist_amd.models import get_model
    assert A.TAG == 0x41554700
    assert all(len(get_model(m, 1).layers) < A.TAG >> 16 for m in ("lenet5", "reference_cnn", "mlp"))


# ------------------------------------------------------------------ 2. refusals
BAD = {
    "augment_shift": [-1, 9, 2.5, True, "x", None, float("nan")],
    "augment_rotate": [-0.1, 180.5, float("nan"), float("inf"), True, "x", None],
    "augment_scale": [-0.1, 0.51, float("nan"), float("inf"), True, "x", None],
    "augment_seed": [-1, 1 << 63, 2.5, True, "x"],
}


@pytest.mark.parametrize("key,bad", [(k, b) for k, vals in BAD.items() for b in vals])
def test_invalid_keys_raise_value_error(pm, key, bad):
    field = key[len("augment_"):]
    with pytest.raises(ValueError, match=key):
        A.AugmentConfig(**{field: bad})
    pm.configure({})
    pm.set_param(key, bad)
    getter = {"augment_shift": pm.getAugmentShift, "augment_rotate": pm.getAugmentRotate,
              "augment_scale": pm.getAugmentScale, "augment_seed": lambda: pm.getAugmentSeed(0)}[key]
    if not (key == "augment_seed" and bad is None):
        with pytest.raises(ValueError, match=key):
            getter()
        with pytest.raises(ValueError, match=key):
            pm.getAugment(0)


def test_key_flag_and_getter_round_trip(pm):
    keys = {"augment_shift", "augment_rotate", "augment_scale", "augment_seed"}
    assert keys <= set(pm.FLAG_KEYS) and keys <= set(pm.DEFAULTS)
    pm.configure({})
    cfg = pm.getAugment(11)
    assert (cfg.shift, cfg.rotate, cfg.scale, cfg.seed) == (0, 0.0, 0.0, 11) and not cfg.enabled
    pm.configure({"augment_shift": 8, "augment_rotate": 180, "augment_scale": 0.5, "augment_seed": (1 << 63) - 1})
    cfg = pm.getAugment(11)
    assert (cfg.shift, cfg.rotate, cfg.scale, cfg.seed) == (8, 180.0, 0.5, (1 << 63) - 1) and cfg.enabled
    for one in ({"augment_shift": 1}, {"augment_rotate": 0.5}, {"augment_scale": 0.01}):
        pm.configure(one)
        assert pm.getAugment(0).enabled

    class Flags:        # the CLI: -1 is "unset", 0 a value
        config = os.path.join(ROOT, "configs", "lenet5_augment.yaml")
        augment_shift = augment_rotate = augment_scale = augment_seed = -1
    pm.configure_from_flags(Flags)
    cfg = pm.getAugment(3)
    assert (cfg.shift, cfg.rotate, cfg.scale, cfg.seed) == (2, 15.0, 0.15, 3) and pm.getOptimizer(0.001).name == "adam"
    Flags.augment_shift, Flags.augment_rotate, Flags.augment_seed = 0, 0.0, 9
    pm.configure_from_flags(Flags)
    cfg = pm.getAugment(3)
    assert (cfg.shift, cfg.rotate, cfg.scale, cfg.seed) == (0, 0.0, 0.15, 9)


def test_main_defines_the_flags_and_ps_mode_takes_them():
    with open(os.path.join(ROOT, "main.py")) as f:
        text = f.read()
    for k in ("augment_shift", "augment_rotate", "augment_scale", "augment_seed"):
        assert f'"{k}", -1' in text
    assert "check_ps_augment" not in text       # a worker augments its own inputs: nothing to refuse


def test_params_and_warp_refuse_bad_arguments():
    cfg = A.AugmentConfig(1, 0.0, 0.0, 0)
    with pytest.raises(ValueError, match="pos0"):
        A.params(cfg, -1, 4)
    with pytest.raises(ValueError, match="pos0"):
        A.params(cfg, (1 << 63) - 2, 4)
    with pytest.raises(ValueError, match="Csrc"):
        A.warp(np.zeros((1, 784 * 3), np.uint8), A.params(cfg, 0, 1), 3, 1)
    with pytest.raises(ValueError, match="uint8"):
        A.warp(np.zeros((1, 784), np.float32), A.params(cfg, 0, 1), 1, 1)


# ------------------------------------------------------------------ 3. the exact case
@pytest.mark.parametrize("C", [1, 3])
def test_pure_shift_is_a_shifted_copy(C):
    """R = Z = 0: every coordinate is an integer, so warp is the shifted image with zero fill, exactly,
    for every (tx, ty) in [-3, 3]^2."""
    img = O.dataset(C)[[7, 1, 4]]
    for ty in range(-3, 4):
        for tx in range(-3, 4):
            prm = np.tile(np.array([tx, ty, 0, 1], np.float32), (3, 1))
            want = O.shifted(img, prm, C).astype(np.float64).reshape(3, 784, C) / 255.0 - 0.5
            assert np.array_equal(A.warp(img, prm, C, C), want), (tx, ty)
    # tx > 0 moves the image to the right, ty > 0 down; 1 -> 3 replicates
    one = np.zeros((1, 784), np.uint8)
    one[0, 10 * 28 + 5] = 255
    out = A.warp(one, np.array([[2, 3, 0, 1]], np.float32), 1, 3)
    assert out.shape == (1, 784, 3) and np.all(out[0, 13 * 28 + 7] == 0.5) and np.count_nonzero(out + 0.5) == 3


def test_shifted_helper_never_wraps():
    img = O.dataset(1)[[4]]                                   # all 255
    out = O.shifted(img, np.array([[3, -2, 0, 1]], np.float32), 1).reshape(28, 28)
    assert np.all(out[:26, 3:] == 255) and np.all(out[26:] == 0) and np.all(out[:, :3] == 0)


# ------------------------------------------------------------------ 4. right from wrong, and the budget
def test_error_budget():
    """E32 over the GPU tests' inputs, computed here and never hard-coded: below 1e-4 of the value
    range (1.0: the outputs span [-0.5, 0.5])."""
    e = O.e32()
    print(f"E32 = {e:.3e}; device bound 4 * E32 = {4 * e:.3e} (+ half a bf16 ulp of the reference for bf16)")
    assert 0 < e < 1e-4
    ref = O.reference(O.AFFINE[0], 1, 1, 70)
    assert np.all(O.bound(ref, False) == 4 * e)
    assert np.all(O.bound(ref, True) >= 4 * e + 2.0 ** -135) and O.bound(ref, True).max() == 4 * e + 2.0 ** -9   # |ref| = 0.5
    assert O.bf16_ulp(0.5) == 2.0 ** -8 and O.bf16_ulp(0.4999) == 2.0 ** -9 and O.bf16_ulp(-0.25) == 2.0 ** -9


@pytest.mark.parametrize("case", O.AFFINE)
def test_the_oracle_tells_right_from_wrong(case):
    """Each transcription error moves some element of the GPU tests' inputs by far more than the bound;
    the same loops without an error agree with the oracle."""
    nb = max(O.NBS)
    imgs, prm = O.dataset(1)[O.indices(nb)], A.params(O.config(case), O.POS0, nb)
    ref = O.reference(case, 1, 1, nb)
    worst_bound = float(O.bound(ref, True).max())
    assert np.abs(O.buggy_warp(imgs, prm, 1, None) - ref).max() < 1e-12
    for bug in O.BUGS:
        d = float(np.abs(O.buggy_warp(imgs, prm, 1, bug) - ref).max())
        print(f"{case} {bug}: max deviation {d:.4f} = {d * 255:.1f} raw grey levels; bound {worst_bound:.3e}")
        assert d > 100 * worst_bound and d * 255 > 1.0, (bug, d)


def test_the_inputs_are_what_the_gpu_tests_need():
    for C in (1, 3):
        d = O.dataset(C)
        assert np.all(d[0::3] == 255) and np.all(d[2::3] == 255)          # the neighbours of every used row
        assert d[7:].min() == 0 and d[7:].max() == 255                     # full range, not MNIST-like
        f = d[1].reshape(28, 28, C)
        assert np.all(f[0] == 255) and np.all(f[:, 0] == 255) and np.all(f[1:-1, 1:-1] == 0) and np.all(d[4] == 255)
    for nb in O.NBS:
        idx = O.indices(nb)
        assert len(idx) == nb and np.all(idx % 3 == 1) and idx[0] == 1
        if nb > 3:
            assert idx[-1] == 4 and len(set(idx.tolist())) < nb and np.any(np.diff(idx) < 0)


# ------------------------------------------------------------------ 5. the loader, CPU path
def _loader(ds, B, cfg, **kw):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceLoader
    return DeviceLoader(ds, torch.full((B, 28, 28, 1), 7.0), torch.full((B,), -77, dtype=torch.int32), augment=cfg, **kw)


@pytest.fixture(scope="module")
def ds():
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceDataset
    return DeviceDataset(torch.from_numpy(O.replica_dataset(1).copy()), torch.arange(O.REPLICA_N) % 10, "cpu")


def test_loader_batches_are_the_oracle_and_seek_resumes(ds):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import perm_positions
    cfg = O.config(O.REPLICA_CFG, 21)
    run = _loader(ds, 16, cfg, seed=4)
    batches = []
    for k in range(14):                                    # 224 positions: past one epoch of 192
        assert run.next() == 16
        batches.append((run.out_images.clone(), run.out_labels.clone()))
    for k in (0, 5, 13):
        rows = perm_positions(16 * k, 16, O.REPLICA_N, 4).numpy()
        want = A.warp(O.replica_dataset(1)[rows], A.params(cfg, 16 * k, 16), 1, 1).astype(np.float32)
        assert np.array_equal(batches[k][0].numpy().reshape(16, 784, 1), want)
        assert np.array_equal(batches[k][1].numpy(), (rows % 10).astype(np.int32))
        other = _loader(ds, 16, cfg, seed=4)
        other.seek(k)
        other.next()
        assert torch.equal(other.out_images, batches[k][0]) and torch.equal(other.out_labels, batches[k][1])
    # the same image gets a new transformation in the next epoch
    rows0, rows12 = perm_positions(0, 16, O.REPLICA_N, 4), perm_positions(192, 16, O.REPLICA_N, 4)
    assert not np.array_equal(A.params(cfg, 0, 16), A.params(cfg, 192, 16)) and rows0.shape == rows12.shape
    assert run.lookahead_job() is None
    # a partial batch leaves the rows past it alone
    run.out_images.fill_(7.0)
    assert run.next(5) == 5 and torch.all(run.out_images[5:] == 7.0) and not torch.any(run.out_images[:5] == 7.0)


def test_sharded_ranks_concatenate_and_unsharded_ranks_differ(ds):
    cfg = O.config(O.REPLICA_CFG, 21)
    one = _loader(ds, 16, cfg, seed=4)
    two = [_loader(ds, 8, cfg, seed=4, rank=r, world=2) for r in (0, 1)]
    for _ in range(3):
        one.next()
        for ld in two:
            ld.next()
        assert torch.equal(torch.cat([ld.out_images for ld in two]), one.out_images)
        assert torch.equal(torch.cat([ld.out_labels for ld in two]), one.out_labels)
    assert not torch.equal(two[0].out_images, two[1].out_images)
    solo = [_loader(ds, 8, cfg, seed=4, rank=r, world=2, shard=False) for r in (0, 1)]
    assert solo[0].augment.seed == 21 and solo[1].augment.seed == 21 + 7919
    # the same rows in the same order (shuffle off) still come out differently
    same = [_loader(ds, 8, cfg, seed=4, rank=r, world=2, shard=False, shuffle=False) for r in (0, 1)]
    for ld in same:
        ld.next()
    assert torch.equal(same[0].out_labels, same[1].out_labels) and not torch.equal(same[0].out_images, same[1].out_images)


def test_no_augment_is_bitwise_todays_path(ds):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import perm_positions
    plain, none, zero = _loader(ds, 16, None, seed=4), _loader(ds, 16, None, seed=4), _loader(ds, 16, A.AugmentConfig(seed=5), seed=4)
    assert zero.augment is None
    for k in range(2):
        for ld in (plain, none, zero):
            ld.next()
        rows = perm_positions(16 * k, 16, O.REPLICA_N, 4)
        want = ds.images[rows].float().view(16, 28, 28, 1) * (1.0 / 255.0) - 0.5
        assert torch.equal(plain.out_images, want) and torch.equal(zero.out_images, want)
    with pytest.raises(ValueError, match="idx_out"):
        _loader(ds, 16, O.config(O.REPLICA_CFG), idx_out=torch.zeros(16, dtype=torch.int64))
    _loader(ds, 16, A.AugmentConfig(), idx_out=torch.zeros(16, dtype=torch.int64))     # all amounts 0: no augmentation


def test_bf16_buffer_gets_one_rounding(ds):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceLoader
    cfg = O.config(O.REPLICA_CFG, 21)
    ld = DeviceLoader(ds, torch.zeros(16, 28, 28, 1, dtype=torch.bfloat16), torch.zeros(16, dtype=torch.int32), seed=4,
                      augment=cfg)
    ld.next()
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import perm_positions
    ref = A.warp(O.replica_dataset(1)[perm_positions(0, 16, O.REPLICA_N, 4).numpy()], A.params(cfg, 0, 16), 1, 1)
    got = ld.out_images.float().numpy().reshape(16, 784, 1).astype(np.float64)
    assert np.all(np.abs(got - ref) <= 0.5 * O.bf16_ulp(ref))
    # either side of the bf16 tie 1 + 2^-8: fp32 rounds both ONTO the tie, rounding to odd does not
    x = np.array([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8 - 2.0 ** -40, 0.3])
    y = torch.from_numpy(A.f32_round_to_odd(x)).to(torch.bfloat16).double().numpy()
    assert y.tolist() == [1.0 + 2.0 ** -7, 1.0, float(torch.tensor(0.3).to(torch.bfloat16))]
    assert torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).double().tolist()[:2] == [1.0, 1.0]


def test_replica_cpu_runs_augmented_and_evaluates_plain():
    """The torch replica on CPU: x0 of a training step is the oracle's batch, evaluate() is that of a
    replica without augmentation."""
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica
    spec = get_model("mlp", 1)
    x = torch.from_numpy(O.replica_dataset(1).copy())
    y = torch.arange(O.REPLICA_N) % 10
    cfg = O.config(O.REPLICA_CFG, 21)
    lines = []

    def make(aug, mode="prep"):
        return Replica(spec, "torch", O.REPLICA_B, "cpu", torch_ref.init_params(spec, seed=0), OptConfig(lr0=0.01), x, y,
                       1, x[:64], y[:64], seed=O.REPLICA_SEED, use_graph=False, fused_input=mode, augment=aug,
                       log=lines.append)
    a, b, z = make(cfg, "bf16"), make(None), make(A.AugmentConfig(seed=3))
    assert len(lines) == 1 and "prep" in lines[0] and a.augment is cfg and z.augment is None and b.augment is None
    assert a.evaluate() == b.evaluate()
    for step in range(2):
        for r in (a, b, z):
            r.step()
        want = O.replica_reference(1, step, 21)
        got = a.net.x0.double().numpy().reshape(O.REPLICA_B, 784, 1)
        tol = 0.5 * O.bf16_ulp(want) if a.net.x0.dtype == torch.bfloat16 else np.abs(want) * 2.0 ** -24 + 1e-45
        assert np.all(np.abs(got - want) <= tol)
        assert torch.equal(b.net.x0, z.net.x0) and torch.equal(b.net.fp.params, z.net.fp.params)
        assert not torch.equal(a.net.x0, b.net.x0) and torch.equal(a.net.labels, b.net.labels)
