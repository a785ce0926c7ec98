"""Shared inputs, wrong transcriptions and the error budget of the augmentation tests.

The oracle itself is ``data/augment.py`` (``params`` bit for bit, ``warp`` in float64), imported.  This
module fixes the inputs both test files use, so that the budget the CPU test computes is the budget
of exactly the images and parameters the GPU test runs:

* images are random full-range uint8 (MNIST's zero border would hide every out-of-image read), plus
  one image that is 255 on its outer frame and 0 inside and one all-255 image;
* the dataset rows next to the used ones are all 255, the index vectors are out of order with repeats;
* ``E32`` is the worst |float32 transcription - float64| over all of them, and the bound of a device
  value is ``4 * E32`` plus, for bf16 output, half a bf16 ulp of the reference (the convention of the
  LRN and LR-schedule budgets: sinf / cosf and the operation order may differ from numpy's by a few
  ulp; a transcription error is orders of magnitude larger, which the CPU test asserts).
"""
import functools

import numpy as np

from distributed_tensorflow_ibm_mnist_amd.data import augment as A

SEED = (0xA5 << 32) | 0x01234567                       # a 40-bit seed
AFFINE = [(2, 15.0, 0.15), (8, 180.0, 0.5)]
CHANNELS = [(1, 1), (3, 3), (1, 3)]
NBS = [1, 3, 64, 70]
POS0 = (1 << 32) - 3                                   # the batch straddles a 32-bit position boundary
USED = 20                                              # used rows 1, 4, 7, ...: every neighbour is all 255
REPLICA_N, REPLICA_B, REPLICA_SEED, REPLICA_STEPS = 192, 64, 5, 3
REPLICA_CFG = (2, 15.0, 0.15)
BUGS = ("centre", "sign", "scale", "edge", "wrap")


def frame_image(C):
    img = np.zeros((28, 28, C), np.uint8)
    img[0], img[-1], img[:, 0], img[:, -1] = 255, 255, 255, 255
    return img.reshape(-1)


@functools.lru_cache(maxsize=None)
def dataset(C):
    """uint8 [3 * USED, 784 * C]: rows 1, 4, 7, ... are the images, every other row is all 255."""
    rng = np.random.default_rng(100 + C)
    d = np.full((3 * USED, 784 * C), 255, np.uint8)
    d[1::3] = rng.integers(0, 256, (USED, 784 * C), dtype=np.uint8)
    d[1] = frame_image(C)
    d[4] = 255
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def labels():
    return (np.arange(3 * USED, dtype=np.int32) * 7 + 3) % 10


@functools.lru_cache(maxsize=None)
def indices(nb):
    """Rows of the batch: out of order, with repeats, the frame and the all-255 image among them."""
    rng = np.random.default_rng(nb)
    idx = 1 + 3 * rng.integers(0, USED, nb)
    idx[0] = 1
    if nb > 1:
        idx[-1] = 4
    if nb > 3:
        idx[2] = idx[1]                    # an adjacent repeat, whatever the draw gave
    idx = idx.astype(np.int64)
    idx.setflags(write=False)
    return idx


def config(case, seed=SEED):
    return A.AugmentConfig(case[0], case[1], case[2], seed)


def reference(case, Csrc, Cdst, nb, pos0=POS0, dtype=np.float64):
    return A.warp(dataset(Csrc)[indices(nb)], A.params(config(case), pos0, nb), Csrc, Cdst, dtype)


@functools.lru_cache(maxsize=None)
def replica_dataset(C):
    """The Replica tests' training set: random full-range rows, the frame and the all-255 image."""
    rng = np.random.default_rng(200 + C)
    d = rng.integers(0, 256, (REPLICA_N, 784 * C), dtype=np.uint8)
    d[0] = frame_image(C)
    d[1] = 255
    d.setflags(write=False)
    return d


def replica_rows(step):
    """Dataset rows of the one-rank Replica's batch at ``step`` (the CPU Feistel shuffle)."""
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import perm_positions
    return perm_positions(step * REPLICA_B, REPLICA_B, REPLICA_N, REPLICA_SEED).numpy()


def replica_reference(C, step, seed, dtype=np.float64):
    """x0 of the Replica tests after ``step + 1`` steps: positions continue across steps."""
    prm = A.params(config(REPLICA_CFG, seed), step * REPLICA_B, REPLICA_B)
    return A.warp(replica_dataset(C)[replica_rows(step)], prm, C, C, dtype)


@functools.lru_cache(maxsize=None)
def e32():
    """The worst |float32 transcription - float64| over every input of the GPU tests."""
    worst = 0.0
    for case in AFFINE:
        for cs, cd in ((1, 1), (3, 3)):          # (1, 3) replicates (1, 1)'s values
            worst = max(worst, float(np.abs(reference(case, cs, cd, max(NBS), dtype=np.float32).astype(np.float64)
                                            - reference(case, cs, cd, max(NBS))).max()))
    for C in (1, 3):
        for step in range(REPLICA_STEPS):
            worst = max(worst, float(np.abs(replica_reference(C, step, REPLICA_SEED, np.float32).astype(np.float64)
                                            - replica_reference(C, step, REPLICA_SEED)).max()))
    return worst


def bf16_ulp(x):
    """The bf16 ulp (8 significant bits) at |x|; x = 0 counts as the smallest normal."""
    _, e = np.frexp(np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126))
    return np.ldexp(1.0, e - 8)


def bound(ref, bf16):
    """Per-element bound of a device value against the float64 reference ``ref``."""
    b = np.full(ref.shape, 4.0 * e32())
    return b + 0.5 * bf16_ulp(ref) if bf16 else b


def shifted(images, prm, C):
    """Host-shifted copies with zero fill: out(i, j) = in(i - ty, j - tx), no np.roll (nothing wraps)."""
    n = images.shape[0]
    src = images.reshape(n, 28, 28, C)
    out = np.zeros_like(src)
    for b in range(n):
        tx, ty = int(prm[b, 0]), int(prm[b, 1])
        ys, yd = (slice(0, 28 - ty), slice(ty, 28)) if ty >= 0 else (slice(-ty, 28), slice(0, 28 + ty))
        xs, xd = (slice(0, 28 - tx), slice(tx, 28)) if tx >= 0 else (slice(-tx, 28), slice(0, 28 + tx))
        out[b, yd, xd] = src[b, ys, xs]
    return out.reshape(n, 784 * C)


def buggy_warp(images, prm, C, bug):
    """``warp`` in float64 with one transcription error: ``centre`` 14.0 for 13.5, ``sign`` -sn for sn,
    ``scale`` s for 1 / s, ``edge`` replication for zero fill, ``wrap`` a tap at x = 28 reading the next
    row's first pixel.  Written apart from ``data/augment.py`` (plain loops over the four taps)."""
    assert bug is None or bug in BUGS        # None: no error (the check of this function itself)
    n = images.shape[0]
    img = images.reshape(n, 784, C).astype(np.float64)
    tx, ty, theta, s = (prm[:, k].astype(np.float64)[:, None, None] for k in range(4))
    ctr = 14.0 if bug == "centre" else 13.5
    c, sn = np.cos(theta), np.sin(theta) * (-1.0 if bug == "sign" else 1.0)
    r = s if bug == "scale" else 1.0 / s
    u = (np.arange(28.0) - ctr)[None, None, :]
    v = (np.arange(28.0) - ctr)[None, :, None]
    sx = (c * u + sn * v) * r + ctr - tx
    sy = (c * v - sn * u) * r + ctr - ty
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    out = np.zeros((n, 28, 28, C))
    b = np.arange(n)[:, None, None]
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            x, y = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
            if bug == "edge":
                tap = img[b, np.clip(y, 0, 27) * 28 + np.clip(x, 0, 27)]
            else:
                ok = (y >= 0) & (y < 28) & (x >= 0) & ((x < 28) | ((bug == "wrap") & (x == 28) & (y < 27)))
                tap = np.where(ok[..., None], img[b, np.clip(y * 28 + x, 0, 783)], 0.0)
            out += tap * (wy * wx)[..., None]
    return (out / 255.0 - 0.5).reshape(n, 784, C)
