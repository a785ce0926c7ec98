"""Shared inputs, wrong transcriptions and the error budget of the elastic-distortion tests.

The oracle is ``data/augment.py`` (``elastic_draws`` bit for bit, ``elastic_field`` and ``warp`` in
float64), imported.  The dataset, the index vectors, the labels, the seed and the stream position are
those of ``augment_oracle``; this module fixes the elastic cases on top of them, so that the budget the
CPU test computes is the budget of exactly the fields and images the GPU test runs:

* ``e32_field(case)`` / ``e32_out(case)``: the worst |float32 transcription - float64| of
  ``elastic_field`` and of ``warp`` with that field over the case's inputs (per case: the cases differ
  by two orders of magnitude, and one budget for all would be the loosest one);
* the bound of a device value is 4 times that, plus half a bf16 ulp of the reference for bf16 images
  -- the convention of the augmentation, LRN and LR-schedule budgets.  The margin covers another
  summation order, contraction and sincosf against numpy; a transcription error is orders of magnitude
  larger, which the CPU test asserts with the wrong fields below.
"""
import functools

import numpy as np

import augment_oracle as O
from distributed_tensorflow_ibm_mnist_amd.data import augment as A

# ((shift, rotate, scale), alpha, sigma): elastic alone; the example recipe; the smallest table with
# displacements far outside the image; the longest table (K = 24), nearly as wide as the image
ELASTIC = [((0, 0.0, 0.0), 34.0, 4.0), ((2, 15.0, 0.15), 34.0, 4.0), ((8, 180.0, 0.5), 64.0, 0.5),
           ((0, 0.0, 0.0), 8.0, 8.0)]
REPLICA_CASE = (O.REPLICA_CFG, 34.0, 4.0)
REPLICA_ONLY_ELASTIC = ((0, 0.0, 0.0), 34.0, 4.0)
REPLICA_SEED = 21                      # the augmentation seed of the Replica tests
NB = max(O.NBS)
FIELD_BUGS = ("swap", "transpose", "sign", "taps", "reflect", "scale")


def config(case, seed=O.SEED):
    (S, R, Z), alpha, sigma = case
    return A.AugmentConfig(S, R, Z, seed, alpha, sigma)


@functools.lru_cache(maxsize=None)
def _field(case, nb, pos0, f32):
    d = A.elastic_field(config(case), pos0, nb, np.float32 if f32 else np.float64)
    d.setflags(write=False)
    return d


def field(case, nb=NB, pos0=O.POS0, dtype=np.float64):
    return _field(case, nb, pos0, np.dtype(dtype) == np.float32)


@functools.lru_cache(maxsize=None)
def _reference(case, Csrc, Cdst, nb, pos0, f32):
    dt = np.float32 if f32 else np.float64
    out = A.warp(O.dataset(Csrc)[O.indices(nb)], A.params(config(case), pos0, nb), Csrc, Cdst, dt,
                 field(case, nb, pos0, dt))
    out.setflags(write=False)
    return out


def reference(case, Csrc, Cdst, nb, pos0=O.POS0, dtype=np.float64):
    return _reference(case, Csrc, Cdst, nb, pos0, np.dtype(dtype) == np.float32)


@functools.lru_cache(maxsize=None)
def _replica_reference(case, C, step, f32):
    dt = np.float32 if f32 else np.float64
    cfg = config(case, REPLICA_SEED)
    out = A.augmented(O.replica_dataset(C)[O.replica_rows(step)], cfg, step * O.REPLICA_B, C, C, dt)
    out.setflags(write=False)
    return out


def replica_reference(C, step, case=REPLICA_CASE, dtype=np.float64):
    """x0 of the Replica tests after ``step + 1`` steps: positions continue across steps."""
    return _replica_reference(case, C, step, np.dtype(dtype) == np.float32)


def _gap(a32, a64):
    return float(np.abs(a32.astype(np.float64) - a64).max())


@functools.lru_cache(maxsize=None)
def e32_field(case):
    """The worst |float32 transcription - float64| of the field over the GPU field test's input."""
    return _gap(field(case, dtype=np.float32), field(case))


@functools.lru_cache(maxsize=None)
def e32_out(case):
    """... of the images over the inputs of the GPU image tests of ``case`` ((1, 3) replicates (1, 1))."""
    return max(_gap(reference(case, cs, cd, NB, dtype=np.float32), reference(case, cs, cd, NB))
               for cs, cd in ((1, 1), (3, 3)))


@functools.lru_cache(maxsize=None)
def e32_replica(case=REPLICA_CASE):
    """... over the batches of the Replica tests, both models."""
    return max(_gap(replica_reference(C, step, case, np.float32), replica_reference(C, step, case))
               for C in (1, 3) for step in range(O.REPLICA_STEPS))


def bound_field(case):
    return 4.0 * e32_field(case)


def bound(ref, bf16, e32):
    """Per-element bound of a device image value against the float64 reference ``ref``."""
    b = np.full(ref.shape, 4.0 * e32)
    return b + 0.5 * O.bf16_ulp(ref) if bf16 else b


def band_matrix(w, reflect=False):
    """G [28, 28]: row i holds the taps of output i, zero extension or (``reflect``) symmetric padding.
    Plain loops, written apart from ``data/augment.py``."""
    K = len(w) - 1
    G = np.zeros((28, 28))
    for i in range(28):
        for a in range(-K, K + 1):
            m = i + a
            if reflect:
                m = -m - 1 if m < 0 else 55 - m if m > 27 else m
            if 0 <= m < 28:
                G[i, m] += float(w[abs(a)])
    return G


def buggy_field(case, bug, nb=NB, pos0=O.POS0):
    """The float64 field as G r G^T with one transcription error: ``swap`` the planes exchanged,
    ``transpose`` the field transposed, ``sign`` -D, ``taps`` K - 1 taps renormalised, ``reflect``
    symmetric padding, ``scale`` every weight times 1.001.  None: no error."""
    assert bug is None or bug in FIELD_BUGS
    cfg = config(case)
    r = (A.elastic_draws(cfg, pos0, nb).astype(np.float64) - 32767.5) * 2.0 ** -15
    w = A.elastic_weights(cfg.elastic_sigma).astype(np.float64)
    if bug == "taps":
        w = w[:-1] / (w[0] + 2.0 * w[1:-1].sum())
    if bug == "scale":
        w = w * 1.001
    G = band_matrix(w, reflect=bug == "reflect")
    d = float(np.float32(cfg.elastic_alpha)) * np.einsum("im,nfmk,jk->nfij", G, r, G)
    if bug == "swap":
        d = d[:, ::-1]
    if bug == "transpose":
        d = d.transpose(0, 1, 3, 2)
    if bug == "sign":
        d = -d
    return d


def source_indexed_warp(case, nb=NB, pos0=O.POS0):
    """``warp`` in float64 with the field looked up at the (rounded, clipped) SOURCE pixel of the affine
    map instead of the output pixel: the error of a kernel that displaces forward."""
    cfg = config(case)
    prm = A.params(cfg, pos0, nb)
    sx, sy = A.source_coords(prm)
    xi = np.clip(np.rint(sx), 0, 27).astype(np.int64)
    yi = np.clip(np.rint(sy), 0, 27).astype(np.int64)
    d = field(case, nb, pos0)
    b = np.arange(nb)[:, None, None]
    moved = np.stack([d[b, 0, yi, xi], d[b, 1, yi, xi]], axis=1)
    return A.warp(O.dataset(1)[O.indices(nb)], prm, 1, 1, np.float64, moved)
