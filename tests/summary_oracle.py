"""numpy reference of the summary_stats kernel (csrc/kernels/summary.hip) and the boundary inputs
its tests share.

reference(values, segs, limits, divisor): per segment ``(offset, rows, cols, row_stride)`` of the
flat float32 array ``values`` (a bf16 source: its exact float32 widening) the ``NB + 1`` bucket
counts and ``min, max, sum, sum of squares``.  A value is divided by ``divisor`` as numpy divides a
float32 array by an int (one correctly rounded fp32 division; ``divisor == 1``: untouched), widened
to float64, and counted at ``np.searchsorted(limits, v, side="left")``.  Column ``NB`` takes what
lies above the last limit, NaN -- and both infinities: -inf would search to column 0, but a
histogram with a non-finite value is the host path's to write, so the kernel reports every
non-finite value in the last column and keeps it out of the moments.
"""
import functools

import numpy as np


def _segment_values(values, seg):
    off, rows, cols, stride = (int(x) for x in seg)
    if rows == 0 or cols == 0:
        return np.zeros(0, np.float32)
    idx = off + np.arange(rows)[:, None] * stride + np.arange(cols)[None, :]
    return np.asarray(values, dtype=np.float32)[idx.reshape(-1)]


def divided(v32, divisor):
    """float32 / int as Monitor._grad does it; divisor 1 leaves every bit (NaN payloads too)."""
    return v32 if divisor == 1 else (v32 / np.float32(divisor)).astype(np.float32)


def reference(values, segs, limits, divisor=1):
    limits = np.asarray(limits, dtype=np.float64)
    nb = limits.size
    counts = np.zeros((len(segs), nb + 1), np.int64)
    stats = np.zeros((len(segs), 4), np.float64)
    for s, seg in enumerate(segs):
        with np.errstate(all="ignore"):
            v = divided(_segment_values(values, seg), divisor).astype(np.float64)
        idx = np.searchsorted(limits, v, side="left")
        idx[~np.isfinite(v)] = nb
        counts[s] = np.bincount(idx, minlength=nb + 1)
        c = v[idx < nb]
        stats[s] = (c.min(), c.max(), c.sum(), (c * c).sum()) if c.size else (np.inf, -np.inf, 0.0, 0.0)
    return counts, stats


def sum_bounds(values, segs, limits, divisor=1):
    """Per segment the allowed |sum - ref| and |sumsq - ref|: n * 2^-52 * sum|v| and n * 2^-52 *
    sum v^2.  Each side's float64 summation error is at most (n - 1) * 2^-53 of the absolute sum in
    any order, and the squares of fp32 values are exact in float64."""
    limits = np.asarray(limits, dtype=np.float64)
    out = np.zeros((len(segs), 2))
    for s, seg in enumerate(segs):
        with np.errstate(all="ignore"):
            v = divided(_segment_values(values, seg), divisor).astype(np.float64)
        c = v[np.isfinite(v) & (v <= limits[-1])]
        out[s] = (c.size * 2.0 ** -52 * np.abs(c).sum(), c.size * 2.0 ** -52 * (c * c).sum())
    return out


# ------------------------------------------------------------------ boundary inputs
def _all_finite_bf16():
    bits = (np.arange(1 << 16, dtype=np.uint32) << 16)
    v = bits.view(np.float32)
    return np.unique(v[np.isfinite(v)].astype(np.float64))      # sorted; -0.0 and 0.0 are one


@functools.lru_cache(maxsize=None)
def boundary_set(kind="fp32"):
    """(values float32, expected bucket int64) around every limit of the TF table but +-DBL_MAX:
    the largest fp32 (kind="bf16": bf16) value <= L_i, which belongs in bucket i, and the smallest
    one > L_i, which belongs in bucket i + 1 -- then both zeros (bucket of the 0.0 limit), fp32
    denormals (kind="fp32" only; the buckets next to zero: the 1e-12 limit's for the positive ones,
    the 0.0 limit's, (-1e-12, 0], for the negative ones) and +-FLT_MAX resp. the largest bf16 (the
    buckets that end at DBL_MAX and start at -DBL_MAX)."""
    from distributed_tensorflow_ibm_mnist_amd.obs.events import BUCKET_LIMITS as L
    nb = L.size
    inner = np.arange(1, nb - 1)
    lim = L[inner]
    if kind == "fp32":
        f = lim.astype(np.float32)
        le = np.where(f.astype(np.float64) > lim, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)
        gt = np.nextafter(le, np.float32(np.inf)).astype(np.float32)
        big = np.float32(np.finfo(np.float32).max)
    else:
        allb = _all_finite_bf16()
        j = np.searchsorted(allb, lim, side="right")
        le, gt = allb[j - 1].astype(np.float32), allb[j].astype(np.float32)
        big = np.float32(allb[-1])
    zero = int(np.where(L == 0.0)[0][0])
    vals = [le, gt, np.array([0.0, -0.0], np.float32), np.array([big, -big], np.float32)]
    want = [inner, inner + 1, np.array([zero, zero]), np.array([nb - 1, 1])]
    if kind == "fp32":
        den = np.array([1e-45, 1e-40, 1.1754942e-38], np.float32)
        assert (den > 0).all() and (den < np.finfo(np.float32).tiny).all()
        vals += [den, -den]
        want += [np.full(3, zero + 1), np.full(3, zero)]
    return np.concatenate(vals).astype(np.float32), np.concatenate(want).astype(np.int64)
