"""Float64 numpy oracle of the label-smoothed softmax cross-entropy, written from the formulas,
for ``test_label_smoothing_gpu.py`` and ``test_label_smoothing_cpu.py``.  It shares no code with
the package (``stats_oracle.py``, loaded by path, supplies the plain pieces and the tolerances).

With eps the smoothing, NC the real class count and y the label:

    q_c   = (1 - eps) * [c == y] + eps / NC
    loss  = -sum_c q_c log p_c
    dl_c  = (p_c - q_c) * scale

eps = 0 is the plain cross-entropy of ``stats_oracle.py``.  The log-softmax subtracts the row
maximum, so large logits of one sign stay finite in float64.
"""
import importlib.util
import os

import numpy as np

_here = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("stats_oracle", os.path.join(_here, "stats_oracle.py"))
so = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(so)

f64, i64, ce_tol, check_ce, top1_count = so.f64, so.i64, so.ce_tol, so.check_ce, so.top1_count


def targets(labels, nc, eps):
    y = i64(labels)
    q = np.full((y.shape[0], nc), eps / nc, dtype=np.float64)
    q[np.arange(y.shape[0]), y] += 1.0 - eps
    return q


def ce_rows(logits, labels, eps):
    """The smoothed loss of every row."""
    lsm = so.log_softmax(logits)
    return -(targets(labels, lsm.shape[1], eps) * lsm).sum(axis=1)


def ce_sum(logits, labels, eps):
    return float(ce_rows(logits, labels, eps).sum())


def dlogits(logits, labels, scale, eps):
    z = f64(logits)
    return (so.softmax(z) - targets(labels, z.shape[1], eps)) * scale


def check_dlogits(dl, logits, labels, scale, eps, what=""):
    """bf16 kernels: one bf16 rounding plus intrinsic error, 2**-8 of the largest gradient
    (``stats_oracle.check_dlogits``)."""
    g = dlogits(logits, labels, scale, eps)
    err = np.abs(f64(dl) - g).max()
    print(f"{what}: dlogits err {err:.3e}, max |g| {np.abs(g).max():.3e}")
    assert err <= 2.0 ** -8 * np.abs(g).max(), f"{what}: dlogits err {err:.3e} vs max |g| {np.abs(g).max():.3e}"
    return g


def check_dlogits_f32(dl, logits, labels, scale, eps, what=""):
    """The fp32 kernel: ``stats_oracle.check_probs``' measure, 1e-5 * max|g| + 1e-6."""
    g = dlogits(logits, labels, scale, eps)
    err = np.abs(f64(dl) - g).max()
    tol = 1e-5 * np.abs(g).max() + 1e-6
    print(f"{what}: fp32 dlogits err {err:.3e}, tol {tol:.3e}")
    assert err <= tol, f"{what}: dlogits err {err:.3e} > tol {tol:.3e}"
    return g


def check_dbias(db, g, what=""):
    """fp32 column sums of the unrounded gradient (tests/test_ce_tail_gpu.py:53)."""
    want = g.sum(axis=0)
    err = np.abs(f64(db) - want).max()
    tol = 1e-2 * np.abs(g).sum(axis=0).max() + 1e-6
    print(f"{what}: dbias err {err:.3e}, tol {tol:.3e}")
    assert err <= tol, f"{what}: dbias err {err:.3e} > tol {tol:.3e}"
