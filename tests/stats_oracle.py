"""Float64 numpy oracle of what the training loop observes of a batch of logits, written from
the formulas, for ``test_stats_path_gpu.py``.  It shares no code with the package.

    cross-entropy sum   sum_rows  logsumexp(logits) - logits[label]
    top-1 count         #rows with logits[label] >= max(logits): the reference's tf.nn.in_top_k
                        rule (mnist_input.py:237-243), under which a tie at the maximum counts
                        for every tied class
    probs               softmax(logits)
    dlogits             (softmax(logits) - onehot(label)) * scale

The log-sum-exp subtracts the row maximum, so +-3e38 logits stay finite in float64.
"""
import numpy as np


def f64(t):
    """A tensor (any device / dtype) or array as a float64 numpy array."""
    if hasattr(t, "detach"):
        t = t.detach().double().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def i64(t):
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.int64)


def log_softmax(logits):
    z = f64(logits)
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def ce_sum(logits, labels):
    lsm = log_softmax(logits)
    return float(-lsm[np.arange(lsm.shape[0]), i64(labels)].sum())


def top1_count(logits, labels):
    z = f64(logits)
    return int((z[np.arange(z.shape[0]), i64(labels)] >= z.max(axis=1)).sum())


def softmax(logits):
    return np.exp(log_softmax(logits))


def dlogits(logits, labels, scale):
    g = softmax(logits)
    g[np.arange(g.shape[0]), i64(labels)] -= 1.0
    return g * scale


def ce_tol(ce):
    """Bound on the kernels' loss sum (fast exp / log intrinsics), tests/test_ce_tail_gpu.py."""
    return 1e-4 * abs(ce) + 1e-4


def check_ce(got, ce, what=""):
    assert np.isfinite(got), f"{what}: loss {got}"
    assert abs(got - ce) <= ce_tol(ce), f"{what}: loss {got!r} vs float64 {ce!r} (tol {ce_tol(ce):.3e})"


def check_dlogits(dl, logits, labels, scale, what=""):
    """One bf16 rounding plus intrinsic error: 2**-8 of the largest gradient."""
    g = dlogits(logits, labels, scale)
    err = np.abs(f64(dl) - g).max()
    assert err <= 2.0 ** -8 * np.abs(g).max(), f"{what}: dlogits err {err:.3e} vs max |g| {np.abs(g).max():.3e}"


def check_probs(pr, logits, what=""):
    """tests/test_kernels_gpu.py::test_softmax_ce's measure at rel = 1e-5; rows sum to 1."""
    ref = softmax(logits)
    out = f64(pr)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    tol = 1e-5 * np.abs(ref).max() + 1e-6
    err = np.abs(out - ref).max()
    assert err <= tol, f"{what}: probs err {err:.3e} > tol {tol:.3e}"
    s = np.abs(out.sum(axis=1) - 1.0).max()
    assert s <= 1e-5 + 1e-6, f"{what}: probs rows sum to 1 +- {s:.3e}"
