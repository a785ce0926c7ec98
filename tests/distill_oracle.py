"""The distillation loss of the softmax-CE kernels in float64 numpy, written from its definition
(README "Distillation"); the oracle of tests/test_distill_cpu.py and tests/test_distill_gpu.py.

Per batch row, with l_c the student's NC real logits, t_c the teacher's, y the label, a = distill_alpha,
T = distill_temperature and iT = 1 / T:

    d_c = l_c - max_c l_c        se  = sum exp(d_c)      p_c  = exp(d_c) / se        hard = log(se) - d_y
    u_c = d_c * iT               seT = sum exp(u_c)      pT_c = exp(u_c) / seT
    v_c = (t_c - max_c t_c) * iT st  = sum exp(v_c)      q_c  = exp(v_c) / st
    soft = sum_c q_c * ((v_c - log st) - (u_c - log seT))
    loss = (1 - a) * hard + a * T^2 * soft
    dl_c = ((1 - a) * (p_c - [c == y]) + a * T * (pT_c - q_c)) * scale
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np


class Distilled(NamedTuple):
    loss: float        # sum over the rows of the row losses
    hard: float        # sum (1 - a) * hard
    ces: float         # sum a T^2 * CEs,  CEs = log seT - sum_c q_c u_c   (the soft cross-entropy)
    hq: float          # sum a T^2 * H(q), H(q) = -sum_c q_c (v_c - log st)  (the teacher entropy)
    soft: float        # sum a T^2 * soft  (= ces - hq, formed per class)
    dl: np.ndarray     # [nb, NC] float64
    correct: int       # rows whose label's logit is the row maximum
    rows: np.ndarray   # [nb] the row losses


def distill(logits, teacher, labels, alpha: float, T: float, scale: float = 1.0) -> Distilled:
    """``logits`` / ``teacher`` [nb, NC] (the real classes only), ``labels`` [nb]."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        l = np.asarray(logits, dtype=np.float64)
        t = np.asarray(teacher, dtype=np.float64)
        y = np.asarray(labels).astype(np.int64)
        nb, nc = l.shape
        a, T, iT = float(alpha), float(T), 1.0 / float(T)
        r = np.arange(nb)
        d = l - l.max(axis=1, keepdims=True)
        se = np.exp(d).sum(axis=1)
        p = np.exp(d) / se[:, None]
        hard = np.log(se) - d[r, y]
        u = d * iT
        seT = np.exp(u).sum(axis=1)
        pT = np.exp(u) / seT[:, None]
        v = (t - t.max(axis=1, keepdims=True)) * iT
        st = np.exp(v).sum(axis=1)
        q = np.exp(v) / st[:, None]
        lq = v - np.log(st)[:, None]
        lp = u - np.log(seT)[:, None]
        soft = (q * (lq - lp)).sum(axis=1)
        ces = np.log(seT) - (q * u).sum(axis=1)
        hq = -(q * lq).sum(axis=1)
        rows = (1.0 - a) * hard + a * T * T * soft
        onehot = np.zeros_like(l)
        onehot[r, y] = 1.0
        dl = ((1.0 - a) * (p - onehot) + a * T * (pT - q)) * scale
        correct = int((l[r, y] >= l.max(axis=1)).sum())
        return Distilled(float(rows.sum()), float(((1.0 - a) * hard).sum()), float((a * T * T * ces).sum()),
                         float((a * T * T * hq).sum()), float((a * T * T * soft).sum()), dl, correct, rows)


def loss_tol(o: Distilled) -> float:
    """The project's ``ce_tol`` applied to the magnitudes that are actually summed: the KL is the soft
    cross-entropy minus the teacher entropy, and the loss adds the weighted hard cross-entropy."""
    return 1e-4 * (abs(o.hard) + abs(o.ces) + abs(o.hq)) + 1e-4


def distill_f32(logits, teacher, labels, alpha: float, T: float) -> float:
    """The same loss sum transcribed in float32 numpy (what fp32 arithmetic alone costs)."""
    f = np.float32
    l = np.asarray(logits, dtype=f)
    t = np.asarray(teacher, dtype=f)
    y = np.asarray(labels).astype(np.int64)
    a, T, iT = f(alpha), f(T), f(1.0) / f(T)
    r = np.arange(l.shape[0])
    d = l - l.max(axis=1, keepdims=True)
    se = np.exp(d).sum(axis=1, dtype=f)
    hard = np.log(se) - d[r, y]
    u = d * iT
    seT = np.exp(u).sum(axis=1, dtype=f)
    v = (t - t.max(axis=1, keepdims=True)) * iT
    ev = np.exp(v)
    st = ev.sum(axis=1, dtype=f)
    q = ev / st[:, None]
    soft = (q * ((v - np.log(st)[:, None]) - (u - np.log(seT)[:, None]))).sum(axis=1, dtype=f)
    rows = (f(1.0) - a) * hard + a * T * T * soft
    tot = f(0.0)
    for x in rows:
        tot = f(tot + x)
    return float(tot)
