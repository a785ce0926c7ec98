"""Confusion matrix, top-k and calibration metrics of a pass over a split.

This file is the definition and the host reference (float64 numpy) of what
``csrc/kernels/eval_metrics.hip`` computes on the device; the CPU executors, the tests and
``EvalAccumulator`` (for CPU tensors) use it directly.

Inputs: logits ``[B, ld]`` with ``NC`` real classes in columns ``0 .. NC - 1``, int labels ``[B]``
or none, a temperature ``T > 0`` and a bin count ``NB``.  ``l_c`` are the raw logits.

* A row is **bad** if any ``l_c``, ``c < NC``, is not finite: it counts in ``n_rows`` (every row
  seen) and ``n_bad`` and in nothing else.
* A row is **labelled** if labels were given and ``0 <= y < NC``.  An unlabelled row (image-mode
  inference, a ``-1`` label) counts in ``n_rows`` and in the extra confusion row ``NC`` only.
* ``pred`` is the first argmax (``np.argmax``).
* ``rank = #{c : l_c > l_y} + #{c < y : l_c == l_y}``, on the raw logits: exact, independent of
  ``T``, and 0 if and only if ``pred == y``.  Top-k accuracy is ``sum_{r<k} rank_hist[r] / n_labelled``.
* Probabilities::

      d_c   = (l_c - mx) * (1 / T)
      se    = sum_{c < NC} exp(d_c)         in class order
      conf  = 1 / se
      nll   = log(se) - d_y
      brier = sum_c (exp(d_c) / se - [c == y])^2
      bin   = min(NB - 1, int(conf * NB))

Accumulators (a dict; every call adds, the caller zeroes): ``confusion [NC + 1, NC]``,
``rank_hist [NC]``, ``bin_count [NB]``, ``bin_correct [NB]`` (int64 arrays), ``n_rows``,
``n_labelled``, ``n_bad`` (ints); ``bin_conf_sum [NB]`` (float64 array), ``nll_sum``, ``brier_sum``
(floats).  ``sum(confusion) + n_bad == n_rows``.

The per-row record is ``int32 [B, 4] = (pred, rank, bin, bits of conf as fp32)``; an unlabelled
row has ``rank = bin = -1``, a bad row ``(-1, -1, -1, bits of NaN)``.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

INT_KEYS = ("confusion", "rank_hist", "bin_count", "bin_correct")
COUNT_KEYS = ("n_rows", "n_labelled", "n_bad")
NAN_BITS = 0x7FC00000


def new_acc(n_classes: int, n_bins: int = 15) -> Dict[str, object]:
    """Zeroed accumulators."""
    return {"confusion": np.zeros((n_classes + 1, n_classes), np.int64),
            "rank_hist": np.zeros(n_classes, np.int64),
            "bin_count": np.zeros(n_bins, np.int64), "bin_correct": np.zeros(n_bins, np.int64),
            "n_rows": 0, "n_labelled": 0, "n_bad": 0,
            "bin_conf_sum": np.zeros(n_bins, np.float64), "nll_sum": 0.0, "brier_sum": 0.0}


def merge_acc(a: Dict[str, object], b: Dict[str, object]) -> Dict[str, object]:
    """a += b; returns a."""
    for k in INT_KEYS + ("bin_conf_sum",):
        a[k] += b[k]
    for k in COUNT_KEYS:
        a[k] = int(a[k]) + int(b[k])
    for k in ("nll_sum", "brier_sum"):
        a[k] = float(a[k]) + float(b[k])
    return a


def _check(n_classes: int, temperature: float, n_bins: int) -> None:
    if not 2 <= int(n_classes) <= 64:
        raise ValueError(f"n_classes: needs 2 <= NC <= 64, got {n_classes}")
    if not (math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"temperature: must be finite and > 0, got {temperature}")
    if not 1 <= int(n_bins) <= 64:
        raise ValueError(f"n_bins: needs 1 <= NB <= 64, got {n_bins}")


def _host(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        t = t.detach()
        if t.dtype == torch.bfloat16:
            t = t.float()
        return t.cpu().numpy()
    return np.asarray(t)


def reference(logits, labels, n_classes: int, temperature: float = 1.0, n_bins: int = 15,
              acc: Optional[Dict[str, object]] = None, rows: bool = False):
    """The accumulators of ``logits`` (all its rows; an array or a tensor) in float64, added to
    ``acc`` (default: fresh ones).  Returns ``acc``, or ``(acc, rows int32 [B, 4])`` with ``rows``."""
    _check(n_classes, temperature, n_bins)
    NC, NB = int(n_classes), int(n_bins)
    L = _host(logits)
    if L.ndim != 2 or L.shape[1] < NC:
        raise ValueError(f"logits: needs [B, ld >= {NC}], got {L.shape}")
    L = L[:, :NC].astype(np.float64)
    B = L.shape[0]
    if acc is None:
        acc = new_acc(NC, NB)
    if labels is None:
        y = np.full(B, -1, np.int64)
    else:
        y = _host(labels).astype(np.int64).reshape(-1)
        if y.shape[0] < B:
            raise ValueError(f"labels: needs {B} elements, has {y.shape[0]}")
        y = y[:B]
    rec = np.empty((B, 4), np.int32)
    rec[:, :3] = -1
    rec[:, 3] = np.array(NAN_BITS, np.uint32).view(np.int32)
    bad = ~np.isfinite(L).all(axis=1)
    good = ~bad
    acc["n_rows"] = int(acc["n_rows"]) + B
    acc["n_bad"] = int(acc["n_bad"]) + int(bad.sum())
    if good.any():
        G = L[good]
        yg = y[good]
        pred = G.argmax(axis=1)
        mx = G.max(axis=1)
        d = (G - mx[:, None]) * (1.0 / float(temperature))
        e = np.exp(d)
        se = np.zeros(G.shape[0])
        for c in range(NC):                       # in class order
            se = se + e[:, c]
        conf = 1.0 / se
        lab = (yg >= 0) & (yg < NC)
        rank = np.full(G.shape[0], -1, np.int64)
        binx = np.full(G.shape[0], -1, np.int64)
        np.add.at(acc["confusion"], (np.full(int((~lab).sum()), NC), pred[~lab]), 1)
        if lab.any():
            Gl, yl, pl = G[lab], yg[lab], pred[lab]
            idx = np.arange(Gl.shape[0])
            ly = Gl[idx, yl]
            cols = np.arange(NC)[None, :]
            rk = (Gl > ly[:, None]).sum(axis=1) + ((Gl == ly[:, None]) & (cols < yl[:, None])).sum(axis=1)
            dl, el, sel, cl = d[lab], e[lab], se[lab], conf[lab]
            nll = np.log(sel) - dl[idx, yl]
            q = el / sel[:, None]
            q[idx, yl] -= 1.0
            q2 = q * q
            brier = np.zeros(Gl.shape[0])
            for c in range(NC):
                brier = brier + q2[:, c]
            b = np.minimum(NB - 1, (cl * NB).astype(np.int64))
            np.add.at(acc["confusion"], (yl, pl), 1)
            np.add.at(acc["rank_hist"], rk, 1)
            np.add.at(acc["bin_count"], b, 1)
            np.add.at(acc["bin_correct"], b[rk == 0], 1)
            np.add.at(acc["bin_conf_sum"], b, cl)
            acc["n_labelled"] = int(acc["n_labelled"]) + int(lab.sum())
            acc["nll_sum"] = float(acc["nll_sum"]) + float(nll.sum())
            acc["brier_sum"] = float(acc["brier_sum"]) + float(brier.sum())
            rank[lab], binx[lab] = rk, b
        gi = np.nonzero(good)[0]
        rec[gi, 0] = pred
        rec[gi, 1] = rank
        rec[gi, 2] = binx
        rec[gi, 3] = conf.astype(np.float32).view(np.int32)
    return (acc, rec) if rows else acc


def _div(a, b) -> float:
    return float(a) / float(b) if b else 0.0


def derive(acc: Dict[str, object]) -> Dict[str, object]:
    """The reported metrics of a set of accumulators (plain Python numbers and lists, so the
    result goes to JSON as it is).  A 0 / 0 is 0.0 (scikit-learn's ``zero_division=0``)."""
    conf_m = np.asarray(acc["confusion"], np.int64)
    NC = conf_m.shape[1]
    rank_hist = np.asarray(acc["rank_hist"], np.int64)
    cnt = np.asarray(acc["bin_count"], np.int64)
    cor = np.asarray(acc["bin_correct"], np.int64)
    csum = np.asarray(acc["bin_conf_sum"], np.float64)
    n_lab = int(acc["n_labelled"])
    out: Dict[str, object] = {}
    for k in (1, 2, 3, 5):
        if k <= NC:
            out[f"top{k}"] = _div(int(rank_hist[:k].sum()), n_lab)
    out["nll"] = _div(acc["nll_sum"], n_lab)
    out["brier"] = _div(acc["brier_sum"], n_lab)
    ece, mce, table = 0.0, 0.0, []
    for b in range(cnt.shape[0]):
        n = int(cnt[b])
        a, c = _div(int(cor[b]), n), _div(csum[b], n)
        table.append([n, a, c])
        if n:
            gap = abs(a - c)
            ece += n / n_lab * gap
            mce = max(mce, gap)
    out["ece"], out["mce"] = ece, mce
    cm = conf_m[:NC]
    tp = np.diag(cm)
    support = cm.sum(axis=1)
    predicted = cm.sum(axis=0)
    prec = [_div(int(tp[c]), int(predicted[c])) for c in range(NC)]
    rec = [_div(int(tp[c]), int(support[c])) for c in range(NC)]
    f1 = [_div(2.0 * p * r, p + r) for p, r in zip(prec, rec)]
    out["precision"], out["recall"], out["f1"] = prec, rec, f1
    out["support"] = [int(s) for s in support]
    out["macro_f1"] = float(sum(f1) / NC)
    out["confusion"] = conf_m.tolist()
    out["reliability"] = table
    for k in COUNT_KEYS:
        out[k] = int(acc[k])
    return out


class EvalAccumulator:
    """The accumulators of one pass, where the logits live.

    On a HIP device it owns ``acc_i`` / ``acc_f`` (one byte buffer, so ``result()`` is ONE copy to
    the host) and the kernel's scratch; ``add`` launches ``eval_metrics`` on the caller's stream
    and never synchronises.  CPU tensors given to ``add`` go through ``reference`` into host
    accumulators; ``result()`` is the sum of both."""

    def __init__(self, device, n_classes: int, temperature: float = 1.0, n_bins: int = 15):
        _check(n_classes, temperature, n_bins)
        self.device = torch.device(device)
        self.n_classes, self.n_bins, self.temperature = int(n_classes), int(n_bins), float(temperature)
        self._host_acc: Optional[Dict[str, object]] = None
        self.copies = 0                 # D2H copies so far (one per result() of a device pass)
        self._buf: Optional[torch.Tensor] = None
        if self.device.type == "cuda":
            from ..ops._ext import kernels
            self.K = kernels()
            self.layout = dict(self.K.eval_metrics_layout(self.n_classes, self.n_bins))
            ni, nf = self.layout["size_i"], self.layout["size_f"]
            self._buf = torch.zeros((ni + nf) * 8, dtype=torch.uint8, device=self.device)
            self.acc_i = self._buf[:ni * 8].view(torch.int64)
            self.acc_f = self._buf[ni * 8:].view(torch.float64)
            self.scratch = torch.empty(int(self.K.eval_metrics_scratch_size(self.n_bins)), dtype=torch.float64,
                                       device=self.device)
        self._device_used = False

    def zero(self) -> None:
        self._host_acc = None
        if self._buf is not None:
            self._buf.zero_()
        self._device_used = False

    def add(self, logits: torch.Tensor, labels: Optional[torch.Tensor], nb: Optional[int] = None,
            rows: Optional[torch.Tensor] = None, temperature: Optional[float] = None):
        """Adds rows ``0 .. nb - 1`` of ``logits`` (default: all).  ``rows``: on the device an
        ``int32 [B, 4]`` tensor the per-row records are written to; on the CPU any true value makes
        the call return them."""
        nb = int(logits.shape[0]) if nb is None else int(nb)
        T = self.temperature if temperature is None else float(temperature)
        if not 0 <= nb <= logits.shape[0]:
            raise ValueError(f"nb: needs 0 <= nb <= B = {logits.shape[0]}, got {nb}")
        if isinstance(logits, torch.Tensor) and logits.is_cuda:
            if self._buf is None:
                raise ValueError(f"EvalAccumulator on {self.device} was given logits on {logits.device}")
            self.K.eval_metrics(logits, labels, nb, self.n_classes, self.acc_i, self.acc_f, self.scratch, rows, T,
                                self.n_bins)
            self._device_used = True
            return rows
        if self._host_acc is None:
            self._host_acc = new_acc(self.n_classes, self.n_bins)
        out = reference(logits[:nb], None if labels is None else labels[:nb], self.n_classes, T, self.n_bins,
                        acc=self._host_acc, rows=rows is not None and rows is not False)
        return out[1] if isinstance(out, tuple) else None

    def result(self) -> Dict[str, object]:
        acc = new_acc(self.n_classes, self.n_bins)
        if self._device_used:
            L, ni = self.layout, self.layout["size_i"]
            host = self._buf.cpu().numpy()
            self.copies += 1
            hi, hf = host[:ni * 8].view(np.int64), host[ni * 8:].view(np.float64)
            NC, NB = self.n_classes, self.n_bins
            acc["confusion"] = hi[L["confusion"]:L["confusion"] + (NC + 1) * NC].reshape(NC + 1, NC).copy()
            acc["rank_hist"] = hi[L["rank_hist"]:L["rank_hist"] + NC].copy()
            acc["bin_count"] = hi[L["bin_count"]:L["bin_count"] + NB].copy()
            acc["bin_correct"] = hi[L["bin_correct"]:L["bin_correct"] + NB].copy()
            for j, k in enumerate(COUNT_KEYS):
                acc[k] = int(hi[L["counts"] + j])
            acc["bin_conf_sum"] = hf[L["bin_conf_sum"]:L["bin_conf_sum"] + NB].copy()
            acc["nll_sum"], acc["brier_sum"] = float(hf[L["nll_sum"]]), float(hf[L["brier_sum"]])
        if self._host_acc is not None:
            merge_acc(acc, self._host_acc)
        return acc


def fit_temperature(logits, labels, n_classes: int, lo: float = 0.05, hi: float = 20.0, iters: int = 48) -> float:
    """The temperature in ``[lo, hi]`` that minimises the NLL of ``logits`` (all rows, held by the
    caller) against ``labels``: a golden-section search over ``beta = 1 / T``, in which the NLL is
    convex.  Device tensors are evaluated by the kernel (one launch pair and one small copy per
    probe), anything else by ``reference``.  Returns ``T`` of the best probe."""
    if not (0 < lo < hi and math.isfinite(hi)):
        raise ValueError(f"fit_temperature: needs 0 < lo < hi, got {lo}, {hi}")
    on_dev = isinstance(logits, torch.Tensor) and logits.is_cuda
    acc = EvalAccumulator(logits.device if on_dev else "cpu", n_classes, 1.0, 1)

    def f(beta: float) -> float:
        acc.zero()
        acc.add(logits, labels, None, temperature=1.0 / beta)
        return float(acc.result()["nll_sum"])

    g = (math.sqrt(5.0) - 1.0) / 2.0
    a, b = 1.0 / hi, 1.0 / lo
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = f(c), f(d)
    best: Tuple[float, float] = (fc, c) if fc <= fd else (fd, d)
    for _ in range(int(iters)):
        if fc <= fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a)
            fc = f(c)
            best = min(best, (fc, c))
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a)
            fd = f(d)
            best = min(best, (fd, d))
    return 1.0 / best[1]
