"""Float64 numpy oracle of the layer-wise rules LARS (You et al. 2017, on momentum) and LAMB (You
et al. 2019, on Adam, without decoupled decay), written from the formulas, for
``test_layerwise_opt_cpu.py`` and ``test_layerwise_opt_gpu.py``.  It shares no code with the package.

Per step and per variable k, with ``wd`` the variable's weight decay and ``t = global_step + 1``:

    g = grad * grad_scale + wd * p
    adapted: rank >= 2 (the */weights); biases always get ratio 1

    lars   pn = ||p||2   gn = ||g||2
           r  = eta * pn / (gn + eps)      if adapted and pn > 0 and gn > 0, else 1
           v  = mu v + r g ;  p -= lr v                                      slot (v,)
    lamb   m  = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g^2
           u  = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)
           pn = ||p||2   un = ||u||2
           r  = pn / un                    if adapted and pn > 0 and un > 0, else 1
           p -= lr r u                                                       slots (m, v)

    a non-finite pn, gn or un of an adapted variable gives r = NaN

then the weight EMA ``ema -= (1 - d) (ema - p)`` with ``d = min(ema_max, (1 + step) / (10 + step))``.
``pn``, ``un`` (gn for lars) and ``r`` record, per step, a dict name -> value.
"""
import importlib.util
import math
import os

import numpy as np

RULES = ("lars", "lamb")


_spec = importlib.util.spec_from_file_location("adaptive_oracle",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                            "adaptive_oracle.py"))
adaptive_oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(adaptive_oracle)
close = adaptive_oracle.close     # max |out - ref| <= 1e-5 * max |ref| + 1e-6


def close_scalar(got, want, rel=1e-5):
    """Norms and ratios: 1e-5 relative, as test_clip_norm_gpu.py takes the global norm."""
    assert np.isfinite(got) and abs(got - want) <= rel * abs(want), (got, want)


def var_norms(rule, p, g_eff, m=None, v=None, t=1, b1=0.9, b2=0.999, eps=None):
    """(pn, un) of one variable in float64; lamb: from the slots *before* the step."""
    p = np.asarray(p, dtype=np.float64)
    g = np.asarray(g_eff, dtype=np.float64)
    if rule == "lars":
        return float(np.sqrt((p * p).sum())), float(np.sqrt((g * g).sum()))
    eps = 1e-6 if eps is None else eps
    m = b1 * np.asarray(m, dtype=np.float64) + (1 - b1) * g
    v = b2 * np.asarray(v, dtype=np.float64) + (1 - b2) * g * g
    u = (m / -math.expm1(t * math.log(b1))) / (np.sqrt(v / -math.expm1(t * math.log(b2))) + eps)
    return float(np.sqrt((p * p).sum())), float(np.sqrt((u * u).sum()))


def ratio(rule, adapted, pn, un, eta=0.001, eps=0.0):
    if not adapted:
        return 1.0
    if not (np.isfinite(pn) and np.isfinite(un)):
        return float("nan")
    if not (pn > 0 and un > 0):
        return 1.0
    return pn / un if rule == "lamb" else eta * pn / (un + eps)


class LayerwiseOracle:
    """State of named tensors in float64 (``p``, ``s1``, ``s2``, ``ema``); ``step(grads)`` applies one
    update.  ``adapted``: name -> bool, default rank >= 2."""

    def __init__(self, rule, params, wds, lr0, decay_rate, decay_steps, ema_max, grad_scale=1.0, step0=0, mu=0.9,
                 eta=0.001, b1=0.9, b2=0.999, eps=None, adapted=None):
        assert rule in RULES, rule
        self.rule, self.grad_scale, self.mu, self.eta, self.b1, self.b2 = rule, grad_scale, mu, eta, b1, b2
        self.eps = ({"lars": 0.0, "lamb": 1e-6}[rule]) if eps is None else eps
        self.p = {n: np.asarray(v, dtype=np.float64).copy() for n, v in params.items()}
        self.wd = {n: float(wds.get(n) or 0.0) for n in self.p}
        self.adapted = {n: (v.ndim >= 2 if adapted is None else bool(adapted[n])) for n, v in self.p.items()}
        self.s1 = {n: np.zeros_like(v) for n, v in self.p.items()}
        self.s2 = {n: np.zeros_like(v) for n, v in self.p.items()} if rule == "lamb" else {}
        self.ema = {n: v.copy() for n, v in self.p.items()}
        self.lr0, self.decay_rate, self.decay_steps, self.ema_max = lr0, decay_rate, decay_steps, ema_max
        self.global_step = step0
        self.pn, self.un, self.r = [], [], []

    def lr(self):
        if self.decay_steps <= 0:
            return self.lr0
        return self.lr0 * self.decay_rate ** (self.global_step // self.decay_steps)

    def step(self, grads):
        lr, t = self.lr(), self.global_step + 1
        pns, uns, rs = {}, {}, {}
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for n in self.p:
                p = self.p[n]
                g = np.asarray(grads[n], dtype=np.float64) * self.grad_scale + self.wd[n] * p
                pn = float(np.sqrt((p * p).sum()))
                if self.rule == "lars":
                    un = float(np.sqrt((g * g).sum()))
                    r = ratio("lars", self.adapted[n], pn, un, self.eta, self.eps)
                    v = self.s1[n] = self.mu * self.s1[n] + r * g
                    p = self.p[n] = p - lr * v
                else:
                    m = self.s1[n] = self.b1 * self.s1[n] + (1 - self.b1) * g
                    v = self.s2[n] = self.b2 * self.s2[n] + (1 - self.b2) * g * g
                    c1 = -math.expm1(t * math.log(self.b1))
                    c2 = -math.expm1(t * math.log(self.b2))
                    u = (m / c1) / (np.sqrt(v / c2) + self.eps)
                    un = float(np.sqrt((u * u).sum()))
                    r = ratio("lamb", self.adapted[n], pn, un)
                    p = self.p[n] = p - lr * r * u
                pns[n], uns[n], rs[n] = pn, un, r
                if self.ema_max >= 0:
                    d = min(self.ema_max, (1.0 + self.global_step) / (10.0 + self.global_step))
                    self.ema[n] = self.ema[n] - (1 - d) * (self.ema[n] - p)
        self.pn.append(pns)
        self.un.append(uns)
        self.r.append(rs)
        self.global_step += 1
