"""Float64 numpy oracle of gradient clipping by global norm (TF1 ``tf.clip_by_global_norm``) in
front of every update rule, written from the formulas, for ``test_clip_norm_cpu.py`` and
``test_clip_norm_gpu.py``.  It shares no code with the package.

Per step, with ``wd`` the variable's weight decay:

    g_eff       = grad * grad_scale + wd * p                       every variable, biases included
    global_norm = sqrt(sum over ALL variables of sum(g_eff^2))
    s           = c / max(global_norm, c)                          1 for global_norm <= c (0 included)
                  NaN for a non-finite global_norm
    the rule sees g_eff * s

    sgd       p -= lr g
    momentum  v = mu v + g;  p -= lr v                              slot (v,)
    nesterov  v = mu v + g;  p -= lr (g + mu v)                     slot (v,)
    adam / rmsprop / adagrad: ``adaptive_oracle.Oracle``, fed g_eff * s as its gradient

then the weight EMA ``ema -= (1 - d) (ema - p)`` with ``d = min(ema_max, (1 + step) / (10 + step))``.
``norms``, ``scales`` and ``active`` record, per step, the norm, s and whether s < 1.
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("adaptive_oracle",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                            "adaptive_oracle.py"))
adaptive_oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(adaptive_oracle)
close = adaptive_oracle.close

CLASSIC = ("sgd", "momentum", "nesterov")
RULES = CLASSIC + ("adam", "rmsprop", "adagrad")


def clip_scale(norm, c):
    if c is None:
        return 1.0
    if not np.isfinite(norm):
        return float("nan")
    return c / max(norm, c)


class ClipOracle:
    """State of named tensors in float64 (``p``, ``s1``, ``s2``, ``ema``); ``step(grads)`` applies
    one clipped update.  clip_norm None: no clipping."""

    def __init__(self, rule, params, wds, lr0, decay_rate, decay_steps, ema_max, clip_norm, grad_scale=1.0, step0=0,
                 mu=0.9, **hyper):
        assert rule in RULES, rule
        self.rule, self.clip_norm, self.grad_scale, self.mu = rule, clip_norm, grad_scale, mu
        self.wd = {n: float(wds.get(n) or 0.0) for n in params}
        self.norms, self.scales, self.active = [], [], []
        if rule in CLASSIC:
            self.inner = None
            self.p = {n: np.asarray(v, dtype=np.float64).copy() for n, v in params.items()}
            self.s1 = {n: np.zeros_like(v) for n, v in self.p.items()}
            self.s2 = {}
            self.ema = {n: v.copy() for n, v in self.p.items()}
            self.lr0, self.decay_rate, self.decay_steps, self.ema_max = lr0, decay_rate, decay_steps, ema_max
            self._step = step0
        else:
            # the inner oracle gets the clipped effective gradient: no weight decay or scale of its own
            self.inner = adaptive_oracle.Oracle(rule, params, {}, lr0, decay_rate, decay_steps, ema_max,
                                                grad_scale=1.0, step0=step0, **hyper)
            self.p, self.s1, self.s2, self.ema = self.inner.p, self.inner.s1, self.inner.s2, self.inner.ema

    @property
    def global_step(self):
        return self._step if self.inner is None else self.inner.global_step

    def lr(self):
        if self.inner is not None:
            return self.inner.lr()
        if self.decay_steps <= 0:
            return self.lr0
        return self.lr0 * self.decay_rate ** (self._step // self.decay_steps)

    def step(self, grads):
        with np.errstate(invalid="ignore", over="ignore"):
            g = {n: np.asarray(grads[n], dtype=np.float64) * self.grad_scale + self.wd[n] * self.p[n] for n in self.p}
            norm = float(np.sqrt(sum(float((v * v).sum()) for v in g.values())))
            s = clip_scale(norm, self.clip_norm)
            self.norms.append(norm)
            self.scales.append(s)
            self.active.append(bool(s < 1.0))
            g = {n: v * s for n, v in g.items()}
            if self.inner is not None:
                self.inner.step(g)
                return
            lr = self.lr()
            for n in self.p:
                if self.rule == "sgd":
                    upd = g[n]
                else:
                    v = self.s1[n] = self.mu * self.s1[n] + g[n]
                    upd = g[n] + self.mu * v if self.rule == "nesterov" else v
                p = self.p[n] = self.p[n] - lr * upd
                if self.ema_max >= 0:
                    d = min(self.ema_max, (1.0 + self._step) / (10.0 + self._step))
                    self.ema[n] = self.ema[n] - (1 - d) * (self.ema[n] - p)
            self._step += 1


def opt_config_kwargs(rule, mu=0.9):
    """Keyword arguments of the package's OptConfig that select ``rule`` (names only: the
    oracle imports nothing from the package)."""
    if rule in CLASSIC:
        return {"rule": "sgd", "use_momentum": rule != "sgd", "nesterov": rule == "nesterov",
                "momentum": mu if rule != "sgd" else 0.0}
    return {"rule": rule}
