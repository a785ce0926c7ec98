"""Float64 numpy oracle of the optimizer's adaptive rules (Adam, RMSProp, Adagrad with TF1
semantics), written from the formulas, for ``test_adaptive_opt_cpu.py`` and
``test_adaptive_opt_gpu.py``.  It shares no code with the package.

In every rule ``g = grad * grad_scale + wd * p`` and ``t = global_step + 1``:

    adam     m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2
             p -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps)        slots (m, v)
    rmsprop  ms = rho ms + (1 - rho) g^2;  mom = mu mom + lr g / sqrt(ms + eps);  p -= mom
                                                                              slots (mom, ms); ms starts at 1
    adagrad  acc += g^2;  p -= lr g / sqrt(acc)                               slot (acc,); acc starts at 0.1

then the weight EMA ``ema -= (1 - d) (ema - p)`` with ``d = min(ema_max, (1 + step) / (10 + step))``.
"""
import numpy as np

HYPER = {"beta1": 0.9, "beta2": 0.999, "adam_eps": 1e-8, "rho": 0.9, "mu": 0.0, "rms_eps": 1e-10, "acc0": 0.1}


def close(out, ref, rel=1e-5):
    """The measure tests/test_kernels_gpu.py::test_fused_optimizer uses: max |out - ref| against
    rel * max |ref| + 1e-6."""
    out = np.asarray(out, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert np.isfinite(out).all(), "non-finite values"
    tol = rel * np.abs(ref).max() + 1e-6
    err = np.abs(out - ref).max()
    assert err <= tol, f"max err {err:.3e} > tol {tol:.3e}"


class Oracle:
    """State of named tensors in float64; ``step(grads)`` applies one update."""

    def __init__(self, rule, params, wds, lr0, decay_rate, decay_steps, ema_max, grad_scale=1.0, step0=0, **hyper):
        self.rule = rule
        self.h = dict(HYPER, **hyper)
        self.p = {n: np.asarray(v, dtype=np.float64).copy() for n, v in params.items()}
        self.wd = {n: float(wds.get(n) or 0.0) for n in params}
        s1 = self.h["acc0"] if rule == "adagrad" else 0.0
        self.s1 = {n: np.full_like(v, s1) for n, v in self.p.items()}
        self.s2 = {n: np.full_like(v, 1.0 if rule == "rmsprop" else 0.0) for n, v in self.p.items()}
        self.ema = {n: v.copy() for n, v in self.p.items()}
        self.lr0, self.decay_rate, self.decay_steps, self.ema_max = lr0, decay_rate, decay_steps, ema_max
        self.grad_scale = grad_scale
        self.global_step = step0

    def lr(self):
        if self.decay_steps <= 0:
            return self.lr0
        return self.lr0 * self.decay_rate ** (self.global_step // self.decay_steps)

    def step(self, grads):
        h, lr, t = self.h, self.lr(), self.global_step + 1
        for n in self.p:
            p = self.p[n]
            g = np.asarray(grads[n], dtype=np.float64) * self.grad_scale + self.wd[n] * p
            if self.rule == "adam":
                m = self.s1[n] = h["beta1"] * self.s1[n] + (1 - h["beta1"]) * g
                v = self.s2[n] = h["beta2"] * self.s2[n] + (1 - h["beta2"]) * g * g
                p = p - lr * np.sqrt(1 - h["beta2"] ** t) / (1 - h["beta1"] ** t) * m / (np.sqrt(v) + h["adam_eps"])
            elif self.rule == "rmsprop":
                ms = self.s2[n] = h["rho"] * self.s2[n] + (1 - h["rho"]) * g * g
                mom = self.s1[n] = h["mu"] * self.s1[n] + lr * g / np.sqrt(ms + h["rms_eps"])
                p = p - mom
            elif self.rule == "adagrad":
                acc = self.s1[n] = self.s1[n] + g * g
                p = p - lr * g / np.sqrt(acc)
            else:
                raise ValueError(self.rule)
            self.p[n] = p
            if self.ema_max >= 0:
                d = min(self.ema_max, (1.0 + self.global_step) / (10.0 + self.global_step))
                self.ema[n] = self.ema[n] - (1 - d) * (self.ema[n] - p)
        self.global_step += 1
