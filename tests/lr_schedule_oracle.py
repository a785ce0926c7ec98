"""Float64 oracle of the learning-rate schedules (linear warmup in front of the staircase, of
polynomial decay and of cosine decay), written from the formulas, for ``test_lr_schedule_cpu.py``
and ``test_lr_schedule_gpu.py``.  It shares no code with the package.

With ``t`` the global step the update reads, ``W`` the warmup steps and ``T`` the total steps:

    warm(t) = (t + 1) / W            if W > 0 and t < W,   else 1
    x(t)    = 0 if t <= W;  1 if t >= T;  else (t - W) / (T - W)

    staircase   base = lr0 * decay_rate ** (t // decay_steps)        (decay_steps <= 0: lr0)
    polynomial  base = lr_end + (lr0 - lr_end) * (1 - x) ** power
    cosine      base = lr_end + (lr0 - lr_end) * 0.5 * (1 + cos(pi x))

    lr(t) = warm(t) * base(t)

``lr`` is that in Python floats.  ``lr_f32`` transcribes the device function operation by operation
into numpy float32: its distance from ``lr`` is what single precision costs, and the GPU tests
derive their bound from it.  The ``Scheduled*`` classes are the existing optimizer oracles with
their ``lr()`` replaced; a schedule is the dict ``{"kind", "W", "T", "lr_end", "power"}``.
"""
import importlib.util
import math
import os

import numpy as np

KINDS = ("staircase", "polynomial", "cosine")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                     name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


adaptive_oracle = _load("adaptive_oracle")
clip_oracle = _load("clip_oracle")
layerwise_oracle = _load("layerwise_oracle")
close = adaptive_oracle.close     # max |out - ref| <= 1e-5 * max |ref| + 1e-6


def schedule(kind="staircase", W=0, T=0, lr_end=0.0, power=1.0):
    assert kind in KINDS, kind
    return {"kind": kind, "W": int(W), "T": int(T), "lr_end": float(lr_end), "power": float(power)}


def lr(t, lr0, decay_rate=0.1, decay_steps=0, kind="staircase", W=0, T=0, lr_end=0.0, power=1.0):
    t = int(t)
    warm = (t + 1) / W if (W > 0 and t < W) else 1.0
    if kind == "staircase":
        base = lr0 if decay_steps <= 0 else lr0 * decay_rate ** (t // decay_steps)
        return warm * base
    x = 0.0 if t <= W else 1.0 if t >= T else (t - W) / (T - W)
    if kind == "polynomial":
        base = lr_end + (lr0 - lr_end) * (1.0 - x) ** power
    elif kind == "cosine":
        base = lr_end + (lr0 - lr_end) * 0.5 * (1.0 + math.cos(math.pi * x))
    else:
        raise ValueError(kind)
    return warm * base


def lr_f32(steps, lr0, decay_rate=0.1, decay_steps=0, kind="staircase", W=0, T=0, lr_end=0.0, power=1.0):
    """The device function in numpy float32, one rounding per operation, over an int64 vector."""
    f = np.float32
    t = np.asarray(steps, dtype=np.int64)
    lr0, lr_end, power, rate = f(lr0), f(lr_end), f(power), f(decay_rate)
    base = np.full(t.shape, lr0, dtype=np.float32)
    if kind == "staircase":
        if decay_steps > 0:
            base = base * np.power(rate, (t // decay_steps).astype(np.float32))
    else:
        with np.errstate(invalid="ignore"):
            x = (t - W).astype(np.float32) / f(T - W)
            if kind == "polynomial":
                shape = np.power(f(1.0) - x, power)
            else:
                shape = f(0.5) * (f(1.0) + np.cos(f(3.14159265358979) * x))
            mid = lr_end + (lr0 - lr_end) * shape
        base = np.where(t > W, mid.astype(np.float32), base)
        base = np.where(t >= T, lr_end, base).astype(np.float32)
    if W > 0:
        base = np.where(t < W, (t + 1).astype(np.float32) / f(W) * base, base).astype(np.float32)
    assert base.dtype == np.float32
    return base


class ScheduledOracle(adaptive_oracle.Oracle):
    """adam / rmsprop / adagrad with the scheduled rate."""

    def __init__(self, *args, sched, **kw):
        super().__init__(*args, **kw)
        self.sched = dict(sched)

    def lr(self):
        return lr(self.global_step, self.lr0, self.decay_rate, self.decay_steps, **self.sched)


class ScheduledClipOracle(clip_oracle.ClipOracle):
    """sgd / momentum / nesterov, and any rule behind clipping, with the scheduled rate."""

    def __init__(self, rule, params, wds, lr0, decay_rate, decay_steps, ema_max, clip_norm, *, sched, step0=0, **kw):
        super().__init__(rule, params, wds, lr0, decay_rate, decay_steps, ema_max, clip_norm, step0=step0, **kw)
        self.sched = dict(sched)
        if self.inner is not None:      # the adaptive rules step through an inner oracle: it takes the rate
            hyper = {k: v for k, v in kw.items() if k not in ("grad_scale", "mu")}
            self.inner = ScheduledOracle(rule, params, {}, lr0, decay_rate, decay_steps, ema_max, grad_scale=1.0,
                                         step0=step0, sched=sched, **hyper)
            self.p, self.s1, self.s2, self.ema = self.inner.p, self.inner.s1, self.inner.s2, self.inner.ema

    def lr(self):
        if self.inner is not None:
            return self.inner.lr()
        return lr(self._step, self.lr0, self.decay_rate, self.decay_steps, **self.sched)


class ScheduledLayerwiseOracle(layerwise_oracle.LayerwiseOracle):
    """lars / lamb with the scheduled rate."""

    def __init__(self, *args, sched, **kw):
        super().__init__(*args, **kw)
        self.sched = dict(sched)

    def lr(self):
        return lr(self.global_step, self.lr0, self.decay_rate, self.decay_steps, **self.sched)


RULES = ("sgd", "momentum", "adam", "rmsprop", "adagrad", "adam+clip", "lars", "lamb")


def make(rule, params, wds, lr0, decay_rate, decay_steps, ema_max, sched, grad_scale=1.0, step0=0, clip_norm=1.0,
         **kw):
    """The scheduled oracle of one of RULES ("adam+clip": adam behind clip_norm)."""
    if rule in ("sgd", "momentum"):
        return ScheduledClipOracle(rule, params, wds, lr0, decay_rate, decay_steps, ema_max, None, sched=sched,
                                   grad_scale=grad_scale, step0=step0, **kw)
    if rule == "adam+clip":
        return ScheduledClipOracle("adam", params, wds, lr0, decay_rate, decay_steps, ema_max, clip_norm, sched=sched,
                                   grad_scale=grad_scale, step0=step0, **kw)
    if rule in ("lars", "lamb"):
        return ScheduledLayerwiseOracle(rule, params, wds, lr0, decay_rate, decay_steps, ema_max, sched=sched,
                                        grad_scale=grad_scale, step0=step0, **kw)
    return ScheduledOracle(rule, params, wds, lr0, decay_rate, decay_steps, ema_max, sched=sched,
                           grad_scale=grad_scale, step0=step0, **kw)


def opt_config_kwargs(rule, sched, mu=0.9, clip_norm=1.0):
    """Keyword arguments of the package's OptConfig for one of RULES and a schedule (names only)."""
    kw = {"schedule": sched["kind"], "warmup_steps": sched["W"], "total_steps": sched["T"], "lr_end": sched["lr_end"],
          "lr_power": sched["power"]}
    if rule in ("sgd", "momentum"):
        kw.update(clip_oracle.opt_config_kwargs(rule, mu))
    elif rule == "adam+clip":
        kw.update(rule="adam", clip_norm=clip_norm)
    elif rule == "lars":
        kw.update(rule="lars", momentum=mu)
    else:
        kw.update(rule=rule)
    return kw
