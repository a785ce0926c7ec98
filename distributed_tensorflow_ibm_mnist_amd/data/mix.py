"""Host reference of mixup and CutMix (``csrc/kernels/mix.hip``), in vectorised numpy.

Every entry of a training batch is mixed with its partner, the entry at the flipped position
``nb - 1 - b`` of the same local batch: mixup (Zhang et al., 2018) blends the two images with a
weight ``lam``, CutMix (Yun et al., 2019) pastes a box of the partner into the entry.  The loss then
takes two labels and the weight per row (the ``MIX`` form of the softmax cross-entropy kernels).

The distribution is a host table, as the elastic Gaussian is; the device knows nothing about Beta:

    T[k] = Q(0.5 + k / 2048), k = 0 .. 1024        Q the quantile function of Beta(alpha, alpha)
    S[k] = floor(28 * sqrt(1 - T_c[k])), k = 0 .. 1023     the CutMix box side in pixels, 0 .. 19

``T`` is the distribution of ``max(L, 1 - L)``: every weight is >= 0.5, so an entry's own label stays
the dominant one.  The draw of batch entry ``b`` is a pure function of ``(seed, p)``, ``p = pos0 + b``
its global stream position: one Philox4x32-10 call (``ops.dropout.philox4x32_10``), every
floating-point line below a single rounded fp32 operation

    counter = (p & 0xffffffff, p >> 32, 0, 0x41554702)     key = (seed & 0xffffffff, seed >> 32)
    apply   = (w0 >> 16) < thr_p          thr_p = clamp(floor(mix_prob * 65536 + 0.5), 0, 65536)
    cut     = cutmix on and (mixup off or (w0 & 1))
    mixup:  u = float(w1 >> 8) * 2^-24    pos = u * 1024    k = int(pos)    fr = pos - k      (all exact)
            d = T[k+1] - T[k]             lam = T[k] + fr * d
    cutmix: side = S[w1 >> 22]            cx = umulhi(w2, 28)    cy = umulhi(w3, 28)
            x0 = max(cx - side/2, 0)      x1 = min(cx - side/2 + side, 28)     (same in y; side/2 floors)
            area = (x1 - x0) * (y1 - y0)  lam = float(784 - area) / 784.0f

An entry is unmixed when ``apply`` is false, when it is its own partner (the middle entry of an odd
batch) or when its CutMix box is empty: its image is not touched, ``lam = 1`` and its second label is
its own.  With ``xa`` the entry's value and ``xb`` the partner's, both as the buffer held them:

    mixup:   om = 1 - lam;  t = om * xb;  out = bf16_rne(fmaf(lam, xa, t))
    cutmix:  out = xb inside the box (a bitwise copy, all channels), xa outside

``params`` is what the device draws, bit for bit; ``mixed`` evaluates the images in float64.  The CPU
loader path uses ``mixed`` rounded once to the buffer's dtype, and the tests' oracle is written from
the same formulas.  Nothing here needs torch or a GPU.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from ..ops.dropout import check_seed, philox4x32_10

TAG = 0x41554702          # counter word 3: continues the augmentation's tags (dropout's layer 16725)
MIN_ALPHA, MAX_ALPHA = 0.1, 8.0
TABLE_N = 1024            # intervals of the lam table (T has TABLE_N + 1 entries, S has TABLE_N)
SIDE = 28
UNMIXED, MIXUP, CUTMIX = 0, 1, 2


def check_alpha(v, key: str = "mixup_alpha") -> float:
    """``v`` as a float: 0 (off), or finite with 0.1 <= v <= 8."""
    try:
        if isinstance(v, bool):
            raise ValueError
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{key} must be 0 or a number with {MIN_ALPHA:g} <= {key} <= {MAX_ALPHA:g}, got {v!r}") from None
    if f != 0.0 and not MIN_ALPHA <= f <= MAX_ALPHA:       # NaN fails every comparison
        raise ValueError(f"{key} must be 0 or finite with {MIN_ALPHA:g} <= {key} <= {MAX_ALPHA:g}, got {f}")
    return f


def check_prob(v, key: str = "mix_prob") -> float:
    """``v`` as a float: finite with 0 <= v <= 1."""
    try:
        if isinstance(v, bool):
            raise ValueError
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{key} must be a number with 0 <= {key} <= 1, got {v!r}") from None
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"{key} must be finite with 0 <= {key} <= 1, got {f}")
    return f


def prob_threshold(prob) -> int:
    """thr_p of ``mix_prob``: an entry is mixed when the high 16 bits of its first word are below it."""
    return min(max(int(math.floor(check_prob(prob) * 65536.0 + 0.5)), 0), 65536)


@dataclasses.dataclass(frozen=True)
class MixConfig:
    """The mixing keys, checked: a ValueError names key and value."""
    mixup_alpha: float = 0.0
    cutmix_alpha: float = 0.0
    prob: float = 1.0
    seed: int = 0

    def __post_init__(self):
        object.__setattr__(self, "mixup_alpha", check_alpha(self.mixup_alpha, "mixup_alpha"))
        object.__setattr__(self, "cutmix_alpha", check_alpha(self.cutmix_alpha, "cutmix_alpha"))
        object.__setattr__(self, "prob", check_prob(self.prob, "mix_prob"))
        object.__setattr__(self, "seed", check_seed(self.seed, "mix_seed"))

    @property
    def enabled(self) -> bool:
        return self.prob > 0.0 and (self.mixup_alpha != 0.0 or self.cutmix_alpha != 0.0)

    @property
    def thr_p(self) -> int:
        return prob_threshold(self.prob)

    def with_seed(self, seed: int) -> "MixConfig":
        return dataclasses.replace(self, seed=seed)


@functools.lru_cache(maxsize=16)
def _lam_table(alpha: float) -> np.ndarray:
    from scipy.special import betaincinv
    q = 0.5 + np.arange(TABLE_N + 1, dtype=np.float64) / (2.0 * TABLE_N)
    t = betaincinv(alpha, alpha, q).astype(np.float32)
    t.setflags(write=False)
    return t


def lam_table(alpha) -> np.ndarray:
    """T[k] = Q(0.5 + k / 2048), k = 0 .. 1024: the quantiles of Beta(alpha, alpha) on its upper half,
    computed in float64 and rounded once to float32 [1025].  The device is handed this table."""
    alpha = check_alpha(alpha, "alpha")
    if alpha == 0.0:
        raise ValueError("alpha must be non-zero for a table, got 0")
    return _lam_table(alpha).copy()


def side_table(alpha) -> np.ndarray:
    """S[k] = floor(28 * sqrt(1 - T[k])), k = 0 .. 1023, evaluated in float64: the CutMix box side in
    pixels, int32 [1024] with values in 0 .. 19 (so the device takes no square root)."""
    t = lam_table(alpha)[:TABLE_N].astype(np.float64)
    return np.floor(SIDE * np.sqrt(1.0 - t)).astype(np.int32)


def _check_window(pos0, n):
    pos0, n = int(pos0), int(n)
    if pos0 < 0 or n < 0 or pos0 + n > 1 << 63:
        raise ValueError(f"pos0 must be >= 0 with pos0 + n <= 2^63, got {pos0} (n = {n})")
    return pos0, n


def params(cfg: MixConfig, pos0: int, n: int) -> np.ndarray:
    """The draws of stream positions ``pos0 .. pos0 + n - 1``: int32 [n, 6] = (kind, the bits of the fp32
    ``lam``, x0, x1, y0, y1), kind 0 unmixed / 1 mixup / 2 CutMix, bitwise what the device draws.  An
    unmixed entry (not applied, or an empty box) has ``lam = 1`` and a zero box, a mixup entry a zero box.
    The partner plays no part here: the draw depends on the position alone."""
    pos0, n = _check_window(pos0, n)
    f32 = np.float32
    p = np.uint64(pos0) + np.arange(n, dtype=np.uint64)
    w = philox4x32_10((p & np.uint64(0xFFFFFFFF), p >> np.uint64(32), 0, TAG),
                      (cfg.seed & 0xFFFFFFFF, cfg.seed >> 32))
    w = [np.broadcast_to(v, (n,)).astype(np.uint32) for v in w]
    mixup_on, cutmix_on = cfg.mixup_alpha != 0.0, cfg.cutmix_alpha != 0.0
    apply = ((w[0] >> np.uint32(16)).astype(np.int64) < cfg.thr_p) & (mixup_on or cutmix_on)
    cut = np.full(n, cutmix_on) & (np.full(n, not mixup_on) | ((w[0] & np.uint32(1)) != 0))
    kind = np.where(apply, np.where(cut, CUTMIX, MIXUP), UNMIXED).astype(np.int32)
    lam = np.ones(n, dtype=f32)
    box = np.zeros((n, 4), dtype=np.int32)
    if mixup_on:
        T = _lam_table(cfg.mixup_alpha)
        u = (w[1] >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)
        pos = u * f32(TABLE_N)
        k = pos.astype(np.int32)
        fr = pos - k.astype(f32)
        d = T[k + 1] - T[k]
        t = fr * d
        lm = (T[k] + t).astype(f32)
        lam = np.where(kind == MIXUP, lm, lam)
    if cutmix_on:
        S = side_table(cfg.cutmix_alpha)
        side = S[(w[1] >> np.uint32(22)).astype(np.int64)].astype(np.int64)
        c28 = np.uint64(SIDE)
        cx = ((w[2].astype(np.uint64) * c28) >> np.uint64(32)).astype(np.int64)
        cy = ((w[3].astype(np.uint64) * c28) >> np.uint64(32)).astype(np.int64)
        x0, x1 = np.maximum(cx - side // 2, 0), np.minimum(cx - side // 2 + side, SIDE)
        y0, y1 = np.maximum(cy - side // 2, 0), np.minimum(cy - side // 2 + side, SIDE)
        area = (x1 - x0) * (y1 - y0)
        lc = ((784 - area).astype(f32) / f32(784.0)).astype(f32)
        empty = (kind == CUTMIX) & (area == 0)
        kind = np.where(empty, UNMIXED, kind).astype(np.int32)
        isc = kind == CUTMIX
        lam = np.where(isc, lc, lam)
        box = np.where(isc[:, None], np.stack([x0, x1, y0, y1], axis=1), 0).astype(np.int32)
    out = np.empty((n, 6), dtype=np.int32)
    out[:, 0] = kind
    out[:, 1] = lam.astype(f32).view(np.int32)
    out[:, 2:] = box
    return out


def mixed(images: np.ndarray, labels: np.ndarray, cfg: MixConfig, pos0: int):
    """The mixed batch: ``images`` [nb, 784, C] (any real dtype: the values the buffer holds) and
    ``labels`` [nb] as stream positions ``pos0 ..`` under ``cfg`` -> (images float64 [nb, 784, C],
    labels2 int32 [nb], lam float32 [nb]).  Entry b's partner is entry nb - 1 - b; an entry that is its
    own partner is unmixed.  The mixup blend is evaluated in float64 from the fp32 ``lam``."""
    x = np.asarray(images).astype(np.float64)
    if x.ndim != 3 or x.shape[1] != SIDE * SIDE:
        raise ValueError(f"images must be [nb, {SIDE * SIDE}, C], got {x.shape}")
    nb, _, C = x.shape
    labels = np.asarray(labels).astype(np.int32)
    if labels.shape != (nb,):
        raise ValueError(f"labels must be [{nb}], got {labels.shape}")
    prm = params(cfg, pos0, nb)
    kind = prm[:, 0].copy()
    lam = prm[:, 1].copy().view(np.float32)
    if nb % 2 == 1:
        kind[nb // 2] = UNMIXED
        lam[nb // 2] = np.float32(1.0)
    xb = x[::-1]
    out = x.copy()
    mu = kind == MIXUP
    l64 = lam.astype(np.float64)[:, None, None]
    out[mu] = (l64 * x + (1.0 - l64) * xb)[mu]
    col = np.arange(SIDE)[None, None, :]
    row = np.arange(SIDE)[None, :, None]
    x0, x1, y0, y1 = (prm[:, 2 + i][:, None, None] for i in range(4))
    inside = (kind == CUTMIX)[:, None, None] & (col >= x0) & (col < x1) & (row >= y0) & (row < y1)
    inside = inside.reshape(nb, SIDE * SIDE)
    out[inside] = xb[inside]
    labels2 = np.where(kind == UNMIXED, labels, labels[::-1]).astype(np.int32)
    return out, labels2, lam
