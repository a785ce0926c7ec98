"""Host reference of the training augmentation (``csrc/kernels/augment.hip``), in vectorised numpy.

Each training image gets a random shift of up to ``shift`` whole pixels, a rotation of up to
``rotate`` degrees about the image centre and an isotropic zoom in ``[1 - scale, 1 + scale)``.  The
transformation of a batch entry is a pure function of ``(seed, p)``, ``p`` its global stream
position (the position the Feistel shuffle of ``device_loader`` maps to a dataset row): one
Philox4x32-10 call (``ops.dropout.philox4x32_10``), every floating-point line below a single rounded
fp32 operation

    counter = (p & 0xffffffff, p >> 32, 0, 0x41554700)     key = (seed & 0xffffffff, seed >> 32)
    tx = float(umulhi(w0, 2S+1)) - S       ty = float(umulhi(w1, 2S+1)) - S       integers in [-S, S]
    u(w)  = float(w >> 8) * 2^-24                                                  [0, 1), exact
    theta = (R * (2 u(w2) - 1)) * float32(pi / 180)        s = 1 + Z * (2 u(w3) - 1)

and the inverse map of output pixel (row i, column j), shared by the channels of a pixel:

    c = cos(theta)  sn = sin(theta)  r = 1 / s      u = j - 13.5   v = i - 13.5
    sx = (c*u + sn*v) * r + 13.5 - tx                sy = (c*v - sn*u) * r + 13.5 - ty
    val = bilinear interpolation of the raw uint8 image at (sx, sy), taps outside [0, 27]^2 worth 0
    out = val / 255 - 0.5

Elastic distortion (Simard, Steinkraus and Platt, 2003) adds a smooth random displacement field to
that inverse map.  The field of a batch entry is again a pure function of ``(seed, p)``:

    e       = f * 784 + 28 * i + j          f = 0: x-displacement, f = 1: y-displacement; output pixel (i, j)
    g       = e >> 3                        0..195: eight 16-bit draws per Philox call
    counter = (p & 0xffffffff, p >> 32, g, 0x41554701)     key as above
    draw(e) = (w[(e & 7) >> 1] >> (16 * (e & 1))) & 0xffff                   dropout's unpacking
    r_f[i,j] = (float(draw) - 32767.5) * 2^-15                               exact in fp32, in (-1, 1)
    K = ceil(3 sigma)    w_k = exp(-k^2 / (2 sigma^2)) / sum_{m=-K..K} exp(-m^2 / (2 sigma^2))   (float64 -> fp32)
    d_f[i,j] = sum_{a,b=-K..K} w_|a| w_|b| r_f[i+a, j+b]                     r_f = 0 outside the image
    sx' = sx + alpha d_0[i,j]      sy' = sy + alpha d_1[i,j]

``elastic_weights`` is the one source of the table: the device takes the table, not sigma.

``params`` and ``elastic_draws`` are what the device draws, bit for bit; ``warp`` evaluates the map in
float64 from those fp32 parameters (and the float64 ``elastic_field``).  The CPU loader path uses ``warp`` rounded once to the buffer's dtype, and the
tests' oracle is the same function.  Nothing here needs torch or a GPU.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from ..ops.dropout import check_seed, philox4x32_10

TAG = 0x41554700          # counter word 3; no dropout layer word reaches it with a real layer index
ELASTIC_TAG = 0x41554701  # ... of the elastic field's draws (counter word 2 is the draw group there)
MAX_SHIFT, MAX_ROTATE, MAX_SCALE = 8, 180.0, 0.5
MAX_ELASTIC_ALPHA, MIN_ELASTIC_SIGMA, MAX_ELASTIC_SIGMA = 64.0, 0.5, 8.0
ELASTIC_GROUPS = 196      # Philox calls per image: 2 * 784 draws, eight per call
SIDE = 28
CENTRE = 13.5


def check_shift(v, key: str = "augment_shift") -> int:
    """``v`` as an int: an integer with 0 <= v <= 8 (3 and 3.0 pass; 3.5, True and "x" do not)."""
    try:
        if isinstance(v, bool) or int(v) != float(v):
            raise ValueError
        s = int(v)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{key} must be an integer with 0 <= {key} <= {MAX_SHIFT}, got {v!r}") from None
    if not 0 <= s <= MAX_SHIFT:
        raise ValueError(f"{key} must be an integer with 0 <= {key} <= {MAX_SHIFT}, got {s}")
    return s


def _check_float(v, key: str, hi: float, lo: float = 0.0) -> float:
    try:
        if isinstance(v, bool):
            raise ValueError
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{key} must be a number with {lo:g} <= {key} <= {hi:g}, got {v!r}") from None
    if not lo <= f <= hi:       # NaN fails both comparisons
        raise ValueError(f"{key} must be finite with {lo:g} <= {key} <= {hi:g}, got {f}")
    return f


def check_rotate(v, key: str = "augment_rotate") -> float:
    """``v`` as a float: finite with 0 <= v <= 180 (degrees)."""
    return _check_float(v, key, MAX_ROTATE)


def check_scale(v, key: str = "augment_scale") -> float:
    """``v`` as a float: finite with 0 <= v <= 0.5."""
    return _check_float(v, key, MAX_SCALE)


def check_elastic_alpha(v, key: str = "augment_elastic_alpha") -> float:
    """``v`` as a float: finite with 0 <= v <= 64 (pixels; 0: no elastic distortion)."""
    return _check_float(v, key, MAX_ELASTIC_ALPHA)


def check_elastic_sigma(v, key: str = "augment_elastic_sigma") -> float:
    """``v`` as a float: finite with 0.5 <= v <= 8 (pixels)."""
    return _check_float(v, key, MAX_ELASTIC_SIGMA, MIN_ELASTIC_SIGMA)


@dataclasses.dataclass(frozen=True)
class AugmentConfig:
    """The augmentation keys, checked: a ValueError names key and value."""
    shift: int = 0
    rotate: float = 0.0
    scale: float = 0.0
    seed: int = 0
    elastic_alpha: float = 0.0
    elastic_sigma: float = 4.0

    def __post_init__(self):
        object.__setattr__(self, "shift", check_shift(self.shift))
        object.__setattr__(self, "rotate", check_rotate(self.rotate))
        object.__setattr__(self, "scale", check_scale(self.scale))
        object.__setattr__(self, "seed", check_seed(self.seed, "augment_seed"))
        object.__setattr__(self, "elastic_alpha", check_elastic_alpha(self.elastic_alpha))
        object.__setattr__(self, "elastic_sigma", check_elastic_sigma(self.elastic_sigma))

    @property
    def enabled(self) -> bool:
        return self.shift != 0 or self.rotate != 0.0 or self.scale != 0.0 or self.elastic_alpha != 0.0

    @property
    def elastic(self) -> bool:
        return self.elastic_alpha != 0.0

    def with_seed(self, seed: int) -> "AugmentConfig":
        return dataclasses.replace(self, seed=seed)


def params(cfg: AugmentConfig, pos0: int, n: int) -> np.ndarray:
    """(tx, ty, theta, s) of stream positions ``pos0 .. pos0 + n - 1``: float32 [n, 4], bitwise
    what the device draws."""
    pos0, n = _check_window(pos0, n)
    f32 = np.float32
    p = np.uint64(pos0) + np.arange(n, dtype=np.uint64)
    w = philox4x32_10((p & np.uint64(0xFFFFFFFF), p >> np.uint64(32), 0, TAG),
                      (cfg.seed & 0xFFFFFFFF, cfg.seed >> 32))
    w = [np.broadcast_to(v, (n,)) for v in w]
    S = cfg.shift
    span = np.uint64(2 * S + 1)
    tx = ((w[0].astype(np.uint64) * span) >> np.uint64(32)).astype(f32) - f32(S)
    ty = ((w[1].astype(np.uint64) * span) >> np.uint64(32)).astype(f32) - f32(S)
    u2 = (w[2] >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)
    u3 = (w[3] >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)
    t2 = f32(2) * u2 - f32(1)
    t3 = f32(2) * u3 - f32(1)
    theta = (f32(cfg.rotate) * t2) * f32(math.pi / 180.0)
    s = f32(1) + f32(cfg.scale) * t3
    out = np.stack([tx, ty, theta, s], axis=1)
    assert out.dtype == np.float32
    return out


def _check_window(pos0, n):
    pos0, n = int(pos0), int(n)
    if pos0 < 0 or n < 0 or pos0 + n > 1 << 63:
        raise ValueError(f"pos0 must be >= 0 with pos0 + n <= 2^63, got {pos0} (n = {n})")
    return pos0, n


def elastic_weights(sigma) -> np.ndarray:
    """The half table w_0 .. w_K of the truncated, normalised Gaussian, K = ceil(3 sigma): computed in
    float64, rounded once to float32 [K + 1].  The device is handed this table."""
    sigma = check_elastic_sigma(sigma)
    K = int(math.ceil(3.0 * sigma))
    k = np.arange(K + 1, dtype=np.float64)
    e = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return (e / (e[0] + 2.0 * e[1:].sum())).astype(np.float32)


def elastic_draws(cfg: AugmentConfig, pos0: int, n: int) -> np.ndarray:
    """The 16-bit draws of the displacement fields of stream positions ``pos0 .. pos0 + n - 1``: uint16
    [n, 2, 28, 28] (x-displacement, y-displacement; output pixel row, column), bitwise the device's."""
    pos0, n = _check_window(pos0, n)
    p = (np.uint64(pos0) + np.arange(n, dtype=np.uint64))[:, None]
    g = np.arange(ELASTIC_GROUPS, dtype=np.uint64)[None, :]
    w = philox4x32_10((p & np.uint64(0xFFFFFFFF), p >> np.uint64(32), g, ELASTIC_TAG),
                      (cfg.seed & 0xFFFFFFFF, cfg.seed >> 32))
    w = np.stack(np.broadcast_arrays(*w), axis=-1)                           # [n, 196, 4]
    out = np.stack([w & np.uint32(0xFFFF), w >> np.uint32(16)], axis=-1)     # [n, 196, 4, 2]: low half first
    return out.reshape(n, 2, SIDE, SIDE).astype(np.uint16)


def _smooth(r: np.ndarray, w: np.ndarray, alpha, dtype) -> np.ndarray:
    """alpha * (G r G^T) of the planes ``r`` [..., 28, 28] under the half table ``w``, zero extension, in
    ``dtype``: taps summed in the order a = -K .. K, the horizontal pass first, then the vertical one,
    then the scale -- one rounded operation per step."""
    t = np.dtype(dtype).type
    w = np.asarray(w).astype(t)
    K = len(w) - 1
    x = np.asarray(r).astype(t)
    for axis in (-1, -2):
        pad = [(0, 0)] * x.ndim
        pad[axis] = (K, K)
        xp = np.pad(x, pad)
        acc = np.zeros_like(x)
        for a in range(-K, K + 1):
            sl = [slice(None)] * x.ndim
            sl[axis] = slice(K + a, K + a + SIDE)
            acc = acc + w[abs(a)] * xp[tuple(sl)]
        x = acc
    return (t(alpha) * x).astype(t)


def elastic_field(cfg: AugmentConfig, pos0: int, n: int, dtype=np.float64) -> np.ndarray:
    """The displacement fields (D_0, D_1) in pixels, ``dtype`` [n, 2, 28, 28], indexed by the output
    pixel.  float64 is the reference; float32 is the one-rounding-per-operation transcription."""
    f32 = np.float32
    r = (elastic_draws(cfg, pos0, n).astype(f32) - f32(32767.5)) * f32(2.0 ** -15)     # exact
    return _smooth(r, elastic_weights(cfg.elastic_sigma), f32(cfg.elastic_alpha), dtype)


def source_coords(prm: np.ndarray, dtype=np.float64):
    """(sx, sy) of every output pixel, [n, 28, 28] each, evaluated in ``dtype`` from the fp32
    parameters ``prm`` [n, 4] (in float32: one rounded operation per step, in the order above)."""
    prm = np.asarray(prm)
    t = dtype
    tx, ty, theta, s = (prm[:, k].astype(t)[:, None, None] for k in range(4))
    c, sn = np.cos(theta), np.sin(theta)
    r = t(1) / s
    u = (np.arange(SIDE, dtype=t) - t(CENTRE))[None, None, :]
    v = (np.arange(SIDE, dtype=t) - t(CENTRE))[None, :, None]
    sx = (c * u + sn * v) * r + t(CENTRE) - tx
    sy = (c * v - sn * u) * r + t(CENTRE) - ty
    return sx, sy


def bilinear_zero(img: np.ndarray, sx: np.ndarray, sy: np.ndarray) -> np.ndarray:
    """Bilinear interpolation of ``img`` [n, 28, 28, C] (any real dtype) at (sx, sy) [n, 28, 28], every
    tap outside the image worth 0; computed in the dtype of ``sx``."""
    t = sx.dtype.type
    n = img.shape[0]
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0f)[..., None], (sy - y0f)[..., None]
    # far-away coordinates are all-zero taps whatever their integer value: keep the casts in range
    x0 = np.clip(x0f, -2, SIDE).astype(np.int64)
    y0 = np.clip(y0f, -2, SIDE).astype(np.int64)
    pad = np.zeros((n, SIDE + 4, SIDE + 4, img.shape[3]), dtype=sx.dtype)     # pixel (x, y) at [y + 2, x + 2]
    pad[:, 2:2 + SIDE, 2:2 + SIDE] = img
    b = np.arange(n)[:, None, None]
    v00, v01 = pad[b, y0 + 2, x0 + 2], pad[b, y0 + 2, x0 + 3]
    v10, v11 = pad[b, y0 + 3, x0 + 2], pad[b, y0 + 3, x0 + 3]
    one = t(1)
    return (v00 * (one - fx) + v01 * fx) * (one - fy) + (v10 * (one - fx) + v11 * fx) * fy


def augmented(images_u8: np.ndarray, cfg: AugmentConfig, pos0: int, Csrc: int, Cdst: int, dtype=np.float64) -> np.ndarray:
    """``warp`` of the rows ``images_u8`` as stream positions ``pos0 ..`` under ``cfg``: the affine draw and,
    when ``cfg.elastic_alpha`` is non-zero, the elastic field, both evaluated in ``dtype``."""
    n = np.asarray(images_u8).shape[0]
    field = elastic_field(cfg, pos0, n, dtype) if cfg.elastic else None
    return warp(images_u8, params(cfg, pos0, n), Csrc, Cdst, dtype, field)


def f32_round_to_odd(x: np.ndarray) -> np.ndarray:
    """float64 -> float32 rounded to odd: an inexact value takes the neighbour whose last mantissa bit
    is set, so a following round-to-nearest-even to bf16 is the single rounding of the float64 value."""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    inexact = f.astype(np.float64) != x
    even = (f.view(np.uint32) & np.uint32(1)) == 0
    toward = np.nextafter(f, np.where(x > f, np.float32(np.inf), np.float32(-np.inf)))
    return np.where(inexact & even, toward, f).astype(np.float32)


def warp(images_u8: np.ndarray, prm: np.ndarray, Csrc: int, Cdst: int, dtype=np.float64, field=None) -> np.ndarray:
    """The augmented, normalised images: ``images_u8`` uint8 [n, 784 * Csrc] (row-major pixels, channels
    innermost) under the fp32 parameters ``prm`` [n, 4] -> ``dtype`` [n, 784, Cdst] (``Cdst`` 3 from
    ``Csrc`` 1 replicates the channel).  float64 is the reference; float32 is the one-rounding-per-step
    transcription the error budget is measured with.  ``field`` [n, 2, 28, 28] (``elastic_field``) is
    added to the source coordinates in ``dtype``; None is no elastic distortion."""
    if (Csrc, Cdst) not in ((1, 1), (3, 3), (1, 3)):
        raise ValueError(f"(Csrc, Cdst) must be (1, 1), (3, 3) or (1, 3), got ({Csrc}, {Cdst})")
    images_u8 = np.asarray(images_u8)
    n = images_u8.shape[0]
    if images_u8.dtype != np.uint8 or images_u8.shape != (n, SIDE * SIDE * Csrc):
        raise ValueError(f"images must be uint8 [n, {SIDE * SIDE * Csrc}], got {images_u8.dtype} {images_u8.shape}")
    t = np.dtype(dtype).type
    sx, sy = source_coords(prm, t)
    if field is not None:
        field = np.asarray(field)
        if field.shape != (n, 2, SIDE, SIDE):
            raise ValueError(f"field must be [n, 2, {SIDE}, {SIDE}], got {field.shape}")
        sx, sy = sx + field[:, 0].astype(t), sy + field[:, 1].astype(t)
    val = bilinear_zero(images_u8.reshape(n, SIDE, SIDE, Csrc), sx, sy)
    out = val / t(255) - t(0.5) if t is np.float64 else (val * t(1.0 / 255.0) - t(0.5)).astype(t)
    if Cdst != Csrc:
        out = np.repeat(out, Cdst, axis=3)
    return out.reshape(n, SIDE * SIDE, Cdst)
