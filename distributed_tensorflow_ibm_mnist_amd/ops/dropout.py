"""Host reference of the dropout masks (``csrc/kernels/dropout_rng.h``), in vectorised numpy.

The keep bit of a unit is a pure function of ``(seed, step, layer, batch row, feature)``: one
Philox4x32-10 call (Random123 constants) gives the eight 16-bit draws of features ``8g .. 8g + 7``

    counter = (t & 0xffffffff, t >> 32, m, (L << 16) | (f >> 3))
    key     = (seed & 0xffffffff, seed >> 32)
    draw(f) = (w[(f & 7) >> 1] >> (16 * (f & 1))) & 0xffff
    keep(f) = draw(f) < thr,   thr = clamp(floor((1 - p) * 65536 + 0.5), 1, 65535)

and a kept unit is scaled by ``inv_keep = float32(65536 / thr)``, the exact reciprocal of the
effective keep probability ``thr / 65536`` (which differs from ``1 - p`` by at most 2^-17 = 7.6e-6,
plus the clamp at the two ends).  The device kernels, ``TorchNet``, the oracle and the tests all use
these functions; nothing here needs torch or a GPU.
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
MAX_LAYER, MAX_N, MAX_ROWS, MAX_SEED = 1 << 16, 524288, 1 << 31, 1 << 63

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def check_rate(p, key: str = "dropout") -> float:
    """``p`` as a float: finite with 0 <= p < 1, else a ValueError naming key and value."""
    try:
        if isinstance(p, bool):
            raise ValueError
        v = float(p)
    except (TypeError, ValueError):
        raise ValueError(f"{key} must be a number with 0 <= {key} < 1, got {p!r}") from None
    if not 0 <= v < 1:        # NaN fails both comparisons
        raise ValueError(f"{key} must be finite with 0 <= {key} < 1, got {v}")
    return v


def check_seed(seed, key: str = "dropout_seed") -> int:
    """``seed`` as an int: an integer with 0 <= seed < 2^63."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"{key} must be an integer with 0 <= {key} < 2^63, got {seed!r}")
    s = int(seed)
    if not 0 <= s < MAX_SEED:
        raise ValueError(f"{key} must be an integer with 0 <= {key} < 2^63, got {s}")
    return s


def threshold(p) -> Tuple[int, float]:
    """(thr, inv_keep) of drop rate ``p``: keep when the 16-bit draw is below thr."""
    p = check_rate(p)
    thr = min(max(int(math.floor((1.0 - p) * 65536.0 + 0.5)), 1), 65535)
    return thr, float(np.float32(65536.0 / thr))


def philox4x32_10(counter, key):
    """Philox4x32-10 on arrays: ``counter`` 4 and ``key`` 2 uint32 words (broadcastable arrays);
    returns the 4 output words as a tuple of uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _M32 for v in counter]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & _M32 for v in key)
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    for r in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _M32, (p0 >> _S32) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + np.uint64(PHILOX_W0)) & _M32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _M32
    return tuple(v.astype(np.uint32) for v in c)


def draws(seed: int, step: int, layer: int, rows: int, n: int) -> np.ndarray:
    """The 16-bit draws of rows ``0 .. rows - 1``, features ``0 .. n - 1``: uint16 [rows, n]."""
    seed = check_seed(seed, "seed")
    step, layer, rows, n = int(step), int(layer), int(rows), int(n)
    if not 0 <= step < MAX_SEED:
        raise ValueError(f"step must be in [0, 2^63), got {step}")
    if not 0 <= layer < MAX_LAYER:
        raise ValueError(f"layer must be in [0, 65536), got {layer}")
    if not 0 <= n <= MAX_N:
        raise ValueError(f"n must be in [0, 524288], got {n}")
    if not 0 <= rows < MAX_ROWS:
        raise ValueError(f"rows must be in [0, 2^31), got {rows}")
    groups = (n + 7) // 8
    m = np.arange(rows, dtype=np.uint64)[:, None]
    g = np.arange(groups, dtype=np.uint64)[None, :]
    w = philox4x32_10((step & 0xFFFFFFFF, step >> 32, m, (np.uint64(layer) << np.uint64(16)) | g),
                      (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(np.broadcast_arrays(*w), axis=-1)                      # [rows, groups, 4]
    out = np.stack([w & np.uint32(0xFFFF), w >> np.uint32(16)], axis=-1)   # [rows, groups, 4, 2]
    return out.reshape(rows, groups * 8)[:, :n].astype(np.uint16)


def keep_mask(seed: int, step: int, layer: int, rows: int, n: int, p) -> np.ndarray:
    """The keep bits the device applies at ``(seed, step, layer)``: bool [rows, n]."""
    thr, _ = threshold(p)
    return draws(seed, step, layer, rows, n) < np.uint16(thr)


def multiplier(seed: int, step: int, layer: int, rows: int, n: int, p) -> np.ndarray:
    """``inv_keep`` where kept, 0 where dropped: float32 [rows, n] (the oracle's multiplier)."""
    _, inv = threshold(p)
    return np.where(keep_mask(seed, step, layer, rows, n, p), np.float32(inv), np.float32(0.0)).astype(np.float32)


def dropout_layers(spec) -> dict:
    """{layer name: index in ``spec.layers``} of the layers dropout applies to: every ``Dense``
    with ``relu=True`` that is not the last layer."""
    from ..models.spec import Dense
    last = len(spec.layers) - 1
    return {L.name: i for i, L in enumerate(spec.layers) if isinstance(L, Dense) and L.relu and i != last}
