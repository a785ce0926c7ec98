"""Float64 numpy oracle of mixup / CutMix and of the two-label softmax cross-entropy, written from the
formulas, for ``test_mix_cpu.py`` and ``test_mix_gpu.py``.  It shares no code with the package: its own
Philox4x32-10, its own tables (``scipy.special.betaincinv``), its own draw and its own blend.
``label_smoothing_oracle.py`` (and through it ``stats_oracle.py``), loaded by path, supplies the
smoothed targets and the project's tolerances.

The draw of stream position p (every floating-point line one fp32 operation):

    counter = (p & 0xffffffff, p >> 32, 0, 0x41554702)     key = (seed & 0xffffffff, seed >> 32)
    apply   = (w0 >> 16) < thr_p          thr_p = clamp(floor(prob * 65536 + 0.5), 0, 65536)
    cut     = cutmix on and (mixup off or (w0 & 1))
    mixup:  u = float(w1 >> 8) * 2^-24    pos = u * 1024    k = int(pos)    fr = pos - k
            d = T[k+1] - T[k]             lam = T[k] + fr * d
    cutmix: side = S[w1 >> 22]            cx = (w2 * 28) >> 32    cy = (w3 * 28) >> 32
            x0 = max(cx - side//2, 0)     x1 = min(cx - side//2 + side, 28)     (same in y)
            area = (x1 - x0) * (y1 - y0)  lam = float32(784 - area) / float32(784)

The image of entry b with partner nb - 1 - b (unmixed: not applied, its own partner, an empty box):

    mixup:   out = lam * xa + (1 - lam) * xb
    cutmix:  out = xb inside [x0, x1) x [y0, y1), xa outside

The loss of a row with labels ya, yb and weight lam (q the smoothed targets of
``label_smoothing_oracle``; a row with lam == 1 has the targets of ya alone):

    Q = lam q(ya) + (1 - lam) q(yb)       loss = -sum_c Q_c log p_c      dl_c = (p_c - Q_c) * scale

Run as a script it prints E32 and the self-check.
"""
import importlib.util
import os

import numpy as np

_here = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("label_smoothing_oracle",
                                               os.path.join(_here, "label_smoothing_oracle.py"))
lso = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lso)
so = lso.so
f64, i64, ce_tol, check_ce, top1_count, check_dbias = so.f64, so.i64, so.ce_tol, so.check_ce, so.top1_count, lso.check_dbias

TAG = 0x41554702
UNMIXED, MIXUP, CUTMIX = 0, 1, 2
SEED = (0xB7 << 32) | 0x089ABCDE                      # a 40-bit seed
ALPHAS = (0.2, 1.0, 4.0)
_M32 = np.uint64(0xFFFFFFFF)
f32 = np.float32


# ------------------------------------------------------------------ the draw
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Random123): uint64 arrays holding 32-bit words in, four such arrays out."""
    c = [np.asarray(v, dtype=np.uint64) & _M32 for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c


def lam_table(alpha):
    from scipy.special import betaincinv
    return betaincinv(float(alpha), float(alpha), 0.5 + np.arange(1025) / 2048.0).astype(f32)


def side_table(alpha):
    return np.floor(28.0 * np.sqrt(1.0 - lam_table(alpha)[:1024].astype(np.float64))).astype(np.int32)


def table_roundtrip(alpha):
    """(lo, hi, q): T[k] is the float32 nearest to Q(q_k), so Q(q_k) lies within half a float32 ulp of
    it -- 2^-25 on [0.5, 1] -- and, the distribution function I being monotone, q_k lies in
    [I(T[k] - 2^-25), I(T[k] + 2^-25)], up to the 1e-12 granted to betainc / betaincinv themselves."""
    from scipy.special import betainc
    t = lam_table(alpha).astype(np.float64)
    h = 2.0 ** -25
    lo = betainc(alpha, alpha, np.clip(t - h, 0.0, 1.0)) - 1e-12
    hi = betainc(alpha, alpha, np.clip(t + h, 0.0, 1.0)) + 1e-12
    return lo, hi, 0.5 + np.arange(1025) / 2048.0


def thr_p(prob):
    return int(min(max(np.floor(prob * 65536.0 + 0.5), 0), 65536))


def draws(mixup_alpha, cutmix_alpha, prob, seed, pos0, n):
    """(kind int [n], lam float32 [n], box int [n, 4] = x0, x1, y0, y1) of positions pos0 .. pos0 + n - 1;
    the partner plays no part."""
    p = np.uint64(pos0) + np.arange(n, dtype=np.uint64)
    w = philox(p & _M32, p >> np.uint64(32), 0, TAG, seed & 0xFFFFFFFF, seed >> 32)
    w = [np.broadcast_to(v, (n,)) for v in w]
    apply = (w[0] >> np.uint64(16)).astype(np.int64) < thr_p(prob)
    kind = np.zeros(n, np.int64)
    lam = np.ones(n, f32)
    box = np.zeros((n, 4), np.int64)
    if cutmix_alpha:
        cut = np.ones(n, bool) if not mixup_alpha else (w[0] & np.uint64(1)) == 1
    else:
        cut = np.zeros(n, bool)
    if mixup_alpha:
        T = lam_table(mixup_alpha)
        u = (w[1] >> np.uint64(8)).astype(f32) * f32(2.0 ** -24)
        pos = (u * f32(1024.0)).astype(f32)
        k = pos.astype(np.int64)
        fr = (pos - k.astype(f32)).astype(f32)
        d = (T[k + 1] - T[k]).astype(f32)
        lm = (T[k] + (fr * d).astype(f32)).astype(f32)
        sel = apply & ~cut
        kind[sel], lam[sel] = MIXUP, lm[sel]
    if cutmix_alpha:
        S = side_table(cutmix_alpha)
        side = S[(w[1] >> np.uint64(22)).astype(np.int64)].astype(np.int64)
        cx = ((w[2] * np.uint64(28)) >> np.uint64(32)).astype(np.int64)
        cy = ((w[3] * np.uint64(28)) >> np.uint64(32)).astype(np.int64)
        x0, x1 = np.maximum(cx - side // 2, 0), np.minimum(cx - side // 2 + side, 28)
        y0, y1 = np.maximum(cy - side // 2, 0), np.minimum(cy - side // 2 + side, 28)
        area = (x1 - x0) * (y1 - y0)
        sel = apply & cut & (area > 0)
        kind[sel] = CUTMIX
        lam[sel] = ((784 - area).astype(f32) / f32(784.0)).astype(f32)[sel]
        box[sel] = np.stack([x0, x1, y0, y1], 1)[sel]
    return kind, lam, box


def params(mixup_alpha, cutmix_alpha, prob, seed, pos0, n):
    """The draws in the layout of the ``mix_params`` probe: int32 [n, 6]."""
    kind, lam, box = draws(mixup_alpha, cutmix_alpha, prob, seed, pos0, n)
    out = np.empty((n, 6), np.int32)
    out[:, 0], out[:, 1], out[:, 2:] = kind, lam.view(np.int32), box
    return out


# ------------------------------------------------------------------ the batch
def batch_draws(mixup_alpha, cutmix_alpha, prob, seed, pos0, nb):
    """The draws of a local batch: the middle entry of an odd batch is its own partner, so unmixed."""
    kind, lam, box = draws(mixup_alpha, cutmix_alpha, prob, seed, pos0, nb)
    if nb % 2:
        kind[nb // 2], lam[nb // 2], box[nb // 2] = UNMIXED, 1.0, 0
    return kind, lam, box


def mixed(x, labels, kind, lam, box, dtype=np.float64, bug=None):
    """x [nb, 784, C] -> (images in ``dtype``, labels2, lam) under the batch draws.  float64 is the
    reference; float32 is the one-rounding-per-operation transcription E32 is measured with.  ``bug``:
    "partner" mixes with entry b + 1 instead of the flip, "swap" exchanges lam and 1 - lam."""
    t = np.dtype(dtype).type
    x = np.asarray(x).astype(t)
    nb, _, C = x.shape
    xb = np.roll(x, -1, axis=0) if bug == "partner" else x[::-1]
    out = x.copy()
    l = lam.astype(t)[:, None, None]
    om = (t(1) - l).astype(t)
    if bug == "swap":
        l, om = om, l
    blend = ((l * x).astype(t) + (om * xb).astype(t)).astype(t)
    mu = kind == MIXUP
    out[mu] = blend[mu]
    col, row = np.arange(784) % 28, np.arange(784) // 28
    inside = ((kind == CUTMIX)[:, None] & (col[None] >= box[:, 0:1]) & (col[None] < box[:, 1:2])
              & (row[None] >= box[:, 2:3]) & (row[None] < box[:, 3:4]))
    out[inside] = xb[inside]
    labels = np.asarray(labels).astype(np.int32)
    labels2 = np.where(kind == UNMIXED, labels, labels[::-1]).astype(np.int32)
    return out, labels2, lam


def bf16_values(rng, shape):
    """Random bf16-representable values in [-0.5, 0.5] as float32 (what the loader's buffer holds), full
    8-bit mantissas: the float32 bits with the low 16 cleared."""
    v = (rng.random(shape, dtype=np.float32) - f32(0.5))
    return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_ulp(x):
    """The bf16 ulp at |x| (8 significant bits), float64; the smallest normal's below it."""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


IMAGE_NBS, IMAGE_CS, IMAGE_POS0 = (1, 2, 7, 77), (1, 3), (1 << 32) - 3
IMAGE_CFGS = ((1.0, 0.0, 1.0), (0.0, 1.0, 1.0), (0.2, 4.0, 0.75))      # (mixup_alpha, cutmix_alpha, prob)


def image_inputs(nb, C):
    rng = np.random.default_rng(1000 * C + nb)
    return bf16_values(rng, (nb, 784, C)), rng.integers(0, 10, nb).astype(np.int32)


def e32():
    """The worst |float32 transcription - float64| of the mixup blend over the image tests' inputs."""
    worst = 0.0
    for nb in IMAGE_NBS:
        for C in IMAGE_CS:
            x, y = image_inputs(nb, C)
            for ma, ca, pr in IMAGE_CFGS:
                d = batch_draws(ma, ca, pr, SEED, IMAGE_POS0, nb)
                a, _, _ = mixed(x, y, *d, dtype=np.float64)
                b, _, _ = mixed(x, y, *d, dtype=np.float32)
                worst = max(worst, float(np.abs(a - b.astype(np.float64)).max()))
    return worst


def image_bound(ref, E32):
    """Half a bf16 ulp of the float64 reference plus 4 * E32, per element."""
    return 0.5 * bf16_ulp(ref) + 4.0 * E32


def self_check(E32=None, verbose=True):
    """The two wrong kernels of the issue exceed the mixup bound by orders of magnitude."""
    E32 = e32() if E32 is None else E32
    out = {}
    x, y = image_inputs(77, 1)
    d = batch_draws(1.0, 0.0, 1.0, SEED, IMAGE_POS0, 77)
    ref, _, _ = mixed(x, y, *d)
    for bug in ("partner", "swap"):
        got, _, _ = mixed(x, y, *d, bug=bug)
        ratio = float((np.abs(got - ref) / image_bound(ref, E32)).max())
        out[bug] = ratio
        if verbose:
            print(f"wrong kernel {bug!r}: worst error / bound = {ratio:.3e}")
    return out


# ------------------------------------------------------------------ the loss
def targets(ya, yb, lam, nc, eps):
    lam = f64(lam)[:, None]
    qa, qb = lso.targets(ya, nc, eps), lso.targets(yb, nc, eps)
    return np.where(lam < 1.0, lam * qa + (1.0 - lam) * qb, qa)


def ce_rows(logits, ya, yb, lam, eps):
    lsm = so.log_softmax(logits)
    q = targets(ya, yb, lam, lsm.shape[1], eps)
    with np.errstate(invalid="ignore"):
        t = np.where(q != 0.0, q * lsm, 0.0)        # a class with target 0 is not read: 0 * -inf is not the loss
    return -t.sum(axis=1)


def ce_sum(logits, ya, yb, lam, eps):
    return float(ce_rows(logits, ya, yb, lam, eps).sum())


def dlogits(logits, ya, yb, lam, scale, eps):
    z = f64(logits)
    return (so.softmax(z) - targets(ya, yb, lam, z.shape[1], eps)) * scale


def check_dlogits(dl, logits, ya, yb, lam, scale, eps, what=""):
    """bf16 kernels: 2**-8 of the largest gradient (``stats_oracle.check_dlogits``)."""
    g = dlogits(logits, ya, yb, lam, scale, eps)
    err = np.abs(f64(dl) - g).max()
    print(f"{what}: dlogits err {err:.3e}, max |g| {np.abs(g).max():.3e}")
    assert err <= 2.0 ** -8 * np.abs(g).max(), f"{what}: dlogits err {err:.3e} vs max |g| {np.abs(g).max():.3e}"
    return g


def lam_vector(rng, n):
    """Weights with 1.0, 0.5 and values in between, as float32."""
    lam = (0.5 + 0.5 * rng.random(n)).astype(f32)
    lam[::4] = 1.0
    lam[1::8] = 0.5
    return lam


if __name__ == "__main__":
    E = e32()
    print(f"E32 = {E:.3e}")
    self_check(E)
