"""Exact-arithmetic oracle for the linear and pooling kernels.

Inputs whose values are small integers times a power of two make every bf16 x bf16
product and every fp32 partial sum exact, whatever the accumulation order, split-K
layout or tile shape.  A kernel's fp32 outputs then equal a float64 reference bit for
bit, its bf16 outputs are the same single round-to-nearest-even, and its argmax codes
are decided.  One wrong, missing or doubled term changes the exact sum.

The condition (checked here, from the reference alone): with all values of a sum on
the grid 2**-unit, sum(|terms|) * 2**unit < 2**22.  The sum of magnitudes bounds every
partial sum of every ordering; fp32 holds integers below 2**24 exactly, and the
convpool / band kernels borrow the two low mantissa bits for the window position.

Layouts are the kernels': activations NHWC, conv weights HWIO, dense weights [Din, Dout].
Every function takes CPU or GPU tensors of any float dtype and computes in float64.
Pool-window positions are d = 2 * row + col; code 4 marks a window whose ReLU output is 0.
"""
import torch
import torch.nn.functional as F

LIMIT = 2 ** 22


# ------------------------------------------------------------------ rounding / checks
def to_bf16(t):
    """float64 -> float32 -> bfloat16: the first step is exact under the magnitude
    condition, the second is the kernels' one round-to-nearest-even (f2bf / pack2)."""
    return t.to(torch.float32).to(torch.bfloat16)


def to_f32(t):
    r = t.to(torch.float32)
    assert torch.equal(r.double(), t.double()), "not exact in fp32"
    return r


def assert_exact(bound, unit, what="value"):
    """`bound`: the sum of the magnitudes of the terms of every output (the reference of
    the same op on |inputs|); every value involved is a multiple of 2**-unit."""
    s = bound.double() * 2.0 ** unit
    assert torch.equal(s, s.round()), f"{what}: not on the 2**-{unit} grid"
    top = s.abs().max().item() if s.numel() else 0.0
    assert top < LIMIT, f"{what}: sum of magnitudes {top:.0f} * 2**-{unit} reaches 2**22; shrink the inputs"


# ------------------------------------------------------------------ input generators
def dyadic(shape, lo, hi, shift, gen, device, density=1.0, dtype=torch.bfloat16):
    """Integers in [lo, hi] (a fraction `density` of them kept, the rest 0) times 2**-shift."""
    assert max(abs(lo), abs(hi)) <= 256, "more than 8 significant bits: not bf16-representable"
    v = torch.randint(lo, hi + 1, tuple(shape), generator=gen, device=device).double()
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=gen, device=device) < density)
    v = v * 2.0 ** -shift
    out = v.to(dtype)
    assert torch.equal(out.double(), v)
    return out


def density_for(k, amp=4, sigma=64.0):
    """Density for both operands of a K-term sum of products of integers in [-amp, amp]
    that keeps the sum's standard deviation near `sigma` (< 2**8: most outputs are then
    exact in bf16, so a single changed term is visible after the rounding too)."""
    var = (amp * (amp + 1) / 3.0) ** 2        # variance of the product of two uniform integers
    return min(1.0, (sigma * sigma / (k * var)) ** 0.5)


def mnist_like(B, gen, device, strokes=0.15, dtype=torch.bfloat16):
    """[B, 28, 28, 1]: constant -0.5 background (as normalised MNIST), 4-pixel-wide blocks
    of stroke values from {-0.5, 0, 0.5}.  Most pool windows see four identical patches."""
    coarse = torch.rand((B, 7, 7), generator=gen, device=device) < strokes
    val = torch.randint(0, 3, (B, 7, 7), generator=gen, device=device).double() * 0.5 - 0.5
    img = torch.where(coarse, val, torch.full_like(val, -0.5))
    img = img.repeat_interleave(4, 1).repeat_interleave(4, 2)
    # single-pixel strokes on top, so that some windows have a unique winner
    dots = torch.rand((B, 28, 28), generator=gen, device=device) < 0.03
    dv = torch.randint(0, 3, (B, 28, 28), generator=gen, device=device).double() * 0.5 - 0.5
    img = torch.where(dots, dv, img)
    return img.view(B, 28, 28, 1).to(dtype)


# ------------------------------------------------------------------ dense
def _chk(fn, args, unit, what, extra=None):
    if unit is None:
        return
    b = fn(*[a.double().abs() for a in args])
    if extra is not None:
        b = b + extra.double().abs()
    assert_exact(b, unit, what)


def _bias_row(b, n, like):
    row = torch.zeros(n, dtype=torch.float64, device=like.device)
    if b is not None:
        row[: b.numel()] = b.double()
    return row


def dense_fwd(x, w, b=None, relu=False, unit=None):
    """[M, K] @ [K, N] + b (b may be shorter than N: padded bias columns add 0)."""
    row = _bias_row(b, w.shape[1], x)
    _chk(torch.matmul, (x, w), unit, "dense_fwd", row)
    y = x.double() @ w.double() + row
    return y.relu() if relu else y


def dense_dgrad(dy, w, mask=None, unit=None):
    """dX = dY @ W^T, zero where mask <= 0."""
    f = lambda a, b: a @ b.t()
    _chk(f, (dy, w), unit, "dense_dgrad")
    dx = f(dy.double(), w.double())
    return dx if mask is None else torch.where(mask.double() > 0, dx, torch.zeros_like(dx))


def dense_wgrad(x, dy, unit=None, bias_unit=None):
    """(X^T dY [Din, Dout], column sums of dY [Dout]): the bias row (dY's own grid, bias_unit)."""
    f = lambda a, b: a.t() @ b
    _chk(f, (x, dy), unit, "dense_wgrad")
    if bias_unit is not None:
        assert_exact(dy.double().abs().sum(0), bias_unit, "dense_wgrad bias row")
    return f(x.double(), dy.double()), dy.double().sum(0)


# ------------------------------------------------------------------ convolution (stride 1)
def _pads(k, padding):
    return ((k - 1) // 2, k // 2) if padding == "SAME" else (0, 0)


def _xpad(x, kh, kw, padding):
    (t, b), (l, r) = _pads(kh, padding), _pads(kw, padding)
    return F.pad(x, (0, 0, l, r, t, b))


def _conv(x, w, padding):
    kh, kw, ci, co = w.shape
    xp = _xpad(x, kh, kw, padding)
    OH, OW = xp.shape[1] - kh + 1, xp.shape[2] - kw + 1
    y = torch.zeros(x.shape[0], OH, OW, co, dtype=torch.float64, device=x.device)
    for i in range(kh):
        for j in range(kw):
            y += xp[:, i:i + OH, j:j + OW, :] @ w[i, j]
    return y


def _conv_dgrad(dy, w, in_hw, padding):
    kh, kw, ci, co = w.shape
    H, W = in_hw
    (t, b), (l, r) = _pads(kh, padding), _pads(kw, padding)
    N, OH, OW, _ = dy.shape
    assert (OH, OW) == (H + t + b - kh + 1, W + l + r - kw + 1)
    dxp = torch.zeros(N, H + t + b, W + l + r, ci, dtype=torch.float64, device=dy.device)
    for i in range(kh):
        for j in range(kw):
            dxp[:, i:i + OH, j:j + OW, :] += dy @ w[i, j].t()
    return dxp[:, t:t + H, l:l + W, :]


def _conv_wgrad(x, dy, kh, kw, padding):
    xp = _xpad(x, kh, kw, padding)
    N, OH, OW, co = dy.shape
    ci = x.shape[3]
    dw = torch.zeros(kh, kw, ci, co, dtype=torch.float64, device=x.device)
    g = dy.reshape(-1, co)
    for i in range(kh):
        for j in range(kw):
            dw[i, j] = xp[:, i:i + OH, j:j + OW, :].reshape(-1, ci).t() @ g
    return dw


def conv_fwd(x, w, b=None, padding="SAME", relu=False, unit=None):
    row = _bias_row(b, w.shape[3], x)
    _chk(lambda a, c: _conv(a, c, padding), (x, w), unit, "conv_fwd", row)
    y = _conv(x.double(), w.double(), padding) + row
    return y.relu() if relu else y


def conv_dgrad(dy, w, in_hw, padding="SAME", mask=None, unit=None):
    _chk(lambda a, c: _conv_dgrad(a, c, in_hw, padding), (dy, w), unit, "conv_dgrad")
    dx = _conv_dgrad(dy.double(), w.double(), in_hw, padding)
    return dx if mask is None else torch.where(mask.double() > 0, dx, torch.zeros_like(dx))


def conv_wgrad(x, dy, kh, kw, padding="SAME", unit=None, bias_unit=None):
    """(dW [kh, kw, Cin, Cout], db [Cout]); bias_unit: the grid of dY, which the bias row sums."""
    _chk(lambda a, c: _conv_wgrad(a, c, kh, kw, padding), (x, dy), unit, "conv_wgrad")
    if bias_unit is not None:
        assert_exact(dy.double().abs().sum((0, 1, 2)), bias_unit, "conv_wgrad bias row")
    return _conv_wgrad(x.double(), dy.double(), kh, kw, padding), dy.double().sum((0, 1, 2))


# ------------------------------------------------------------------ 2x2 / 2 max-pool
TIES = ("first", "mantissa")


def _windows(y):
    """[N, 2h, 2w, C] -> [N, h, w, C, 4], last axis the window position d = 2 * row + col."""
    return torch.stack([y[:, a::2, b::2, :] for a in (0, 1) for b in (0, 1)], dim=-1)


def pool_select(v, tie):
    """v [..., 4] -> (max, winning position) under a tie rule:
    "first":    the lowest position among equal maxima (a strict `>` scan in position order);
    "mantissa": the position rides in the two low mantissa bits of the fp32 value and a bare
                fp32 max picks the winner: among equal sums >= +0 the HIGHEST position has the
                largest bit pattern, among equal negative sums the LOWEST."""
    assert tie in TIES, tie
    m = v.max(dim=-1, keepdim=True).values
    tied = v == m
    d = torch.arange(4, device=v.device).expand_as(v)
    first = torch.where(tied, d, torch.full_like(d, 4)).min(dim=-1).values
    last = torch.where(tied, d, torch.full_like(d, -1)).max(dim=-1).values
    m = m.squeeze(-1)
    if tie == "first":
        return m, first
    return m, torch.where(m >= 0, last, first)


def maxpool2x2(x, tie="first"):
    """Ceil mode (a trailing odd row / column pools alone).  -> (y float64, positions uint8)."""
    N, H, W, C = x.shape
    xp = F.pad(x.double(), (0, 0, 0, W % 2, 0, H % 2), value=float("-inf"))
    m, d = pool_select(_windows(xp), tie)
    return m, d.to(torch.uint8)


def unpool(dP, codes, out_hw=None):
    """[N, h, w, C] pooled gradient + codes (0..3, anything else: nowhere) -> [N, H, W, C]."""
    N, h, w, C = dP.shape
    H, W = out_hw if out_hw is not None else (2 * h, 2 * w)
    out = torch.zeros(N, 2 * h, 2 * w, C, dtype=torch.float64, device=dP.device)
    g = dP.double()
    for d in range(4):
        out[:, d >> 1::2, d & 1::2, :] = torch.where(codes == d, g, torch.zeros_like(g))
    return out[:, :H, :W, :]


def convpool_fwd(x, w, b, padding, tie, unit=None):
    """conv + bias + ReLU + 2x2 pool as the fused kernels order it: pool the raw sums, add
    the bias to the winner, ReLU.  -> (pooled float64 before the bf16 rounding,
    codes uint8: the winner's position, 4 where the output is 0)."""
    row = _bias_row(b, w.shape[3], x)
    _chk(lambda a, c: _conv(a, c, padding), (x, w), unit, "convpool_fwd", row)
    y = _conv(x.double(), w.double(), padding)
    ph, pw = y.shape[1] // 2, y.shape[2] // 2
    m, d = pool_select(_windows(y[:, :2 * ph, :2 * pw, :]), tie)
    o = (m + row).relu()
    codes = torch.where(o > 0, d, torch.full_like(d, 4)).to(torch.uint8)
    return o, codes


def tie_conv_params(cin_pad, cin, cout_pad, cout, live, gen, device, wdtype=torch.bfloat16):
    """5 x 5 weights (integers in [-3, 3] * 2**-2) and biases (multiples of 2**-3) for the tie
    tests.  On a constant-sign input every window of a same-sign channel ties with a sum of
    known sign; the biases make some of those live after ReLU and some not.  Channel c % 6:
    0: w > 0, bias +live      1: w > 0, bias 0        2: w < 0, bias +1/8
    3: w < 0, bias +live      4: w > 0, small bias    5: w < 0, bias -live
    (No channel mixes signs: mixed weights cancel to exactly zero sums on such inputs all the
    time, and a zero sum is the one case the tie tests keep out; test_exact_kernels_gpu.py
    covers mixed signs.)"""
    mag = torch.randint(1, 4, (5, 5, cin_pad, cout_pad), generator=gen, device=device).double()
    small = torch.randint(-8, 9, (cout_pad,), generator=gen, device=device).double() / 8
    c = torch.arange(cout_pad, device=device) % 6
    sign = torch.where((c == 0) | (c == 1) | (c == 4), 1.0, -1.0).double()
    w = mag * sign * 0.25
    zero = torch.zeros((), dtype=torch.float64, device=device)
    b = torch.where((c == 0) | (c == 3), zero + live, torch.where(c == 5, zero - live, torch.where(
        c == 2, zero + 0.125, torch.where(c == 4, small, zero))))
    w[:, :, cin:, :] = 0
    w[..., cout:] = 0
    return w.to(wdtype), b[:cout].to(torch.float32).contiguous()


def zero_tie_free(x, w, padding, cout_real=None):
    """Per image: no pool window of conv(x, w) has its maximum raw sum tied at exactly 0."""
    co = w.shape[3] if cout_real is None else cout_real
    y = _conv(x.double(), w.double(), padding)[..., :co]
    ph, pw = y.shape[1] // 2, y.shape[2] // 2
    win = _windows(y[:, :2 * ph, :2 * pw, :])
    m = win.max(dim=-1).values
    bad = ((win == m.unsqueeze(-1)).sum(-1) > 1) & (m == 0)
    return ~bad.flatten(1).any(1)


def tie_census(x, w, b, padding, cout_real=None):
    """What the tied pool windows of conv(x, w) look like, from the reference alone:
    counts of windows whose maximum raw sum is attained more than once, split into
    positive sums, negative sums that bias + ReLU leaves positive, negative sums that end
    at 0, and -- what the tie tests must not contain -- exactly zero sums."""
    co = w.shape[3] if cout_real is None else cout_real
    y = _conv(x.double(), w.double(), padding)[..., :co]
    ph, pw = y.shape[1] // 2, y.shape[2] // 2
    win = _windows(y[:, :2 * ph, :2 * pw, :])
    m = win.max(dim=-1).values
    tied = (win == m.unsqueeze(-1)).sum(-1) > 1
    o = m + _bias_row(b, co, x)
    return {"windows": m.numel(), "tied": int(tied.sum()),
            "tied_positive": int((tied & (m > 0)).sum()),
            "tied_negative_live": int((tied & (m < 0) & (o > 0)).sum()),
            "tied_negative_dead": int((tied & (m < 0) & (o <= 0)).sum()),
            "tied_zero": int((tied & (m == 0)).sum())}


# ------------------------------------------------------------------ LeNet-5 conv stack
def lenet_inputs(B, seed, device, extra_shift=0):
    """Dyadic x, w1 (6 of 8 channels), b1, w2 (6 of 8 input channels), b2, dP2 for the LeNet-5
    conv stack, and the units of its sums: (forward units, backward units) for lenet_fwd /
    lenet_bwd.  extra_shift scales the images by 2**-extra_shift."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = dyadic((B, 28, 28, 1), -8, 8, 4 + extra_shift, g, device, density=0.5)
    w1 = dyadic((5, 5, 1, 8), -3, 3, 2, g, device)
    w1[..., 6:] = 0
    b1 = dyadic((6,), -32, 32, 6 + extra_shift, g, device, dtype=torch.float32)
    w2 = dyadic((5, 5, 8, 16), -3, 3, 2, g, device, density=0.5)
    w2[:, :, 6:, :] = 0
    b2 = dyadic((16,), -64, 64, 8 + extra_shift, g, device, dtype=torch.float32)
    dP2 = dyadic((B, 400), -4, 4, 3, g, device, density=0.5)
    e = extra_shift
    # x 2**-(4+e) * w1 2**-2; pool1 (2**-(6+e) grid) * w2 2**-2 | pool1 * dP2 2**-3;
    # dP2 * w2: 2**-5; x * bf16(dP1)
    return (x, w1, b1, w2, b2, dP2), (6 + e, 8 + e), (9 + e, 5, 9 + e)


def lenet_fwd(x, w1, b1, w2, b2, tie="mantissa", units=None):
    """x [B, 28, 28, 1]; w1 [5, 5, 1, 8] (6 real), b1 [6]; w2 [5, 5, 8, 16], b2 [16].
    pool1 is rounded to bf16 before conv2 reads it (lenet_band.hip stages it in LDS as
    bf16).  units = (unit of conv1's sums, unit of conv2's sums).
    -> P1 bf16 [B, 14, 14, 8], C1 uint8, P2 bf16 [B, 5, 5, 16], C2 uint8."""
    u1, u2 = units if units is not None else (None, None)
    o1, c1 = convpool_fwd(x, w1, b1, "SAME", tie, u1)
    P1 = to_bf16(o1)
    o2, c2 = convpool_fwd(P1, w2, b2, "VALID", tie, u2)
    return P1, c1, to_bf16(o2), c2


def lenet_bwd(x, P1, c1, c2, dP2, w2, units=None):
    """dY2 = unpool(dP2) -> dW2, db2, dP1 (conv2 VALID); dY1 = unpool(bf16(dP1)) -> dW1 (conv1
    SAME); db1 sums the fp32 dP1 (lenet_bwd.hip's bias path does not see the bf16 staging).
    units = (unit of dW2's sums, of dP1's, of dW1's).
    -> dW1 [5, 5, 6], db1 [6], dW2 [5, 5, 6, 16], db2 [16] (float64)."""
    uw2, up1, uw1 = units if units is not None else (None, None, None)
    B = x.shape[0]
    dY2 = unpool(dP2.view(B, 5, 5, 16), c2.view(B, 5, 5, 16))
    dW2, db2 = conv_wgrad(P1, dY2, 5, 5, "VALID", uw2, None if uw2 is None else 3)   # dP2: 2**-3
    dP1 = conv_dgrad(dY2, w2, (14, 14), "VALID", None, up1)
    dY1 = unpool(to_bf16(dP1).double(), c1)
    dW1, _ = conv_wgrad(x, dY1, 5, 5, "SAME", uw1)
    g1 = unpool(dP1, c1)
    if up1 is not None:
        assert_exact(g1.abs().sum((0, 1, 2)), up1, "lenet_bwd db1")
    return dW1[:, :, 0, :6], g1.sum((0, 1, 2))[:6], dW2[:, :, :6, :], db2


def unpack_codes(arg):
    """LeNet conv1's packed codes: byte k = code(c = k) | code(c = k + 4) << 4."""
    return torch.cat([arg & 15, arg >> 4], dim=-1)


def pack_codes(codes):
    return (codes[..., :4] | (codes[..., 4:] << 4)).to(torch.uint8)
