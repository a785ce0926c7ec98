"""Per-element float64 oracle and error budget for the LRN kernel family.

LRN is not exact by nature (a power of a sum), so its oracle is a float64 reference
plus a budget per element: the output may differ from the reference by half a bf16 ulp
(bf16 kernels only) plus c * 2**-23 * A, where A is the scale of the terms that make up
that element (below).  An element far below the tensor's maximum is held as tightly as
the maximum itself, and an element that must be zero is held to zero.

    s[c]  = sum_{|c'-c| <= r} x[c']^2,   sc[c] = bias + alpha s[c]
    y[c]  = x[c] sc[c]^-beta                                              A = |y|
    dx[c] = g[c] sc[c]^-beta - 2 alpha beta x[c] sum_{|c'-c| <= r} g[c'] x[c'] sc[c']^-(beta+1)
            A = |g| sc^-beta + 2 alpha beta |x| sum |g x sc^-(beta+1)|    (0 where masked)

Channels are the last dimension of every tensor; everything before it is pixels.  The
functions take CPU or GPU tensors and compute on the tensor's device; nothing here
imports the extension.

The constants c come from float32 transcriptions of the same formulas (every operation
rounded on its own, the power as exp2(p * log2 sc) like the kernels'): `lrn_f32(...,
running=False)` sums each window directly, `running=True` keeps the running sum
restarted every 8 channels that lrn_math.h's window_sums_e documents.  Each c is 4 to 8
times the transcription's worst error over the very inputs the GPU tests use
(tests/test_lrn_oracle_cpu.py measures it and holds c to that range); the margin covers
the 1-ulp hardware log / exp2 / rsq / sqrt.
"""
import math

import torch

U23 = 2.0 ** -23
# measured by tests/test_lrn_oracle_cpu.py (see its header): at least 4x the worst of the
# transcription, rounded up to sit well inside the 4x .. 8x the CPU test allows (float32 log2 /
# exp2 differ by an ulp between CPU math libraries)
C_F32 = 20.0       # direct window sums, over the fp32 kernels' inputs:  worst 3.32
C_BF16 = 640.0     # running window sums, over the bf16 kernels' inputs: worst 118.4
# running window sums in the LRN-backward folds (refc1_wgrad.hip, convpool.hip) over the
# probe sweeps of tests/refc1_oracle.py (dense signed gradients, no ReLU mask: C_BF16 is
# more than 8x their worst), measured by tests/test_refc1_oracle_cpu.py:         worst 15.40
C_FOLD = 100.0
# the condition on the bf16 inputs: the fp32 part of the budget stays below an eighth of the
# smallest bf16 half-ulp (2**-9 relative), so the bf16 rounding is what the budget is about
C_BF16_CAP = 2.0 ** -12 / U23

REF_ALPHA = 0.001 / 9.0          # the model's constants (bias 1, beta 0.75)
BIG_ALPHA = 0.05
LRN_ALL = [(8, 4), (16, 4), (32, 4), (64, 4), (32, 2), (64, 2), (32, 5), (64, 5)]   # pool_lrn.hip LRN_ALL
BETAS = [0.75, 0.5, 1.0]
BIASES = [1.0, 2.0]
ALPHAS = [REF_ALPHA, BIG_ALPHA]
RAND_PIXELS = 5 * 13 * 13        # 845 pixels: a partial wave at every C


# ------------------------------------------------------------------ reference
def window_sum(t, r):
    """sum over |c' - c| <= r along the last dimension (zeros outside the C channels)."""
    C = t.shape[-1]
    p = torch.nn.functional.pad(t, (r, r))
    s = p[..., 0:C].clone()
    for d in range(1, 2 * r + 1):
        s = s + p[..., d:d + C]
    return s


def vector_extent_sum(t, r):
    """for every channel, the sum of t over all that the running sum of its 8-channel vector
    passes through: the vector's channels and r neighbours on either side."""
    e = torch.nn.functional.pad(t, (r, r)).unfold(-1, 8 + 2 * r, 8).sum(-1)
    return e.repeat_interleave(8, dim=-1)


def lrn_ref(x, g, r, bias, alpha, beta, relu_mask, vector_scale=False):
    """float64 closed form.  Returns (y, dx, Ay, Adx); g may be None (then dx, Adx are None).
    vector_scale: Adx sums |g x sc^-(beta+1)| over the whole extent of the element's 8-channel
    vector, not over its own window.  This is the scale of a running sum's error, for a
    gradient that is zero at most channels (un-pooled through argmax codes): there an
    element's own window can be all zeros, A = 0, while the running sum that reaches it has
    added and removed other channels' terms and keeps their rounding residue."""
    x = x.double()
    sc = bias + alpha * window_sum(x * x, r)
    pw = sc ** -beta
    y = x * pw
    if g is None:
        return y, None, y.abs(), None
    g = g.double()
    pw1 = sc ** -(beta + 1.0)
    t = g * x * pw1
    k = 2.0 * alpha * beta
    dx = g * pw - k * x * window_sum(t, r)
    A = g.abs() * pw + k * x.abs() * (vector_extent_sum(t.abs(), r) if vector_scale else window_sum(t.abs(), r))
    if relu_mask:
        keep = x > 0
        dx = dx * keep
        A = A * keep
    return y, dx, y.abs(), A


def round_to(t, bf16):
    """float64 -> the kernels' output format (one round-to-nearest-even) -> float64."""
    t = t.to(torch.float32)
    return (t.to(torch.bfloat16) if bf16 else t).double()


def lrn_pool_ref(x, H, W, r, bias, alpha, beta, bf16, c=None):
    """LRN, rounded to the output format, then the 2 x 2 / 2 max-pool; x is [N, H, W, C].
    The first maximum in window order d = 2 * row + col wins, as the kernels state.  Returns
      pooled   the maximum of the rounded LRN outputs (what a correct kernel stores when
               none of its four candidates rounds the other way);
      exact    the maximum of the unrounded float64 outputs: the value the budget is about
               (rounding is monotonic, so round(max) == max(round));
      A        the largest |y| of the window: the error of a maximum is at most the
               largest error of its candidates;
      codes    uint8 argmax codes of the rounded outputs;
      decided  True where the code does not depend on the kernel's last bits: the winner,
               moved down by its fp32 budget c 2**-23 |y| and rounded, still beats every other
               candidate moved up by its own and rounded.  That is "the top two differ after
               rounding", less the few windows where a candidate sits within its budget of a
               rounding boundary and the kernel's value may round the other way into a tie.
               Candidates equal in float64 (zeros after a ReLU, mostly) are decided: the
               first wins."""
    N, C = x.shape[0], x.shape[-1]
    c = (C_BF16 if bf16 else C_F32) if c is None else c
    y = lrn_ref(x.reshape(N, H, W, C), None, r, bias, alpha, beta, False)[0]
    cand = y.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)
    rc = round_to(cand, bf16)
    pooled = rc.max(dim=-1).values
    # torch.max may return any index of a tie: take the first by hand
    first = (rc == pooled.unsqueeze(-1)).to(torch.uint8).argmax(dim=-1, keepdim=True)
    b = c * U23 * cand.abs()
    low, high = round_to(cand - b, bf16), round_to(cand + b, bf16)
    win, win_low = cand.gather(-1, first), low.gather(-1, first)
    is_first = torch.arange(4, device=x.device) == first
    decided = (is_first | (win_low > high) | (cand == win)).all(dim=-1)
    return pooled, cand.max(dim=-1).values, cand.abs().max(dim=-1).values, first.squeeze(-1).to(torch.uint8), decided


def unpool(dP, codes, H, W):
    """dL/d(LRN output) [N, H, W, C] from dL/d pooled and the codes: the code's position
    gets the gradient, the other three get 0."""
    N, OH, OW, C = dP.shape
    d = torch.arange(4, device=dP.device, dtype=torch.uint8)
    g = dP.double().unsqueeze(-1) * (codes.unsqueeze(-1) == d)
    return g.reshape(N, OH, OW, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C)


# ------------------------------------------------------------------ float32 transcriptions
def _direct_f32(t, r):
    C = t.shape[-1]
    p = torch.nn.functional.pad(t, (r, r))
    a = torch.zeros_like(t)
    for d in range(2 * r + 1):
        a = a + p[..., d:d + C]
    return a


def _running_f32(t, r):
    """per 8-channel vector: e = r left neighbours, the 8 values, r right neighbours;
    s[0] = e[0] + ... + e[2r] left to right, then s[j] = s[j-1] + (e[j+2r] - e[j-1])."""
    C = t.shape[-1]
    assert C % 8 == 0
    e = torch.nn.functional.pad(t, (r, r)).unfold(-1, 8 + 2 * r, 8)     # [..., C/8, 8 + 2r]
    a = torch.zeros_like(e[..., 0])
    for d in range(2 * r + 1):
        a = a + e[..., d]
    s = [a]
    for j in range(1, 8):
        a = a + (e[..., j + 2 * r] - e[..., j - 1])
        s.append(a)
    return torch.stack(s, dim=-1).reshape(t.shape)


def lrn_f32(x, g, r, bias, alpha, beta, relu_mask, running, b075=False):
    """float32 transcription, every operation rounded on its own.  Returns (y, dx).
    b075 (beta 0.75 only): the powers as lrn_math.h's pow_beta<true> forms them, r = rsqrt(sc),
    q = sqrt(r), sc^-0.75 = r q, sc^-1.75 = (r q) (r r) -- what the LRN-backward folds of
    refc1_wgrad.hip and convpool.hip (LRNB 2) run."""
    f = torch.float32
    win = _running_f32 if running else _direct_f32
    x = x.to(f)
    assert not b075 or beta == 0.75
    bias, alpha, beta = (torch.tensor(v, dtype=f, device=x.device) for v in (bias, alpha, beta))
    sc = alpha * win(x * x, r) + bias
    if b075:
        rs = torch.rsqrt(sc)
        pw = rs * torch.sqrt(rs)
    else:
        lg = torch.log2(sc)
        pw = torch.exp2(-beta * lg)
    y = x * pw
    if g is None:
        return y, None
    g = g.to(f)
    pw1 = pw * (rs * rs) if b075 else torch.exp2(-(beta + 1.0) * lg)
    u = win(g * x * pw1, r)
    dx = g * pw - ((2.0 * alpha * beta) * x) * u
    if relu_mask:
        dx = torch.where(x > 0, dx, torch.zeros_like(dx))
    return y, dx


# ------------------------------------------------------------------ the budget
def half_ulp_bf16(v):
    """half a bf16 ulp (8 significant bits) of |v|; 0 at 0."""
    _, e = torch.frexp(v.abs().double())           # |v| = m 2**e, 0.5 <= m < 1
    return torch.where(v == 0, torch.zeros_like(v, dtype=torch.float64), torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 9))


def units(out, ref, A, bf16=False):
    """largest |out - ref| (bf16: what of it exceeds half a bf16 ulp) in units of 2**-23 A,
    over the elements with A > 0."""
    d = (out.double() - ref).abs()
    if bf16:
        d = (d - half_ulp_bf16(torch.maximum(out.double().abs(), ref.abs()))).clamp_min(0)
    ok = A > 0
    return (d[ok] / (U23 * A[ok])).max().item() if ok.any() else 0.0


def within_budget(out, ref, A, c, bf16):
    """Per element |out - ref| <= (half a bf16 ulp of max(|out|, |ref|) if bf16) + c 2**-23 A,
    and out == 0 exactly where every term of ref is 0 (A == 0: x == 0 in the forward, a masked
    element in the backward; a reference that cancels to 0 from non-zero terms keeps its
    budget).  Returns (ok, report); the report names the worst element (largest error over
    its budget): flat index, channel, both values."""
    o = out.double()
    assert o.shape == ref.shape == A.shape, (o.shape, ref.shape, A.shape)
    d = (o - ref).abs()
    tol = c * U23 * A
    if bf16:
        tol = tol + half_ulp_bf16(torch.maximum(o.abs(), ref.abs()))
    assert not bool(((A == 0) & (ref != 0)).any()), "a reference with no scale"
    zero_bad = (A == 0) & (o != 0)
    bad = (d > tol) | zero_bad | ~torch.isfinite(o)
    n = int(bad.sum().item())
    if n == 0:
        return True, "within budget"
    over = torch.where(zero_bad | ~torch.isfinite(o), torch.full_like(d, math.inf), d / tol.clamp_min(1e-300))
    over = torch.where(bad, over, torch.zeros_like(over))
    i = int(over.reshape(-1).argmax().item())
    C = ref.shape[-1]
    return False, (f"{n} of {ref.numel()} elements over budget (c = {c:g}, bf16 = {bf16}); worst at flat index {i} "
                   f"(pixel {i // C}, channel {i % C}): out {o.reshape(-1)[i].item():.9g}, ref "
                   f"{ref.reshape(-1)[i].item():.9g}, error {d.reshape(-1)[i].item():.3e}, budget "
                   f"{tol.reshape(-1)[i].item():.3e}, A {A.reshape(-1)[i].item():.3e}")


# ------------------------------------------------------------------ input generators (bf16-representable)
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _bf(t):
    return t.to(torch.bfloat16)


def spike_value(alpha):
    """bf16 value v with alpha v^2 about 3: being inside or outside one window changes y by
    tens of percent."""
    return float(_bf(torch.tensor(math.sqrt(3.0 / alpha))))


def spike_probes(C, alpha, signed=False):
    """[2C + 2, C]: pixel 2p is all ones with a spike at channel p (every window edge, every
    vector boundary); pixel 2p + 1 has spikes at channels 0 and C - 1, which sit next to the
    probe's lanes inside a 16-lane row: a term leaking over the pixel boundary shows.  Two
    all-zero pixels close the tensor.  signed: alternating signs along the channels."""
    v = spike_value(alpha)
    x = torch.ones(2 * C + 2, C)
    for p in range(C):
        x[2 * p, p] = v
        x[2 * p + 1, 0] = v
        x[2 * p + 1, C - 1] = v
    if signed:
        x = x * (1.0 - 2.0 * (torch.arange(C) % 3 == 1))
    x[2 * C:] = 0
    out = _bf(x)
    assert torch.equal(out.float(), x)
    return out


def random_pixels(P, C, scale, seed, signed=False):
    """[P, C] normal * scale cut at 4.15 sigma (scale 3 at alpha = 0.05 then stays inside
    DOMAIN), post-ReLU unless signed; pixels 3 and P - 1 are all zero."""
    x = (torch.randn(P, C, generator=_gen(seed)) * scale).clamp(-4.15 * scale, 4.15 * scale)
    if not signed:
        x = x.relu()
    x[3] = 0
    x[P - 1] = 0
    return _bf(x)


def wide_range(P, C, seed):
    """[P, C]: values near 0.25 with one 128 per pixel (a 500 : 1 range inside a window)."""
    g = _gen(seed)
    x = 0.25 + torch.rand(P, C, generator=g) / 16
    x[torch.arange(P), torch.randint(0, C, (P,), generator=g)] = 128.0
    return _bf(x)


def grads(shape, seed):
    return _bf(torch.randn(*shape, generator=_gen(seed)))


def pool_input(N, H, W, C, seed, signed=False):
    """[N, H, W, C] for the LRN -> pool kernels: post-ReLU normal values, each pixel scaled by
    its own factor from 0.25 .. 2.8 so that the candidates of a window rarely round alike,
    |x| <= 12 (inside the domain at alpha = 0.05); one all-zero window."""
    g = _gen(seed)
    x = torch.randn(N, H, W, C, generator=g)
    if not signed:
        x = x.relu()
    x = (x * torch.exp2(3.5 * torch.rand(N, H, W, 1, generator=g) - 2)).clamp(-12, 12)
    x[0, :2, :2, :] = 0
    return _bf(x)


# ------------------------------------------------------------------ the cases of the GPU tests
# tests/test_lrn_oracle_gpu.py runs exactly these; tests/test_lrn_oracle_cpu.py measures the
# transcriptions over exactly these.  Everything is generated on the CPU from fixed seeds.
def standalone_inputs(C, alpha, relu_mask, P=RAND_PIXELS):
    """The inputs of one standalone-kernel case, by name: (x, g).  Signed x where relu_mask
    is False.  Scale 30 only at the model's alpha: at alpha = 0.05 it leaves the domain in
    which the running sum keeps c_bf16 under its cap (DOMAIN below)."""
    signed = not relu_mask
    seed = 1000 * C + (1 if signed else 0)
    out = {"spike": spike_probes(C, alpha, signed), "rand3": random_pixels(P, C, 3.0, seed, signed)}
    if alpha == REF_ALPHA:
        out["rand30"] = random_pixels(P, C, 30.0, seed + 2, signed)
    return {k: (x, grads(x.shape, seed + 7)) for k, x in out.items()}


def standalone_cases():
    """Every (C, r, bias, alpha, beta, relu_mask) of the bf16 standalone kernels' tests."""
    for C, r in LRN_ALL:
        for beta in BETAS:
            for bias in BIASES:
                for alpha in ALPHAS:
                    for relu_mask in (True, False):
                        yield C, r, bias, alpha, beta, relu_mask


def wide_inputs(C):
    """The wide-range case (run at the model's constants only)."""
    x = wide_range(RAND_PIXELS, C, 50 + C)
    return x, grads(x.shape, 60 + C)


# one launch past the 16384-block cap of the standalone kernels' grid (256 lanes per block, 8
# lanes per pixel at C = 64): the grid-stride loop takes a second trip.  The tensor repeats a
# tile of whole pixels, so the reference of the tile, repeated, is the reference of the tensor.
GRID_C, GRID_R, GRID_P = 64, 4, 16384 * 256 // 8 + 37


def grid_tile():
    return standalone_inputs(GRID_C, BIG_ALPHA, True)["rand3"]


def tile_to(t, P):
    return t.repeat((P + t.shape[0] - 1) // t.shape[0], 1)[:P].contiguous()


# (N, H, W, C): 7 * 49, 3 * 49, 5 * 15 and 3 * 15 windows are odd counts, so the last block's
# second window of the two-window unrolling is past the end for part of its lanes
POOL_CASES = [(7, 14, 14, 64), (3, 14, 14, 32), (5, 6, 10, 64), (3, 6, 10, 32)]
POOL_BETAS = [0.75, 0.5]
POOL_R, POOL_BIAS = 4, 1.0
MAX_UNDECIDED = 0.01


def pool_inputs(N, H, W, C, relu):
    """(x [N, H, W, C], dP [N, H/2, W/2, C])"""
    seed = 7000 + 10 * (N * H + C) + (0 if relu else 1)
    return pool_input(N, H, W, C, seed, signed=not relu), grads((N, H // 2, W // 2, C), seed + 5)


# fp32 kernels.  843 pixels is no multiple of 256 / C for any C below (a partial last block,
# and a partial wave on the vector path); C = 24 and 48 do not divide 256 (idle threads).
F32_PIXELS = 843
F32_V4 = [(C, r) for C in (32, 64) for r in (1, 2, 3, 4)]          # lrn_f32_*_v4_k
F32_SCALAR = [(8, 4), (16, 4), (24, 4), (48, 4), (24, 2), (32, 5)]   # lrn_f32_*_k
F32_BETAS = [0.75, 0.5]


def f32_inputs(C, alpha, relu_mask):
    """The bf16 kernels' families (bf16-representable values) held as fp32."""
    return {k: (x.float(), g.float()) for k, (x, g) in standalone_inputs(C, alpha, relu_mask, F32_PIXELS).items()}


def _flat(t):
    return t.reshape(-1, t.shape[-1])


def _pool_points(bf16):
    for N, H, W, C in POOL_CASES:
        for relu in (True, False):
            x, dP = pool_inputs(N, H, W, C, relu)
            for alpha in ALPHAS:
                for beta in POOL_BETAS:
                    codes = lrn_pool_ref(x, H, W, POOL_R, POOL_BIAS, alpha, beta, bf16)[3]
                    g = unpool(dP, codes, H, W)
                    yield f"pool{N}x{H}x{W}x{C}", _flat(x), _flat(g), POOL_R, POOL_BIAS, alpha, beta, relu, bf16


def bf16_points():
    """(name, x, g, r, bias, alpha, beta, relu_mask, vector_scale) of every LRN evaluation the
    bf16 GPU tests ask of a kernel; x, g are [pixels, C].  The pool backward's gradient is
    un-pooled through the reference's codes and held to the vector scale (lrn_ref)."""
    for C, r, bias, alpha, beta, m in standalone_cases():
        for name, (x, g) in standalone_inputs(C, alpha, m).items():
            yield name, x, g, r, bias, alpha, beta, m, False
    for C, r in LRN_ALL:
        x, g = wide_inputs(C)
        for m in (True, False):
            yield "wide", x, g, r, 1.0, REF_ALPHA, 0.75, m, False
    x, g = grid_tile()
    yield "grid", x, g, GRID_R, 1.0, BIG_ALPHA, 0.75, True, False
    yield from _pool_points(True)


def f32_points():
    """The same for the fp32 kernels."""
    for C, r in F32_V4 + F32_SCALAR:
        for alpha in ALPHAS:
            for beta in F32_BETAS:
                for m in (True, False):
                    for name, (x, g) in f32_inputs(C, alpha, m).items():
                        yield name, x, g, r, 1.0, alpha, beta, m, False
    yield from _pool_points(False)


# the domain of the running window sum, as a bound on alpha * max x^2 over a tensor: every
# bf16 input above lies inside it (checked on the CPU), the wide-range case at alpha = 0.05
# (alpha * max x^2 = 819) lies outside and is never sent to a kernel
DOMAIN = 8.0

