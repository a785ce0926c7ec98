"""Max-pool ties: the kernels on inputs where most pool windows hold bit-for-bit equal
candidates (MNIST-like images: a constant -0.5 background, strokes from {-0.5, 0, 0.5}),
against the exact oracle under each kernel's own tie rule, values and codes bitwise, and the
"bitwise the kernel it replaces" claims on the same tied inputs.

The two rules, read from the sources (not from what the kernels return):
* "mantissa" -- convpool.hip (convpool_fwd_k: `vmax(vmax(pos_embed(v[0], 0u), pos_embed(v[1],
  1u)), ...)`; convpool_fwd_quad_k: `vmax(pos_embed(acc[2 * t], sp), pos_embed(acc[2 * t + 1],
  2u + sp))`) and lenet_band.hip (`vmax(vmax3(acc[i] & ~3u, embed(acc[4 + i], 1u), embed(acc[8 +
  i], 2u)), embed(acc[12 + i], 3u))` in lenet_band_fwd_k, refc1n_fwd_k and refc1n3_fwd_k): the
  window position rides in the two low mantissa bits of the raw fp32 sum and a bare v_max_f32
  picks the winner.  Among equal positive sums the highest position has the largest bit
  pattern and wins; among equal negative sums the lowest.
* "first" -- pool_lrn.hip maxpool_fwd_k / lrn_pool_fwd_k (`if (f > best[j])` over d = 0..3),
  lrn_pool14_fwd_k (integer keys `bits << 16 | 3 - d`), f32.hip maxpool_f32_fwd_k and
  conv1_f32.hip conv1_f32_fwd_pool_k (`if (v[d] > bv)`): the first maximum wins.

So the bf16 and the fp32 paths differ on ties (test_bf16_and_f32_paths_differ_on_ties pins it).

Raw sums tied at exactly zero are kept out of these inputs (exact_oracle.zero_tie_free drops
the few images that have one; tie_census asserts it): with a position embedded a zero is a
denormal, and its order then depends on the fp32 denormal mode of the build.
"""
import pytest
import torch

import exact_oracle as xo
from test_lenet_band_gpu import _band
from test_lenet_bwd_gpu import _fused

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
LRN = dict(r=4, bias=1.0, alpha=0.001 / 9.0, beta=0.75)


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _nan(*shape, dev, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _ee(*shape, dev):
    return torch.full(shape, 0xEE, dtype=torch.uint8, device=dev)


def _tied_images(dev, B, cin, w, cout, seed, dtype=BF):
    """B MNIST-like images (replicated over cin channels) without a zero-sum tie under w"""
    g = _gen(dev, seed)
    x = xo.mnist_like(3 * B + 8, g, dev, dtype=dtype).expand(-1, 28, 28, cin).contiguous()
    x = x[xo.zero_tie_free(x, w, "SAME", cout)][:B].contiguous()
    assert x.shape[0] == B
    return x


def _covered(census):
    """the input condition, from the reference alone"""
    assert census["tied_zero"] == 0, census
    assert census["tied"] > census["windows"] // 4, census
    assert min(census["tied_positive"], census["tied_negative_live"], census["tied_negative_dead"]) > 0, census


def _convpool(K, x, w, b, co, B, Ci, Co, pad, H):
    PH = (H if pad else H - 4) // 2
    ab = K.convpool_arg_bytes(Ci, Co, 5, pad, H, H)
    P = _nan(B, PH, PH, Co, dev=x.device, dtype=BF)
    A = _ee(B, PH, PH, ab, dev=x.device)
    K.convpool_fwd(x, w, b, co, P, A, B, Ci, Co, 5, pad, H, H)
    return P, (A if ab == Co else xo.unpack_codes(A))


# ------------------------------------------------------------------ forward: convpool / band / refc1n
def _lenet_tied(dev, B, seed):
    g = _gen(dev, seed)
    w1, b1 = xo.tie_conv_params(1, 1, 8, 6, 16.0, g, dev)
    w2, b2 = xo.tie_conv_params(8, 6, 16, 16, 2048.0, g, dev)
    x = _tied_images(dev, B, 1, w1, 6, seed + 1)
    P1, c1, P2, c2 = xo.lenet_fwd(x, w1, b1, w2, b2, "mantissa", (3, 5))
    _covered(xo.tie_census(x, w1, b1, "SAME", 6))
    c2s = xo.tie_census(P1, w2, b2, "VALID")
    assert c2s["tied_zero"] == 0 and c2s["tied_positive"] > 0 and c2s["tied_negative_live"] > 0, c2s
    return x, w1, b1, w2, b2, P1, c1, P2, c2


@pytest.mark.parametrize("B,cap", [(17, 0), (40, 2)])
def test_lenet_forward_ties(dev, K, grid_cap, B, cap):
    """lenet_band_fwd_k and the per-layer convpool kernels (convpool_fwd_quad_k for conv1,
    convpool_fwd_k for conv2) under the mantissa rule, and band == convpool bitwise"""
    grid_cap(cap)
    x, w1, b1, w2, b2, P1, c1, P2, c2 = _lenet_tied(dev, B, 21)
    assert set(c1.unique().tolist()) == {0, 1, 2, 3, 4} and set(c2.unique().tolist()) == {0, 1, 2, 3, 4}
    Q1, A1, Q2, A2 = _band(K, x, w1, b1, w2, b2, B)
    for got, ref, what in ((Q1, P1, "P1"), (xo.unpack_codes(A1), c1, "A1"), (Q2, P2, "P2"), (A2, c2, "A2")):
        assert torch.equal(got, ref), "band " + what
    T1, D1 = _convpool(K, x, w1, b1, 6, B, 1, 8, 2, 28)
    T2, D2 = _convpool(K, P1, w2, b2, 16, B, 8, 16, 0, 14)
    for got, ref, what in ((T1, P1, "P1"), (D1, c1, "A1"), (T2, P2, "P2"), (D2, c2, "A2")):
        assert torch.equal(got, ref), "convpool " + what


@pytest.mark.parametrize("cin", [1, 3])
def test_refc1_forward_ties(dev, K, grid_cap, cin):
    """reference conv1 (28 x 28 x cin -> 32): refc1n_fwd_k / refc1n3_fwd_k (variant 2) and the
    kernels they replaced (variant 1: the round-5 band kernel for 1 channel, the generic
    convpool_fwd_k for 3), all under the mantissa rule and bitwise each other"""
    grid_cap(3)
    B = 20
    g = _gen(dev, 30 + cin)
    w, b = xo.tie_conv_params(cin, cin, 32, 32, 16.0 * cin, g, dev)
    x = _tied_images(dev, B, cin, w, 32, 40 + cin)
    _covered(xo.tie_census(x, w, b, "SAME"))
    o, codes = xo.convpool_fwd(x, w, b, "SAME", "mantissa", 3)
    outs = {}
    for variant in (1, 2):
        K.refc1_set_fwd_variant(variant)
        try:
            outs[variant] = _convpool(K, x, w, b, 32, B, cin, 32, 2, 28)
        finally:
            K.refc1_set_fwd_variant(2)
        assert torch.equal(outs[variant][0], xo.to_bf16(o)), ("pool1", variant)
        assert torch.equal(outs[variant][1], codes), ("codes", variant)
    assert torch.equal(outs[1][0], outs[2][0]) and torch.equal(outs[1][1], outs[2][1])


# ------------------------------------------------------------------ forward: the "first" family
def _tied_activations(dev, N, H, W, C, seed, dtype=BF):
    """post-ReLU activations whose 2x2 windows are, in turn: four identical pixel vectors,
    two identical rows, two identical columns, small repeated integers"""
    g = _gen(dev, seed)
    oh, ow = (H + 1) // 2, (W + 1) // 2
    base = xo.dyadic((N, oh, ow, C), -3, 6, 1, g, dev, dtype=dtype).relu()
    alt = xo.dyadic((N, oh, ow, C), -3, 6, 1, g, dev, dtype=dtype).relu()
    kind = torch.randint(0, 4, (N, oh, ow, 1), generator=g, device=dev)
    full = lambda t: t.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
    xb, xa, k = full(base), full(alt), full(kind)
    row = (torch.arange(H, device=dev) % 2).view(1, H, 1, 1)
    col = (torch.arange(W, device=dev) % 2).view(1, 1, W, 1)
    x = torch.where((k == 1) & (row == 1), xa, xb)             # kind 1: rows differ, columns tie
    x = torch.where((k == 2) & (col == 1), xa, x)              # kind 2: columns differ, rows tie
    rnd = xo.dyadic((N, H, W, C), 0, 2, 1, g, dev, dtype=dtype)
    x = torch.where(k == 3, rnd, x)                            # kind 3: three values, many partial ties
    return x.contiguous()


@pytest.mark.parametrize("N,H,W,C", [(4, 28, 28, 8), (3, 14, 14, 64), (2, 7, 7, 16)])
def test_maxpool_ties(dev, K, N, H, W, C):
    """maxpool_fwd_k (bf16) and maxpool_f32_fwd_k: the first maximum wins (pool_lrn.hip: `if (f >
    best[j])`; f32.hip: `if (v > best)`), the two paths agree with each other"""
    x = _tied_activations(dev, N, H, W, C, 50 + H)
    ry, rarg = xo.maxpool2x2(x, "first")
    assert set(rarg.unique().tolist()) == {0, 1, 2, 3}
    assert not torch.equal(rarg, xo.maxpool2x2(x, "mantissa")[1])       # the rules differ on this input
    OH, OW = rarg.shape[1:3]
    y = _nan(N, OH, OW, C, dev=dev, dtype=BF)
    arg = _ee(N, OH, OW, C, dev=dev)
    K.maxpool_fwd(x, y, arg, N, H, W, C, OH, OW)
    assert torch.equal(y, xo.to_bf16(ry)) and torch.equal(arg, rarg)
    y32 = _nan(N, OH, OW, C, dev=dev)
    a32 = _ee(N, OH, OW, C, dev=dev)
    K.f32_maxpool_fwd(x.float(), y32, a32, N, H, W, C)
    assert torch.equal(y32, xo.to_f32(ry)) and torch.equal(a32, rarg)


@pytest.mark.parametrize("N", [1, 77])
def test_lrn_pool_ties(dev, K, N):
    """lrn_pool14_fwd_k == lrn_pool_fwd_k == lrn_fwd + maxpool_fwd (values and codes) on
    windows of identical pixel vectors, whose post-LRN values tie exactly; a fully tied
    window reports position 0.  lrn_pool_bwd (packed and generic) == maxpool_bwd + lrn_bwd
    bitwise on the forward's codes and on codes that hold every value 0..4."""
    x = _tied_activations(dev, N, 14, 14, 64, 60 + N)
    r, bias, alpha, beta = LRN["r"], LRN["bias"], LRN["alpha"], LRN["beta"]
    l = _nan(N, 14, 14, 64, dev=dev, dtype=BF)
    K.lrn_fwd(x, l, N * 196, 64, r, bias, alpha, beta)
    y0 = _nan(N, 7, 7, 64, dev=dev, dtype=BF)
    a0 = _ee(N, 7, 7, 64, dev=dev)
    K.maxpool_fwd(l, y0, a0, N, 14, 14, 64, 7, 7)
    win = xo._windows(x.double())
    all_tied = (win == win[..., :1]).all(-1).all(-1, keepdim=True).expand_as(a0)    # the whole pixel vector repeats
    assert all_tied.float().mean() > 0.05
    assert torch.equal(a0[all_tied], torch.zeros_like(a0[all_tied]))
    g = _gen(dev, 61)
    dP = xo.dyadic((N, 7, 7, 64), -4, 4, 2, g, dev)
    any_codes = torch.randint(0, 5, (N, 7, 7, 64), generator=g, device=dev).to(torch.uint8)
    for packed in (True, False):
        K.lrn_set_packed(packed)
        try:
            y = _nan(N, 7, 7, 64, dev=dev, dtype=BF)
            a = _ee(N, 7, 7, 64, dev=dev)
            K.lrn_pool_fwd(x, y, a, N, 14, 14, 64, r, bias, alpha, beta, nonneg=True)
            assert torch.equal(y, y0) and torch.equal(a, a0), packed
            for codes in (a0, any_codes):
                dx = _nan(N, 14, 14, 64, dev=dev, dtype=BF)
                K.lrn_pool_bwd(x, dP, codes, dx, N, 14, 14, 64, r, bias, alpha, beta, True)
                dl = _nan(N, 14, 14, 64, dev=dev, dtype=BF)
                K.maxpool_bwd(dP, codes, y0, False, dl, N, 14, 14, 64, 7, 7)
                dx2 = _nan(N, 14, 14, 64, dev=dev, dtype=BF)
                K.lrn_bwd(x, dl, dx2, N * 196, 64, r, bias, alpha, beta, True)
                assert torch.equal(dx, dx2), packed
        finally:
            K.lrn_set_packed(True)


def _f32_conv1_tied(dev, B, seed):
    g = _gen(dev, seed)
    w, b = xo.tie_conv_params(1, 1, 32, 32, 16.0, g, dev, wdtype=F32)
    x = _tied_images(dev, B, 1, w, 32, seed + 1, dtype=F32)
    return x, w, b


def test_f32_conv1_pool_ties(dev, K, grid_cap):
    """f32_conv1_fwd_pool (conv1_f32_fwd_pool_k: bias + ReLU, then `if (v[d] > bv)`) against the
    oracle under "first", and == the unfused f32_conv_fwd + f32_maxpool_fwd: the same values,
    the same codes wherever the output is positive; the fused kernel writes 4 where it is 0
    (the unfused pool has no ReLU mask in its codes and reports the first zero)"""
    grid_cap(5)
    B = 40
    x, w, b = _f32_conv1_tied(dev, B, 70)
    _covered(xo.tie_census(x, w, b, "SAME"))
    o, codes = xo.convpool_fwd(x, w, b, "SAME", "first", 3)
    y = _nan(B, 14, 14, 32, dev=dev)
    arg = _ee(B, 14, 14, 32, dev=dev)
    K.f32_conv1_fwd_pool(x, w, b, y, arg, B)
    assert torch.equal(y, xo.to_f32(o)) and torch.equal(arg, codes)
    c = _nan(B, 28, 28, 32, dev=dev)
    K.f32_conv_fwd(x, w, c, B, 28, 28, 1, 28, 28, 5, 5, 2, 2, 32, b, True)
    y2 = _nan(B, 14, 14, 32, dev=dev)
    a2 = _ee(B, 14, 14, 32, dev=dev)
    K.f32_maxpool_fwd(c, y2, a2, B, 28, 28, 32)
    assert torch.equal(y2, y)
    live = y > 0
    assert torch.equal(a2[live], arg[live])
    assert torch.equal(arg[~live], torch.full_like(arg[~live], 4))
    assert torch.equal(a2, xo.maxpool2x2(c, "first")[1])


def test_bf16_and_f32_paths_differ_on_ties(dev, K):
    """Existing behaviour, pinned: on the same tied input the bf16 path (mantissa rule) and the
    fp32 path (first maximum) produce the same pooled values but other codes -- position 3
    against position 0 where four equal positive sums meet.  Either routes the whole gradient
    to one of the equal candidates."""
    B = 12
    x, w, b = _f32_conv1_tied(dev, B, 80)
    P, A = _convpool(K, x.to(BF), w.to(BF), b, 32, B, 1, 32, 2, 28)
    y = _nan(B, 14, 14, 32, dev=dev)
    arg = _ee(B, 14, 14, 32, dev=dev)
    K.f32_conv1_fwd_pool(x, w, b, y, arg, B)
    assert torch.equal(P, y.to(BF))
    assert torch.equal(A == 4, arg == 4)
    win = xo._windows(xo._conv(x.double(), w.double(), "SAME"))
    four_pos = (win == win[..., :1]).all(-1) & (win[..., 0] > 0) & (y > 0)
    assert four_pos.any()
    assert torch.equal(A[four_pos], torch.full_like(A[four_pos], 3))
    assert torch.equal(arg[four_pos], torch.zeros_like(arg[four_pos]))


# ------------------------------------------------------------------ backward: kernels that consume codes
def _code_sets(codes, g):
    """the forward's own codes (every tied pattern of the input) and uniformly random 0..4"""
    rnd = torch.randint(0, 5, tuple(codes.shape), generator=g, device=codes.device).to(torch.uint8)
    return (("forward", codes), ("random", rnd))


@pytest.mark.parametrize("N,H,W,C", [(3, 14, 14, 64), (2, 7, 7, 16)])
def test_maxpool_bwd_any_codes(dev, K, N, H, W, C):
    x = _tied_activations(dev, N, H, W, C, 90 + H)
    ry, rarg = xo.maxpool2x2(x, "first")
    OH, OW = rarg.shape[1:3]
    g = _gen(dev, 91)
    dy = xo.dyadic((N, OH, OW, C), -4, 4, 1, g, dev)
    y = xo.to_bf16(ry)
    for name, codes in _code_sets(rarg, g):
        if H % 2:                      # no code may point outside a 7 x 7 input
            edge = torch.zeros_like(codes, dtype=torch.bool)
            edge[:, -1, :, :] = True
            edge[:, :, -1, :] = True
            codes = torch.where(edge & (codes < 4), rarg, codes)
        for relu_mask in (False, True):
            dx = _nan(N, H, W, C, dev=dev, dtype=BF)
            K.maxpool_bwd(dy, codes, y, relu_mask, dx, N, H, W, C, OH, OW)
            gy = torch.where(ry > 0, dy.double(), torch.zeros_like(ry)) if relu_mask else dy.double()
            assert torch.equal(dx, xo.to_bf16(xo.unpool(gy, codes, (H, W)))), (name, relu_mask)
            dx32 = _nan(N, H, W, C, dev=dev)
            K.f32_maxpool_bwd(dy.float(), codes, y.float(), relu_mask, dx32, N, H, W, C)
            assert torch.equal(dx32, xo.to_f32(xo.unpool(gy, codes, (H, W)))), (name, relu_mask, "f32")


@pytest.mark.parametrize("cap", [0, 2])
def test_convpool_bwd_any_codes(dev, K, grid_cap, cap):
    """convpool_dgrad / convpool_wgrad (LeNet conv2 and conv1 geometries) on tied inputs with
    the forward's codes and with random codes 0..4"""
    grid_cap(cap)
    B = 19
    x, w1, b1, w2, b2, P1, c1, P2, c2 = _lenet_tied(dev, B, 100)
    g = _gen(dev, 101)
    for (xin, w, codes0, Ci, ci, Co, co, pad, H, ux) in ((P1, w2, c2, 8, 6, 16, 16, 0, 14, 3),
                                                        (x, w1, c1, 1, 1, 8, 6, 2, 28, 1)):
        padding = "SAME" if pad else "VALID"
        PH = codes0.shape[1]
        dP = xo.dyadic((B, PH, PH, Co), -4, 4, 3, g, dev, density=0.5)
        KM = K.convpool_rows(Ci, Co, 5, pad, H, H)
        G, Ip, I, brow = K.convpool_reduce_args(Ci, Co, 5, pad, H, H, ci)
        for name, codes in _code_sets(codes0, g):
            arg = codes if K.convpool_arg_bytes(Ci, Co, 5, pad, H, H) == Co else xo.pack_codes(codes)
            dY = xo.unpool(dP, codes)
            rw, rb = xo.conv_wgrad(xin, dY, 5, 5, padding, ux + 3, 3)
            grid = cap or 7
            slab = _nan(grid * KM * Co, dev=dev)
            K.convpool_wgrad(xin, dP, arg, slab, grid, B, Ci, Co, 5, pad, H, H)
            dw = _nan(5, 5, ci, co, dev=dev)
            db = _nan(co, dev=dev)
            K.splitk_reduce(slab, grid, KM, Co, G, Ip, I, co, brow, dw, db, 1.0)
            assert torch.equal(dw, xo.to_f32(rw[:, :, :ci, :co])), (name, Ci, "dw")
            assert torch.equal(db, xo.to_f32(rb[:co])), (name, Ci, "db")
            if K.convpool_has_dgrad(Ci, Co, 5, pad, H, H):
                dx = _nan(B, H, H, Ci, dev=dev, dtype=BF)
                K.convpool_dgrad(dP, arg, w, dx, B, Ci, Co, 5, pad, H, H)
                ref = xo.to_bf16(xo.conv_dgrad(dY, w, (H, H), padding, None, 5))
                assert torch.equal(dx[..., :ci], ref[..., :ci]), (name, "dx")


@pytest.mark.parametrize("B,cap", [(13, 0), (40, 2)])
def test_lenet_bwd_any_codes(dev, K, grid_cap, B, cap):
    """lenet_bwd on the tied forward's codes and on random ones.  The random pool1 codes keep
    the forward's invariant "code 4 exactly where pool1 is 0": lenet_bwd.hip takes conv1's
    bias gradient over the windows whose pool1 value is > 0 instead of re-reading the code
    words (the comment at its `pv[u]` loads says why), so codes that break the invariant are
    not an input it accepts.  Within it the positions 0..3 are random.  pool2 codes are free."""
    grid_cap(cap)
    x, w1, b1, w2, b2, P1, c1, P2, c2 = _lenet_tied(dev, B, 110)
    g = _gen(dev, 111)
    dP2 = xo.dyadic((B, 400), -4, 4, 3, g, dev, density=0.5)
    r1 = torch.randint(0, 4, tuple(c1.shape), generator=g, device=dev).to(torch.uint8)
    r1 = torch.where(P1 > 0, r1, torch.full_like(r1, 4))
    r2 = torch.randint(0, 5, tuple(c2.shape), generator=g, device=dev).to(torch.uint8)
    for what, k1, k2 in (("forward", c1, c2), ("random", r1, r2)):
        want = xo.lenet_bwd(x, P1, k1, k2, dP2, w2, (6, 5, 6))      # P1 2**-3 * dP2 2**-3; dP2 * w2 2**-2; x 2**-1 * dP1
        got = _fused(K, x, P1, xo.pack_codes(k1), k2, dP2, w2, B)
        for name, gk, wk in zip(("dW1", "db1", "dW2", "db2"), got[:4], want):
            assert torch.equal(gk, xo.to_f32(wk)), (what, name)
