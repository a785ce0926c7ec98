"""Every linear and pooling HIP kernel against the exact oracle (tests/exact_oracle.py), bit for bit.

Inputs are small integers times a power of two (optionally sparse), so every product and
every fp32 partial sum is exact in any order: fp32 outputs (split-K slabs after
splitk_reduce included) equal the float64 reference, bf16 outputs are its one
round-to-nearest-even, and the argmax codes are decided.  The only comparison in this file
is torch.equal; outputs are poisoned (NaN / 0xEE) before each launch.

Tie rules used here, from the kernel sources:
* convpool.hip (pos_embed / vmax, the epilogues of convpool_fwd_k and convpool_fwd_quad_k) and
  lenet_band.hip (embed / vmax / vmax3, the epilogues of lenet_band_fwd_k, refc1n_fwd_k and
  refc1n3_fwd_k): the position rides in the two low mantissa bits of the raw fp32 sum and a bare
  v_max_f32 picks the winner -- "mantissa".  A raw sum of exactly +0 with a position embedded
  is a positive denormal; the extensions are built without any flush-to-zero flag (_build.py:
  -O3 only, fp32 denormals stay enabled), so zero sums order like positive ones.
* pool_lrn.hip maxpool_fwd_k, f32.hip maxpool_f32_fwd_k, conv1_f32.hip conv1_f32_fwd_pool_k: a
  strict `>` scan in position order -- "first".
"""
import pytest
import torch

import exact_oracle as xo
from distributed_tensorflow_ibm_mnist_amd.ops import functional as Fk
from test_kernels_gpu import CONV_CASES, CP_CASES
from test_lenet_band_gpu import _band, _combined
from test_lenet_bwd_gpu import _fused

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _nan(*shape, dev, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _as(ref, dtype):
    return xo.to_bf16(ref) if dtype == BF else xo.to_f32(ref)


def _same(got, ref, what=""):
    """bitwise-in-value equality (NaN poison left behind fails it)"""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    assert torch.equal(got, ref), what


# ================================================================== gemm.hip: dense
# (M, N, K, extra shift): the extra shift repeats one case with the inputs scaled by 2**-4
DENSE = [(37, 120, 400, 0), (5, 16, 88, 0), (3, 1024, 3136, 0), (300, 192, 1024, 0), (37, 120, 400, 4),
         (77, 13, 37, 0), (5, 3, 9, 0)]      # the last two: the general (scalar-tail) loaders


def _dense_inputs(dev, M, N, Kd, e, seed, dtype=BF):
    g = _gen(dev, seed)
    d = xo.density_for(Kd)
    x = xo.dyadic((M, Kd), -4, 4, 1 + e, g, dev, density=d, dtype=dtype)
    w = xo.dyadic((Kd, N), -4, 4, 2, g, dev, density=d, dtype=dtype)
    b = xo.dyadic((N,), -64, 64, 3 + e, g, dev, dtype=F32)
    return g, x, w, b, 3 + e


@pytest.mark.parametrize("M,N,Kd,e", DENSE)
@pytest.mark.parametrize("relu", [False, True])
def test_dense_forward_exact(dev, K, M, N, Kd, e, relu):
    g, x, w, b, unit = _dense_inputs(dev, M, N, Kd, e, 100 + M)
    ref = xo.dense_fwd(x, w, b, relu, unit)
    for dt in (BF, F32):
        out = _nan(M, N, dev=dev, dtype=dt)
        Fk.dense(x, w, b, relu, out_dtype=dt, out=out)
        _same(out, _as(ref, dt), dt)


def test_dense_bias_padding_exact(dev, K):
    """bias for the first 10 of 16 columns; the padded columns (zero weights) are exactly 0"""
    g, x, w, b, unit = _dense_inputs(dev, 50, 16, 88, 0, 7)
    w[:, 10:] = 0
    ref = xo.dense_fwd(x, w, b[:10], False, unit)
    for dt in (BF, F32):
        out = _nan(50, 16, dev=dev, dtype=dt)
        Fk.dense(x, w, b[:10].contiguous(), False, out_dtype=dt, bias_n=10, out=out)
        _same(out, _as(ref, dt), dt)
        assert torch.equal(out[:, 10:], torch.zeros_like(out[:, 10:]))


@pytest.mark.parametrize("M,N,Kd,e", DENSE)
def test_dense_dgrad_exact(dev, K, M, N, Kd, e):
    """dX[M, Din = Kd] = dY[M, Dout = N] . W[Din, Dout]^T, with and without the ReLU mask"""
    g = _gen(dev, 200 + M)
    d = xo.density_for(N)
    dy = xo.dyadic((M, N), -4, 4, 1 + e, g, dev, density=d)
    w = xo.dyadic((Kd, N), -4, 4, 2, g, dev, density=d)
    mask = xo.dyadic((M, Kd), -2, 2, 1, g, dev)
    for m in (None, mask):
        out = _nan(M, Kd, dev=dev, dtype=BF)
        Fk.dense_dgrad(dy, w, mask=m, out=out)
        _same(out, xo.to_bf16(xo.dense_dgrad(dy, w, m, 3 + e)), "masked" if m is not None else "plain")


def _dense_wgrad(K, x, dy, din, dout, splits, scale, tile=-1):
    B, Dp = x.shape
    Np = dy.shape[1]
    M = Dp + 1
    S = Fk.pick_splits(M, Np, B, dense=True) if splits is None else Fk.eff_splits(B, splits)
    slab = _nan(S * M * Np, dev=x.device)
    S = K.dense_wgrad(x, dy, slab, Dp, Np, B, Dp, Np, True, S, tile)
    dw = _nan(din, dout, dev=x.device)
    db = _nan(dout, dev=x.device)
    K.splitk_reduce(slab, S, M, Np, 1, Dp, din, dout, Dp, dw, db, scale)
    return dw, db, S


# (B, Din, Dout, splits, extra shift); 37 rows are 2 K steps: splits = 7 exceeds them
WGRAD = [(37, 400, 120, None, 0), (37, 400, 120, 1, 0), (37, 400, 120, 3, 0), (37, 400, 120, 7, 0),
         (5, 88, 16, None, 0), (5, 88, 16, 3, 0), (3, 3136, 1024, None, 0), (300, 1024, 192, None, 0),
         (300, 1024, 192, 3, 0), (300, 1024, 192, 1, 4), (64, 88, 16, 3, 0), (77, 37, 13, None, 0), (5, 9, 3, 1, 0)]


@pytest.mark.parametrize("B,Din,Dout,splits,e", WGRAD)
def test_dense_wgrad_exact(dev, K, B, Din, Dout, splits, e):
    """split-K slabs + splitk_reduce (Din / Dout unpadded where the layer pads them), with
    scale 1 and, for a power-of-two batch, 1 / B (exact)"""
    g = _gen(dev, 300 + B + Din)
    x = xo.dyadic((B, Din), -4, 4, 1 + e, g, dev)
    dy = xo.dyadic((B, Dout), -4, 4, 2, g, dev)
    din = Din - 4 if (Din % 8 == 0 and Din > 100) else Din
    dout = Dout - 6 if Dout == 16 else Dout
    rw, rb = xo.dense_wgrad(x, dy, 3 + e, 2)
    scales = (1.0, 1.0 / B) if B & (B - 1) == 0 else (1.0,)
    for scale in scales:
        dw, db, S = _dense_wgrad(K, x, dy, din, dout, splits, scale)
        _same(dw, xo.to_f32(rw[:din, :dout] * scale), ("dw", scale))
        _same(db, xo.to_f32(rb[:dout] * scale), ("db", scale))


# every tile code of launch_any on a small problem: the bindings' tile= argument is the code
# (gemm.hip launch_pick passes it to launch_any when both operands take the vector loaders).
# M = two tile heights + 3, N = one tile width + 8, K = 72 (two 32-deep steps and a tail of 8)
TILE_BM = [256, 256, 128, 64, 128, 64, 64, 64, 256, 32, 64, 128]      # gemm.hip gemm_tile(): BMS / BNS
TILE_BN = [16, 32, 64, 128, 128, 16, 32, 64, 128, 192, 192, 192]


@pytest.mark.parametrize("code", range(12))
def test_gemm_tile_codes_fwd_dgrad_exact(dev, K, code):
    bm, bn = TILE_BM[code], TILE_BN[code]
    M, N, Kd = 2 * bm + 3, bn + 8, 72
    g, x, w, b, unit = _dense_inputs(dev, M, N, Kd, 0, 400 + code)
    ref = xo.dense_fwd(x, w, b, True, unit)
    for dt in (BF, F32):
        out = _nan(M, N, dev=dev, dtype=dt)
        K.dense_fwd(x, w, out, M, N, Kd, Kd, N, N, b, N, True, None, 0, code)
        _same(out, _as(ref, dt), ("fwd", dt))
    # dgrad on the same tile: dX[M, Din = N] = dY[M, Dout = Kd] . W[Din, Dout]^T
    wd = xo.dyadic((N, Kd), -4, 4, 2, g, dev)
    mask = xo.dyadic((M, N), -2, 2, 1, g, dev)
    for m in (None, mask):
        out = _nan(M, N, dev=dev, dtype=BF)
        K.dense_dgrad(x, wd, out, M, N, Kd, Kd, Kd, N, m, N if m is not None else 0, code)
        _same(out, xo.to_bf16(xo.dense_dgrad(x, wd, m, 3)), ("dgrad", m is not None))


# weight-gradient tiles launch_any offers (no 256 x 16 / 256 x 32 / 32 x 192 / 64 x 192 there)
@pytest.mark.parametrize("code", [2, 3, 4, 5, 6, 7, 8, 11])
def test_gemm_tile_codes_wgrad_exact(dev, K, code):
    bm, bn = TILE_BM[code], TILE_BN[code]
    Din, Dout, B = 2 * bm + 8, bn + 8, 72          # M = Din + 1 bias row: a third, 9-row tile
    g = _gen(dev, 500 + code)
    x = xo.dyadic((B, Din), -4, 4, 1, g, dev)
    dy = xo.dyadic((B, Dout), -4, 4, 2, g, dev)
    rw, rb = xo.dense_wgrad(x, dy, 3, 2)
    for splits in (1, 2):
        dw, db, S = _dense_wgrad(K, x, dy, Din, Dout, splits, 1.0, tile=code)
        assert S == splits
        _same(dw, xo.to_f32(rw), "dw")
        _same(db, xo.to_f32(rb), "db")


# ================================================================== gemm256.hip
@pytest.fixture(params=[0, 2, 4, 16], ids=["bk32_4stage", "bk64_2stage", "bk32_5stage", "bk32_4stage_rp"])
def ring(request, K):
    K.set_gemm256_debug(request.param)
    yield request.param
    K.set_gemm256_debug(0)


_G256 = {}


def _g256_case(dev, M, N, Kd, e=0):
    """inputs and float64 references (a float64 matmul on the device), once per shape"""
    key = (M, N, Kd, e)
    if key not in _G256:
        g, x, w, b, unit = _dense_inputs(dev, M, N, Kd, e, M + N + Kd)
        ref = xo.dense_fwd(x, w, b, True, unit)
        _G256[key] = (x, w, b, xo.to_bf16(ref), xo.to_f32(ref))
    return _G256[key]


def _routes(K, f):
    """f() on the gemm256 route and on gemm.hip"""
    assert K.gemm256_enabled()
    try:
        new = f()
        K.set_gemm256(False)
        old = f()
    finally:
        K.set_gemm256(True)
    return new, old


@pytest.mark.parametrize("M,N,Kd", [(8104, 2040, 520), (4096, 4096, 512)])
@pytest.mark.parametrize("dt", [BF, F32])
def test_gemm256_fwd_exact(dev, K, ring, M, N, Kd, dt):
    x, w, b, ref_bf, ref_f32 = _g256_case(dev, M, N, Kd)

    def run():
        out = _nan(M, N, dev=dev, dtype=dt)
        K.dense_fwd(x, w, out, M, N, Kd, Kd, N, N, b, N, True, None, 0)
        return out
    new, old = _routes(K, run)
    ref = ref_bf if dt == BF else ref_f32
    _same(new, ref, "gemm256")
    _same(old, ref, "gemm.hip")


@pytest.mark.parametrize("dt", [BF, F32])
def test_gemm256_fwd_scaled_exact(dev, K, dt):
    """the tail shape again with the inputs scaled by 2**-4 (default ring)"""
    M, N, Kd = 8104, 2040, 520
    x, w, b, ref_bf, ref_f32 = _g256_case(dev, M, N, Kd, 4)
    assert K.gemm256_enabled()
    out = _nan(M, N, dev=dev, dtype=dt)
    K.dense_fwd(x, w, out, M, N, Kd, Kd, N, N, b, N, True, None, 0)
    _same(out, ref_bf if dt == BF else ref_f32, dt)


@pytest.mark.parametrize("with_mask", [False, True])
def test_gemm256_dgrad_exact(dev, K, ring, with_mask):
    M, N, Kd = 8104, 2040, 520           # dX[M, N] = dY[M, Kd] . W[N, Kd]^T (test_gemm256_dgrad's roles)
    key = ("dgrad", with_mask)
    if key not in _G256:
        g = _gen(dev, 7 * M + N)
        d = xo.density_for(Kd)
        dy = xo.dyadic((M, Kd), -4, 4, 1, g, dev, density=d)
        w = xo.dyadic((N, Kd), -4, 4, 2, g, dev, density=d)
        mask = xo.dyadic((M, N), -2, 2, 1, g, dev) if with_mask else None
        _G256[key] = (dy, w, mask, xo.to_bf16(xo.dense_dgrad(dy, w, mask, 3)))
    dy, w, mask, ref = _G256[key]

    def run():
        out = _nan(M, N, dev=dev, dtype=BF)
        K.dense_dgrad(dy, w, out, M, N, Kd, Kd, Kd, N, mask, N if with_mask else 0)
        return out
    new, old = _routes(K, run)
    _same(new, ref, "gemm256")
    _same(old, ref, "gemm.hip")


def test_gemm256_wgrad_bias_row_exact(dev, K, ring):
    B, Din, Dout, cap = 5000, 3000, 1000, 8
    key = "wgrad"
    if key not in _G256:
        g = _gen(dev, B + Din)
        x = xo.dyadic((B, Din), -4, 4, 1, g, dev, density=0.5)
        dy = xo.dyadic((B, Dout), -4, 4, 2, g, dev, density=0.5)
        rw, rb = xo.dense_wgrad(x, dy, 3, 2)
        _G256[key] = (x, dy, xo.to_f32(rw), xo.to_f32(rb))
    x, dy, rw, rb = _G256[key]
    M = Din + 1

    def run():
        slab = _nan(cap * M * Dout, dev=dev)
        S = K.dense_wgrad(x, dy, slab, Din, Dout, B, Din, Dout, True, cap)
        dw = _nan(Din, Dout, dev=dev)
        db = _nan(Dout, dev=dev)
        K.splitk_reduce(slab, S, M, Dout, 1, Din, Din, Dout, Din, dw, db, 1.0)
        return dw, db, S
    (dw, db, s_new), (dw0, db0, s_old) = _routes(K, run)
    assert 1 <= s_new < cap and s_old == cap          # the 256 x 256 path took it
    _same(dw, rw, "gemm256 dw")
    _same(db, rb, "gemm256 db")
    _same(dw0, rw, "gemm.hip dw")
    _same(db0, rb, "gemm.hip db")


@pytest.mark.parametrize("M,N,Kd", [(8104, 2040, 520), (4096, 512, 4096)])
def test_gemm256_f32_twin_exact(dev, K, M, N, Kd):
    """the fp32 twin (v_mfma_f32_16x16x4_f32): forward and masked dgrad, whichever engine the
    fp32 router picks for the shape"""
    g, x, w, b, unit = _dense_inputs(dev, M, N, Kd, 0, 3 * M + Kd, dtype=F32)
    y = _nan(M, N, dev=dev)
    K.f32_dense_fwd(x, w, y, M, N, Kd, N, b, True)
    _same(y, xo.to_f32(xo.dense_fwd(x, w, b, True, unit)), "fwd")
    d = xo.density_for(N)
    dy = xo.dyadic((M, N), -4, 4, 1, g, dev, density=d, dtype=F32)
    mask = xo.dyadic((M, Kd), -2, 2, 1, g, dev, dtype=F32)
    dx = _nan(M, Kd, dev=dev)
    K.f32_dense_dgrad(dy, w, dx, M, Kd, N, mask)
    _same(dx, xo.to_f32(xo.dense_dgrad(dy, w, mask, 3)), "dgrad")


def test_gemm256_f32_wgrad_bias_row_exact(dev, K):
    B, Din, Dout, cap = 5000, 3000, 1000, 8
    g = _gen(dev, B + Dout)
    x = xo.dyadic((B, Din), -4, 4, 1, g, dev, density=0.5, dtype=F32)
    dy = xo.dyadic((B, Dout), -4, 4, 2, g, dev, density=0.5, dtype=F32)
    assert 1 <= K.f32_wgrad_splits_cap(Din, Dout, B) < cap
    slab = _nan(cap * (Din + 1) * Dout, dev=dev)
    S = K.f32_dense_wgrad(x, dy, slab, B, Din, Dout, cap)
    assert S == K.f32_wgrad_splits_cap(Din, Dout, B)
    tot = slab.view(cap, Din + 1, Dout)[:S].sum(0)
    rw, rb = xo.dense_wgrad(x, dy, 3, 2)
    _same(tot[:Din], xo.to_f32(rw), "dw")
    _same(tot[Din], xo.to_f32(rb), "db")


# ================================================================== implicit-GEMM conv
def _conv_inputs(dev, N, H, W, Ci, Co, k, e, seed, dtype=BF):
    g = _gen(dev, seed)
    d = xo.density_for(k * k * Ci)
    x = xo.dyadic((N, H, W, Ci), -4, 4, 1 + e, g, dev, density=d, dtype=dtype)
    w = xo.dyadic((k, k, Ci, Co), -4, 4, 2, g, dev, density=d, dtype=dtype)
    b = xo.dyadic((Co,), -64, 64, 3 + e, g, dev, dtype=F32)
    return g, x, w, b, 3 + e


CONV_E = [c + (0,) for c in CONV_CASES] + [CONV_CASES[3] + (4,)]


@pytest.mark.parametrize("N,H,W,Ci,Co,k,pad,e", CONV_E)
def test_conv_fwd_exact(dev, K, N, H, W, Ci, Co, k, pad, e):
    g, x, w, b, unit = _conv_inputs(dev, N, H, W, Ci, Co, k, e, 600 + Ci)
    for relu in (True, False):
        ref = xo.to_bf16(xo.conv_fwd(x, w, b, pad, relu, unit))
        out = _nan(*ref.shape, dev=dev, dtype=BF)
        Fk.conv2d(x, w, b, pad, relu=relu, out=out)
        _same(out, ref, relu)


@pytest.mark.parametrize("N,H,W,Ci,Co,k,pad,e", [c for c in CONV_E if c[3] % 8 == 0])
def test_conv_dgrad_exact(dev, K, N, H, W, Ci, Co, k, pad, e):
    g = _gen(dev, 700 + Ci)
    OH, OW = Fk.conv_out_hw(H, W, k, k, pad)
    d = xo.density_for(k * k * Co)
    dy = xo.dyadic((N, OH, OW, Co), -4, 4, 1 + e, g, dev, density=d)
    w = xo.dyadic((k, k, Ci, Co), -4, 4, 2, g, dev, density=d)
    mask = xo.dyadic((N, H, W, Ci), -2, 2, 1, g, dev)
    for m in (None, mask):
        out = _nan(N, H, W, Ci, dev=dev, dtype=BF)
        Fk.conv2d_dgrad(dy, w, (H, W), pad, mask=m, out=out)
        _same(out, xo.to_bf16(xo.conv_dgrad(dy, w, (H, W), pad, m, 3 + e)), m is not None)


def _conv_wgrad(K, x, dy, k, pad, cin, cout, splits):
    N, H, W, C = x.shape
    _, OH, OW, CO = dy.shape
    ph, pw = Fk.conv_pads(k, k, pad)
    M, P = k * k * C + 1, N * OH * OW
    S = Fk.pick_splits(M, CO, P) if splits is None else Fk.eff_splits(P, splits)
    slab = _nan(S * M * CO, dev=x.device)
    S = K.conv_wgrad(x, dy, slab, N, H, W, C, OH, OW, k, k, ph, pw, CO, True, S)
    dw = _nan(k, k, cin, cout, dev=x.device)
    db = _nan(cout, dev=x.device)
    K.splitk_reduce(slab, S, M, CO, k * k, C, cin, cout, k * k * C, dw, db, 1.0)
    return dw, db


@pytest.mark.parametrize("N,H,W,Ci,Co,k,pad,e", CONV_E)
@pytest.mark.parametrize("splits", [None, 1])
def test_conv_wgrad_exact(dev, K, N, H, W, Ci, Co, k, pad, e, splits):
    g = _gen(dev, 800 + Ci)
    OH, OW = Fk.conv_out_hw(H, W, k, k, pad)
    x = xo.dyadic((N, H, W, Ci), -4, 4, 1 + e, g, dev)
    dy = xo.dyadic((N, OH, OW, Co), -4, 4, 2, g, dev, density=0.5)
    ci_real = Ci - 2 if Ci == 8 else Ci          # padded-channel unpadding
    co_real = Co - 2 if Co == 8 else Co
    rw, rb = xo.conv_wgrad(x, dy, k, k, pad, 3 + e, 2)
    dw, db = _conv_wgrad(K, x, dy, k, pad, ci_real, co_real, splits)
    _same(dw, xo.to_f32(rw[:, :, :ci_real, :co_real]), "dw")
    _same(db, xo.to_f32(rb[:co_real]), "db")


# ================================================================== conv_halo.hip
@pytest.mark.parametrize("cap", [0, 2])
@pytest.mark.parametrize("v", range(10))
def test_conv_halo_variants_exact(dev, K, grid_cap, v, cap):
    """all ten (fv, dv) launch variants at the reference conv2 geometry: N = 5 (a partial image
    group), and N = 25 on 2 persistent blocks (every block loops, the next group prefetched):
    forward + bias + ReLU and the masked data gradient"""
    N, H, W, Ci, Co, k, pad = 5, 14, 14, 32, 64, 5, "SAME"
    if cap:
        grid_cap(cap)
        N = 25
    g, x, w, b, unit = _conv_inputs(dev, N, H, W, Ci, Co, k, 0, 900 + cap)
    d = xo.density_for(k * k * Co)
    dy = xo.dyadic((N, H, W, Co), -4, 4, 1, g, dev, density=d)
    wd = xo.dyadic((k, k, Ci, Co), -4, 4, 2, g, dev, density=d)
    mask = xo.dyadic((N, H, W, Ci), -2, 2, 1, g, dev)
    ref_y = xo.to_bf16(xo.conv_fwd(x, w, b, pad, True, unit))
    ref_dx = xo.to_bf16(xo.conv_dgrad(dy, wd, (H, W), pad, mask, 3))
    K.set_halo_variants(v, v)
    try:
        y = _nan(N, H, W, Co, dev=dev, dtype=BF)
        Fk.conv2d(x, w, b, pad, relu=True, out=y)
        dx = _nan(N, H, W, Ci, dev=dev, dtype=BF)
        Fk.conv2d_dgrad(dy, wd, (H, W), pad, mask=mask, out=dx)
    finally:
        K.set_halo_variants(-1, -1)
    _same(y, ref_y, "fwd")
    _same(dx, ref_dx, "dgrad")


@pytest.mark.parametrize("N,cap,e", [(5, 0, 0), (25, 2, 0), (5, 0, 4)])
def test_conv_halo_geometry_wgrad_exact(dev, K, grid_cap, N, cap, e):
    grid_cap(cap)
    g = _gen(dev, 950 + N)
    x = xo.dyadic((N, 14, 14, 32), -4, 4, 1 + e, g, dev)
    dy = xo.dyadic((N, 14, 14, 64), -4, 4, 2, g, dev, density=0.5)
    rw, rb = xo.conv_wgrad(x, dy, 5, 5, "SAME", 3 + e, 2)
    for splits in (None, 1):
        dw, db = _conv_wgrad(K, x, dy, 5, "SAME", 32, 64, splits)
        _same(dw, xo.to_f32(rw), "dw")
        _same(db, xo.to_f32(rb), "db")


# ================================================================== convpool.hip
def _cp_inputs(dev, N, H, W, Ci, ci, Co, co, e, seed):
    g = _gen(dev, seed)
    x = xo.dyadic((N, H, W, Ci), -8, 8, 4 + e, g, dev, density=0.5 if Ci < 8 else 0.3)
    x[..., ci:] = 0
    w = xo.dyadic((5, 5, Ci, Co), -3, 3, 2, g, dev)
    w[:, :, ci:, :] = 0
    w[..., co:] = 0
    b = xo.dyadic((co,), -32, 32, 6 + e, g, dev, dtype=F32)
    return g, x, w, b, 6 + e


def _unpack(arg, ab, Co):
    return arg if ab == Co else xo.unpack_codes(arg)


CP_E = [c + (0,) for c in CP_CASES] + [CP_CASES[1] + (4,)]


@pytest.mark.parametrize("cap", [0, 2])
@pytest.mark.parametrize("N,H,W,Ci,ci,Co,co,pad,e", CP_E)
def test_convpool_exact(dev, K, grid_cap, N, H, W, Ci, ci, Co, co, pad, e, cap):
    """forward (values and codes), weight gradient and -- where the geometry has one -- the
    data gradient; cap: 3x the batch on 2 persistent blocks"""
    if cap:
        grid_cap(cap)
        N *= 3
    padding = "SAME" if pad else "VALID"
    g, x, w, b, unit = _cp_inputs(dev, N, H, W, Ci, ci, Co, co, e, 1000 + Ci + Co)
    o, codes = xo.convpool_fwd(x, w, b, padding, "mantissa", unit)
    PH, PW = o.shape[1], o.shape[2]
    pooled = _nan(N, PH, PW, Co, dev=dev, dtype=BF)
    ab = K.convpool_arg_bytes(Ci, Co, 5, pad, H, W)
    arg = torch.full((N, PH, PW, ab), 0xEE, dtype=torch.uint8, device=dev)
    K.convpool_fwd(x, w, b, co, pooled, arg, N, Ci, Co, 5, pad, H, W)
    _same(pooled, xo.to_bf16(o), "pooled")
    _same(_unpack(arg, ab, Co), codes, "codes")
    # backward from the oracle's codes (the kernels' own input format)
    arg_ref = codes if ab == Co else xo.pack_codes(codes)
    dP = xo.dyadic((N, PH, PW, Co), -4, 4, 3, g, dev, density=0.5)
    dY = xo.unpool(dP, codes)
    rw, rb = xo.conv_wgrad(x, dY, 5, 5, padding, 4 + e + 3, 3)      # x 2**-(4+e) * dP 2**-3
    KM = K.convpool_rows(Ci, Co, 5, pad, H, W)
    grid = cap or 37
    slab = _nan(grid * KM * Co, dev=dev)
    K.convpool_wgrad(x, dP, arg_ref, slab, grid, N, Ci, Co, 5, pad, H, W)
    dw = _nan(5, 5, ci, co, dev=dev)
    db = _nan(co, dev=dev)
    G, Ip, I, brow = K.convpool_reduce_args(Ci, Co, 5, pad, H, W, ci)
    K.splitk_reduce(slab, grid, KM, Co, G, Ip, I, co, brow, dw, db, 1.0)
    _same(dw, xo.to_f32(rw[:, :, :ci, :co]), "dw")
    _same(db, xo.to_f32(rb[:co]), "db")
    if K.convpool_has_dgrad(Ci, Co, 5, pad, H, W):
        dx = _nan(N, H, W, Ci, dev=dev, dtype=BF)
        K.convpool_dgrad(dP, arg_ref, w, dx, N, Ci, Co, 5, pad, H, W)
        ref = xo.to_bf16(xo.conv_dgrad(dY, w, (H, W), padding, None, 5))
        _same(dx[..., :ci], ref[..., :ci], "dx")


def _fold_inputs(dev, B, cin, e, seed, n=None):
    """the LRN-backward folds at lrn_alpha = 0, lrn_bias = 1: dyadic images (n of them: a
    resident set) and dL/d norm1, any finite pool1, codes uniform in 0..4"""
    g = _gen(dev, seed)
    x = xo.dyadic((n or B, 28, 28, cin), -8, 8, 4 + e, g, dev, density=0.5)
    dn = xo.dyadic((B, 14, 14, 32), -4, 4, 3, g, dev, density=0.5)
    p1 = torch.randn(B, 14, 14, 32, generator=g, device=dev) * 3.0
    p1 = (p1 * torch.exp2(torch.randint(-8, 9, p1.shape, generator=g, device=dev).float())).to(BF)
    codes = torch.randint(0, 5, (B, 14, 14, 32), generator=g, device=dev, dtype=torch.uint8)
    return x, dn, p1, codes


def _lrn_identity(K, p1, dn):
    """the precondition of the fold tests, on the standalone kernel: with alpha = 0 and bias =
    1 lrn_math.h's backward is sc = fma(0, s, 1) = 1, k = 0, d = fma(g, pw, -0), and the
    bf16 rounding returns the bf16 g even if pw is an ulp off 1"""
    P = dn.numel() // 32
    assert bool(torch.isfinite(p1.float()).all())
    for beta in (0.75, 0.5):
        dx = _nan(P, 32, dev=dn.device, dtype=BF)
        K.lrn_bwd(p1.view(P, 32), dn.view(P, 32), dx, P, 32, 4, 1.0, 0.0, beta, False)
        _same(dx, dn.view(P, 32), ("lrn_bwd at alpha 0", beta))


def _fold_reduce(K, slab, grid, cin, dev):
    G, Ip, I, brow = K.convpool_reduce_args(cin, 32, 5, 2, 28, 28, cin)
    dw = _nan(5, 5, cin, 32, dev=dev)
    db = _nan(32, dev=dev)
    K.splitk_reduce(slab, grid, K.convpool_rows(cin, 32, 5, 2, 28, 28), 32, G, Ip, I, 32, brow, dw, db, 1.0)
    return dw, db


@pytest.mark.parametrize("cin", [1, 3], ids=["cin1", "cin3"])
@pytest.mark.parametrize("beta", [0.75, 0.5])
@pytest.mark.parametrize("B,grid", [(5, 2), (77, 37)])
def test_convpool_lrn_fold_exact(dev, K, B, grid, beta, cin):
    """convpool_wgrad_k<..., LRNB> (beta 0.75: LRNB 2, else 1) with the LRN made the identity:
    everything but the LRN math -- staging, un-pooling, the GEMM, the split-K slabs"""
    x, dn, p1, codes = _fold_inputs(dev, B, cin, 0, 1050 + B + cin)
    _lrn_identity(K, p1, dn)
    rw, rb = xo.conv_wgrad(x, xo.unpool(dn, codes), 5, 5, "SAME", 7, 3)
    KM = K.convpool_rows(cin, 32, 5, 2, 28, 28)
    slab = _nan(grid * KM * 32, dev=dev)
    K.convpool_wgrad(x, dn, codes, slab, grid, B, cin, 32, 5, 2, 28, 28, lrn_p=p1, lrn_bias=1.0, lrn_alpha=0.0,
                     lrn_beta=beta, lrn_r=4)
    dw, db = _fold_reduce(K, slab, grid, cin, dev)
    _same(dw, xo.to_f32(rw), "dw")
    _same(db, xo.to_f32(rb), "db")


# ================================================================== lenet_band.hip
def _lenet(dev, B, e=0):
    (x, w1, b1, w2, b2, dP2), fu, bu = xo.lenet_inputs(B, 1100 + B, dev, e)
    P1, c1, P2, c2 = xo.lenet_fwd(x, w1, b1, w2, b2, "mantissa", fu)
    return x, w1, b1, w2, b2, dP2, P1, c1, P2, c2, bu


@pytest.mark.parametrize("B,cap,e", [(1, 0, 0), (17, 0, 0), (333, 3, 0), (17, 0, 4)])
def test_lenet_band_fwd_exact(dev, K, grid_cap, B, cap, e):
    """P1, A1, P2, A2 and the combined pool1 records against the oracle; the codes bitwise
    those of the per-layer convpool kernels (no allowance for near-ties: there are none)"""
    grid_cap(cap)
    x, w1, b1, w2, b2, dP2, P1, c1, P2, c2, _ = _lenet(dev, B, e)
    Q1, A1, Q2, A2 = _band(K, x, w1, b1, w2, b2, B)
    _same(Q1, P1, "P1")
    _same(xo.unpack_codes(A1), c1, "A1")
    _same(Q2, P2, "P2")
    _same(A2, c2, "A2")
    # p1 without arg1: one 16-byte record per pool1 window (what lenet_bwd reads)
    R = torch.full((B, 14, 14, 8), 7.0, dtype=BF, device=dev)
    S2 = _nan(B, 5, 5, 16, dev=dev, dtype=BF)
    C2 = torch.full((B, 5, 5, 16), 0xEE, dtype=torch.uint8, device=dev)
    K.lenet_band_fwd(x, w1, b1, 6, w2, b2, B, S2, C2, p1=R)
    assert torch.equal(R.view(torch.uint8), _combined(P1, xo.pack_codes(c1)).view(torch.uint8))
    _same(S2, P2, "P2 (records)")
    _same(C2, c2, "A2 (records)")
    # the per-layer kernels
    T1 = _nan(B, 14, 14, 8, dev=dev, dtype=BF)
    D1 = torch.full((B, 14, 14, 4), 0xEE, dtype=torch.uint8, device=dev)
    K.convpool_fwd(x, w1, b1, 6, T1, D1, B, 1, 8, 5, 2, 28, 28)
    T2 = _nan(B, 5, 5, 16, dev=dev, dtype=BF)
    D2 = torch.full((B, 5, 5, 16), 0xEE, dtype=torch.uint8, device=dev)
    K.convpool_fwd(Q1, w2, b2, 16, T2, D2, B, 8, 16, 5, 0, 14, 14)
    _same(T1, Q1, "convpool P1")
    _same(D1, A1, "convpool A1")
    _same(T2, Q2, "convpool P2")
    _same(D2, A2, "convpool A2")


# ================================================================== lenet_bwd.hip
@pytest.mark.parametrize("B,cap,e", [(1, 0, 0), (13, 0, 0), (77, 2, 0), (200, 3, 0), (13, 0, 4)])
def test_lenet_bwd_exact(dev, K, grid_cap, B, cap, e):
    """all four gradients; the kernel reads the oracle's pool1 records and codes, so this
    does not depend on the forward kernel"""
    grid_cap(cap)
    x, w1, b1, w2, b2, dP2, P1, c1, P2, c2, bu = _lenet(dev, B, e)
    want = xo.lenet_bwd(x, P1, c1, c2, dP2, w2, bu)
    got = _fused(K, x, P1, xo.pack_codes(c1), c2, dP2, w2, B)
    if cap:
        assert got[4] == min(cap, (B + 7) // 8)
    for name, gk, wk in zip(("dW1", "db1", "dW2", "db2"), got[:4], want):
        _same(gk, xo.to_f32(wk), name)


# ================================================================== refc1_wgrad.hip
# (B, grid cap, extra shift, through idx): every path of the 2-image tile pipeline -- half a
# tile; one tile; a partial last tile; one block over three tiles (both LDS buffers reused,
# accumulators carried); two blocks over four tiles; 39 tiles uncapped; a resident set read
# through repeated, out-of-order rows; the inputs scaled by 2**-4
REFC1 = [(1, 0, 0, False), (2, 0, 0, False), (3, 0, 0, False), (5, 1, 0, False), (7, 2, 0, False), (77, 0, 0, False),
         (7, 2, 0, True), (5, 1, 4, False)]


@pytest.mark.parametrize("cin", [1, 3], ids=["cin1", "cin3"])
@pytest.mark.parametrize("B,cap,e,idx", REFC1)
def test_refc1_wgrad_exact(dev, K, grid_cap, B, cap, e, idx, cin):
    """refc1_wgrad_k with the LRN made the identity (alpha 0, bias 1): the pool-window-phase
    GEMM of unpool(dn, codes) against x, the bias row and the slab layout, bit for bit.  The
    uint8 input mode is not dyadic after its normalisation and stays with
    test_refc1_wgrad_gpu.test_refc1_wgrad_gathered_input."""
    grid_cap(cap)
    n = 11 if idx else None
    xs, dn, p1, codes = _fold_inputs(dev, B, cin, e, 1900 + 10 * B + cin + e, n=n)
    _lrn_identity(K, p1, dn)
    rows = torch.tensor([9, 2, 2, 0, 10, 5, 2], device=dev) if idx else None
    x = xs[rows] if idx else xs
    rw, rb = xo.conv_wgrad(x, xo.unpool(dn, codes), 5, 5, "SAME", 7 + e, 3)
    grid = K.refc1_wgrad_blocks(B)
    assert grid == min(cap or grid, (B + 1) // 2)
    slab = _nan(grid * (48 if cin == 1 else 80) * 32, dev=dev)
    src = dict(idx=rows) if idx else {}
    K.refc1_wgrad(xs.view(-1, 784 * cin) if idx else xs, dn, p1, codes, slab, grid, B, 1.0, 0.0, 0.75, cin=cin, **src)
    dw, db = _fold_reduce(K, slab, grid, cin, dev)
    _same(dw, xo.to_f32(rw), "dw")
    _same(db, xo.to_f32(rb), "db")


# ================================================================== refc1n_fwd_k / refc1n3_fwd_k
@pytest.mark.parametrize("cin,e", [(1, 0), (3, 0), (1, 4)])
def test_refc1n_pool1_exact(dev, K, grid_cap, cin, e):
    """pool1 and codes of the reference conv1 forward (norm1 is not exact and stays with its
    own oracle), B = 77 on 3 persistent blocks, with and without norm1 written"""
    grid_cap(3)
    B = 77
    g = _gen(dev, 1200 + cin)
    x = xo.dyadic((B, 28, 28, cin), -8, 8, 4 + e, g, dev, density=0.5)
    w = xo.dyadic((5, 5, cin, 32), -3, 3, 2, g, dev)
    b = xo.dyadic((32,), -32, 32, 6 + e, g, dev, dtype=F32)
    o, codes = xo.convpool_fwd(x, w, b, "SAME", "mantissa", 6 + e)
    for with_norm in (False, True):
        P1 = _nan(B, 14, 14, 32, dev=dev, dtype=BF)
        A1 = torch.full((B, 14, 14, 32), 0xEE, dtype=torch.uint8, device=dev)
        kw = {}
        if with_norm:
            kw = dict(lrn_out=torch.zeros(B, 14, 14, 32, dtype=BF, device=dev), lrn_bias=1.0,
                      lrn_alpha=0.001 / 9.0, lrn_beta=0.75, lrn_r=4)
        K.convpool_fwd(x, w, b, 32, P1, A1, B, cin, 32, 5, 2, 28, 28, **kw)
        _same(P1, xo.to_bf16(o), ("pool1", with_norm))
        _same(A1, codes, ("codes", with_norm))


# ================================================================== bf16 max-pool
@pytest.mark.parametrize("N,H,W,C,e", [(4, 28, 28, 8, 0), (3, 14, 14, 64, 0), (2, 7, 7, 16, 0), (5, 10, 10, 16, 0),
                                       (2, 7, 7, 16, 4)])
def test_maxpool_exact(dev, K, N, H, W, C, e):
    """values, codes (ReLU zeros and repeated small integers tie all the time: pool_lrn.hip
    maxpool_fwd_k scans positions 0..3 with a strict `>`, so the first maximum wins) and the
    backward with and without the ReLU mask; 7 x 7 pools its last row / column alone"""
    g = _gen(dev, 1300 + H)
    x = xo.dyadic((N, H, W, C), -6, 6, 2 + e, g, dev).relu()
    OH, OW = (H + 1) // 2, (W + 1) // 2
    ry, rarg = xo.maxpool2x2(x, "first")
    y = _nan(N, OH, OW, C, dev=dev, dtype=BF)
    arg = torch.full((N, OH, OW, C), 0xEE, dtype=torch.uint8, device=dev)
    Fk.maxpool2x2(x, out=y, arg=arg)
    _same(y, xo.to_bf16(ry), "y")
    _same(arg, rarg, "arg")
    dy = xo.dyadic((N, OH, OW, C), -4, 4, 1, g, dev)
    for relu_mask in (True, False):
        dx = _nan(N, H, W, C, dev=dev, dtype=BF)
        Fk.maxpool2x2_bwd(dy, rarg, y, (H, W), relu_mask=relu_mask, out=dx)
        gy = torch.where(ry > 0, dy.double(), torch.zeros_like(ry)) if relu_mask else dy.double()
        _same(dx, xo.to_bf16(xo.unpool(gy, rarg, (H, W))), relu_mask)


# ================================================================== fp32 path (f32.hip, conv_halo_f32.hip, conv1_f32.hip)
@pytest.mark.parametrize("M,N,Kk,relu,e", [(77, 10, 192, False, 0), (5, 130, 33, True, 0), (77, 10, 192, True, 4)])
def test_f32_dense_exact(dev, K, M, N, Kk, relu, e):
    g, x, w, b, unit = _dense_inputs(dev, M, N, Kk, e, 1400 + M, dtype=F32)
    y = _nan(M, N, dev=dev)
    K.f32_dense_fwd(x, w, y, M, N, Kk, N, b, relu)
    _same(y, xo.to_f32(xo.dense_fwd(x, w, b, relu, unit)), "fwd")
    dy = xo.dyadic((M, N), -4, 4, 1, g, dev, dtype=F32)
    mask = xo.dyadic((M, Kk), -2, 2, 1, g, dev, dtype=F32)
    dx = _nan(M, Kk, dev=dev)
    K.f32_dense_dgrad(dy, w, dx, M, Kk, N, mask)
    _same(dx, xo.to_f32(xo.dense_dgrad(dy, w, mask, 3)), "dgrad")
    rw, rb = xo.dense_wgrad(x, dy, 2 + e, 1)
    for S in (1, 3):
        slab = _nan(S * (Kk + 1) * N, dev=dev)
        K.f32_dense_wgrad(x, dy, slab, M, Kk, N, S)
        tot = slab.view(S, Kk + 1, N).sum(0)
        _same(tot[:Kk], xo.to_f32(rw), ("dw", S))
        _same(tot[Kk], xo.to_f32(rb), ("db", S))


@pytest.mark.parametrize("Nb,H,Ci,Co,k,pad,e", [(3, 28, 3, 32, 5, "SAME", 0), (5, 14, 6, 16, 5, "VALID", 0),
                                                 (1, 9, 1, 8, 3, "SAME", 0), (5, 14, 6, 16, 5, "VALID", 4)])
def test_f32_conv_exact(dev, K, Nb, H, Ci, Co, k, pad, e):
    g, x, w, b, unit = _conv_inputs(dev, Nb, H, H, Ci, Co, k, e, 1500 + Ci, dtype=F32)
    p = (k - 1) // 2 if pad == "SAME" else 0
    OH = H if pad == "SAME" else H - k + 1
    y = _nan(Nb, OH, OH, Co, dev=dev)
    K.f32_conv_fwd(x, w, y, Nb, H, H, Ci, OH, OH, k, k, p, p, Co, b, False)
    _same(y, xo.to_f32(xo.conv_fwd(x, w, b, pad, False, unit)), "fwd")
    dy = xo.dyadic((Nb, OH, OH, Co), -4, 4, 1, g, dev, density=0.5, dtype=F32)
    dx = _nan(Nb, H, H, Ci, dev=dev)
    K.f32_conv_dgrad(dy, w, dx, Nb, OH, OH, Co, H, H, k, k, p, p, Ci, None)
    _same(dx, xo.to_f32(xo.conv_dgrad(dy, w, (H, H), pad, None, 3)), "dgrad")
    M = k * k * Ci + 1
    rw, rb = xo.conv_wgrad(x, dy, k, k, pad, 2 + e, 1)
    for S in (1, 4):
        slab = _nan(S * M * Co, dev=dev)
        K.f32_conv_wgrad(x, dy, slab, Nb, H, H, Ci, OH, OH, k, k, p, p, Co, S)
        tot = slab.view(S, M, Co).sum(0)
        _same(tot[:-1].view(k, k, Ci, Co), xo.to_f32(rw), ("dw", S))
        _same(tot[-1], xo.to_f32(rb), ("db", S))


@pytest.mark.parametrize("fv", [0, 1])
def test_f32_halo_conv2_exact(dev, K, grid_cap, fv):
    """conv_halo_f32.hip, Nb = 37 on 3 persistent blocks: forward + bias + ReLU and the dgrad
    of a 64-channel dY with the input-ReLU mask"""
    grid_cap(3)
    Nb, Co = 37, 64
    g, x, w, b, unit = _conv_inputs(dev, Nb, 14, 14, 32, Co, 5, 0, 1600 + fv, dtype=F32)
    d = xo.density_for(25 * 64)
    w2 = xo.dyadic((5, 5, 32, 64), -4, 4, 2, g, dev, density=d, dtype=F32)
    dy = xo.dyadic((Nb, 14, 14, 64), -4, 4, 1, g, dev, density=d, dtype=F32)
    xm = xo.dyadic((Nb, 14, 14, 32), -2, 2, 1, g, dev, dtype=F32)
    K.set_f32_halo_fwd_variant(fv)
    try:
        y = _nan(Nb, 14, 14, Co, dev=dev)
        K.f32_conv_fwd(x, w, y, Nb, 14, 14, 32, 14, 14, 5, 5, 2, 2, Co, b, True)
        dx = _nan(Nb, 14, 14, 32, dev=dev)
        K.f32_conv_dgrad(dy, w2, dx, Nb, 14, 14, 64, 14, 14, 5, 5, 2, 2, 32, xm)
    finally:
        K.set_f32_halo_fwd_variant(0)
    _same(y, xo.to_f32(xo.conv_fwd(x, w, b, "SAME", True, unit)), "fwd")
    _same(dx, xo.to_f32(xo.conv_dgrad(dy, w2, (14, 14), "SAME", xm, 3)), "dgrad")


def test_f32_conv1_pool_kernels_exact(dev, K, grid_cap):
    """conv1_f32.hip fused with pool1, Nb = 300, 5 persistent blocks: f32_conv1_fwd_pool
    (bias + ReLU, then the first maximum: conv1_f32_fwd_pool_k's strict `>` scan; code 4 where
    the maximum is 0 -- the same values and codes as pooling the raw sums first) and
    f32_conv1_wgrad_unpool over S = 7 partials"""
    grid_cap(5)
    Nb, S = 300, 7
    g = _gen(dev, 1700)
    x = xo.dyadic((Nb, 28, 28, 1), -8, 8, 4, g, dev, density=0.5, dtype=F32)
    w = xo.dyadic((5, 5, 1, 32), -3, 3, 2, g, dev, dtype=F32)
    b = xo.dyadic((32,), -32, 32, 6, g, dev, dtype=F32)
    o, codes = xo.convpool_fwd(x, w, b, "SAME", "first", 6)
    y = _nan(Nb, 14, 14, 32, dev=dev)
    arg = torch.full((Nb, 14, 14, 32), 0xEE, dtype=torch.uint8, device=dev)
    K.f32_conv1_fwd_pool(x, w, b, y, arg, Nb)
    _same(y, xo.to_f32(o), "pool1")
    _same(arg, codes, "codes")
    dp = xo.dyadic((Nb, 14, 14, 32), -4, 4, 3, g, dev, density=0.5, dtype=F32)
    rw, rb = xo.conv_wgrad(x, xo.unpool(dp, codes), 5, 5, "SAME", 7, 3)
    slab = _nan(S * 26 * 32, dev=dev)
    K.f32_conv1_wgrad_unpool(x, dp, codes, slab, Nb, S)
    tot = slab.view(S, 26, 32).sum(0)
    _same(tot[:25].view(5, 5, 1, 32), xo.to_f32(rw), "dw")
    _same(tot[25], xo.to_f32(rb), "db")


def test_f32_maxpool_exact(dev, K):
    g = _gen(dev, 1800)
    x = xo.dyadic((3, 14, 14, 64), -6, 6, 2, g, dev, dtype=F32).relu()
    ry, rarg = xo.maxpool2x2(x, "first")
    y = _nan(3, 7, 7, 64, dev=dev)
    arg = torch.full((3, 7, 7, 64), 0xEE, dtype=torch.uint8, device=dev)
    K.f32_maxpool_fwd(x, y, arg, 3, 14, 14, 64)
    _same(y, xo.to_f32(ry), "y")
    _same(arg, rarg, "arg")
    dy = xo.dyadic((3, 7, 7, 64), -4, 4, 1, g, dev, dtype=F32)
    for relu_mask in (False, True):
        dx = _nan(3, 14, 14, 64, dev=dev)
        K.f32_maxpool_bwd(dy, rarg, y, relu_mask, dx, 3, 14, 14, 64)
        gy = torch.where(ry > 0, dy.double(), torch.zeros_like(ry)) if relu_mask else dy.double()
        _same(dx, xo.to_f32(xo.unpool(gy, rarg)), relu_mask)
