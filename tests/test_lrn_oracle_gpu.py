"""Every standalone LRN kernel against the float64 oracle (tests/lrn_oracle.py), element by
element: |out - ref| <= half a bf16 ulp (bf16 kernels) + c 2**-23 A with A the scale of the
element's own terms, and exactly 0 where every term is 0.  `within_budget` and `torch.equal`
are the only comparisons; the reference runs in float64 on the device.  The constants c and
the inputs' domain are measured and pinned on the CPU (tests/test_lrn_oracle_cpu.py).

These kernels are the root of a chain of bitwise tests, which stay as they are:
  lrn_fwd_k / lrn_bwd_k (here)
    == lrn_pool_fwd_k / lrn_pool_bwd_k        test_kernels_gpu.test_lrn_pool_matches_two_step
       == lrn_pool14_fwd_k / lrn_pool14_bwd_k test_kernels_gpu.test_lrn_pool_packed
    == the refc1n* norm1 epilogue             test_refc1_fwd_gpu
  the refc1_wgrad and convpool LRN-backward folds are not in that chain (their dP1 never
  leaves LDS): test_refc1_oracle_gpu holds them to this oracle through probe inputs
  lrn_f32_*_v4_k (here)
    == lrn_pool_f32_*_k, conv1_f32_wgrad_lrn_k           test_f32_gpu
The fused LRN -> pool kernels are also held to the oracle directly here, pooled values,
argmax codes and the gradient through the kernel's own codes.
"""
import pytest
import torch

import lrn_oracle as lo

pytestmark = pytest.mark.gpu

def _check(out, ref, A, c, bf16, what):
    ok, report = lo.within_budget(out, ref, A, c, bf16)
    print(f"{what}: {lo.units(out, ref, A, bf16):.1f} units of 2**-23 A" + (" past the bf16 half-ulp" if bf16 else ""))
    assert ok, f"{what}: {report}"


def _standalone(K, x, g, r, bias, alpha, beta, mask, what, f32=False):
    """one forward + backward launch on [P, C] inputs, both held to the budget"""
    P, C = x.shape
    fwd, bwd, c = (K.f32_lrn_fwd, K.f32_lrn_bwd, lo.C_F32) if f32 else (K.lrn_fwd, K.lrn_bwd, lo.C_BF16)
    y = torch.full_like(x, 3.0)
    dx = torch.full_like(x, 5.0)
    fwd(x, y, P, C, r, bias, alpha, beta)
    bwd(x, g, dx, P, C, r, bias, alpha, beta, mask)
    yr, dxr, Ay, Adx = lo.lrn_ref(x, g, r, bias, alpha, beta, mask)
    _check(y, yr, Ay, c, not f32, f"{what} forward")
    _check(dx, dxr, Adx, c, not f32, f"{what} backward")


# ------------------------------------------------------------------ bf16 standalone kernels
@pytest.mark.parametrize("alpha", lo.ALPHAS)
@pytest.mark.parametrize("beta", lo.BETAS)
@pytest.mark.parametrize("C,r", lo.LRN_ALL)
def test_lrn_bf16(dev, K, C, r, beta, alpha):
    """Every (C, r) instantiation; beta 0.75 takes lrn_bwd_k<32|64, 4, true>, the others the
    <., ., false> ones; spike probes, post-ReLU and signed random tensors, all-zero pixels."""
    for bias in lo.BIASES:
        for mask in (True, False):
            for name, (x, g) in lo.standalone_inputs(C, alpha, mask).items():
                _standalone(K, x.to(dev), g.to(dev), r, bias, alpha, beta, mask,
                            f"{name} C {C} r {r} beta {beta} bias {bias} alpha {alpha:.3g} mask {mask}")


@pytest.mark.parametrize("C,r", lo.LRN_ALL)
def test_lrn_bf16_wide_range(dev, K, C, r):
    """One 128 among values near 0.25, at the model's constants (inside the running sum's
    domain; at alpha = 0.05 it is outside, test_lrn_oracle_cpu)."""
    x, g = lo.wide_inputs(C)
    for mask in (True, False):
        _standalone(K, x.to(dev), g.to(dev), r, 1.0, lo.REF_ALPHA, 0.75, mask, f"wide C {C} r {r} mask {mask}")


def test_lrn_bf16_grid_stride(dev, K):
    """P just past 16384 blocks x 256 lanes / 8 lanes per pixel: a second grid-stride trip."""
    C, r, P = lo.GRID_C, lo.GRID_R, lo.GRID_P
    assert P * (C // 8) > 16384 * 256
    xt, gt = (t.to(dev) for t in lo.grid_tile())
    x, g = lo.tile_to(xt, P), lo.tile_to(gt, P)
    y = torch.full_like(x, 3.0)
    dx = torch.full_like(x, 5.0)
    K.lrn_fwd(x, y, P, C, r, 1.0, lo.BIG_ALPHA, 0.75)
    K.lrn_bwd(x, g, dx, P, C, r, 1.0, lo.BIG_ALPHA, 0.75, True)
    yr, dxr, Ay, Adx = (lo.tile_to(t, P) for t in lo.lrn_ref(xt, gt, r, 1.0, lo.BIG_ALPHA, 0.75, True))
    _check(y, yr, Ay, lo.C_BF16, True, "grid-stride forward")
    _check(dx, dxr, Adx, lo.C_BF16, True, "grid-stride backward")


# ------------------------------------------------------------------ LRN -> pool
def _pool(K, dev, N, H, W, C, relu, f32):
    x, dP = (t.to(dev) for t in lo.pool_inputs(N, H, W, C, relu))
    if f32:
        x, dP = x.float(), dP.float()
    c, r, bias = (lo.C_F32 if f32 else lo.C_BF16), lo.POOL_R, lo.POOL_BIAS
    for alpha in lo.ALPHAS:
        for beta in lo.POOL_BETAS:
            what = f"{'f32 ' if f32 else ''}pool {N}x{H}x{W}x{C} relu {relu} alpha {alpha:.3g} beta {beta}"
            y = torch.full((N, H // 2, W // 2, C), 3.0, dtype=x.dtype, device=dev)
            arg = torch.full((N, H // 2, W // 2, C), 9, dtype=torch.uint8, device=dev)
            dx = torch.full_like(x, 5.0)
            if f32:
                K.f32_lrn_pool_fwd(x, y, arg, N, H, W, C, r, bias, alpha, beta)
                K.f32_lrn_pool_bwd(x, dP, arg, dx, N, H, W, C, r, bias, alpha, beta, relu)
            else:
                K.lrn_pool_fwd(x, y, arg, N, H, W, C, r, bias, alpha, beta, nonneg=relu)
                K.lrn_pool_bwd(x, dP, arg, dx, N, H, W, C, r, bias, alpha, beta, relu)
            pooled, exact, A, codes, decided = lo.lrn_pool_ref(x, H, W, r, bias, alpha, beta, not f32)
            _check(y, exact, A, c, not f32, f"{what} pooled")
            # a condition on the inputs, from the reference alone
            undecided = 1.0 - decided.double().mean().item()
            assert undecided <= lo.MAX_UNDECIDED, f"{what}: {undecided:.4f} of the windows undecided"
            assert int(arg.max()) <= 3
            assert torch.equal(arg[decided], codes[decided]), f"{what}: codes"
            # the gradient through the kernel's own codes; the running kernels to the vector scale
            g = lo.unpool(dP, arg, H, W)
            _, dxr, _, Adx = lo.lrn_ref(x, g, r, bias, alpha, beta, relu, vector_scale=not f32)
            _check(dx, dxr, Adx, c, not f32, f"{what} backward")


@pytest.mark.parametrize("N,H,W,C", lo.POOL_CASES)
@pytest.mark.parametrize("relu", [True, False])
def test_lrn_pool_bf16(dev, K, N, H, W, C, relu):
    """lrn_pool_fwd_k / lrn_pool_bwd_k<., 4, true | false>; at 14 x 14 x 64 on a post-ReLU
    input the packed lrn_pool14 kernels (their backward at beta 0.75 only)."""
    _pool(K, dev, N, H, W, C, relu, f32=False)


def test_lrn_pool_bf16_generic_at_14x14x64(dev, K):
    K.lrn_set_packed(False)
    try:
        _pool(K, dev, *lo.POOL_CASES[0], True, f32=False)
    finally:
        K.lrn_set_packed(True)


@pytest.mark.parametrize("N,H,W,C", lo.POOL_CASES)
@pytest.mark.parametrize("relu", [True, False])
def test_lrn_pool_f32(dev, K, N, H, W, C, relu):
    _pool(K, dev, N, H, W, C, relu, f32=True)


# ------------------------------------------------------------------ fp32 standalone kernels
def _f32_cases(K, dev, C, r, place=lambda t: t):
    for alpha in lo.ALPHAS:
        for beta in lo.F32_BETAS:
            for mask in (True, False):
                for name, (x, g) in lo.f32_inputs(C, alpha, mask).items():
                    _standalone(K, place(x.to(dev)), place(g.to(dev)), r, 1.0, alpha, beta, mask,
                                f"f32 {name} C {C} r {r} beta {beta} alpha {alpha:.3g} mask {mask}", f32=True)


@pytest.mark.parametrize("C,r", lo.F32_V4)
def test_lrn_f32_vector(dev, K, C, r):
    """lrn_f32_fwd_v4_k / lrn_f32_bwd_v4_k: C 32 / 64, every radius 1..4."""
    _f32_cases(K, dev, C, r)


@pytest.mark.parametrize("C,r", lo.F32_SCALAR)
def test_lrn_f32_scalar(dev, K, C, r):
    """lrn_f32_fwd_k / lrn_f32_bwd_k: every other C (24 and 48 leave idle threads in a block),
    r = 5 at C = 32; 843 pixels is no multiple of 256 / C."""
    assert lo.F32_PIXELS % (256 // C) != 0
    _f32_cases(K, dev, C, r)


def test_lrn_f32_scalar_on_unaligned_pointers(dev, K):
    """a view one float into its buffer is not 16-byte aligned: C = 32, r = 4 on the scalar kernels"""
    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    def run(K2, x, g):
        P, C = x.shape
        y, dx = shifted(torch.full_like(x, 3.0)), shifted(torch.full_like(x, 5.0))
        K2.f32_lrn_fwd(x, y, P, C, 4, 1.0, lo.BIG_ALPHA, 0.75)
        K2.f32_lrn_bwd(x, g, dx, P, C, 4, 1.0, lo.BIG_ALPHA, 0.75, True)
        return y, dx

    for name, (x, g) in lo.f32_inputs(32, lo.BIG_ALPHA, True).items():
        x, g = shifted(x.to(dev)), shifted(g.to(dev))
        y, dx = run(K, x, g)
        yr, dxr, Ay, Adx = lo.lrn_ref(x, g, 4, 1.0, lo.BIG_ALPHA, 0.75, True)
        _check(y, yr, Ay, lo.C_F32, False, f"unaligned {name} forward")
        _check(dx, dxr, Adx, lo.C_F32, False, f"unaligned {name} backward")
