"""The exact oracle (tests/exact_oracle.py) checked on the CPU: it agrees with PyTorch's
float64 conv2d / max_pool2d / autograd, fp32 evaluation in any order gives the same bits
(which validates the magnitude condition), and three one-term errors that the suite's
tolerance predicates accept are rejected by bitwise equality."""
import pytest
import torch
import torch.nn.functional as F

import exact_oracle as xo

CPU = torch.device("cpu")


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# the tolerance predicates of the GPU tests, copied (test_kernels_gpu.close,
# test_lenet_bwd_gpu._rel)
def close(out, ref, rel=2e-2):
    out = out.float()
    ref = ref.float()
    tol = rel * ref.abs().max().item() + 1e-6
    err = (out - ref).abs().max().item()
    return err <= tol


def rel_norm(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _torch_conv(x, w, b, padding):
    kh, kw = w.shape[:2]
    xn = _nchw(x)
    if padding == "SAME":
        xn = F.pad(xn, ((kw - 1) // 2, kw // 2, (kh - 1) // 2, kh // 2))
    return F.conv2d(xn, w.double().permute(3, 2, 0, 1), None if b is None else b.double())


CASES = [(3, 28, 28, 1, 8, 5, "SAME"), (2, 14, 14, 8, 16, 5, "VALID"), (1, 7, 9, 16, 32, 3, "SAME"),
         (2, 14, 14, 32, 64, 5, "SAME")]


@pytest.mark.parametrize("N,H,W,Ci,Co,k,pad", CASES)
def test_conv_matches_torch_float64(N, H, W, Ci, Co, k, pad):
    g = _gen(1)
    x = xo.dyadic((N, H, W, Ci), -4, 4, 2, g, CPU)
    w = xo.dyadic((k, k, Ci, Co), -4, 4, 3, g, CPU)
    b = xo.dyadic((Co,), -8, 8, 5, g, CPU, dtype=torch.float32)
    xt = _nchw(x).requires_grad_(True)
    wt = w.double().permute(3, 2, 0, 1).requires_grad_(True)
    bt = b.double().requires_grad_(True)
    p = (k - 1) // 2 if pad == "SAME" else 0
    yt = F.conv2d(xt, wt, bt, padding=p)
    y = xo.conv_fwd(x, w, b, pad, relu=False, unit=5)
    assert torch.equal(y, yt.permute(0, 2, 3, 1))
    assert torch.equal(xo.conv_fwd(x, w, b, pad, relu=True, unit=5), yt.relu().permute(0, 2, 3, 1))
    dy = xo.dyadic(tuple(y.shape), -4, 4, 1, g, CPU)
    yt.backward(_nchw(dy))
    mask = xo.dyadic((N, H, W, Ci), -1, 1, 0, g, CPU)
    dx = xo.conv_dgrad(dy, w, (H, W), pad, unit=4)
    assert torch.equal(dx, xt.grad.permute(0, 2, 3, 1))
    dxm = xo.conv_dgrad(dy, w, (H, W), pad, mask=mask, unit=4)
    assert torch.equal(dxm, xt.grad.permute(0, 2, 3, 1) * (mask.double() > 0))
    dw, db = xo.conv_wgrad(x, dy, k, k, pad, unit=3)
    assert torch.equal(dw, wt.grad.permute(2, 3, 1, 0))
    assert torch.equal(db, bt.grad)


def test_dense_matches_torch_float64():
    g = _gen(2)
    x = xo.dyadic((37, 400), -4, 4, 1, g, CPU)
    w = xo.dyadic((400, 120), -4, 4, 2, g, CPU)
    b = xo.dyadic((100,), -8, 8, 3, g, CPU, dtype=torch.float32)     # 20 padded bias columns
    xt, wt = x.double().requires_grad_(True), w.double().requires_grad_(True)
    bt = torch.cat([b.double(), torch.zeros(20, dtype=torch.float64)])
    yt = xt @ wt + bt
    assert torch.equal(xo.dense_fwd(x, w, b, False, unit=3), yt)
    assert torch.equal(xo.dense_fwd(x, w, b, True, unit=3), yt.relu())
    dy = xo.dyadic((37, 120), -4, 4, 0, g, CPU)
    yt.backward(dy.double())
    mask = xo.dyadic((37, 400), -1, 1, 0, g, CPU)
    assert torch.equal(xo.dense_dgrad(dy, w, unit=2), xt.grad)
    assert torch.equal(xo.dense_dgrad(dy, w, mask, unit=2), xt.grad * (mask.double() > 0))
    dw, db = xo.dense_wgrad(x, dy, unit=1)
    assert torch.equal(dw, wt.grad) and torch.equal(db, dy.double().sum(0))


@pytest.mark.parametrize("H,W", [(14, 14), (7, 7), (10, 10), (5, 8)])
def test_maxpool_matches_torch_float64(H, W):
    """Tie-free input (a permutation of distinct values): both rules agree with max_pool2d
    (ceil mode), and un-pooling by the codes is its gradient."""
    g = _gen(3)
    n = 2 * H * W * 8
    x = (torch.randperm(n, generator=g).double() - n // 2).view(2, H, W, 8)
    xt = _nchw(x).requires_grad_(True)
    yt = F.max_pool2d(xt, 2, 2, ceil_mode=True)
    dy = torch.randint(-4, 5, tuple(yt.shape), generator=g).double()
    yt.backward(dy)
    for tie in xo.TIES:
        y, arg = xo.maxpool2x2(x, tie)
        assert torch.equal(y, yt.permute(0, 2, 3, 1)), tie
        dx = xo.unpool(dy.permute(0, 2, 3, 1), arg, (H, W))
        assert torch.equal(dx, xt.grad.permute(0, 2, 3, 1)), tie


def test_pool_tie_rules():
    v = torch.tensor([[2., 2., 2., 2.], [-3., -3., -3., -3.], [1., 5., 5., 0.], [-1., -4., -1., -1.],
                      [0., 0., -1., -2.], [7., 1., 2., 3.]], dtype=torch.float64)
    m, first = xo.pool_select(v, "first")
    assert m.tolist() == [2., -3., 5., -1., 0., 7.]
    assert first.tolist() == [0, 0, 1, 0, 0, 0]
    m2, man = xo.pool_select(v, "mantissa")
    assert torch.equal(m, m2)
    assert man.tolist() == [3, 0, 2, 0, 1, 0]


def test_convpool_matches_torch_float64():
    """Tie-free (distinct conv sums are not guaranteed, so compare only values and, where the
    window maximum is unique, the codes) against conv2d + relu + max_pool2d with indices."""
    g = _gen(4)
    x = xo.dyadic((3, 28, 28, 1), -8, 8, 4, g, CPU)
    w = xo.dyadic((5, 5, 1, 8), -3, 3, 2, g, CPU)
    w[..., 6:] = 0
    b = xo.dyadic((6,), -32, 32, 6, g, CPU, dtype=torch.float32)
    yt = _torch_conv(x, w, torch.cat([b, torch.zeros(2)]), "SAME")
    pt = F.max_pool2d(yt.relu(), 2, 2).permute(0, 2, 3, 1)
    raw = _torch_conv(x, w, None, "SAME").permute(0, 2, 3, 1)
    win = xo._windows(raw)
    unique = (win == win.max(-1, keepdim=True).values).sum(-1) == 1
    for tie in xo.TIES:
        o, codes = xo.convpool_fwd(x, w, b, "SAME", tie, unit=6)
        assert torch.equal(o, pt)
        assert torch.equal(codes == 4, o == 0)
        want = win.argmax(-1)
        live = unique & (o > 0)
        assert torch.equal(codes.long()[live], want[live])
    assert unique.float().mean() > 0.5


def _lenet_inputs(B, seed):
    (x, w1, b1, w2, b2, dP2), fu, bu = xo.lenet_inputs(B, seed, CPU)
    assert (fu, bu) == (LENET_FWD_UNITS, LENET_BWD_UNITS)
    return x, w1, b1, w2, b2, dP2


LENET_FWD_UNITS = (6, 8)
LENET_BWD_UNITS = (9, 5, 9)


def test_lenet_stack_matches_autograd_float64():
    """The LeNet conv-stack oracle against float64 autograd through conv2d / max_pool2d with
    the same staging (pool1 rounded to bf16; dP1 rounded to bf16 for dW1 only).  The pooled
    values are compared with max_pool2d; the gradients flow through the oracle's own
    un-pooling (checked against max_pool2d's gradient in test_maxpool_matches_torch_float64),
    so tied windows do not depend on PyTorch's choice."""
    x, w1, b1, w2, b2, dP2 = _lenet_inputs(3, 5)
    P1, c1, P2, c2 = xo.lenet_fwd(x, w1, b1, w2, b2, "first", LENET_FWD_UNITS)
    b1p = torch.cat([b1, torch.zeros(2)])
    y1 = _torch_conv(x, w1, b1p, "SAME").relu()
    p1t = F.max_pool2d(y1, 2, 2)
    assert torch.equal(P1.double(), xo.to_bf16(p1t.permute(0, 2, 3, 1)).double())
    p1in = P1.double().permute(0, 3, 1, 2).requires_grad_(True)
    w2t = w2.double().permute(3, 2, 0, 1).requires_grad_(True)
    b2t = b2.double().requires_grad_(True)
    y2 = F.conv2d(p1in, w2t, b2t).relu()
    p2t = F.max_pool2d(y2, 2, 2)
    assert torch.equal(P2.double(), xo.to_bf16(p2t.permute(0, 2, 3, 1)).double())
    dW1, db1, dW2, db2 = xo.lenet_bwd(x, P1, c1, c2, dP2, w2, LENET_BWD_UNITS)
    # dW2 / db2 / dP1 through the oracle's own un-pooling (tie rule "first" as PyTorch's CPU pool)
    dY2 = xo.unpool(dP2.view(3, 5, 5, 16), c2).permute(0, 3, 1, 2)
    y2lin = F.conv2d(p1in, w2t, b2t)
    y2lin.backward(dY2)
    assert torch.equal(dW2, w2t.grad.permute(2, 3, 1, 0)[:, :, :6, :])
    assert torch.equal(db2, b2t.grad)
    dP1 = p1in.grad.permute(0, 2, 3, 1)
    xt = _nchw(x)
    w1t = w1.double().permute(3, 2, 0, 1).requires_grad_(True)
    y1lin = F.conv2d(xt, w1t, padding=2)
    y1lin.backward(xo.unpool(xo.to_bf16(dP1).double(), c1).permute(0, 3, 1, 2))
    assert torch.equal(dW1, w1t.grad.permute(2, 3, 1, 0)[:, :, 0, :6])
    assert torch.equal(db1, xo.unpool(dP1, c1).sum((0, 1, 2))[:6])


# ------------------------------------------------------------------ order independence
def _shuffled_f32_matmul(x, w, g, parts):
    """fp32 x @ w with the K dimension permuted and cut into `parts` random-length partial
    sums, each accumulated term by term... in fp32, then the partials added in fp32."""
    K = x.shape[1]
    perm = torch.randperm(K, generator=g)
    cuts = sorted(torch.randperm(K - 1, generator=g)[: parts - 1].add(1).tolist())
    x32, w32 = x.float()[:, perm], w.float()[perm, :]
    tot = torch.zeros(x.shape[0], w.shape[1], dtype=torch.float32)
    for a, b in zip([0] + cuts, cuts + [K]):
        part = torch.zeros_like(tot)
        for k in range(a, b):                       # one rounding per added term
            part = part + x32[:, k:k + 1] * w32[k:k + 1, :]
        tot = tot + part
    return tot


@pytest.mark.parametrize("M,N,K,parts", [(7, 24, 800, 5), (5, 16, 3136, 13), (9, 8, 25, 3)])
def test_fp32_order_independence(M, N, K, parts):
    """Under the magnitude condition any fp32 summation order gives the oracle's bits."""
    g = _gen(K)
    x = xo.dyadic((M, K), -4, 4, 2, g, CPU)
    w = xo.dyadic((K, N), -4, 4, 3, g, CPU)
    ref = xo.to_f32(xo.dense_fwd(x, w, None, False, unit=5))
    for _ in range(3):
        assert torch.equal(_shuffled_f32_matmul(x, w, g, parts), ref)
    assert torch.equal(x.float() @ w.float(), ref)


def test_magnitude_check_fails_loudly():
    g = _gen(6)
    x = xo.dyadic((4, 4096), 200, 256, 0, g, CPU)
    w = xo.dyadic((4096, 4), 200, 256, 0, g, CPU)
    with pytest.raises(AssertionError, match="2\\*\\*22"):
        xo.dense_fwd(x, w, None, False, unit=0)
    with pytest.raises(AssertionError, match="grid"):
        xo.dense_fwd(x[:, :8] * 0.5, w[:8], None, False, unit=0)


# ------------------------------------------------------------------ sensitivity
def test_sensitivity_one_k_element_dropped_from_conv2():
    """Reference conv2 (14 x 14, 5 x 5 SAME, 32 -> 64: K = 800): one term x * w missing from
    one output.  close(rel=2e-2) on the bf16 outputs accepts it, bitwise equality does not.
    (The dropped term is a typical one, |x * w| <= 4 with x, w in [-4, 4], as a lost K element
    is on average; the output is one below 2**8 units, where bf16 holds every integer.)"""
    g = _gen(7)
    d = xo.density_for(800)
    x = xo.dyadic((2, 14, 14, 32), -4, 4, 0, g, CPU, density=d)
    w = xo.dyadic((5, 5, 32, 64), -4, 4, 0, g, CPU, density=d)
    y = xo.conv_fwd(x, w, None, "SAME", unit=0)
    xp = F.pad(x.double(), (0, 0, 2, 2, 2, 2))
    done = False
    for (n, h, wi, co) in [(0, 6, 7, 3), (1, 0, 0, 10), (1, 13, 5, 63), (0, 3, 13, 31)]:
        if abs(y[n, h, wi, co].item()) >= 128:
            continue
        terms = xp[n, h:h + 5, wi:wi + 5, :] * w.double()[:, :, :, co]
        ok = (terms.abs() >= 1) & (terms.abs() <= 4)
        if not ok.any():
            continue
        lost = terms[ok][0]
        bad = y.clone()
        bad[n, h, wi, co] -= lost
        assert close(xo.to_bf16(bad), xo.to_bf16(y), rel=2e-2)
        assert not torch.equal(xo.to_bf16(bad), xo.to_bf16(y))
        assert not torch.equal(xo.to_f32(bad), xo.to_f32(y))
        done = True
    assert done


def test_sensitivity_border_pixel_dropped_from_dw1():
    """LeNet dW1: one tap loses the contribution of one border pixel (in every image, as a
    wrong halo value would).  The whole-tensor relative norm stays under the 1e-2 that
    test_lenet_bwd_gpu allows; the fp32 result differs."""
    B = 16
    x, w1, b1, w2, b2, dP2 = _lenet_inputs(B, 8)
    P1, c1, P2, c2 = xo.lenet_fwd(x, w1, b1, w2, b2, "mantissa", LENET_FWD_UNITS)
    dW1, db1, dW2, db2 = xo.lenet_bwd(x, P1, c1, c2, dP2, w2, LENET_BWD_UNITS)
    # recompute the terms of tap (i, j) = (3, 1) at the border output pixel (0, w)
    dP1 = xo.conv_dgrad(xo.unpool(dP2.view(B, 5, 5, 16), c2), w2, (14, 14), "VALID")
    dY1 = xo.unpool(xo.to_bf16(dP1).double(), c1)
    xp = F.pad(x.double(), (0, 0, 2, 2, 2, 2))
    i, j = 3, 1          # reads input row 1, column w - 1: inside the image for w >= 1
    done = False
    for wcol in range(28):
        lost = (xp[:, 0 + i, wcol + j, 0:1] * dY1[:, 0, wcol, :6]).sum(0)       # [6]
        if lost.abs().max() == 0:
            continue
        bad = dW1.clone()
        bad[i, j, :] -= lost
        assert rel_norm(xo.to_f32(bad), xo.to_f32(dW1)) < 1e-2
        assert not torch.equal(xo.to_f32(bad), xo.to_f32(dW1))
        done = True
        break
    assert done


def test_sensitivity_image_of_partial_tile_duplicated():
    """Dense weight gradient over B = 20000 rows (64-row K steps: the last one holds 32): the
    last row counted twice.  Relative norm ~ 1 / sqrt(B) < 1e-2 passes the gradient tolerance;
    bitwise equality fails."""
    g = _gen(9)
    B, Din, Dout = 20000, 120, 88
    x = xo.dyadic((B, Din), -4, 4, 1, g, CPU)
    dy = xo.dyadic((B, Dout), -4, 4, 2, g, CPU)
    dw, db = xo.dense_wgrad(x, dy, unit=3)
    bad_w = dw + x[-1:].double().t() @ dy[-1:].double()
    bad_b = db + dy[-1].double()
    assert rel_norm(xo.to_f32(bad_w), xo.to_f32(dw)) < 1e-2
    assert rel_norm(xo.to_f32(bad_b), xo.to_f32(db)) < 1e-2
    assert not torch.equal(xo.to_f32(bad_w), xo.to_f32(dw))
    assert not torch.equal(xo.to_f32(bad_b), xo.to_f32(db))


def test_mnist_like_is_mostly_tied():
    g = _gen(10)
    x = xo.mnist_like(8, g, CPU)
    assert set(x.double().unique().tolist()) <= {-0.5, 0.0, 0.5}
    win = xo._windows(x.double())
    tied = (win == win[..., :1]).all(-1).float().mean().item()
    assert tied > 0.5
