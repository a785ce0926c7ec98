"""The LRN oracle (tests/lrn_oracle.py) checked on the CPU: its float64 closed form agrees
with float64 autograd of torch_ref.lrn_tf, the budget constants are what the float32
transcriptions measure, the domain of the running window sum is pinned, and five small
errors of an LRN kernel are rejected by the budget on the spike probes.

Measured here (units of 2**-23 times the element's scale A; the worst element over every
LRN evaluation that tests/test_lrn_oracle_gpu.py asks of a kernel):

  direct sums,  the fp32 kernels' inputs   worst  3.32   x 4 = 13.3, x 8 = 26.6   ->  c_f32  = 20
  running sums, the bf16 kernels' inputs   worst 118.4   x 4 = 474,  x 8 = 947    ->  c_bf16 = 640
      (the backward at alpha = 0.05 on post-ReLU normal values of scale 3; the forward's
       worst is 4.4, and the direct sums stay below 3.5 on the same inputs)
  cap on c_bf16: 2**-12 / 2**-23 = 2048, an eighth of the smallest bf16 half-ulp

  outside the domain (one 128 among values near 0.25, alpha = 0.05, alpha max x^2 = 819):
  running sums 1100 .. 2130 forward, 13900 .. 38300 backward (0.46 % of A, more than half
  of a bf16 half-ulp); direct sums stay below 7.2.
"""
import pytest
import torch

import lrn_oracle as lo
from distributed_tensorflow_ibm_mnist_amd.models.torch_ref import lrn_tf


# the tolerance predicate of test_kernels_gpu.test_lrn, copied
def close(out, ref, rel=2e-2):
    out = out.float()
    ref = ref.float()
    tol = rel * ref.abs().max().item() + 1e-6
    err = (out - ref).abs().max().item()
    return err <= tol


def _autograd(x, g, r, bias, alpha, beta):
    """float64 autograd of the model's LRN (NCHW, pixels as a 1 x P image)."""
    xt = x.double().t().reshape(1, x.shape[1], 1, x.shape[0]).requires_grad_(True)
    y = lrn_tf(xt, r, bias, alpha, beta)
    y.backward(g.double().t().reshape(y.shape))
    back = lambda t: t.detach().reshape(x.shape[1], x.shape[0]).t()
    return back(y), back(xt.grad)


def _generators(C):
    yield "spike", lo.spike_probes(C, lo.REF_ALPHA)
    yield "spike, alpha 0.05", lo.spike_probes(C, lo.BIG_ALPHA)
    yield "spike, signed", lo.spike_probes(C, lo.BIG_ALPHA, signed=True)
    yield "post-ReLU scale 3", lo.random_pixels(61, C, 3.0, 1)
    yield "post-ReLU scale 30", lo.random_pixels(61, C, 30.0, 2)
    yield "signed", lo.random_pixels(61, C, 3.0, 3, signed=True)
    yield "wide range", lo.wide_range(61, C, 4)
    yield "all zero", torch.zeros(5, C, dtype=torch.bfloat16)
    yield "pool", lo.pool_input(2, 4, 6, C, 5).reshape(-1, C)


@pytest.mark.parametrize("C,r", [(8, 4), (16, 4), (32, 2), (64, 5), (24, 4)])
@pytest.mark.parametrize("bias,alpha,beta", [(1.0, lo.REF_ALPHA, 0.75), (2.0, lo.BIG_ALPHA, 0.5), (1.0, lo.BIG_ALPHA, 1.0)])
def test_reference_matches_float64_autograd(C, r, bias, alpha, beta):
    for name, x in _generators(C):
        g = lo.grads(x.shape, 9)
        yt, dxt = _autograd(x, g, r, bias, alpha, beta)
        for mask in (False, True):
            y, dx, Ay, Adx = lo.lrn_ref(x, g, r, bias, alpha, beta, mask)
            want = dxt * (x.double() > 0) if mask else dxt
            assert (y - yt).abs().max().item() <= 1e-12 * max(1.0, yt.abs().max().item()), name
            assert (dx - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item()), name
            assert torch.equal(Ay, y.abs()) and bool((Adx >= dx.abs() * (1 - 1e-12)).all()), name
            assert bool((dx[x.double() <= 0] == 0).all()) or not mask, name


@pytest.mark.parametrize("bf16", [True, False])
def test_pool_reference(bf16):
    N, H, W, C = 3, 6, 10, 32
    x = lo.pool_input(N, H, W, C, 21)
    x[1, 2:4, 4:6, 3] = x[1, 2, 4, 3]                      # a tie of all four: the first wins
    x[1, 2:4, 4:6, :3] = 0                                  # (its window's neighbours alike)
    x[1, 2:4, 4:6, 4:] = x[1, 2, 4, 4:].clone()
    pooled, exact, A, codes, decided = lo.lrn_pool_ref(x, H, W, 4, 1.0, lo.BIG_ALPHA, 0.75, bf16)
    y = lo.round_to(lo.lrn_ref(x, None, 4, 1.0, lo.BIG_ALPHA, 0.75, False)[0], bf16)
    yt = y.permute(0, 3, 1, 2).clone().requires_grad_(True)
    pt = torch.nn.functional.max_pool2d(yt, 2, 2)
    assert torch.equal(pooled, pt.detach().permute(0, 2, 3, 1))
    assert torch.equal(lo.round_to(exact, bf16), pooled) and bool((A >= exact.abs()).all())
    assert int(codes[1, 1, 2, 3]) == 0 and bool(decided[1, 1, 2, 3])
    assert int(codes[0, 0, 0, 0]) == 0 and bool(decided[0, 0, 0, 0])       # the all-zero window
    # the codes select the pooled value, and no earlier position holds it
    cand = y.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)
    assert torch.equal(cand.gather(-1, codes.long().unsqueeze(-1)).squeeze(-1), pooled)
    earlier = torch.arange(4) < codes.long().unsqueeze(-1)
    assert not bool(((cand == pooled.unsqueeze(-1)) & earlier).any())
    # un-pooling through the codes is max_pool2d's gradient wherever the maximum is unique
    dP = lo.grads(tuple(pooled.shape), 22)
    pt.backward(dP.double().permute(0, 3, 1, 2))
    g = lo.unpool(dP, codes, H, W)
    unique = ((cand == pooled.unsqueeze(-1)).sum(-1) == 1)
    full = unique.unsqueeze(-1).expand(cand.shape).reshape(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C)
    assert torch.equal(g[full], yt.grad.permute(0, 2, 3, 1)[full])
    assert torch.equal(g.reshape(N, H // 2, 2, W // 2, 2, C).sum(dim=(2, 4)), dP.double())


@pytest.mark.parametrize("bf16", [True, False])
def test_pool_inputs_decide_the_codes(bf16):
    """the condition the GPU test asserts too: at most 1 % of the windows are left out of the
    code comparison, and decided windows are those whose top two differ after rounding"""
    for N, H, W, C in lo.POOL_CASES:
        for relu in (True, False):
            x = lo.pool_inputs(N, H, W, C, relu)[0]
            for alpha in lo.ALPHAS:
                for beta in lo.POOL_BETAS:
                    decided = lo.lrn_pool_ref(x, H, W, lo.POOL_R, lo.POOL_BIAS, alpha, beta, bf16)[4]
                    assert 1.0 - decided.double().mean().item() <= lo.MAX_UNDECIDED, (N, H, W, C, relu, alpha, beta)
                    plain = lo.lrn_pool_ref(x, H, W, lo.POOL_R, lo.POOL_BIAS, alpha, beta, bf16, c=0.0)[4]
                    assert bool((plain | ~decided).all())
                    assert (plain & ~decided).double().mean().item() <= 1e-3


def _worst(points, running):
    worst, top = 0.0, 0.0
    for name, x, g, r, bias, alpha, beta, m, vs in points:
        y, dx, Ay, Adx = lo.lrn_ref(x, g, r, bias, alpha, beta, m, vector_scale=vs)
        yf, dxf = lo.lrn_f32(x, g, r, bias, alpha, beta, m, running)
        worst = max(worst, lo.units(yf, y, Ay), lo.units(dxf, dx, Adx))
        top = max(top, alpha * float(x.float().abs().max()) ** 2)
        assert bool((yf[Ay == 0] == 0).all()) and bool((dxf[Adx == 0] == 0).all()), name
    return worst, top


def test_c_f32_is_four_times_the_direct_transcription():
    worst, _ = _worst(lo.f32_points(), running=False)
    print(f"direct sums over the fp32 kernels' inputs: worst {worst:.2f} units, c_f32 = {lo.C_F32:g}")
    assert 4 * worst <= lo.C_F32 <= 8 * worst, worst


def test_c_bf16_is_four_times_the_running_transcription():
    worst, top = _worst(lo.bf16_points(), running=True)
    print(f"running sums over the bf16 kernels' inputs: worst {worst:.2f} units, c_bf16 = {lo.C_BF16:g}, "
          f"alpha max x^2 <= {top:.2f}")
    assert 4 * worst <= lo.C_BF16 <= 8 * worst, worst
    # the condition on the inputs: the fp32 part of the budget is an eighth of a bf16 half-ulp
    assert lo.C_BF16 * lo.U23 <= 2.0 ** -12 and lo.C_BF16 <= lo.C_BF16_CAP
    # every input sent to a bf16 kernel lies inside the documented domain
    assert top <= lo.DOMAIN, top


@pytest.mark.parametrize("C,r", lo.LRN_ALL)
def test_wide_range_at_large_alpha_is_outside_the_domain(C, r):
    """One 128 among values near 0.25 at alpha = 0.05: the running sum, having held 128^2,
    keeps an absolute error of a few 2**-10 that alpha = 0.05 does not scale away.  The
    running transcription leaves the cap (the direct one does not), so this input is
    outside the domain and stays out of the GPU tests; at the model's alpha it is inside."""
    x, g = lo.wide_inputs(C)
    assert lo.BIG_ALPHA * float(x.float().max()) ** 2 > 100 * lo.DOMAIN
    for alpha, inside in ((lo.REF_ALPHA, True), (lo.BIG_ALPHA, False)):
        y, dx, Ay, Adx = lo.lrn_ref(x, g, r, 1.0, alpha, 0.75, True)
        yr, dxr = lo.lrn_f32(x, g, r, 1.0, alpha, 0.75, True, running=True)
        yd, dxd = lo.lrn_f32(x, g, r, 1.0, alpha, 0.75, True, running=False)
        run = max(lo.units(yr, y, Ay), lo.units(dxr, dx, Adx))
        direct = max(lo.units(yd, y, Ay), lo.units(dxd, dx, Adx))
        print(f"C {C} r {r} alpha {alpha:.3g}: running {run:.1f}, direct {direct:.1f} units")
        assert direct <= lo.C_F32
        if inside:
            assert run <= lo.C_BF16 / 4
        else:
            assert run > 4 * lo.C_BF16_CAP           # a bf16 half-ulp is 8 to 16 caps
            assert not lo.within_budget(dxr, dx, Adx, lo.C_BF16_CAP, False)[0]


def test_unpooled_gradient_needs_the_vector_scale():
    """The pool backward's dL/dy is zero at three of a window's four positions.  Where every
    term of an element's own window is zero its scale A is 0 and dx is 0; the running sum
    reaches that element after adding and removing other channels' terms and keeps their
    rounding residue (times 2 alpha beta x: some 1e-9 of the pixel's largest gradient).  The
    direct sums give 0 there.  So the running kernels' pool backward is held to the scale of
    the whole 8-channel vector's extent (lrn_ref vector_scale), the fp32 kernels' to the
    window's own."""
    N, H, W, C = lo.POOL_CASES[0]
    x, dP = lo.pool_inputs(N, H, W, C, False)
    codes = lo.lrn_pool_ref(x, H, W, 4, 1.0, lo.BIG_ALPHA, 0.75, True)[3]
    x, g = x.reshape(-1, C), lo.unpool(dP, codes, H, W).reshape(-1, C)
    _, dx, _, A = lo.lrn_ref(x, g, 4, 1.0, lo.BIG_ALPHA, 0.75, False)
    _, _, _, Avec = lo.lrn_ref(x, g, 4, 1.0, lo.BIG_ALPHA, 0.75, False, vector_scale=True)
    run = lo.lrn_f32(x, g, 4, 1.0, lo.BIG_ALPHA, 0.75, False, running=True)[1]
    direct = lo.lrn_f32(x, g, 4, 1.0, lo.BIG_ALPHA, 0.75, False, running=False)[1]
    empty = (A == 0) & (x.double() != 0)
    assert int(empty.sum()) > 100 and bool((dx[empty] == 0).all())
    assert bool((direct[empty] == 0).all()) and lo.within_budget(direct, dx, A, lo.C_F32, False)[0]
    left = run[empty].abs()
    print(f"{int((left > 0).sum())} of {int(empty.sum())} elements with an empty window keep a residue, up to {left.max():.2e}")
    assert int((left > 0).sum()) > 0 and not lo.within_budget(run, dx, A, lo.C_BF16, False)[0]
    assert bool((Avec >= A * (1 - 1e-12)).all()) and lo.within_budget(run, dx, Avec, lo.C_BF16, False)[0]
    assert left.max().item() <= 1e-6 * dx.abs().max().item()


# ------------------------------------------------------------------ sensitivity
MUTATIONS = ["drop_at_vector_boundary", "radius_short_at_last_vector", "leak_from_next_pixel", "pow_beta_for_beta_plus_1",
             "mask_ge"]


def _mutant(x, g, r, bias, alpha, beta, relu_mask, mut):
    """lrn_ref with one error of the kind a channel-parallel kernel can make; x is [P, C]."""
    x, g = x.double(), g.double()
    P, C = x.shape
    c = torch.arange(C)
    band = ((c.unsqueeze(1) - c.unsqueeze(0)).abs() <= r).double()          # [c, c']
    if mut == "drop_at_vector_boundary":
        band[8, 7] = 0                       # channel 8 misses its left neighbour in the previous vector
    if mut == "radius_short_at_last_vector":
        far = (c.unsqueeze(1) - c.unsqueeze(0)).abs() == r
        band[C - 8:] = band[C - 8:] * (~far[C - 8:]).double()

    def win(t):
        s = t @ band.t()
        if mut == "leak_from_next_pixel":    # the last channel's window runs on into the next pixel's first
            s[:-1, C - 1] += t[1:, 0]
        return s

    sc = bias + alpha * win(x * x)
    pw = sc ** -beta
    pw1 = pw if mut == "pow_beta_for_beta_plus_1" else sc ** -(beta + 1.0)
    y = x * pw
    dx = g * pw - 2.0 * alpha * beta * x * win(g * x * pw1)
    if relu_mask:
        dx = dx * ((x >= 0) if mut == "mask_ge" else (x > 0))
    return y, dx


def _accepts(x, g, r, bias, alpha, beta, mut, predicate):
    """does `predicate(out, ref, A)` accept the mutant's bf16-rounded forward, backward and
    masked backward, as test_lrn checks them?"""
    ok = True
    for mask in (False, True):
        y, dx, Ay, Adx = lo.lrn_ref(x, g, r, bias, alpha, beta, mask)
        ym, dxm = _mutant(x, g, r, bias, alpha, beta, mask, mut)
        ok = ok and predicate(lo.round_to(ym, True), y, Ay) and predicate(lo.round_to(dxm, True), dx, Adx)
    return ok


def _budget(out, ref, A):
    return lo.within_budget(out, ref, A, lo.C_BF16, True)[0]


def _close(out, ref, A):
    return close(out, ref)


@pytest.mark.parametrize("alpha", lo.ALPHAS)
@pytest.mark.parametrize("C,r", [(16, 4), (64, 4), (32, 2), (64, 5)])
def test_budget_rejects_every_mutation_on_the_spike_probes(C, r, alpha):
    x = lo.spike_probes(C, alpha)
    g = lo.grads(x.shape, 31)
    assert _accepts(x, g, r, 1.0, alpha, 0.75, None, _budget)            # the unmutated reference passes
    for mut in MUTATIONS:
        assert not _accepts(x, g, r, 1.0, alpha, 0.75, mut, _budget), mut
    # the report names the element: the dropped term is channel 7's, missing at channel 8
    y, _, Ay, _ = lo.lrn_ref(x, g, r, 1.0, alpha, 0.75, False)
    ym = _mutant(x, g, r, 1.0, alpha, 0.75, False, "drop_at_vector_boundary")[0]
    ok, report = lo.within_budget(lo.round_to(ym, True), y, Ay, lo.C_BF16, True)
    assert not ok and "(pixel 14, channel 8)" in report and "out " in report and "ref " in report, report


# which mutations test_lrn's close(rel=2e-2) accepts on its own inputs (post-ReLU normal
# values of scale 3 on 5 x 13 x 13 pixels, beta 0.75, bias 1), at the model's alpha and at
# the large one.  At the model's alpha LRN is nearly the identity: every wrong window and
# even the wrong power pass, only the `>=` mask (a whole gradient where 0 belongs) does
# not.  At alpha = 0.05 the tolerance rejects all five, but of test_lrn's cases only C = 64
# and 32 with r = 4 run at the model's alpha and none varies beta or bias.
CLOSE_ACCEPTS = {
    lo.REF_ALPHA: {"drop_at_vector_boundary", "radius_short_at_last_vector", "leak_from_next_pixel",
                   "pow_beta_for_beta_plus_1"},
    lo.BIG_ALPHA: set(),
}


@pytest.mark.parametrize("alpha", lo.ALPHAS)
def test_what_the_maximum_relative_tolerance_accepts(alpha):
    torch.manual_seed(7)
    C, r = 64, 4
    x = (torch.randn(5 * 13 * 13, C) * 3.0).to(torch.bfloat16).relu()
    g = torch.randn(5 * 13 * 13, C).to(torch.bfloat16)
    accepted = {m for m in MUTATIONS if _accepts(x, g, r, 1.0, alpha, 0.75, m, _close)}
    rejected_by_budget = {m for m in MUTATIONS if not _accepts(x, g, r, 1.0, alpha, 0.75, m, _budget)}
    print(f"alpha {alpha:.3g}: close(rel=2e-2) accepts {sorted(accepted)}; the budget rejects {sorted(rejected_by_budget)}")
    assert _accepts(x, g, r, 1.0, alpha, 0.75, None, _close) and _accepts(x, g, r, 1.0, alpha, 0.75, None, _budget)
    assert rejected_by_budget == set(MUTATIONS)
    assert accepted == CLOSE_ACCEPTS[alpha]
    if alpha == lo.REF_ALPHA:
        assert accepted & rejected_by_budget                 # the gap this oracle closes
