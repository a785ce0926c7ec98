"""The probe oracle of the LRN-backward folds (tests/refc1_oracle.py) checked on the CPU:
the probe algebra against float64 autograd through conv2d . unpool . LRN, the budget
constant against the float32 transcription of the folds' arithmetic over exactly the probe
inputs, the sensitivity of those inputs to five errors a fold can make, and the coverage
of the sweep.

Measured here (units of 2**-23 times the element's scale A, the worst element of pool1 x
dL/d norm1 over every launch of the sweeps; running window sums):

  beta 0.75 as pow_beta<true> forms it (rsqrt, sqrt; both folds)    worst 15.40 (alpha 0.05), 8.25 (the model's)
  beta 0.5 as exp2(-beta log2 sc) (the convpool fold, LRNB 1)       worst 13.35 (alpha 0.05), 8.93 (the model's)
  x 4 = 61.6, x 8 = 123.2   ->  C_FOLD = 100 (lrn_oracle.C_BF16 = 640 is more than 8x: not reused)
"""
import pytest
import torch

import lrn_oracle as lo
import refc1_oracle as ro
from distributed_tensorflow_ibm_mnist_amd.models.torch_ref import lrn_tf

BETAS = [0.75, 0.5]           # refc1_wgrad takes 0.75 only, the convpool fold both
CINS = [1, 3]


def _sweep(cin, alpha):
    return [ro.probe(cin, alpha, L) for L in range(ro.launches(cin))]


def _autograd_dw(pr, bias, alpha, beta):
    """dL/dW of L = <dn, LRN(pool(conv(x, W)))> at pool = p1, the pool taken through the fixed codes"""
    x = pr.x.double().permute(0, 3, 1, 2)
    W = torch.zeros(ro.C, pr.cin, 5, 5, dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.conv2d(x, W, padding=2)
    win = out.reshape(ro.B, ro.C, 14, 2, 14, 2).permute(0, 1, 2, 4, 3, 5).reshape(ro.B, ro.C, 14, 14, 4)
    codes = pr.codes.permute(0, 3, 1, 2).long()
    P = win.gather(-1, codes.clamp(max=3).unsqueeze(-1)).squeeze(-1) * (codes != 4)
    z = pr.p1.double().permute(0, 3, 1, 2) + (P - P.detach())
    N = lrn_tf(z, ro.R, bias, alpha, beta)
    (N * pr.dn.double().permute(0, 3, 1, 2)).sum().backward()
    return W.grad.permute(2, 3, 1, 0)


@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("bias,alpha,beta", [(1.0, lo.REF_ALPHA, 0.75), (2.0, lo.BIG_ALPHA, 0.5), (1.0, lo.BIG_ALPHA, 0.75)])
def test_probe_algebra_matches_float64_autograd(cin, bias, alpha, beta):
    for pr in _sweep(cin, alpha):
        ref, A, mask = ro.expected(pr, bias, alpha, beta)
        want = _autograd_dw(pr, bias, alpha, beta)
        got = ref * pr.scale
        assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
        assert bool((ref[~mask] == 0).all()) and bool((A[~mask] == 0).all())
        assert bool((A >= ref.abs() * (1 - 1e-12)).all())
        # every active channel of every reached window is observed, exactly once
        active = sum(int((pr.codes[pr.bstar, yp, xp] != 4).sum()) for _, yp, xp in ro.reached(pr.centres))
        assert int(mask.sum()) == active


def _transcription(pr, bias, alpha, beta):
    x, g = pr.lrn_inputs()
    return lo.lrn_f32(x, g, ro.R, bias, alpha, beta, False, running=True, b075=(beta == 0.75))[1]


def _shown(pr, dp1):
    """what the kernel's dW / 2**k shows of a dP1 [pixels, 32]: rounded to bf16 as staged"""
    return pr.observe(lo.round_to(dp1.double(), True).reshape(ro.B, 14, 14, ro.C))


def test_c_fold_is_four_times_the_transcription():
    worst = {}
    top = 0.0
    for cin in CINS:
        for bias, alpha in ro.SETTINGS:
            for pr in _sweep(cin, alpha):
                x, g = pr.lrn_inputs()
                top = max(top, alpha * float(x.float().abs().max()) ** 2)
                for beta in BETAS:
                    _, dx, _, A = lo.lrn_ref(x, g, ro.R, bias, alpha, beta, False)
                    f = _transcription(pr, bias, alpha, beta)
                    assert bool((f[A == 0] == 0).all())
                    key = (beta, "ref" if alpha == lo.REF_ALPHA else "big")
                    worst[key] = max(worst.get(key, 0.0), lo.units(f, dx, A))
                    # the transcription alone passes every probe launch
                    ref, Ao, _ = ro.expected(pr, bias, alpha, beta)
                    ok, report = lo.within_budget(_shown(pr, f), ref, Ao, lo.C_FOLD, True)
                    assert ok, report
    for key in sorted(worst):
        print(f"running sums over the probe inputs, beta {key[0]} alpha {key[1]}: worst {worst[key]:.2f} units")
    w = max(worst.values())
    print(f"worst {w:.2f} units, c_fold = {lo.C_FOLD:g}, alpha max x^2 <= {top:.2f}")
    assert 4 * w <= lo.C_FOLD <= 8 * w, w
    assert lo.C_FOLD <= lo.C_BF16_CAP and top <= lo.DOMAIN, top


# ------------------------------------------------------------------ sensitivity
MUTATIONS = ["identity", "cross_term_dropped", "radius_3", "exchange_zeroed_at_vector_boundary", "tile_images_swapped"]


def _mutant(pr, bias, alpha, beta, mut):
    """float64 dP1 [pixels, 32] with one error a fold can make"""
    x, g = (t.double() for t in pr.lrn_inputs())
    if mut == "tile_images_swapped":          # images (0, 1) and (2, 3) share a tile; 4 is alone
        g = pr.dn.double()[[1, 0, 3, 2, 4]].reshape(-1, ro.C)
    if mut == "identity":
        return g
    c = torch.arange(ro.C)
    r = 3 if mut == "radius_3" else ro.R
    band = ((c.unsqueeze(1) - c.unsqueeze(0)).abs() <= r).double()            # [c, c']
    if mut == "exchange_zeroed_at_vector_boundary":
        band[8:16, 0:8] = 0                   # vector 1 gets zeros for its left neighbours
    sc = bias + alpha * (x * x) @ band.t()
    dx = g * sc ** -beta
    if mut != "cross_term_dropped":
        dx = dx - 2.0 * alpha * beta * x * ((g * x * sc ** -(beta + 1.0)) @ band.t())
    return dx


@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("beta", BETAS)
def test_budget_rejects_every_mutation_at_both_alphas(cin, beta):
    for mut in MUTATIONS:
        for alpha in lo.ALPHAS:
            failed = 0
            for pr in _sweep(cin, alpha):
                ref, A, _ = ro.expected(pr, 1.0, alpha, beta)
                failed += not lo.within_budget(_shown(pr, _mutant(pr, 1.0, alpha, beta, mut)), ref, A, lo.C_FOLD, True)[0]
            print(f"cin {cin} beta {beta} alpha {alpha:.3g} {mut}: {failed} of {ro.launches(cin)} launches rejected")
            assert failed >= 1, (mut, alpha)
    # the unmutated float64 form passes
    for alpha in lo.ALPHAS:
        for pr in _sweep(cin, alpha):
            ref, A, _ = ro.expected(pr, 1.0, alpha, beta)
            assert lo.within_budget(_shown(pr, _mutant(pr, 1.0, alpha, beta, None)), ref, A, lo.C_FOLD, True)[0]


@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("bias,alpha", ro.SETTINGS)
def test_sweep_coverage(cin, bias, alpha):
    for beta in BETAS:
        cov = ro.Coverage()
        for pr in _sweep(cin, alpha):
            cov.add(pr, ro.expected(pr, bias, alpha, beta)[1])
        cov.check()


def test_bias_budget_holds_for_the_transcription():
    """db summed in fp32 from the transcription's bf16 dP1 lies inside bias_expected's bound"""
    for cin in CINS:
        for bias, alpha in ro.SETTINGS:
            pr = ro.probe(cin, alpha, 3)
            f = lo.round_to(_transcription(pr, bias, alpha, 0.75).double(), True).float()
            act = (pr.codes.reshape(-1, ro.C) != 4)
            db = torch.zeros(ro.C)
            for row in (f * act):                      # one fp32 rounding per term
                db = db + row
            ref, tol = ro.bias_expected(pr, bias, alpha, 0.75, lo.C_FOLD)
            assert bool(((db.double() - ref).abs() <= tol).all())
            assert bool((tol < 0.05 * (f.double().abs() * act).sum(0)).all())      # and the bound is not vacuous
