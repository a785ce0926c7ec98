"""The LRN backward folded into conv1's weight gradient -- refc1_wgrad_k (csrc/kernels/
refc1_wgrad.hip) and convpool_wgrad_k<..., LRNB> (csrc/kernels/convpool.hip) -- against the
per-element float64 oracle of tests/lrn_oracle.py, through the probe inputs of
tests/refc1_oracle.py: one image is a power of two at one pixel per plane, so every dW
element is one bf16 dP1 element (or exactly 0) times that power.

Per launch: observed elements within half a bf16 ulp + C_FOLD 2**-23 A, every other dW
element exactly 0, db within the summed budgets.  Per sweep (25 launches at cin 1, 9 at
cin 3, B = 5 on one block): all 196 windows, 4 channel groups and 5 image slots observed.
C_FOLD = 100 comes from the float32 transcription (tests/test_refc1_oracle_cpu.py: worst
15.40 units), not from the kernels.  What the kernels measured on an MI355X (units of
2**-23 A past the bf16 half-ulp, worst element of a sweep over both biases; the half-ulp
is 32768 .. 65536 units, so the fp32 error rarely shows past it, and at most 1 of the ~6000
observed elements of a sweep is not the bf16 rounding of the float64 reference;
profiles/r7/refc1_oracle/):

                                   the model's alpha   alpha 0.05   transcription (unrounded)
  refc1_wgrad, cin 1 / 3           0.1 / 0.0           0.0 / 0.0    8.25, 15.40
  refc1_wgrad, cin 3, PK3=0        0.0                 0.0          8.25, 15.40
  convpool fold, beta 0.75         0.1 / 0.0           0.0 / 0.0    8.25, 15.40
  convpool fold, beta 0.5          0.0 / 0.0           0.3 / 0.2    8.93, 13.35

The bit-exact side of the same kernels (everything but the LRN math) is
test_exact_kernels_gpu.test_refc1_wgrad_exact / test_convpool_lrn_fold_exact.
"""
import os
import subprocess
import sys

import pytest
import torch

import lrn_oracle as lo
import refc1_oracle as ro
from test_refc1_wgrad_gpu import _reduce

pytestmark = pytest.mark.gpu

CINS = pytest.mark.parametrize("cin", [1, 3], ids=["cin1", "cin3"])
SETTINGS = pytest.mark.parametrize("bias,alpha", ro.SETTINGS)


def _refc1(K, dev, pr, bias, alpha, beta):
    x, p1, dn, codes = pr.to(dev)
    grid = K.refc1_wgrad_blocks(ro.B)
    assert grid == 1
    slab = torch.full((grid * (48 if pr.cin == 1 else 80) * 32,), float("nan"), device=dev)
    K.refc1_wgrad(x, dn, p1, codes, slab, grid, ro.B, bias, alpha, beta, cin=pr.cin)
    return _reduce(K, slab, grid, dev, pr.cin)


def _convpool(K, dev, pr, bias, alpha, beta):
    x, p1, dn, codes = pr.to(dev)
    grid = 1
    slab = torch.full((grid * K.convpool_rows(pr.cin, 32, 5, 2, 28, 28) * 32,), float("nan"), device=dev)
    K.convpool_wgrad(x, dn, codes, slab, grid, ro.B, pr.cin, 32, 5, 2, 28, 28, lrn_p=p1, lrn_bias=bias,
                     lrn_alpha=alpha, lrn_beta=beta, lrn_r=4)
    return _reduce(K, slab, grid, dev, pr.cin)


def _sweep(K, dev, run, cin, bias, alpha, beta, what):
    cov = ro.Coverage()
    worst, seen, differ = 0.0, 0, 0
    for L in range(ro.launches(cin)):
        pr = ro.probe(cin, alpha, L)
        dw, db = run(K, dev, pr, bias, alpha, beta)
        full = ro.reference(pr, bias, alpha, beta)
        ref, A, mask = ro.expected(pr, bias, alpha, beta, full)
        cov.add(pr, A)
        dw, db = dw.double().cpu(), db.double().cpu()
        where = f"{what} launch {L} (image {pr.bstar}, centres {pr.centres}, k {pr.k})"
        assert bool((dw[~mask] == 0).all()), f"{where}: an unobserved dW element is not 0"
        got = dw / pr.scale
        worst = max(worst, lo.units(got, ref, A, bf16=True))
        seen += int(mask.sum())
        differ += int((got != lo.round_to(ref, True))[mask].sum())
        ok, report = lo.within_budget(got, ref, A, lo.C_FOLD, True)
        assert ok, f"{where}: {report} (flat index over [ky, kx, ci, co])"
        rb, tol = ro.bias_expected(pr, bias, alpha, beta, lo.C_FOLD, full)
        over = ((db - rb).abs() - tol).max().item()
        assert over <= 0, f"{where}: db off by {over:.3e} more than its budget"
    print(f"{what}: {worst:.1f} units of 2**-23 A past the bf16 half-ulp; {differ} of {seen} observed elements "
          f"are not the bf16 rounding of the reference")
    cov.check()


@CINS
@SETTINGS
def test_refc1_wgrad_probe(dev, K, grid_cap, cin, bias, alpha):
    """one block over three 2-image tiles: the probed image sits in either half of a tile, in
    either LDS buffer, or alone in the partial last tile"""
    grid_cap(1)
    _sweep(K, dev, _refc1, cin, bias, alpha, 0.75, f"refc1_wgrad cin {cin} bias {bias} alpha {alpha:.3g}")


@CINS
@SETTINGS
@pytest.mark.parametrize("beta", [0.75, 0.5])
def test_convpool_fold_probe(dev, K, cin, bias, alpha, beta):
    """LRNB 2 (beta 0.75) and 1: one block over five 1-image groups"""
    _sweep(K, dev, _convpool, cin, bias, alpha, beta, f"convpool fold cin {cin} beta {beta} bias {bias} alpha {alpha:.3g}")


def test_scalar_round_cin3_producers(dev):
    """kRefc1x3[0] (one LRN round at a time) is selected by MNISTX_REFC1_PK3=0, read once when
    the extension loads: the cin-3 cases of the exact and the probe test in one fresh
    process.  Nothing else runs here after it, and it is not tried again."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", "-q", "-x", "-s", "-p", "no:cacheprovider",
           "tests/test_exact_kernels_gpu.py::test_refc1_wgrad_exact",
           "tests/test_refc1_oracle_gpu.py::test_refc1_wgrad_probe", "-k", "cin3"]
    r = subprocess.run(cmd, cwd=root, env=dict(os.environ, MNISTX_REFC1_PK3="0"), capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-6000:]}\n{r.stderr[-3000:]}"
