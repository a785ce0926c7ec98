"""Probe inputs that make the LRN backward folded into conv1's weight gradient observable.

refc1_wgrad_k and convpool_wgrad_k<..., LRNB> compute dP1 = LRN backward of (pool1, dL/d
norm1), keep it in LDS as bf16, un-pool it through the argmax codes and contract it with
the input images.  dP1 never reaches memory; a probe image does the contraction by hand:

    image b* = 2**k at pixel (r, c) of plane ci, every other image 0
      =>  dW[ky, kx, ci, co] = 2**k * dY[b*, r - ky + 2, c - kx + 2, co]

and dY = unpool(dP1, codes) is either one bf16 dP1 element or 0, so dW / 2**k is exact in
fp32 and can be held to the per-element float64 budget of tests/lrn_oracle.py.  The 5 x 5
patch around an odd-row (or odd-column) centre reaches 3 x 3 pool windows; the codes of
those windows point inside the patch (varied by channel, about 1 in 16 inactive), so every
channel of every reached window is observed or must read exactly 0.  The other four images
keep finite non-zero pool1, gradients and codes: their dP1 is computed and multiplied by
zero, so a leak between the two images of a tile shows as a wrong value.

One sweep is 25 launches (cin 1: one centre each) or 9 (cin 3: one centre per plane) of
B = 5 images on one block: b* = launch mod 5 walks both images of a 2-image tile, both LDS
buffers and the partial last tile.  `Coverage` asserts, from the reference alone, that the
sweep observes all 196 windows, all 4 channel groups and all 5 image slots.

Nothing here imports the extension; everything is generated on the CPU from fixed seeds.
"""
import functools

import torch

import exact_oracle as xo
import lrn_oracle as lo

B, NWIN, C, R = 5, 196, 32, 4
# centres of the 5 x 5 patches: rows reach windows 0-2, 3-5, 6-8, 9-11, 12-13 (the patch
# around row 27 hangs over the bottom padding), columns -, 0-1 (over the left padding),
# 2-4, 5-7, 8-10, 11-13
ROWS = (3, 9, 15, 21, 27)
COLS = (1, 7, 13, 19, 25)
CENTRES = [(r, c) for r in ROWS for c in COLS]
SETTINGS = [(bias, alpha) for bias in lo.BIASES for alpha in lo.ALPHAS]
SPIKE_ROLL = 7


def launches(cin):
    """25 centres, one per plane and launch"""
    return (len(CENTRES) + cin - 1) // cin


class Probe:
    """The inputs of one launch: x [B, 28, 28, cin], p1 / dn [B, 14, 14, 32] (bf16), codes
    uint8; bstar the probed image, centres / k per input plane."""

    def __init__(self, cin, x, p1, dn, codes, bstar, centres, k):
        self.cin, self.x, self.p1, self.dn, self.codes = cin, x, p1, dn, codes
        self.bstar, self.centres, self.k = bstar, centres, k
        # dW = scale * (observed dP1), per plane
        self.scale = torch.tensor([2.0 ** e for e in k], dtype=torch.float64).view(1, 1, cin, 1)

    def to(self, dev):
        return tuple(t.to(dev) for t in (self.x, self.p1, self.dn, self.codes))

    def observe(self, t):
        """t [B, 14, 14, 32] (any per-element quantity of dP1) -> [5, 5, cin, 32] float64: what
        of it each dW element shows, 0 where the code points elsewhere or the tap reads padding"""
        b = self.bstar
        full = xo.unpool(t[b:b + 1].cpu(), self.codes[b:b + 1])[0]          # [28, 28, 32]
        out = torch.zeros(5, 5, self.cin, C, dtype=torch.float64)
        for ci, (r, c) in enumerate(self.centres):
            for ky in range(5):
                for kx in range(5):
                    oy, ox = r - ky + 2, c - kx + 2
                    if 0 <= oy < 28 and 0 <= ox < 28:
                        out[ky, kx, ci] = full[oy, ox]
        return out

    def lrn_inputs(self):
        """(pool1, dL/d norm1) as [pixels, 32] for the lrn_oracle functions"""
        return self.p1.reshape(-1, C), self.dn.reshape(-1, C)


def reached(centres):
    """(plane, window row, window column) of every pool window a patch reaches"""
    return [(ci, yp, xp) for ci, (r, c) in enumerate(centres)
            for yp in range(max((r - 3) // 2, 0), min((r + 1) // 2, 13) + 1)
            for xp in range(max((c - 3) // 2, 0), min((c + 1) // 2, 13) + 1)]


def _inside(w, centre):
    """which of window w's two rows (columns) lie inside the patch and the image"""
    return [p for p in (0, 1) if centre - 2 <= 2 * w + p <= centre + 2 and 0 <= 2 * w + p < 28]


@functools.lru_cache(maxsize=None)
def probe(cin, alpha, L):
    """launch L of the sweep for `cin` input planes; the spike height follows alpha"""
    assert cin in (1, 3) and 0 <= L < launches(cin)
    seed = 100000 * cin + (50000 if alpha == lo.BIG_ALPHA else 0) + 10 * L
    g = lo._gen(seed)
    bstar = L % B
    centres = [CENTRES[(cin * L + ci) % len(CENTRES)] for ci in range(cin)]
    k = [((L + 2 * ci) % 7) - 3 for ci in range(cin)]

    p1 = lo.random_pixels(B * NWIN, C, 3.0, seed + 1, signed=True).reshape(B, NWIN, C).clone()
    # the spike probes, in their own pixel order (a spiked pixel next to an all-ones one in
    # lane order), over the middle and last window rows of the first patch; the first row
    # of the patch keeps random values
    spikes = lo.spike_probes(C, alpha, signed=True).roll((SPIKE_ROLL * L) % (2 * C + 2), 0)
    r0, c0 = centres[0]
    w0 = 14 * ((r0 - 1) // 2) + max((c0 - 3) // 2, 0) - 1
    w0 = max(0, min(NWIN - spikes.shape[0], w0))
    p1[bstar, w0:w0 + spikes.shape[0]] = spikes
    p1 = p1.reshape(B, 14, 14, C)
    dn = lo.grads((B, 14, 14, C), seed + 2)
    codes = torch.randint(0, 5, (B, 14, 14, C), generator=g, dtype=torch.uint8)

    x = torch.zeros(B, 28, 28, cin, dtype=torch.float64)
    for ci, (r, c) in enumerate(centres):
        x[bstar, r, c, ci] = 2.0 ** k[ci]
    for ci, yp, xp in reached(centres):
        rows, cols = _inside(yp, centres[ci][0]), _inside(xp, centres[ci][1])
        assert rows and cols
        rb = torch.tensor(rows)[torch.randint(0, len(rows), (C,), generator=g)]
        cb = torch.tensor(cols)[torch.randint(0, len(cols), (C,), generator=g)]
        code = (2 * rb + cb).to(torch.uint8)
        off = torch.rand(C, generator=g) < 1.0 / 16.0
        codes[bstar, yp, xp] = torch.where(off, torch.full_like(code, 4), code)
    xb = x.to(torch.bfloat16)
    assert torch.equal(xb.double(), x)
    return Probe(cin, xb, p1, dn, codes, bstar, centres, k)


def reference(pr, bias, alpha, beta):
    """(dP1, A) [pixels, 32] in float64: dn is dense, so the scale is the element's own
    window's (vector_scale=False)"""
    x, g = pr.lrn_inputs()
    _, dx, _, A = lo.lrn_ref(x, g, R, bias, alpha, beta, False, vector_scale=False)
    return dx, A


def expected(pr, bias, alpha, beta, ref=None):
    """(ref, A, mask): the float64 dW / 2**k, the budget's scale per element and the mask of
    observed elements; ref: `reference` of the same arguments, if the caller has it"""
    dx, A = ref if ref is not None else reference(pr, bias, alpha, beta)
    mask = pr.observe(torch.ones(B, 14, 14, C, dtype=torch.float64)) > 0
    return pr.observe(dx.reshape(B, 14, 14, C)), pr.observe(A.reshape(B, 14, 14, C)), mask


def element_budget(ref, A, c):
    """bound on |bf16(v) - ref| for any fp32 v with |v - ref| <= c 2**-23 A: the fp32 part
    plus half a bf16 ulp at the largest magnitude v can have"""
    f = c * lo.U23 * A
    return f + lo.half_ulp_bf16(ref.abs() + f)


def bias_expected(pr, bias, alpha, beta, c, ref=None):
    """(ref, tol) [32]: db sums the bf16 dP1 of every active window of all B images in fp32.
    tol = the sum of the elements' budgets + B * 196 * 2**-23 * sum |terms| for the
    accumulation (any order, one rounding of at most 2**-24 relative per partial sum and as
    much again for the MFMA's internal alignment)."""
    dx, A = ref if ref is not None else reference(pr, bias, alpha, beta)
    act = (pr.codes.reshape(-1, C) != 4).double()
    eb = element_budget(dx, A, c) * act
    terms = (dx.abs() * act + eb).sum(0)
    return (dx * act).sum(0), eb.sum(0) + B * NWIN * lo.U23 * terms


class Coverage:
    """what a sweep observes with a non-zero scale"""

    def __init__(self):
        self.windows, self.groups, self.slots = set(), set(), set()

    def add(self, pr, A):
        """A: the observed scale [5, 5, cin, 32] of `expected`"""
        widx = torch.arange(1, NWIN + 1, dtype=torch.float64).view(1, 14, 14, 1).expand(B, 14, 14, C)
        w = pr.observe(widx)
        seen = (A > 0) & (w > 0)
        self.windows.update(int(v) - 1 for v in w[seen].unique())
        self.groups.update(int(v) // 8 for v in seen.nonzero()[:, 3].unique())
        if bool(seen.any()):
            self.slots.add(pr.bstar)

    def check(self):
        assert self.windows == set(range(NWIN)), sorted(set(range(NWIN)) - self.windows)
        assert self.groups == set(range(C // 8)), self.groups
        assert self.slots == set(range(B)), self.slots
