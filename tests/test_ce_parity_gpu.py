"""Bitwise parity of the softmax cross-entropy kernels -- softmax_ce_k, softmax_ce_rows_k, softmax_ce_f32_k,
ce_tail_k, mlp_head_k, every label-target form (plain, smoothed, two-label, dropped; gradient and eval) --
with the build that wrote ``tests/golden/ce_parity.json``.

Every launch runs on fixed inputs drawn from the host generator and the raw bytes of everything it wrote
(whole buffers, rows >= nb included, and stats[0..5]) are hashed; the digests must equal the fixture's.
The kernels are deterministic in the ``ticket`` and ``defer`` statistics modes; the generic kernel
(ld 24) adds one loss per wave atomically, so beyond two waves its stats[0] is left out and its dl is still
compared.  A mismatch
means that an expression of a kernel changed shape (another contraction, another order of a sum).

    MNISTX_WRITE_GOLDEN=1 [MNISTX_GOLDEN_COMMIT=<hash>] pytest tests/test_ce_parity_gpu.py

rewrites the fixture from the build it runs on (it records that commit and the device's name).

Batch sizes: 1 (a single row), 33 (a partial second 32-row wave tile), 77 (two ce_tail_k blocks), 300 (two
mlp_head_k blocks, two softmax_ce_rows_k blocks).
"""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ce_parity.json")
NBS = [1, 33, 77, 300]
EXTRA = 8                # buffer rows past nb: they keep their sentinel, and the digest says so
SENT = -776.0
# (name, label_smoothing or None, two labels)
TARGETS = [("plain", None, False), ("smooth", 0.1, False), ("mix0", 0.0, True), ("mix", 0.1, True)]
DROP = dict(dropout=0.2, drop_seed=1234567, drop_layer3=4, drop_layer4=5)


def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:16]


def _labels(g, n):
    y = torch.randint(0, 10, (n,), generator=g, dtype=torch.int32)
    y2 = torch.randint(0, 10, (n,), generator=g, dtype=torch.int32)
    y2[2::5] = y[2::5]                                  # rows with ya == yb
    lam = 0.5 + 0.5 * torch.rand(n, generator=g)
    lam[::4], lam[1::7] = 1.0, 0.5                      # rows that drop the second label, even mixes
    return y, y2, lam


def _kw(dev, eps, two, y2, lam):
    kw = {} if eps is None else {"label_smoothing": eps}
    if two:
        kw.update(labels2=y2.to(dev), lam=lam.to(dev))
    return kw


def _finalize(K, dev, stats, work, nblk):
    K.finalize_step(torch.zeros(1, dtype=torch.int64, device=dev), stats, None, None, 0, None, 0, 1, False, None,
                    work, nblk)


def _work(dev):
    return torch.zeros(4 * 1024 + 1, device=dev)


def _softmax_ce(K, dev, out):
    for nb in NBS:
        n = nb + EXTRA
        for ld, mode in [(16, "ticket"), (16, "defer"), (32, "ticket"), (32, "defer"), (24, "atomic")]:
            g = torch.Generator().manual_seed(1000 * ld + nb)
            lg = torch.full((n, ld), 1e30)
            lg[:, :10] = torch.randn(n, 10, generator=g) * 3
            y, y2, lam = _labels(g, n)
            lg, y = lg.to(dev), y.to(dev)
            for name, eps, two in TARGETS:
                for grads in (True, False):
                    stats = torch.zeros(8, device=dev)
                    work = _work(dev) if mode != "atomic" else None
                    dl = torch.full((n, ld), SENT, dtype=torch.bfloat16, device=dev) if grads else None
                    nblk = K.softmax_ce_dbias_blocks(nb, ld)
                    db = torch.full((nblk * ld,), 9.0, device=dev) if grads and nblk > 0 else None
                    ndef = K.softmax_ce(lg, ld, y, nb, 10, 1.0 / nb, dl, ld, stats, None, work,
                                        defer_stats=mode == "defer", dbias=db, **_kw(dev, eps, two, y2, lam))
                    if mode == "defer":
                        _finalize(K, dev, stats, work, ndef)
                    # one atomic add per wave: up to two of them commute, more depend on their order
                    st = stats[1:6] if mode == "atomic" and nb > 128 else stats[:6]
                    key = f"softmax_ce/ld{ld}/{mode}/{name}/{'grad' if grads else 'eval'}/nb{nb}"
                    out[key] = _digest([t for t in (dl, db, st) if t is not None])


def _f32_softmax_ce(K, dev, out):
    ld = 10
    for nb in NBS:
        n = nb + EXTRA
        g = torch.Generator().manual_seed(7000 + nb)
        lg = (torch.randn(n, ld, generator=g) * 3).to(dev)
        y = _labels(g, n)[0].to(dev)
        for name, eps, _ in TARGETS[:2]:
            for grads in (True, False):
                stats = torch.zeros(8, device=dev)
                dl = torch.full((n, ld), SENT, device=dev) if grads else None
                K.f32_softmax_ce(lg, ld, y, nb, 10, 1.0 / nb, dl, ld, stats, None, _work(dev),
                                 **({} if eps is None else {"label_smoothing": eps}))
                out[f"f32_softmax_ce/{name}/{'grad' if grads else 'eval'}/nb{nb}"] = _digest(
                    [t for t in (dl, stats[:6]) if t is not None])


def _tr(w, rows, cols):
    t = torch.zeros(rows, cols, dtype=torch.bfloat16)
    t[:w.shape[1], :w.shape[0]] = w.t()
    return t


def _ce_tail(K, dev, out):
    for nb in NBS:
        n = nb + EXTRA
        g = torch.Generator().manual_seed(3000 + nb)
        x = torch.relu(torch.randn(n, 192, generator=g)).to(torch.bfloat16).to(dev)
        wt = _tr((torch.randn(192, 10, generator=g) * 0.2).to(torch.bfloat16), 16, 192).to(dev)
        b = (torch.randn(10, generator=g) * 0.1).to(dev)
        y, y2, lam = _labels(g, n)
        y = y.to(dev)
        nblk = K.ce_tail_blocks(nb)
        for mode in ("ticket", "defer"):
            for name, eps, two, grads in [(*t, True) for t in TARGETS] + [("plain", None, False, False)]:
                o = [torch.full((n, 16), SENT, device=dev)]
                if grads:
                    o += [torch.full((n, c), SENT, dtype=torch.bfloat16, device=dev) for c in (16, 192)]
                    o += [torch.full((nblk * 16,), 9.0, device=dev)]
                stats, work = torch.zeros(8, device=dev), _work(dev)
                K.ce_tail(x, wt, b, 10, y, nb, 1.0 / nb, o[0], dl=o[1] if grads else None, dx=o[2] if grads else None,
                          stats=stats, work=work, defer_stats=mode == "defer", dbias=o[3] if grads else None,
                          **_kw(dev, eps, two, y2, lam))
                if mode == "defer":
                    _finalize(K, dev, stats, work, nblk)
                out[f"ce_tail/{mode}/{name}/{'grad' if grads else 'eval'}/nb{nb}"] = _digest(o + [stats[:6]])


def _mlp_head(K, dev, out):
    step = torch.full((1,), 5, dtype=torch.int64, device=dev)
    forms = [(n_, e, t, True, False) for n_, e, t in TARGETS] + [("plain", None, False, False, False)]
    forms += [(n_ + "+drop", e, t, True, True) for n_, e, t in (TARGETS[0], TARGETS[1], TARGETS[3])]
    for nb in NBS:
        n = nb + EXTRA
        g = torch.Generator().manual_seed(5000 + nb)
        x = torch.relu(torch.randn(n, 400, generator=g)).to(torch.bfloat16).to(dev)
        w3 = _tr((torch.randn(400, 120, generator=g) * 0.07).to(torch.bfloat16), 128, 416).to(dev)
        w4 = _tr((torch.randn(120, 84, generator=g) * 0.13).to(torch.bfloat16), 96, 128).to(dev)
        w5 = _tr((torch.randn(84, 10, generator=g) * 0.3).to(torch.bfloat16), 16, 96).to(dev)
        b3, b4, b5 = ((torch.randn(k, generator=g) * 0.1).to(dev) for k in (120, 84, 10))
        y, y2, lam = _labels(g, n)
        y = y.to(dev)
        nblk = K.mlp_head_blocks(nb)
        for mode in ("ticket", "defer"):
            for name, eps, two, grads, drop in forms:
                bf = dict(dtype=torch.bfloat16, device=dev)
                h3, h4 = torch.full((n, 120), SENT, **bf), torch.full((n, 88), SENT, **bf)
                logits = torch.full((n, 16), SENT, device=dev)
                gr = [torch.full((n, c), SENT, **bf) for c in (16, 88, 120, 400)] if grads else [None] * 4
                db = torch.full((nblk * 16,), 9.0, device=dev) if grads else None
                stats, work = torch.zeros(8, device=dev), _work(dev)
                kw = _kw(dev, eps, two, y2, lam)
                if drop:
                    kw.update(DROP, drop_step=step)
                K.mlp_head(x, w3, b3, 120, w4, b4, 84, w5, b5, 10, y, nb, 1.0 / nb, h3, h4, logits, dl=gr[0], dh4=gr[1],
                           dh3=gr[2], dx=gr[3], stats=stats, work=work, defer_stats=mode == "defer", dbias=db, **kw)
                if mode == "defer":
                    _finalize(K, dev, stats, work, nblk)
                out[f"mlp_head/{mode}/{name}/{'grad' if grads else 'eval'}/nb{nb}"] = _digest(
                    [t for t in (h3, h4, logits, *gr, db, stats[:6]) if t is not None])


FAMILIES = {"softmax_ce": _softmax_ce, "f32_softmax_ce": _f32_softmax_ce, "ce_tail": _ce_tail, "mlp_head": _mlp_head}


@pytest.fixture(scope="module")
def golden(dev, K):
    """The fixture; with MNISTX_WRITE_GOLDEN=1 it is first rewritten from this build."""
    if os.environ.get("MNISTX_WRITE_GOLDEN") == "1":
        digests = {}
        for fn in FAMILIES.values():
            fn(K, dev, digests)
        torch.cuda.synchronize()
        with open(GOLDEN, "w") as f:
            json.dump({"commit": os.environ.get("MNISTX_GOLDEN_COMMIT", ""), "device": torch.cuda.get_device_name(dev),
                       "digests": digests}, f, indent=0, sort_keys=True)
            f.write("\n")
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_outputs_are_bitwise_those_of_the_golden_build(dev, K, golden, family):
    got = {}
    FAMILIES[family](K, dev, got)
    want = {k: v for k, v in golden["digests"].items() if k.split("/")[0] == family}
    assert sorted(got) == sorted(want), "the fixture holds other cases than the test runs"
    wrong = [k for k in got if got[k] != want[k]]
    print(f"{family}: {len(got)} launches, {len(wrong)} differ from {golden['commit'][:12]} on {golden['device']}")
    assert not wrong, f"{len(wrong)} of {len(got)} differ from the golden build: {wrong[:20]}"
