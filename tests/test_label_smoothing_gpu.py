"""Label smoothing in the softmax cross-entropy kernels -- mlp_head_k, ce_tail_k, softmax_ce_rows_k,
softmax_ce_k and softmax_ce_f32_k with their SMOOTH switch -- against a float64 oracle written
from the formulas (tests/label_smoothing_oracle.py), evaluated on the kernels' own fp32 logits:

    q_c = (1 - eps) [c == y] + eps / 10,  loss = -sum_c q_c log p_c,  dl_c = (p_c - q_c) * scale

Tolerances are the project's: the loss sum ``ce_tol`` (1e-4 |ce| + 1e-4), the bf16 dlogits
2**-8 max|g|, the fp32 dlogits 1e-5 max|g| + 1e-6, dbias 1e-2 max_c sum|g| + 1e-6.

The NaN-flag tests write NaN / inf *values* and read a flag; nothing here provokes a fault.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
from distributed_tensorflow_ibm_mnist_amd.runtime.executor_f32 import HipNetF32
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("label_smoothing_oracle",
                                               os.path.join(ROOT, "tests", "label_smoothing_oracle.py"))
lso = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lso)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SENT = -776.0            # exact in fp32 and bf16
PAD = 1e30               # what the padded logit columns hold: large, finite, and never to be read
EPS = [0.1, 0.5]
NBS = [1, 77, 300]
EXTRA = 40               # buffer rows past nb


def rel_err(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _work(dev):
    return torch.zeros(4 * 1024 + 1, device=dev)


def _finalize(K, dev, stats, work, nblk):
    """The step's combine of deferred per-block partials; batch 1: stats[4], [5] are the sums."""
    K.finalize_step(torch.zeros(1, dtype=torch.int64, device=dev), stats, None, None, 0, None, 0, 1, False, None,
                    work, nblk)


# ------------------------------------------------------------------ 1, 2. the layered kernels
def _ce_launch(K, dev, kind, logits, ld, y, nb, mode, scale, eps, grads=True, dbias=False):
    """softmax_ce (rows kernel at ld 16 / 32, generic otherwise) or f32_softmax_ce with
    ``label_smoothing=eps`` (None: the keyword is not passed).  Returns (loss sum, count, flag,
    dl, dbias column sums or None)."""
    kw = {} if eps is None else {"label_smoothing": eps}
    stats = torch.zeros(8, device=dev)
    work = _work(dev) if mode in ("ticket", "defer") else None
    n = logits.shape[0]
    db = None
    if kind == "f32":
        dl = torch.full((n, ld), SENT, device=dev) if grads else None
        K.f32_softmax_ce(logits, ld, y, nb, 10, scale, dl, ld, stats, None, work, **kw)
    else:
        dl = torch.full((n, ld), SENT, dtype=torch.bfloat16, device=dev) if grads else None
        nblk = K.softmax_ce_dbias_blocks(nb, ld)
        if dbias and nblk > 0:
            db = torch.full((nblk * ld,), 9.0, device=dev)
        ndef = K.softmax_ce(logits, ld, y, nb, 10, scale, dl, ld, stats, None, work, defer_stats=mode == "defer",
                            dbias=db, **kw)
        if mode == "defer":
            assert ndef > 0 and stats[:3].tolist() == [0.0, 0.0, 0.0]
            _finalize(K, dev, stats, work, ndef)
        if db is not None:
            db = db.view(nblk, ld).sum(0)
    torch.cuda.synchronize()
    st = stats.tolist()
    if mode == "defer":
        st[0], st[1] = st[4], st[5]
    return st[0], st[1], st[2], dl, db


# (kernel, row stride, statistics path): the rows kernel's three combines, the generic kernel's
# atomics, the fp32 kernel's ticket and atomic paths
CE_KERNELS = [("bf16", 16, "ticket"), ("bf16", 16, "defer"), ("bf16", 16, "atomic"), ("bf16", 32, "ticket"),
              ("bf16", 32, "defer"), ("bf16", 24, "atomic"), ("f32", 10, "ticket"), ("f32", 10, "atomic")]
CE_IDS = [f"{k}-ld{l}-{m}" for k, l, m in CE_KERNELS]


def _logits(dev, nb, ld, seed):
    """Ordinary logits in columns < 10 of nb + EXTRA rows; PAD in the padded columns."""
    torch.manual_seed(seed)
    n = nb + EXTRA
    lg = torch.full((n, ld), PAD, device=dev)
    lg[:, :10] = torch.randn(n, 10, device=dev) * 3
    y = torch.randint(0, 10, (n,), device=dev, dtype=torch.int32)
    return lg, y


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("kind,ld,mode", CE_KERNELS, ids=CE_IDS)
@pytest.mark.parametrize("nb", NBS)
def test_softmax_ce_smoothed(dev, K, nb, kind, ld, mode, eps):
    """Cases 1 and 2.  Loss, count, flag, dlogits and (rows kernel) dbias of the smoothed
    instantiations.  The padded columns >= 10 of the input hold 1e30: they enter neither se, the
    class sum nor dl (dl[:, 10:] is all zero and the loss is that of the 10 real columns); rows
    >= nb keep their sentinel."""
    lg, y = _logits(dev, nb, ld, 1000 + nb)
    scale = 1.0 / nb
    loss, corr, bad, dl, db = _ce_launch(K, dev, kind, lg, ld, y, nb, mode, scale, eps, dbias=True)
    z, lab = lg[:nb, :10], y[:nb]
    ce = lso.ce_sum(z, lab, eps)
    print(f"{kind} ld={ld} {mode} nb={nb} eps={eps}: loss {loss!r} vs float64 {ce!r} (tol {lso.ce_tol(ce):.3e})")
    assert bad == 0.0
    lso.check_ce(loss, ce, "smoothed loss")
    assert corr == lso.top1_count(z, lab)
    what = f"{kind} ld={ld} nb={nb} eps={eps}"
    if kind == "f32":
        g = lso.check_dlogits_f32(dl[:nb, :10], z, lab, scale, eps, what)
    else:
        g = lso.check_dlogits(dl[:nb, :10], z, lab, scale, eps, what)
        assert not dl[:nb, 10:].any(), "padded columns reached dl"
    assert bool((dl[nb:] == SENT).all()), "dl rows >= nb were written"
    if db is not None:
        lso.check_dbias(db[:10], g, what)
        assert not db[10:].any()


# ------------------------------------------------------------------ 3. ce_tail
def _tail_inputs(dev, nb, wscale=0.2):
    torch.manual_seed(nb)
    n = nb + EXTRA
    x = torch.relu(torch.randn(n, 192, device=dev)).to(torch.bfloat16)
    w = (torch.randn(192, 10, device=dev) * wscale).to(torch.bfloat16)
    wt = torch.zeros(16, 192, dtype=torch.bfloat16, device=dev)
    wt[:10] = w.t()
    b = torch.randn(10, device=dev) * 0.1
    y = torch.randint(0, 9, (n,), device=dev, dtype=torch.int32)
    y[nb - 1] = 9
    return x, w, wt, b, y


def _run_tail(K, dev, x, wt, b, y, nb, eps, mode="ticket"):
    """One gradient-form ce_tail launch over sentinel-filled outputs of nb + EXTRA rows."""
    kw = {} if eps is None else {"label_smoothing": eps}
    n = x.shape[0]
    out = {"logits": torch.full((n, 16), SENT, device=dev),
           "dl": torch.full((n, 16), SENT, dtype=torch.bfloat16, device=dev),
           "dx": torch.full((n, 192), SENT, dtype=torch.bfloat16, device=dev)}
    stats, work = torch.zeros(8, device=dev), _work(dev)
    nblk = K.ce_tail_blocks(nb)
    dbias = torch.full((nblk * 16,), 9.0, device=dev)
    K.ce_tail(x, wt, b, 10, y, nb, 1.0 / nb, out["logits"], dl=out["dl"], dx=out["dx"], stats=stats, work=work,
              defer_stats=mode == "defer", dbias=dbias, **kw)
    if mode == "defer":
        assert stats[:3].tolist() == [0.0, 0.0, 0.0]
        _finalize(K, dev, stats, work, nblk)
    torch.cuda.synchronize()
    st = stats.tolist()
    if mode == "defer":
        st[0], st[1] = st[4], st[5]
    out["dbias"] = dbias.view(nblk, 16).sum(0)
    out["dbias_blocks"] = dbias
    return st, out


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("mode", ["ticket", "defer"])
@pytest.mark.parametrize("nb", NBS)
def test_ce_tail_smoothed(dev, K, nb, mode, eps):
    """Case 3.  ce_tail_k<.., SMOOTH>: dl, dbias, the loss and the count from the kernel's own
    logits; dx from the kernel's own bf16 dl with the 2**-7 rule of test_ce_tail_matches_oracle;
    rows >= nb of every output keep their sentinel."""
    x, w, wt, b, y = _tail_inputs(dev, nb)
    st, o = _run_tail(K, dev, x, wt, b, y, nb, eps, mode)
    z, lab, scale = o["logits"][:nb, :10], y[:nb], 1.0 / nb
    ref = x[:nb].float() @ w.float() + b
    assert (z - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-5
    assert not o["logits"][:nb, 10:].any()
    ce = lso.ce_sum(z, lab, eps)
    print(f"ce_tail {mode} nb={nb} eps={eps}: loss {st[0]!r} vs float64 {ce!r} (tol {lso.ce_tol(ce):.3e})")
    assert st[2] == 0.0
    lso.check_ce(st[0], ce, "ce_tail")
    cnt = lso.top1_count(z, lab)
    assert round(st[1]) == cnt and abs(st[1] - cnt) < 1e-3
    g = lso.check_dlogits(o["dl"][:nb, :10], z, lab, scale, eps, "ce_tail")
    assert not o["dl"][:nb, 10:].any()
    lso.check_dbias(o["dbias"][:10], g, "ce_tail")
    gx = (o["dl"][:nb, :10].float() @ w.float().t()) * (x[:nb].float() > 0)
    assert (o["dx"][:nb].float() - gx).abs().max().item() <= 2 ** -7 * gx.abs().max().item()
    assert not o["dx"][:nb][x[:nb] == 0].any()
    for k in ("logits", "dl", "dx"):
        assert bool((o[k][nb:] == SENT).all()), f"ce_tail wrote {k} rows >= nb"


# ------------------------------------------------------------------ 4. mlp_head
def _head_inputs(dev, nb, seed=None):
    """A LeNet-5 head on random post-ReLU inputs: bf16 weights, their zero-padded transposes."""
    torch.manual_seed(500 + nb if seed is None else seed)
    n = nb + EXTRA
    x = torch.relu(torch.randn(n, 400, device=dev)).to(torch.bfloat16)
    w3 = (torch.randn(400, 120, device=dev) * 0.07).to(torch.bfloat16)
    w4 = (torch.randn(120, 84, device=dev) * 0.13).to(torch.bfloat16)
    w5 = (torch.randn(84, 10, device=dev) * 0.3).to(torch.bfloat16)
    b3, b4, b5 = (torch.randn(k, device=dev) * 0.1 for k in (120, 84, 10))
    y = torch.randint(0, 9, (n,), device=dev, dtype=torch.int32)
    y[nb - 1] = 9
    return {"x": x, "w3": w3, "w4": w4, "w5": w5, "b3": b3, "b4": b4, "b5": b5, "y": y}


def _tr(w, rows, cols):
    t = torch.zeros(rows, cols, dtype=torch.bfloat16, device=w.device)
    t[:w.shape[1], :w.shape[0]] = w.t()
    return t


def _run_head(K, dev, p, nb, eps, mode="ticket"):
    kw = {} if eps is None else {"label_smoothing": eps}
    n = p["x"].shape[0]
    bf = dict(dtype=torch.bfloat16, device=dev)
    o = {"h3": torch.full((n, 120), SENT, **bf), "h4": torch.full((n, 88), SENT, **bf),
         "logits": torch.full((n, 16), SENT, device=dev), "dl": torch.full((n, 16), SENT, **bf),
         "dh4": torch.full((n, 88), SENT, **bf), "dh3": torch.full((n, 120), SENT, **bf),
         "dx": torch.full((n, 400), SENT, **bf)}
    stats, work = torch.zeros(8, device=dev), _work(dev)
    nblk = K.mlp_head_blocks(nb)
    dbias = torch.full((nblk * 16,), 9.0, device=dev)
    K.mlp_head(p["x"], _tr(p["w3"], 128, 416), p["b3"], 120, _tr(p["w4"], 96, 128), p["b4"], 84,
               _tr(p["w5"], 16, 96), p["b5"], 10, p["y"], nb, 1.0 / nb, o["h3"], o["h4"], o["logits"],
               dl=o["dl"], dh4=o["dh4"], dh3=o["dh3"], dx=o["dx"], stats=stats, work=work,
               defer_stats=mode == "defer", dbias=dbias, **kw)
    if mode == "defer":
        assert stats[:3].tolist() == [0.0, 0.0, 0.0]
        _finalize(K, dev, stats, work, nblk)
    torch.cuda.synchronize()
    st = stats.tolist()
    if mode == "defer":
        st[0], st[1] = st[4], st[5]
    o["dbias"] = dbias.view(nblk, 16).sum(0)
    o["dbias_blocks"] = dbias
    return st, o


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("mode", ["ticket", "defer"])
@pytest.mark.parametrize("nb", [1, 33, 77])
def test_mlp_head_smoothed(dev, K, nb, mode, eps):
    """Case 4.  mlp_head_k<.., SMOOTH>: the checks of ce_tail on the kernel's own logits, and the
    data-gradient chain against the layered composition built from the kernel's own bf16 dl
    (dh4 = (dl W5^T) [h4 > 0], dh3 = (dh4 W4^T) [h3 > 0], dx = dh3 W3^T, each rounded to bf16 as
    the layered kernels store it) with test_mlp_head_gpu.py's bounds: logits and activations
    1e-2, gradients 2e-2 relative; dx from the kernel's own dh3 (one product, as ce_tail's dx
    from dl) with the 2**-7 rule."""
    p = _head_inputs(dev, nb)
    st, o = _run_head(K, dev, p, nb, eps, mode)
    x = p["x"][:nb].float()
    w3, w4, w5 = p["w3"].float(), p["w4"].float(), p["w5"].float()
    h3 = torch.relu(x @ w3 + p["b3"]).to(torch.bfloat16)
    h4 = torch.relu(h3.float() @ w4 + p["b4"]).to(torch.bfloat16)
    ref = h4.float() @ w5 + p["b5"]
    assert rel_err(o["h3"][:nb], h3) < 1e-2 and rel_err(o["h4"][:nb, :84], h4) < 1e-2
    assert not o["h4"][:nb, 84:].any()
    z, lab, scale = o["logits"][:nb, :10], p["y"][:nb], 1.0 / nb
    assert rel_err(z, ref) < 1e-2 and not o["logits"][:nb, 10:].any()
    ce = lso.ce_sum(z, lab, eps)
    print(f"mlp_head {mode} nb={nb} eps={eps}: loss {st[0]!r} vs float64 {ce!r} (tol {lso.ce_tol(ce):.3e})")
    assert st[2] == 0.0
    lso.check_ce(st[0], ce, "mlp_head")
    cnt = lso.top1_count(z, lab)
    assert round(st[1]) == cnt and abs(st[1] - cnt) < 1e-3
    g = lso.check_dlogits(o["dl"][:nb, :10], z, lab, scale, eps, "mlp_head")
    assert not o["dl"][:nb, 10:].any()
    lso.check_dbias(o["dbias"][:10], g, "mlp_head")
    m4, m3 = o["h4"][:nb, :84].float() > 0, o["h3"][:nb].float() > 0
    dh4 = ((o["dl"][:nb, :10].float() @ w5.t()) * m4).to(torch.bfloat16)
    dh3 = ((dh4.float() @ w4.t()) * m3).to(torch.bfloat16)
    dx = dh3.float() @ w3.t()
    for name, got, want in (("dh4", o["dh4"][:nb, :84], dh4), ("dh3", o["dh3"][:nb], dh3), ("dx", o["dx"][:nb], dx)):
        e = rel_err(got, want)
        print(f"  {name}: rel err {e:.3e}")
        assert e < 2e-2, (name, e)
    assert not o["dh4"][:nb, 84:].any()
    gx = o["dh3"][:nb].float() @ w3.t()
    assert (o["dx"][:nb].float() - gx).abs().max().item() <= 2 ** -7 * gx.abs().max().item()
    for k in ("h3", "h4", "logits", "dl", "dh4", "dh3", "dx"):
        assert bool((o[k][nb:] == SENT).all()), f"mlp_head wrote {k} rows >= nb"


# ------------------------------------------------------------------ 5. eps = 0 is the plain launch
@pytest.mark.parametrize("kind,ld,mode", CE_KERNELS, ids=CE_IDS)
def test_zero_smoothing_is_bitwise_plain_softmax_ce(dev, K, kind, ld, mode):
    """Case 5.  label_smoothing=0.0 passed explicitly launches the plain instantiation: loss,
    count, dl and dbias are bitwise those of the call without the keyword."""
    nb = 300
    lg, y = _logits(dev, nb, ld, 5)
    a = _ce_launch(K, dev, kind, lg, ld, y, nb, mode, 1.0 / nb, None, dbias=True)
    b = _ce_launch(K, dev, kind, lg, ld, y, nb, mode, 1.0 / nb, 0.0, dbias=True)
    if mode != "atomic":          # the atomic path's sums depend on the order the blocks arrive in
        assert a[:3] == b[:3]
    assert torch.equal(a[3], b[3])
    assert (a[4] is None) == (b[4] is None) and (a[4] is None or torch.equal(a[4], b[4]))
    # and smoothing changes what it should
    c = _ce_launch(K, dev, kind, lg, ld, y, nb, mode, 1.0 / nb, 0.1)
    assert not torch.equal(a[3], c[3]) and c[0] != a[0]


@pytest.mark.parametrize("mode", ["ticket", "defer"])
def test_zero_smoothing_is_bitwise_plain_heads(dev, K, mode):
    """Case 5, fused heads: loss partials, dl, dbias partials and dx / dh* bitwise."""
    nb = 300
    x, w, wt, b, y = _tail_inputs(dev, nb)
    (sa, a), (sb, bb) = _run_tail(K, dev, x, wt, b, y, nb, None, mode), _run_tail(K, dev, x, wt, b, y, nb, 0.0, mode)
    assert sa == sb
    for k in ("logits", "dl", "dx", "dbias_blocks"):
        assert torch.equal(a[k], bb[k]), ("ce_tail", k)
    sc, c = _run_tail(K, dev, x, wt, b, y, nb, 0.1, mode)
    assert not torch.equal(a["dl"], c["dl"]) and sc[0] != sa[0] and torch.equal(a["logits"], c["logits"])
    p = _head_inputs(dev, nb)
    (sa, a), (sb, bb) = _run_head(K, dev, p, nb, None, mode), _run_head(K, dev, p, nb, 0.0, mode)
    assert sa == sb
    for k in ("h3", "h4", "logits", "dl", "dh4", "dh3", "dx", "dbias_blocks"):
        assert torch.equal(a[k], bb[k]), ("mlp_head", k)
    sc, c = _run_head(K, dev, p, nb, 0.1, mode)
    assert not torch.equal(a["dl"], c["dl"]) and sc[0] != sa[0] and torch.equal(a["logits"], c["logits"])


def test_bindings_validate_label_smoothing(dev, K):
    """0 <= eps < 1 and finite, checked before any launch; the fused heads take it in their
    gradient form only (a training quantity)."""
    lg, y = _logits(dev, 8, 16, 1)
    st = torch.zeros(8, device=dev)
    for bad in (1.0, -0.1, NAN, INF):
        with pytest.raises(ValueError, match="label_smoothing"):
            K.softmax_ce(lg, 16, y, 8, 10, 1.0, None, 16, st, None, label_smoothing=bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            K.f32_softmax_ce(lg, 16, y, 8, 10, 1.0, None, 16, st, None, label_smoothing=bad)
    x, w, wt, b, yt = _tail_inputs(dev, 8)
    logits = torch.zeros(8 + EXTRA, 16, device=dev)
    with pytest.raises(ValueError, match="label_smoothing"):
        K.ce_tail(x, wt, b, 10, yt, 8, 1.0, logits, stats=st, work=_work(dev), label_smoothing=1.5)
    with pytest.raises(RuntimeError, match="label_smoothing"):
        K.ce_tail(x, wt, b, 10, yt, 8, 1.0, logits, stats=st, work=_work(dev), label_smoothing=0.1)
    torch.cuda.synchronize()
    assert st.tolist() == [0.0] * 8


# ------------------------------------------------------------------ 6. large logits
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("kind,ld", [("bf16", 16), ("bf16", 24), ("bf16", 32), ("f32", 10)])
def test_large_logits_smoothed(dev, K, kind, ld, eps):
    """Case 6.  A +80 spike at the label (exp(80) alone is fine, a sum over raw l_c times eps is
    not the loss) and a row whose other classes sit at -1e4 (their differences to the maximum,
    not their exponentials, carry the smoothed loss: 9 * 1e4 * eps / 10): finite, no flag, within
    ce_tol of float64.  |l_c - mx| stays far below the 1e37 the fp32 class sum allows."""
    nb = 77
    lg, y = _logits(dev, nb, ld, 6)
    lg[3, :10] = torch.randn(10, device=dev)
    lg[3, 7] += 80.0
    y[3] = 7
    lg[nb - 1, :10] = -1e4
    lg[nb - 1, 2] = 1.5
    y[nb - 1] = 2
    mode = "ticket" if (kind == "f32" or ld in (16, 32)) else "atomic"
    scale = 1.0 / nb
    loss, corr, bad, dl, _ = _ce_launch(K, dev, kind, lg, ld, y, nb, mode, scale, eps)
    z, lab = lg[:nb, :10], y[:nb]
    ce = lso.ce_sum(z, lab, eps)
    rows = lso.ce_rows(z, lab, eps)
    print(f"{kind} ld={ld} eps={eps}: loss {loss!r} vs {ce!r}; spike row {rows[3]!r}, -1e4 row {rows[nb - 1]!r}")
    assert abs(rows[nb - 1] - 9e3 * eps) <= 1e-6 * 9e3 * eps + 2.0      # the oracle itself, by hand
    assert bad == 0.0 and np.isfinite(loss)
    lso.check_ce(loss, ce, "large logits")
    assert corr == lso.top1_count(z, lab)
    assert bool(torch.isfinite(dl[:nb].float()).all())
    (lso.check_dlogits_f32 if kind == "f32" else lso.check_dlogits)(dl[:nb, :10], z, lab, scale, eps, "large logits")


@pytest.mark.parametrize("eps", EPS)
def test_ce_tail_large_logits_smoothed(dev, K, eps):
    """Case 6 on the fused tail: weights scaled until its own |logits| pass 1e3."""
    nb = 77
    x, w, wt, b, y = _tail_inputs(dev, nb, wscale=200.0)
    st, o = _run_tail(K, dev, x, wt, b, y, nb, eps)
    z = o["logits"][:nb, :10]
    assert z.abs().max().item() >= 1e3
    assert st[2] == 0.0
    lso.check_ce(st[0], lso.ce_sum(z, y[:nb], eps), "ce_tail large logits")
    lso.check_dlogits(o["dl"][:nb, :10], z, y[:nb], 1.0 / nb, eps, "ce_tail large logits")


# ------------------------------------------------------------------ 7. the NaN flag
@pytest.mark.parametrize("kind,ld,mode", CE_KERNELS, ids=CE_IDS)
@pytest.mark.parametrize("nb", NBS)
def test_nan_flag_non_label_class_softmax_ce(dev, K, nb, kind, ld, mode):
    """Case 7.  The smoothed loss reads every class: a NaN or a +inf logit in a non-label class
    of row nb - 1 raises stats[2]; the same poison in row nb raises nothing."""
    lg, y = _logits(dev, nb, ld, 70 + nb)
    y[nb - 1], y[nb] = 9, 9
    assert _ce_launch(K, dev, kind, lg, ld, y, nb, mode, 1.0, 0.1, grads=False)[2] == 0.0
    for v in (NAN, INF):
        lp = lg.clone()
        lp[nb - 1, 2] = v
        assert _ce_launch(K, dev, kind, lp, ld, y, nb, mode, 1.0, 0.1, grads=False)[2] == 1.0, v
        lp = lg.clone()
        lp[nb, 2] = v
        loss, _, bad, _, _ = _ce_launch(K, dev, kind, lp, ld, y, nb, mode, 1.0, 0.1, grads=False)
        assert bad == 0.0, v
        lso.check_ce(loss, lso.ce_sum(lg[:nb, :10], y[:nb], 0.1), "poison past nb")


def _overflow_column(x, row, col):
    """x with column ``col`` zero except a large finite value in one row."""
    xp = x.clone()
    xp[:, col] = 0.0
    xp[row, col] = 1e20
    return xp


@pytest.mark.parametrize("mode", ["ticket", "defer"])
@pytest.mark.parametrize("nb", NBS)
def test_nan_flag_non_label_class_ce_tail(dev, K, nb, mode):
    """Case 7, ce_tail_k: input feature 5 is 1e20 in one row and 0 elsewhere, its weight to
    class 4 is 1e20 and 0 to the other classes, so that row's class-4 logit alone overflows to
    +inf (label 9).  Row nb - 1 raises the flag, row nb does not."""
    x, w, wt, b, y = _tail_inputs(dev, nb)
    y[nb] = 9
    wt[:, 5] = 0.0
    wt[4, 5] = 1e20
    st, o = _run_tail(K, dev, _overflow_column(x, nb - 1, 5), wt, b, y, nb, 0.1, mode)
    assert st[2] == 1.0
    assert bool(torch.isinf(o["logits"][nb - 1, 4])) and bool(torch.isfinite(o["logits"][nb - 1, 9]))
    assert bool(torch.isfinite(o["logits"][:nb - 1]).all())
    st, o = _run_tail(K, dev, _overflow_column(x, nb, 5), wt, b, y, nb, 0.1, mode)
    assert st[2] == 0.0 and bool(torch.isfinite(o["logits"][:nb]).all())
    lso.check_ce(st[0], lso.ce_sum(o["logits"][:nb, :10], y[:nb], 0.1), "poison past nb")


@pytest.mark.parametrize("mode", ["ticket", "defer"])
@pytest.mark.parametrize("nb", [1, 33, 77])
def test_nan_flag_non_label_class_mlp_head(dev, K, nb, mode):
    """Case 7, mlp_head_k: one chain input 7 -> fc3 unit 11 -> fc4 unit 13 -> class 4 with weights
    1e10, 1e7 and 1e3 and zeros beside it; an input of 1e20 in one row (0 in the others) stays
    finite through h3 (1e30) and h4 (1e37) and overflows in that row's class-4 logit alone."""
    p = _head_inputs(dev, nb)
    p["y"][nb] = 9
    for w, r, c, v in ((p["w3"], 7, 11, 1e10), (p["w4"], 11, 13, 1e7), (p["w5"], 13, 4, 1e3)):
        w[r, :] = 0.0
        w[:, c] = 0.0
        w[r, c] = v
    x = p["x"]
    p["x"] = _overflow_column(x, nb - 1, 7)
    st, o = _run_head(K, dev, p, nb, 0.1, mode)
    assert st[2] == 1.0
    assert bool(torch.isinf(o["logits"][nb - 1, 4])) and bool(torch.isfinite(o["logits"][nb - 1, 9]))
    assert bool(torch.isfinite(o["logits"][:nb - 1]).all())
    p["x"] = _overflow_column(x, nb, 7)
    st, o = _run_head(K, dev, p, nb, 0.1, mode)
    assert st[2] == 0.0 and bool(torch.isfinite(o["logits"][:nb]).all())
    lso.check_ce(st[0], lso.ce_sum(o["logits"][:nb, :10], p["y"][:nb], 0.1), "poison past nb")


# ------------------------------------------------------------------ 8. the tie rule
@pytest.mark.parametrize("eps", EPS)
def test_tie_rule_all_equal_counts_every_row(dev, K, eps):
    """Case 8.  All logits equal: logit[label] >= max holds in every row, whatever eps; the
    smoothed loss of such a row is log 10 for every eps."""
    nb = 77
    y = (torch.arange(nb + EXTRA, device=dev) % 10).to(torch.int32)
    for kind, ld, mode in CE_KERNELS:
        lg = torch.full((nb + EXTRA, ld), PAD, device=dev)
        lg[:, :10] = 0.25
        loss, corr, bad, _, _ = _ce_launch(K, dev, kind, lg, ld, y, nb, mode, 1.0, eps, grads=False)
        assert corr == nb and bad == 0.0, (kind, ld, mode)
        lso.check_ce(loss, nb * np.log(10.0), f"{kind} ld={ld} {mode}")
    x, _, wt, _, _ = _tail_inputs(dev, nb)
    st, o = _run_tail(K, dev, x, torch.zeros_like(wt), torch.full((10,), 0.25, device=dev), y, nb, eps)
    assert round(st[1]) == nb and abs(st[1] - nb) < 1e-3
    lso.check_ce(st[0], nb * np.log(10.0), "ce_tail")
    p = _head_inputs(dev, nb)
    p["y"] = y
    p["w5"].zero_()
    p["b5"] = torch.full((10,), 0.25, device=dev)
    st, o = _run_head(K, dev, p, nb, eps)
    assert round(st[1]) == nb and abs(st[1] - nb) < 1e-3
    lso.check_ce(st[0], nb * np.log(10.0), "mlp_head")


# ------------------------------------------------------------------ 9 - 11. the executors
B = 96
NETS = [("lenet5", 1, "bf16"), ("reference_cnn", 1, "bf16"), ("reference_cnn", 3, "bf16"), ("mlp", 1, "bf16"),
        ("reference_cnn", 1, "fp32")]
NET_IDS = [f"{m}-{c}-{p}" for m, c, p in NETS]
HEAD = {("lenet5", "bf16"): "mlp", ("reference_cnn", "bf16"): "tail", ("mlp", "bf16"): None}


def _opt(eps):
    return OptConfig(lr0=0.05, decay_steps=0, use_momentum=False, ema_max=0.9999, label_smoothing=eps)


def _net(dev, model, cin, prec, eps, batch=B, opt=None, last_scale=None):
    """``last_scale``: softmax_linear/weights times this, so that the logits leave the
    neighbourhood of 0 where the smoothed and the plain loss nearly coincide."""
    spec = get_model(model, cin)
    init = torch_ref.init_params(spec, seed=1)
    if last_scale is not None:
        init["softmax_linear/weights"] = init["softmax_linear/weights"] * last_scale
    net = (HipNetF32 if prec == "fp32" else HipNet)(spec, batch, dev, init, opt or _opt(eps))
    if prec == "bf16":
        assert net.head_kind == HEAD[(model, prec)]
    return spec, init, net


def _batch(dev, cin, n=B, seed=21):
    g = torch.Generator(device="cpu").manual_seed(seed + cin)
    x = (torch.rand(n, 28, 28, cin, generator=g) - 0.5).to(torch.bfloat16).to(dev)
    y = torch.randint(0, 10, (n,), generator=g, dtype=torch.int32).to(dev)
    return x, y


def _load(net, x, y):
    net.x0.copy_(x.to(net.x0.dtype))
    net.labels.copy_(y)


def _grad_step(net, nb, backward=True):
    net.stats.zero_()
    net.forward(nb, defer_head=True)
    net.loss_and_grad(nb)
    if backward:
        net.backward(nb)
    net.finalize(nb, increment=False)
    torch.cuda.synchronize()


@pytest.mark.parametrize("model,cin,prec", NETS, ids=NET_IDS)
def test_executor_gradients_match_smoothed_oracle(dev, K, model, cin, prec):
    """Case 9.  forward(defer_head=True); loss_and_grad(); backward() under
    OptConfig(label_smoothing=0.1): every gradient against torch_ref with
    F.cross_entropy(label_smoothing=0.1) (bf16-rounded weights for the bf16 plans) under
    test_executor_gpu._check_step's rule max(3e-2, 3 x the bf16-autocast floor); the
    cross_entropy statistic within 2e-2 max(1, ce) of the float64 smoothed mean of the kernel's
    own logits -- also for a partial batch nb = 33 (statistics only)."""
    eps = 0.1
    spec, init, net = _net(dev, model, cin, prec, eps)
    x, y = _batch(dev, cin)
    _load(net, x, y)
    _grad_step(net, B)
    rnd = (lambda v: v.to(torch.bfloat16).float()) if prec == "bf16" else (lambda v: v.float())
    p = {k: rnd(v.to(dev)).requires_grad_(True) for k, v in init.items()}
    p16 = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    lg, _ = torch_ref.forward(spec, p, x.float())
    F.cross_entropy(lg, y.long(), label_smoothing=eps).backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        l16, _ = torch_ref.forward(spec, p16, x.float())
    F.cross_entropy(l16.float(), y.long(), label_smoothing=eps).backward()
    assert rel_err(net.logits[:, :10], lg) < 3e-2
    for name in init:
        e = rel_err(net.fp.grad_view(name), p[name].grad)
        floor = rel_err(p16[name].grad, p[name].grad)
        print(f"{model}-{cin}-{prec} {name}: rel err {e:.3e} (bf16 floor {floor:.3e})")
        assert e < max(3e-2, 3.0 * floor), f"{name}: rel err {e:.3e} (bf16 floor {floor:.3e})"
    for nb in (B, 33):
        if nb != B:
            _grad_step(net, nb, backward=False)
        st = net.read_stats()
        z, lab = net.logits[:nb, :10], y[:nb]
        ce = lso.ce_sum(z, lab, eps) / nb
        plain = lso.ce_sum(z, lab, 0.0) / nb
        print(f"nb={nb}: cross_entropy {st['cross_entropy']!r} vs smoothed {ce!r} (plain {plain!r})")
        assert st["nan"] == 0.0
        assert abs(st["cross_entropy"] - ce) <= 2e-2 * max(1.0, ce)
        assert abs(st["accuracy"] * nb - lso.top1_count(z, lab)) < 1e-3


@pytest.mark.parametrize("model,cin,prec", NETS, ids=NET_IDS)
def test_eval_batch_keeps_plain_cross_entropy(dev, K, model, cin, prec):
    """Case 10.  After a smoothed training pass, eval_batch reports the plain cross-entropy of
    its own logits (ce_tol), bitwise the value of a net built with label_smoothing=0."""
    x, y = _batch(dev, cin)
    _, _, net = _net(dev, model, cin, prec, 0.1, last_scale=30.0)
    _load(net, x, y)
    _grad_step(net, B)
    st = torch.zeros(8, device=dev)
    net.eval_batch(B, st)
    _, _, plain = _net(dev, model, cin, prec, 0.0, last_scale=30.0)
    _load(plain, x, y)
    st0 = torch.zeros(8, device=dev)
    plain.eval_batch(B, st0)
    torch.cuda.synchronize()
    z = net.logits[:B, :10]
    ce, sm = lso.ce_sum(z, y, 0.0), lso.ce_sum(z, y, 0.1)
    print(f"eval loss {st[0].item()!r} vs plain {ce!r} (smoothed would be {sm!r})")
    lso.check_ce(st[0].item(), ce, "eval_batch")
    # (the reference CNN's initial logits are so small that the two losses lie within ce_tol of
    # each other; they differ by far more than an fp32 ulp, which the bitwise comparison sees)
    assert abs(sm - ce) > 1e-6 * ce, "the two losses must differ for this test to mean anything"
    assert torch.equal(st[:3], st0[:3])
    assert st[1].item() == lso.top1_count(z, y)


@pytest.mark.parametrize("model", ["lenet5", "reference_cnn"])
def test_graph_replay_equals_eager_bitwise(dev, K, model):
    """Case 11.  eps is a plain kernel argument: three steps as one eager warm-up plus two replays
    of the captured step are bitwise three eager steps."""
    from distributed_tensorflow_ibm_mnist_amd.runtime.graph import StepGraph
    steps = 3
    data = [_batch(dev, 1, 64, seed=30 + k) for k in range(steps)]
    out = []
    for graph in (False, True):
        opt = OptConfig(lr0=0.02, use_momentum=True, momentum=0.9, ema_max=0.9999, label_smoothing=0.1)
        _, _, net = _net(dev, model, 1, "bf16", 0.1, batch=64, opt=opt)
        sg = None
        for k in range(steps):
            _load(net, *data[k])
            if not graph:
                net.train_step()
            elif sg is None:
                sg = StepGraph(net.train_step, warmup=1)    # the warm-up is step 0; capture executes nothing
            else:
                sg.replay()
        torch.cuda.synchronize()
        assert int(net.fp.step.item()) == steps
        out.append([t.clone() for t in (net.fp.params, net.fp.mom, net.fp.ema, net.stats)])
    for a, b, name in zip(out[0], out[1], ("params", "momentum", "ema", "stats")):
        assert torch.equal(a, b), name
    # the statistic the steps left is the smoothed loss of the last batch
    z, y = net.logits[:, :10], data[-1][1]
    ce = lso.ce_sum(z, y, 0.1) / 64
    assert abs(out[1][3][4].item() - ce) <= 2e-2 * max(1.0, ce)


# ------------------------------------------------------------------ 12. the module
@pytest.mark.parametrize("ld", [16, 24])
def test_module_matches_torch(dev, K, ld):
    """Case 12.  ops.nn.SoftmaxCrossEntropy(10, label_smoothing=0.1): the mean loss and
    logits.grad against F.cross_entropy in fp32 with the bounds of case 1 (ce_tol on the sum,
    2**-8 max|g| on the bf16 gradient)."""
    from distributed_tensorflow_ibm_mnist_amd.ops.nn import SoftmaxCrossEntropy
    nb, eps = 77, 0.1
    torch.manual_seed(12)
    logits = torch.zeros(nb, ld, device=dev)
    logits[:, :10] = torch.randn(nb, 10, device=dev) * 3
    logits.requires_grad_(True)
    y = torch.randint(0, 10, (nb,), device=dev)
    mod = SoftmaxCrossEntropy(10, label_smoothing=eps)
    loss = mod(logits, y)
    loss.backward()
    ref_in = logits.detach()[:, :10].clone().requires_grad_(True)
    ref = F.cross_entropy(ref_in, y, label_smoothing=eps)
    ref.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() * nb - ref.item() * nb) <= lso.ce_tol(ref.item() * nb)
    g = ref_in.grad
    assert (logits.grad[:, :10] - g).abs().max().item() <= 2 ** -8 * g.abs().max().item()
    assert not logits.grad[:, 10:].any()
    assert mod.last_stats[1].item() == lso.top1_count(logits.detach()[:, :10], y)
    with pytest.raises(ValueError, match="label_smoothing"):
        SoftmaxCrossEntropy(10, label_smoothing=1.0)
