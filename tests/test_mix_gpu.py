"""Mixup and CutMix on the device: the mixing kernel (``mix.hip``: ``mix_params`` bit for bit the host's
draw, ``mix_images`` against the float64 oracle), the two-label (MIX) form of the softmax cross-entropy
kernels -- softmax_ce_rows_k, softmax_ce_k, ce_tail_k, mlp_head_k -- against the float64 oracle written
from the formulas (tests/mix_oracle.py), the executors, the loader and graph replay.

Tolerances are the project's (tests/test_label_smoothing_gpu.py): the loss sum ``ce_tol``, the bf16
dlogits 2**-8 max|g|, dbias 1e-2 max_c sum|g| + 1e-6, dx 2**-7, the head's chain 2e-2.  A mixup pixel
is held to half a bf16 ulp of the float64 reference plus 4 * E32 (E32 = 3.7e-8, computed by the oracle
and asserted by the CPU test, where two wrong kernels exceed the bound a million times).

The NaN-flag tests write NaN / inf *values* and read a flag; nothing here provokes a fault.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from distributed_tensorflow_ibm_mnist_amd.data import mix as M
from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _by_path(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mo = _by_path("mix_oracle")
lsg = _by_path("test_label_smoothing_gpu")      # its input builders: _logits, _tail_inputs, _head_inputs, _tr
lso = mo.lso

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SENT, EXTRA = lsg.SENT, lsg.EXTRA
EPS = [0.0, 0.1]
NBS = [1, 77, 300]
rel_err, _work, _finalize = lsg.rel_err, lsg._work, lsg._finalize


@pytest.fixture(scope="module")
def E32():
    return mo.e32()


def _tables(dev, ma, ca):
    T = torch.from_numpy(M.lam_table(ma)).to(dev) if ma else None
    S = torch.from_numpy(M.side_table(ca)).to(dev) if ca else None
    return T, S


# ------------------------------------------------------------------ 1. draws
DRAW_CFGS = [(1.0, 0.0, 1.0), (0.0, 1.0, 1.0), (0.2, 4.0, 1.0), (4.0, 0.2, 0.25)]


@pytest.mark.parametrize("ma,ca,pr", DRAW_CFGS)
@pytest.mark.parametrize("pos0", [0, (1 << 32) - 3, (1 << 40) + 5])
def test_draws_match_the_host_bit_for_bit(dev, K, ma, ca, pr, pos0):
    T, S = _tables(dev, ma, ca)
    cfg = M.MixConfig(ma, ca, pr, mo.SEED)       # a 40-bit seed
    kinds = set()
    for n in (1, 2, 7, 300):
        out = torch.full((n + 2, 6), -7, dtype=torch.int32, device=dev)
        K.mix_params(out[:n], pos0, mo.SEED, cfg.thr_p, lam_table=T, side_table=S)
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], M.params(cfg, pos0, n)) and np.array_equal(got[:n], mo.params(ma, ca, pr, mo.SEED, pos0, n))
        assert np.all(got[n:] == -7)
        kinds |= set(got[:n, 0].tolist())
    assert kinds >= ({M.MIXUP} if ma else set()) | ({M.CUTMIX} if ca else set())


# ------------------------------------------------------------------ 2. images
def _run_images(K, dev, nb, C, ma, ca, pr, pos0=mo.IMAGE_POS0):
    x, y = mo.image_inputs(nb, C)
    n = nb + 8
    img = torch.full((n, 784, C), SENT, dtype=torch.bfloat16, device=dev)
    img[:nb] = torch.from_numpy(x).to(dev).to(torch.bfloat16)
    assert np.array_equal(img[:nb].float().cpu().numpy(), x)        # the inputs are bf16 values
    lab = torch.full((n,), -77, dtype=torch.int32, device=dev)
    lab[:nb] = torch.from_numpy(y).to(dev)
    lab2 = torch.full((n,), -55, dtype=torch.int32, device=dev)
    lam = torch.full((n,), -3.0, device=dev)
    T, S = _tables(dev, ma, ca)
    K.mix_images(img, lab, lab2, lam, nb, C, pos0, mo.SEED, M.prob_threshold(pr), lam_table=T, side_table=S)
    torch.cuda.synchronize()
    return x, y, img, lab, lab2, lam


def _check_images(x, y, img, lab, lab2, lam, nb, ma, ca, pr, E32, what, pos0=mo.IMAGE_POS0):
    kind, wlam, box = mo.batch_draws(ma, ca, pr, mo.SEED, pos0, nb)
    got_lam = lam[:nb].cpu().numpy()
    assert np.array_equal(got_lam.view(np.uint32), wlam.view(np.uint32)), f"{what}: lam"
    ref, l2, _ = mo.mixed(x, y, kind, got_lam, box)      # the reference at the device's own lam
    assert np.array_equal(lab2[:nb].cpu().numpy(), l2), f"{what}: labels2"
    assert np.array_equal(lab[:nb].cpu().numpy(), y), f"{what}: labels were written"
    got = img[:nb].double().cpu().numpy()
    exact = kind != mo.MIXUP
    assert np.array_equal(got[exact], ref[exact]), f"{what}: CutMix / unmixed entries are not bitwise the reference"
    if (~exact).any():
        worst = float((np.abs(got[~exact] - ref[~exact]) / mo.image_bound(ref[~exact], E32)).max())
        print(f"{what}: worst mixup error / bound = {worst:.3f}")
        assert worst <= 1.0, f"{what}: worst mixup error / bound = {worst:.3f}"
    # rows >= nb of all four buffers keep their sentinel
    assert bool((img[nb:] == SENT).all()) and bool((lab[nb:] == -77).all())
    assert bool((lab2[nb:] == -55).all()) and bool((lam[nb:] == -3.0).all())
    return kind


@pytest.mark.parametrize("ma,ca,pr", mo.IMAGE_CFGS)
@pytest.mark.parametrize("C", mo.IMAGE_CS)
def test_images_match_the_oracle(dev, K, E32, C, ma, ca, pr):
    kinds = set()
    for nb in mo.IMAGE_NBS:      # its own partner, one pair, an odd batch, several groups
        out = _run_images(K, dev, nb, C, ma, ca, pr)
        kinds |= set(_check_images(*out, nb, ma, ca, pr, E32, f"C={C} nb={nb} cfg={(ma, ca, pr)}").tolist())
    assert kinds >= ({mo.MIXUP} if ma else set()) | ({mo.CUTMIX} if ca else set()) | ({mo.UNMIXED})


def test_images_grid_stride_walk_and_position(dev, K, E32, grid_cap):
    """One block walks every group (the grid-stride loop); a draw belongs to the position."""
    grid_cap(1)
    ma, ca, pr = 0.2, 4.0, 0.75
    out = _run_images(K, dev, 77, 1, ma, ca, pr)
    _check_images(*out, 77, ma, ca, pr, E32, "one block")
    grid_cap(0)
    again = _run_images(K, dev, 77, 1, ma, ca, pr)
    assert torch.equal(out[2], again[2]) and torch.equal(out[5], again[5])
    a = _run_images(K, dev, 7, 1, ma, ca, pr, pos0=5)[5][:7]
    b = torch.empty(300, 6, dtype=torch.int32, device=dev)
    K.mix_params(b, 0, mo.SEED, M.prob_threshold(pr), *_tables(dev, ma, ca))
    want = b[5:12, 1].contiguous().view(torch.float32).clone()
    want[3] = 1.0                                         # the middle entry of the batch of 7
    assert torch.equal(a, want)


def test_mix_bindings_validate(dev, K):
    T, S = _tables(dev, 1.0, 1.0)
    img = torch.zeros(8, 784, 1, dtype=torch.bfloat16, device=dev)
    lab, lab2, lam = (torch.zeros(8, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32))
    good = dict(images=img, labels=lab, labels2=lab2, lam=lam, nb=8, cdst=1, pos0=0, seed=1, thr_p=65536, lam_table=T,
                side_table=S)
    K.mix_images(**good)
    bad = [dict(lam_table=None, side_table=None), dict(lam_table=T[:1024].contiguous()), dict(lam_table=T.double()),
           dict(lam_table=T.cpu()), dict(side_table=S.long()), dict(side_table=S[:1000].contiguous()),
           dict(side_table=S.cpu()), dict(thr_p=65537), dict(thr_p=-1), dict(seed=-1), dict(pos0=-1), dict(cdst=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            K.mix_images(**{**good, **kw})
    with pytest.raises(RuntimeError):
        K.mix_images(**{**good, "nb": 9})
    with pytest.raises(RuntimeError):
        K.mix_images(**{**good, "images": img.float()})
    with pytest.raises(ValueError):
        K.mix_params(torch.zeros(4, 6, dtype=torch.int32, device=dev), 0, 1, 65536)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. the heads
CE_KERNELS = [(16, "ticket"), (16, "defer"), (16, "atomic"), (32, "ticket"), (32, "defer"), (24, "atomic")]
CE_IDS = [f"ld{l}-{m}" for l, m in CE_KERNELS]


def _second(dev, y, seed):
    """A second label and a weight per row: rows with ya == yb; weights 1.0, 0.5 and values in between."""
    rng = np.random.default_rng(seed)
    n = y.shape[0]
    yb = torch.from_numpy(rng.integers(0, 10, n).astype(np.int32)).to(dev)
    yb[2::5] = y[2::5]
    lam = torch.from_numpy(mo.lam_vector(rng, n)).to(dev)
    return yb, lam


def _mixkw(eps, y2, lam):
    kw = {} if eps is None else {"label_smoothing": eps}
    if y2 is not None:
        kw.update(labels2=y2, lam=lam)
    return kw


def _ce_launch(K, dev, logits, ld, y, nb, mode, scale, eps, y2=None, lam=None, grads=True, dbias=False):
    """softmax_ce (rows kernel at ld 16 / 32, generic otherwise): (loss sum, count, flag, dl, dbias sums)."""
    stats = torch.zeros(8, device=dev)
    work = _work(dev) if mode in ("ticket", "defer") else None
    n = logits.shape[0]
    dl = torch.full((n, ld), SENT, dtype=torch.bfloat16, device=dev) if grads else None
    nblk = K.softmax_ce_dbias_blocks(nb, ld)
    db = torch.full((nblk * ld,), 9.0, device=dev) if (dbias and nblk > 0) else None
    ndef = K.softmax_ce(logits, ld, y, nb, 10, scale, dl, ld, stats, None, work, defer_stats=mode == "defer", dbias=db,
                        **_mixkw(eps, y2, lam))
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


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("ld,mode", CE_KERNELS, ids=CE_IDS)
@pytest.mark.parametrize("nb", NBS)
def test_softmax_ce_mixed(dev, K, nb, ld, mode, eps):
    lg, y = lsg._logits(dev, nb, ld, 2000 + nb)
    y2, lam = _second(dev, y, nb)
    scale = 1.0 / nb
    loss, corr, bad, dl, db = _ce_launch(K, dev, lg, ld, y, nb, mode, scale, eps, y2, lam, dbias=True)
    z, ya, yb, lm = lg[:nb, :10], y[:nb], y2[:nb], lam[:nb]
    ce = mo.ce_sum(z, ya, yb, lm, eps)
    print(f"ld={ld} {mode} nb={nb} eps={eps}: loss {loss!r} vs float64 {ce!r} (tol {mo.ce_tol(ce):.3e})")
    assert bad == 0.0
    mo.check_ce(loss, ce, "mixed loss")
    assert corr == mo.top1_count(z, ya)
    g = mo.check_dlogits(dl[:nb, :10], z, ya, yb, lm, scale, eps, f"ld={ld} nb={nb} eps={eps}")
    assert not dl[:nb, 10:].any(), "padded columns reached dl"
    assert bool((dl[nb:] == SENT).all()), "dl rows >= nb were written"
    if db is not None:
        mo.check_dbias(db[:10], g, "softmax_ce")
        assert not db[10:].any()
    if nb > 1:      # the second label matters
        assert abs(ce - lso.ce_sum(z, ya, eps)) > 10 * mo.ce_tol(ce)


def _run_tail(K, dev, x, wt, b, y, nb, eps, y2=None, lam=None, mode="ticket"):
    n = x.shape[0]
    out = {"logits": torch.full((n, 16), SENT, device=dev),
           "dl": torch.full((n, 16), SENT, dtype=torch.bfloat16, device=dev),
           "dx": torch.full((n, 192), SENT, dtype=torch.bfloat16, device=dev)}
    stats, work = torch.zeros(8, device=dev), _work(dev)
    nblk = K.ce_tail_blocks(nb)
    dbias = torch.full((nblk * 16,), 9.0, device=dev)
    K.ce_tail(x, wt, b, 10, y, nb, 1.0 / nb, out["logits"], dl=out["dl"], dx=out["dx"], stats=stats, work=work,
              defer_stats=mode == "defer", dbias=dbias, **_mixkw(eps, y2, lam))
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
def test_ce_tail_mixed(dev, K, nb, mode, eps):
    x, w, wt, b, y = lsg._tail_inputs(dev, nb)
    y2, lam = _second(dev, y, 10 + nb)
    st, o = _run_tail(K, dev, x, wt, b, y, nb, eps, y2, lam, mode)
    z, ya, yb, lm, scale = o["logits"][:nb, :10], y[:nb], y2[:nb], lam[:nb], 1.0 / nb
    ref = x[:nb].float() @ w.float() + b
    assert (z - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-5
    assert not o["logits"][:nb, 10:].any()
    ce = mo.ce_sum(z, ya, yb, lm, eps)
    print(f"ce_tail {mode} nb={nb} eps={eps}: loss {st[0]!r} vs float64 {ce!r} (tol {mo.ce_tol(ce):.3e})")
    assert st[2] == 0.0
    mo.check_ce(st[0], ce, "ce_tail")
    cnt = mo.top1_count(z, ya)
    assert round(st[1]) == cnt and abs(st[1] - cnt) < 1e-3
    g = mo.check_dlogits(o["dl"][:nb, :10], z, ya, yb, lm, scale, eps, "ce_tail")
    assert not o["dl"][:nb, 10:].any()
    mo.check_dbias(o["dbias"][:10], g, "ce_tail")
    gx = (o["dl"][:nb, :10].float() @ w.float().t()) * (x[:nb].float() > 0)
    assert (o["dx"][:nb].float() - gx).abs().max().item() <= 2 ** -7 * gx.abs().max().item()
    assert not o["dx"][:nb][x[:nb] == 0].any()
    for k in ("logits", "dl", "dx"):
        assert bool((o[k][nb:] == SENT).all()), f"ce_tail wrote {k} rows >= nb"


def _run_head(K, dev, p, nb, eps, y2=None, lam=None, mode="ticket", **kw):
    n = p["x"].shape[0]
    bf = dict(dtype=torch.bfloat16, device=dev)
    o = {"h3": torch.full((n, 120), SENT, **bf), "h4": torch.full((n, 88), SENT, **bf),
         "logits": torch.full((n, 16), SENT, device=dev), "dl": torch.full((n, 16), SENT, **bf),
         "dh4": torch.full((n, 88), SENT, **bf), "dh3": torch.full((n, 120), SENT, **bf),
         "dx": torch.full((n, 400), SENT, **bf)}
    stats, work = torch.zeros(8, device=dev), _work(dev)
    nblk = K.mlp_head_blocks(nb)
    dbias = torch.full((nblk * 16,), 9.0, device=dev)
    tr = lsg._tr
    K.mlp_head(p["x"], tr(p["w3"], 128, 416), p["b3"], 120, tr(p["w4"], 96, 128), p["b4"], 84,
               tr(p["w5"], 16, 96), p["b5"], 10, p["y"], nb, 1.0 / nb, o["h3"], o["h4"], o["logits"],
               dl=o["dl"], dh4=o["dh4"], dh3=o["dh3"], dx=o["dx"], stats=stats, work=work,
               defer_stats=mode == "defer", dbias=dbias, **_mixkw(eps, y2, lam), **kw)
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
def test_mlp_head_mixed(dev, K, nb, mode, eps):
    p = lsg._head_inputs(dev, nb)
    y2, lam = _second(dev, p["y"], 20 + nb)
    st, o = _run_head(K, dev, p, nb, eps, y2, lam, mode)
    x = p["x"][:nb].float()
    w3, w4, w5 = p["w3"].float(), p["w4"].float(), p["w5"].float()
    h3 = torch.relu(x @ w3 + p["b3"]).to(torch.bfloat16)
    h4 = torch.relu(h3.float() @ w4 + p["b4"]).to(torch.bfloat16)
    ref = h4.float() @ w5 + p["b5"]
    assert rel_err(o["h3"][:nb], h3) < 1e-2 and rel_err(o["h4"][:nb, :84], h4) < 1e-2
    assert not o["h4"][:nb, 84:].any()
    z, ya, yb, lm, scale = o["logits"][:nb, :10], p["y"][:nb], y2[:nb], lam[:nb], 1.0 / nb
    assert rel_err(z, ref) < 1e-2 and not o["logits"][:nb, 10:].any()
    ce = mo.ce_sum(z, ya, yb, lm, eps)
    print(f"mlp_head {mode} nb={nb} eps={eps}: loss {st[0]!r} vs float64 {ce!r} (tol {mo.ce_tol(ce):.3e})")
    assert st[2] == 0.0
    mo.check_ce(st[0], ce, "mlp_head")
    cnt = mo.top1_count(z, ya)
    assert round(st[1]) == cnt and abs(st[1] - cnt) < 1e-3
    g = mo.check_dlogits(o["dl"][:nb, :10], z, ya, yb, lm, scale, eps, "mlp_head")
    assert not o["dl"][:nb, 10:].any()
    mo.check_dbias(o["dbias"][:10], g, "mlp_head")
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


@pytest.mark.parametrize("nb", [33, 77])
def test_mlp_head_mixed_with_dropout(dev, K, nb):
    """The MIX + DROP instantiation: the loss and dl of its own logits, the chain from its own dropped
    activations (h' > 0 is the kept-and-active mask), each data gradient scaled by 1 / keep."""
    from distributed_tensorflow_ibm_mnist_amd.ops import dropout as D
    eps, pdrop, t = 0.1, 0.25, 5
    p = lsg._head_inputs(dev, nb)
    y2, lam = _second(dev, p["y"], 40 + nb)
    step = torch.full((1,), t, dtype=torch.int64, device=dev)
    st, o = _run_head(K, dev, p, nb, eps, y2, lam, dropout=pdrop, drop_step=step, drop_seed=mo.SEED, drop_layer3=4,
                      drop_layer4=5)
    _, inv = D.threshold(pdrop)
    m3 = torch.from_numpy(D.keep_mask(mo.SEED, t, 4, nb, 120, pdrop)).to(dev)
    m4 = torch.from_numpy(D.keep_mask(mo.SEED, t, 5, nb, 84, pdrop)).to(dev)
    assert not o["h3"][:nb][~m3].any() and not o["h4"][:nb, :84][~m4].any()
    z, ya, yb, lm, scale = o["logits"][:nb, :10], p["y"][:nb], y2[:nb], lam[:nb], 1.0 / nb
    ref = o["h4"][:nb, :84].float() @ p["w5"].float() + p["b5"]
    assert rel_err(z, ref) < 1e-2
    assert st[2] == 0.0
    mo.check_ce(st[0], mo.ce_sum(z, ya, yb, lm, eps), "mlp_head mix + drop")
    g = mo.check_dlogits(o["dl"][:nb, :10], z, ya, yb, lm, scale, eps, "mlp_head mix + drop")
    mo.check_dbias(o["dbias"][:10], g, "mlp_head mix + drop")
    k4, k3 = o["h4"][:nb, :84].float() > 0, o["h3"][:nb].float() > 0
    dh4 = ((o["dl"][:nb, :10].float() @ p["w5"].float().t()) * k4 * inv).to(torch.bfloat16)
    dh3 = ((dh4.float() @ p["w4"].float().t()) * k3 * inv).to(torch.bfloat16)
    for name, got, want in (("dh4", o["dh4"][:nb, :84], dh4), ("dh3", o["dh3"][:nb], dh3)):
        assert rel_err(got, want) < 2e-2, name
    for k in ("h3", "h4", "logits", "dl", "dh4", "dh3", "dx"):
        assert bool((o[k][nb:] == SENT).all()), f"mlp_head wrote {k} rows >= nb"


# ------------------------------------------------------------------ 3b. the NaN flag
@pytest.mark.parametrize("ld,mode", CE_KERNELS, ids=CE_IDS)
@pytest.mark.parametrize("nb", NBS)
def test_nan_flag_softmax_ce(dev, K, nb, ld, mode):
    """A NaN (or a -inf) at class yb of row nb - 1 with lam < 1 raises the flag; the same in row nb does
    not; a -inf l_yb in a row with lam == 1 does not either (eps = 0: no class sum reads it)."""
    lg, y = lsg._logits(dev, nb, ld, 3000 + nb)
    y2, lam = _second(dev, y, nb)
    for r in (nb - 1, nb):
        y[r], y2[r], lam[r] = 9, 2, 0.75
    assert _ce_launch(K, dev, lg, ld, y, nb, mode, 1.0, 0.0, y2, lam, grads=False)[2] == 0.0
    for v in (NAN, -INF):
        lp = lg.clone()
        lp[nb - 1, 2] = v
        assert _ce_launch(K, dev, lp, ld, y, nb, mode, 1.0, 0.0, y2, lam, grads=False)[2] == 1.0, v
        lp = lg.clone()
        lp[nb, 2] = v
        loss, _, bad, _, _ = _ce_launch(K, dev, lp, ld, y, nb, mode, 1.0, 0.0, y2, lam, grads=False)
        assert bad == 0.0, v
        mo.check_ce(loss, mo.ce_sum(lg[:nb, :10], y[:nb], y2[:nb], lam[:nb], 0.0), "poison past nb")
    lp = lg.clone()
    lp[nb - 1, 2] = -INF
    lam[nb - 1] = 1.0
    loss, _, bad, dl, _ = _ce_launch(K, dev, lp, ld, y, nb, mode, 1.0, 0.0, y2, lam)
    assert bad == 0.0 and bool(torch.isfinite(dl[:nb].float()).all())
    mo.check_ce(loss, mo.ce_sum(lp[:nb, :10], y[:nb], y2[:nb], lam[:nb], 0.0), "-inf at yb, lam == 1")


@pytest.mark.parametrize("mode", ["ticket", "defer"])
@pytest.mark.parametrize("nb", NBS)
def test_nan_flag_ce_tail(dev, K, nb, mode):
    """ce_tail_k: input feature 5 is 1e20 in one row and 0 elsewhere, its weight to class 4 is -1e20 and
    0 to the other classes, so that row's class-4 logit alone is -inf; class 4 is the row's yb."""
    x, w, wt, b, y = lsg._tail_inputs(dev, nb)
    y2, lam = _second(dev, y, nb)
    for r in (nb - 1, nb):
        y[r], y2[r], lam[r] = 9, 4, 0.75
    wt[:, 5] = 0.0
    wt[4, 5] = -1e20
    st, o = _run_tail(K, dev, lsg._overflow_column(x, nb - 1, 5), wt, b, y, nb, 0.0, y2, lam, mode)
    assert st[2] == 1.0 and o["logits"][nb - 1, 4].item() == -INF and bool(torch.isfinite(o["logits"][nb - 1, 9]))
    st, o = _run_tail(K, dev, lsg._overflow_column(x, nb, 5), wt, b, y, nb, 0.0, y2, lam, mode)
    assert st[2] == 0.0 and bool(torch.isfinite(o["logits"][:nb]).all())
    mo.check_ce(st[0], mo.ce_sum(o["logits"][:nb, :10], y[:nb], y2[:nb], lam[:nb], 0.0), "poison past nb")
    lam[nb - 1] = 1.0
    st, o = _run_tail(K, dev, lsg._overflow_column(x, nb - 1, 5), wt, b, y, nb, 0.0, y2, lam, mode)
    assert st[2] == 0.0 and o["logits"][nb - 1, 4].item() == -INF
    mo.check_ce(st[0], mo.ce_sum(o["logits"][:nb, :10], y[:nb], y2[:nb], lam[:nb], 0.0), "-inf at yb, lam == 1")


@pytest.mark.parametrize("mode", ["ticket", "defer"])
@pytest.mark.parametrize("nb", [1, 33, 77])
def test_nan_flag_mlp_head(dev, K, nb, mode):
    """mlp_head_k: the chain of test_label_smoothing_gpu with -1e3 as its last weight: a -inf class-4 logit."""
    p = lsg._head_inputs(dev, nb)
    y2, lam = _second(dev, p["y"], nb)
    for r in (nb - 1, nb):
        p["y"][r], y2[r], lam[r] = 9, 4, 0.75
    for w, r, c, v in ((p["w3"], 7, 11, 1e10), (p["w4"], 11, 13, 1e7), (p["w5"], 13, 4, -1e3)):
        w[r, :] = 0.0
        w[:, c] = 0.0
        w[r, c] = v
    x = p["x"]
    p["x"] = lsg._overflow_column(x, nb - 1, 7)
    st, o = _run_head(K, dev, p, nb, 0.0, y2, lam, mode)
    assert st[2] == 1.0 and o["logits"][nb - 1, 4].item() == -INF and bool(torch.isfinite(o["logits"][nb - 1, 9]))
    lam1 = lam.clone()
    lam1[nb - 1] = 1.0
    st, o = _run_head(K, dev, p, nb, 0.0, y2, lam1, mode)
    assert st[2] == 0.0 and o["logits"][nb - 1, 4].item() == -INF
    mo.check_ce(st[0], mo.ce_sum(o["logits"][:nb, :10], p["y"][:nb], y2[:nb], lam1[:nb], 0.0), "-inf at yb, lam == 1")
    p["x"] = lsg._overflow_column(x, nb, 7)
    st, o = _run_head(K, dev, p, nb, 0.0, y2, lam, mode)
    assert st[2] == 0.0 and bool(torch.isfinite(o["logits"][:nb]).all())
    mo.check_ce(st[0], mo.ce_sum(o["logits"][:nb, :10], p["y"][:nb], y2[:nb], lam[:nb], 0.0), "poison past nb")


# ------------------------------------------------------------------ 4. the plain path is unchanged
@pytest.mark.parametrize("ld,mode", CE_KERNELS, ids=CE_IDS)
def test_absent_keywords_are_the_plain_launch_softmax_ce(dev, K, ld, mode):
    """Without the keywords (or with both None) the launch is the plain one, held to the plain oracle and
    bitwise itself; labels2 = labels, lam = 1 is the mixed instantiation, held to the same oracle."""
    nb = 300
    lg, y = lsg._logits(dev, nb, ld, 5)
    z, lab, scale = lg[:nb, :10], y[:nb], 1.0 / nb
    for eps in (None, 0.1):
        e = eps or 0.0
        a = _ce_launch(K, dev, lg, ld, y, nb, mode, scale, eps, dbias=True)
        stats = torch.zeros(8, device=dev)
        dl = torch.full_like(a[3], SENT)
        K.softmax_ce(lg, ld, y, nb, 10, scale, dl, ld, stats, None, None, label_smoothing=e, labels2=None, lam=None)
        assert torch.equal(dl, a[3])
        b = _ce_launch(K, dev, lg, ld, y, nb, mode, scale, e, y.clone(), torch.ones(lg.shape[0], device=dev), dbias=True)
        for r in (a, b):
            lso.check_ce(r[0], lso.ce_sum(z, lab, e), "plain path")
            assert r[1] == lso.top1_count(z, lab) and r[2] == 0.0
            lso.check_dlogits(r[3][:nb, :10], z, lab, scale, e, "plain path")
            assert bool((r[3][nb:] == SENT).all())


@pytest.mark.parametrize("mode", ["ticket", "defer"])
def test_absent_keywords_are_the_plain_launch_heads(dev, K, mode):
    nb = 300
    x, w, wt, b, y = lsg._tail_inputs(dev, nb)
    ones = torch.ones(nb + EXTRA, device=dev)
    (sa, a), (sb, bb) = _run_tail(K, dev, x, wt, b, y, nb, None, mode=mode), lsg._run_tail(K, dev, x, wt, b, y, nb, None, mode)
    assert sa == sb
    for k in ("logits", "dl", "dx", "dbias_blocks"):
        assert torch.equal(a[k], bb[k]), ("ce_tail", k)
    sc, c = _run_tail(K, dev, x, wt, b, y, nb, 0.0, y.clone(), ones, mode)
    assert torch.equal(a["logits"], c["logits"])
    z = c["logits"][:nb, :10]
    lso.check_ce(sc[0], lso.ce_sum(z, y[:nb], 0.0), "ce_tail lam = 1")
    lso.check_dlogits(c["dl"][:nb, :10], z, y[:nb], 1.0 / nb, 0.0, "ce_tail lam = 1")
    p = lsg._head_inputs(dev, nb)
    (sa, a), (sb, bb) = _run_head(K, dev, p, nb, None, mode=mode), lsg._run_head(K, dev, p, nb, None, mode)
    assert sa == sb
    for k in ("h3", "h4", "logits", "dl", "dh4", "dh3", "dx", "dbias_blocks"):
        assert torch.equal(a[k], bb[k]), ("mlp_head", k)
    sc, c = _run_head(K, dev, p, nb, 0.0, p["y"].clone(), ones, mode)
    assert torch.equal(a["logits"], c["logits"]) and torch.equal(a["h3"], c["h3"])
    z = c["logits"][:nb, :10]
    lso.check_ce(sc[0], lso.ce_sum(z, p["y"][:nb], 0.0), "mlp_head lam = 1")
    lso.check_dlogits(c["dl"][:nb, :10], z, p["y"][:nb], 1.0 / nb, 0.0, "mlp_head lam = 1")


def test_bindings_validate_the_pair(dev, K):
    lg, y = lsg._logits(dev, 8, 16, 1)
    st = torch.zeros(8, device=dev)
    lam = torch.ones(8 + EXTRA, device=dev)
    with pytest.raises(ValueError, match="labels2"):
        K.softmax_ce(lg, 16, y, 8, 10, 1.0, None, 16, st, None, labels2=y)
    with pytest.raises(ValueError, match="lam"):
        K.softmax_ce(lg, 16, y, 8, 10, 1.0, None, 16, st, None, lam=lam)
    x, w, wt, b, yt = lsg._tail_inputs(dev, 8)
    logits = torch.zeros(8 + EXTRA, 16, device=dev)
    with pytest.raises(ValueError, match="labels2"):
        K.ce_tail(x, wt, b, 10, yt, 8, 1.0, logits, stats=st, work=_work(dev), labels2=yt)
    with pytest.raises(RuntimeError, match="labels2"):      # the fused heads: the gradient form only
        K.ce_tail(x, wt, b, 10, yt, 8, 1.0, logits, stats=st, work=_work(dev), labels2=yt, lam=lam)
    from distributed_tensorflow_ibm_mnist_amd.ops import functional as Fk
    with pytest.raises(ValueError, match="labels2"):
        Fk.softmax_ce(lg, y, 10, labels2=y)
    torch.cuda.synchronize()
    assert st.tolist() == [0.0] * 8


def test_module_takes_two_labels(dev, K):
    from distributed_tensorflow_ibm_mnist_amd.ops.nn import SoftmaxCrossEntropy
    nb, eps = 77, 0.1
    torch.manual_seed(12)
    logits = torch.zeros(nb, 16, device=dev)
    logits[:, :10] = torch.randn(nb, 10, device=dev) * 3
    logits.requires_grad_(True)
    y = torch.randint(0, 10, (nb,), device=dev)
    y2, lam = _second(dev, y, 3)
    mod = SoftmaxCrossEntropy(10, label_smoothing=eps)
    loss = mod(logits, y, y2, lam)
    loss.backward()
    ref_in = logits.detach()[:, :10].clone().requires_grad_(True)
    ref = torch_ref.two_label_cross_entropy(ref_in, y, y2, lam, eps).mean()
    ref.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() * nb - ref.item() * nb) <= mo.ce_tol(ref.item() * nb)
    g = ref_in.grad
    assert (logits.grad[:, :10] - g).abs().max().item() <= 2 ** -8 * g.abs().max().item()
    assert mod.last_stats[1].item() == mo.top1_count(logits.detach()[:, :10], y)
    with pytest.raises(ValueError, match="lam"):
        mod(logits, y, y2)


# ------------------------------------------------------------------ 5. the executors
B = 96
NETS = [("lenet5", 1), ("reference_cnn", 1), ("reference_cnn", 3), ("mlp", 1)]
NET_IDS = [f"{m}-{c}" for m, c in NETS]
HEAD = {"lenet5": "mlp", "reference_cnn": "tail", "mlp": None}


def _opt(mix, eps=0.1, **kw):
    return OptConfig(lr0=0.05, decay_steps=0, use_momentum=False, ema_max=0.9999, label_smoothing=eps, mix=mix, **kw)


def _net(dev, model, cin, opt, batch=B, last_scale=None):
    spec = get_model(model, cin)
    init = torch_ref.init_params(spec, seed=1)
    if last_scale is not None:
        init["softmax_linear/weights"] = init["softmax_linear/weights"] * last_scale
    net = HipNet(spec, batch, dev, init, opt)
    assert net.head_kind == HEAD[model]
    assert (net.labels2 is not None) == opt.mix and (net.mix_lam is not None) == opt.mix
    return spec, init, net


def _load(net, x, y, y2=None, lam=None):
    net.x0.copy_(x)
    net.labels.copy_(y)
    if y2 is not None:
        net.labels2.copy_(y2)
        net.mix_lam.copy_(lam)


@pytest.mark.parametrize("model,cin", NETS, ids=NET_IDS)
def test_executor_gradients_match_the_two_label_oracle(dev, K, model, cin):
    """forward(defer_head=True); loss_and_grad(); backward() under OptConfig(mix=True, label_smoothing=0.1):
    every gradient against torch_ref with the two-label loss under test_executor_gpu._check_step's rule
    max(3e-2, 3 x the bf16-autocast floor); the cross_entropy statistic within 2e-2 max(1, ce) of the
    float64 mean on the kernel's own logits; eval_batch afterwards bitwise that of a net without the key."""
    eps = 0.1
    spec, init, net = _net(dev, model, cin, _opt(True, eps))
    x, y = lsg._batch(dev, cin)
    y2, lam = _second(dev, y, 50 + cin)
    _load(net, x, y, y2, lam)
    lsg._grad_step(net, B)
    p = {k: v.to(dev).to(torch.bfloat16).float().requires_grad_(True) for k, v in init.items()}
    p16 = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    lg, _ = torch_ref.forward(spec, p, x.float())
    torch_ref.losses(spec, p, lg, y, eps, labels2=y2, lam=lam)["cross_entropy"].backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        l16, _ = torch_ref.forward(spec, p16, x.float())
    torch_ref.two_label_cross_entropy(l16.float(), y, y2, lam, eps).mean().backward()
    assert rel_err(net.logits[:, :10], lg) < 3e-2
    for name in init:
        e = rel_err(net.fp.grad_view(name), p[name].grad)
        floor = rel_err(p16[name].grad, p[name].grad)
        print(f"{model}-{cin} {name}: rel err {e:.3e} (bf16 floor {floor:.3e})")
        assert e < max(3e-2, 3.0 * floor), f"{name}: rel err {e:.3e} (bf16 floor {floor:.3e})"
    st = net.read_stats()
    z = net.logits[:B, :10]
    ce, hard = mo.ce_sum(z, y, y2, lam, eps) / B, lso.ce_sum(z, y, eps) / B
    print(f"cross_entropy {st['cross_entropy']!r} vs two-label {ce!r} (one label {hard!r})")
    assert st["nan"] == 0.0 and abs(st["cross_entropy"] - ce) <= 2e-2 * max(1.0, ce)
    assert abs(st["accuracy"] * B - mo.top1_count(z, y)) < 1e-3
    # eval stays hard-label
    _, _, plain = _net(dev, model, cin, _opt(False, eps))
    _load(plain, x, y)
    sa, sb = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    net.eval_batch(B, sa)
    plain.eval_batch(B, sb)
    torch.cuda.synchronize()
    assert torch.equal(sa[:3], sb[:3]) and torch.equal(net.logits, plain.logits)
    lso.check_ce(sa[0].item(), lso.ce_sum(net.logits[:B, :10], y, 0.0), "eval_batch")


def test_lenet5_with_dropout_smoothing_and_mix(dev, K):
    """dropout 0.2 + label_smoothing 0.1 + mix through the fused head's MIX + DROP instantiation: the
    gradients against torch_ref given the host-reference multipliers and the two-label loss."""
    from distributed_tensorflow_ibm_mnist_amd.ops import dropout as D
    pdrop, eps, t = 0.2, 0.1, 7
    spec, init, net = _net(dev, "lenet5", 1, _opt(True, eps, dropout=pdrop, dropout_seed=mo.SEED))
    x, y = lsg._batch(dev, 1)
    y2, lam = _second(dev, y, 60)
    _load(net, x, y, y2, lam)
    net.fp.step.fill_(t)
    lsg._grad_step(net, B)
    mult = {n: torch.from_numpy(D.multiplier(mo.SEED, t, i, B, spec.layers[i].dout, pdrop)).to(dev)
            for n, i in D.dropout_layers(spec).items()}
    p = {k: v.to(dev).to(torch.bfloat16).float().requires_grad_(True) for k, v in init.items()}
    p16 = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    lg, _ = torch_ref.forward(spec, p, x.float(), dropout=mult)
    torch_ref.two_label_cross_entropy(lg, y, y2, lam, eps).mean().backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        l16, _ = torch_ref.forward(spec, p16, x.float(), dropout=mult)
    torch_ref.two_label_cross_entropy(l16.float(), y, y2, lam, eps).mean().backward()
    assert rel_err(net.logits[:, :10], lg) < 3e-2
    for name in init:
        e, floor = rel_err(net.fp.grad_view(name), p[name].grad), rel_err(p16[name].grad, p[name].grad)
        print(f"{name}: rel err {e:.3e} (bf16 floor {floor:.3e})")
        assert e < max(3e-2, 3.0 * floor), f"{name}: rel err {e:.3e} (bf16 floor {floor:.3e})"
    ce = mo.ce_sum(net.logits[:B, :10], y, y2, lam, eps) / B
    st = net.read_stats()
    assert st["nan"] == 0.0 and abs(st["cross_entropy"] - ce) <= 2e-2 * max(1.0, ce)


# ------------------------------------------------------------------ 6. the loader
N_DS = 192


def _dataset(dev, C=1):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceDataset
    rng = np.random.default_rng(9 + C)
    return DeviceDataset(torch.from_numpy(rng.integers(0, 256, (N_DS, 784 * C), dtype=np.uint8)),
                         torch.arange(N_DS) % 10, dev, channels=C)


def _loader(ds, dev, Bl, C, mix, **kw):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceLoader
    extra = {}
    if mix is not None:
        extra = dict(mix=mix, out_labels2=torch.full((Bl,), -55, dtype=torch.int32, device=dev),
                     out_lam=torch.full((Bl,), -3.0, device=dev))
    return DeviceLoader(ds, torch.full((Bl, 28, 28, C), SENT, dtype=torch.bfloat16, device=dev),
                        torch.full((Bl,), -77, dtype=torch.int32, device=dev), **extra, **kw)


def _check_loader_batch(mixed, plain, cfg, pos0, nb, E32, what):
    x = plain.out_images[:nb].float().cpu().numpy().reshape(nb, 784, -1)
    y = plain.out_labels[:nb].cpu().numpy()
    img = mixed.out_images.reshape(mixed.B, 784, -1)
    kind, wlam, box = mo.batch_draws(cfg.mixup_alpha, cfg.cutmix_alpha, cfg.prob, cfg.seed, pos0, nb)
    got_lam = mixed.out_lam[:nb].cpu().numpy()
    assert np.array_equal(got_lam.view(np.uint32), wlam.view(np.uint32)), what
    ref, l2, _ = mo.mixed(x, y, kind, got_lam, box)
    assert np.array_equal(mixed.out_labels2[:nb].cpu().numpy(), l2) and np.array_equal(mixed.out_labels[:nb].cpu().numpy(), y)
    got = img[:nb].double().cpu().numpy()
    exact = kind != mo.MIXUP
    assert np.array_equal(got[exact], ref[exact]), what
    assert np.all(np.abs(got[~exact] - ref[~exact]) <= mo.image_bound(ref[~exact], E32)), what
    assert (kind == mo.MIXUP).any() and (kind == mo.CUTMIX).any()


@pytest.mark.parametrize("C,shift", [(1, 0), (3, 0), (1, 2)])
def test_loader_mixes_the_gathered_or_augmented_batch(dev, K, E32, C, shift):
    from distributed_tensorflow_ibm_mnist_amd.data.augment import AugmentConfig
    ds = _dataset(dev, C)
    cfg = M.MixConfig(0.4, 1.0, 0.9, 21)
    aug = AugmentConfig(shift=shift, seed=8) if shift else None
    run, plain = _loader(ds, dev, 64, C, cfg, seed=4, augment=aug), _loader(ds, dev, 64, C, None, seed=4, augment=aug)
    assert run.lookahead_job() is None
    kept = []
    for k in range(3):
        assert run.next() == 64 and plain.next() == 64
        torch.cuda.synchronize()
        _check_loader_batch(run, plain, cfg, 64 * k, 64, E32, f"C={C} shift={shift} step {k}")
        kept.append([t.clone() for t in (run.out_images, run.out_labels, run.out_labels2, run.out_lam)])
    other = _loader(ds, dev, 64, C, cfg, seed=4, augment=aug)
    other.seek(2)
    other.next()
    for a, b in zip(kept[2], (other.out_images, other.out_labels, other.out_labels2, other.out_lam)):
        assert torch.equal(a, b)
    # a partial batch flips itself; the rows past it keep what they held
    run.out_lam.fill_(-3.0)
    for ld in (run, plain):
        ld.out_images.fill_(SENT)
        ld.seek(5)
        assert ld.next(33) == 33
    torch.cuda.synchronize()
    _check_loader_batch(run, plain, cfg, 64 * 5, 33, E32, "partial batch")
    assert bool((run.out_images[33:] == SENT).all()) and bool((run.out_lam[33:] == -3.0).all())
    with pytest.raises(ValueError, match="idx_out"):
        _loader(ds, dev, 64, C, cfg, idx_out=torch.zeros(64, dtype=torch.int64, device=dev))


# ------------------------------------------------------------------ 7. graph replay
def _replica(dev, model, C, mix, graph, mode="prep", lines=None):
    from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica
    spec = get_model(model, C)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.integers(0, 256, (N_DS, 784 * C), dtype=np.uint8))
    y = torch.arange(N_DS) % 10
    opt = OptConfig(lr0=0.01, decay_steps=0, use_momentum=True, momentum=0.9, ema_max=0.9999, label_smoothing=0.1,
                    mix=mix is not None and mix.enabled)
    return Replica(spec, "hip", 64, dev, torch_ref.init_params(spec, seed=0), opt, x, y, C, x[:100], y[:100], seed=5,
                   use_graph=graph, fused_input=mode, mix=mix, log=(lines.append if lines is not None else print))


@pytest.mark.parametrize("model,C", [("lenet5", 1), ("reference_cnn", 3)])
def test_graph_replay_is_bitwise_the_eager_run(dev, K, model, C):
    """Three steps with the loader feeding each: one eager warm-up plus two replays against three eager
    steps.  The mix launch is the loader's, outside the captured step; the heads read fixed buffers."""
    cfg = M.MixConfig(0.4, 1.0, 1.0, 21)
    lines = []
    eager, graph = _replica(dev, model, C, cfg, False), _replica(dev, model, C, cfg, True, mode="bf16", lines=lines)
    assert any("prep" in ln for ln in lines) and graph.net.idx_buf is None
    for _ in range(3):
        eager.step()
        graph.step()
    torch.cuda.synchronize()
    assert graph._graph is not None and eager._graph is None
    for name in ("x0", "labels", "labels2", "mix_lam", "stats"):
        assert torch.equal(getattr(eager.net, name), getattr(graph.net, name)), name
    assert torch.equal(eager.net.fp.params, graph.net.fp.params) and torch.equal(eager.net.fp.mom, graph.net.fp.mom)
    assert int(graph.net.fp.step.item()) == 3 and graph.net.read_stats()["nan"] == 0.0
    assert np.array_equal(graph.net.mix_lam.cpu().numpy(), mo.batch_draws(0.4, 1.0, 1.0, 21, 128, 64)[1])
    # Replica.evaluate is unmixed and hard-label: the labels2 / mix_lam buffers are left alone by it
    lam = graph.net.mix_lam.clone()
    assert graph.evaluate() == eager.evaluate() and torch.equal(lam, graph.net.mix_lam)


def test_fp32_executor_refuses_mixing(dev, K):
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor_f32 import HipNetF32
    spec = get_model("lenet5", 1)
    with pytest.raises(ValueError, match="mixup_alpha"):
        HipNetF32(spec, 32, dev, torch_ref.init_params(spec, seed=0), OptConfig(mix=True))
