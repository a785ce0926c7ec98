"""Knowledge distillation on the device: the distilled (DISTILL) form of the five softmax cross-entropy
kernels -- softmax_ce_rows_k, softmax_ce_k, softmax_ce_f32_k, ce_tail_k, mlp_head_k -- against the float64
oracle written from the definition (tests/distill_oracle.py), their bindings, the executors, the frozen
teacher and the command line (graph replay: tests/test_teacher_replay_gpu.py).

Tolerances are the project's: the loss sum ``ce_tol`` applied to the magnitudes that are summed
(distill_oracle.loss_tol), the bf16 dlogits 2**-8 max|g|, the fp32 dlogits 1e-5 max|g| + 1e-6, dbias
1e-2 max_c sum|g| + 1e-6, dx 2**-7, the head's chain 2e-2 (tests/test_mix_gpu.py).

The NaN-flag tests write NaN / inf *values* and read a flag; nothing here provokes a fault.
"""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
from distributed_tensorflow_ibm_mnist_amd.runtime.executor_f32 import HipNetF32
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _by_path(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


do = _by_path("distill_oracle")
lsg = _by_path("test_label_smoothing_gpu")      # its input builders: _logits, _tail_inputs, _head_inputs, _tr
lso = lsg.lso

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SENT, EXTRA = lsg.SENT, lsg.EXTRA
rel_err, _work, _finalize = lsg.rel_err, lsg._work, lsg._finalize
NBS = [1, 77, 300]
AT = [(1.0, 1.0), (0.5, 2.0), (0.25, 8.0), (0.5, 0.5)]
AT_IDS = [f"a{a}-T{t}" for a, t in AT]
# (kind, the student's row stride, statistics path, the teacher's row stride)
CE_KERNELS = [("bf16", 16, "ticket", 10), ("bf16", 16, "defer", 16), ("bf16", 16, "atomic", 10), ("bf16", 32, "ticket", 16),
              ("bf16", 32, "defer", 10), ("bf16", 24, "atomic", 16), ("f32", 10, "ticket", 16), ("f32", 10, "atomic", 10)]
CE_IDS = [f"{k}-ld{l}-{m}-ldt{t}" for k, l, m, t in CE_KERNELS]
HEAD_MODES = [("ticket", 10), ("defer", 16)]
HEAD_IDS = [f"{m}-ldt{t}" for m, t in HEAD_MODES]


def _teacher(dev, n, ldt, seed, nb=None, scale=5.0, poison=True):
    """Teacher logits [n, ldt]: ordinary values in the 10 real columns of the rows < nb; with ``poison``
    NaN everywhere else (the padded columns and the rows >= nb are never to be read), else zeros there.
    The scale is the one tests/test_distill_cpu.py checks with the oracle alone: at 5 the bounds tell a
    wrong temperature and the hard-label loss apart with room to spare."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.full((n, ldt), NAN if poison else 0.0)
    rows = n if nb is None else nb
    t[:rows, :10] = torch.randn(rows, 10, generator=g) * scale
    return t.to(dev)


def _tkw(t, ldt, a, T):
    return {} if t is None else dict(teacher_logits=t, teacher_ld=ldt, distill_alpha=a, distill_temperature=T)


# ------------------------------------------------------------------ launches over sentinel-filled outputs
_LAST = {}      # the outputs and statistics of the latest launch, kept for a launch that raises


def _fresh(**kw):
    _LAST.clear()
    _LAST.update(kw)


def _run_ce(K, dev, kind, lg, ld, y, nb, mode, scale, grads=True, **kw):
    stats = torch.zeros(8, device=dev)
    work = _work(dev) if mode in ("ticket", "defer") else None
    n = lg.shape[0]
    o = {}
    if kind == "f32":
        o["dl"] = torch.full((n, ld), SENT, device=dev) if grads else None
        _fresh(stats=stats, outs=[o["dl"]], fills=[])
        K.f32_softmax_ce(lg, ld, y, nb, 10, scale, o["dl"], ld, stats, None, work, **kw)
    else:
        o["dl"] = torch.full((n, ld), SENT, dtype=torch.bfloat16, device=dev) if grads else None
        nblk = K.softmax_ce_dbias_blocks(nb, ld)
        db = torch.full((nblk * ld,), 9.0, device=dev) if (grads and nblk > 0) else None
        _fresh(stats=stats, outs=[o["dl"]], fills=[db])
        ndef = K.softmax_ce(lg, ld, y, nb, 10, scale, o["dl"], ld, stats, None, work, defer_stats=mode == "defer",
                            dbias=db, **kw)
        if mode == "defer":
            assert ndef > 0 and stats[:3].tolist() == [0.0, 0.0, 0.0]
            _finalize(K, dev, stats, work, ndef)
        if db is not None:
            o["dbias_blocks"], o["dbias"] = db, db.view(nblk, ld).sum(0)
    torch.cuda.synchronize()
    st = stats.tolist()
    if mode == "defer":
        st[0], st[1] = st[4], st[5]
    o["logits"] = lg
    return st, o


def _run_tail(K, dev, inp, nb, mode, **kw):
    x, w, wt, b, y = inp
    n = x.shape[0]
    o = {"logits": torch.full((n, 16), SENT, device=dev), "dl": torch.full((n, 16), SENT, dtype=torch.bfloat16, device=dev),
         "dx": torch.full((n, 192), SENT, dtype=torch.bfloat16, device=dev)}
    stats, work = torch.zeros(8, device=dev), _work(dev)
    nblk = K.ce_tail_blocks(nb)
    dbias = torch.full((nblk * 16,), 9.0, device=dev)
    _fresh(stats=stats, outs=list(o.values()), fills=[dbias])
    K.ce_tail(x, wt, b, 10, y, nb, 1.0 / nb, o["logits"], dl=o["dl"], dx=o["dx"], stats=stats, work=work,
              defer_stats=mode == "defer", dbias=dbias, **kw)
    if mode == "defer":
        assert stats[:3].tolist() == [0.0, 0.0, 0.0]
        _finalize(K, dev, stats, work, nblk)
    torch.cuda.synchronize()
    st = stats.tolist()
    if mode == "defer":
        st[0], st[1] = st[4], st[5]
    o["dbias_blocks"], o["dbias"] = dbias, dbias.view(nblk, 16).sum(0)
    return st, o


def _run_head(K, dev, p, nb, mode, **kw):
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
    _fresh(stats=stats, outs=list(o.values()), fills=[dbias])
    K.mlp_head(p["x"], tr(p["w3"], 128, 416), p["b3"], 120, tr(p["w4"], 96, 128), p["b4"], 84,
               tr(p["w5"], 16, 96), p["b5"], 10, p["y"], nb, 1.0 / nb, o["h3"], o["h4"], o["logits"],
               dl=o["dl"], dh4=o["dh4"], dh3=o["dh3"], dx=o["dx"], stats=stats, work=work,
               defer_stats=mode == "defer", dbias=dbias, **kw)
    if mode == "defer":
        assert stats[:3].tolist() == [0.0, 0.0, 0.0]
        _finalize(K, dev, stats, work, nblk)
    torch.cuda.synchronize()
    st = stats.tolist()
    if mode == "defer":
        st[0], st[1] = st[4], st[5]
    o["dbias_blocks"], o["dbias"] = dbias, dbias.view(nblk, 16).sum(0)
    return st, o


def _np(t):
    return t.detach().double().cpu().numpy()


def _check(what, st, o, z, t, y, a, T, scale, nb, f32=False):
    """The loss sum, the count, the flag, dl, dbias and the padded columns of one distilled launch against
    the oracle on the kernel's own logits z; then that the bounds tell a wrong temperature and the plain
    hard-label loss from the right one."""
    z, t, y = _np(z), _np(t), y.cpu().numpy()
    ref = do.distill(z, t, y, a, T, scale)
    tol = do.loss_tol(ref)
    share = abs(st[0] - ref.loss) / tol
    print(f"{what}: loss {st[0]!r} vs float64 {ref.loss!r}: {100 * share:.2f} % of tol {tol:.3e} "
          f"(hard {ref.hard:.4g}, CEs {ref.ces:.4g}, H(q) {ref.hq:.4g})")
    assert st[2] == 0.0, f"{what}: flag"
    assert share <= 1.0, f"{what}: loss {st[0]!r} vs {ref.loss!r}, {share:.3f} of the bound"
    assert round(st[1]) == ref.correct and abs(st[1] - ref.correct) < 1e-3, f"{what}: count"
    dl = _np(o["dl"])
    g = ref.dl
    gmax = np.abs(g).max()
    bound = 1e-5 * gmax + 1e-6 if f32 else 2.0 ** -8 * gmax
    err = np.abs(dl[:nb, :10] - g).max()
    print(f"{what}: dl err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: dl err {err:.3e} > {bound:.3e}"
    assert not dl[:nb, 10:].any(), f"{what}: padded columns reached dl"
    assert bool((o["dl"][nb:] == SENT).all()), f"{what}: dl rows >= nb were written"
    if o.get("dbias") is not None:
        lso.check_dbias(o["dbias"][:10], g, what)
        assert not o["dbias"][10:].any()
    if nb > 1:      # the bounds discriminate
        others = [("hard labels", do.distill(z, t, y, 0.0, 1.0, scale))]
        if T != 1.0:
            others.append(("T = 1", do.distill(z, t, y, a, 1.0, scale)))
        for name, w in others:
            assert abs(w.loss - ref.loss) > 10 * tol, f"{what}: the loss bound does not tell {name} apart"
            assert np.abs(w.dl - g).max() > 10 * bound, f"{what}: the dl bound does not tell {name} apart"
    return share


# ------------------------------------------------------------------ 1 - 3. the five kernels against the oracle
@pytest.mark.parametrize("a,T", AT, ids=AT_IDS)
@pytest.mark.parametrize("kind,ld,mode,ldt", CE_KERNELS, ids=CE_IDS)
@pytest.mark.parametrize("nb", NBS)
def test_softmax_ce_distilled(dev, K, nb, kind, ld, mode, ldt, a, T):
    lg, y = lsg._logits(dev, nb, ld, 4000 + nb)
    t = _teacher(dev, nb + EXTRA, ldt, 17 + nb, nb)
    scale = 1.0 / nb
    st, o = _run_ce(K, dev, kind, lg, ld, y, nb, mode, scale, **_tkw(t, ldt, a, T))
    _check(f"{kind} ld={ld} {mode} nb={nb} a={a} T={T}", st, o, lg[:nb, :10], t[:nb, :10], y[:nb], a, T, scale, nb,
           f32=kind == "f32")


@pytest.mark.parametrize("a,T", AT, ids=AT_IDS)
@pytest.mark.parametrize("mode,ldt", HEAD_MODES, ids=HEAD_IDS)
@pytest.mark.parametrize("nb", NBS)
def test_ce_tail_distilled(dev, K, nb, mode, ldt, a, T):
    inp = lsg._tail_inputs(dev, nb)
    x, w, wt, b, y = inp
    t = _teacher(dev, nb + EXTRA, ldt, 23 + nb, nb)
    st, o = _run_tail(K, dev, inp, nb, mode, **_tkw(t, ldt, a, T))
    z = o["logits"][:nb, :10]
    ref = x[:nb].float() @ w.float() + b
    assert (z - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-5
    assert not o["logits"][:nb, 10:].any()
    _check(f"ce_tail {mode} nb={nb} a={a} T={T}", st, o, z, t[:nb, :10], y[:nb], a, T, 1.0 / nb, nb)
    gx = (o["dl"][:nb, :10].float() @ w.float().t()) * (x[:nb].float() > 0)
    assert (o["dx"][:nb].float() - gx).abs().max().item() <= 2 ** -7 * gx.abs().max().item()
    assert not o["dx"][:nb][x[:nb] == 0].any()
    for k in ("logits", "dl", "dx"):
        assert bool((o[k][nb:] == SENT).all()), f"ce_tail wrote {k} rows >= nb"


@pytest.mark.parametrize("a,T", AT, ids=AT_IDS)
@pytest.mark.parametrize("mode,ldt", HEAD_MODES, ids=HEAD_IDS)
@pytest.mark.parametrize("nb", [1, 33, 77])
def test_mlp_head_distilled(dev, K, nb, mode, ldt, a, T):
    p = lsg._head_inputs(dev, nb)
    t = _teacher(dev, nb + EXTRA, ldt, 29 + nb, nb)
    st, o = _run_head(K, dev, p, nb, mode, **_tkw(t, ldt, a, T))
    x = p["x"][:nb].float()
    w3, w4, w5 = p["w3"].float(), p["w4"].float(), p["w5"].float()
    h3 = torch.relu(x @ w3 + p["b3"]).to(torch.bfloat16)
    h4 = torch.relu(h3.float() @ w4 + p["b4"]).to(torch.bfloat16)
    ref = h4.float() @ w5 + p["b5"]
    assert rel_err(o["h3"][:nb], h3) < 1e-2 and rel_err(o["h4"][:nb, :84], h4) < 1e-2
    assert not o["h4"][:nb, 84:].any()
    z = o["logits"][:nb, :10]
    assert rel_err(z, ref) < 1e-2 and not o["logits"][:nb, 10:].any()
    _check(f"mlp_head {mode} nb={nb} a={a} T={T}", st, o, z, t[:nb, :10], p["y"][:nb], a, T, 1.0 / nb, nb)
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


# ------------------------------------------------------------------ 4. edge rows
def _runner(K, dev, kern, nb):
    """One of the five kernels as run(teacher, ldt, a, T, student=None) -> (stats, outputs); ``student``
    names what is done to the student's logits: None, or "inf" (an infinite logit in row nb - 1)."""
    kind = kern[0]
    if kind in ("bf16", "f32"):
        _, ld, mode = kern
        lg, y = lsg._logits(dev, nb, ld, 4100 + nb)

        def run(t, ldt, a, T, student=None, grads=True):
            l2 = lg
            if student == "inf":
                l2 = lg.clone()
                l2[nb - 1, 4] = INF
            return _run_ce(K, dev, kind, l2, ld, y, nb, mode, 1.0 / nb, grads=grads, **_tkw(t, ldt, a, T))
        return run, y
    if kind == "tail":
        inp = list(lsg._tail_inputs(dev, nb))

        def run(t, ldt, a, T, student=None, grads=True):
            i2 = list(inp)
            if student == "inf":     # class 4 of row nb - 1 overflows to +inf (tests/test_label_smoothing_gpu.py)
                wt = inp[2].clone()
                wt[:, 5] = 0.0
                wt[4, 5] = 1e20
                i2[0], i2[2] = lsg._overflow_column(inp[0], nb - 1, 5), wt
            return _run_tail(K, dev, i2, nb, kern[1], **_tkw(t, ldt, a, T))
        return run, inp[4]
    p = lsg._head_inputs(dev, nb)

    def run(t, ldt, a, T, student=None, grads=True):
        q = dict(p)
        if student == "inf":
            q.update({k: p[k].clone() for k in ("w3", "w4", "w5")})
            for w, r, c, v in ((q["w3"], 7, 11, 1e10), (q["w4"], 11, 13, 1e7), (q["w5"], 13, 4, 1e3)):
                w[r, :] = 0.0
                w[:, c] = 0.0
                w[r, c] = v
            q["x"] = lsg._overflow_column(p["x"], nb - 1, 7)
        return _run_head(K, dev, q, nb, kern[1], **_tkw(t, ldt, a, T))
    return run, p["y"]


EDGE_KERNELS = [("bf16", 16, "ticket"), ("bf16", 32, "defer"), ("bf16", 24, "atomic"), ("f32", 10, "ticket"),
                ("tail", "ticket"), ("tail", "defer"), ("head", "ticket"), ("head", "defer")]
EDGE_IDS = ["-".join(str(v) for v in k) for k in EDGE_KERNELS]


@pytest.mark.parametrize("kern", EDGE_KERNELS, ids=EDGE_IDS)
@pytest.mark.parametrize("nb", [1, 77])
def test_edge_rows(dev, K, kern, nb):
    run, y = _runner(K, dev, kern, nb)
    n, a, T = nb + EXTRA, 0.5, 2.0
    f32 = kern[0] == "f32"
    for ldt in (10, 16):
        # a teacher row equal to the student's: the soft part is 0, its gradient too
        st0, o0 = run(None, 0, 0.0, 1.0)
        z = o0["logits"][:nb, :10]
        t = torch.full((n, ldt), NAN, device=dev)
        t[:nb, :10] = z
        st, o = run(t, ldt, a, T)
        ref = do.distill(_np(z), _np(z), y[:nb].cpu().numpy(), a, T, 1.0 / nb)
        tol = do.loss_tol(ref)
        assert ref.soft == 0.0 and st[2] == 0.0
        assert abs(st[0] - ref.hard) <= tol, (st[0], ref.hard, tol)
        g = _np(o["dl"])[:nb, :10]
        assert np.abs(g - ref.dl).max() <= (1e-5 * np.abs(ref.dl).max() + 1e-6 if f32 else 2.0 ** -8 * np.abs(ref.dl).max())
        # one-hot teachers: +-80 at T = 0.5 underflows every other class of q to 0
        t = torch.full((n, ldt), NAN, device=dev)
        t[:nb, :10] = -80.0
        t[torch.arange(nb, device=dev), (torch.arange(nb, device=dev) * 3) % 10] = 80.0
        st, o = run(t, ldt, 0.5, 0.5)
        ref = do.distill(_np(z), _np(t[:nb, :10]), y[:nb].cpu().numpy(), 0.5, 0.5, 1.0 / nb)
        assert st[2] == 0.0 and np.isfinite(st[0]) and abs(st[0] - ref.loss) <= do.loss_tol(ref)
        assert bool(torch.isfinite(o["dl"][:nb].float()).all())
        # poison in the teacher rows >= nb and in its columns >= NC changes no output bit
        clean = _teacher(dev, n, ldt, 31, poison=False)
        dirty = clean.clone()
        dirty[nb:] = NAN
        dirty[:, 10:] = NAN
        (sa, oa), (sb, ob) = run(clean, ldt, a, T), run(dirty, ldt, a, T)
        assert sa == sb and sa[2] == 0.0
        for k in oa:
            if oa[k] is not None:
                assert torch.equal(oa[k], ob[k]), k
        # a NaN or a +inf in the teacher's row nb - 1 raises the flag, and so does an infinite student logit
        for v in (NAN, INF):
            bad = clean.clone()
            bad[nb - 1, 7] = v
            assert run(bad, ldt, a, T)[0][2] == 1.0, v
        assert run(clean, ldt, a, T, student="inf")[0][2] == 1.0
        assert run(clean, ldt, 1.0, T, student="inf")[0][2] == 1.0


# ------------------------------------------------------------------ 5. off is the plain launch
@pytest.mark.parametrize("kern", EDGE_KERNELS, ids=EDGE_IDS)
def test_off_is_the_plain_launch(dev, K, kern):
    nb = 77
    run, _ = _runner(K, dev, kern, nb)
    t = _teacher(dev, nb + EXTRA, 16, 5, nb)
    base = run(None, 0, 0.0, 1.0)
    assert base[0][2] == 0.0
    for other in (run(t, 16, 0.0, 2.0), _off_none(K, dev, kern, nb)):
        assert other[0] == base[0]
        for k, v in base[1].items():
            if v is not None:
                assert torch.equal(v, other[1][k]), k


def _off_none(K, dev, kern, nb):
    """The call with teacher_logits=None spelled out, the other keywords at values of their own."""
    kw = dict(teacher_logits=None, teacher_ld=0, distill_alpha=0.5, distill_temperature=2.0)
    if kern[0] in ("bf16", "f32"):
        lg, y = lsg._logits(dev, nb, kern[1], 4100 + nb)
        return _run_ce(K, dev, kern[0], lg, kern[1], y, nb, kern[2], 1.0 / nb, **kw)
    if kern[0] == "tail":
        return _run_tail(K, dev, lsg._tail_inputs(dev, nb), nb, kern[1], **kw)
    return _run_head(K, dev, lsg._head_inputs(dev, nb), nb, kern[1], **kw)


# ------------------------------------------------------------------ 6. the bindings validate
def test_bindings_validate(dev, K):
    nb = 8
    n = nb + EXTRA
    good = _teacher(dev, n, 16, 3, poison=False)
    bad_kw = [("float32", dict(teacher_logits=good.double())), ("device", dict(teacher_logits=good.cpu())),
              ("contiguous", dict(teacher_logits=good.t().contiguous().t())),
              ("teacher_ld", dict(teacher_ld=9)), ("elements", dict(teacher_logits=good[:nb - 1].contiguous())),
              ("distill_alpha", dict(distill_alpha=1.5)), ("distill_alpha", dict(distill_alpha=-0.1)),
              ("distill_alpha", dict(distill_alpha=NAN)), ("distill_temperature", dict(distill_temperature=0.0)),
              ("distill_temperature", dict(distill_temperature=INF)), ("distill_temperature", dict(distill_temperature=1e30)),
              ("label_smoothing", dict(label_smoothing=0.1))]
    base = dict(teacher_logits=good, teacher_ld=16, distill_alpha=0.5, distill_temperature=2.0)
    lg, y = lsg._logits(dev, nb, 16, 1)
    lam = torch.ones(n, device=dev)
    def ce(kind):
        def go(**kw):
            st, o = _run_ce(K, dev, kind, lg if kind == "bf16" else lg[:, :10].contiguous(), 16 if kind == "bf16" else 10,
                            y, nb, "ticket", 1.0, **kw)
            return st, o
        return go
    tail_in, head_in = lsg._tail_inputs(dev, nb), lsg._head_inputs(dev, nb)
    calls = [("softmax_ce", ce("bf16"), [("labels2", dict(labels2=y, lam=lam))]),
             ("f32_softmax_ce", ce("f32"), []),
             ("ce_tail", lambda **kw: _run_tail(K, dev, tail_in, nb, "ticket", **kw), [("labels2", dict(labels2=tail_in[4], lam=lam))]),
             ("mlp_head", lambda **kw: _run_head(K, dev, head_in, nb, "ticket", **kw),
              [("labels2", dict(labels2=head_in["y"], lam=lam)),
               ("dropout", dict(dropout=0.25, drop_step=torch.zeros(1, dtype=torch.int64, device=dev), drop_seed=1,
                                drop_layer3=2, drop_layer4=3))])]
    for name, go, extra in calls:
        go(**base)      # the good call launches
        for match, kw in bad_kw + extra:
            with pytest.raises(ValueError, match=match):
                go(**{**base, **kw})
            torch.cuda.synchronize()
            assert _LAST["outs"] and all(bool((v == SENT).all()) for v in _LAST["outs"]), f"{name} / {match}: an output was written"
            assert all(bool((v == 9.0).all()) for v in _LAST["fills"] if v is not None), f"{name} / {match}: dbias was written"
            assert _LAST["stats"].tolist() == [0.0] * 8, f"{name} / {match}: the statistics were written"
    # a teacher in an eval-form head
    st = torch.zeros(8, device=dev)
    logits = torch.full((n, 16), SENT, device=dev)
    x, w, wt, b, yt = tail_in
    with pytest.raises(ValueError, match="needs dl"):
        K.ce_tail(x, wt, b, 10, yt, nb, 1.0, logits, stats=st, work=_work(dev), **base)
    p = head_in
    h3, h4 = torch.zeros(n, 120, dtype=torch.bfloat16, device=dev), torch.zeros(n, 88, dtype=torch.bfloat16, device=dev)
    tr = lsg._tr
    with pytest.raises(ValueError, match="needs dl"):
        K.mlp_head(p["x"], tr(p["w3"], 128, 416), p["b3"], 120, tr(p["w4"], 96, 128), p["b4"], 84, tr(p["w5"], 16, 96),
                   p["b5"], 10, p["y"], nb, 1.0, h3, h4, logits, stats=st, work=_work(dev), **base)
    torch.cuda.synchronize()
    assert st.tolist() == [0.0] * 8 and bool((logits == SENT).all())


# ------------------------------------------------------------------ 7. the executors
from distributed_tensorflow_ibm_mnist_amd.runtime.teacher import Teacher      # noqa: E402

B = 64
# (student, precision, the student's head, the teacher: another registry model)
NETS = [("lenet5", "bf16", "mlp", "reference_cnn"), ("reference_cnn", "bf16", "tail", "lenet5"), ("mlp", "bf16", None, "lenet5"),
        ("lenet5", "fp32", None, "mlp")]
NET_IDS = [f"{m}-{p}" for m, p, _, _ in NETS]


def _opt(a, T, **kw):
    return OptConfig(lr0=0.05, decay_steps=0, use_momentum=False, ema_max=0.9999, distill_alpha=a, distill_temperature=T,
                     **kw)


def _student(dev, model, prec, opt, batch=B):
    spec = get_model(model, 1)
    init = torch_ref.init_params(spec, seed=1)
    net = (HipNetF32 if prec == "fp32" else HipNet)(spec, batch, dev, init, opt)
    return spec, init, net


def _teacher_for(net, model, prec, seed=3, scale=4.0):
    """A frozen teacher with random weights, its last layer scaled so that its targets are not flat."""
    tspec = get_model(model, 1)
    tinit = torch_ref.init_params(tspec, seed=seed)
    tinit["softmax_linear/weights"] = tinit["softmax_linear/weights"] * scale
    return tspec, tinit, Teacher(tspec, tinit, net, "hip", prec)


@pytest.mark.parametrize("model,prec,head,tmodel", NETS, ids=NET_IDS)
def test_executor_gradients_match_the_distillation_oracle(dev, K, model, prec, head, tmodel):
    """Teacher.forward; forward(defer_head=True); loss_and_grad(); backward() under OptConfig(distill_alpha=0.5,
    distill_temperature=2): every gradient against torch_ref with the distillation loss on the teacher's
    own logits, under the rule of test_executor_gradients_match_the_two_label_oracle, max(3e-2, 3 x the
    bf16-autocast floor); the cross_entropy statistic within 2e-2 max(1, ce) of the float64 mean on the
    kernel's own logits; eval_batch afterwards bitwise that of a net built without distillation."""
    a, T = 0.5, 2.0
    spec, init, net = _student(dev, model, prec, _opt(a, T))
    if prec == "bf16":
        assert net.head_kind == head
    with pytest.raises(RuntimeError, match="teacher_logits"):      # on without a teacher is an error
        lsg._grad_step(net, B, backward=False)
    net._head_pending = None
    tspec, tinit, teacher = _teacher_for(net, tmodel, prec)
    assert teacher.net.x0 is net.x0 and net.teacher_logits is teacher.logits
    x, y = lsg._batch(dev, 1, B)
    lsg._load(net, x, y)
    teacher.forward(B)
    lsg._grad_step(net, B)
    t = teacher.logits[:B, :10].clone()
    rnd = (lambda v: v.to(torch.bfloat16).float()) if prec == "bf16" else (lambda v: v.float())
    p = {k: rnd(v.to(dev)).requires_grad_(True) for k, v in init.items()}
    p16 = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    lg, _ = torch_ref.forward(spec, p, x.float())
    torch_ref.losses(spec, p, lg, y, teacher_logits=t, distill_alpha=a, distill_temperature=T)["cross_entropy"].backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        l16, _ = torch_ref.forward(spec, p16, x.float())
    torch_ref.distillation_loss(l16.float(), y, t, a, T).mean().backward()
    assert rel_err(net.logits[:, :10], lg) < 3e-2
    for name in init:
        e = rel_err(net.fp.grad_view(name), p[name].grad)
        floor = rel_err(p16[name].grad, p[name].grad)
        print(f"{model}-{prec} {name}: rel err {e:.3e} (bf16 floor {floor:.3e})")
        assert e < max(3e-2, 3.0 * floor), f"{name}: rel err {e:.3e} (bf16 floor {floor:.3e})"
    st = net.read_stats()
    z = net.logits[:B, :10]
    ref = do.distill(_np(z), _np(t), y.cpu().numpy(), a, T)
    ce, hard = ref.loss / B, do.distill(_np(z), _np(t), y.cpu().numpy(), 0.0, 1.0).loss / B
    print(f"cross_entropy {st['cross_entropy']!r} vs distilled {ce!r} (hard labels {hard!r})")
    assert st["nan"] == 0.0 and abs(st["cross_entropy"] - ce) <= 2e-2 * max(1.0, ce)
    assert abs(hard - ce) > 4e-2 * max(1.0, ce), "the two losses must differ for this test to mean anything"
    assert abs(st["accuracy"] * B - ref.correct) < 1e-3
    # eval stays the plain cross-entropy
    _, _, plain = _student(dev, model, prec, _opt(0.0, 2.0))
    lsg._load(plain, x, y)
    sa, sb = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    net.eval_batch(B, sa)
    plain.eval_batch(B, sb)
    torch.cuda.synchronize()
    assert torch.equal(sa[:3], sb[:3]) and torch.equal(net.logits, plain.logits)
    lso.check_ce(sa[0].item(), lso.ce_sum(net.logits[:B, :10], y, 0.0), "eval_batch")


# ------------------------------------------------------------------ 8. the teacher
@pytest.mark.parametrize("model,prec", [("reference_cnn", "bf16"), ("lenet5", "bf16"), ("lenet5", "fp32")])
def test_teacher_forward_is_the_eval_forward_and_it_stays_frozen(dev, K, model, prec):
    from distributed_tensorflow_ibm_mnist_amd.obs.eval_metrics import EvalAccumulator
    spec, init, net = _student(dev, "mlp", prec, OptConfig(lr0=0.05, use_momentum=True, momentum=0.9, distill_alpha=0.5))
    tspec, tinit, teacher = _teacher_for(net, model, prec)
    alone = (HipNetF32 if prec == "fp32" else HipNet)(tspec, B, dev, tinit, OptConfig())
    x, y = lsg._batch(dev, 1, B)
    lsg._load(net, x, y)
    lsg._load(alone, x, y)
    for nb in (B, 33):
        teacher.logits.fill_(SENT)
        teacher.forward(nb)
        # eval_batch's stored logits: with an accumulator its head runs layer by layer and stores them
        alone.eval_batch(nb, torch.zeros(8, device=dev), metrics=EvalAccumulator(dev, 10))
        torch.cuda.synchronize()
        assert torch.equal(teacher.logits[:nb], alone.logits[:nb])
        assert bool((teacher.logits[nb:] == SENT).all())
    before = [t.clone() for t in (teacher.net.fp.params, teacher.net.fp.step)]
    bf = None if prec == "fp32" else teacher.net.fp.bf16.clone()
    for k in range(5):
        xk, yk = lsg._batch(dev, 1, B, seed=60 + k)
        lsg._load(net, xk, yk)
        teacher.forward(B)
        net.train_step()
    torch.cuda.synchronize()
    assert int(net.fp.step.item()) == 5 and net.read_stats()["nan"] == 0.0
    assert torch.equal(before[0], teacher.net.fp.params) and torch.equal(before[1], teacher.net.fp.step)
    assert bf is None or torch.equal(bf, teacher.net.fp.bf16)
    other = get_model("lenet5", 3)
    with pytest.raises(ValueError, match="lenet5.*mlp"):
        Teacher(other, torch_ref.init_params(other, seed=0), net, "hip", prec)
    with pytest.raises(ValueError, match="x0"):
        HipNet(spec, B, dev, init, OptConfig(), x0=torch.zeros(B, 28, 28, 1, device=dev))


# 9. graph replay: tests/test_teacher_replay_gpu.py (a file of its own, collected after every other GPU file: each
# captured step takes one more stream out of the process's stream pool, and which hardware queue a later
# test's side stream lands on follows from how many were taken before it)


# ------------------------------------------------------------------ 10. the command line
def _main(args, timeout=170):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout, env=dict(os.environ, PYTHONUNBUFFERED="1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout + r.stderr


def test_cli_distills_from_a_checkpoint(tmp_path, dev):
    td, sd = str(tmp_path / "teacher"), str(tmp_path / "student")
    common = ["--in_channels=1", "--batch_size=64", "--test_interval=1000", "--log_step_count_steps=0",
              "--save_summaries_steps=1", "--train_data=synthetic://2000", "--test_data=synthetic://256?seed=1",
              "--eval_examples=128"]
    _main(["--model=reference_cnn", "--max_steps=6", f"--train_dir={td}"] + common)
    out = _main(["--model=lenet5", "--max_steps=8", f"--train_dir={sd}", f"--distill_from={td}",
                 "--distill_model=reference_cnn", "--augment_shift=2"] + common)
    assert "distillation teacher reference_cnn: test accuracy" in out, out[-3000:]
    from distributed_tensorflow_ibm_mnist_amd.ckpt.saver import Saver
    t = Saver.restore(os.path.join(sd, "model.ckpt-8"))
    assert int(t["global_step"]) == 8
    student = {f"{L.name}/{k}" for L in get_model("lenet5", 1).weights() for k in ("weights", "biases")}
    assert student <= set(t)
    assert not [k for k in t if k.startswith(("local3/", "local4/"))], sorted(t)      # no teacher variable
    from distributed_tensorflow_ibm_mnist_amd.obs.events import find_event_files, read_events
    ce = {}
    for f in find_event_files(sd):
        for ev in read_events(f):
            if "cross_entropy" in ev["values"]:
                ce[ev["step"]] = ev["values"]["cross_entropy"]
    assert len(ce) >= 8 and all(np.isfinite(v) for v in ce.values()), ce
    # a teacher that does not fit is refused before training starts
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--model=lenet5", "--max_steps=2",
                        f"--train_dir={tmp_path / 'bad'}", f"--distill_from={td}"] + common, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "distill_model" in (r.stdout + r.stderr)
