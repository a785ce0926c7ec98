"""What the training loop observes -- the cross-entropy sum, the top-1 count, the NaN flag, the
eval pass and ``probs()`` -- against a float64 oracle (tests/stats_oracle.py), on the kernels that
run by default: the fused LeNet-5 head (mlp_head_k), the reference CNN's tail (ce_tail_k), the
layered softmax_ce_rows_k / softmax_ce_k and the fp32 plan's softmax_ce_f32_k.

  A  partial batches (nb < B) over stale B-row buffers: rows >= nb are neither read nor written
  B  an eval pass between training steps does not perturb training (eager and hipGraph replay)
  C  the NaN flag on the ticket path, the deferred-partial path and through whole steps
  D  softmax stability at extreme logits
  E  the tie rule: logit[label] >= max counts (tf.nn.in_top_k, mnist_input.py:237-243)

These tests write NaN / inf *values* and read a flag; nothing here provokes a fault.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
from distributed_tensorflow_ibm_mnist_amd.runtime.executor_f32 import HipNetF32
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("stats_oracle", os.path.join(ROOT, "tests", "stats_oracle.py"))
so = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(so)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
B = 96
# (model, input channels, precision): HipNet's fused mlp_head_k, ce_tail_k (1 and 3 channels) and
# layered softmax_ce_rows_k heads, and HipNetF32's f32_softmax_ce
NETS = [("lenet5", 1, "bf16"), ("reference_cnn", 1, "bf16"), ("reference_cnn", 3, "bf16"), ("mlp", 1, "bf16"),
        ("reference_cnn", 1, "fp32")]
HEAD = {("lenet5", "bf16"): "mlp", ("reference_cnn", "bf16"): "tail", ("mlp", "bf16"): None,
        ("reference_cnn", "fp32"): None}
NET_IDS = [f"{m}{c}-{p}" for m, c, p in NETS]
# (nb, grid cap): one row, under one 8-image tile, just past a 32-row wave tile, one short of
# full; and nb = 33 with every persistent kernel capped to 2 blocks (several tiles per block)
PARTIAL = [(1, 0), (7, 0), (33, 0), (B - 1, 0), (33, 2)]
SENT = -776.0           # exact in fp32 and bf16


def rel_err(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _opt():
    return OptConfig(lr0=0.05, decay_steps=0, use_momentum=False, ema_max=0.9999)


def _build(dev, model, cin, prec, batch=B, seed=1, opt=None):
    spec = get_model(model, cin)
    init = torch_ref.init_params(spec, seed=seed)
    cls = HipNetF32 if prec == "fp32" else HipNet
    net = cls(spec, batch, dev, init, opt or _opt())
    if prec == "bf16":
        assert net.head_kind == HEAD[(model, prec)], (model, net.head_kind)
    return spec, init, net


_DATA = {}


def _data(dev, model, cin, prec):
    """Fixed inputs, labels and the fp32 oracle's logits for all B rows of one net, computed once
    (rows are independent, so rows [:nb] are the oracle of any partial batch)."""
    key = (model, cin, prec)
    if key not in _DATA:
        g = torch.Generator(device="cpu").manual_seed(11 + cin)
        x = (torch.rand(B, 28, 28, cin, generator=g) - 0.5).to(torch.bfloat16).to(dev)
        y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32).to(dev)
        xbig = ((torch.rand(B, 28, 28, cin, generator=g) - 0.5) * 16).to(torch.bfloat16).to(dev)
        ybig = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32).to(dev)
        spec = get_model(model, cin)
        init = torch_ref.init_params(spec, seed=1)
        # the bf16 plan computes on bf16-rounded weights (tests/test_executor_gpu._check_step)
        p = {k: (v.to(dev).to(torch.bfloat16).float() if prec == "bf16" else v.to(dev).float())
             for k, v in init.items()}
        with torch.no_grad():
            ref, _ = torch_ref.forward(spec, p, x.float())
        _DATA[key] = (x, y, xbig, ybig, ref.detach().clone())
    return _DATA[key]


def _load(net, x, y, nb, tail=0.0):
    """x0[:nb], labels[:nb] = the batch; rows >= nb: ``tail`` pixels and valid labels."""
    net.x0.fill_(tail)
    net.x0[:nb].copy_(x[:nb])
    net.labels.copy_((torch.arange(net.B, device=net.labels.device) % 10).to(torch.int32))
    net.labels[:nb].copy_(y[:nb])


# ------------------------------------------------------------------ A. partial batches
@pytest.mark.parametrize("nb,cap", PARTIAL, ids=[f"nb{n}-cap{c}" for n, c in PARTIAL])
@pytest.mark.parametrize("model,cin,prec", NETS, ids=NET_IDS)
def test_partial_batch_ignores_stale_rows(dev, K, grid_cap, model, cin, prec, nb, cap):
    """A1 + A2.  eval_batch(nb) over buffers whose rows >= nb hold a full training step's stale
    activations, gradients and logits, NaN pixels and sentinels gives bitwise the logits[:nb] and
    st[:3] of the same eval over zeroed rows (identical launches, so bitwise is the derived
    bound); st[2] stays 0; rows >= nb of the logits and of every layer's output keep their
    sentinel, through eval_batch and through probs(nb)."""
    grid_cap(cap)
    x, y, xbig, ybig, _ = _data(dev, model, cin, prec)
    _, _, net = _build(dev, model, cin, prec)
    _load(net, x, y, nb)
    st1 = torch.zeros(8, device=dev)
    net.eval_batch(nb, st1)
    torch.cuda.synchronize()
    lg1 = net.logits[:nb].clone()
    assert lg1.abs().max() > 0
    # one full training step on other, large data: every buffer now holds B stale rows
    params, bf = net.fp.params.clone(), net.fp.bf16.clone()
    net.x0.copy_(xbig)
    net.labels.copy_(ybig)
    net.train_step()
    net.fp.params.copy_(params)
    net.fp.bf16.copy_(bf)
    _load(net, x, y, nb, tail=NAN)
    net.logits[nb:].fill_(SENT)
    for lay in net.layers:
        lay.out[nb:].fill_(SENT)
    st2 = torch.zeros(8, device=dev)
    net.eval_batch(nb, st2)
    torch.cuda.synchronize()
    assert torch.equal(net.logits[:nb], lg1), "logits[:nb] depend on rows >= nb"
    assert torch.equal(st2[:3], st1[:3]), (st1.tolist(), st2.tolist())
    assert st2[2].item() == 0.0
    assert bool((net.logits[nb:] == SENT).all()), "eval_batch wrote logits rows >= nb"
    for lay in net.layers:
        assert bool((lay.out[nb:] == SENT).all()), f"eval_batch wrote {lay.name} rows >= nb"
    pr = net.probs(nb)
    torch.cuda.synchronize()
    assert tuple(pr.shape) == (nb, 10)
    assert bool((net.logits[nb:] == SENT).all()), "probs wrote logits rows >= nb"
    for lay in net.layers:
        assert bool((lay.out[nb:] == SENT).all()), f"probs wrote {lay.name} rows >= nb"


@pytest.mark.parametrize("nb,cap", PARTIAL, ids=[f"nb{n}-cap{c}" for n, c in PARTIAL])
@pytest.mark.parametrize("model,cin,prec", NETS, ids=NET_IDS)
def test_partial_batch_stats_match_float64(dev, K, grid_cap, model, cin, prec, nb, cap):
    """A3.  From the kernel's own fp32 logits[:nb]: the top-1 count exactly (a comparison of the
    same numbers, tie rule included), the loss sum to the fast-intrinsic bound, probs(nb) to
    1e-5; and the logits themselves against the fp32 oracle's rows."""
    grid_cap(cap)
    x, y, _, _, ref = _data(dev, model, cin, prec)
    _, _, net = _build(dev, model, cin, prec)
    _load(net, x, y, nb)
    st = torch.zeros(8, device=dev)
    net.eval_batch(nb, st)
    torch.cuda.synchronize()
    lg = net.logits[:nb, :10].clone()
    got = st.tolist()
    ce, cnt = so.ce_sum(lg, y[:nb]), so.top1_count(lg, y[:nb])
    print(f"{model}{cin}-{prec} nb={nb}: loss {got[0]!r} vs {ce!r}, correct {got[1]} vs {cnt}, "
          f"logits rel err {rel_err(lg, ref[:nb]):.3e}")
    assert got[1] == cnt
    so.check_ce(got[0], ce, "eval_batch")
    assert got[2] == 0.0
    assert rel_err(lg, ref[:nb]) < 3e-2
    pr = net.probs(nb)
    torch.cuda.synchronize()
    so.check_probs(pr, net.logits[:nb, :10], "probs")


def _eval_pass(net, eds, st, collect=None):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import eval_batches
    n = 0
    for nb in eval_batches(eds, net.x0, net.labels):
        net.eval_batch(nb, st)
        if collect is not None:
            torch.cuda.synchronize()
            collect.append((net.logits[:nb, :10].clone(), net.labels[:nb].clone()))
        n += nb
    return n


def _datasets(dev, cin, n_train=0):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceDataset
    from distributed_tensorflow_ibm_mnist_amd.data.synthetic import make_synthetic
    ei, el = make_synthetic(100, seed=5, device=dev, channels=cin)
    eds = DeviceDataset(ei, el, dev, channels=cin)
    if not n_train:
        return None, eds
    ti, tl = make_synthetic(n_train, seed=4, device=dev, channels=cin)
    return DeviceDataset(ti, tl, dev, channels=cin), eds


@pytest.mark.parametrize("model,cin", [("lenet5", 1), ("reference_cnn", 3)])
def test_eval_split_with_smaller_final_batch(dev, K, model, cin):
    """A4.  Replica.evaluate's arithmetic: eval_batches + eval_batch over 100 examples at B = 64
    (batches of 64 and 36) accumulate st[:2]; st[:2] / 100 is the float64 mean loss and the
    tie-rule accuracy of the per-batch logits."""
    _, eds = _datasets(dev, cin)
    _, _, net = _build(dev, model, cin, "bf16", batch=64)
    st = net.eval_stats
    st.zero_()
    seen = []
    assert _eval_pass(net, eds, st, seen) == 100 and [len(l) for _, l in seen] == [64, 36]
    torch.cuda.synchronize()
    ce = sum(so.ce_sum(lg, lab) for lg, lab in seen)
    cnt = sum(so.top1_count(lg, lab) for lg, lab in seen)
    loss, acc = (st[:2] / 100).tolist()
    print(f"{model}{cin}: mean loss {loss!r} vs {ce / 100!r}, accuracy {acc!r} vs {cnt / 100!r}")
    assert st[1].item() == cnt and abs(acc - cnt / 100) <= 1e-7
    assert abs(loss - ce / 100) <= so.ce_tol(ce) / 100
    assert st[2].item() == 0.0


# ------------------------------------------------------------------ B. eval must not perturb training
def _train_run(dev, model, cin, with_eval, graph):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import DeviceLoader
    from distributed_tensorflow_ibm_mnist_amd.runtime.graph import StepGraph
    ds, eds = _datasets(dev, cin, n_train=1000)
    opt = OptConfig(lr0=0.02, use_momentum=True, momentum=0.9, ema_max=0.9999)
    _, _, net = _build(dev, model, cin, "bf16", batch=64, seed=3, opt=opt)
    assert net.bind_u8_input(ds.bf16_images(), bwd_images=ds.images)
    loader = DeviceLoader(ds, net.x0, net.labels, seed=9, idx_out=net.idx_buf)
    g = None
    for i in range(4):
        loader.next()
        if graph and g is None:
            g = StepGraph(net.train_step, warmup=1)     # the warm-up is this step; capture runs nothing
        elif graph:
            g.replay()
        else:
            net.train_step()
        if with_eval and i < 3:
            net.eval_stats.zero_()
            assert _eval_pass(net, eds, net.eval_stats) == 100
            assert net.eval_stats[0].item() > 0
    torch.cuda.synchronize()
    fp = net.fp
    return {"params": fp.params.clone(), "mom": fp.mom.clone(), "ema": fp.ema.clone(),
            "loss_ema": net.loss_ema.clone(), "stats[4:8]": net.stats[4:8].clone(), "step": fp.step.clone()}


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("model,cin", [("lenet5", 1), ("reference_cnn", 3)])
def test_eval_between_steps_does_not_perturb_training(dev, K, model, cin, graph):
    """4 training steps on a bound resident dataset (bf16, DeviceLoader idx_out) with a 100-example
    eval pass (batches 64 + 36) between every two steps == the same 4 steps without eval, bitwise:
    the eval pass clears use_u8 and overwrites x0, labels and ce_work, and neither an eager step
    nor a replayed one may care."""
    ref = _train_run(dev, model, cin, False, graph)
    got = _train_run(dev, model, cin, True, graph)
    assert int(ref["step"].item()) == 4
    assert float(ref["stats[4:8]"][3]) == 4.0 and bool(torch.isfinite(ref["params"]).all())
    for k in ref:
        assert torch.equal(got[k], ref[k]), k


# ------------------------------------------------------------------ C. the NaN flag
def _tail_inputs(dev, nb, extra=40, wscale=0.2):
    """test_ce_tail_matches_oracle's inputs with ``extra`` more rows in every row buffer; the
    label of row nb - 1 (class 9) occurs nowhere else."""
    torch.manual_seed(nb)
    n = nb + extra
    x = torch.relu(torch.randn(n, 192, device=dev)).to(torch.bfloat16)
    w = (torch.randn(192, 10, device=dev) * wscale).to(torch.bfloat16)
    wt = torch.zeros(16, 192, dtype=torch.bfloat16, device=dev)
    wt[:10] = w.t()
    b = torch.randn(10, device=dev) * 0.1
    y = torch.randint(0, 9, (n,), device=dev, dtype=torch.int32)
    y[nb - 1] = 9
    return x, w, wt, b, y


def _run_tail(K, dev, mode, x, wt, b, y, nb):
    """One ce_tail launch; returns (stats after the launch / the step's finalize, logits, dl, dx).
    mode: "ticket" (last block combines), "defer" (finalize_step combines, as HipNet.finalize)
    or "eval" (no gradients)."""
    n = x.shape[0]
    logits = torch.full((n, 16), SENT, device=dev)
    dl = torch.full((n, 16), SENT, dtype=torch.bfloat16, device=dev)
    dx = torch.full((n, 192), SENT, dtype=torch.bfloat16, device=dev)
    stats = torch.zeros(8, device=dev)
    work = torch.zeros(4 * 1024 + 1, device=dev)
    nblk = K.ce_tail_blocks(nb)
    if mode == "eval":
        K.ce_tail(x, wt, b, 10, y, nb, 1.0, logits, stats=stats, work=work)
    else:
        dbias = torch.zeros(nblk * 16, device=dev)
        K.ce_tail(x, wt, b, 10, y, nb, 1.0 / nb, logits, dl=dl, dx=dx, stats=stats, work=work,
                  defer_stats=mode == "defer", dbias=dbias)
    if mode == "defer":
        assert stats[:3].tolist() == [0.0, 0.0, 0.0]        # nothing combined yet
        K.finalize_step(torch.zeros(1, dtype=torch.int64, device=dev), stats, None, None, 0, None, 0, nb, False,
                        None, work, nblk)
    torch.cuda.synchronize()
    return stats.tolist(), logits, dl, dx


@pytest.mark.parametrize("mode", ["ticket", "defer", "eval"])
@pytest.mark.parametrize("nb", [1, 77, 300])
def test_ce_tail_nan_flag(dev, K, nb, mode):
    """C1.  ce_tail_k raises stats[2] for one poisoned row at index nb - 1 (the last partial
    wave) -- a NaN input, a -inf bias of its label class (loss +inf), a +inf bias entry -- on the
    ticket path, the deferred path (after the step's finalize) and the eval form; a NaN in a
    buffer row past nb raises nothing and changes nothing."""
    x, w, wt, b, y = _tail_inputs(dev, nb)
    ctl, lg, _, _ = _run_tail(K, dev, mode, x, wt, b, y, nb)
    assert ctl[2] == 0.0
    ce, cnt = so.ce_sum(lg[:nb, :10], y[:nb]), so.top1_count(lg[:nb, :10], y[:nb])
    loss, corr = (ctl[4] * nb, ctl[5] * nb) if mode == "defer" else (ctl[0], ctl[1])
    so.check_ce(loss, ce, "control")
    assert round(corr) == cnt and abs(corr - cnt) < 1e-3
    assert bool((lg[nb:] == SENT).all())

    xp = x.clone()
    xp[nb - 1, 5] = NAN
    assert _run_tail(K, dev, mode, xp, wt, b, y, nb)[0][2] == 1.0, "NaN input row"
    bp = b.clone()
    bp[9] = -INF
    st, lgp, _, _ = _run_tail(K, dev, mode, x, wt, bp, y, nb)
    assert st[2] == 1.0, "-inf bias of the label class"
    assert bool(torch.isinf(lgp[nb - 1, 9])) and bool(torch.isfinite(lgp[:nb, :9]).all())
    bp = b.clone()
    bp[4] = INF
    assert _run_tail(K, dev, mode, x, wt, bp, y, nb)[0][2] == 1.0, "+inf bias entry"
    xp = x.clone()
    xp[nb:] = NAN
    st, lgp, dlp, dxp = _run_tail(K, dev, mode, xp, wt, b, y, nb)
    assert st == ctl, "rows past nb reached the statistics"
    assert torch.equal(lgp, lg)
    assert bool((dlp[nb:] == SENT).all()) and bool((dxp[nb:] == SENT).all())


def _ce_launch(K, dev, kind, logits, ld, y, nb, mode, scale=1.0, grads=False):
    """softmax_ce (rows kernel at ld 16 / 32, generic kernel otherwise) or f32_softmax_ce;
    returns (stats list with [0], [1] the loss sum and top-1 count, dlogits or None)."""
    stats = torch.zeros(8, device=dev)
    work = torch.zeros(4 * 1024 + 1, device=dev) if mode in ("ticket", "defer") else None
    n = logits.shape[0]
    if kind == "f32":
        dl = torch.full((n, ld), SENT, device=dev) if grads else None
        K.f32_softmax_ce(logits, ld, y, nb, 10, scale, dl, ld, stats, None, work)
    else:
        dl = torch.full((n, ld), SENT, dtype=torch.bfloat16, device=dev) if grads else None
        nblk = K.softmax_ce(logits, ld, y, nb, 10, scale, dl, ld, stats, None, work, defer_stats=mode == "defer")
        if mode == "defer":
            assert nblk > 0 and stats[:3].tolist() == [0.0, 0.0, 0.0]
            K.finalize_step(torch.zeros(1, dtype=torch.int64, device=dev), stats, None, None, 0, None, 0, 1, False,
                            None, work, nblk)      # batch 1: stats[4], [5] are the sums themselves
    torch.cuda.synchronize()
    st = stats.tolist()
    if mode == "defer":
        st[0], st[1] = st[4], st[5]
    return st, dl


# (kernel, row stride, statistics path): the rows kernel's three combines, the generic kernel's
# atomics, the fp32 kernel's ticket and atomic paths
CE_KERNELS = [("bf16", 16, "ticket"), ("bf16", 16, "defer"), ("bf16", 16, "atomic"), ("bf16", 32, "ticket"),
              ("bf16", 32, "defer"), ("bf16", 24, "atomic"), ("f32", 10, "ticket"), ("f32", 10, "atomic")]
CE_IDS = [f"{k}-ld{l}-{m}" for k, l, m in CE_KERNELS]


@pytest.mark.parametrize("kind,ld,mode", CE_KERNELS, ids=CE_IDS)
@pytest.mark.parametrize("nb", [1, 77, 300])
def test_softmax_ce_nan_flag(dev, K, nb, kind, ld, mode):
    """C2.  The layered softmax-CE kernels raise stats[2] for one poisoned fp32 logits row at
    index nb - 1: NaN at the label class, -inf at the label class (loss +inf), a +inf entry, a
    NaN in a non-label class; NaN rows past nb raise nothing."""
    torch.manual_seed(100 + nb)
    n = nb + 40
    logits = torch.zeros(n, ld, device=dev)
    logits[:, :10] = torch.randn(n, 10, device=dev) * 3
    y = torch.randint(0, 9, (n,), device=dev, dtype=torch.int32)
    y[nb - 1] = 9
    ctl, _ = _ce_launch(K, dev, kind, logits, ld, y, nb, mode)
    assert ctl[2] == 0.0
    so.check_ce(ctl[0], so.ce_sum(logits[:nb, :10], y[:nb]), "control")
    assert ctl[1] == so.top1_count(logits[:nb, :10], y[:nb])
    for what, col, v in [("NaN at the label class", 9, NAN), ("-inf at the label class", 9, -INF),
                         ("+inf entry", 4, INF), ("NaN in a non-label class", 2, NAN)]:
        lp = logits.clone()
        lp[nb - 1, col] = v
        assert _ce_launch(K, dev, kind, lp, ld, y, nb, mode)[0][2] == 1.0, what
    lp = logits.clone()
    lp[nb:] = NAN
    st, _ = _ce_launch(K, dev, kind, lp, ld, y, nb, mode)
    assert st[2] == 0.0 and st[1] == ctl[1]
    so.check_ce(st[0], so.ce_sum(logits[:nb, :10], y[:nb]), "NaN rows past nb")


def _partials(dev, nblk, bad_at):
    """Hand-written per-block CE partials whose sums are exact in fp32 in any order."""
    work = torch.zeros(4 * 1024 + 1, device=dev)
    i = torch.arange(nblk, device=dev)
    w = work[:4 * nblk].view(nblk, 4)
    w[:, 0] = (i % 7).float() * 0.25
    w[:, 1] = (i % 3).float()
    if bad_at is not None:
        w[bad_at, 2] = 1.0
    return work, float(((i % 7).double() * 0.25).sum()), float((i % 3).sum())


@pytest.mark.parametrize("nblk", [1, 65, 600, 1024])
def test_finalize_combines_deferred_partials(dev, K, nblk):
    """The deferred combine's contract (ce_stats.h): finalize_step sums every block's loss and
    count partial and raises stats[2] when ANY block's bad partial is set, first or last --
    also where the loss partials themselves are finite, so the flag cannot ride on
    !isfinite(total)."""
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    for bad_at in (None, 0, nblk - 1):
        work, loss, corr = _partials(dev, nblk, bad_at)
        stats = torch.zeros(8, device=dev)
        K.finalize_step(step, stats, None, None, 0, None, 0, 1, False, None, work, nblk)
        torch.cuda.synchronize()
        st = stats.tolist()
        assert st[4] == loss and st[5] == corr, (bad_at, st)
        assert st[2] == (0.0 if bad_at is None else 1.0), (bad_at, st)


@pytest.mark.parametrize("fin_fused", [0, 1])
def test_update_combines_deferred_partials(dev, K, fin_fused):
    """The same contract where the optimizer launch's last block runs the step's finalize
    (set_opt_fin_fused(1)) and on the two-launch path (0), through HipNet.update()."""
    prev = K.opt_fin_fused_enabled()
    K.set_opt_fin_fused(fin_fused)
    try:
        for bad_at in (None, 0, 64):
            _, _, net = _build(dev, "mlp", 1, "bf16", batch=64)
            work, loss, corr = _partials(dev, 65, bad_at)
            net.ce_work.copy_(work)
            net._ce_defer_blocks = 65
            net.update()
            torch.cuda.synchronize()
            st = net.stats.tolist()
            assert st[4] == loss / 64 and st[5] == corr / 64, st      # exact: quarters over a power of two
            assert st[2] == (0.0 if bad_at is None else 1.0), (bad_at, st)
    finally:
        K.set_opt_fin_fused(int(prev))


def _fixed_batch(net, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    net.x0.copy_((torch.rand(net.x0.shape, generator=g) - 0.5).to(torch.bfloat16).to(dev))
    net.labels.copy_(torch.randint(0, 10, (net.B,), generator=g, dtype=torch.int32).to(dev))


def _last_bias(net):
    name = f"{net.spec.weights()[-1].name}/biases"
    assert name == "softmax_linear/biases"
    return net.fp.param_view(name)


@pytest.mark.parametrize("fin_fused", [0, 1])
@pytest.mark.parametrize("model", ["lenet5", "reference_cnn"])
def test_step_nan_flag_is_raised_and_sticky(dev, K, model, fin_fused):
    """C3.  A NaN, or a +inf, in one element of the last bias (the one position that passes no
    ReLU) makes train_step() raise read_stats()["nan"]; two further steps keep it (the hook
    relies on "never cleared"); three clean steps read 0.  Fused head / tail, whose deferred
    partials the optimizer launch (1) or finalize_k (0) combines."""
    prev = K.opt_fin_fused_enabled()
    K.set_opt_fin_fused(fin_fused)
    try:
        for poison in (None, NAN, INF):
            _, _, net = _build(dev, model, 1, "bf16", batch=64,
                               opt=OptConfig(lr0=0.05, use_momentum=True, momentum=0.9))
            _fixed_batch(net, dev)
            if poison is not None:
                _last_bias(net)[3] = poison
            seen = []
            for _ in range(3):
                net.train_step()
                torch.cuda.synchronize()
                seen.append(net.read_stats()["nan"])
            assert seen == [0.0 if poison is None else 1.0] * 3, (poison, seen)
    finally:
        K.set_opt_fin_fused(int(prev))


@pytest.mark.parametrize("model", ["lenet5", "reference_cnn"])
def test_step_nan_flag_under_graph_replay(dev, K, model):
    """C3, hipGraph: the poison is written between replays of one captured step."""
    from distributed_tensorflow_ibm_mnist_amd.runtime.graph import StepGraph
    _, _, net = _build(dev, model, 1, "bf16", batch=64, opt=OptConfig(lr0=0.05, use_momentum=True, momentum=0.9))
    _fixed_batch(net, dev)
    g = StepGraph(net.train_step, warmup=1)
    g.replay()
    torch.cuda.synchronize()
    assert net.read_stats()["nan"] == 0.0 and int(net.fp.step.item()) == 2
    _last_bias(net)[3] = NAN
    seen = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        seen.append(net.read_stats()["nan"])
    assert seen == [1.0, 1.0, 1.0]


def test_nan_weight_reaches_flag_through_total_loss(dev, K):
    """C4.  A NaN in conv1/weights of LeNet-5 never reaches the cross-entropy: the conv's
    fmaxf(v, 0) ReLU turns the NaN pre-activations into 0.  The flag rises through the total
    loss instead, at the FIRST step after the injection: conv1/weights is a weight-decay entry
    (coefficient 0.0), the optimizer launch of that step sums w^2 of the pre-update weights
    (NaN), and the step's finalize computes total = ce + 0.0 * 0.5 * NaN = NaN, which
    !isfinite(total) catches.  This is the only route by which train/replica.py inject_nan
    (params[0]) reaches the guard on the HIP path."""
    _, _, net = _build(dev, "lenet5", 1, "bf16", batch=64, opt=OptConfig(lr0=0.05))
    e = net.fp.by_name["conv1/weights"]
    assert e in net.fp.wd_entries and float(e.wd) == 0.0 and e.off == 0
    _fixed_batch(net, dev)
    net.fp.params[0] = NAN
    net.fp.refresh_bf16()
    assert bool(torch.isnan(net.fp.bf16_view("conv1/weights").float()).any())
    net.train_step()
    torch.cuda.synchronize()
    st = net.read_stats()
    print(st)
    assert st["nan"] == 1.0
    assert np.isfinite(st["cross_entropy"]) and np.isnan(st["total_loss"])


# ------------------------------------------------------------------ D. extreme logits
def _extreme_logits(dev, nb, ld):
    torch.manual_seed(7)
    lg = torch.zeros(nb, ld, device=dev)
    lg[:, :10] = torch.randn(nb, 10, device=dev) * 3
    y = torch.randint(0, 10, (nb,), device=dev, dtype=torch.int32)
    lg[0, :10] = 0.0
    lg[0, 0], lg[0, 1] = 1e4, -1e4
    y[0] = 1                                   # loss 2e4
    lg[1, :10] = 0.0
    lg[1, 0], lg[1, 1] = 1e4, -1e4
    y[1] = 0                                   # loss ~0
    lg[2, :10] = 3e38
    lg[3, :10] = -3e38
    lg[4, :10] = torch.linspace(-88.8, 88.8, 10, device=dev)
    y[4] = 0                                   # loss 177.6
    lg[5, :10] = torch.linspace(-88.8, 88.8, 10, device=dev)
    y[5] = 9
    lg[nb - 1, :10] = 0.0
    lg[nb - 1, 9], lg[nb - 1, 3] = 1e4, -1e4
    y[nb - 1] = 9
    return lg, y


@pytest.mark.parametrize("kind,ld", [("bf16", 10), ("bf16", 16), ("bf16", 24), ("bf16", 32), ("bf16", 40),
                                     ("f32", 10), ("f32", 16)])
def test_softmax_ce_extreme_logits(dev, K, kind, ld):
    """D1.  +-1e4, all-equal +-3e38 and +-88.8 (the overflow edge of exp) rows among ordinary
    ones: a softmax that did not subtract the row maximum overflows on them.  Loss against the
    float64 log-sum-exp, no NaN flag, dlogits against float64 (softmax - onehot) * scale to one
    bf16 rounding, padding columns exactly 0; every launchable row stride."""
    nb = 77
    lg, y = _extreme_logits(dev, nb, ld)
    scale = 1.0 / nb
    mode = "ticket" if (kind == "f32" or ld in (16, 32)) else "atomic"
    st, dl = _ce_launch(K, dev, kind, lg, ld, y, nb, mode, scale=scale, grads=True)
    assert st[2] == 0.0
    so.check_ce(st[0], so.ce_sum(lg[:, :10], y), f"{kind} ld={ld}")
    assert st[1] == so.top1_count(lg[:, :10], y)
    assert bool(torch.isfinite(dl.float()).all())
    so.check_dlogits(dl[:, :10], lg[:, :10], y, scale, f"{kind} ld={ld}")
    assert not dl[:, 10:].any()
    if kind == "bf16":
        pr = torch.empty(nb, 10, device=dev)
        K.softmax_ce(lg, ld, None, nb, 10, 1.0, None, ld, None, pr)
        torch.cuda.synchronize()
        so.check_probs(pr, lg[:, :10], f"probs ld={ld}")


@pytest.mark.parametrize("mode", ["ticket", "defer", "eval"])
def test_ce_tail_extreme_logits(dev, K, mode):
    """D2.  ce_tail_k with weights scaled until its own |logits| pass 1e3: loss, flag and
    dlogits from the kernel's own logits against float64, dx as test_ce_tail_matches_oracle."""
    nb = 77
    x, w, wt, b, y = _tail_inputs(dev, nb, extra=0, wscale=200.0)
    st, lg, dl, dx = _run_tail(K, dev, mode, x, wt, b, y, nb)
    lg = lg[:, :10]
    assert lg.abs().max().item() >= 1e3, "the logits must be extreme for this test to mean anything"
    assert st[2] == 0.0
    loss, corr = (st[4] * nb, st[5] * nb) if mode == "defer" else (st[0], st[1])
    so.check_ce(loss, so.ce_sum(lg, y), mode)
    assert round(corr) == so.top1_count(lg, y) and abs(corr - round(corr)) < 1e-3
    if mode != "eval":
        so.check_dlogits(dl[:, :10], lg, y, 1.0 / nb, mode)
        assert not dl[:, 10:].any()
        gx = (dl[:, :10].float() @ w.float().t()) * (x.float() > 0)
        assert (dx.float() - gx).abs().max().item() <= 2 ** -7 * gx.abs().max().item()
        assert not dx[x == 0].any()


def test_mlp_head_extreme_logits(dev, K):
    """D3.  The fused LeNet-5 head with softmax_linear/weights scaled by 1e3 in fp.params
    (FlatParams.refresh_bf16() rebuilds the bf16 and the transposed copies the head stages):
    forward(defer_head=True); loss_and_grad(); finalize(B, increment=False), same checks."""
    nb = 77
    _, _, net = _build(dev, "lenet5", 1, "bf16", batch=nb)
    net.fp.param_view("softmax_linear/weights").mul_(1e3)
    net.fp.refresh_bf16()
    _fixed_batch(net, dev)
    net.forward(defer_head=True)
    net.loss_and_grad()
    net.finalize(nb, increment=False)
    torch.cuda.synchronize()
    lg, y = net.logits[:, :10].clone(), net.labels
    print("max logit", lg.max().item(), "max |logit|", lg.abs().max().item())
    assert lg.max().item() >= 100.0, "past the overflow edge of exp (88.7), or the test goes soft"
    st = net.stats.tolist()
    assert st[2] == 0.0
    so.check_ce(st[4] * nb, so.ce_sum(lg, y), "mlp_head")
    cnt = so.top1_count(lg, y)
    assert round(st[5] * nb) == cnt and abs(st[5] * nb - cnt) < 1e-3
    so.check_dlogits(net.dlogits[:, :10], lg, y, 1.0 / nb, "mlp_head")
    assert not net.dlogits[:, 10:].any() and not net.logits[:, 10:].any()


# ------------------------------------------------------------------ E. the tie rule
TIE = [0.1, 0.2, 1.5, 0.3, -1.0, 0.0, 0.4, 1.5, 0.2, -0.3]      # two equal maxima: classes 2 and 7
DEAD = [0.25] * 10                                              # a dead network: every class ties
BIASES = {"two_maxima": (TIE, (2, 7)), "all_equal": (DEAD, tuple(range(10)))}


def _expected(nb, winners):
    return sum(1 for r in range(nb) if r % 10 in winners)


@pytest.mark.parametrize("bias", list(BIASES))
@pytest.mark.parametrize("kind,ld,mode", CE_KERNELS, ids=CE_IDS)
def test_tie_rule_softmax_ce(dev, K, kind, ld, mode, bias):
    """E.  Exact ties at the maximum count for every tied class (logit[label] >= max): labels
    cycle over 0..9, and the correct count is exactly the rows whose label is a tied maximum;
    one extra row has all logits equal, where every label counts."""
    nb = 77
    vals, winners = BIASES[bias]
    lg = torch.zeros(nb, ld, device=dev)
    lg[:, :10] = torch.tensor(vals, device=dev)
    lg[nb - 1, :10] = -3.0                       # the all-equal row (label 6)
    y = (torch.arange(nb, device=dev) % 10).to(torch.int32)
    st, _ = _ce_launch(K, dev, kind, lg, ld, y, nb, mode)
    want = _expected(nb - 1, winners) + 1
    assert st[1] == want == so.top1_count(lg[:, :10], y)
    so.check_ce(st[0], so.ce_sum(lg[:, :10], y), "tie rows")


@pytest.mark.parametrize("bias", list(BIASES))
@pytest.mark.parametrize("mode", ["ticket", "defer", "eval"])
def test_tie_rule_ce_tail(dev, K, mode, bias):
    """E.  ce_tail_k with a zero W5t: the logits are the bias."""
    nb = 77
    vals, winners = BIASES[bias]
    x, _, wt, _, _ = _tail_inputs(dev, nb, extra=0)
    wt.zero_()
    b = torch.tensor(vals, device=dev)
    y = (torch.arange(nb, device=dev) % 10).to(torch.int32)
    st, lg, _, _ = _run_tail(K, dev, mode, x, wt, b, y, nb)
    assert torch.equal(lg[:, :10], b.expand(nb, 10))
    corr = st[5] * nb if mode == "defer" else st[1]
    assert round(corr) == _expected(nb, winners) and abs(corr - round(corr)) < 1e-3


@pytest.mark.parametrize("bias", list(BIASES))
@pytest.mark.parametrize("model", ["lenet5", "reference_cnn"])
def test_tie_rule_executor(dev, K, model, bias):
    """E.  The fused head (mlp_head_k) and tail through HipNet with softmax_linear/weights
    zeroed: eval_batch on a partial batch and the training step agree with the in_top_k rule."""
    vals, winners = BIASES[bias]
    _, _, net = _build(dev, model, 1, "bf16", batch=B)
    net.fp.param_view("softmax_linear/weights").zero_()
    _last_bias(net).copy_(torch.tensor(vals, device=dev))
    net.fp.refresh_bf16()
    _fixed_batch(net, dev)
    net.labels.copy_((torch.arange(B, device=dev) % 10).to(torch.int32))
    st = torch.zeros(8, device=dev)
    net.eval_batch(77, st)
    torch.cuda.synchronize()
    assert torch.equal(net.logits[:77, :10], torch.tensor(vals, device=dev).expand(77, 10))
    assert st[1].item() == _expected(77, winners)
    net.forward(defer_head=True)
    net.loss_and_grad()
    net.finalize(B, increment=False)
    torch.cuda.synchronize()
    assert round(net.stats[5].item() * B) == _expected(B, winners)
    assert abs(net.stats[5].item() - _expected(B, winners) / B) <= 1e-7
