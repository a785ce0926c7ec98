"""The evaluation-metrics kernel (csrc/kernels/eval_metrics.hip) against the float64 host
reference (obs/eval_metrics.py), and its wiring through the executors, Replica.evaluate and the
two command-line tools.

Rules of comparison
* ``pred``, ``rank``, ``confusion``, ``rank_hist`` and the three row counts are exact.
* ``bin``: the integer accumulators equal the aggregation of the device's own per-row records;
  against the oracle a row's bin is exact unless ``conf * NB`` (float64) lies within 1e-4 of an
  integer, and at most 1 % of a case's rows may be such edge rows (asserted on the oracle alone).
* ``conf``, ``nll`` and ``brier``: the device may be 4 times as far from the float64 oracle as a
  numpy float32 transcription of the definition (``f32_transcription`` below) is at its worst over
  this file's kernel-level inputs with the same class count (the error grows with the number of
  terms of the sums); a sum over rows may be ``n_labelled`` times that.
"""
import gc
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

from distributed_tensorflow_ibm_mnist_amd.obs import eval_metrics as E
from distributed_tensorflow_ibm_mnist_amd.obs import events

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A
EDGE = 1e-4
Case = namedtuple("Case", "name nb B ld NC bf16 T s NB cap seed")
CASES = [
    Case("one_row", 1, 4, 16, 10, False, 1.0, 1, 15, 0, 0),
    Case("63_ld_is_nc_bf16", 63, 64, 10, 10, True, 2.5, 3, 15, 0, 1),
    Case("64_two_classes", 64, 70, 2, 2, False, 1.0, 3, 15, 0, 2),
    Case("65_32_classes_bf16", 65, 80, 32, 32, True, 1.0, 1, 15, 0, 3),
    Case("257_bf16", 257, 300, 16, 10, True, 1.0, 3, 15, 0, 4),
    Case("257_f32_t_64_bins", 257, 260, 16, 10, False, 2.5, 1, 64, 0, 5),
    Case("257_two_classes_bf16_one_bin", 257, 258, 16, 2, True, 2.5, 1, 1, 0, 6),
    Case("257_32_classes_f32", 257, 259, 32, 32, False, 2.5, 3, 15, 0, 7),
    Case("257_ld_is_nc_f32", 257, 258, 10, 10, False, 1.0, 1, 15, 0, 8),
    Case("4096_capped_f32", 4096, 4100, 16, 10, False, 1.0, 3, 15, 3, 9),
    Case("4096_capped_bf16_ld32", 4096, 4097, 32, 10, True, 2.5, 1, 15, 5, 10),
    Case("65_odd_ld_bf16", 65, 66, 11, 10, True, 1.0, 3, 15, 0, 11),     # rows aligned to 2 bytes only
]


def make_case(c):
    """(logits [B, ld] fp32 holding bf16-exact values, labels int32 [B]): real columns are
    bf16-rounded randn * s; the columns from NC on hold +1e30 in even rows and NaN in odd ones;
    the rows from nb on hold NaN; ties, unlabelled and bad rows are planted where there is room."""
    rng = np.random.default_rng(100 + c.seed)
    L = torch.from_numpy((rng.standard_normal((c.B, c.ld)) * c.s).astype(np.float32)).bfloat16().float().numpy()
    y = rng.integers(0, c.NC, c.B).astype(np.int32)
    if c.nb >= 16:
        L[0, 0] = L[0, c.NC - 1] = 8.0        # a tie at the maximum, the true class the higher index
        y[0] = c.NC - 1
        L[1, 0] = L[1, 1]                     # a tie with the true class
        y[1] = 1
        L[2, :c.NC] = 0.25
        y[2] = c.NC - 1
        y[3] = -1
        y[4] = c.NC
        y[5] = 1 << 30
        L[6, c.NC - 1] = np.inf
        L[7, 0] = np.nan
        L[8, 1] = -np.inf
    L[0::2, c.NC:] = 1e30
    L[1::2, c.NC:] = np.nan
    L[c.nb:] = np.nan
    return L, y


def f32_transcription(L, y, NC, T, NB):
    """The definition in numpy float32, every operation rounded on its own, sums in class order.
    Per good row: conf; per labelled row: nll, brier (NaN elsewhere)."""
    f = np.float32
    l = L[:, :NC].astype(f)
    n = l.shape[0]
    good = np.isfinite(l).all(axis=1)
    conf, nll, brier = (np.full(n, np.nan, f) for _ in range(3))
    g = l[good]
    with np.errstate(all="ignore"):
        mx = g.max(axis=1)
        d = ((g - mx[:, None]).astype(f) * (f(1) / f(T))).astype(f)
        e = np.exp(d).astype(f)
        se = np.zeros(g.shape[0], f)
        for c in range(NC):
            se = (se + e[:, c]).astype(f)
        conf[good] = (f(1) / se).astype(f)
        yy = y[good].astype(np.int64)
        lab = (yy >= 0) & (yy < NC)
        idx = np.nonzero(lab)[0]
        yl = yy[lab]
        nl = (np.log(se[lab]).astype(f) - d[idx, yl]).astype(f)
        q = (e[lab] / se[lab][:, None]).astype(f)
        q[np.arange(len(yl)), yl] = (q[np.arange(len(yl)), yl] - f(1)).astype(f)
        q2 = (q * q).astype(f)
        br = np.zeros(len(yl), f)
        for c in range(NC):
            br = (br + q2[:, c]).astype(f)
    gi = np.nonzero(good)[0][lab]
    nll[gi], brier[gi] = nl, br
    return conf, nll, brier


def oracle_rows(L, y, NC, T):
    """float64 per-row conf (good rows), nll and brier (labelled rows), NaN elsewhere."""
    n = L.shape[0]
    l = L[:, :NC].astype(np.float64)
    good = np.isfinite(l).all(axis=1)
    conf, nll, brier = (np.full(n, np.nan) for _ in range(3))
    for i in np.nonzero(good)[0]:
        d = (l[i] - l[i].max()) * (1.0 / T)
        e = np.exp(d)
        se = 0.0
        for c in range(NC):
            se += e[c]
        conf[i] = 1.0 / se
        if 0 <= y[i] < NC:
            nll[i] = np.log(se) - d[y[i]]
            q = e / se
            q[y[i]] -= 1.0
            b = 0.0
            for c in range(NC):
                b += q[c] * q[c]
            brier[i] = b
    return conf, nll, brier


def _worst(a, b):
    m = np.isfinite(b)
    assert np.array_equal(m, np.isfinite(a))
    return float(np.abs(a[m].astype(np.float64) - b[m]).max()) if m.any() else 0.0


@pytest.fixture(scope="module")
def world():
    """Inputs, oracle and bounds of every kernel-level case, computed once and never changed."""
    out, err = {}, {}
    for c in CASES:
        L, y = make_case(c)
        Ln, yn = L[:c.nb], y[:c.nb]
        acc, rows = E.reference(Ln, yn, c.NC, c.T, c.NB, rows=True)
        o = oracle_rows(Ln, yn, c.NC, c.T)
        t = f32_transcription(Ln, yn, c.NC, c.T, c.NB)
        e = err.setdefault(c.NC, [0.0, 0.0, 0.0])
        for k in range(3):
            e[k] = max(e[k], _worst(t[k], o[k]))
        out[c.name] = dict(L=L, y=y, acc=acc, rows=rows, oracle=o)
    for c in CASES:
        out[c.name]["tol"] = [4.0 * v for v in err[c.NC]]
    return out


def device_inputs(c, w, dev):
    L = torch.from_numpy(w["L"]).to(dev)
    if c.bf16:
        L = L.bfloat16()
    return L.contiguous(), torch.from_numpy(w["y"]).to(dev)


def run_kernel(K, c, L, y, nb=None, acc=None, rows=None):
    lay = K.eval_metrics_layout(c.NC, c.NB)
    dev = L.device
    if acc is None:
        acc = (torch.zeros(lay["size_i"], dtype=torch.int64, device=dev),
               torch.zeros(lay["size_f"], dtype=torch.float64, device=dev))
    scratch = torch.full((K.eval_metrics_scratch_size(c.NB),), float("nan"), dtype=torch.float64, device=dev)
    K.eval_metrics(L, y, c.nb if nb is None else nb, c.NC, acc[0], acc[1], scratch, rows, c.T, c.NB)
    return acc


def unpack(K, NC, NB, acc_i, acc_f):
    lay = K.eval_metrics_layout(NC, NB)
    i, f = acc_i.cpu().numpy(), acc_f.cpu().numpy()
    cut = lambda a, k, n: a[lay[k]:lay[k] + n]  # noqa: E731
    return {"confusion": cut(i, "confusion", (NC + 1) * NC).reshape(NC + 1, NC), "rank_hist": cut(i, "rank_hist", NC),
            "bin_count": cut(i, "bin_count", NB), "bin_correct": cut(i, "bin_correct", NB),
            "n_rows": int(i[lay["counts"]]), "n_labelled": int(i[lay["counts"] + 1]), "n_bad": int(i[lay["counts"] + 2]),
            "bin_conf_sum": cut(f, "bin_conf_sum", NB), "nll_sum": float(f[lay["nll_sum"]]),
            "brier_sum": float(f[lay["brier_sum"]])}


def check(got, rows, want, wrows, oracle, tol, NC, NB, what):
    """The rules of the module docstring: device accumulators ``got`` and per-row records ``rows``
    against the oracle's ``want`` / ``wrows`` / per-row float64 ``oracle``."""
    n = wrows.shape[0]
    conf64, nll64, brier64 = oracle
    # the condition on the inputs, on the oracle alone
    lab = wrows[:, 1] >= 0
    x = conf64 * NB
    edge = lab & (np.abs(x - np.round(x)) < EDGE)
    assert edge.sum() <= 0.01 * n, f"{what}: {edge.sum()} edge rows of {n}"
    # exact
    assert np.array_equal(rows[:, 0], wrows[:, 0]), f"{what}: pred"
    assert np.array_equal(rows[:, 1], wrows[:, 1]), f"{what}: rank"
    for k in ("confusion", "rank_hist"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k}"
    for k in ("n_rows", "n_labelled", "n_bad"):
        assert got[k] == want[k], f"{what}: {k} {got[k]} != {want[k]}"
    # bins
    b = rows[:, 2]
    assert np.array_equal(b >= 0, lab) and (b[lab] < NB).all(), f"{what}: bin range"
    assert np.array_equal(got["bin_count"], np.bincount(b[lab], minlength=NB)), f"{what}: bin_count"
    assert np.array_equal(got["bin_correct"], np.bincount(b[lab & (rows[:, 1] == 0)], minlength=NB)), f"{what}: bin_correct"
    assert np.array_equal(b[~edge], wrows[~edge, 2]), f"{what}: bin"
    assert (np.abs(b[edge] - wrows[edge, 2]) <= 1).all()
    # conf of every row: NaN bits on a bad row
    bad = wrows[:, 0] < 0
    assert (rows[bad, 3].view(np.uint32) == 0x7FC00000).all() and (rows[bad, :3] == -1).all(), f"{what}: bad rows"
    conf = rows[:, 3].copy().view(np.float32).astype(np.float64)
    e_conf = float(np.abs(conf[~bad] - conf64[~bad]).max()) if (~bad).any() else 0.0
    n_lab = int(lab.sum())
    by_bin = np.zeros(NB)
    np.add.at(by_bin, b[lab], conf64[lab])
    e_bins = float(np.abs(got["bin_conf_sum"] - by_bin).max())
    e_nll = abs(got["nll_sum"] - float(nll64[lab].sum()))
    e_brier = abs(got["brier_sum"] - float(brier64[lab].sum()))
    # every figure before it is asserted (pytest -s shows them)
    print(f"{what}: conf {e_conf:.3e} (bound {tol[0]:.3e})  bin_conf_sum {e_bins:.3e}  nll_sum {e_nll:.3e} "
          f"(per row bound {tol[1]:.3e})  brier_sum {e_brier:.3e} (per row bound {tol[2]:.3e})  "
          f"n_labelled {n_lab}  edge rows {int(edge.sum())}  bins off {int((b != wrows[:, 2]).sum())}")
    assert e_conf <= tol[0], f"{what}: conf off by {e_conf}, bound {tol[0]}"
    assert e_bins <= n_lab * tol[0], f"{what}: bin_conf_sum off by {e_bins}, bound {n_lab * tol[0]}"
    assert e_nll <= n_lab * tol[1], f"{what}: nll_sum off by {e_nll}, bound {n_lab * tol[1]}"
    assert e_brier <= n_lab * tol[2], f"{what}: brier_sum off by {e_brier}, bound {n_lab * tol[2]}"


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_kernel_against_the_oracle(dev, K, grid_cap, world, c):
    w = world[c.name]
    L, y = device_inputs(c, w, dev)
    rows = torch.full((c.B, 4), SENT, dtype=torch.int32, device=dev)
    if c.cap:
        grid_cap(c.cap)
    acc = run_kernel(K, c, L, y, rows=rows)
    torch.cuda.synchronize()
    r = rows.cpu().numpy()
    assert (r[c.nb:] == SENT).all(), "rows at and past nb were written"
    check(unpack(K, c.NC, c.NB, *acc), r[:c.nb], w["acc"], w["rows"], w["oracle"], w["tol"], c.NC, c.NB, c.name)


def test_two_passes_give_the_same_bits(dev, K, world):
    c = CASES[9]
    L, y = device_inputs(c, world[c.name], dev)
    out = []
    for _ in range(2):
        rows = torch.full((c.B, 4), SENT, dtype=torch.int32, device=dev)
        acc = run_kernel(K, c, L, y, rows=rows)
        out.append((acc[0].clone(), acc[1].clone(), rows))
    torch.cuda.synchronize()
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # and without the per-row record, and with no labels: the unlabelled row of the confusion matrix
    acc = run_kernel(K, c, L, None)
    got = unpack(K, c.NC, c.NB, *acc)
    assert got["n_labelled"] == 0 and got["confusion"][:c.NC].sum() == 0 and got["nll_sum"] == 0.0
    assert got["confusion"][c.NC].sum() + got["n_bad"] == got["n_rows"] == c.nb


def test_calls_accumulate(dev, K, world):
    """257 rows, then 65 more into the same accumulators: the oracle of the concatenation."""
    c = Case("257_then_65", 322, 330, 16, 10, True, 2.5, 3, 15, 0, 20)
    L, y = make_case(c)
    w = dict(L=L, y=y)
    Ld, yd = device_inputs(c, w, dev)
    rows = torch.full((c.B, 4), SENT, dtype=torch.int32, device=dev)
    acc = run_kernel(K, c, Ld, yd, nb=257, rows=rows)
    run_kernel(K, c, Ld[257:], yd[257:], nb=65, acc=acc, rows=rows[257:])
    run_kernel(K, c, Ld, yd, nb=0, acc=acc, rows=rows)             # nothing
    torch.cuda.synchronize()
    want, wrows = E.reference(L[:322], y[:322], 10, 2.5, 15, rows=True)
    o = oracle_rows(L[:322], y[:322], 10, 2.5)
    r = rows.cpu().numpy()
    assert (r[322:] == SENT).all()
    check(unpack(K, 10, 15, *acc), r[:322], want, wrows, o, world[CASES[4].name]["tol"], 10, 15, c.name)


def test_every_refusal_is_a_value_error_and_launches_nothing(dev, K):
    NC, NB = 10, 15
    lay = K.eval_metrics_layout(NC, NB)
    L = torch.randn(8, 16, device=dev)
    y = torch.zeros(8, dtype=torch.int32, device=dev)
    ai = torch.zeros(lay["size_i"], dtype=torch.int64, device=dev)
    af = torch.zeros(lay["size_f"], dtype=torch.float64, device=dev)
    sc = torch.zeros(K.eval_metrics_scratch_size(NB), dtype=torch.float64, device=dev)
    rows = torch.full((8, 4), SENT, dtype=torch.int32, device=dev)
    ok = dict(logits=L, labels=y, nb=8, n_classes=NC, acc_i=ai, acc_f=af, scratch=sc, rows=rows, temperature=1.0,
              n_bins=NB)
    bad = [dict(logits=L.half()), dict(logits=L.cpu()), dict(logits=L[:, :12]), dict(logits=L.view(-1)),
           dict(labels=y.long()), dict(labels=y[:7]), dict(labels=y.cpu()),
           dict(nb=9), dict(nb=-1), dict(n_classes=1), dict(n_classes=65), dict(n_classes=17),
           dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
           dict(temperature=1e-60), dict(n_bins=0), dict(n_bins=65),
           dict(acc_i=ai[:-1]), dict(acc_i=ai.int()), dict(acc_f=af[:-1]), dict(acc_f=af.float()), dict(acc_i=ai.cpu()),
           dict(scratch=sc[:-1]), dict(scratch=sc.float()), dict(n_bins=16),          # scratch and acc_f too small for 16
           dict(rows=rows[:7]), dict(rows=rows.long()), dict(rows=rows.view(-1)[1:]), dict(rows=rows.cpu())]
    for kw in bad:
        with pytest.raises(ValueError):
            K.eval_metrics(**{**ok, **kw})
    with pytest.raises(ValueError):
        K.eval_metrics_layout(1, 15)
    with pytest.raises(ValueError):
        K.eval_metrics_scratch_size(0)
    torch.cuda.synchronize()
    assert not ai.any() and not af.any() and (rows == SENT).all() and not sc.any()
    K.eval_metrics(**ok)
    from distributed_tensorflow_ibm_mnist_amd.ops import functional as Fk
    a2, _ = Fk.eval_metrics(L, y, NC)
    torch.cuda.synchronize()
    assert int(ai[lay["counts"]]) == 8 and torch.equal(a2, ai) and (rows[:, 0] >= 0).all()


# ---------------------------------------------------------------------------- end to end
@pytest.fixture(autouse=True)
def no_dead_graphs():
    """A Replica with a captured step is a reference cycle (its StepGraph holds its bound step), so
    the replicas of finished tests wait for the cycle collector, and a CUDAGraph that is destroyed
    while another step is being captured aborts the process (its destructor synchronises).  They
    are collected here, between tests, where nothing is capturing."""
    gc.collect()
    yield
    gc.collect()


def _replica(dev, model, precision="bf16", n_eval=300):
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica
    spec = get_model(model, 1)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.integers(0, 256, (1024, 784), dtype=np.uint8))
    y = torch.arange(1024) % 10
    return Replica(spec, "hip", 128, dev, torch_ref.init_params(spec, seed=0),
                   OptConfig(lr0=0.01, decay_steps=0, use_momentum=True, momentum=0.9), x, y, 1, x[:n_eval], y[:n_eval],
                   seed=5, precision=precision, log=lambda *_: None)


@pytest.mark.parametrize("model,precision,head", [("lenet5", "bf16", "mlp"), ("reference_cnn", "bf16", "tail"),
                                                  ("lenet5", "fp32", None)])
def test_evaluate_with_metrics(dev, K, model, precision, head):
    rep = _replica(dev, model, precision)
    if precision == "bf16":
        assert rep.net.head_kind == head
    for _ in range(3):
        rep.step()
    plain = rep.evaluate()
    assert plain == rep.evaluate(metrics=False) and set(plain) == {"loss", "accuracy"}
    rep.evaluate(metrics=True)                       # makes the accumulator
    seen = []
    add = rep._eval_acc.add

    def spy(logits, labels, nb, rows=None, temperature=None):
        rows = torch.full((logits.shape[0], 4), SENT, dtype=torch.int32, device=logits.device)
        add(logits, labels, nb, rows=rows)
        seen.append((logits[:nb].clone(), labels[:nb].clone(), rows[:nb].clone()))

    rep._eval_acc.add = spy
    got = rep.evaluate(metrics=True)
    torch.cuda.synchronize()
    assert [s[0].shape[0] for s in seen] == [128, 128, 44]
    assert got["loss"] == pytest.approx(plain["loss"], rel=1e-5) and np.isfinite(got["loss"])
    assert rep._eval_acc.copies == 2                 # one copy to the host per pass
    acc = rep._eval_acc.result()
    assert got["metrics"] == E.derive(acc)
    L = torch.cat([s[0] for s in seen]).float().cpu().numpy()
    y = torch.cat([s[1] for s in seen]).cpu().numpy()
    rows = torch.cat([s[2] for s in seen]).cpu().numpy()
    want, wrows = E.reference(L, y, 10, rows=True)
    o = oracle_rows(L, y, 10, 1.0)
    t = f32_transcription(L, y, 10, 1.0, 15)
    tol = [4.0 * _worst(t[k], o[k]) for k in range(3)]
    check(acc, rows, want, wrows, o, tol, 10, 15, f"{model} {precision}")
    m, ref = got["metrics"], E.derive(want)
    for k in ("top1", "top2", "top3", "top5", "confusion", "precision", "recall", "f1", "support", "macro_f1", "n_rows",
              "n_labelled", "n_bad"):
        assert m[k] == ref[k], k
    assert m["n_rows"] == m["n_labelled"] == 300 and m["n_bad"] == 0
    assert abs(m["nll"] - ref["nll"]) <= tol[1] and abs(m["brier"] - ref["brier"]) <= tol[2]
    if np.array_equal(rows[:, 2], wrows[:, 2]):
        assert abs(m["ece"] - ref["ece"]) <= tol[0] and abs(m["mce"] - ref["mce"]) <= tol[0]


def test_a_step_after_evaluate_with_metrics_is_the_step_without(dev, K):
    a, b = _replica(dev, "lenet5"), _replica(dev, "lenet5")
    for _ in range(2):
        a.step()
        b.step()
    a.evaluate(metrics=True)
    a.step()
    b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.net.fp.params, b.net.fp.params) and torch.equal(a.net.fp.mom, b.net.fp.mom)
    assert torch.equal(a.net.stats, b.net.stats) and int(a.net.fp.step.item()) == 3


def _run(args, script="main.py", timeout=240):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout, env=dict(os.environ, PYTHONUNBUFFERED="1"))
    return r.returncode, r.stdout + r.stderr


@pytest.mark.timeout(400)
def test_main_and_inference_with_the_switch(dev, tmp_path):
    d = str(tmp_path / "t")
    rc, out = _run(["--model=lenet5", "--in_channels=1", "--batch_size=64", "--max_steps=4", "--test_interval=2",
                    "--log_step_count_steps=0", "--train_data=synthetic://1000", "--test_data=synthetic://300?seed=1",
                    "--eval_examples=300", f"--train_dir={d}", "--eval_metrics=1"])
    assert rc == 0, out[-3000:]
    assert "  ECE " in out and "  macro-F1 " in out
    tags = []
    for f in events.find_event_files(os.path.join(d, "log")):
        for ev in events.read_events(f):
            if "test loss" in ev["values"]:
                tags.append(list(ev["values"]))
    assert tags and tags[0][:2] == ["test loss", "test accuracy"]
    assert tags[0][2:9] == ["test top2 accuracy", "test top3 accuracy", "test nll", "test brier", "test ece", "test mce",
                            "test macro_f1"]
    assert tags[0][9:] == [f"test recall/{c}" for c in range(10)] + [f"test precision/{c}" for c in range(10)]
    recs = [json.loads(l) for l in open(os.path.join(d, "log", "eval_metrics.jsonl"))]
    assert len(recs) == len(tags) and recs[0]["n_rows"] == 300 and {"step", "ece", "confusion", "reliability"} <= set(recs[0])

    res = {}
    for name, extra in (("plain", []), ("metrics", ["--eval_metrics=1", "--fit_temperature"])):
        rc, out = _run([f"--model={d}", "--validate", "--val_data=synthetic://300?seed=2",
                        f"--output_dir={tmp_path / 'inf'}", f"--output_file={name}.json", "--impl=hip"] + extra,
                       script="inference.py")
        assert rc == 0 and "Predictions are Finished" in out, out[-3000:]
        assert ("fitted temperature: " in out) == bool(extra)
        res[name] = json.load(open(tmp_path / "inf" / f"{name}.json"))
    s0, s1 = res["plain"]["summary"], res["metrics"]["summary"]
    assert set(s0) == {"count", "accuracy"} and set(s1) == {"count", "accuracy", "metrics", "temperature", "metrics_T1"}
    assert s1["accuracy"] == s0["accuracy"] and res["plain"]["results"] == res["metrics"]["results"]
    assert 0.05 <= s1["temperature"] <= 20.0 and s1["metrics"]["nll"] <= s1["metrics_T1"]["nll"]
    assert s1["metrics"]["n_labelled"] == 300 and s1["metrics"]["confusion"] == s1["metrics_T1"]["confusion"]
