"""Evaluation metrics, the parts that need no GPU: the vectorised float64 ``reference`` against a
plain Python double loop, its invariants, ``derive`` on a hand-worked example, accumulation,
the temperature search, and the CPU executor / Monitor wiring."""
import json
import math
import os

import numpy as np
import pytest
import torch

from distributed_tensorflow_ibm_mnist_amd.obs import eval_metrics as E
from distributed_tensorflow_ibm_mnist_amd.obs import events

INT_KEYS = ("confusion", "rank_hist", "bin_count", "bin_correct")


def loop_reference(L, y, NC, T, NB):
    """Section by section the definition, one row and one class at a time, in Python floats."""
    acc = {"confusion": [[0] * NC for _ in range(NC + 1)], "rank_hist": [0] * NC, "bin_count": [0] * NB,
           "bin_correct": [0] * NB, "n_rows": 0, "n_labelled": 0, "n_bad": 0, "bin_conf_sum": [0.0] * NB,
           "nll_sum": 0.0, "brier_sum": 0.0}
    rows = []
    for i in range(len(L)):
        l = [float(L[i][c]) for c in range(NC)]
        acc["n_rows"] += 1
        if any(not math.isfinite(v) for v in l):
            acc["n_bad"] += 1
            rows.append((-1, -1, -1, None))
            continue
        mx, pred = l[0], 0
        for c in range(1, NC):
            if l[c] > mx:
                mx, pred = l[c], c
        d = [(l[c] - mx) * (1.0 / T) for c in range(NC)]
        se = 0.0
        for c in range(NC):
            se += math.exp(d[c])
        conf = 1.0 / se
        yi = -1 if y is None else int(y[i])
        if not 0 <= yi < NC:
            acc["confusion"][NC][pred] += 1
            rows.append((pred, -1, -1, conf))
            continue
        rank = sum(1 for c in range(NC) if l[c] > l[yi]) + sum(1 for c in range(yi) if l[c] == l[yi])
        nll = math.log(se) - d[yi]
        brier = 0.0
        for c in range(NC):
            brier += (math.exp(d[c]) / se - (1.0 if c == yi else 0.0)) ** 2
        b = min(NB - 1, int(conf * NB))
        acc["confusion"][yi][pred] += 1
        acc["rank_hist"][rank] += 1
        acc["bin_count"][b] += 1
        acc["bin_correct"][b] += int(rank == 0)
        acc["bin_conf_sum"][b] += conf
        acc["n_labelled"] += 1
        acc["nll_sum"] += nll
        acc["brier_sum"] += brier
        rows.append((pred, rank, b, conf))
    return acc, rows


def tiny_inputs(NC, seed):
    """bf16-exact logits with planted ties (at the maximum, and with the true class), a -1 label,
    a label >= NC, a row with inf and a row with NaN."""
    rng = np.random.default_rng(seed)
    L = torch.from_numpy(rng.standard_normal((24, NC + 3)).astype(np.float32) * 2).bfloat16().float().numpy()
    y = rng.integers(0, NC, 24).astype(np.int64)
    L[0, 0] = L[0, NC - 1] = 50.0                # a tie at the maximum: pred is the lower index
    y[0] = NC - 1                                # ... and the true class is the higher one: rank 1
    L[1, 0] = L[1, 1]                            # a tie with the true class below the maximum
    y[1] = 1
    L[2, :NC] = 0.25                             # all equal
    y[2] = NC - 1
    y[3] = -1
    y[4] = NC
    L[5, 1] = np.inf
    L[6, 0] = np.nan
    L[7, NC] = np.nan                            # a padding column: not part of the row
    L[8, NC + 1] = 1e30
    return L, y


@pytest.mark.parametrize("NC", [2, 10])
@pytest.mark.parametrize("T", [1.0, 2.5])
@pytest.mark.parametrize("NB", [1, 15])
def test_reference_is_the_double_loop(NC, T, NB):
    L, y = tiny_inputs(NC, NC)
    acc, rows = E.reference(L, y, NC, temperature=T, n_bins=NB, rows=True)
    want, wrows = loop_reference(L, y, NC, T, NB)
    for k in INT_KEYS:
        assert np.array_equal(np.asarray(acc[k]), np.asarray(want[k])), k
    for k in ("n_rows", "n_labelled", "n_bad"):
        assert acc[k] == want[k], k
    assert want["n_bad"] == 2 and want["n_rows"] == 24 and want["n_labelled"] == 20
    assert np.allclose(acc["bin_conf_sum"], want["bin_conf_sum"], rtol=1e-13, atol=0)
    assert acc["nll_sum"] == pytest.approx(want["nll_sum"], rel=1e-13)
    assert acc["brier_sum"] == pytest.approx(want["brier_sum"], rel=1e-13)
    for i, (p, r, b, c) in enumerate(wrows):
        assert tuple(rows[i, :3]) == (p, r, b), i
        bits = int(rows[i, 3:4].view(np.uint32)[0])
        if c is None:
            assert bits == 0x7FC00000
        else:
            assert bits == int(np.float32(c).view(np.uint32))
    # the planted rows
    assert tuple(rows[0, :2]) == (0, 1) and rows[1, 1] >= 1 and tuple(rows[2, :2]) == (0, NC - 1)
    # invariants
    cm = np.asarray(acc["confusion"])
    assert acc["rank_hist"][0] == np.trace(cm[:NC])
    assert cm.sum() + acc["n_bad"] == acc["n_rows"]
    assert acc["bin_count"].sum() == acc["n_labelled"]
    assert cm[NC].sum() == 2


def test_no_labels_is_image_mode():
    L, _ = tiny_inputs(10, 1)
    acc, rows = E.reference(L, None, 10, rows=True)
    assert acc["n_labelled"] == 0 and acc["confusion"][:10].sum() == 0 and acc["confusion"][10].sum() == 22
    assert (rows[:, 1] == -1).all() and acc["nll_sum"] == 0.0


def test_derive_hand_worked():
    """Three classes, six labelled rows; class 2 is never predicted.
        truth 0: predicted 0, 0, 1     truth 1: predicted 1     truth 2: predicted 0, 1
    """
    acc = E.new_acc(3, 2)
    acc["confusion"][:3] = [[2, 1, 0], [0, 1, 0], [1, 1, 0]]
    acc["confusion"][3] = [4, 0, 0]
    acc["rank_hist"][:] = [3, 2, 1]
    acc["bin_count"][:] = [2, 4]
    acc["bin_correct"][:] = [0, 3]
    acc["bin_conf_sum"][:] = [0.8, 3.6]
    acc["n_rows"], acc["n_labelled"], acc["n_bad"] = 11, 6, 1
    acc["nll_sum"], acc["brier_sum"] = 3.0, 1.5
    d = E.derive(acc)
    assert d["top1"] == 0.5 and d["top2"] == pytest.approx(5 / 6) and d["top3"] == 1.0 and "top5" not in d
    assert d["nll"] == 0.5 and d["brier"] == 0.25
    # bins: (2, acc 0, conf 0.4) and (4, acc 0.75, conf 0.9)
    assert d["reliability"] == [[2, 0.0, 0.4], [4, 0.75, pytest.approx(0.9)]]
    assert d["ece"] == pytest.approx(2 / 6 * 0.4 + 4 / 6 * 0.15) and d["mce"] == pytest.approx(0.4)
    assert d["precision"] == [pytest.approx(2 / 3), pytest.approx(1 / 3), 0.0]
    assert d["recall"] == [pytest.approx(2 / 3), 1.0, 0.0] and d["support"] == [3, 1, 2]
    assert d["f1"] == [pytest.approx(2 / 3), pytest.approx(0.5), 0.0]
    assert d["macro_f1"] == pytest.approx((2 / 3 + 0.5) / 3)
    assert d["confusion"][3] == [4, 0, 0] and (d["n_rows"], d["n_labelled"], d["n_bad"]) == (11, 6, 1)
    json.dumps(d)
    # nothing labelled: every ratio is 0.0, nothing divides by zero
    z = E.derive(E.new_acc(3, 2))
    assert z["top1"] == 0.0 and z["ece"] == 0.0 and z["macro_f1"] == 0.0 and z["nll"] == 0.0


def test_two_calls_are_one_call_on_the_concatenation():
    rng = np.random.default_rng(7)
    L = rng.standard_normal((322, 10)) * 3
    y = rng.integers(-1, 10, 322)
    L[5, 3] = np.nan
    one = E.reference(L, y, 10, 2.5)
    two = E.reference(L[:257], y[:257], 10, 2.5)
    assert E.reference(L[257:], y[257:], 10, 2.5, acc=two) is two
    for k in INT_KEYS:
        assert np.array_equal(one[k], two[k]), k
    for k in ("n_rows", "n_labelled", "n_bad"):
        assert one[k] == two[k]
    assert np.allclose(one["bin_conf_sum"], two["bin_conf_sum"], rtol=1e-12, atol=0)
    assert two["nll_sum"] == pytest.approx(one["nll_sum"], rel=1e-12)
    assert two["brier_sum"] == pytest.approx(one["brier_sum"], rel=1e-12)
    # the accumulator class, on CPU tensors: the same numbers
    acc = E.EvalAccumulator("cpu", 10, temperature=2.5)
    acc.zero()
    acc.add(torch.from_numpy(L[:257]), torch.from_numpy(y[:257]))
    acc.add(torch.from_numpy(L), torch.from_numpy(y[257:]), 0)          # nb = 0 adds nothing
    acc.add(torch.from_numpy(L[257:]), torch.from_numpy(y[257:]), 65)
    got = acc.result()
    for k in INT_KEYS:
        assert np.array_equal(got[k], two[k]), k
    assert got["nll_sum"] == two["nll_sum"] and got["n_rows"] == 322
    acc.zero()
    assert acc.result()["n_rows"] == 0


def test_arguments_are_checked():
    L = np.zeros((4, 10))
    for kw in (dict(n_classes=1), dict(n_classes=65), dict(n_classes=11), dict(n_classes=10, temperature=0.0),
               dict(n_classes=10, temperature=float("nan")), dict(n_classes=10, n_bins=0),
               dict(n_classes=10, n_bins=65)):
        with pytest.raises(ValueError):
            E.reference(L, None, **kw)
    with pytest.raises(ValueError):
        E.reference(L, np.zeros(3, np.int64), 10)
    with pytest.raises(ValueError):
        E.EvalAccumulator("cpu", 10).add(torch.zeros(4, 10), None, 5)


def test_fit_temperature_finds_the_minimum_of_the_nll():
    """Logits that are 3 x a hidden set, labels drawn from the hidden softmax: a property of the
    search (no neighbour of the fitted T has a lower NLL), not a statistical claim about T."""
    rng = np.random.default_rng(11)
    h = rng.standard_normal((3000, 10))
    p = np.exp(h)
    p /= p.sum(1, keepdims=True)
    y = (p.cumsum(1) < rng.random((3000, 1))).sum(1).clip(0, 9)
    L = 3.0 * h
    T = E.fit_temperature(L, y, 10)
    assert 0.05 <= T <= 20.0
    nll = lambda t: E.reference(L, y, 10, temperature=t)["nll_sum"]  # noqa: E731
    at = nll(T)
    for f in (0.9, 0.95, 1.05, 1.1):
        assert at <= nll(T * f), f
    assert at < nll(1.0)


def _cpu_replica(n_eval=150, batch=64):
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica
    spec = get_model("mlp", 1)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.integers(0, 256, (256, 784), dtype=np.uint8))
    y = torch.arange(256) % 10
    return Replica(spec, "torch", batch, "cpu", torch_ref.init_params(spec, seed=0), OptConfig(lr0=0.01), x, y, 1,
                   x[:n_eval], y[:n_eval], seed=5, use_graph=False, log=lambda *_: None)


def test_torchnet_evaluate_with_metrics_is_the_reference_over_its_logits():
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import eval_batches
    rep = _cpu_replica()
    for _ in range(3):
        rep.step()
    plain = rep.evaluate()
    assert plain == rep.evaluate(metrics=False) and set(plain) == {"loss", "accuracy"}
    got = rep.evaluate(metrics=True)
    assert got["loss"] == plain["loss"] and got["accuracy"] == plain["accuracy"]
    acc = E.new_acc(10)
    sizes = []
    for nb in eval_batches(rep.eval_ds, rep.net.x0, rep.net.labels):
        with torch.no_grad():
            logits = rep.net.forward(nb, grad=False)
        E.reference(logits, rep.net.labels[:nb], 10, acc=acc)
        sizes.append(nb)
    assert sizes == [64, 64, 22]
    assert got["metrics"] == E.derive(acc)
    m = got["metrics"]
    assert m["n_rows"] == m["n_labelled"] == 150 and m["n_bad"] == 0 and m["top1"] <= m["top2"] <= m["top5"]
    assert rep.evaluate(100, metrics=True)["metrics"]["n_rows"] == 128      # the cap rounds up to whole batches


def _test_events(logdir):
    out = []
    for f in events.find_event_files(logdir):
        for ev in events.read_events(f):
            if "test loss" in ev["values"]:
                out.append(ev)
    return out


def test_monitor_tags_with_and_without_the_switch(tmp_path):
    from distributed_tensorflow_ibm_mnist_amd.obs.monitor import Monitor
    rep = _cpu_replica()
    rep.step()
    lines = {}
    for on in (False, True):
        d = str(tmp_path / f"m{int(on)}")
        lines[on] = []
        kw = dict(eval_metrics=True) if on else {}
        m = Monitor(d, 1, 2, rep, eval_examples=0, log=lines[on].append, **kw)
        m.register_reference_summaries()
        m.write_test(1)
        m.write_test(2)
        m.close()
    off, on = _test_events(str(tmp_path / "m0")), _test_events(str(tmp_path / "m1"))
    assert len(off) == len(on) == 2
    assert list(off[0]["values"]) == ["test loss", "test accuracy"]
    assert not os.path.exists(tmp_path / "m0" / "eval_metrics.jsonl")
    assert lines[False][0].startswith("step 1: test loss ") and "ECE" not in lines[False][0]
    new = (["test top2 accuracy", "test top3 accuracy", "test nll", "test brier", "test ece", "test mce",
            "test macro_f1"] + [f"test recall/{c}" for c in range(10)] + [f"test precision/{c}" for c in range(10)])
    assert list(on[0]["values"]) == ["test loss", "test accuracy"] + new
    assert on[0]["values"]["test loss"] == off[0]["values"]["test loss"]
    assert on[0]["values"]["test accuracy"] == off[0]["values"]["test accuracy"]
    assert lines[True][0].startswith(lines[False][0]) and "  ECE " in lines[True][0] and "  macro-F1 " in lines[True][0]
    recs = [json.loads(l) for l in open(tmp_path / "m1" / "eval_metrics.jsonl")]
    assert [r["step"] for r in recs] == [1, 2]
    want = rep.evaluate(metrics=True)["metrics"]
    assert recs[1] == {"step": 2, **want}
    assert on[1]["values"]["test ece"] == pytest.approx(want["ece"], rel=1e-6)
    assert on[1]["values"]["test recall/3"] == pytest.approx(want["recall"][3], rel=1e-6)
