"""Elastic distortion on the device (``csrc/kernels/augment_elastic.hip``): the draws bit for bit against
the host reference, the displacement field and the distorted images within the error budget of
``tests/elastic_oracle.py`` (4 * E32 of the case, plus half a bf16 ulp of the reference for bf16 output;
tests/test_elastic_cpu.py computes E32 and shows that a transcription error is orders of magnitude
larger), alpha = 0 bitwise the call without the keywords, every refusal of the bindings, and the Replica
/ executor paths."""
import numpy as np
import pytest
import torch

import augment_oracle as O
import elastic_oracle as E
from distributed_tensorflow_ibm_mnist_amd.data import augment as A

pytestmark = pytest.mark.gpu

SENTINEL, LAB_SENTINEL = 7.0, -77
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


def _table(case):
    return torch.from_numpy(A.elastic_weights(case[2]).copy())


def _device_inputs(dev, Csrc, nb):
    src = torch.from_numpy(O.dataset(Csrc).copy()).to(dev)
    idx = torch.from_numpy(O.indices(nb).copy()).to(dev)
    lab = torch.from_numpy(O.labels().copy()).to(dev)
    return src, idx, lab


def _buffers(dev, rows, Cdst, dt):
    return (torch.full((rows, 784, Cdst), SENTINEL, dtype=DT[dt], device=dev),
            torch.full((rows,), LAB_SENTINEL, dtype=torch.int32, device=dev))


def _run(K, dev, case, Csrc, Cdst, nb, dt, pos0=O.POS0, extra=2):
    src, idx, lab = _device_inputs(dev, Csrc, nb)
    out, lab_out = _buffers(dev, nb + extra, Cdst, dt)
    (S, R, Z), alpha, _ = case
    K.augment_images(src, idx, lab, out, lab_out, Csrc, Cdst, pos0, O.SEED, S, R, Z, elastic_alpha=alpha,
                     elastic_weights=_table(case))
    torch.cuda.synchronize()
    # rows >= nb are not written, every row < nb is
    assert torch.all(out[nb:] == SENTINEL) and torch.all(lab_out[nb:] == LAB_SENTINEL)
    assert np.array_equal(lab_out[:nb].cpu().numpy(), O.labels()[O.indices(nb)])
    return out[:nb]


def _check(got, ref, bf16, e32, what):
    err = np.abs(got.double().cpu().numpy() - ref)
    bound = E.bound(ref, bf16, e32)
    worst = float((err / bound).max())
    print(f"{what}: max |device - float64| = {err.max():.3e}, worst error / bound = {worst:.3f} (4 * E32 = {4 * e32:.3e})")
    assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} elements over the bound, worst ratio {worst:.3f}"


# ------------------------------------------------------------------ 1. the draws
@pytest.mark.parametrize("pos0", [0, (1 << 32) - 3, (1 << 40) + 5])
def test_draws_match_the_host_bit_for_bit(dev, K, grid_cap, pos0):
    n = 70
    want = A.elastic_draws(A.AugmentConfig(seed=O.SEED), pos0, n).reshape(n, 2, 784).astype(np.int32)
    for cap in (0, 2):
        out = torch.full((n + 2, 2, 784), -5, dtype=torch.int32, device=dev)
        grid_cap(cap)
        K.augment_elastic_draws(out[:n], pos0, O.SEED)
        grid_cap(0)
        assert np.array_equal(out[:n].cpu().numpy(), want) and torch.all(out[n:] == -5)


# ------------------------------------------------------------------ 2. the field
@pytest.mark.parametrize("case", E.ELASTIC)
def test_field_within_the_budget(dev, K, grid_cap, case):
    ref = E.field(case).reshape(E.NB, 2, 784)
    bound = E.bound_field(case)
    first = None
    for cap in (0, 2):
        out = torch.full((E.NB + 2, 2, 784), SENTINEL, dtype=torch.float32, device=dev)
        grid_cap(cap)
        K.augment_elastic_field(out[:E.NB], O.POS0, O.SEED, case[1], _table(case))
        grid_cap(0)
        torch.cuda.synchronize()
        assert torch.all(out[E.NB:] == SENTINEL)
        first = out if first is None else first
        assert torch.equal(out, first)
    err = np.abs(first[:E.NB].double().cpu().numpy() - ref)
    print(f"{case}: max |device field - float64| = {err.max():.3e} px, worst error / bound = {err.max() / bound:.3f} "
          f"(4 * E32_field = {bound:.3e})")
    assert err.max() <= bound
    # a shorter window of the stream is the same field
    part = torch.zeros((3, 2, 784), dtype=torch.float32, device=dev)
    K.augment_elastic_field(part, O.POS0 + 37, O.SEED, case[1], _table(case))
    assert torch.equal(part, first[37:40])


def test_a_table_with_a_zero_inside_is_not_cut_short(dev, K):
    """The smoothing chooses its band from the table's LENGTH: a hand-made table with w_13 = 0 and
    w_14 > 0 (valid for the binding) is applied whole, as the host applies it."""
    w = np.zeros(15, np.float32)
    w[:13] = A.elastic_weights(4.0) * np.float32(0.9)
    w[14] = np.float32(0.5 * (1.0 - (float(w[0]) + 2.0 * float(w[1:13].astype(np.float64).sum()))))
    r = (A.elastic_draws(A.AugmentConfig(seed=O.SEED), O.POS0, 6).astype(np.float32) - np.float32(32767.5)) * np.float32(2.0 ** -15)
    ref, f32 = A._smooth(r, w, np.float32(34.0), np.float64), A._smooth(r, w, np.float32(34.0), np.float32)
    bound = 4.0 * float(np.abs(f32.astype(np.float64) - ref).max())
    cut = A._smooth(r, w[:13], np.float32(34.0), np.float64)
    assert np.abs(cut - ref).max() > 100 * bound                # what a band chosen from w_13 == 0 would give
    out = torch.zeros((6, 2, 784), dtype=torch.float32, device=dev)
    K.augment_elastic_field(out, O.POS0, O.SEED, 34.0, torch.from_numpy(w))
    err = np.abs(out.double().cpu().numpy() - ref.reshape(6, 2, 784)).max()
    print(f"hand-made table: max |device field - float64| = {err:.3e} px, bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------ 3. the images
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("Csrc,Cdst", O.CHANNELS)
@pytest.mark.parametrize("case", E.ELASTIC)
def test_images_within_the_budget(dev, K, grid_cap, case, Csrc, Cdst, dt):
    for nb in O.NBS:                       # one image, a partial group, whole groups, several blocks + a tail
        got = _run(K, dev, case, Csrc, Cdst, nb, dt)
        ref = E.reference(case, Csrc, Cdst, nb)
        _check(got, ref, dt == "bf16", E.e32_out(case), f"{case} ({Csrc}, {Cdst}) {dt} nb = {nb}")
        if nb == E.NB:                     # the kernel is grid-strided: two blocks walk the eighteen groups
            grid_cap(2)
            again = _run(K, dev, case, Csrc, Cdst, nb, dt)
            grid_cap(0)
            assert torch.equal(again, got)


def test_a_field_belongs_to_the_position_not_the_batch(dev, K):
    """Entry b at pos0 is entry 0 at pos0 + b: the same row comes out identically."""
    case = E.ELASTIC[1]
    whole = _run(K, dev, case, 1, 1, 70, "bf16")
    src, idx, lab = _device_inputs(dev, 1, 70)
    out, lab_out = _buffers(dev, 4, 1, "bf16")
    K.augment_images(src, idx[37:40].contiguous(), lab, out, lab_out, 1, 1, O.POS0 + 37, O.SEED, *case[0],
                     elastic_alpha=case[1], elastic_weights=_table(case))
    assert torch.equal(out[:3], whole[37:40]) and torch.all(out[3] == SENTINEL)


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("Csrc,Cdst", O.CHANNELS)
def test_alpha_zero_is_bitwise_the_call_without_the_keywords(dev, K, Csrc, Cdst, dt):
    src, idx, lab = _device_inputs(dev, Csrc, 70)
    outs = []
    for kw in ({}, {"elastic_alpha": 0.0}, {"elastic_alpha": 0.0, "elastic_weights": _table(E.ELASTIC[0])},
               {"elastic_weights": _table(E.ELASTIC[3])}):
        out, lab_out = _buffers(dev, 72, Cdst, dt)
        K.augment_images(src, idx, lab, out, lab_out, Csrc, Cdst, O.POS0, O.SEED, *O.AFFINE[0], **kw)
        outs.append((out, lab_out))
    for out, lab_out in outs[1:]:
        assert torch.equal(out, outs[0][0]) and torch.equal(lab_out, outs[0][1])


# ------------------------------------------------------------------ 4. refusals
def test_every_refusal_of_the_bindings(dev, K):
    src, idx, lab = _device_inputs(dev, 1, 8)
    out, lab_out = _buffers(dev, 8, 1, "bf16")
    w = _table(E.ELASTIC[0])
    good = dict(src=src, idx=idx, lab_src=lab, out=out, lab_out=lab_out, Csrc=1, Cdst=1, pos0=0, seed=1, shift=1,
                rotate=1.0, scale=0.1, elastic_alpha=3.0, elastic_weights=w)
    fld = torch.zeros(4, 2, 784, device=dev)
    nan_w, neg_w, big_w = w.clone(), w.clone(), w * 1.0001
    nan_w[2] = float("nan")
    neg_w[-1] = -neg_w[-1]
    bad_tables = [w.to(dev), w.double(), w.view(1, -1), w[:2], torch.cat([w, w])[:26], torch.zeros(40)[::2][:13],
                  nan_w, neg_w, big_w, w * 0.5, torch.full((13,), float("inf"))]
    for key, name, bad in ([("elastic_alpha", "elastic_alpha", v) for v in (-0.5, 64.5, float("nan"), float("inf"))]
                           + [("elastic_weights", "elastic_weights", t) for t in bad_tables]
                           + [("elastic_weights", "elastic_weights", None)]):
        with pytest.raises(ValueError, match=name):
            K.augment_images(**{**good, key: bad})
        if bad is not None:
            with pytest.raises(ValueError, match=name):
                K.augment_elastic_field(fld, 0, 1, **{"elastic_alpha": 3.0, "elastic_weights": w, key: bad})
    # a bad table is refused whatever alpha is
    with pytest.raises(ValueError, match="elastic_weights"):
        K.augment_images(**{**good, "elastic_alpha": 0.0, "elastic_weights": w * 0.5})
    # everything augment_images refuses without the keywords, with them
    for key, name, bad in [("shift", "augment_shift", 9), ("rotate", "augment_rotate", float("nan")),
                           ("scale", "augment_scale", 0.51), ("seed", "augment_seed", -1), ("pos0", "pos0", -1),
                           ("pos0", "pos0", (1 << 63) - 4)]:
        with pytest.raises(ValueError, match=name):
            K.augment_images(**{**good, key: bad})
    for name, args in [("augment_seed", (0, -1)), ("pos0", (-1, 1)), ("pos0", ((1 << 63) - 2, 1))]:
        with pytest.raises(ValueError, match=name):
            K.augment_elastic_field(fld, *args, 3.0, w)
        with pytest.raises(ValueError, match=name):
            K.augment_elastic_draws(fld.int(), *args)
    src3 = torch.from_numpy(O.dataset(3).copy()).to(dev)
    for bad in [dict(src=src.cpu()), dict(src=src[:, :780]), dict(src=src3), dict(idx=idx.int()),
                dict(idx=torch.cat([idx, idx])), dict(lab_src=lab[:10]), dict(out=out.half()), dict(out=out.cpu()),
                dict(out=torch.zeros(8, 784, 3, dtype=torch.bfloat16, device=dev)), dict(lab_out=lab_out[:4]),
                dict(Csrc=3), dict(Cdst=2), dict(Csrc=3, Cdst=1, src=src3)]:
        with pytest.raises((RuntimeError, ValueError)):
            K.augment_images(**{**good, **bad})
    for dtype, call in ((torch.float32, lambda o: K.augment_elastic_field(o, 0, 1, 3.0, w)),
                        (torch.int32, lambda o: K.augment_elastic_draws(o, 0, 1))):
        for bad_out in (torch.zeros(4, 2, 783, dtype=dtype, device=dev), torch.zeros(4, 784, 2, dtype=dtype, device=dev),
                        torch.zeros(4, 2, 784, dtype=dtype), torch.zeros(4, 2, 784, dtype=torch.int64, device=dev),
                        torch.zeros(4, 2, 784, dtype=torch.half, device=dev),
                        torch.zeros(4, 2, 1568, dtype=dtype, device=dev)[:, :, :784]):
            with pytest.raises((RuntimeError, ValueError)):
                call(bad_out)
    torch.cuda.synchronize()
    assert torch.all(lab_out == LAB_SENTINEL) and torch.all(out == SENTINEL) and torch.all(fld == 0)   # nothing wrote
    K.augment_images(**good)
    K.augment_elastic_field(fld, 0, 1, 3.0, w)
    torch.cuda.synchronize()
    assert torch.all(lab_out != LAB_SENTINEL) and not torch.any(out == SENTINEL) and torch.any(fld != 0)


# ------------------------------------------------------------------ 5. Replica and executors
def _replica(dev, model, C, aug, graph=False, mode="prep", precision="bf16", rule="sgd", lines=None):
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica
    spec = get_model(model, C)
    x = torch.from_numpy(O.replica_dataset(C).copy())
    y = torch.arange(O.REPLICA_N) % 10
    opt = (OptConfig(lr0=0.001, decay_steps=0, ema_max=0.9999, rule="adam") if rule == "adam"
           else OptConfig(lr0=0.01, decay_steps=0, use_momentum=True, momentum=0.9, ema_max=0.9999))
    kw = {} if aug == "absent" else {"augment": aug}
    return Replica(spec, "hip", O.REPLICA_B, dev, torch_ref.init_params(spec, seed=0), opt, x, y, C, x[:100], y[:100],
                   seed=O.REPLICA_SEED, use_graph=graph, fused_input=mode, precision=precision,
                   log=(lines.append if lines is not None else print), **kw)


CFG = E.config(E.REPLICA_CASE, E.REPLICA_SEED)


@pytest.mark.parametrize("model,C", [("lenet5", 1), ("reference_cnn", 3)])
def test_replica_steps_see_the_oracle_batches(dev, K, model, C):
    rep = _replica(dev, model, C, CFG)
    before = rep.net.fp.params.clone()
    for step in range(O.REPLICA_STEPS):                 # positions continue across steps
        rep.step()
        torch.cuda.synchronize()
        got = rep.net.x0.reshape(O.REPLICA_B, 784, C)
        _check(got, E.replica_reference(C, step), True, E.e32_replica(), f"{model} step {step}")
        assert np.array_equal(rep.net.labels.cpu().numpy(), (O.replica_rows(step) % 10).astype(np.int32))
    assert int(rep.net.fp.step.item()) == O.REPLICA_STEPS and not torch.equal(before, rep.net.fp.params)
    assert rep.net.read_stats()["nan"] == 0.0


def test_graph_replay_is_bitwise_the_eager_run(dev, K):
    eager, graph = (_replica(dev, "lenet5", 1, CFG, graph=g, rule="adam") for g in (False, True))
    for _ in range(O.REPLICA_STEPS):
        eager.step()
        graph.step()
    torch.cuda.synchronize()
    assert graph._graph is not None and eager._graph is None
    assert torch.equal(eager.net.x0, graph.net.x0) and torch.equal(eager.net.fp.params, graph.net.fp.params)
    assert torch.equal(eager.net.fp.mom, graph.net.fp.mom)


def test_f32_executor_runs_an_elastic_step(dev, K):
    rep = _replica(dev, "lenet5", 1, CFG, precision="fp32")
    assert rep.net.x0.dtype == torch.float32
    rep.step()
    torch.cuda.synchronize()
    _check(rep.net.x0.reshape(O.REPLICA_B, 784, 1), E.replica_reference(1, 0), False, E.e32_replica(), "HipNetF32 step 0")
    assert int(rep.net.fp.step.item()) == 1 and rep.net.read_stats()["nan"] == 0.0


def test_eval_paths_stay_plain(dev, K):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import eval_batches
    aug, plain = _replica(dev, "lenet5", 1, CFG), _replica(dev, "lenet5", 1, None)
    aug.loader.next()                                    # a distorted batch sits in x0 before the eval
    plain.loader.next()
    assert not torch.equal(aug.net.x0, plain.net.x0) and torch.equal(aug.net.labels, plain.net.labels)
    assert aug.evaluate() == plain.evaluate()            # 100 rows at B = 64: a partial last batch
    assert torch.equal(aug.net.eval_stats, plain.net.eval_stats) and torch.equal(aug.net.x0, plain.net.x0)
    stats = []
    for rep in (aug, plain):
        st = torch.zeros_like(rep.net.eval_stats)
        for nb in eval_batches(rep.eval_ds, rep.net.x0, rep.net.labels):
            rep.net.eval_batch(nb, st)
        stats.append(st)
    assert torch.equal(stats[0], stats[1])
    n = len(aug.train_ds)                                # the whole-split bf16 copy is the plain normalisation too
    want, lab_out = _buffers(dev, n, 1, "bf16")
    K.prep_images(aug.train_ds.images, torch.arange(n, device=dev), aug.train_ds.labels, want, lab_out, 784, 1, 1)
    assert torch.equal(aug.train_ds.bf16_images(), want.view(n, 784))


def test_input_mode_interaction(dev, K):
    lines = []
    only = E.config(E.REPLICA_ONLY_ELASTIC, E.REPLICA_SEED)
    rep = _replica(dev, "lenet5", 1, only, mode="bf16", lines=lines)
    assert len(lines) == 1 and "prep" in lines[0] and "bf16" in lines[0]
    assert rep.net.idx_buf is None and rep.loader.idx_out is None and rep.loader.augment is not None
    assert rep.loader.lookahead_job() is None
    rep.step()
    torch.cuda.synchronize()
    _check(rep.net.x0.reshape(O.REPLICA_B, 784, 1), E.replica_reference(1, 0, E.REPLICA_ONLY_ELASTIC), True,
           E.e32_replica(E.REPLICA_ONLY_ELASTIC), "elastic alone, input_mode bf16 -> prep")
    # alpha 0 and no affine amount: bitwise a Replica without the argument, in the fused-gather mode it asked for
    lines = []
    zero = _replica(dev, "lenet5", 1, A.AugmentConfig(seed=21, elastic_alpha=0.0, elastic_sigma=2.0), mode="bf16", lines=lines)
    absent = _replica(dev, "lenet5", 1, "absent", mode="bf16", lines=lines)
    assert not lines and zero.net.idx_buf is not None and absent.net.idx_buf is not None and zero.loader.augment is None
    for _ in range(O.REPLICA_STEPS):
        zero.step()
        absent.step()
    torch.cuda.synchronize()
    assert torch.equal(zero.net.fp.params, absent.net.fp.params) and torch.equal(zero.net.idx_buf, absent.net.idx_buf)
    assert torch.equal(zero.net.labels, absent.net.labels)
