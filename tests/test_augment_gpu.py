"""Training augmentation on the device (``csrc/kernels/augment.hip``): the draw bit for bit against the
host reference, the pure shift bit for bit against ``prep_images`` on host-shifted copies, the full
affine map within the error budget of ``tests/augment_oracle.py`` (4 * E32, plus half a bf16 ulp of
the reference for bf16 output; tests/test_augment_cpu.py computes E32 and shows that a transcription
error is orders of magnitude larger), every refusal of the binding, and the Replica / executor paths:
positions continue across steps, a graph replay is the eager run, every eval path stays plain."""
import numpy as np
import pytest
import torch

import augment_oracle as O
from distributed_tensorflow_ibm_mnist_amd.data import augment as A

pytestmark = pytest.mark.gpu

SENTINEL, LAB_SENTINEL = 7.0, -77
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


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
    K.augment_images(src, idx, lab, out, lab_out, Csrc, Cdst, pos0, O.SEED, case[0], case[1], case[2])
    torch.cuda.synchronize()
    # rows >= nb are not written, every row < nb is
    assert torch.all(out[nb:] == SENTINEL) and torch.all(lab_out[nb:] == LAB_SENTINEL)
    assert np.array_equal(lab_out[:nb].cpu().numpy(), O.labels()[O.indices(nb)])      # as prep_images gathers them
    return out[:nb]


def _check(got, ref, bf16, what):
    err = np.abs(got.double().cpu().numpy() - ref)
    bound = O.bound(ref, bf16)
    worst = float((err / bound).max())
    print(f"{what}: max |device - float64| = {err.max():.3e}, worst error / bound = {worst:.3f} (4 * E32 = {4 * O.e32():.3e})")
    assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} elements over the bound, worst ratio {worst:.3f}"


# ------------------------------------------------------------------ 1. the draw
@pytest.mark.parametrize("case", [(0, 0.0, 0.0), (3, 0.0, 0.0), (2, 15.0, 0.15), (8, 180.0, 0.5)])
@pytest.mark.parametrize("pos0", [0, (1 << 32) - 3, (1 << 40) + 5])
def test_params_match_the_host_bit_for_bit(dev, K, case, pos0):
    out = torch.full((70, 4), SENTINEL, dtype=torch.float32, device=dev)
    K.augment_params(out, pos0, O.SEED, case[0], case[1], case[2])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), A.params(O.config(case), pos0, 70).view(np.uint32))


# ------------------------------------------------------------------ 2. the exact case
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("Csrc,Cdst", O.CHANNELS)
@pytest.mark.parametrize("S", [0, 1, 3, 8])
def test_pure_shift_is_bitwise_prep_images_of_the_shifted_rows(dev, K, S, Csrc, Cdst, dt):
    nb, case = 70, (S, 0.0, 0.0)
    got = _run(K, dev, case, Csrc, Cdst, nb, dt)
    prm = A.params(O.config(case), O.POS0, nb)
    assert S == 0 or (prm[:, :2].min() == -S and prm[:, :2].max() == S)
    moved = torch.from_numpy(O.shifted(O.dataset(Csrc)[O.indices(nb)], prm, Csrc)).to(dev)
    want, lab_out = _buffers(dev, nb, Cdst, dt)
    prep = K.f32_prep_images if dt == "fp32" else K.prep_images
    prep(moved, torch.arange(nb, device=dev), torch.zeros(nb, dtype=torch.int32, device=dev), want, lab_out, 784, Csrc, Cdst)
    assert torch.equal(got, want)


# ------------------------------------------------------------------ 3. the full affine map
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("Csrc,Cdst", O.CHANNELS)
@pytest.mark.parametrize("case", O.AFFINE)
def test_affine_within_the_budget(dev, K, grid_cap, case, Csrc, Cdst, dt):
    for nb in O.NBS:                       # one image, a partial group, whole groups, several blocks + a tail
        got = _run(K, dev, case, Csrc, Cdst, nb, dt)
        ref = O.reference(case, Csrc, Cdst, nb)
        _check(got, ref, dt == "bf16", f"{case} ({Csrc}, {Cdst}) {dt} nb = {nb}")
        if nb == max(O.NBS):               # the kernel is grid-strided: two blocks walk the nine groups
            grid_cap(2)
            again = _run(K, dev, case, Csrc, Cdst, nb, dt)
            grid_cap(0)
            assert torch.equal(again, got)


def test_a_draw_belongs_to_the_position_not_the_batch(dev, K):
    """Entry b at pos0 is entry 0 at pos0 + b: the same row comes out identically."""
    case = O.AFFINE[0]
    whole = _run(K, dev, case, 1, 1, 70, "bf16")
    src, idx, lab = _device_inputs(dev, 1, 70)
    out, lab_out = _buffers(dev, 4, 1, "bf16")
    K.augment_images(src, idx[37:40].contiguous(), lab, out, lab_out, 1, 1, O.POS0 + 37, O.SEED, *case)
    assert torch.equal(out[:3], whole[37:40]) and torch.all(out[3] == SENTINEL)


# ------------------------------------------------------------------ 4. refusals
def test_every_refusal_of_the_binding(dev, K):
    src, idx, lab = _device_inputs(dev, 1, 8)
    out, lab_out = _buffers(dev, 8, 1, "bf16")
    good = dict(src=src, idx=idx, lab_src=lab, out=out, lab_out=lab_out, Csrc=1, Cdst=1, pos0=0, seed=1, shift=1,
                rotate=1.0, scale=0.1)
    K.augment_images(**good)
    for key, name, bad in [("shift", "augment_shift", -1), ("shift", "augment_shift", 9),
                           ("rotate", "augment_rotate", -0.5), ("rotate", "augment_rotate", 180.5),
                           ("rotate", "augment_rotate", float("nan")), ("rotate", "augment_rotate", float("inf")),
                           ("scale", "augment_scale", -0.1), ("scale", "augment_scale", 0.51),
                           ("scale", "augment_scale", float("nan")), ("seed", "augment_seed", -1),
                           ("pos0", "pos0", -1), ("pos0", "pos0", (1 << 63) - 4)]:
        with pytest.raises(ValueError, match=name):
            K.augment_images(**{**good, key: bad})
        if key != "pos0" or bad < 0:
            with pytest.raises(ValueError, match=name):
                K.augment_params(torch.zeros(4, 4, device=dev), **{k: {**good, key: bad}[k] for k in
                                                                   ("pos0", "seed", "shift", "rotate", "scale")})
    src3 = torch.from_numpy(O.dataset(3).copy()).to(dev)
    for bad in [dict(src=src.cpu()), dict(src=src.to(torch.int8)), dict(src=src[:, :780]), dict(src=src.t().contiguous().t()),
                dict(src=src3), dict(src=src.view(-1)),                                     # src.size(1) != 784 * Csrc
                dict(idx=idx.int()), dict(idx=idx.cpu()), dict(idx=torch.cat([idx, idx])),  # more indices than rows
                dict(lab_src=lab[:10]), dict(lab_src=lab.long()),
                dict(out=out.half()), dict(out=out.cpu()), dict(out=torch.zeros(8, 784, 2, dtype=torch.bfloat16, device=dev)[:, :, :1]),   # not contiguous
                dict(out=torch.zeros(8, 784, 3, dtype=torch.bfloat16, device=dev)),         # [B, 784 * 3] for Cdst 1
                dict(lab_out=lab_out[:4]), dict(lab_out=lab_out.long()),
                dict(Csrc=3), dict(Cdst=2), dict(Csrc=3, Cdst=1, src=src3), dict(Csrc=2, Cdst=2)]:
        with pytest.raises((RuntimeError, ValueError)):
            K.augment_images(**{**good, **bad})
    for bad_out in (torch.zeros(4, 3, device=dev), torch.zeros(4, 4, device=dev).half(), torch.zeros(4, 4),
                    torch.zeros(16, device=dev), torch.zeros(4, 8, device=dev)[:, :4]):
        with pytest.raises((RuntimeError, ValueError)):
            K.augment_params(bad_out, 0, 1, 1, 1.0, 0.1)
    torch.cuda.synchronize()
    assert torch.all(lab_out != LAB_SENTINEL)          # only the good call wrote


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


@pytest.mark.parametrize("model,C", [("lenet5", 1), ("reference_cnn", 3)])
def test_replica_steps_see_the_oracle_batches(dev, K, model, C):
    rep = _replica(dev, model, C, O.config(O.REPLICA_CFG, 21))
    before = rep.net.fp.params.clone()
    for step in range(O.REPLICA_STEPS):                 # positions continue across steps
        rep.step()
        torch.cuda.synchronize()
        got = rep.net.x0.reshape(O.REPLICA_B, 784, C)
        _check(got, O.replica_reference(C, step, 21), True, f"{model} step {step}")
        assert np.array_equal(rep.net.labels.cpu().numpy(), (O.replica_rows(step) % 10).astype(np.int32))
    assert int(rep.net.fp.step.item()) == O.REPLICA_STEPS and not torch.equal(before, rep.net.fp.params)
    assert rep.net.read_stats()["nan"] == 0.0


def test_graph_replay_is_bitwise_the_eager_run(dev, K):
    cfg = O.config(O.REPLICA_CFG, 21)
    eager, graph = (_replica(dev, "lenet5", 1, cfg, graph=g, rule="adam") for g in (False, True))
    for _ in range(O.REPLICA_STEPS):
        eager.step()
        graph.step()
    torch.cuda.synchronize()
    assert graph._graph is not None and eager._graph is None
    assert torch.equal(eager.net.x0, graph.net.x0) and torch.equal(eager.net.fp.params, graph.net.fp.params)
    assert torch.equal(eager.net.fp.mom, graph.net.fp.mom)


def test_f32_executor_runs_an_augmented_step(dev, K):
    rep = _replica(dev, "lenet5", 1, O.config(O.REPLICA_CFG, 21), precision="fp32")
    assert rep.net.x0.dtype == torch.float32
    rep.step()
    torch.cuda.synchronize()
    _check(rep.net.x0.reshape(O.REPLICA_B, 784, 1), O.replica_reference(1, 0, 21), False, "HipNetF32 step 0")
    assert int(rep.net.fp.step.item()) == 1 and rep.net.read_stats()["nan"] == 0.0


def test_eval_paths_stay_plain(dev, K):
    from distributed_tensorflow_ibm_mnist_amd.data.device_loader import eval_batches
    aug, plain = _replica(dev, "lenet5", 1, O.config(O.REPLICA_CFG, 21)), _replica(dev, "lenet5", 1, None)
    aug.loader.next()                                    # an augmented batch sits in x0 before the eval
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
    # the whole-split bf16 copy is the plain normalisation too
    n = len(aug.train_ds)
    want, lab_out = _buffers(dev, n, 1, "bf16")
    K.prep_images(aug.train_ds.images, torch.arange(n, device=dev), aug.train_ds.labels, want, lab_out, 784, 1, 1)
    assert torch.equal(aug.train_ds.bf16_images(), want.view(n, 784))


def test_input_mode_interaction(dev, K):
    lines = []
    rep = _replica(dev, "lenet5", 1, O.config(O.REPLICA_CFG, 21), mode="bf16", lines=lines)
    assert len(lines) == 1 and "prep" in lines[0] and "bf16" in lines[0]
    assert rep.net.idx_buf is None and rep.loader.idx_out is None and rep.loader.augment is not None   # no bound dataset
    rep.step()
    torch.cuda.synchronize()
    _check(rep.net.x0.reshape(O.REPLICA_B, 784, 1), O.replica_reference(1, 0, 21), True, "input_mode bf16 -> prep")
    # all three amounts 0: bitwise a Replica without the argument, in the fused-gather mode it asked for
    lines = []
    zero = _replica(dev, "lenet5", 1, A.AugmentConfig(seed=21), mode="bf16", lines=lines)
    absent = _replica(dev, "lenet5", 1, "absent", mode="bf16", lines=lines)
    assert not lines and zero.net.idx_buf is not None and absent.net.idx_buf is not None and zero.loader.augment is None
    for _ in range(O.REPLICA_STEPS):
        zero.step()
        absent.step()
    torch.cuda.synchronize()
    assert torch.equal(zero.net.fp.params, absent.net.fp.params) and torch.equal(zero.net.idx_buf, absent.net.idx_buf)
    assert torch.equal(zero.net.labels, absent.net.labels)
