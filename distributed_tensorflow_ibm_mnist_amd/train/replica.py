"""One training replica: model executor + on-device input pipeline + DP wiring.

Bridges the session/hook layer (host-side, step-count driven) and the device
(`HipNet` on the HIP kernels, or `TorchNet` for CPU / the PyTorch baseline).
The host keeps a mirror of the global step so hooks never read device memory
on the hot path; device state (loss, accuracy, NaN flag) is read only when a
hook asks for it.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.distributed as dist

from ..data.device_loader import DeviceDataset, DeviceLoader, eval_batches
from ..models import torch_ref
from ..models.spec import ModelSpec
from ..parallel.dp import DataParallel
from ..runtime.params import FlatParams, OptConfig


def build_net(impl: str, spec: ModelSpec, batch: int, device, init, opt: OptConfig, precision: str = "bf16", x0=None):
    """``x0``: an input buffer the executor adopts instead of allocating one (runtime/teacher.py)."""
    kw = {} if x0 is None else {"x0": x0}
    if impl == "hip" and precision == "fp32":
        from ..runtime.executor_f32 import HipNetF32
        return HipNetF32(spec, batch, device, init, opt, **kw)
    if impl == "hip":
        assert precision == "bf16", f"unknown precision {precision!r}"
        from ..runtime.executor import HipNet
        return HipNet(spec, batch, device, init, opt, **kw)
    from ..runtime.torchnet import TorchNet
    return TorchNet(spec, batch, device, init, opt, **kw)


def state_tensors(net, include_momentum: bool = True) -> Dict[str, np.ndarray]:
    """Device state -> checkpoint dict with the reference's variable names."""
    fp: FlatParams = net.fp
    out: Dict[str, np.ndarray] = {}
    params = fp.params.detach().cpu().numpy()
    ema = fp.ema.detach().cpu().numpy()
    # slot variables under TF1's names: <var>/Momentum; <var>/Adam (m), <var>/Adam_1 (v);
    # <var>/RMSProp (ms), <var>/RMSProp_1 (mom); <var>/Adagrad
    n1, n2 = net.opt.slot_names() if include_momentum else (None, None)
    mom = fp.mom.detach().cpu().numpy() if n1 else None
    slot2 = fp.slot2.detach().cpu().numpy() if n2 else None
    for e in fp.entries:
        sl = slice(e.off, e.off + e.n)
        out[e.name] = params[sl].reshape(e.shape).copy()
        if net.opt.ema_max >= 0:
            out[f"{e.name}/ExponentialMovingAverage"] = ema[sl].reshape(e.shape).copy()
        if n1:
            out[f"{e.name}/{n1}"] = mom[sl].reshape(e.shape).copy()
        if n2:
            out[f"{e.name}/{n2}"] = slot2[sl].reshape(e.shape).copy()
    step = int(fp.step.item())
    if include_momentum and net.opt.rule in ("adam", "lamb"):
        # TF1's Adam keeps beta^t as variables; written as beta^(global_step + 1), ignored on
        # restore (the update derives them from the step)
        out["beta1_power"] = np.asarray(net.opt.beta1 ** (step + 1), dtype=np.float32)
        out["beta2_power"] = np.asarray(net.opt.beta2 ** (step + 1), dtype=np.float32)
    out["global_step"] = np.asarray(step, dtype=np.int64)
    le = net.loss_ema.detach().cpu().numpy().reshape(-1, 3)
    for i, name in enumerate(net.loss_names):
        out[f"{name}/avg"] = np.asarray(le[i, 2], dtype=np.float32)
        out[f"{name}/avg/biased"] = np.asarray(le[i, 0], dtype=np.float32)
        out[f"{name}/avg/local_step"] = np.asarray(le[i, 1], dtype=np.float32)
    return out


def load_state(net, tensors: Dict[str, np.ndarray], strict: bool = True) -> int:
    fp: FlatParams = net.fp
    missing = [e.name for e in fp.entries if e.name not in tensors]
    if missing and strict:
        raise KeyError(f"checkpoint lacks {missing}")
    vals = {n: torch.from_numpy(np.asarray(tensors[n])) for n in fp.names() if n in tensors}
    emas = {n: torch.from_numpy(np.asarray(tensors[f"{n}/ExponentialMovingAverage"])) for n in fp.names()
            if f"{n}/ExponentialMovingAverage" in tensors}
    # slots the checkpoint lacks keep their initial values, as TF would create them
    n1, n2 = net.opt.slot_names()
    n1 = n1 or "Momentum"
    moms = {n: torch.from_numpy(np.asarray(tensors[f"{n}/{n1}"])) for n in fp.names() if f"{n}/{n1}" in tensors}
    slot2 = {n: torch.from_numpy(np.asarray(tensors[f"{n}/{n2}"])) for n in fp.names()
             if n2 and f"{n}/{n2}" in tensors}
    fp.load_state(vals, ema_too=not emas, ema_values=emas, mom_values=moms, slot2_values=slot2)
    step = int(np.asarray(tensors.get("global_step", 0)))
    fp.step.fill_(step)
    le = net.loss_ema.view(-1, 3)
    for i, name in enumerate(net.loss_names):
        if f"{name}/avg/biased" in tensors:
            le[i, 0] = float(tensors[f"{name}/avg/biased"])
            le[i, 1] = float(tensors[f"{name}/avg/local_step"])
            le[i, 2] = float(tensors[f"{name}/avg"])
    return step


class Replica:
    def __init__(self, spec: ModelSpec, impl: str, batch: int, device, init: Dict[str, torch.Tensor], opt: OptConfig,
                 train_images: torch.Tensor, train_labels: torch.Tensor, src_channels: int,
                 eval_images: Optional[torch.Tensor] = None, eval_labels: Optional[torch.Tensor] = None,
                 seed: int = 0, shard: bool = True, use_graph: bool = True, bucket_mb: float = 4.0,
                 group=None, standalone: bool = False, fused_input=False, precision: str = "bf16",
                 dp_graph: bool = False, augment=None, mix=None, log=print, teacher=None):
        """``augment``: a ``data.augment.AugmentConfig``; when any of its amounts is non-zero the
        training batches (and only those) are shifted / rotated / zoomed on the device.
        ``mix``: a ``data.mix.MixConfig``; when it mixes anything, ``opt.mix`` must be set (the net then
        holds ``labels2`` / ``mix_lam``) and the training batches are mixed by the loader.
        ``teacher``: knowledge distillation -- a callable ``(student net, impl, precision) -> Teacher``
        (``runtime.teacher.TeacherSource``), called once the net exists; ``opt.distill_alpha`` must be > 0.
        The teacher's forward then runs in the step body, before the student's step."""
        self.spec, self.impl, self.B, self.device = spec, impl, batch, torch.device(device)
        self.net = build_net(impl, spec, batch, self.device, init, opt, precision)
        self.teacher = None
        if teacher is not None:
            if not opt.distill_alpha > 0:
                raise ValueError("a teacher needs OptConfig(distill_alpha > 0): the training loss reads its logits")
            self.teacher = teacher(self.net, impl, precision)
        elif opt.distill_alpha > 0:
            raise ValueError(f"distill_alpha={opt.distill_alpha} needs a teacher (distill_from)")
        # standalone: a parameter-server worker (no data-parallel group of its own)
        dp_on = dist.is_initialized() and not standalone
        self.world = dist.get_world_size(group) if dp_on else 1
        self.rank = dist.get_rank(group) if dp_on else 0
        self.dp = DataParallel(self.net, group=group, bucket_cap_mb=bucket_mb, world=self.world)
        self.train_ds = DeviceDataset(train_images, train_labels, self.device, hw=784, channels=src_channels)
        self.eval_ds = (DeviceDataset(eval_images, eval_labels, self.device, hw=784, channels=src_channels)
                        if eval_images is not None else None)
        # --input_mode u8 / bf16 (HIP; --fused_input = u8): the first fused conv gathers the
        # resident training set (uint8, or normalised once to bf16) through the batch index
        mode = "u8" if fused_input is True else (fused_input or "prep")
        self.augment = augment if augment is not None and augment.enabled else None
        if self.augment is not None and mode != "prep":
            # the first fused conv can only gather un-augmented dataset rows
            log(f"augmentation is on: input mode {mode!r} -> 'prep' (the augmentation kernel writes the input buffer)")
            mode = "prep"
        self.mix = mix if mix is not None and mix.enabled else None
        if self.mix is not None and not opt.mix:
            raise ValueError("a MixConfig that mixes needs OptConfig(mix=True): the training loss reads two labels")
        if self.mix is not None and mode != "prep":
            # the first fused conv can only gather unmixed dataset rows
            log(f"mixup / CutMix is on: input mode {mode!r} -> 'prep' (the mix kernel works on the input buffer)")
            mode = "prep"
        if self.teacher is not None and mode != "prep":
            # the teacher reads the input buffer, which the gathering first conv never writes
            log(f"distillation is on: input mode {mode!r} -> 'prep' (the teacher reads the input buffer)")
            mode = "prep"
        # eligibility first: a model that cannot gather (3-channel input, fp32 executor) never
        # gets a normalised bf16 copy of the whole split built for nothing
        fused_in = (impl == "hip" and mode != "prep" and getattr(self.net, "can_gather_input", lambda: True)()
                    and self.net.bind_u8_input(self.train_ds.images if mode == "u8" else self.train_ds.bf16_images(),
                                                bwd_images=None if mode == "u8" else self.train_ds.images))
        self.loader = DeviceLoader(self.train_ds, self.net.x0, self.net.labels, rank=self.rank, world=self.world,
                                   seed=seed, shard=shard, idx_out=self.net.idx_buf if fused_in else None,
                                   augment=self.augment, mix=self.mix,
                                   out_labels2=getattr(self.net, "labels2", None),
                                   out_lam=getattr(self.net, "mix_lam", None))
        # hipGraph: single replica, or (dp_graph) the DP step with its RCCL all-reduces captured
        self.use_graph = (use_graph and impl == "hip" and self.device.type == "cuda"
                          and (self.world == 1 or (dp_graph and dist.get_backend(group) == "nccl")))
        self._graph = None
        self._eval_acc = None      # obs.eval_metrics.EvalAccumulator of evaluate(metrics=True), made on first use
        self.global_step = 0
        self.examples_per_step = batch * self.world
        if self.teacher is not None and self.eval_ds is not None:
            ev = self.teacher.evaluate(self.eval_ds)
            log(f"distillation teacher {self.teacher.spec.name}: test accuracy {ev['accuracy']:.4f} "
                f"(loss {ev['loss']:.4f}, {ev['examples']} examples)")

    # ------------------------------------------------------------------ steps
    def _body(self) -> None:
        if self.teacher is not None:      # the soft targets of the batch the loader just wrote
            self.teacher.forward(self.B)
        self.dp.train_step()

    def step(self) -> None:
        self.loader.next()
        if self.use_graph and self._graph is None:
            from ..runtime.graph import StepGraph
            # the warm-up inside StepGraph IS this step (on the batch just loaded);
            # capture itself executes nothing, so exactly one update happens here
            self._graph = StepGraph(self._body, warmup=1)
        elif self.use_graph:
            self._graph.replay()
        else:
            self._body()
        self.global_step += 1

    def sync_step_from_device(self) -> None:
        self.global_step = int(self.net.fp.step.item())

    def learning_rate(self) -> float:
        return self.net.opt.lr_at(self.global_step)

    def read_stats(self) -> Dict[str, float]:
        # local replica's last step (no collective: hooks run on the chief only)
        return self.net.read_stats()

    def evaluate(self, max_examples: Optional[int] = None, metrics: bool = False) -> Dict[str, float]:
        """Full (or capped) pass over the eval split; returns loss / accuracy.
        ``metrics``: the dict gains ``"metrics"``, ``obs.eval_metrics.derive`` of the pass's
        accumulators (confusion matrix, top-k, NLL, Brier, ECE, per-class scores), computed on the
        device where the logits are (one small copy for the whole pass).  ``loss`` / ``accuracy``
        then come from the HIP executor's layered head, not its fused one: they may differ from
        those of ``metrics=False`` in the last bits."""
        if self.eval_ds is None:
            return {"loss": float("nan"), "accuracy": float("nan")}
        acc = None
        if metrics:
            from ..obs.eval_metrics import EvalAccumulator, derive
            if self._eval_acc is None:
                self._eval_acc = EvalAccumulator(self.device, self.net.n_classes)
            acc = self._eval_acc
            acc.zero()
        st = self.net.eval_stats
        st.zero_()
        n = 0
        for nb in eval_batches(self.eval_ds, self.net.x0, self.net.labels):
            if acc is None:
                self.net.eval_batch(nb, st)
            else:
                self.net.eval_batch(nb, st, metrics=acc)
            n += nb
            if max_examples and n >= max_examples:
                break
        # local pass (no collective, so chief-only hooks can call it safely)
        v = (st[:2] / max(n, 1)).tolist()
        out = {"loss": v[0], "accuracy": v[1]}
        if acc is not None:
            out["metrics"] = derive(acc.result())
        return out

    def inject_nan(self) -> None:
        """Fault injection: poison params[0], the first layer's first weight.  On the torch path
        the NaN propagates to the loss; on the HIP path the layer's fmaxf ReLU turns it into 0,
        and the NaN guard fires through the weight-decay term alone -- the weight is a
        weight-decay entry (coefficient 0.0 included), so the step's total loss is
        ce + wd / 2 * sum(w^2) = NaN (tests/test_stats_path_gpu.py, total-loss route)."""
        with torch.no_grad():
            self.net.fp.params[0] = float("nan")
        self.net.fp.refresh_bf16()

    def synchronize(self) -> None:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
