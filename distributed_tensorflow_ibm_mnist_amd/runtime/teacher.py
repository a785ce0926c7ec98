"""The frozen teacher of knowledge distillation.

A ``Teacher`` holds an executor of its own (``build_net``: HipNet, HipNetF32 or TorchNet, whatever the
student runs on) with the weights of a checkpoint, shares the student's input buffer ``x0`` -- so it sees
exactly the batch the student sees, augmentation included -- and leaves its fp32 logits in a fixed
buffer that the student's training loss reads in place (the executors' ``teacher_logits``,
``OptConfig.distill_alpha`` / ``distill_temperature``; csrc/kernels/ce_stats.h DISTILL).  It is never
updated: nothing here touches its parameters after the restore.

``Teacher.forward(nb)`` is the eval-form forward (``from_x0=True``, the head not deferred, no dropout):
plain launches on the current stream, the same eagerly and under hipGraph capture.
"""
from __future__ import annotations

import dataclasses
import os
from typing import Dict, Optional

import numpy as np
import torch

from ..models.spec import ModelSpec
from .params import OptConfig


def _shape_of(spec: ModelSpec):
    return (spec.in_channels, tuple(spec.input_hw), spec.num_classes)


def check_specs(teacher: ModelSpec, student: ModelSpec) -> None:
    """The teacher reads the student's input buffer and its logits are the student's target: the
    input channels, the input size and the class count must be the same."""
    if _shape_of(teacher) != _shape_of(student):
        def fmt(s):
            return f"{s.name} (in_channels {s.in_channels}, input_hw {tuple(s.input_hw)}, num_classes {s.num_classes})"
        raise ValueError(f"the teacher {fmt(teacher)} does not fit the student {fmt(student)}: in_channels, input_hw "
                         f"and num_classes must be equal")


def checkpoint_params(ckpt_dir: str, spec: ModelSpec, use_ema: bool = False) -> Dict[str, torch.Tensor]:
    """The weights and biases of ``spec`` from the latest checkpoint in ``ckpt_dir`` (``Saver.restore``, the
    path inference.py takes); ``use_ema``: the ``ExponentialMovingAverage`` shadows."""
    from ..ckpt.saver import Saver, get_checkpoint_state
    ckpt = get_checkpoint_state(ckpt_dir)
    if not (ckpt and ckpt.model_checkpoint_path):
        raise ValueError(f"distill_from: no checkpoint found in {ckpt_dir!r}")
    tensors = Saver.restore(ckpt.model_checkpoint_path)
    params = {}
    for L in spec.weights():
        for kind in ("weights", "biases"):
            n = f"{L.name}/{kind}"
            key = f"{n}/ExponentialMovingAverage" if use_ema else n
            if key not in tensors:
                raise ValueError(f"distill_from: the checkpoint {ckpt.model_checkpoint_path!r} lacks {key!r} "
                                 f"(distill_model {spec.name!r})")
            params[n] = torch.from_numpy(np.asarray(tensors[key], dtype=np.float32))
    return params


class Teacher:
    def __init__(self, spec: ModelSpec, params: Dict[str, torch.Tensor], student, impl: str, precision: str = "bf16"):
        """``student``: the executor that is trained; the teacher takes its batch size, its device and its
        input buffer, and hands it the logits buffer (``student.teacher_logits``)."""
        from ..train.replica import build_net
        check_specs(spec, student.spec)
        self.spec, self.B, self.device = spec, student.B, student.device
        # no EMA and no slots to speak of: the executor is only ever run forward
        self.net = build_net(impl, spec, self.B, self.device, params, OptConfig(ema_max=-1.0), precision, x0=student.x0)
        assert self.net.x0 is student.x0
        self.n_classes = spec.num_classes
        own = getattr(self.net, "logits", None)
        # HipNet / HipNetF32 write their logits into a fixed fp32 buffer; TorchNet's are copied into one
        self._copy = own is None
        self.logits = torch.zeros(self.B, self.n_classes, dtype=torch.float32, device=self.device) if self._copy else own
        student.teacher_logits = self.logits

    @classmethod
    def from_checkpoint(cls, ckpt_dir: str, model: str, student, impl: str, precision: str = "bf16",
                        use_ema: bool = False) -> "Teacher":
        from ..models import get_model
        spec = get_model(model, student.spec.in_channels)
        check_specs(spec, student.spec)
        return cls(spec, checkpoint_params(ckpt_dir, spec, use_ema), student, impl, precision)

    def forward(self, nb: Optional[int] = None) -> torch.Tensor:
        """The teacher's logits of rows < nb of the shared input buffer, left in ``self.logits``."""
        nb = self.B if nb is None else nb
        if self._copy:
            with torch.no_grad():
                self.logits[:nb].copy_(self.net.forward(nb, grad=False)[:, :self.n_classes])
        else:
            self.net.forward(nb, from_x0=True)
        return self.logits

    def evaluate(self, eval_ds, max_examples: Optional[int] = None) -> Dict[str, float]:
        """The teacher's own loss and top-1 accuracy over an eval split (it overwrites the shared input
        buffer: for start-up, before the first training batch is loaded)."""
        from ..data.device_loader import eval_batches
        st = self.net.eval_stats
        st.zero_()
        n = 0
        for nb in eval_batches(eval_ds, self.net.x0, self.net.labels):
            self.net.eval_batch(nb, st)
            n += nb
            if max_examples and n >= max_examples:
                break
        v = (st[:2] / max(n, 1)).tolist()
        return {"loss": v[0], "accuracy": v[1], "examples": n}


@dataclasses.dataclass(frozen=True)
class TeacherSource:
    """Where a ``Replica`` gets its teacher from: called with the student's executor once that exists.
    Every data-parallel rank and every parameter-server worker loads the checkpoint itself."""
    ckpt_dir: str
    model: str
    use_ema: bool = False

    def __post_init__(self):
        if not self.model:
            raise ValueError(f"distill_model is required with distill_from ({self.ckpt_dir!r})")
        if not os.path.isdir(self.ckpt_dir):
            raise ValueError(f"distill_from must be a checkpoint directory, got {self.ckpt_dir!r}")

    def __call__(self, student, impl: str, precision: str = "bf16") -> Teacher:
        return Teacher.from_checkpoint(self.ckpt_dir, self.model, student, impl, precision, self.use_ema)
