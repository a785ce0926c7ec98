"""Chief-only training monitor — the in-repo equivalent of DLI's ``monitor_cb.CMonitor``.

The reference registers, on the chief (``main.py:75-109``):
``SummaryHist`` (weights / biases / activations of conv1, conv2, local3, local4),
``SummaryNorm2`` (weight L2 norms), ``SummaryGradient`` (gradient histograms),
``SummaryGWRatio`` (gradient/weight ratio) and the scalars ``train loss``,
``train accuracy``, ``test loss``, ``test accuracy``, merged into a TRAIN and a
TEST collection written by ``_LoggerHook`` every ``test_interval`` steps to
``train_dir/log``.  ``monitor_cb`` itself is not in the repository [DLI]; this
class reproduces each summary type as TensorBoard event data under the same
names.  Unlike the reference (Q5), "test" scalars come from a real pass over
the held-out split, not from the next training batch.

Activations are the reference's ``<layer>/<layer>:0`` tensors (``main.py:97-100``):
a conv layer's bias+ReLU output BEFORE pooling (conv1: ``[n,28,28,32]``), for the
first ``sample`` images of the last batch.  Where conv and pool run as one fused
kernel that tensor never exists, so the executor recomputes it for the sample with
the unfused conv kernel (``HipNet.layer_activation``); dense layers expose their
live output buffers.  Channel padding is stripped.
"""
from __future__ import annotations

import json
import math
import os
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from .events import EventFileWriter, histogram_value, scalar_value, summary

DLMAO_TRAIN_SUMMARIES = "DLMAO_TRAIN_SUMMARIES"
DLMAO_TEST_SUMMARIES = "DLMAO_TEST_SUMMARIES"


class Monitor:
    def __init__(self, log_dir: str, test_interval: int, max_steps: int, replica, sample: int = 64,
                 eval_examples: Optional[int] = 10000, log=print, device_summaries: bool = False,
                 eval_metrics: bool = False):
        self.log_dir = log_dir
        self.test_interval, self.max_steps = test_interval, max_steps
        self.replica = replica
        self.sample = sample
        self.eval_examples = eval_examples
        self.writer = EventFileWriter(log_dir)
        self.log = log
        self._train: List[Tuple[str, Callable[[], bytes]]] = []
        self._test: List[Tuple[str, Callable[[], bytes]]] = []
        self._test_cache: Dict[str, float] = {}
        # device_summaries: write_train computes its histograms and norms on the device
        # (obs/device_summary.py) when the parameters live on one; _kinds: what each registered
        # train tag is made of, for that path (tags not in it are always computed by their closure)
        self.device_summaries = bool(device_summaries)
        self._kinds: Dict[str, Tuple[str, str]] = {}
        self._summarizer = None
        # eval_metrics: write_test also evaluates obs/eval_metrics.py's metrics (on the device
        # for a HIP executor), appends their scalars after the registered test tags and one JSON
        # line per write to <log_dir>/eval_metrics.jsonl
        self.eval_metrics = bool(eval_metrics)

    # ---- registration API (names as in monitor_cb) ------------------------
    def _fp(self):
        return self.replica.net.fp

    def SummaryHist(self, kind: str, layer: str) -> None:
        """kind: 'weight' | 'bias' | 'activation'."""
        tag = f"{layer}/{kind}"
        if kind == "weight":
            fn = lambda: self._fp().param_view(f"{layer}/weights").detach().float().cpu().numpy()  # noqa: E731
            self._kinds[tag] = ("param_hist", f"{layer}/weights")
        elif kind == "bias":
            fn = lambda: self._fp().param_view(f"{layer}/biases").detach().float().cpu().numpy()  # noqa: E731
            self._kinds[tag] = ("param_hist", f"{layer}/biases")
        elif kind == "activation":
            fn = lambda: self._activation(layer)  # noqa: E731
            self._kinds[tag] = ("act_hist", layer)
        else:
            raise ValueError(kind)
        self._train.append((tag, lambda: histogram_value(tag, fn())))

    def SummaryNorm2(self, kind: str, layer: str) -> None:
        tag = f"{layer}/{kind}_norm2"
        name = f"{layer}/weights" if kind == "weight" else f"{layer}/biases"
        self._kinds[tag] = ("param_norm", name)
        self._train.append((tag, lambda: scalar_value(tag, float(self._fp().param_view(name).norm().item()))))

    def SummaryGradient(self, kind: str = "weight", loss=None) -> None:
        fp = self._fp()
        for e in fp.entries:
            if kind == "weight" and not e.name.endswith("/weights"):
                continue
            tag = f"gradient/{e.name}"
            self._kinds[tag] = ("grad_hist", e.name)
            self._train.append((tag, (lambda n=e.name, t=tag: histogram_value(t, self._grad(n)))))

    def SummaryGWRatio(self) -> None:
        fp = self._fp()
        for e in fp.entries:
            if not e.name.endswith("/weights"):
                continue
            tag = f"gw_ratio/{e.name}"
            self._kinds[tag] = ("gw_ratio", e.name)

            def fn(n=e.name, t=tag):
                w = float(self._fp().param_view(n).norm().item())
                g = float(np.linalg.norm(self._grad(n)))
                return scalar_value(t, g / w if w > 0 else 0.0)
            self._train.append((tag, fn))

    def SummaryScalar(self, name: str, source: Optional[str] = None) -> None:
        """'train loss' / 'train accuracy' / 'test loss' / 'test accuracy'."""
        if name.startswith("test"):
            key = "loss" if "loss" in name else "accuracy"
            self._test.append((name, lambda k=key, n=name: scalar_value(n, self._test_cache.get(k, float("nan")))))
        else:
            key = "total_loss" if "loss" in name else "accuracy"
            self._train.append((name, lambda k=key, n=name: scalar_value(n, self.replica.read_stats()[k])))

    def register_reference_summaries(self, layers=("conv1", "conv2", "local3", "local4")) -> None:
        """The exact registration block of main.py:95-107 (layers present in the model)."""
        names = {e.name.split("/")[0] for e in self._fp().entries}
        for layer in layers:
            if layer not in names:
                continue
            self.SummaryHist("weight", layer)
            self.SummaryHist("bias", layer)
            self.SummaryHist("activation", layer)
            self.SummaryNorm2("weight", layer)
        self.SummaryGradient("weight")
        self.SummaryGWRatio()
        for s in ("train loss", "train accuracy", "test loss", "test accuracy"):
            self.SummaryScalar(s)

    # ---- helpers --------------------------------------------------------------
    def _grad(self, name: str) -> np.ndarray:
        g = self._fp().grad_view(name).detach().float().cpu().numpy()
        w = max(1, self.replica.world)
        return g / w

    def _activation(self, layer: str) -> np.ndarray:
        net = self.replica.net
        try:
            a = net.layer_activation(layer, self.sample)
        except KeyError:
            return np.zeros(1)
        a = a[: self.sample].detach().float().cpu().numpy()
        spec = {L.name: L for L in self.replica.spec.layers}.get(layer)
        real = getattr(spec, "cout", None) or getattr(spec, "dout", None)
        if real is not None and a.shape[-1] > real:
            a = a[..., :real]
        return a

    # ---- device path (device_summaries=True and the parameters on a HIP device) ----------
    def _on_device(self) -> bool:
        if not self.device_summaries:
            return False
        fp = getattr(getattr(self.replica, "net", None), "fp", None)
        return fp is not None and fp.params.is_cuda and fp.grads.is_cuda

    def _device_activation(self, layer: str):
        """The activation tensor as it lies on the device and its one segment: rows of the padded
        channel count, of which the real ones count.  None: the host path takes this tag."""
        try:
            a = self.replica.net.layer_activation(layer, self.sample)
        except KeyError:
            return None
        a = a[: self.sample].detach()
        if not (a.is_cuda and a.dim() >= 1 and a.numel() > 0 and a.is_contiguous()
                and a.dtype in (torch.bfloat16, torch.float32)):
            return None
        spec = {L.name: L for L in self.replica.spec.layers}.get(layer)
        real = getattr(spec, "cout", None) or getattr(spec, "dout", None)
        padded = a.shape[-1]
        cols = real if real is not None and padded > real else padded
        return a, (0, a.numel() // padded, cols, padded)

    def _device_jobs(self):
        """(parameter names, gradient names, {layer: (tensor, segment)}, jobs for
        DeviceSummarizer.run): one job over the parameters, one over the gradients (divided by
        world, as _grad does), one per activation tensor."""
        fp = self._fp()
        p_names: List[str] = []
        g_names: List[str] = []
        acts: Dict[str, tuple] = {}
        for tag, _ in self._train:
            kind, arg = self._kinds.get(tag, ("", ""))
            if kind in ("param_hist", "param_norm", "gw_ratio") and arg not in p_names:
                p_names.append(arg)
            if kind in ("grad_hist", "gw_ratio") and arg not in g_names:
                g_names.append(arg)
            if kind == "act_hist" and arg not in acts:
                t = self._device_activation(arg)
                if t is not None:
                    acts[arg] = t
        flat = lambda names: [(fp.by_name[n].off, 1, fp.by_name[n].n, fp.by_name[n].n) for n in names]  # noqa: E731
        jobs = [(fp.params, flat(p_names), 1.0), (fp.grads, flat(g_names), float(max(1, self.replica.world)))]
        jobs += [(a, [seg], 1.0) for a, seg in acts.values()]
        return p_names, g_names, acts, jobs

    def _device_values(self) -> List[bytes]:
        """The train summaries with every histogram and norm of a device tensor reduced there
        and brought over in one copy.  A tensor with a NaN or an infinity (counted in the last
        column) is redone by its closure, as is every tag that is not of a device tensor."""
        from .device_summary import DeviceSummarizer
        from .events import histogram_proto_from_stats
        from ..utils import proto
        dev = self._fp().params.device
        if self._summarizer is None or self._summarizer.device != dev:
            self._summarizer = DeviceSummarizer(dev)
        nb = self._summarizer.nb
        p_names, g_names, acts, jobs = self._device_jobs()
        res = self._summarizer.run(jobs)
        P = {n: (res[0][0][i], res[0][1][i]) for i, n in enumerate(p_names)}
        G = {n: (res[1][0][i], res[1][1][i]) for i, n in enumerate(g_names)}
        A = {n: (res[2 + i][0][0], res[2 + i][1][0]) for i, n in enumerate(acts)}

        def hist(tag, cs):
            c, s = cs
            if c[nb] != 0:
                return None
            h = histogram_proto_from_stats(s[0], s[1], int(c.sum()), s[2], s[3], c[:nb])
            return proto.f_bytes(1, tag) + proto.f_bytes(5, h)

        vals = []
        for tag, fn in self._train:
            kind, arg = self._kinds.get(tag, ("", ""))
            v = None
            if kind == "param_hist":
                v = hist(tag, P[arg])
            elif kind == "grad_hist":
                v = hist(tag, G[arg])
            elif kind == "act_hist" and arg in A:
                v = hist(tag, A[arg])
            elif kind == "param_norm" and P[arg][0][nb] == 0:
                v = scalar_value(tag, math.sqrt(P[arg][1][3]))
            elif kind == "gw_ratio" and P[arg][0][nb] == 0 and G[arg][0][nb] == 0:
                w, g = math.sqrt(P[arg][1][3]), math.sqrt(G[arg][1][3])
                v = scalar_value(tag, g / w if w > 0 else 0.0)
            vals.append(fn() if v is None else v)
        return vals

    # ---- writers ----------------------------------------------------------------
    def write_train(self, step: int) -> None:
        vals = self._device_values() if self._on_device() else [fn() for _, fn in self._train]
        if vals:
            self.writer.add_summary(summary(vals), step)

    def _metric_values(self, m: Dict[str, object]) -> List[bytes]:
        vals = [scalar_value(f"test {k} accuracy", float(m[k])) for k in ("top2", "top3") if k in m]
        vals += [scalar_value(f"test {k}", float(m[k])) for k in ("nll", "brier", "ece", "mce", "macro_f1")]
        vals += [scalar_value(f"test recall/{c}", float(v)) for c, v in enumerate(m["recall"])]
        vals += [scalar_value(f"test precision/{c}", float(v)) for c, v in enumerate(m["precision"])]
        return vals

    def write_test(self, step: int) -> None:
        if not self.eval_metrics:
            res = self.replica.evaluate(self.eval_examples)
        else:
            res = self.replica.evaluate(self.eval_examples, metrics=True)
        self._test_cache = res
        vals = [fn() for _, fn in self._test]
        m = res.get("metrics") if self.eval_metrics else None
        if m is not None:
            vals += self._metric_values(m)
        if vals:
            self.writer.add_summary(summary(vals), step)
        line = f"step {step}: test loss {res['loss']:.4f}  test accuracy {res['accuracy']:.4f}"
        if m is not None:
            line += f"  ECE {m['ece']:.4f}  macro-F1 {m['macro_f1']:.4f}"
            with open(os.path.join(self.log_dir, "eval_metrics.jsonl"), "a") as f:
                f.write(json.dumps({"step": int(step), **m}) + "\n")
        self.log(line)

    def flush(self) -> None:
        self.writer.flush()

    def close(self) -> None:
        self.writer.close()
