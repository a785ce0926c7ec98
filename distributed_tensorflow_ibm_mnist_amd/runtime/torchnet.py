"""Plain-PyTorch replica with the same interface as ``HipNet``.

Used for (a) the CPU test path (multi-process gloo tests of data-parallel and
parameter-server logic, the BASELINE "MLP single-process CPU" config), and
(b) ``--impl torch``: the PyTorch-ROCm baseline (MIOpen convolutions,
hipBLASLt GEMMs, bf16 autocast) that the HIP kernels are measured against.
It shares ``FlatParams`` (flat fp32 params/grads/slots) so checkpoints, DP
buckets and PS transfers are identical between the two implementations.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F

from ..models import torch_ref
from ..models.spec import Conv, Dense, ModelSpec
from .params import FlatParams, OptConfig


def _adaptive_update(fp: FlatParams, cfg: OptConfig, g: torch.Tensor, lr: float, t: int) -> None:
    """Adam / RMSProp / Adagrad with TF1 semantics (the fused kernel's adaptive rules); the
    slots are ``fp.mom`` and ``fp.slot2`` as ``OptConfig.slot_names`` lays them out."""
    if cfg.rule == "adam":
        m, v = fp.mom, fp.slot2
        m.mul_(cfg.beta1).add_(g, alpha=1.0 - cfg.beta1)
        v.mul_(cfg.beta2).add_(g * g, alpha=1.0 - cfg.beta2)
        # bias corrections in double: fp32 1 - 0.999**t is off by 6e-5 at t = 1
        c1 = -math.expm1(t * math.log(cfg.beta1)) if cfg.beta1 > 0 else 1.0
        c2 = -math.expm1(t * math.log(cfg.beta2)) if cfg.beta2 > 0 else 1.0
        # epsilon outside the root: m = v = 0 gives a zero update, never 0 * inf
        fp.params.sub_(m / (v.sqrt() + cfg.eps), alpha=lr * math.sqrt(c2) / c1)
    elif cfg.rule == "rmsprop":
        mom, ms = fp.mom, fp.slot2
        ms.mul_(cfg.rmsprop_decay).add_(g * g, alpha=1.0 - cfg.rmsprop_decay)
        mom.mul_(cfg.momentum).add_(g / (ms + cfg.eps).sqrt(), alpha=lr)
        fp.params.sub_(mom)
    else:
        acc = fp.mom
        acc.add_(g * g)
        fp.params.sub_(g / acc.sqrt(), alpha=lr)


def _trust_ratio(adapted: bool, pn: torch.Tensor, un: torch.Tensor, num: torch.Tensor) -> torch.Tensor:
    """``num`` where the variable is adapted and both norms are > 0, else 1; NaN for a non-finite
    norm of an adapted variable (never hidden behind the > 0 tests)."""
    one = torch.ones_like(pn)
    if not adapted:
        return one
    r = torch.where((pn > 0) & (un > 0), num, one)
    return torch.where(torch.isfinite(pn) & torch.isfinite(un), r, torch.full_like(pn, float("nan")))


def _layerwise_update(fp: FlatParams, cfg: OptConfig, g: torch.Tensor, lr: float, t: int) -> None:
    """LARS (momentum) and LAMB (Adam, no decoupled decay) in fp32: one trust ratio per variable
    of rank >= 2, 1 for the biases; fills ``fp.tnorm[:3 * nvar]`` as the fused kernels do."""
    if fp.tnorm is None or (cfg.rule == "lamb" and fp.slot2 is None):
        raise RuntimeError(f"optimizer rule {cfg.rule!r} needs FlatParams.init_slots(cfg) before the first step")
    if cfg.rule == "lamb":
        m, v = fp.mom, fp.slot2
        m.mul_(cfg.beta1).add_(g, alpha=1.0 - cfg.beta1)
        v.mul_(cfg.beta2).add_(g * g, alpha=1.0 - cfg.beta2)
        c1 = -math.expm1(t * math.log(cfg.beta1)) if cfg.beta1 > 0 else 1.0
        c2 = -math.expm1(t * math.log(cfg.beta2)) if cfg.beta2 > 0 else 1.0
        u = (m / c1) / ((v / c2).sqrt() + cfg.eps)
    else:
        u = g
    scaled = torch.empty_like(u)
    for i, e in enumerate(fp.entries):
        sl = slice(e.off, e.off + e.n)
        pn, un = fp.params[sl].square().sum().sqrt(), u[sl].square().sum().sqrt()
        num = pn / un if cfg.rule == "lamb" else cfg.lars_eta * pn / (un + cfg.eps)
        r = _trust_ratio(len(e.shape) >= 2, pn, un, num)
        fp.tnorm[3 * i], fp.tnorm[3 * i + 1], fp.tnorm[3 * i + 2] = pn, un, r
        scaled[sl] = u[sl] * r
    if cfg.rule == "lamb":
        fp.params.sub_(scaled, alpha=lr)
    else:
        fp.mom.mul_(cfg.momentum).add_(scaled)
        fp.params.sub_(lr * fp.mom)


def torch_update(fp: FlatParams, cfg: OptConfig, grad_scale: float = 1.0) -> None:
    """Reference-semantics update (same math as the fused K9 kernel)."""
    with torch.no_grad():
        step = int(fp.step.item())
        lr = cfg.lr_at(step)
        wd = torch.zeros_like(fp.params)
        for i, e in enumerate(fp.entries):
            if e.wd:
                wd[e.off:e.off + e.n] = e.wd
            if e.l2_index >= 0:
                v = fp.params[e.off:e.off + e.n]
                fp.l2[e.l2_index] += (v * v).sum()
        g = fp.grads * grad_scale + wd * fp.params
        if cfg.clip_norm is not None:
            # tf.clip_by_global_norm in fp32: s = c / max(norm, c) (1 exactly at or below c),
            # NaN for a non-finite norm
            if fp.gnorm is None:
                raise RuntimeError("clip_norm needs FlatParams.init_slots(cfg) before the first step")
            c = torch.tensor(cfg.clip_norm, dtype=torch.float32, device=g.device)
            gn = (g * g).sum().sqrt()
            s = torch.where(torch.isfinite(gn), c / torch.maximum(gn, c), torch.full_like(gn, float("nan")))
            fp.gnorm[0] = gn
            fp.gnorm[1] = s
            g = g * s
        if cfg.layerwise:
            _layerwise_update(fp, cfg, g, lr, step + 1)
        elif cfg.adaptive:
            _adaptive_update(fp, cfg, g, lr, step + 1)
        else:
            if cfg.use_momentum:
                fp.mom.mul_(cfg.momentum).add_(g)
                upd = g + cfg.momentum * fp.mom if cfg.nesterov else fp.mom
            else:
                upd = g
            fp.params.sub_(lr * upd)
        if cfg.ema_max >= 0:
            d = min(cfg.ema_max, (1.0 + step) / (10.0 + step))
            fp.ema.sub_((1.0 - d) * (fp.ema - fp.params))


def _in_top1(logits: torch.Tensor, lab: torch.Tensor) -> torch.Tensor:
    """Top-1 count with the reference's tf.nn.in_top_k rule (mnist_input.py:237-243), which is
    also the HIP kernels': a row is correct when logit[label] >= max(logits), so a tie at the
    maximum counts for every tied class (argmax would credit only the first)."""
    return (logits.gather(1, lab.view(-1, 1)).squeeze(1) >= logits.max(1).values).sum().float()


class TorchNet:
    def __init__(self, spec: ModelSpec, batch: int, device, init: Dict[str, torch.Tensor],
                 opt: Optional[OptConfig] = None, autocast: Optional[bool] = None, x0: Optional[torch.Tensor] = None):
        """``x0``: an input buffer to adopt instead of allocating one (HipNet)."""
        dev = torch.device(device)
        self.spec, self.B, self.device = spec, batch, dev
        self.opt = opt or OptConfig()
        specs = []
        for L in spec.weights():
            shp = (L.kh, L.kw, L.cin, L.cout) if isinstance(L, Conv) else (L.din, L.dout)
            specs.append((f"{L.name}/weights", shp, L.wd))
            specs.append((f"{L.name}/biases", (L.cout if isinstance(L, Conv) else L.dout,), None))
        self.fp = FlatParams.build(specs, init, dev)
        self.fp.init_slots(self.opt)
        H, W = spec.input_hw
        self.autocast = (dev.type == "cuda") if autocast is None else autocast
        xdt = torch.bfloat16 if dev.type == "cuda" else torch.float32
        if x0 is not None and (tuple(x0.shape) != (batch, H, W, spec.in_channels) or x0.dtype != xdt or x0.device != dev):
            raise ValueError(f"x0 must be a {xdt} tensor of shape {(batch, H, W, spec.in_channels)} on {dev}, got "
                             f"{x0.dtype} {tuple(x0.shape)} on {x0.device}")
        self.x0 = torch.zeros(batch, H, W, spec.in_channels, dtype=xdt, device=dev) if x0 is None else x0
        self.labels = torch.zeros(batch, dtype=torch.int32, device=dev)
        # knowledge distillation (opt.distill_alpha > 0): the teacher's logits [>= batch, >= classes] that the
        # training loss reads (HipNet.teacher_logits)
        self.teacher_logits: Optional[torch.Tensor] = None
        # mixup / CutMix: the loader's second labels and weights, read by the training loss alone
        self.labels2: Optional[torch.Tensor] = None
        self.mix_lam: Optional[torch.Tensor] = None
        if self.opt.mix:
            self.labels2 = torch.zeros(batch, dtype=torch.int32, device=dev)
            self.mix_lam = torch.ones(batch, dtype=torch.float32, device=dev)
        self.stats = torch.zeros(8, dtype=torch.float32, device=dev)
        self.eval_stats = torch.zeros(8, dtype=torch.float32, device=dev)
        names = [e.name for e in self.fp.wd_entries]
        self.loss_names = [n.replace("/weights", "/weight_loss") for n in names] + ["cross_entropy", "total_loss"]
        self.loss_ema = torch.zeros(3 * len(self.loss_names), dtype=torch.float32, device=dev)
        self.grad_ready_hooks: List[Callable[[int], None]] = []
        self.n_classes = spec.num_classes
        self._logits: Optional[torch.Tensor] = None
        self._loss: Optional[torch.Tensor] = None
        self._leaf: Optional[torch.Tensor] = None
        self._acts: Dict[str, torch.Tensor] = {}
        self.keep_activations = False

    def _params(self, leaf: torch.Tensor) -> Dict[str, torch.Tensor]:
        return {e.name: leaf[e.off:e.off + e.n].view(e.shape) for e in self.fp.entries}

    def forward(self, nb: Optional[int] = None, grad: bool = True, defer_head: bool = False) -> torch.Tensor:
        nb = self.B if nb is None else nb
        leaf = self.fp.params.detach().requires_grad_(grad)
        self._leaf = leaf
        x = self.x0[:nb].float() if not self.autocast else self.x0[:nb]
        # dropout on the training forward alone (grad=True; eval_batch / probs pass grad=False): the
        # host reference's masks at the current global step, bit for bit the HIP executor's
        drop = self.dropout_multipliers(nb) if (grad and self.opt.dropout > 0) else None
        with torch.autocast(self.device.type, dtype=torch.bfloat16, enabled=self.autocast):
            logits, acts = torch_ref.forward(self.spec, self._params(leaf), x, keep_activations=self.keep_activations,
                                             dropout=drop)
        self._acts = acts
        self._logits = logits.float()
        return self._logits

    def dropout_multipliers(self, nb: int, step: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """{layer name: multiplier [nb, dout]} of the dropped layers at ``step`` (default: now)."""
        from ..ops import dropout as D
        t = int(self.fp.step.item()) if step is None else int(step)
        return {name: torch.from_numpy(D.multiplier(self.opt.dropout_seed, t, idx, nb, self.spec.layers[idx].dout,
                                                    self.opt.dropout)).to(self.device)
                for name, idx in D.dropout_layers(self.spec).items()}

    def loss_and_grad(self, nb: Optional[int] = None, scale: Optional[float] = None) -> None:
        nb = self.B if nb is None else nb
        if self._leaf is None or not self._leaf.requires_grad:
            self.forward(nb, grad=True)
        lab = self.labels[:nb].long()
        # the training loss (and its cross_entropy scalar) is the smoothed one; eval_batch is not
        if self.opt.distill_alpha > 0:      # torch_ref.losses' distilled form, as a sum over the rows
            if self.teacher_logits is None:
                raise RuntimeError(f"distill_alpha={self.opt.distill_alpha} needs the net's teacher_logits, which is not set")
            loss = torch_ref.distillation_loss(self._logits, lab, self.teacher_logits[:nb, :self.n_classes],
                                               self.opt.distill_alpha, self.opt.distill_temperature).sum()
        elif self.opt.mix:    # torch_ref.losses' two-label form, as a sum over the rows
            loss = torch_ref.two_label_cross_entropy(self._logits, lab, self.labels2[:nb], self.mix_lam[:nb],
                                                     self.opt.label_smoothing).sum()
        else:
            loss = F.cross_entropy(self._logits, lab, reduction="sum", label_smoothing=self.opt.label_smoothing)
        with torch.no_grad():
            self.stats[0] += loss.detach()
            self.stats[1] += _in_top1(self._logits, lab)
            if not torch.isfinite(loss.detach()):
                self.stats[2] = 1.0
        self._loss = loss * ((1.0 / nb) if scale is None else scale)

    def backward(self, nb: Optional[int] = None) -> None:
        (g,) = torch.autograd.grad(self._loss, self._leaf)
        self.fp.grads.copy_(g)
        self._leaf = None
        for i in range(len(self.spec.layers) - 1, -1, -1):
            if isinstance(self.spec.layers[i], (Conv, Dense)):
                for h in self.grad_ready_hooks:
                    h(i)

    def update(self, grad_scale: float = 1.0, increment: bool = True, batch_for_stats: Optional[int] = None) -> None:
        torch_update(self.fp, self.opt, grad_scale)
        self.finalize(batch_for_stats or self.B, increment)

    def finalize(self, batch: int, increment: bool = True) -> None:
        fp = self.fp
        with torch.no_grad():
            ce = self.stats[0] / batch
            acc = self.stats[1] / batch
            wl = [float(e.wd) * 0.5 * fp.l2[e.l2_index] for e in fp.wd_entries]
            total = ce + (sum(wl) if wl else 0.0)
            vals = wl + [ce, total]
            for i, v in enumerate(vals):
                e = self.loss_ema[3 * i:3 * i + 3]
                e[0] = 0.9 * e[0] + 0.1 * v
                e[1] += 1
                e[2] = e[0] / (1 - 0.9 ** e[1])
            self.stats[4] = ce
            self.stats[5] = acc
            self.stats[6] = total
            self.stats[7] += 1
            self.stats[0] = 0
            self.stats[1] = 0
            fp.l2.zero_()
            if increment:
                fp.step += 1

    def train_step(self, grad_scale: float = 1.0) -> None:
        self.forward()
        self.loss_and_grad()
        self.backward()
        self.update(grad_scale)

    def eval_batch(self, nb: int, stats: Optional[torch.Tensor] = None, metrics=None) -> torch.Tensor:
        """``metrics``: an ``obs.eval_metrics.EvalAccumulator``; the batch's logits go to its host
        reference (``obs/eval_metrics.py``), wherever this net lives."""
        st = self.eval_stats if stats is None else stats
        with torch.no_grad():
            logits = self.forward(nb, grad=False)
            lab = self.labels[:nb].long()
            st[0] += F.cross_entropy(logits, lab, reduction="sum")
            st[1] += _in_top1(logits, lab)
            if metrics is not None:
                metrics.add(logits.float().cpu(), self.labels[:nb].cpu(), nb)
        return st

    def probs(self, nb: int) -> torch.Tensor:
        with torch.no_grad():
            return torch.softmax(self.forward(nb, grad=False)[:, : self.n_classes], 1)

    def activation(self, layer_name: str) -> torch.Tensor:
        return self._acts[layer_name]

    def layer_activation(self, layer_name: str, n: int) -> torch.Tensor:
        """``<layer>/<layer>:0`` (main.py:97-100) for the first n images of the
        current batch, recomputed without autograd (monitoring only)."""
        n = max(1, min(n, self.B))
        with torch.no_grad():
            x = self.x0[:n].float() if not self.autocast else self.x0[:n]
            with torch.autocast(self.device.type, dtype=torch.bfloat16, enabled=self.autocast):
                _, acts = torch_ref.forward(self.spec, self._params(self.fp.params), x, keep_activations=True)
        return acts[layer_name]

    def read_stats(self) -> Dict[str, float]:
        s = self.stats.detach().cpu().tolist()
        out = {"cross_entropy": s[4], "accuracy": s[5], "total_loss": s[6], "nan": s[2]}
        if self.opt.clip_norm is not None:   # the last update's norm before clipping, and its scale
            out["global_norm"], out["clip_scale"] = self.fp.gnorm[:2].detach().cpu().tolist()
        if self.opt.layerwise:   # the last update's trust ratio of every adapted variable
            out.update(self.fp.trust_ratio_stats())
        return out
