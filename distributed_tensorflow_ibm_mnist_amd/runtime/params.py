"""Flat parameter / gradient / optimizer-slot buffers (device resident).

All trainable variables live in ONE contiguous fp32 buffer (and so do their
gradients, momentum slots and EMA shadows), laid out in the reference's
creation order (``mnist_input.py:137-205``).  This gives:

* one fused optimizer launch for every tensor (K9, ``csrc/kernels/optimizer.hip``):
  L2 weight decay, SGD / momentum / Nesterov or Adam / RMSProp / Adagrad (TF1
  semantics; a second slot buffer where the rule has one), the staircase LR schedule
  (``mnist_input.py:252-256``, read from the device-side global step — no host
  sync, hipGraph capturable) or a linear warmup with polynomial / cosine decay computed
  the same way, the weight EMA with TF's
  ``min(decay, (1+t)/(10+t))`` (``mnist_input.py:265-267``), and the refresh of
  the zero-padded bf16 weight copies the GEMM kernels read;
* contiguous gradient buckets for RCCL all-reduce (``parallel/dp.py``);
* a single buffer to send/receive in parameter-server mode (``parallel/ps.py``).
"""
from __future__ import annotations

import dataclasses
import math
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import torch


ADAPTIVE_RULES = ("adam", "rmsprop", "adagrad")
# layer-wise trust ratios (LARS on momentum, LAMB on Adam): every variable of rank >= 2 scales its
# update by a ratio of its own parameter norm to its update norm; biases keep ratio 1
LAYERWISE_RULES = ("lars", "lamb")
LR_SCHEDULES = ("staircase", "polynomial", "cosine")


def check_distill(alpha, temperature) -> Tuple[float, float]:
    """``distill_alpha`` (finite, 0 <= alpha <= 1) and ``distill_temperature`` (finite, > 0, its square
    finite in fp32) as floats; anything else is a ValueError naming key and value."""
    out = []
    for key, v in (("distill_alpha", alpha), ("distill_temperature", temperature)):
        try:
            if isinstance(v, bool):
                raise ValueError
            out.append(float(v))
        except (TypeError, ValueError):
            raise ValueError(f"{key} must be a number, got {v!r}") from None
    a, t = out
    if not 0 <= a <= 1:       # NaN fails both comparisons
        raise ValueError(f"distill_alpha must be finite with 0 <= distill_alpha <= 1, got {a}")
    if not (math.isfinite(t) and t > 0 and t * t <= 3.4028234663852886e38 and 1.0 / t <= 3.4028234663852886e38
            and t >= 1.1754943508222875e-38):
        raise ValueError(f"distill_temperature must be finite and > 0 with its square finite in fp32, got {t}")
    return a, t


@dataclasses.dataclass
class OptConfig:
    lr0: float = 0.1
    decay_rate: float = 0.1
    decay_steps: int = 0          # <= 0: constant learning rate
    momentum: float = 0.0
    nesterov: bool = False
    use_momentum: bool = False
    ema_max: float = 0.9999       # MOVING_AVERAGE_DECAY (mnist_input.py:20); < 0 disables
    # update rule: "sgd" (SGD / momentum / Nesterov as use_momentum and nesterov say) or one of
    # the adaptive rules "adam" | "rmsprop" | "adagrad" (TF1 semantics and defaults).  With
    # "rmsprop", ``momentum`` is RMSProp's own momentum (TF1 default 0.0).
    # "lars" (momentum, ``lars_eta``, ``epsilon`` default 0.0) and "lamb" (beta1, beta2,
    # ``epsilon`` default 1e-6, no decoupled decay) add the layer-wise trust ratio.
    rule: str = "sgd"
    beta1: float = 0.9            # adam
    beta2: float = 0.999          # adam
    epsilon: Optional[float] = None   # None: the rule's default (adam 1e-8, rmsprop 1e-10, lars 0, lamb 1e-6)
    rmsprop_decay: float = 0.9
    adagrad_initial_accumulator: float = 0.1
    # tf.clip_by_global_norm of the gradient the rule consumes (grad * grad_scale + wd * p, every
    # variable, biases included): scaled by clip_norm / max(global_norm, clip_norm).  None: off.
    clip_norm: Optional[float] = None
    lars_eta: float = 0.001       # lars: trust coefficient, r = eta * ||p|| / (||g|| + epsilon)
    # the learning-rate schedule, a pure function of global_step t (lr_at; sched_lr in optimizer.hip):
    #   lr(t) = warm(t) * base(t),  warm(t) = (t + 1) / warmup_steps for t < warmup_steps, else 1
    #   "staircase"   base = lr0 * decay_rate ** (t // decay_steps)
    #   "polynomial"  base = lr_end + (lr0 - lr_end) * (1 - x) ** lr_power
    #   "cosine"      base = lr_end + (lr0 - lr_end) * 0.5 * (1 + cos(pi x))
    #   x = 0 up to warmup_steps, then (t - warmup_steps) / (total_steps - warmup_steps), 1 from
    #   total_steps on (where the rate is lr_end exactly)
    schedule: str = "staircase"
    warmup_steps: int = 0
    total_steps: int = 0          # polynomial | cosine: > warmup_steps
    lr_end: float = 0.0
    lr_power: float = 1.0         # polynomial
    # the training loss is the cross-entropy against (1 - eps) * onehot + eps / classes (the
    # softmax-CE kernels' smoothed instantiations); eval paths keep the hard labels.  Not an
    # optimizer quantity, but OptConfig is the nets' one training-config channel.
    label_smoothing: float = 0.0
    # inverted dropout (drop rate, as torch.nn.Dropout) on the output of every hidden ReLU Dense
    # layer, training paths only; the masks are a pure function of (dropout_seed, global step,
    # layer, row, feature) (ops/dropout.py), so there is no state.  0: nothing extra is launched.
    dropout: float = 0.0
    dropout_seed: int = 0
    # mixup / CutMix (data/mix.py): the training loss takes a second label and a weight per row, which
    # the loader's mix launch writes into the net's ``labels2`` and ``mix_lam`` buffers; eval paths keep
    # the hard labels.  The draw itself is the loader's (MixConfig); this flag only says that the
    # training loss reads the two buffers.  False: nothing is allocated, the launches are today's.
    mix: bool = False
    # knowledge distillation: the training loss is (1 - alpha) * CE(labels) + alpha * T^2 * KL(q || pT) with q
    # the softmax of a frozen teacher's logits at the temperature T and pT the student's (the softmax-CE
    # kernels' distilled instantiations, which read the net's ``teacher_logits`` buffer); eval paths keep
    # the plain cross-entropy.  0: off, nothing extra is launched.  Not combined with label_smoothing,
    # mix or dropout: those need further instantiations of the fused head.
    distill_alpha: float = 0.0
    distill_temperature: float = 2.0

    def __post_init__(self):
        if not isinstance(self.mix, (bool,)):
            raise ValueError(f"mix must be a bool, got {self.mix!r}")
        self.distill_alpha, self.distill_temperature = check_distill(self.distill_alpha, self.distill_temperature)
        from ..ops.dropout import check_rate, check_seed
        self.dropout = check_rate(self.dropout, "dropout")
        self.dropout_seed = check_seed(self.dropout_seed, "dropout_seed")
        try:
            if isinstance(self.label_smoothing, bool):
                raise ValueError
            self.label_smoothing = float(self.label_smoothing)
        except (TypeError, ValueError):
            raise ValueError(f"label_smoothing must be a number with 0 <= label_smoothing < 1, "
                             f"got {self.label_smoothing!r}") from None
        if not 0 <= self.label_smoothing < 1:     # NaN fails both comparisons
            raise ValueError(f"label_smoothing must be finite with 0 <= label_smoothing < 1, "
                             f"got {self.label_smoothing}")
        if self.distill_alpha > 0:
            for key, on in (("label_smoothing", self.label_smoothing > 0), ("mix", self.mix), ("dropout", self.dropout > 0)):
                if on:
                    raise ValueError(f"distill_alpha ({self.distill_alpha}) cannot be combined with {key} "
                                     f"({getattr(self, key)})")
        self.schedule = str(self.schedule).lower()
        if self.schedule not in LR_SCHEDULES:
            raise ValueError(f"schedule must be one of {'|'.join(LR_SCHEDULES)}, got {self.schedule!r}")
        for key in ("warmup_steps", "total_steps"):
            v = getattr(self, key)
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"{key} must be an integer, got {v!r}")
            setattr(self, key, int(v))
        if self.warmup_steps < 0:
            raise ValueError(f"warmup_steps must be >= 0, got {self.warmup_steps}")
        if self.schedule != "staircase" and self.total_steps <= self.warmup_steps:
            raise ValueError(f"total_steps must be > warmup_steps ({self.warmup_steps}), got {self.total_steps}")
        self.lr_end, self.lr_power = float(self.lr_end), float(self.lr_power)
        if not (math.isfinite(self.lr_end) and self.lr_end >= 0):
            raise ValueError(f"lr_end must be finite and >= 0, got {self.lr_end}")
        if not (math.isfinite(self.lr_power) and self.lr_power > 0):
            raise ValueError(f"lr_power must be finite and > 0, got {self.lr_power}")
        if self.clip_norm is not None:
            self.clip_norm = float(self.clip_norm)
            if not (math.isfinite(self.clip_norm) and self.clip_norm > 0):
                raise ValueError(f"clip_norm must be finite and > 0, got {self.clip_norm}")
        if self.rule in ("momentum", "nesterov"):
            self.rule = "sgd"
        if self.rule not in ("sgd",) + ADAPTIVE_RULES + LAYERWISE_RULES:
            raise ValueError(f"unknown update rule {self.rule!r} "
                             f"(sgd|{'|'.join(ADAPTIVE_RULES + LAYERWISE_RULES)})")
        if self.rule in LAYERWISE_RULES:
            if self.clip_norm is not None:
                raise ValueError(f"rule {self.rule!r} cannot be combined with clip_norm")
            self.lars_eta = float(self.lars_eta)
            if not (math.isfinite(self.lars_eta) and self.lars_eta > 0):
                raise ValueError(f"lars_eta must be finite and > 0, got {self.lars_eta}")
        if self.rule == "lars":     # momentum with a trust ratio: always the momentum slot
            self.use_momentum, self.nesterov = True, False
        if self.rule == "adagrad" and not self.adagrad_initial_accumulator > 0:
            raise ValueError("adagrad_initial_accumulator must be > 0")   # as TF1 requires

    @staticmethod
    def from_spec(spec, decay_steps: int, decay_rate: float, ema: float = 0.9999,
                  label_smoothing: float = 0.0, dropout: float = 0.0, dropout_seed: int = 0,
                  mix: bool = False, distill_alpha: float = 0.0, distill_temperature: float = 2.0) -> "OptConfig":
        """From a parameter-manager ``OptimizerSpec`` (which does not carry ``label_smoothing`` or
        the dropout keys: the caller passes ``getLabelSmoothing()``, ``getDropout()`` and the seed)."""
        lr = spec.learning_rate
        adaptive = spec.name in ADAPTIVE_RULES + LAYERWISE_RULES
        return OptConfig(lr0=float(lr), decay_rate=float(decay_rate), decay_steps=int(decay_steps),
                         momentum=float(spec.momentum), nesterov=bool(spec.nesterov),
                         use_momentum=spec.name == "momentum", ema_max=ema,
                         rule=spec.name if adaptive else "sgd", beta1=float(spec.beta1), beta2=float(spec.beta2),
                         epsilon=None if spec.epsilon is None else float(spec.epsilon),
                         rmsprop_decay=float(spec.rmsprop_decay),
                         adagrad_initial_accumulator=float(spec.adagrad_initial_accumulator),
                         clip_norm=getattr(spec, "clip_norm", None),
                         lars_eta=float(getattr(spec, "lars_eta", 0.001)),
                         schedule=getattr(spec, "lr_schedule", "staircase"),
                         warmup_steps=getattr(spec, "warmup_steps", 0),
                         total_steps=getattr(spec, "lr_total_steps", 0),
                         lr_end=getattr(spec, "lr_end", 0.0), lr_power=getattr(spec, "lr_power", 1.0),
                         label_smoothing=label_smoothing, dropout=dropout, dropout_seed=dropout_seed, mix=mix,
                         distill_alpha=distill_alpha, distill_temperature=distill_temperature)

    @property
    def scheduled(self) -> bool:
        """Anything but the plain staircase: a warmup or one of the decays after it."""
        return self.schedule != "staircase" or self.warmup_steps > 0

    def schedule_kwargs(self) -> dict:
        """The fused_optimizer / lr_at_steps keywords of the schedule."""
        return {"lr_schedule": self.schedule, "warmup_steps": self.warmup_steps, "lr_total_steps": self.total_steps,
                "lr_end": self.lr_end, "lr_power": self.lr_power}

    def lr_at(self, step: int) -> float:
        step = int(step)
        W, T = self.warmup_steps, self.total_steps
        if self.schedule == "staircase":
            base = self.lr0 if self.decay_steps <= 0 else self.lr0 * self.decay_rate ** (step // self.decay_steps)
        elif step >= T:
            return self.lr_end                    # exactly, whatever cos(pi) rounds to
        elif step <= W:
            base = self.lr0                       # x = 0: the decay starts when the warmup ends
        else:
            x = (step - W) / (T - W)
            if self.schedule == "polynomial":
                shape = (1.0 - x) ** self.lr_power
            else:
                shape = 0.5 * (1.0 + math.cos(math.pi * x))
            base = self.lr_end + (self.lr0 - self.lr_end) * shape
        if W > 0 and step < W:
            return (step + 1) / W * base
        return base

    @property
    def adaptive(self) -> bool:
        return self.rule in ADAPTIVE_RULES

    @property
    def layerwise(self) -> bool:
        return self.rule in LAYERWISE_RULES

    @property
    def eps(self) -> float:
        return self.epsilon if self.epsilon is not None else {"adam": 1e-8, "rmsprop": 1e-10,
                                                              "lamb": 1e-6}.get(self.rule, 0.0)

    def slot_names(self) -> Tuple[Optional[str], Optional[str]]:
        """TF1's slot-variable suffixes of (``FlatParams.mom``, ``FlatParams.slot2``); None: unused."""
        if self.rule in ("adam", "lamb"):
            return "Adam", "Adam_1"            # m, v
        if self.rule == "rmsprop":
            return "RMSProp_1", "RMSProp"      # mom, ms (TF1 creates the "rms" slot first)
        if self.rule == "adagrad":
            return "Adagrad", None             # accumulator
        return ("Momentum" if self.use_momentum else None), None

    def slot_init(self) -> Tuple[float, float]:
        """Initial values of the two slots, as TF1 creates them."""
        return (self.adagrad_initial_accumulator if self.rule == "adagrad" else 0.0,
                1.0 if self.rule == "rmsprop" else 0.0)


@dataclasses.dataclass
class Entry:
    name: str
    shape: Tuple[int, ...]
    wd: Optional[float]
    off: int
    n: int
    G: int
    I: int
    J: int
    Ip: int
    Jp: int
    bf_off: int
    l2_index: int   # -1: not tracked


def _f32_bits(x: float) -> int:
    return struct.unpack("<i", struct.pack("<f", float(x)))[0]


class FlatParams:
    def __init__(self, entries: List[Entry], total: int, bf_total: int, device: torch.device):
        self.entries = entries
        self.by_name = {e.name: e for e in entries}
        self.total = total
        self.device = device
        self.params = torch.zeros(total, dtype=torch.float32, device=device)
        self.grads = torch.zeros(total, dtype=torch.float32, device=device)
        # slot buffers: mom = Momentum, Adam m, RMSProp mom or the Adagrad accumulator;
        # slot2 = Adam v or RMSProp ms, allocated by init_slots() for those rules only
        self.mom = torch.zeros(total, dtype=torch.float32, device=device)
        self.slot2: Optional[torch.Tensor] = None
        # clipping by global norm: [norm before clipping, scale, the reduction's per-block
        # partials], allocated by init_slots() when OptConfig.clip_norm is set
        self.gnorm: Optional[torch.Tensor] = None
        # lars / lamb: [per variable (parameter norm, gradient / update norm, trust ratio) | the
        # reduction's per-block partials], allocated by init_slots() for those rules
        self.tnorm: Optional[torch.Tensor] = None
        self.ema = torch.zeros(total, dtype=torch.float32, device=device)
        self.bf16 = torch.zeros(max(bf_total, 1), dtype=torch.bfloat16, device=device)
        self.step = torch.zeros(1, dtype=torch.int64, device=device)
        self.wd_entries = [e for e in entries if e.l2_index >= 0]
        # [per-tensor sum(w^2) | one partial per fused-optimizer block (optimizer.hip OPT_CHUNK =
        # 512 elements)]: the partials are combined in block order (deterministic)
        n_opt_blocks = sum(-(-e.n // 512) for e in entries)
        self.l2 = torch.zeros(max(len(self.wd_entries), 1) + n_opt_blocks, dtype=torch.float32, device=device)
        self.wds = torch.tensor([float(e.wd) for e in self.wd_entries] or [0.0], dtype=torch.float32,
                                device=device)
        # name -> (offset in bf16, Jt, It): optional transposed bf16 copies W^T [Jt][It]
        self.bft: Dict[str, Tuple[int, int, int]] = {}
        self._build_segs()
        # finalize_step: {weight index, first, end fused-optimizer block} per tracked weight
        ranges, b = [], 0
        for e in entries:
            nb = -(-e.n // 512)
            if e.l2_index >= 0:
                ranges.append([e.l2_index, b, b + nb])
            b += nb
        self.l2_ranges = torch.tensor(ranges or [[0, 0, 0]], dtype=torch.int32, device=device)

    def _build_segs(self) -> None:
        rows = []
        for e in self.entries:
            t = self.bft.get(e.name)
            rows.append([e.off, e.n, e.G, e.I, e.J, e.Ip, e.Jp, e.bf_off, _f32_bits(e.wd or 0.0),
                         e.l2_index + 1, t[0] if t else -1, t[1] if t else 0, t[2] if t else 0,
                         1 if len(e.shape) >= 2 else 0])   # last: adapted by lars / lamb (the weights)
        self.segs = torch.tensor(rows, dtype=torch.int64)

    def enable_transposed(self, tdims: Dict[str, Tuple[int, int]]) -> None:
        """Also keep a transposed, zero-padded bf16 copy W^T [Jt][It] of these 2-D
        weights, rewritten by every optimizer step (the fused dense head stages
        them into LDS with straight 16-byte copies instead of transposing)."""
        off = (self.bf16.numel() + 7) // 8 * 8
        for name, (Jt, It) in tdims.items():
            e = self.by_name[name]
            assert e.G == 1 and Jt >= e.J and It >= e.I, name
            self.bft[name] = (off, int(Jt), int(It))
            off = (off + Jt * It + 7) // 8 * 8
        grown = torch.zeros(off, dtype=torch.bfloat16, device=self.device)
        grown[:self.bf16.numel()].copy_(self.bf16)
        self.bf16 = grown
        self._build_segs()
        self.refresh_bf16()

    def bf16t_view(self, name: str) -> torch.Tensor:
        off, Jt, It = self.bft[name]
        return self.bf16[off:off + Jt * It].view(Jt, It)

    # -- construction -----------------------------------------------------
    @classmethod
    def build(cls, specs: Sequence[Tuple[str, Tuple[int, ...], Optional[float]]],
              init: Dict[str, torch.Tensor], device, pads: Optional[Dict[str, Tuple[int, int]]] = None,
              bias_names_have_no_bf16: bool = True, bf16_copies: bool = True) -> "FlatParams":
        """specs: (name, shape, wd) in creation order.  pads: name -> (I_pad, J_pad)
        for tensors that get a bf16 copy (weights; 4-D = [KH,KW,I,J], 2-D = [I,J]).
        bf16_copies=False: no bf16 copies at all (the fp32 plan reads the masters)."""
        pads = pads or {}
        entries: List[Entry] = []
        off = 0
        bf_off = 0
        l2i = 0
        for name, shape, wd in specs:
            shape = tuple(int(s) for s in shape)
            n = math.prod(shape)
            if len(shape) == 4:
                G, I, J = shape[0] * shape[1], shape[2], shape[3]
            elif len(shape) == 2:
                G, I, J = 1, shape[0], shape[1]
            else:
                G, I, J = 1, 1, shape[0]
            has_bf = bf16_copies and (len(shape) >= 2 or not bias_names_have_no_bf16)
            Ip, Jp = pads.get(name, (I, J))
            e = Entry(name, shape, wd, off, n, G, I, J, Ip, Jp, bf_off if has_bf else -1,
                      l2i if (wd is not None and len(shape) >= 2) else -1)
            if e.l2_index >= 0:
                l2i += 1
            if has_bf:
                bf_off += G * Ip * Jp
                bf_off = (bf_off + 7) // 8 * 8   # keep every copy 16-byte aligned
            entries.append(e)
            off += n
        fp = cls(entries, off, bf_off, torch.device(device))
        fp.load_state({k: v for k, v in init.items() if k in fp.by_name}, ema_too=True)
        return fp

    # -- views ------------------------------------------------------------
    def _view(self, buf: torch.Tensor, name: str) -> torch.Tensor:
        e = self.by_name[name]
        return buf[e.off:e.off + e.n].view(e.shape)

    def param_view(self, name: str) -> torch.Tensor:
        return self._view(self.params, name)

    def grad_view(self, name: str) -> torch.Tensor:
        return self._view(self.grads, name)

    def mom_view(self, name: str) -> torch.Tensor:
        return self._view(self.mom, name)

    def slot_views(self, name: str) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """(first slot, second slot or None) of one variable; which quantity each holds
        depends on the rule (``OptConfig.slot_names``)."""
        return self._view(self.mom, name), (None if self.slot2 is None else self._view(self.slot2, name))

    def init_slots(self, cfg: OptConfig) -> None:
        """Give the slots the rule's initial values, allocating the second slot buffer if the
        rule has one, the global-norm buffer if clipping is on and the per-variable norm buffer
        for lars / lamb.  The executors call this once
        at construction (before any graph capture: the captured launch holds the buffers'
        addresses)."""
        s1, s2 = cfg.slot_init()
        self.mom.fill_(s1)
        if cfg.rule in ("adam", "rmsprop", "lamb"):
            if self.slot2 is None:
                self.slot2 = torch.empty(self.total, dtype=torch.float32, device=self.device)
            self.slot2.fill_(s2)
        if cfg.clip_norm is not None and self.gnorm is None:
            nblk = 0
            if self.device.type == "cuda":
                from ..ops._ext import kernels
                nblk = int(kernels().grad_norm_max_blocks())
            self.gnorm = torch.zeros(2 + nblk, dtype=torch.float32, device=self.device)
        if cfg.layerwise and self.tnorm is None:
            n = 3 * len(self.entries)
            if self.device.type == "cuda":
                from ..ops._ext import kernels
                n = int(kernels().var_norm_buffer_size(len(self.entries)))
            self.tnorm = torch.zeros(n, dtype=torch.float32, device=self.device)

    def trust_ratios(self) -> Dict[str, Tuple[float, float, float]]:
        """name -> (parameter norm, gradient (lars) / update (lamb) norm, trust ratio) of the last
        update, for every variable (the biases' ratio is always 1)."""
        assert self.tnorm is not None, "trust ratios exist under lars / lamb only"
        t = self.tnorm[:3 * len(self.entries)].detach().cpu().tolist()
        return {e.name: (t[3 * i], t[3 * i + 1], t[3 * i + 2]) for i, e in enumerate(self.entries)}

    def trust_ratio_stats(self) -> Dict[str, float]:
        """``trust_ratio/<var>`` of the adapted variables (rank >= 2), for read_stats()."""
        tr = self.trust_ratios()
        return {f"trust_ratio/{e.name}": tr[e.name][2] for e in self.entries if len(e.shape) >= 2}

    def ema_view(self, name: str) -> torch.Tensor:
        return self._view(self.ema, name)

    def bf16_view(self, name: str) -> torch.Tensor:
        e = self.by_name[name]
        assert e.bf_off >= 0, f"{name} has no bf16 copy"
        n = e.G * e.Ip * e.Jp
        v = self.bf16[e.bf_off:e.bf_off + n]
        if len(e.shape) == 4:
            return v.view(e.shape[0], e.shape[1], e.Ip, e.Jp)
        return v.view(e.Ip, e.Jp)

    def names(self) -> List[str]:
        return [e.name for e in self.entries]

    # -- state --------------------------------------------------------------
    def load_state(self, values: Dict[str, torch.Tensor], ema_too: bool = False,
                   ema_values: Optional[Dict[str, torch.Tensor]] = None,
                   mom_values: Optional[Dict[str, torch.Tensor]] = None,
                   slot2_values: Optional[Dict[str, torch.Tensor]] = None) -> None:
        with torch.no_grad():
            for name, v in values.items():
                self.param_view(name).copy_(v.reshape(self.by_name[name].shape))
                if ema_too:
                    self.ema_view(name).copy_(v.reshape(self.by_name[name].shape))
            for name, v in (ema_values or {}).items():
                self.ema_view(name).copy_(v.reshape(self.by_name[name].shape))
            for name, v in (mom_values or {}).items():
                self.mom_view(name).copy_(v.reshape(self.by_name[name].shape))
            if slot2_values:
                assert self.slot2 is not None, "second-slot values for a rule without a second slot"
                for name, v in slot2_values.items():
                    self._view(self.slot2, name).copy_(v.reshape(self.by_name[name].shape))
        self.refresh_bf16()

    def refresh_bf16(self) -> None:
        """Rebuild the padded bf16 copies from the fp32 masters (GPU kernel)."""
        if self.device.type != "cuda":
            return
        from ..ops._ext import kernels
        K = kernels()
        for e in self.entries:
            if e.bf_off >= 0:
                K.cast_f32_bf16_padded(self.param_view(e.name).contiguous(), self.bf16[e.bf_off:], e.G, e.I, e.J,
                                       e.Ip, e.Jp)
        with torch.no_grad():
            for name in self.bft:
                e = self.by_name[name]
                self.bf16t_view(name)[:e.J, :e.I].copy_(self.param_view(name).reshape(e.I, e.J).t())

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {e.name: self.param_view(e.name).detach().cpu().clone() for e in self.entries}

    # -- K9 -------------------------------------------------------------------
    def apply(self, cfg: OptConfig, grad_scale: float = 1.0, track_l2: bool = True, fin: Optional[tuple] = None,
              perm: Optional[tuple] = None) -> None:
        """``fin``: finalize_step's arguments after ``step`` -- the step's finalize then runs
        in the same launch (HipNet.update); ``perm``: the next batch's perm_positions job
        (DeviceLoader.lookahead_job), run by extra blocks of the launch."""
        from ..ops._ext import kernels
        l2 = self.l2 if (track_l2 and self.wd_entries) else None
        sched = cfg.schedule_kwargs()    # the rate itself is computed on the device, from self.step
        clip = {}
        if cfg.clip_norm is not None:
            if self.gnorm is None:
                raise RuntimeError("clip_norm needs FlatParams.init_slots(cfg) before the first step")
            clip = {"clip_norm": cfg.clip_norm, "gnorm": self.gnorm}
        if cfg.layerwise:
            if self.tnorm is None or (cfg.rule == "lamb" and self.slot2 is None):
                raise RuntimeError(f"optimizer rule {cfg.rule!r} needs FlatParams.init_slots(cfg) before the first step")
            kernels().fused_optimizer(self.params, self.grads, self.mom, self.ema, self.bf16, self.segs, self.step,
                                      cfg.lr0, cfg.decay_rate, cfg.decay_steps, cfg.momentum, False, cfg.rule == "lars",
                                      grad_scale, cfg.ema_max, l2, fin=fin, perm=perm, rule=cfg.rule,
                                      slot2=self.slot2 if cfg.rule == "lamb" else None, beta1=cfg.beta1,
                                      beta2=cfg.beta2, epsilon=cfg.eps, lars_eta=cfg.lars_eta, tnorm=self.tnorm,
                                      **sched)
            return
        if not cfg.adaptive:
            kernels().fused_optimizer(self.params, self.grads, self.mom, self.ema, self.bf16, self.segs, self.step,
                                      cfg.lr0, cfg.decay_rate, cfg.decay_steps, cfg.momentum, cfg.nesterov,
                                      cfg.use_momentum, grad_scale, cfg.ema_max, l2, fin=fin, perm=perm, **clip,
                                      **sched)
            return
        if cfg.rule != "adagrad" and self.slot2 is None:
            raise RuntimeError(f"optimizer rule {cfg.rule!r} needs FlatParams.init_slots(cfg) before the first step")
        kernels().fused_optimizer(self.params, self.grads, self.mom, self.ema, self.bf16, self.segs, self.step,
                                  cfg.lr0, cfg.decay_rate, cfg.decay_steps, cfg.momentum, False, False,
                                  grad_scale, cfg.ema_max, l2, fin=fin, perm=perm, rule=cfg.rule, slot2=self.slot2,
                                  beta1=cfg.beta1, beta2=cfg.beta2, epsilon=cfg.epsilon,
                                  rmsprop_decay=cfg.rmsprop_decay, **clip, **sched)
