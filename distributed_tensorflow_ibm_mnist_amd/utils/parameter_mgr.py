"""Hyper-parameter manager: the in-repo replacement for DLI's ``tf_parameter_mgr``.

The reference pulls every hyper-parameter and data list from an external
IBM Spectrum Conductor module (``main.py:35,38-40``; ``mnist_input.py:10,22-23,
47,50,261``; ``inference.py:63``).  That module is not in the repository; its API
surface is inferred from the call sites.  This module exposes
the same getters, backed by a YAML/JSON config file plus programmatic
overrides:

    getMaxSteps()            -> int
    getTestInterval()        -> int
    getTrainBatchSize()      -> int
    getLearningRateDecay()   -> float   (staircase decay factor)
    getBaseLearningRate()    -> float
    getTrainData()           -> list[str]
    getTestData()            -> list[str]
    getValData()             -> list[str]
    getOptimizer(lr)         -> OptimizerSpec
    getLabelSmoothing()      -> float   (eps of the smoothed training targets; 0.0: hard labels)
    getDropout()             -> float   (drop rate of the hidden dense layers; 0.0: off)
    getDropoutSeed(default)  -> int     (seed of the dropout masks; unset: ``default``, the run's seed)
    getAugmentShift() / getAugmentRotate() / getAugmentScale() / getAugmentSeed(default)
                             -> int / float / float / int   (training-input augmentation; 0: off)
    getAugmentElasticAlpha() / getAugmentElasticSigma()
                             -> float / float   (elastic distortion: displacement scale, 0: off; smoothing sigma)
    getAugment(default_seed) -> AugmentConfig   (the six keys, checked)
    getMixupAlpha() / getCutmixAlpha() / getMixProb() / getMixSeed(default)
                             -> float / float / float / int   (mixup and CutMix of training batches; alpha 0: off)
    getMix(default_seed)     -> MixConfig   (the four keys, checked)

Defaults are the TF CIFAR-10 tutorial values that ``mnist_input.py`` mirrors
 — they are *chosen* defaults, not numbers the reference
publishes.  Data lists accept file paths / globs, ``synthetic://N`` or
``idx://<dir>`` / ``png://<dir>`` URIs (see ``data/``).

Unlike the reference (which evaluates the getters at import time,
``main.py:38-40``), values are read lazily so a ``--config`` flag parsed after
import still takes effect.
"""
from __future__ import annotations

import dataclasses
import json
import os
from typing import Any, Dict, List, Optional, Union

DEFAULTS: Dict[str, Any] = {
    "max_steps": 1000,
    "test_interval": 100,
    "batch_size": 128,
    "base_lr": 0.1,
    "lr_decay": 0.1,
    "optimizer": "sgd",          # sgd | momentum | nesterov | adam | rmsprop | adagrad | lars | lamb
    "momentum": 0.9,             # momentum | nesterov (rmsprop: 0.0 unless the config sets it)
    "beta1": 0.9,                # adam (TF1 defaults)
    "beta2": 0.999,
    "epsilon": None,             # adam 1e-8, rmsprop 1e-10, lars 0.0, lamb 1e-6
    "rmsprop_decay": 0.9,
    "adagrad_initial_accumulator": 0.1,
    "clip_norm": None,           # tf.clip_by_global_norm threshold for every rule; None: off
    "lars_eta": 0.001,           # lars: the trust coefficient
    "lr_schedule": "staircase",  # staircase | polynomial | cosine (the last two decay after the warmup)
    "warmup_steps": 0,           # linear warmup (t + 1) / warmup_steps in front of any schedule; 0: none
    "lr_total_steps": None,      # polynomial | cosine: the step at which lr_end is reached; None: max_steps
    "lr_end": 0.0,               # polynomial | cosine: the rate from lr_total_steps on
    "lr_power": 1.0,             # polynomial: the exponent
    "label_smoothing": 0.0,      # training loss against (1 - eps) * onehot + eps / classes; 0: hard labels
    "dropout": 0.0,              # drop rate on the hidden ReLU dense layers' outputs (training only); 0: off
    "dropout_seed": None,        # seed of the counter-based dropout masks; None: the run's seed
    "augment_shift": 0,          # training images: random translation of up to this many whole pixels (0..8); 0: off
    "augment_rotate": 0.0,       # ... random rotation about the centre of up to this many degrees (0..180); 0: off
    "augment_scale": 0.0,        # ... random zoom in [1 - z, 1 + z) (0..0.5); 0: off
    "augment_seed": None,        # seed of the counter-based augmentation draws; None: the run's seed
    "augment_elastic_alpha": 0.0,   # ... elastic distortion: displacement scale in pixels of the smoothed field (0..64); 0: off
    "augment_elastic_sigma": 4.0,   # ... standard deviation in pixels of the Gaussian that smooths the field (0.5..8)
    "mixup_alpha": 0.0,          # training batches: mixup with its weight from Beta(a, a) (0.1..8); 0: off
    "cutmix_alpha": 0.0,         # ... CutMix with the box area from Beta(a, a) (0.1..8); 0: off; both set: one of the two per entry
    "mix_prob": 1.0,             # ... probability that an entry is mixed at all (0..1)
    "mix_seed": None,            # seed of the counter-based mixing draws; None: the run's seed
    "distill_from": "",          # knowledge distillation: the frozen teacher's checkpoint directory; '': off
    "distill_model": "",         # ... the teacher's registry name (required with distill_from)
    "distill_alpha": None,       # ... weight of the soft part of the loss, 0..1; None: 0.5 with distill_from, else 0
    "distill_temperature": 2.0,  # ... the temperature T > 0 of both softmaxes
    "distill_use_ema": 0,        # ... 1: the teacher's ExponentialMovingAverage shadows
    "train_data": ["synthetic://60000"],
    "test_data": ["synthetic://10000?seed=1"],
    "val_data": ["synthetic://10000?seed=2"],
}

ENV_VAR = "MNISTX_PARAMS"


@dataclasses.dataclass(frozen=True)
class OptimizerSpec:
    """What ``getOptimizer(lr)`` returns: enough to build the fused K9 update."""
    name: str            # "sgd" | "momentum" | "adam" | "rmsprop" | "adagrad" | "lars" | "lamb"
    learning_rate: Any   # float, or a callable/step-schedule
    momentum: float = 0.0
    nesterov: bool = False
    beta1: float = 0.9
    beta2: float = 0.999
    epsilon: Optional[float] = None   # None: the rule's TF1 default
    rmsprop_decay: float = 0.9
    adagrad_initial_accumulator: float = 0.1
    clip_norm: Optional[float] = None   # clip the gradients by this global norm; None: off
    lars_eta: float = 0.001             # lars: trust coefficient of the layer-wise ratio
    # the learning-rate schedule (getLrSchedule): kind, warmup and the decay's end
    lr_schedule: str = "staircase"
    warmup_steps: int = 0
    lr_total_steps: int = 0             # polynomial | cosine only
    lr_end: float = 0.0
    lr_power: float = 1.0


_config: Dict[str, Any] = {}
_loaded_from: Optional[str] = None


def _load_file(path: str) -> Dict[str, Any]:
    with open(path, "r") as f:
        text = f.read()
    if path.endswith((".yaml", ".yml")):
        import yaml
        data = yaml.safe_load(text) or {}
    else:
        data = json.loads(text)
    if not isinstance(data, dict):
        raise ValueError(f"config {path} must hold a mapping")
    return data


def _as_list(v: Union[str, List[str], None]) -> List[str]:
    if v is None:
        return []
    if isinstance(v, str):
        return [s for s in (p.strip() for p in v.split(",")) if s]
    return [str(x) for x in v]


def configure(source: Union[None, str, Dict[str, Any]] = None, **overrides: Any) -> None:
    """Load a config file/dict (replaces the current one) and apply overrides."""
    global _config, _loaded_from
    cfg: Dict[str, Any] = {}
    if source is None:
        env = os.environ.get(ENV_VAR)
        if env:
            cfg.update(_load_file(env))
            _loaded_from = env
    elif isinstance(source, str):
        cfg.update(_load_file(source))
        _loaded_from = source
    else:
        cfg.update(source)
        _loaded_from = "<dict>"
    for k, v in overrides.items():
        if v is not None:
            cfg[k] = v
    unknown = set(cfg) - set(DEFAULTS) - {"model", "in_channels", "seed", "weight_decay",
                                          "moving_average_decay", "num_epochs_per_decay",
                                          "examples_per_epoch"}
    if unknown:
        raise ValueError(f"unknown parameter(s) in config: {sorted(unknown)}")
    _config = cfg


FLAG_KEYS = ("max_steps", "test_interval", "batch_size", "base_lr", "lr_decay", "optimizer", "momentum",
             "train_data", "test_data", "val_data", "beta1", "beta2", "epsilon", "rmsprop_decay",
             "adagrad_initial_accumulator", "clip_norm", "lars_eta", "lr_schedule", "warmup_steps",
             "lr_total_steps", "lr_end", "lr_power", "label_smoothing", "dropout", "dropout_seed",
             "augment_shift", "augment_rotate", "augment_scale", "augment_seed", "augment_elastic_alpha",
             "augment_elastic_sigma", "mixup_alpha", "cutmix_alpha", "mix_prob", "mix_seed", "distill_from",
             "distill_model", "distill_alpha", "distill_temperature", "distill_use_ema")
ADAPTIVE_OPTIMIZERS = ("adam", "rmsprop", "adagrad")
LAYERWISE_OPTIMIZERS = ("lars", "lamb")   # layer-wise trust ratios on top of momentum / Adam


def configure_from_flags(FLAGS) -> None:
    """``--config`` (or ``MNISTX_PARAMS``) plus the override flags that are set ('' and -1: unset)."""
    configure(getattr(FLAGS, "config", "") or None,
              **{k: v for k, v in ((k, getattr(FLAGS, k, None)) for k in FLAG_KEYS) if v not in (None, "", -1)})


def check_ps_optimizer(job_name: str, log=print) -> None:
    """Parameter-server mode moves exactly one slot buffer between workers and servers, so the
    adaptive rules are not available there, and the servers' update code takes no per-variable
    norms, so neither are the layer-wise rules: a PS or worker task exits at start-up."""
    name = str(get("optimizer")).lower()
    if job_name in ("ps", "worker") and name in ADAPTIVE_OPTIMIZERS + LAYERWISE_OPTIMIZERS:
        others = ADAPTIVE_OPTIMIZERS + (LAYERWISE_OPTIMIZERS if name in LAYERWISE_OPTIMIZERS else ())
        log(f"optimizer {name!r} is not supported in parameter-server mode (--job_name={job_name}): use "
            f"sgd|momentum|nesterov there; {'|'.join(others)} run single-process and data-parallel")
        raise SystemExit(2)


def getClipNorm() -> Optional[float]:
    """The ``clip_norm`` key: None (off) or a finite threshold > 0."""
    c = get("clip_norm")
    if c is None:
        return None
    c = float(c)
    if not (c > 0 and c != float("inf")):
        raise ValueError(f"clip_norm must be finite and > 0, got {c}")
    return c


def check_ps_clip_norm(job_name: str, log=print) -> None:
    """The parameter servers apply the update themselves (the native shm loop has its own update
    code) and none of them clips: a PS or worker task with ``clip_norm`` set exits at start-up."""
    if job_name in ("ps", "worker") and get("clip_norm") is not None:
        log(f"clip_norm is not supported in parameter-server mode (--job_name={job_name}): the servers apply "
            f"the update unclipped; gradient clipping runs single-process and data-parallel")
        raise SystemExit(2)


LR_SCHEDULES = ("staircase", "polynomial", "cosine")


def _as_int(key: str, v: Any) -> int:
    """An integer key: 3 and 3.0 pass, 3.5, True and "x" do not."""
    try:
        if isinstance(v, bool) or int(v) != float(v):
            raise ValueError
        return int(v)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{key} must be an integer, got {v!r}") from None


def getLrSchedule() -> str:
    """The ``lr_schedule`` key: staircase | polynomial | cosine, case-insensitive."""
    name = str(get("lr_schedule")).lower()
    if name not in LR_SCHEDULES:
        raise ValueError(f"lr_schedule must be one of {'|'.join(LR_SCHEDULES)}, got {get('lr_schedule')!r}")
    return name


def getWarmupSteps() -> int:
    """The ``warmup_steps`` key: an integer >= 0 (0: no warmup)."""
    w = _as_int("warmup_steps", get("warmup_steps"))
    if w < 0:
        raise ValueError(f"warmup_steps must be >= 0, got {w}")
    return w


def getLrTotalSteps() -> int:
    """The ``lr_total_steps`` key (default ``max_steps``): an integer > ``warmup_steps``.  Only
    polynomial and cosine read it."""
    t = get("lr_total_steps")
    t = getMaxSteps() if t is None else _as_int("lr_total_steps", t)
    w = getWarmupSteps()
    if t <= w:
        raise ValueError(f"lr_total_steps must be > warmup_steps ({w}), got {t}")
    return t


def getLrEnd() -> float:
    """The ``lr_end`` key: finite and >= 0."""
    e = float(get("lr_end"))
    if not (e >= 0 and e != float("inf")):
        raise ValueError(f"lr_end must be finite and >= 0, got {e}")
    return e


def getLrPower() -> float:
    """The ``lr_power`` key (polynomial): finite and > 0."""
    p = float(get("lr_power"))
    if not (p > 0 and p != float("inf")):
        raise ValueError(f"lr_power must be finite and > 0, got {p}")
    return p


def getLabelSmoothing() -> float:
    """The ``label_smoothing`` key: finite, 0 <= eps < 1.  It shapes the training loss only (the
    workers compute it, so parameter-server mode takes it as it is) and is no optimizer state."""
    v = get("label_smoothing")
    try:
        if isinstance(v, bool):
            raise ValueError
        eps = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"label_smoothing must be a number with 0 <= label_smoothing < 1, got {v!r}") from None
    if not 0 <= eps < 1:       # NaN fails both comparisons
        raise ValueError(f"label_smoothing must be finite with 0 <= label_smoothing < 1, got {eps}")
    return eps


def getDropout() -> float:
    """The ``dropout`` key: the drop rate (as ``torch.nn.Dropout``), finite with 0 <= p < 1."""
    from ..ops.dropout import check_rate
    return check_rate(get("dropout"), "dropout")


def getDropoutSeed(default: int = 0) -> int:
    """The ``dropout_seed`` key: an integer with 0 <= seed < 2^63; unset: ``default`` (the run's seed)."""
    from ..ops.dropout import check_seed
    v = get("dropout_seed")
    return check_seed(default if v is None else v, "dropout_seed")


def getAugmentShift() -> int:
    """The ``augment_shift`` key: an integer with 0 <= S <= 8, the largest translation in pixels."""
    from ..data.augment import check_shift
    return check_shift(get("augment_shift"), "augment_shift")


def getAugmentRotate() -> float:
    """The ``augment_rotate`` key: finite with 0 <= R <= 180, the largest rotation in degrees."""
    from ..data.augment import check_rotate
    return check_rotate(get("augment_rotate"), "augment_rotate")


def getAugmentScale() -> float:
    """The ``augment_scale`` key: finite with 0 <= Z <= 0.5, the zoom is drawn from [1 - Z, 1 + Z)."""
    from ..data.augment import check_scale
    return check_scale(get("augment_scale"), "augment_scale")


def getAugmentSeed(default: int = 0) -> int:
    """The ``augment_seed`` key: an integer with 0 <= seed < 2^63; unset: ``default`` (the run's seed)."""
    from ..ops.dropout import check_seed
    v = get("augment_seed")
    return check_seed(default if v is None else v, "augment_seed")


def getAugmentElasticAlpha() -> float:
    """The ``augment_elastic_alpha`` key: finite with 0 <= alpha <= 64, the displacement scale in pixels
    of the smoothed random field (0: no elastic distortion)."""
    from ..data.augment import check_elastic_alpha
    return check_elastic_alpha(get("augment_elastic_alpha"), "augment_elastic_alpha")


def getAugmentElasticSigma() -> float:
    """The ``augment_elastic_sigma`` key: finite with 0.5 <= sigma <= 8, the standard deviation in pixels
    of the smoothing Gaussian (always checked, read only when alpha > 0)."""
    from ..data.augment import check_elastic_sigma
    return check_elastic_sigma(get("augment_elastic_sigma"), "augment_elastic_sigma")


def getAugment(default_seed: int = 0):
    """The six augmentation keys as a ``data.augment.AugmentConfig`` (its ``enabled`` says whether any
    amount is non-zero).  The workers augment their own inputs and the servers never see inputs, so
    parameter-server mode takes the keys as they are."""
    from ..data.augment import AugmentConfig
    return AugmentConfig(getAugmentShift(), getAugmentRotate(), getAugmentScale(), getAugmentSeed(default_seed),
                         getAugmentElasticAlpha(), getAugmentElasticSigma())


def getMixupAlpha() -> float:
    """The ``mixup_alpha`` key: 0 (off), or finite with 0.1 <= alpha <= 8, Beta(alpha, alpha) of the weight."""
    from ..data.mix import check_alpha
    return check_alpha(get("mixup_alpha"), "mixup_alpha")


def getCutmixAlpha() -> float:
    """The ``cutmix_alpha`` key: 0 (off), or finite with 0.1 <= alpha <= 8, Beta(alpha, alpha) behind the box."""
    from ..data.mix import check_alpha
    return check_alpha(get("cutmix_alpha"), "cutmix_alpha")


def getMixProb() -> float:
    """The ``mix_prob`` key: finite with 0 <= p <= 1, the probability that an entry is mixed at all."""
    from ..data.mix import check_prob
    return check_prob(get("mix_prob"), "mix_prob")


def getMixSeed(default: int = 0) -> int:
    """The ``mix_seed`` key: an integer with 0 <= seed < 2^63; unset: ``default`` (the run's seed)."""
    from ..ops.dropout import check_seed
    v = get("mix_seed")
    return check_seed(default if v is None else v, "mix_seed")


def getMix(default_seed: int = 0):
    """The four mixing keys as a ``data.mix.MixConfig`` (its ``enabled`` says whether anything is mixed).
    The workers own their loader and their loss, so parameter-server mode takes the keys as they are."""
    from ..data.mix import MixConfig
    return MixConfig(getMixupAlpha(), getCutmixAlpha(), getMixProb(), getMixSeed(default_seed))


@dataclasses.dataclass(frozen=True)
class DistillSpec:
    """What ``getDistill()`` returns; ``enabled``: a teacher is loaded and the loss reads its logits."""
    ckpt_dir: str
    model: str
    alpha: float
    temperature: float
    use_ema: bool

    @property
    def enabled(self) -> bool:
        return bool(self.ckpt_dir) and self.alpha > 0


def getDistill() -> DistillSpec:
    """The five distillation keys.  ``distill_from`` '' is off (the other keys are still checked);
    ``distill_alpha`` unset is 0.5 with a teacher.  The workers own their loss and each loads the
    teacher itself, so data-parallel and parameter-server mode take the keys as they are.  Together
    with label_smoothing, mixup / CutMix or dropout it is refused (the fused head has no such form)."""
    from ..runtime.params import check_distill
    src, model = get("distill_from"), get("distill_model")
    for key, v in (("distill_from", src), ("distill_model", model)):
        if v is not None and not isinstance(v, str):
            raise ValueError(f"{key} must be a string, got {v!r}")
    src, model = src or "", model or ""
    a = get("distill_alpha")
    alpha, T = check_distill((0.5 if src else 0.0) if a is None else a, get("distill_temperature"))
    ema = get("distill_use_ema")
    if isinstance(ema, str) or ema not in (0, 1, False, True):
        raise ValueError(f"distill_use_ema must be 0 or 1, got {ema!r}")
    if src and not model:
        raise ValueError(f"distill_model is required with distill_from ({src!r})")
    if model and not src:
        raise ValueError(f"distill_model ({model!r}) needs distill_from")
    if alpha > 0 and not src:
        raise ValueError(f"distill_alpha ({alpha}) needs distill_from")
    spec = DistillSpec(src, model, alpha, T, bool(ema))
    if spec.enabled:
        for key, on in (("label_smoothing", getLabelSmoothing() > 0), ("mixup_alpha", getMixupAlpha() > 0),
                        ("cutmix_alpha", getCutmixAlpha() > 0), ("dropout", getDropout() > 0)):
            if on:
                raise ValueError(f"distill_from ({src!r}) cannot be combined with {key} ({get(key)})")
    return spec


def check_ps_dropout(job_name: str, log=print) -> None:
    """The dropout masks are drawn from the device-side global step, and a parameter-server worker's
    device step is not the global step: a PS or worker task with ``dropout`` > 0 exits at start-up."""
    if job_name in ("ps", "worker") and getDropout() > 0:
        log(f"dropout is not supported in parameter-server mode (--job_name={job_name}): the masks follow the "
            f"device-side global step, which a worker does not hold; dropout runs single-process and data-parallel")
        raise SystemExit(2)


def check_ps_lr_schedule(job_name: str, log=print) -> None:
    """The parameter servers' update code knows the staircase alone: a PS or worker task with another
    ``lr_schedule`` or a warmup exits at start-up."""
    if job_name not in ("ps", "worker"):
        return
    name, w = getLrSchedule(), getWarmupSteps()
    if name != "staircase" or w > 0:
        what = f"lr_schedule {name!r}" if name != "staircase" else f"warmup_steps {w}"
        log(f"{what} is not supported in parameter-server mode (--job_name={job_name}): the servers apply the "
            f"staircase rate; warmup and the polynomial / cosine schedules run single-process and data-parallel")
        raise SystemExit(2)


def set_param(key: str, value: Any) -> None:
    _config[key] = value


def get(key: str, default: Any = None) -> Any:
    if key in _config:
        return _config[key]
    if key in DEFAULTS:
        return DEFAULTS[key]
    return default


def snapshot() -> Dict[str, Any]:
    out = dict(DEFAULTS)
    out.update(_config)
    return out


# --- the DLI getter surface --------------------------------
def getMaxSteps() -> int:
    return int(get("max_steps"))


def getTestInterval() -> int:
    return int(get("test_interval"))


def getTrainBatchSize() -> int:
    return int(get("batch_size"))


def getLearningRateDecay() -> float:
    return float(get("lr_decay"))


def getBaseLearningRate() -> float:
    return float(get("base_lr"))


def getTrainData() -> List[str]:
    return _as_list(get("train_data"))


def getTestData() -> List[str]:
    return _as_list(get("test_data"))


def getValData() -> List[str]:
    return _as_list(get("val_data"))


def getOptimizer(lr: Any) -> OptimizerSpec:
    """Config-driven optimizer choice (``mnist_input.py:261``), with the ``clip_norm`` key."""
    spec, clip = _optimizer_rule(lr), getClipNorm()
    if clip is not None and spec.name in LAYERWISE_OPTIMIZERS:
        raise ValueError(f"optimizer {spec.name!r} cannot be combined with clip_norm: the layer-wise trust ratio "
                         f"already rescales every variable's update")
    kind = getLrSchedule()
    # lr_total_steps and lr_power are only read by the schedules that use them
    total = getLrTotalSteps() if kind != "staircase" else 0
    power = getLrPower() if kind == "polynomial" else 1.0
    return dataclasses.replace(spec, clip_norm=clip, lr_schedule=kind, warmup_steps=getWarmupSteps(),
                               lr_total_steps=total, lr_end=getLrEnd(), lr_power=power)


def getLarsEta() -> float:
    """The ``lars_eta`` key (LARS trust coefficient): finite and > 0."""
    eta = float(get("lars_eta"))
    if not (eta > 0 and eta != float("inf")):
        raise ValueError(f"lars_eta must be finite and > 0, got {eta}")
    return eta


def _optimizer_rule(lr: Any) -> OptimizerSpec:
    name = str(get("optimizer")).lower()
    mom = float(get("momentum"))
    if name in ("sgd", "gradientdescent", "gradient_descent"):
        return OptimizerSpec("sgd", lr, 0.0, False)
    if name == "momentum":
        return OptimizerSpec("momentum", lr, mom, False)
    if name == "nesterov":
        return OptimizerSpec("momentum", lr, mom, True)
    eps = get("epsilon")
    eps = None if eps is None else float(eps)
    if name == "adam":
        return OptimizerSpec("adam", lr, beta1=float(get("beta1")), beta2=float(get("beta2")), epsilon=eps)
    if name == "rmsprop":
        # TF1's RMSProp momentum defaults to 0.0: only a momentum the config itself sets applies,
        # never the manager's general default
        return OptimizerSpec("rmsprop", lr, momentum=float(_config["momentum"]) if "momentum" in _config else 0.0,
                             epsilon=eps, rmsprop_decay=float(get("rmsprop_decay")))
    if name == "adagrad":
        acc0 = float(get("adagrad_initial_accumulator"))
        if not acc0 > 0:
            raise ValueError(f"adagrad_initial_accumulator must be > 0, got {acc0}")
        return OptimizerSpec("adagrad", lr, adagrad_initial_accumulator=acc0)
    if name == "lars":     # momentum with a layer-wise trust ratio (epsilon: 0.0 unless set)
        return OptimizerSpec("lars", lr, mom, False, epsilon=eps, lars_eta=getLarsEta())
    if name == "lamb":     # Adam with a layer-wise trust ratio (epsilon: 1e-6 unless set)
        return OptimizerSpec("lamb", lr, beta1=float(get("beta1")), beta2=float(get("beta2")), epsilon=eps)
    raise ValueError(f"unsupported optimizer {name!r} (sgd|momentum|nesterov|adam|rmsprop|adagrad|lars|lamb)")


configure()
