"""Knowledge distillation under hipGraph capture: a ``Replica`` with a frozen teacher and shift augmentation,
five captured steps against five eager steps bit for bit (item 9 of tests/test_distill_gpu.py, whose helpers
it loads by path).

A file of its own that sorts after every other GPU test file.  Each captured step takes one more stream
out of the process's stream pool, and the hardware queue that a later test's side stream lands on follows
from how many were taken before it: tests/test_dp_coresidency_gpu.py measures whether a probe on a fresh
side stream starts beside a running kernel, and with these two captures collected in front of it its
probe queued behind the kernel instead.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
from distributed_tensorflow_ibm_mnist_amd.runtime.teacher import Teacher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("test_distill_gpu", os.path.join(ROOT, "tests", "test_distill_gpu.py"))
dg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dg)
_opt = dg._opt

pytestmark = pytest.mark.gpu


def _replica(dev, model, tmodel, graph, lines, shift=2):
    from distributed_tensorflow_ibm_mnist_amd.data.augment import AugmentConfig
    from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica
    spec, tspec = get_model(model, 1), get_model(tmodel, 1)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.integers(0, 256, (192, 784), dtype=np.uint8))
    y = torch.arange(192) % 10
    tinit = torch_ref.init_params(tspec, seed=3)
    tinit["softmax_linear/weights"] = tinit["softmax_linear/weights"] * 4.0
    opt = OptConfig(lr0=0.01, decay_steps=0, use_momentum=True, momentum=0.9, ema_max=0.9999, distill_alpha=0.5,
                    distill_temperature=2.0)
    return Replica(spec, "hip", 64, dev, torch_ref.init_params(spec, seed=0), opt, x, y, 1, x[:100], y[:100], seed=5,
                   use_graph=graph, fused_input="bf16", augment=AugmentConfig(shift=shift, seed=8), log=lines.append,
                   teacher=lambda net, impl, prec: Teacher(tspec, tinit, net, impl, prec))


@pytest.mark.parametrize("model,tmodel", [("lenet5", "reference_cnn"), ("reference_cnn", "lenet5")])
def test_graph_replay_is_bitwise_the_eager_run(dev, K, model, tmodel):
    """Five steps with the loader (shift augmentation) feeding each: one eager warm-up plus four replays
    against five eager steps.  The teacher's forward is part of the captured body."""
    la, lb = [], []
    eager, graph = _replica(dev, model, tmodel, False, la), _replica(dev, model, tmodel, True, lb)
    for lines in (la, lb):      # the augmentation has switched the input mode already: its line, not a second one
        assert sum("'prep'" in ln for ln in lines) == 1
        assert sum(ln.startswith("distillation teacher " + tmodel) and "test accuracy" in ln for ln in lines) == 1
    assert graph.net.idx_buf is None
    lc = []
    assert _replica(dev, model, tmodel, True, lc, shift=0).net.idx_buf is None      # without augmentation: the teacher's line
    assert sum("distillation is on" in ln and "'prep'" in ln for ln in lc) == 1
    for _ in range(5):
        eager.step()
        graph.step()
    torch.cuda.synchronize()
    assert graph._graph is not None and eager._graph is None
    for name in ("x0", "labels", "stats", "teacher_logits", "loss_ema"):
        assert torch.equal(getattr(eager.net, name), getattr(graph.net, name)), name
    for name in ("params", "mom", "ema", "step"):
        assert torch.equal(getattr(eager.net.fp, name), getattr(graph.net.fp, name)), name
    assert int(graph.net.fp.step.item()) == 5 and graph.net.read_stats()["nan"] == 0.0
    assert torch.equal(eager.teacher.net.fp.params, graph.teacher.net.fp.params)
    assert graph.evaluate() == eager.evaluate()
    from distributed_tensorflow_ibm_mnist_amd.train.replica import Replica
    spec = get_model("mlp", 1)
    x, y = torch.zeros(64, 784, dtype=torch.uint8), torch.zeros(64, dtype=torch.int64)
    with pytest.raises(ValueError, match="distill_alpha"):
        Replica(spec, "hip", 64, dev, torch_ref.init_params(spec, seed=0), _opt(0.5, 2.0), x, y, 1, use_graph=False)
