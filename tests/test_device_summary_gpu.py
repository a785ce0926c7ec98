"""summary_stats (csrc/kernels/summary.hip) against the numpy oracle (tests/summary_oracle.py), and
the Monitor's device path against its host path, on the GPU.  Counts compare with array_equal, min
and max with ==, sums exactly where the arithmetic is exact and within the derived float64
summation bound (summary_oracle.sum_bounds) elsewhere."""
import importlib.util
import os
import struct

import numpy as np
import pytest
import torch

from distributed_tensorflow_ibm_mnist_amd.obs.events import BUCKET_LIMITS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("summary_oracle", os.path.join(ROOT, "tests", "summary_oracle.py"))
oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(oracle)

pytestmark = pytest.mark.gpu
NB = len(BUCKET_LIMITS)
SPECIALS = np.array([np.nan, np.inf, -np.inf], np.float32)


@pytest.fixture(scope="module")
def limits(dev):
    return torch.from_numpy(BUCKET_LIMITS).to(dev)


def to_dev(v32, dev, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(v32, dtype=np.float32))
    if bf16:
        t = t.to(torch.bfloat16)
        assert np.array_equal(t.float().numpy(), v32, equal_nan=True)      # the values are bf16 already
    return t.to(dev)


def run(K, src, segs, lim, divisor=1.0, fill=7):
    """Every output and the scratch start as 7: stale contents must not survive."""
    nseg, nb = len(segs), lim.numel()
    counts = torch.full((nseg, nb + 1), fill, dtype=torch.int32, device=src.device)
    stats = torch.full((nseg, 4), float(fill), dtype=torch.float64, device=src.device)
    scratch = torch.full((int(K.summary_scratch_size(nseg)),), float(fill), dtype=torch.float64, device=src.device)
    K.summary_stats(src, torch.tensor(segs, dtype=torch.int64).view(nseg, 4), lim, counts, stats, scratch,
                    divisor=divisor)
    return counts.cpu().numpy(), stats.cpu().numpy()


def compare(got, ref, bounds=None):
    (gc, gs), (rc, rs) = got, ref
    assert np.array_equal(gc, rc), np.argwhere(gc != rc)[:8]
    assert (gs[:, 0] == rs[:, 0]).all() and (gs[:, 1] == rs[:, 1]).all(), (gs[:, :2], rs[:, :2])
    for s in range(len(rs)):
        for k, what in ((2, "sum"), (3, "sumsq")):
            tol = 0.0 if bounds is None else bounds[s, k - 2]
            err = abs(gs[s, k] - rs[s, k])
            print(f"segment {s} {what}: got {gs[s, k]!r} ref {rs[s, k]!r} |diff| {err:.3e} allowed {tol:.3e}")
            assert err <= tol, (s, what)


# ------------------------------------------------------------------ every boundary
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_every_boundary(dev, K, limits, kind):
    vals, want = oracle.boundary_set(kind)
    v = np.concatenate([vals, SPECIALS])
    segs = [(0, 1, v.size, v.size)]
    got = run(K, to_dev(v, dev, kind == "bf16"), segs, limits)
    assert got[0][0, NB] == 3
    assert np.array_equal(got[0][0, :NB], np.bincount(want, minlength=NB))
    compare(got, oracle.reference(v, segs, BUCKET_LIMITS), oracle.sum_bounds(v, segs, BUCKET_LIMITS))


# ------------------------------------------------------------------ segment and chunk edges
EDGE_SIZES = [1, 6, 150, 511, 512, 513, 1025, 2400]


def edge_layout(rng, gap=3, first=5):
    segs, off = [], first
    for n in EDGE_SIZES:
        segs.append((off, 1, n, n))
        off += n + gap
    v = np.full(off, 1e30, np.float32)
    for o, _, n, _ in segs:
        v[o:o + n] = rng.standard_normal(n).astype(np.float32) * 0.1
    return v, segs


def test_segment_and_chunk_edges(dev, K, limits):
    v, segs = edge_layout(np.random.default_rng(11))
    got = run(K, to_dev(v, dev), segs, limits)
    ref = oracle.reference(v, segs, BUCKET_LIMITS)
    assert (got[0].sum(axis=1) == EDGE_SIZES).all()            # nothing of the 1e30 gaps, nothing stale
    assert got[1][:, 1].max() < 1.0
    compare(got, ref, oracle.sum_bounds(v, segs, BUCKET_LIMITS))


def test_more_segments_than_one_launch_takes(dev, K, limits):
    """70 segments (a launch carries a table of 32), one of them empty."""
    rng = np.random.default_rng(12)
    v = rng.standard_normal(70 * 40).astype(np.float32)
    segs = [(40 * i, 1, 0 if i == 33 else 1 + (i * 7) % 40, 40) for i in range(70)]
    got = run(K, to_dev(v, dev), segs, limits)
    assert list(got[1][33]) == [np.inf, -np.inf, 0.0, 0.0] and got[0][33].sum() == 0
    compare(got, oracle.reference(v, segs, BUCKET_LIMITS), oracle.sum_bounds(v, segs, BUCKET_LIMITS))


def test_second_grid_stride_trip(dev, K, limits):
    """2 * 512 * summary_max_blocks() + 777 elements: every block walks several chunks and the
    last one's range is ragged and ends in a partial chunk."""
    nb = int(K.summary_max_blocks())
    assert 1 <= nb <= 4096
    n = 2 * 512 * nb + 777
    v = np.random.default_rng(13).standard_normal(n).astype(np.float32)
    segs = [(0, 1, n, n)]
    got = run(K, to_dev(v, dev), segs, limits)
    compare(got, oracle.reference(v, segs, BUCKET_LIMITS), oracle.sum_bounds(v, segs, BUCKET_LIMITS))


# ------------------------------------------------------------------ channel padding
@pytest.mark.parametrize("bf16", [False, True])
def test_padding_is_neither_read_nor_counted(dev, K, limits, bf16):
    rng = np.random.default_rng(14)
    rows, pairs = 37, [(6, 8), (6, 16), (6, 32), (16, 16), (16, 32), (32, 32)]
    segs, off, parts = [], 3, [np.full(3, 1e30, np.float32)]
    for cols, stride in pairs:
        a = np.full((rows, stride), 1e30, np.float32)
        a[:, :cols] = rng.standard_normal((rows, cols)).astype(np.float32)
        parts.append(a.reshape(-1))
        segs.append((off, rows, cols, stride))
        off += rows * stride
    v = np.concatenate(parts)
    if bf16:
        v = torch.from_numpy(v).to(torch.bfloat16).float().numpy()
    got = run(K, to_dev(v, dev, bf16), segs, limits)
    assert (got[0].sum(axis=1) == [rows * c for c, _ in pairs]).all() and got[1][:, 1].max() < 10.0
    compare(got, oracle.reference(v, segs, BUCKET_LIMITS), oracle.sum_bounds(v, segs, BUCKET_LIMITS))


# ------------------------------------------------------------------ divisor
@pytest.mark.parametrize("divisor", [2, 3, 7])
def test_divisor_is_numpy_float32_division(dev, K, limits, divisor):
    vals, _ = oracle.boundary_set("fp32")
    rng = np.random.default_rng(15 + divisor)
    # the boundary values and their multiples by the divisor (whose quotients land on the
    # boundaries again, off by the rounding), plus normals: one wrong rounding moves a count
    with np.errstate(over="ignore"):
        v = np.concatenate([vals, vals * np.float32(divisor), rng.standard_normal(3000).astype(np.float32), SPECIALS])
    segs = [(0, 1, v.size, v.size)]
    got = run(K, to_dev(v, dev), segs, limits, divisor=float(divisor))
    ref = oracle.reference(v, segs, BUCKET_LIMITS, divisor)
    assert ref[0][0, NB] >= 3
    compare(got, ref, oracle.sum_bounds(v, segs, BUCKET_LIMITS, divisor))


def test_divisor_one_leaves_denormals_and_nan_payloads_alone(dev, K, limits):
    den = np.array([1e-45, -1e-45, 1e-40, -1.1754942e-38, 3e-39], np.float32)
    nan = np.zeros(2, np.float32)
    nan.view(np.uint32)[:] = [0x7fc12345, 0xffa00001]
    v = np.concatenate([den, nan])
    segs = [(0, 1, 5, 5), (0, 1, 7, 7)]
    got = run(K, to_dev(v, dev), segs, limits)
    ref = oracle.reference(v, segs, BUCKET_LIMITS)
    assert got[1][0, 0] == float(np.float32(-1.1754942e-38)) and got[1][0, 1] == float(np.float32(3e-39))
    assert got[0][1, NB] == 2
    compare(got, ref)      # five denormals: their float64 sums are exact


# ------------------------------------------------------------------ sums
def test_exact_sums(dev, K, limits):
    """Small integers times a power of two: every partial sum is exact in float64 in any order."""
    rng = np.random.default_rng(16)
    v = (rng.integers(-1000, 1001, size=5000) * 2.0 ** -7).astype(np.float32)
    segs = [(0, 1, 5000, 5000), (100, 50, 30, 64)]
    compare(run(K, to_dev(v, dev), segs, limits), oracle.reference(v, segs, BUCKET_LIMITS))


def test_general_sums_within_the_summation_bound(dev, K, limits):
    rng = np.random.default_rng(17)
    n = 40000
    v = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, size=n)).astype(np.float32)
    segs = [(0, 1, n, n), (1, 1, 777, 777)]
    compare(run(K, to_dev(v, dev), segs, limits), oracle.reference(v, segs, BUCKET_LIMITS),
            oracle.sum_bounds(v, segs, BUCKET_LIMITS))


def test_two_calls_are_bitwise_equal(dev, K, limits):
    v, segs = edge_layout(np.random.default_rng(18))
    n = 300000
    v = np.concatenate([v, np.random.default_rng(19).standard_normal(n).astype(np.float32)])
    segs = segs + [(v.size - n, 1, n, n)]
    src = to_dev(v, dev)
    a = run(K, src, segs, limits, divisor=3.0, fill=7)
    b = run(K, src, segs, limits, divisor=3.0, fill=-3)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_an_arbitrary_table(dev, K):
    """Not TF's: 5 limits, several thousand values per bucket, values on the limits themselves."""
    lim = np.array([-2.5, -1.0, 0.25, 0.5, 3.0])
    v = np.concatenate([np.random.default_rng(20).standard_normal(9000).astype(np.float32) * 2,
                        lim.astype(np.float32), np.array([4.0, -0.0, 0.0], np.float32)])
    segs = [(0, 1, v.size, v.size)]
    got = run(K, to_dev(v, dev), segs, torch.from_numpy(lim).to(dev))
    assert got[0][0, 5] > 0
    compare(got, oracle.reference(v, segs, lim), oracle.sum_bounds(v, segs, lim))


# ------------------------------------------------------------------ the binding refuses
def test_binding_refusals(dev, K, limits):
    src = torch.zeros(1000, device=dev)
    counts = torch.zeros(2, NB + 1, dtype=torch.int32, device=dev)
    stats = torch.zeros(2, 4, dtype=torch.float64, device=dev)
    scratch = torch.zeros(int(K.summary_scratch_size(2)), dtype=torch.float64, device=dev)

    def call(src=src, segs=((0, 1, 10, 10), (10, 5, 6, 8)), lim=limits, counts=counts, stats=stats, scratch=scratch,
             divisor=1.0):
        K.summary_stats(src, torch.tensor(segs, dtype=torch.int64), lim, counts, stats, scratch, divisor=divisor)

    call()
    with pytest.raises(ValueError, match="past src"):
        call(segs=((0, 1, 10, 10), (963, 5, 6, 8)))          # last element 963 + 4 * 8 + 5 = 1000
    with pytest.raises(ValueError, match="past src"):
        call(segs=((995, 1, 6, 6), (0, 1, 1, 1)))
    with pytest.raises(ValueError, match="row_stride"):
        call(segs=((0, 5, 9, 8), (0, 1, 1, 1)))
    with pytest.raises(ValueError, match="ascending"):
        call(lim=torch.from_numpy(BUCKET_LIMITS[::-1].copy()).to(dev))
    with pytest.raises(ValueError, match="NB"):
        call(lim=torch.arange(2049, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        call(src=src.to(torch.float16))
    with pytest.raises(ValueError, match="limits"):
        call(lim=limits.float())
    with pytest.raises(ValueError, match="counts"):
        call(counts=counts.to(torch.int64))
    with pytest.raises(ValueError, match="scratch"):
        call(scratch=scratch[:-1])
    with pytest.raises(ValueError, match="2\\^31"):
        call(segs=((0, 1 << 16, 1 << 15, 1 << 15), (0, 1, 1, 1)))
    with pytest.raises(ValueError, match="divisor"):
        call(divisor=0.0)
    torch.cuda.synchronize()
    assert int(counts.sum()) == 40                             # only the first call ran


# ------------------------------------------------------------------ the Monitor, end to end
class StubReplica:
    def __init__(self, net, spec, world):
        self.net, self.spec, self.world = net, spec, world

    def read_stats(self):
        return self.net.read_stats()


def decode(logdir):
    """[(tag, float | histogram dict)] of the one summary event, in file order."""
    from distributed_tensorflow_ibm_mnist_amd.obs.events import find_event_files
    from distributed_tensorflow_ibm_mnist_amd.ops._ext import host
    from distributed_tensorflow_ibm_mnist_amd.utils import proto
    out = []
    for path in find_event_files(logdir):
        for rec in host().tfrecord_read(path, True):
            d = proto.to_dict(rec)
            if 5 not in d:
                continue
            for f, _, val in proto.fields(d[5][0]):
                if f != 1:
                    continue
                vd = proto.to_dict(val)
                tag = vd[1][0].decode()
                if 2 in vd:
                    out.append((tag, struct.unpack("<f", vd[2][0])[0]))
                else:
                    h = proto.to_dict(vd[5][0])
                    dbl = lambda k: struct.unpack("<d", h[k][0])[0]  # noqa: E731
                    out.append((tag, {"min": dbl(1), "max": dbl(2), "num": dbl(3), "sum": dbl(4), "sum_squares": dbl(5),
                                      "bucket_limit": np.frombuffer(h[6][0], dtype="<f8"),
                                      "bucket": np.frombuffer(h[7][0], dtype="<f8")}))
    return out


@pytest.mark.parametrize("model,f32,world", [("lenet5", False, 1), ("reference_cnn", False, 1), ("lenet5", False, 3),
                                             ("lenet5", True, 1)])
def test_monitor_device_path_writes_what_the_host_path_writes(dev, K, tmp_path, model, f32, world):
    from distributed_tensorflow_ibm_mnist_amd.models import get_model, torch_ref
    from distributed_tensorflow_ibm_mnist_amd.obs.monitor import Monitor
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor import HipNet
    from distributed_tensorflow_ibm_mnist_amd.runtime.executor_f32 import HipNetF32
    from distributed_tensorflow_ibm_mnist_amd.runtime.params import OptConfig
    B = 32
    spec = get_model(model, 1)
    net = (HipNetF32 if f32 else HipNet)(spec, B, dev, torch_ref.init_params(spec, seed=21),
                                         OptConfig(lr0=0.05, use_momentum=True, momentum=0.9))
    g = torch.Generator(device=dev).manual_seed(21)
    x = torch.rand(B, 28, 28, 1, device=dev, generator=g) - 0.5
    net.x0.copy_(x if f32 else x.to(torch.bfloat16))
    net.labels.copy_(torch.randint(0, 10, (B,), device=dev, generator=g, dtype=torch.int32))
    net.train_step()
    torch.cuda.synchronize()
    rep = StubReplica(net, spec, world)
    mons = {}
    for flag in (False, True):
        m = Monitor(str(tmp_path / f"dev{int(flag)}"), 1, 1, rep, device_summaries=flag)
        m.register_reference_summaries()
        m.write_train(1)
        m.close()
        mons[flag] = m
    assert mons[False]._summarizer is None
    assert mons[True]._summarizer is not None and mons[True]._summarizer.copies == 1   # ONE copy to the host
    host_ev, dev_ev = decode(str(tmp_path / "dev0")), decode(str(tmp_path / "dev1"))
    assert [t for t, _ in host_ev] == [t for t, _ in dev_ev] and len(host_ev) > 10
    fp, mon = net.fp, mons[False]
    w64 = lambda n: fp.param_view(n).detach().cpu().numpy().astype(np.float64).reshape(-1)  # noqa: E731
    nhist = nscalar = 0
    for (tag, hv), (_, dv) in zip(host_ev, dev_ev):
        kind, arg = mon._kinds.get(tag, ("", ""))
        if isinstance(hv, dict):
            vals = {"param_hist": lambda: w64(arg), "grad_hist": lambda: mon._grad(arg),
                    "act_hist": lambda: mon._activation(arg)}[kind]()
            v = np.asarray(vals, dtype=np.float64).reshape(-1)
            assert dv["num"] == hv["num"] == v.size and dv["min"] == hv["min"] and dv["max"] == hv["max"], tag
            assert np.array_equal(dv["bucket_limit"], hv["bucket_limit"]) and np.array_equal(dv["bucket"], hv["bucket"]), tag
            b1, b2 = v.size * 2.0 ** -52 * np.abs(v).sum(), v.size * 2.0 ** -52 * (v * v).sum()
            print(f"{tag}: n {v.size} sum diff {abs(dv['sum'] - hv['sum']):.3e} (allowed {b1:.3e}) "
                  f"sumsq diff {abs(dv['sum_squares'] - hv['sum_squares']):.3e} (allowed {b2:.3e})")
            assert abs(dv["sum"] - hv["sum"]) <= b1 and abs(dv["sum_squares"] - hv["sum_squares"]) <= b2, tag
            nhist += 1
        elif kind in ("param_norm", "gw_ratio"):
            ref = np.sqrt((w64(arg) ** 2).sum())
            if kind == "gw_ratio":
                ref = np.sqrt((mon._grad(arg).astype(np.float64) ** 2).sum()) / ref
            ulp = float(np.spacing(np.float32(ref)))
            print(f"{tag}: device {dv!r} host {hv!r} float64 {ref!r} ({abs(dv - ref) / ulp:.2f} ulp)")
            assert abs(dv - ref) <= 2 * ulp and ref > 0, tag
            nscalar += 1
        else:
            assert dv == hv, tag                                # train loss / accuracy: the same closure
    n_layers = len({e.name.split("/")[0] for e in fp.entries} & {"conv1", "conv2", "local3", "local4"})
    assert nhist >= 3 * n_layers + 1 and nscalar >= n_layers + 1
    if world == 3:
        assert mon._grad(fp.entries[0].name).dtype == np.float32
