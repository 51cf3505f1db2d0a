"""Solver debug_info on the GPU: the records of a real step against the CPU
path of the same feature, what the fused backward tails report, bf16 records
against the statistics of the tensors that outlive the step, the graphed step
against the eager one, and that nothing is launched when the switch is off.

The net is conv(16) -> relu -> lrn -> max pool -> conv -> relu -> ip -> loss
at batch 4 on 8x8 inputs. PS_BWD_TAIL_MIN_BYTES=0 while the Net is built
makes the backward-tail pass take convs this small, so conv1's tail runs
fused: the LRN's backward gathers the pool's and applies relu1's mask."""

import functools
import os

import pytest
import torch

import poseidon_amd as pa
from poseidon_amd.ops import functional as ops
from poseidon_amd.proto import Message, parse_text
from poseidon_amd.solver.solver import SGDSolver

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16

_NET = """
    name: "dbgnet"
    layers { name: "data" type: DUMMY_DATA top: "data" top: "label"
             dummy_data_param { num: 4 channels: 3 height: 8 width: 8
                 num: 4 channels: 1 height: 1 width: 1
                 data_filler { type: "gaussian" std: 1.0 }
                 data_filler { type: "constant" } } }
    layers { name: "conv1" type: CONVOLUTION bottom: "data" top: "conv1"
             blobs_lr: 1 blobs_lr: 2
             convolution_param { num_output: 16 kernel_size: 3 pad: 1
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "relu1" type: RELU bottom: "conv1" top: "conv1" }
    layers { name: "norm1" type: LRN bottom: "conv1" top: "norm1"
             lrn_param { local_size: 5 alpha: 0.5 beta: 0.75 } }
    layers { name: "pool1" type: POOLING bottom: "norm1" top: "pool1"
             pooling_param { pool: MAX kernel_size: 2 stride: 2 } }
    layers { name: "conv2" type: CONVOLUTION bottom: "pool1" top: "conv2"
             blobs_lr: 1 blobs_lr: 2
             convolution_param { num_output: 8 kernel_size: 3 pad: 1
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "relu2" type: RELU bottom: "conv2" top: "conv2" }
    layers { name: "ip1" type: INNER_PRODUCT bottom: "conv2" top: "ip1"
             blobs_lr: 1 blobs_lr: 2
             inner_product_param { num_output: 10
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" } } }
    layers { name: "loss" type: SOFTMAX_LOSS bottom: "ip1" bottom: "label"
             top: "loss" }
"""

_ENV = ("PS_NO_BWD_TAIL_FUSION", "PS_BWD_TAIL_MIN_BYTES")


@pytest.fixture(autouse=True)
def _restore_context():
    yield
    pa.init(device="cpu", compute_dtype=torch.float32, deterministic=False)


def _solver(device, dtype, debug=True, fuse=True, det=False):
    """The solver over the net above with fixed weights and input, display 2.
    fuse: conv1's backward tail fused (GPU only), else the per-layer path."""
    old = {k: os.environ.pop(k, None) for k in _ENV}
    os.environ["PS_BWD_TAIL_MIN_BYTES" if fuse
               else "PS_NO_BWD_TAIL_FUSION"] = "0" if fuse else "1"
    try:
        pa.init(device=device, seed=5, compute_dtype=dtype, deterministic=det)
        sp = Message("SolverParameter", base_lr=0.02, lr_policy="fixed",
                     momentum=0.9, weight_decay=0.001, max_iter=100,
                     display=2, snapshot=0, debug_info=debug)
        sp.net_param = parse_text("NetParameter", _NET)
        s = SGDSolver(sp, verbose=False)
    finally:
        for k in _ENV:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    g = torch.Generator().manual_seed(8)
    for i, ps in enumerate(s.net.params):
        w = torch.randn(ps.blob.data.shape, generator=g) * 0.1
        ps.blob.data.copy_(w.abs() if ps.param_idx else w)
    net = s.net
    net.blobs["data"].data = torch.randn(4, 3, 8, 8, generator=g).to(
        device, dtype)
    net.blobs["label"].data = (torch.arange(4) % 10).float().view(
        4, 1, 1, 1).to(device)
    net.layers[0]._filled = True
    net.layers[0].refill = [False, False]
    if device == "cuda":
        pool = net.layers[net.layer_names.index("pool1")]
        assert bool(pool.bwd_fused_into_producer) is fuse
    return s


def _key(r):
    return (r["phase"], r["layer"], r["kind"],
            r.get("name", r.get("param_idx")), r.get("param_idx"))


@functools.lru_cache(maxsize=None)
def _one_step(device, dtype, fuse):
    s = _solver(device, dtype, fuse=fuse)
    s.step(1)
    return s


def _close(a, b, rel=5e-4):
    return a == b or abs(a - b) <= rel * abs(b)


@pytest.mark.parametrize("fuse", [False, True], ids=["unfused", "fused"])
def test_fp32_records_match_the_cpu_path(fuse):
    """5e-4 relative: what tests/test_gpu_ops.py allows GPU conv gradients
    against torch on the CPU; a mean of magnitudes is no more sensitive than
    the elements it averages."""
    gpu = _one_step("cuda", F32, fuse).debug_records
    cpu = _one_step("cpu", F32, False).debug_records
    assert [_key(r) for r in gpu] == [_key(r) for r in cpu]
    assert all(r["available"] for r in cpu)
    compared = 0
    for g, c in zip(gpu, cpu):
        if fuse and g["phase"] == "backward" and g["kind"] == "bottom" \
                and g["layer"] in ("pool1", "norm1"):
            # defined departures: never written / reported masked
            continue
        assert g["available"] and g["count"] == c["count"], _key(g)
        for f in ("mean_abs", "max_abs", "data_mean_abs"):
            if f in c:
                print(_key(g), f, g[f], c[f])
                assert _close(g[f], c[f]), (_key(g), f, g[f], c[f])
        assert g["nonfinite"] == c["nonfinite"] == 0
        assert c["mean_abs"] > 0
        compared += 1
    assert compared == len(cpu) - (2 if fuse else 0)


def _bottom(recs, layer):
    return next(r for r in recs if r["phase"] == "backward"
                and r["kind"] == "bottom" and r["layer"] == layer)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_fused_path_records(dtype):
    recs = _one_step("cuda", dtype, True).debug_records
    pool = _bottom(recs, "pool1")
    assert pool["available"] is False and pool["note"] == "fused"
    assert pool["mean_abs"] == 0.0 and pool["count"] == 4 * 16 * 8 * 8
    relu, lrn = _bottom(recs, "relu1"), _bottom(recs, "norm1")
    assert relu["available"] and lrn["available"]
    assert relu["note"] == lrn["note"] == "masked"
    for f in ("mean_abs", "max_abs", "nonfinite", "count"):
        assert relu[f] == lrn[f]
    assert relu["mean_abs"] > 0
    from poseidon_amd.core.debug_info import format_records
    lines = format_records(recs)
    assert "    [Backward] Layer pool1, bottom blob norm1 diff: n/a (fused)" \
        in lines
    unfused = _one_step("cuda", dtype, False).debug_records
    assert all(r["available"] for r in unfused)
    assert [_key(r) for r in unfused] == [_key(r) for r in recs]


def _direct(t):
    out = ops.BlobStatsBuffer(1, "cuda")
    ops.blob_stats(t, out, 0)
    ops.blob_stats_finalize(out)
    asum, maxabs, nf = out.records()[0]
    return asum / t.numel(), maxabs, nf


def test_bf16_records_match_the_surviving_tensors():
    s = _one_step("cuda", BF16, True)
    net, recs = s.net, s.debug_records
    assert net.blobs["conv1"].data.dtype == BF16
    checked = 0
    for r in recs:
        if r["phase"] == "forward" and r["layer"] in ("ip1", "loss"):
            t = net.blobs[r["name"]].data
        elif r["phase"] == "backward" and r["kind"] == "param":
            li = net.layer_names.index(r["layer"])
            t = net.layers[li].blobs[r["param_idx"]].diff
        elif r["phase"] == "update":
            i = next(i for i, ps in enumerate(net.params)
                     if net.layers[ps.layer_idx].name == r["layer"]
                     and ps.param_idx == r["param_idx"])
            t = s.history[i]
        else:
            continue
        assert (r["mean_abs"], r["max_abs"], r["nonfinite"]) == _direct(t), \
            _key(r)
        assert r["count"] == t.numel()
        checked += 1
    assert checked == 2 + 6 + 6


@functools.lru_cache(maxsize=None)
def _six_steps(graphed, debug):
    s = _solver("cuda", BF16, debug=debug, det=True)
    if graphed:
        assert s.enable_graph() is True
    shown = []
    for it in range(6):
        s.step(1)
        if it % 2 == 0:
            shown.append(list(s.debug_records))
        else:
            assert s.debug_records is shown[-1] or s.debug_records == shown[-1]
    torch.cuda.synchronize()
    if graphed:
        assert s._use_graph and s._graph is not None
    params = [ps.blob.data.detach().cpu().clone() for ps in s.net.params]
    return shown, params


def test_graphed_records_equal_eager():
    eager, p_eager = _six_steps(False, True)
    graphed, p_graphed = _six_steps(True, True)
    _none, p_plain = _six_steps(True, False)
    assert len(eager) == len(graphed) == 3 and eager[0]
    assert all(not recs for recs in _none)
    for it, (e, g) in enumerate(zip(eager, graphed)):
        assert len(e) == len(g)
        for re_, rg in zip(e, g):
            assert re_ == rg, (2 * it, _key(re_), re_, rg)
    # the records move with training
    assert eager[0] != eager[1] != eager[2]
    for a, b, c in zip(p_eager, p_graphed, p_plain):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b) and torch.equal(a, c)


def test_nothing_is_launched_when_off():
    s = _solver("cuda", BF16, debug=False)
    s.step(1)
    before = ops.blob_stats_launches()
    s.step(2)
    torch.cuda.synchronize()
    assert ops.blob_stats_launches() == before
    assert s.debug_records == [] and s.net._dbg is None
    # and with it on, a display iteration launches: one per top and written
    # bottom diff, three tables, three finalizes
    s = _solver("cuda", BF16, debug=True)
    before = ops.blob_stats_launches()
    s.step(1)
    n_debug = ops.blob_stats_launches() - before
    tops = sum(len(t) for t in s.net.tops)
    bottoms = sum(r["kind"] == "bottom" and r["available"]
                  for r in s.debug_records)
    assert n_debug == tops + bottoms + 3 + 3
    before = ops.blob_stats_launches()
    s.step(1)  # iteration 1 is no display iteration
    assert ops.blob_stats_launches() == before
