"""Device-transform path on the GPU: the data_transform HIP kernel against the
torch CPU op (exact: one fp32 subtract, one fp32 multiply, one rounding to
the output dtype on both sides), the DATA layer with the switch on against
the layer with it off, and graphed training over a DATA layer against eager
training on the host path."""

import functools
import glob
import os

import pytest
import torch

import poseidon_amd as pa
from poseidon_amd.ops import functional as ops
from poseidon_amd.proto import Message, parse_text, read_proto_binary

from data_transform_util import data_layer_text, write_mean, write_pdb

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 64            # sentinel elements on either side of out
SENTINEL = 7777.0
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


# ---------------------------------------------------------------------------
# A. kernel == CPU op
# ---------------------------------------------------------------------------

# (N, C, H, W, crop)
S_ODD = (3, 3, 9, 11, 5)         # odd rows, flat size 225: ragged tail, groups
                                 # of 8 straddle rows, planes and images
S_NOCROP = (2, 1, 7, 13, 0)      # single channel, mirror over the full width
S_FULLCROP = (1, 3, 8, 8, 8)     # crop == source: offsets forced to 0
S_ROWS8 = (2, 3, 37, 41, 32)     # rows a multiple of 8: groups never straddle
S_WRAP = (16, 3, 300, 300, 0)    # 4.32 M outputs > 2048 x 256 x 8: the
                                 # grid-stride loop wraps

MODES = {"none": ops.MEAN_NONE, "scalar": ops.MEAN_SCALAR,
         "channel": ops.MEAN_CHANNEL, "image": ops.MEAN_IMAGE}
SCALES = [1.0, 0.00390625, 0.017]

KERNEL_CASES = [(S_ODD, m, s) for m in MODES for s in SCALES] + [
    (shape, "image", 0.017)
    for shape in (S_NOCROP, S_FULLCROP, S_ROWS8, S_WRAP)]


@functools.lru_cache(maxsize=None)
def _inputs(shape, mode):
    """raw cycling through all 256 byte values, hand-set params that hit both
    corners and one interior offset with flip mixed within the batch, and a
    non-integral mean."""
    N, C, H, W, crop = shape
    Ho, Wo = (crop, crop) if crop else (H, W)
    i = torch.arange(N * C * H * W)
    raw = ((i * 7 + i // 256) % 256).to(torch.uint8).view(N, C, H, W)
    assert len(torch.unique(raw)) == min(256, raw.numel())
    corners = [(0, 0), (H - Ho, W - Wo), ((H - Ho) // 2, (W - Wo) // 3)]
    params = torch.tensor([[*corners[n % 3], (n + n // 3 + (N == 1)) % 2]
                           for n in range(N)], dtype=torch.int32)
    if N > 1:
        assert 0 < int(params[:, 2].sum()) < N
    g = torch.Generator().manual_seed(3)
    count = {"none": 0, "scalar": 1, "channel": C, "image": C * H * W}[mode]
    mean = (torch.rand(count, generator=g) * 40 + 100) if count else None
    return raw, params, mean, (N, C, Ho, Wo)


@functools.lru_cache(maxsize=None)
def _reference(shape, mode, scale):
    """The CPU op's fp32 result, computed once per case."""
    raw, params, mean, oshape = _inputs(shape, mode)
    ref = torch.empty(oshape, dtype=torch.float32)
    ops.data_transform(raw, params, mean, MODES[mode], scale, ref)
    return ref


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize(
    "shape,mode,scale", KERNEL_CASES,
    ids=[f"{'x'.join(map(str, s))}-{m}-{sc}" for s, m, sc in KERNEL_CASES])
def test_kernel_equals_cpu_op(shape, mode, scale, dtype):
    raw, params, mean, oshape = _inputs(shape, mode)
    dt = DTYPES[dtype]
    ref = _reference(shape, mode, scale).to(dt)   # one RNE for bf16
    total = ref.numel()
    buf = torch.full((total + 2 * PAD,), SENTINEL, dtype=dt, device=DEV)
    out = buf[PAD:PAD + total].view(oshape)
    ops.data_transform(raw.to(DEV), params.to(DEV),
                       None if mean is None else mean.to(DEV), MODES[mode],
                       scale, out)
    torch.cuda.synchronize()
    got = buf.cpu()
    want = torch.full_like(got, SENTINEL)
    want[PAD:PAD + total] = ref.reshape(-1)
    bad = (got != want)
    assert torch.equal(got, want), \
        f"{int(bad.sum())} of {total} differ, first at " \
        f"{int(bad.nonzero()[0]) - PAD} (negative / >= {total}: a sentinel)"


def test_binding_rejects_what_the_kernel_cannot_take():
    raw, params, mean, oshape = _inputs(S_ODD, "image")
    out = torch.empty(oshape, device=DEV)
    r, p, m = raw.to(DEV), params.to(DEV), mean.to(DEV)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.data_transform(r.float(), p, m, ops.MEAN_IMAGE, 1.0, out)
    with pytest.raises(RuntimeError, match="params"):
        ops.data_transform(r, p[:2].contiguous(), m, ops.MEAN_IMAGE, 1.0, out)
    with pytest.raises(RuntimeError, match="mean"):
        ops.data_transform(r, p, m[:5].contiguous(), ops.MEAN_IMAGE, 1.0, out)
    with pytest.raises(RuntimeError, match="out"):
        ops.data_transform(r, p, m, ops.MEAN_IMAGE, 1.0,
                           torch.empty(3, 3, 10, 5, device=DEV))
    with pytest.raises(RuntimeError, match="aligned"):
        ops.data_transform(
            r, p, m, ops.MEAN_IMAGE, 1.0,
            torch.empty(226, device=DEV)[1:].view(oshape))


# ---------------------------------------------------------------------------
# B. the DATA layer, switch on == switch off
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gdt")
    write_pdb(d / "ten.pdb", 10, 3, 9, 11)
    write_mean(d / "mean.binaryproto", 3, 9, 11)
    write_pdb(d / "twelve.pdb", 12, 3, 10, 10, seed=21)
    return d


def _layer_forwards(files, switch):
    from poseidon_amd.core.net import Net, TRAIN
    pa.init(device="cuda", seed=11, compute_dtype=torch.bfloat16,
            device_transform=switch)
    try:
        transform = (f'crop_size: 5 mirror: true scale: 0.017 '
                     f'mean_file: "{files / "mean.binaryproto"}"')
        net = Net(parse_text("NetParameter", 'name: "dt"' + data_layer_text(
            files / "ten.pdb", 4, transform)), phase=TRAIN, verbose=False)
        assert net.layers[0].on_device is switch
        out = []
        for _ in range(6):
            net.forward()
            torch.cuda.synchronize()
            out.append((net.blobs["data"].data.cpu().clone(),
                        net.blobs["label"].data.cpu().clone()))
        return out
    finally:
        pa.init(device="cpu", compute_dtype=torch.float32,
                device_transform=False)


def test_layer_switch_on_equals_switch_off(files):
    off = _layer_forwards(files, False)
    on = _layer_forwards(files, True)
    for k in range(6):
        assert on[k][0].dtype == off[k][0].dtype == torch.bfloat16
        assert on[k][0].shape == (4, 3, 5, 5)
        assert torch.equal(on[k][0], off[k][0]), f"data, forward {k}"
        assert torch.equal(on[k][1], off[k][1]), f"label, forward {k}"
    assert not torch.equal(off[0][0], off[1][0])


# ---------------------------------------------------------------------------
# C. graphed real-data training equals eager training
# ---------------------------------------------------------------------------

# tests/test_gpu_step_kernels.py's step net below its data layer
_STEP_NET_TAIL = """
    layers { name: "c1" type: CONVOLUTION bottom: "data" top: "c1"
             blobs_lr: 1 blobs_lr: 2 weight_decay: 1 weight_decay: 0
             convolution_param { num_output: 8 kernel_size: 3 pad: 1
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "r1" type: RELU bottom: "c1" top: "c1" }
    layers { name: "p1" type: POOLING bottom: "c1" top: "p1"
             pooling_param { pool: MAX kernel_size: 2 stride: 2 } }
    layers { name: "ip" type: INNER_PRODUCT bottom: "p1" top: "ip"
             inner_product_param { num_output: 5
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" } } }
    layers { name: "loss" type: SOFTMAX_LOSS bottom: "ip" bottom: "label"
             top: "loss" }
"""
_TRANSFORM = ("crop_size: 8 mirror: true mean_value: 104.0 "
              "mean_value: 117.0 mean_value: 123.0")

# Worst element-wise difference of any owned parameter or history tensor
# between two EAGER, SWITCH-OFF runs of _train (same seed, same records), over
# three pairs of runs per compute dtype, measured on an MI355X:
# 6.104e-05, 3.052e-05 and 6.104e-05 in fp32 (the records are unscaled pixel
# values, so the conv history reaches several hundred and one f32 ulp of it
# is 6.1e-05; some f32 kernel accumulates in an order that varies). bf16
# training repeated bit for bit in all three pairs. In the same session the
# device path against the host path gave 6.104e-05 (fp32) and 0 (bf16), eager
# and graphed alike.
D0 = {"fp32": 6.104e-05, "bf16": 0.0}


def _solver(files, dtype, switch, prefix):
    from poseidon_amd.solver.solver import SGDSolver
    pa.init(device="cuda", seed=1234, compute_dtype=dtype,
            device_transform=switch)
    sp = Message("SolverParameter", base_lr=0.05, lr_policy="step",
                 stepsize=2, gamma=0.5, momentum=0.9, weight_decay=0.001,
                 max_iter=100, display=0, snapshot=4,
                 snapshot_prefix=str(prefix))
    sp.net_param = parse_text("NetParameter", 'name: "stepnet"'
                              + data_layer_text(files / "twelve.pdb", 4,
                                                _TRANSFORM) + _STEP_NET_TAIL)
    return SGDSolver(sp, verbose=False)


def _train(files, dtype, switch, graphed, outdir):
    """step(5) then step(3) over the 12-record DATA net, snapshot every 4;
    returns iter, the data layer's cursor once its prefetch has settled,
    parameters and history of the owned parameters, the snapshot files'
    names and the blobs of the iteration-4 .caffemodel."""
    os.makedirs(outdir, exist_ok=True)
    prefix = os.path.join(str(outdir), "snap")
    try:
        s = _solver(files, dtype, switch, prefix)
        layer = s.net.layers[0]
        assert layer.on_device is switch
        if graphed:
            assert s.enable_graph() is True
            assert layer.external_staging is True
        s.step(5)
        s.step(3)
        torch.cuda.synchronize()
        if graphed:
            # a capture that failed falls back to eager and clears these
            assert s._use_graph and s._graph is not None
        layer._ready.wait(30)   # the batch being prefetched is complete
        owned = [i for i, ps in enumerate(s.net.params) if ps.owner == i]
        assert sorted(s.history) == owned and len(owned) == 4
        names = sorted(os.path.basename(f) for f in glob.glob(prefix + "*"))
        model = read_proto_binary(prefix + "_iter_4.caffemodel",
                                  "NetParameter")
        blobs = [torch.tensor(list(b.data), dtype=torch.float32)
                 for lp in model.layers for b in lp.blobs]
        return {"iter": s.iter, "cursor": layer.cursor,
                "params": [s.net.params[i].blob.data.detach().cpu().clone()
                           for i in owned],
                "history": [s.history[i].detach().cpu().clone()
                            for i in owned],
                "files": names, "snap4": blobs}
    finally:
        pa.init(device="cpu", compute_dtype=torch.float32,
                device_transform=False)


def _state_diff(a, b):
    return max((x.double() - y.double()).abs().max().item()
               for k in ("params", "history") for x, y in zip(a[k], b[k]))


def _ulp32(x):
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


_REFS = {}


def _eager_off(files, name, tmp_path_factory):
    """(a): eager on the host path, the behaviour before the switch existed.
    Run once per dtype and shared."""
    if name not in _REFS:
        _REFS[name] = _train(files, DTYPES[name], False, False,
                             tmp_path_factory.mktemp("ref_" + name))
    return _REFS[name]


def _assert_same_training(got, ref, name, what):
    print(f"{name} {what}: worst |got - eager switch-off| "
          f"{_state_diff(got, ref):.3e} (D0 {D0[name]:.3e})")
    assert got["iter"] == 8 and ref["iter"] == 8
    # 8 batches trained on + the one prefetched ahead, 4 records each
    assert got["cursor"] == ref["cursor"] == 36
    assert got["files"] == ref["files"] == [
        "snap_iter_4.caffemodel", "snap_iter_4.solverstate.0.0"]
    for kind in ("params", "history", "snap4"):
        assert len(got[kind]) == len(ref[kind]) == 4
        for k, (tg, te) in enumerate(zip(got[kind], ref[kind])):
            err = (tg.double() - te.double()).abs()
            bound = _ulp32(te).clamp(min=4.0 * D0[name])
            assert bool((err <= bound).all()), \
                f"{name} {what} {kind} {k}: max err {err.max().item():.3e}, " \
                f"bound {bound.min().item():.3e}"


@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_eager_training_on_the_device_path_equals_the_host_path(
        files, name, tmp_path, tmp_path_factory):
    """(b) against (a): same records, same crops and mirrors, so the same
    batches bit for bit; what is left is eager training's own run-to-run
    difference. Bound: max(one f32 ulp of the value, 4 * D0)."""
    ref = _eager_off(files, name, tmp_path_factory)
    got = _train(files, DTYPES[name], True, False, tmp_path / "b")
    _assert_same_training(got, ref, name, "eager switch-on")


@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_graphed_real_data_training_equals_eager(files, name, tmp_path,
                                                 tmp_path_factory):
    """(c) against (a): with the switch on enable_graph() takes a net with a
    DATA layer; step(5) + step(3) consume the records eager training does
    (the capture's warm-up passes run on the first batch and take no
    further one), the lr halves every 2 iterations, and the iteration-4
    snapshot is written at the same boundary with the same content. Same
    bound as above."""
    ref = _eager_off(files, name, tmp_path_factory)
    got = _train(files, DTYPES[name], True, True, tmp_path / "c")
    _assert_same_training(got, ref, name, "graphed switch-on")


def test_switch_off_still_refuses_the_graph(files, tmp_path):
    try:
        s = _solver(files, torch.bfloat16, False, tmp_path / "snap")
        assert s.enable_graph() is False
        assert s._use_graph is False
        assert s.net.layers[0].external_staging is False
    finally:
        pa.init(device="cpu", compute_dtype=torch.float32,
                device_transform=False)
