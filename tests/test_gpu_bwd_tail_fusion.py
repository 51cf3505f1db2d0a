"""The fused backward tails of a conv block (conv -> relu -> [lrn] -> [max
pool]) against the unfused chain of ops of the same build, and the wave-seam
case of the vec8 LRN kernels.

dx of a fused kernel must be bit-identical to the chain's (torch.equal):
every value rounds where the chain rounded it. db is held against the fp64
column sum of that dx; COLSUM_ERR documents the bound."""

import os

import pytest
import torch

import poseidon_amd as pa
from poseidon_amd.ops import functional as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(a, b, rtol=2e-4, atol=2e-4, what=""):
    """The project's fp32 tolerance (tests/test_gpu_ops.py)."""
    a = a.detach().cpu().float()
    b = b.detach().cpu().float()
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    err = (a - b).abs()
    denom = b.abs().clamp(min=1.0)
    rel = (err / denom).max().item()
    print(f"{what}: max abs {err.max().item():.3e} rel {rel:.3e}")
    assert rel <= rtol or err.max().item() <= atol, \
        f"{what}: max abs {err.max():.3e} rel {rel:.3e}"


# ---------------------------------------------------------------------------
# vec8 LRN at channel counts whose rows do not divide a 64-lane wave
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("size", [3, 5])
@pytest.mark.parametrize("C", [24, 96])
def test_lrn_v8_wave_seam(C, size):
    """C = 24 / 96 give 3 / 12 lanes per pixel row: with rows packed
    back to back over a 256-thread block some row straddles two waves, where
    a one-lane shuffle cannot deliver the neighbour's halo. 2*7*7 = 98 rows
    span several such rows (row 21 at C = 24, row 5 at C = 96). alpha = 1
    makes a wrong halo an O(1) error."""
    x = rnd(2, C, 7, 7, seed=25)
    dy = rnd(2, C, 7, 7, seed=26)
    y_ref, sc_ref = ops.lrn_forward(x, size, 1.0, 0.75)
    dx_ref = ops.lrn_backward(x, y_ref, sc_ref, dy, size, 1.0, 0.75)
    y, sc = ops.lrn_forward(x.to(DEV), size, 1.0, 0.75)
    assert sc.numel() == 0, "expected the vec8 path"
    dx = ops.lrn_backward(x.to(DEV), y, sc, dy.to(DEV), size, 1.0, 0.75)
    close(y, y_ref, what=f"lrn fwd C={C} size={size}")
    close(dx, dx_ref, what=f"lrn bwd C={C} size={size}")


# ---------------------------------------------------------------------------
# fused tails against the unfused chain
# ---------------------------------------------------------------------------

# max abs error of ops.colsum_acc against the fp64 column sum of the same
# dx, worst over every dx checked below (three runs each), measured once on
# an MI355X. The bf16 figure is smaller because bf16 addends carry 8
# significant bits and few f32 additions of them round at all. A fused kernel
# sums the same stored values in another f32 order, so it gets 4x that and
# nothing else. (Worst fused errors at the time: 2.4e-07 / 1.4e-06.)
COLSUM_ERR = {torch.bfloat16: 4.768e-07, torch.float32: 2.399e-06}

K, S = (3, 3), (2, 2)
SHAPES = [(C, hw, pad) for C in (16, 24, 96) for hw in (7, 8)
          for pad in (0, 1)]
DTYPES = [torch.bfloat16, torch.float32]


def _ids(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    return None


_cache = {}


def block(C, hw, pad, size, dtype):
    """Activations of conv -> relu -> lrn -> pool(3/2, pad) at N = 2 and the
    chain's gradients, built once per case with the unfused ops:
    x (post-ReLU, about half exact zeros), y = lrn(x), the pool's u8 mask
    from a real forward of y, a random pool top diff, and
    dnorm -> dlrn -> dx (= dlrn masked by x > 0) plus relu-only and
    pool-only chains on the same x."""
    key = (C, hw, pad, size, dtype)
    if key in _cache:
        return _cache[key]
    p = (pad, pad)
    x = torch.relu(rnd(2, C, hw, hw, seed=31)).to(DEV, dtype)
    x = x.contiguous(memory_format=torch.channels_last)
    assert 0.3 < (x == 0).float().mean().item() < 0.7
    y, sc = ops.lrn_forward(x, size, 1.0, 0.75)
    assert sc.numel() == 0
    ypool, mask = ops.pool_max_forward(y, K, S, p)
    dpool = rnd(*ypool.shape, seed=32).to(DEV, dtype).contiguous(
        memory_format=torch.channels_last)
    dfull = rnd(2, C, hw, hw, seed=33).to(DEV, dtype).contiguous(
        memory_format=torch.channels_last)
    d = dict(x=x, y=y, sc=sc, mask=mask, dpool=dpool, dfull=dfull, p=p)
    # lrn + pool chain
    dnorm = ops.pool_max_backward(dpool, mask, x.shape, K, S, p)
    d["dlrn_pool"] = ops.lrn_backward(x, y, sc, dnorm, size, 1.0, 0.75)
    d["dx_lrn_pool"] = ops.relu_backward(x, d["dlrn_pool"], 0.0)
    # lrn alone (its own top diff)
    d["dlrn"] = ops.lrn_backward(x, y, sc, dfull, size, 1.0, 0.75)
    d["dx_lrn"] = ops.relu_backward(x, d["dlrn"], 0.0)
    # relu -> pool (the pool reads x itself: its own forward mask)
    _, xmask = ops.pool_max_forward(x, K, S, p)
    d["xmask"] = xmask
    d["dpool_x"] = ops.pool_max_backward(dpool, xmask, x.shape, K, S, p)
    d["dx_pool"] = ops.relu_backward(x, d["dpool_x"], 0.0)
    # relu alone
    d["dx_relu"] = ops.relu_backward(x, dfull, 0.0)
    torch.cuda.synchronize()
    _cache[key] = d
    return d


def colsum_err(dx):
    """(fp64 column sum of dx, max abs error of ops.colsum_acc against it)"""
    ref = dx.double().sum(dim=(0, 2, 3)).cpu()
    db = torch.zeros(dx.shape[1], device=DEV)
    ops.colsum_acc(dx, db)
    return ref, (db.cpu().double() - ref).abs().max().item()


def check_db(db, dx, base, dtype, what):
    ref, own = colsum_err(dx)
    err = (db.cpu().double() - (ref + base.double())).abs().max().item()
    bound = 4.0 * COLSUM_ERR[dtype]
    print(f"{what}: db max abs err {err:.3e} (bound {bound:.3e}; "
          f"colsum_acc here {own:.3e})")
    assert err <= bound, f"{what}: db max abs err {err:.3e} > {bound:.3e}"


def check_dx(dx, chain, what):
    n = (dx != chain).sum().item()
    print(f"{what}: {n} of {dx.numel()} dx elements differ from the chain")
    assert torch.equal(dx, chain), f"{what}: {n} elements differ"


def bias_base(C, prefill):
    return rnd(C, seed=34) if prefill else torch.zeros(C)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("size", [3, 5])
@pytest.mark.parametrize("C,hw,pad", SHAPES)
def test_lrn_tail_pool_relu_bias(C, hw, pad, size, dtype):
    """pool gather in + ReLU mask + bias sum: the whole conv1/conv2 tail.
    2 * hw * hw rows never fill whole blocks of 4 * (64 / (C/8)) rows."""
    d = block(C, hw, pad, size, dtype)
    base = bias_base(C, prefill=(hw == 8))
    db = base.clone().to(DEV)
    dx = ops.lrn_backward_tail(d["x"], d["y"], d["dpool"], size, 1.0, 0.75,
                               relu=True, db=db,
                               pool=(d["mask"], K, S, d["p"]))
    what = f"lrn+pool+relu+bias C={C} hw={hw} pad={pad} size={size}"
    check_dx(dx, d["dx_lrn_pool"], what)
    check_db(db, dx, base, dtype, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("C,hw,pad", SHAPES)
def test_lrn_tail_single_flags(C, hw, pad, dtype):
    """Each flag on its own (size 5): gather only, mask only, and mask +
    bias without a pool (an LRN whose consumer is not a max pool)."""
    size = 5
    d = block(C, hw, pad, size, dtype)
    what = f"C={C} hw={hw} pad={pad}"
    dx = ops.lrn_backward_tail(d["x"], d["y"], d["dpool"], size, 1.0, 0.75,
                               pool=(d["mask"], K, S, d["p"]))
    check_dx(dx, d["dlrn_pool"], "lrn+pool " + what)
    dx = ops.lrn_backward_tail(d["x"], d["y"], d["dfull"], size, 1.0, 0.75,
                               relu=True)
    check_dx(dx, d["dx_lrn"], "lrn+relu " + what)
    base = bias_base(C, prefill=(pad == 1))
    db = base.clone().to(DEV)
    dx = ops.lrn_backward_tail(d["x"], d["y"], d["dfull"], size, 1.0, 0.75,
                               relu=True, db=db)
    check_dx(dx, d["dx_lrn"], "lrn+relu+bias " + what)
    check_db(db, dx, base, dtype, "lrn+relu+bias " + what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("C,hw,pad", SHAPES)
def test_pool_tail_relu_bias(C, hw, pad, dtype):
    """conv -> relu -> max pool (AlexNet pool5, every CaffeNet block)."""
    d = block(C, hw, pad, 5, dtype)
    base = bias_base(C, prefill=(hw == 8))
    db = base.clone().to(DEV)
    dx = ops.pool_max_backward_tail(d["dpool"], d["xmask"], d["x"], K, S,
                                    d["p"], db=db)
    what = f"pool+relu+bias C={C} hw={hw} pad={pad}"
    check_dx(dx, d["dx_pool"], what)
    check_db(db, dx, base, dtype, what)
    dx = ops.pool_max_backward_tail(d["dpool"], d["xmask"], d["x"], K, S,
                                    d["p"])
    check_dx(dx, d["dx_pool"], "pool+relu " + what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("C,hw", [(16, 7), (24, 8), (96, 7)])
def test_relu_tail_bias(C, hw, dtype):
    """conv -> relu -> conv (conv3, conv4): in-place ReLU backward + bias."""
    d = block(C, hw, 0, 5, dtype)
    base = bias_base(C, prefill=(C == 24))
    db = base.clone().to(DEV)
    dy = d["dfull"].clone(memory_format=torch.preserve_format)
    dx = ops.relu_backward_bias(d["x"], dy, db)
    assert dx.data_ptr() == dy.data_ptr(), "expected the in-place form"
    what = f"relu+bias C={C} hw={hw}"
    check_dx(dx, d["dx_relu"], what)
    check_db(db, dx, base, dtype, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_tails_stride_the_grid(dtype):
    """With the block cap at 3 every kernel runs several grid-stride
    iterations per thread, each keeping its channel chunk (C = 96: 12 chunks
    per row, so the flat kernels need a block count that is a multiple of 3;
    rows = 2*8*8 = 128 against 20 LRN rows per block)."""
    C, hw, pad, size = 96, 8, 1, 5
    d = block(C, hw, pad, size, dtype)
    ops.set_bwd_tail_blocks(3)
    try:
        base = bias_base(C, True)
        db = base.clone().to(DEV)
        dx = ops.lrn_backward_tail(d["x"], d["y"], d["dpool"], size, 1.0,
                                   0.75, relu=True, db=db,
                                   pool=(d["mask"], K, S, d["p"]))
        check_dx(dx, d["dx_lrn_pool"], "strided lrn tail")
        check_db(db, dx, base, dtype, "strided lrn tail")
        db = base.clone().to(DEV)
        dx = ops.pool_max_backward_tail(d["dpool"], d["xmask"], d["x"], K, S,
                                        d["p"], db=db)
        check_dx(dx, d["dx_pool"], "strided pool tail")
        check_db(db, dx, base, dtype, "strided pool tail")
        db = base.clone().to(DEV)
        dx = ops.relu_backward_bias(
            d["x"], d["dfull"].clone(memory_format=torch.preserve_format), db)
        check_dx(dx, d["dx_relu"], "strided relu tail")
        check_db(db, dx, base, dtype, "strided relu tail")
    finally:
        ops.set_bwd_tail_blocks(0)


# ---------------------------------------------------------------------------
# net level
# ---------------------------------------------------------------------------

NET = """
    name: "tails"
    layers { name: "data" type: DUMMY_DATA top: "data" top: "label"
             dummy_data_param { num: 2 channels: 8 height: 15 width: 15
                 num: 2 channels: 1 height: 1 width: 1
                 data_filler { type: "gaussian" std: 1.0 }
                 data_filler { type: "constant" } } }
    layers { name: "conv1" type: CONVOLUTION bottom: "data" top: "conv1"
             convolution_param { num_output: 24 kernel_size: 3 pad: 1
                 weight_filler { type: "xavier" }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "relu1" type: RELU bottom: "conv1" top: "conv1" }
    layers { name: "norm1" type: LRN bottom: "conv1" top: "norm1"
             lrn_param { local_size: 5 alpha: 0.5 beta: 0.75 } }
    layers { name: "pool1" type: POOLING bottom: "norm1" top: "pool1"
             pooling_param { pool: MAX kernel_size: 3 stride: 2 } }
    layers { name: "conv2" type: CONVOLUTION bottom: "pool1" top: "conv2"
             convolution_param { num_output: 16 kernel_size: 3 pad: 1
                 weight_filler { type: "xavier" }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "relu2" type: RELU bottom: "conv2" top: "conv2" }
    layers { name: "conv3" type: CONVOLUTION bottom: "conv2" top: "conv3"
             convolution_param { num_output: 16 kernel_size: 3 pad: 1
                 weight_filler { type: "xavier" }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "relu3" type: RELU bottom: "conv3" top: "conv3" }
    layers { name: "pool3" type: POOLING bottom: "conv3" top: "pool3"
             pooling_param { pool: MAX kernel_size: 3 stride: 2 } }
    layers { name: "ip" type: INNER_PRODUCT bottom: "pool3" top: "ip"
             inner_product_param { num_output: 4
                 weight_filler { type: "xavier" } } }
    layers { name: "loss" type: SOFTMAX_LOSS bottom: "ip" bottom: "label"
             top: "loss" }
"""


def _net_step(fuse):
    from poseidon_amd.core.net import Net, TRAIN
    from poseidon_amd.proto import parse_text
    keys = ("PS_NO_BWD_TAIL_FUSION", "PS_BWD_TAIL_MIN_BYTES")
    old = {k: os.environ.pop(k, None) for k in keys}
    os.environ["PS_BWD_TAIL_MIN_BYTES"] = "0"  # the pass skips small convs
    if not fuse:
        os.environ["PS_NO_BWD_TAIL_FUSION"] = "1"
    try:
        pa.init(device="cuda", seed=31, compute_dtype=torch.bfloat16)
        net = Net(parse_text("NetParameter", NET), phase=TRAIN, verbose=False)
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    g = torch.Generator().manual_seed(21)
    net.blobs["data"].data = torch.randn(2, 8, 15, 15, generator=g).to(
        DEV, torch.bfloat16)
    net.blobs["label"].data = torch.tensor([1.0, 3.0]).view(2, 1, 1, 1).to(DEV)
    net.layers[0]._filled = True
    net.layers[0].refill = [False, False]
    net.forward()
    net.zero_param_diffs()
    net.backward()
    torch.cuda.synchronize()
    return net


def test_net_tails_match_unfused_step():
    """One step of conv-relu-lrn-pool-conv-relu-conv-relu-pool with the pass
    on and off (same seed, same weights): the three tails are in place, every
    conv's top diff (the fused kernels' dx) is bit-identical, and parameter
    gradients differ by f32 summation order only."""
    try:
        ref = _net_step(fuse=False)
        net = _net_step(fuse=True)
        by = dict(zip(net.layer_names, net.layers))
        assert by["norm1"]._tail_conv is by["conv1"]
        assert by["norm1"]._tail_pool is by["pool1"]
        assert by["pool1"].bwd_fused_into_producer
        assert by["relu2"]._tail_conv is by["conv2"]
        assert by["pool3"]._tail_conv is by["conv3"]
        assert by["relu1"].bwd_fused_into_consumer
        assert by["relu3"].bwd_fused_into_consumer
        assert all(by[c].bias_grad_by_consumer
                   for c in ("conv1", "conv2", "conv3"))
        assert not any(getattr(l, "bias_grad_by_consumer", False)
                       or getattr(l, "_tail_conv", None) is not None
                       for l in ref.layers)
        for name in ("conv3", "conv2", "pool1", "conv1"):
            check_dx(net.blobs[name].diff, ref.blobs[name].diff,
                     f"net diff of {name}")
        for ps_, rs in zip(net.learnable_params, ref.learnable_params):
            a, b = ps_.blob.diff.cpu().double(), rs.blob.diff.cpu().double()
            err = (a - b).abs().max().item()
            print(f"{ps_.blob.name}: max abs diff {err:.3e}")
            # the same dy bits go into the same kernels; only the bias sums
            # (and split-K atomics) add in another f32 order
            assert err <= 4.0 * COLSUM_ERR[torch.bfloat16], ps_.blob.name
    finally:
        pa.init(device="cpu", compute_dtype=torch.float32)
