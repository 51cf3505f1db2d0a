"""Deterministic mode (ops.set_deterministic / pa.init(deterministic=True) /
PS_DETERMINISTIC=1): every float reduction of the HIP kernels runs in an order
fixed by the shape and the plan.

Three kinds of checks.

Exactness: inputs are small multiples of 1/8 (exact in bf16 too), so every
partial sum in any order is exact in f32 and the ordered kernels must return
the integer reference bit for bit. The LRN tail's dx is not made of eighths
whatever its inputs are; its db is held to the a-priori bound of a recursive
f32 sum instead, |err| <= (n - 1) u sum|dx_i| (Higham, Accuracy and Stability
of Numerical Algorithms, eq. 4.4 to first order), which depends on the number
format and the values summed, not on the kernel.

Repeatability: inexact inputs (torch.randn), each op 20 times on the same
inputs with the mode on, all 20 outputs torch.equal. The shapes are ones at
which the same loop with the mode off gave more than one result on an MI355X
(profiles/deterministic_mode.md lists the counts); that disorder is not asserted here.

End to end: two solvers from one seed leave identical parameters, momentum
and loss after 5 steps, eager against eager and graphed against eager, in
bf16 and fp32, and with the backward-tail fusion forced on."""

import functools
import os

import pytest
import torch

import poseidon_amd as pa
from poseidon_amd.ops import functional as ops

from test_gpu_step_kernels import (Arena, _COLSUM_MT, _COLSUM_MT_CHUNKS,
                                   _eighths, _prefill8)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24
K3, S2 = (3, 3), (2, 2)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _name(dtype):
    return "bf16" if dtype is BF16 else "f32"


@pytest.fixture
def det():
    """The mode on for one test, off again whatever happens."""
    ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(False)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed),
                         dtype=torch.int32)


# ---------------------------------------------------------------------------
# interface
# ---------------------------------------------------------------------------

def test_interface():
    assert ops.deterministic() is False
    try:
        ops.set_deterministic(True)
        assert ops.deterministic() is True and pa.ctx().deterministic is True
        ops.set_deterministic(False)
        assert ops.deterministic() is False and pa.ctx().deterministic is False
        epoch = ops.conv_policy_epoch()
        pa.init(device="cuda", deterministic=True)
        assert ops.deterministic() is True and pa.ctx().deterministic is True
        # cached plans key on the epoch: toggling re-plans
        assert ops.conv_policy_epoch() > epoch
        n = ops.float_atomic_launches()
        assert isinstance(n, int) and ops.float_atomic_launches(reset=True) == n
        assert ops.float_atomic_launches() == 0
    finally:
        pa.init(device="cpu", deterministic=False)
    assert ops.deterministic() is False


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------

_DET_NET = """
    name: "detnet"
    layers { name: "data" type: DUMMY_DATA top: "data" top: "label"
             dummy_data_param { num: 16 channels: 3 height: 24 width: 24
                 num: 16 channels: 1 height: 1 width: 1
                 data_filler { type: "gaussian" std: 1.0 }
                 data_filler { type: "constant" } } }
    layers { name: "conv1" type: CONVOLUTION bottom: "data" top: "conv1"
             blobs_lr: 1 blobs_lr: 2 weight_decay: 1 weight_decay: 0
             convolution_param { num_output: 16 kernel_size: 3 pad: 1
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "relu1" type: RELU bottom: "conv1" top: "conv1" }
    layers { name: "pool1" type: POOLING bottom: "conv1" top: "pool1"
             pooling_param { pool: MAX kernel_size: 3 stride: 2 } }
    layers { name: "norm1" type: LRN bottom: "pool1" top: "norm1"
             lrn_param { local_size: 5 alpha: 0.5 beta: 0.75 } }
    layers { name: "conv2" type: CONVOLUTION bottom: "norm1" top: "conv2"
             blobs_lr: 1 blobs_lr: 2 weight_decay: 1 weight_decay: 0
             convolution_param { num_output: 32 kernel_size: 3 pad: 1 group: 2
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "relu2" type: RELU bottom: "conv2" top: "conv2" }
    layers { name: "ip1" type: INNER_PRODUCT bottom: "conv2" top: "ip1"
             blobs_lr: 1 blobs_lr: 2 weight_decay: 1 weight_decay: 0
             inner_product_param { num_output: 64
                 weight_filler { type: "gaussian" std: 0.05 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "drop1" type: DROPOUT bottom: "ip1" top: "ip1"
             dropout_param { dropout_ratio: 0.5 } }
    layers { name: "ip2" type: INNER_PRODUCT bottom: "ip1" top: "ip2"
             blobs_lr: 1 blobs_lr: 2 weight_decay: 1 weight_decay: 0
             inner_product_param { num_output: 10
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" } } }
    layers { name: "loss" type: SOFTMAX_LOSS bottom: "ip2" bottom: "label"
             top: "loss" }
"""


def _train(dtype, graphed=False, fuse=False, det=True, steps=5):
    """`steps` SGD steps of the net above from seed 77; returns (tensors,
    fused tail count, atomic-float launches during the steps): every owned
    parameter, its momentum and the loss, on the CPU."""
    from poseidon_amd.proto import Message, parse_text
    from poseidon_amd.solver.solver import SGDSolver

    keys = ("PS_NO_BWD_TAIL_FUSION", "PS_BWD_TAIL_MIN_BYTES")
    old = {k: os.environ.pop(k, None) for k in keys}
    # the pass skips convs this small; MIN_BYTES = 0 reaches the fused kernels
    os.environ["PS_BWD_TAIL_MIN_BYTES" if fuse
               else "PS_NO_BWD_TAIL_FUSION"] = "0" if fuse else "1"
    try:
        pa.init(device="cuda", seed=77, compute_dtype=dtype,
                deterministic=det)
        sp = Message("SolverParameter", base_lr=0.02, lr_policy="fixed",
                     momentum=0.9, weight_decay=0.001, max_iter=100,
                     display=0, snapshot=0)
        sp.net_param = parse_text("NetParameter", _DET_NET)
        s = SGDSolver(sp, verbose=False)
        data = torch.randn(16, 3, 24, 24, generator=_gen(5))
        s.net.blobs["data"].data = data.to(DEV, dtype)
        s.net.blobs["label"].data = (torch.arange(16) % 10).float().view(
            16, 1, 1, 1).to(DEV)
        s.net.layers[0]._filled = True
        s.net.layers[0].refill = [False, False]
        tails = sum(getattr(l, "_tail_conv", None) is not None
                    for l in s.net.layers)
        if graphed:
            assert s.enable_graph() is True
        before = ops.float_atomic_launches()
        s.step(steps)
        torch.cuda.synchronize()
        launches = ops.float_atomic_launches() - before
        if graphed:
            assert s._use_graph and s._graph is not None
        owned = [i for i, ps in enumerate(s.net.params) if ps.owner == i]
        assert len(owned) == 8 and s.iter == steps
        out = [s.net.params[i].blob.data.detach().cpu().clone() for i in owned]
        out += [s.history[i].detach().cpu().clone() for i in owned]
        out.append(s.net.blobs["loss"].data.detach().float().cpu().reshape(1))
        return out, tails, launches
    finally:
        pa.init(device="cpu", compute_dtype=torch.float32,
                deterministic=False)
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@functools.lru_cache(maxsize=None)
def _eager(dtype):
    return _train(dtype)


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.isfinite(x).all()
        n = int((x != y).sum())
        assert torch.equal(x, y), \
            f"{what}: tensor {k}: {n} of {x.numel()} elements differ, max " \
            f"{(x.double() - y.double()).abs().max().item():.3e}"


def test_training_step_launches_no_float_atomics():
    out, _tails, launches = _eager(BF16)
    assert launches == 0, f"{launches} atomic-float launches with the mode on"
    # the steps did train: the loss is finite and the momentum is not zero
    assert torch.isfinite(out[-1]).all() and float(out[8].abs().max()) > 0


def test_counter_sees_the_default_kernels():
    """The same step with the mode off takes atomic paths (split-K wgrads,
    bias column sums, the loss): the counter is wired to the real sites."""
    _out, _tails, launches = _train(BF16, det=False, steps=1)
    assert launches >= 3, f"only {launches} atomic-float launches counted"


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_same_seed_same_bits(dtype):
    _assert_same(_train(dtype)[0], _eager(dtype)[0],
                 f"{_name(dtype)} eager vs eager")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_graphed_equals_eager_bitwise(dtype):
    out, _tails, launches = _train(dtype, graphed=True)
    assert launches == 0
    _assert_same(out, _eager(dtype)[0], f"{_name(dtype)} graphed vs eager")


def test_same_seed_same_bits_with_fused_tails():
    a, tails, launches = _train(BF16, fuse=True)
    b, _t, _l = _train(BF16, fuse=True)
    assert tails >= 1 and launches == 0  # conv1 -> relu1 -> pool1
    _assert_same(a, b, "fused tails, eager vs eager")


# ---------------------------------------------------------------------------
# GEMM: tr16 workspace split-K, gathered wgrad, generic workspace split
# ---------------------------------------------------------------------------

TR_TILES = [(16, 64), (16, 128), (32, 64), (32, 128), (64, 64), (64, 128),
            (96, 128), (128, 128), (192, 128)]
TR_K = 1344  # four slices of 384: the last one half full
TR_CASES = [(bm, bn, M, N) for bm, bn in TR_TILES for M in (bm, 2 * bm)
            for N in ((bn, bn + 64) if bn == 128 else (bn,))]


@functools.lru_cache(maxsize=1)
def _tr_ints():
    """A8 [K, 384], B8 [K, 192] (ints in [-8, 8]) and A8^T B8 as int64."""
    a8 = _ints((TR_K, 384), -8, 8, 11)
    b8 = _ints((TR_K, 192), -8, 8, 12)
    return a8, b8, a8.t().long() @ b8.long()


def _tr_gemm(ext, bm, bn, M, N, A, B):
    tiles = (M // bm) * ((N + bn - 1) // bn)
    ext.set_tr16_tune(bm, bn, 4 * tiles)
    try:
        return ext.gemm(A, B, M, N, TR_K, False, False)
    finally:
        ext.set_tr16_tune(0, 0, 0)


@pytest.mark.parametrize("bm,bn,M,N", TR_CASES,
                         ids=[f"{bm}x{bn}-{M}x{N}" for bm, bn, M, N in TR_CASES])
def test_tr16_workspace_splitk_exact(det, bm, bn, M, N):
    from poseidon_amd.ops._backend import load
    ext = load()
    a8, b8, ref64 = _tr_ints()
    A = (a8[:, :M].float() / 8).contiguous().to(DEV, BF16)
    B = (b8[:, :N].float() / 8).contiguous().to(DEV, BF16)
    tiles = (M // bm) * ((N + bn - 1) // bn)
    ext.set_tr16_tune(bm, bn, 4 * tiles)
    try:
        plan = ops.gemm_plan(M, N, TR_K, False, False, True)
    finally:
        ext.set_tr16_tune(0, 0, 0)
    assert plan["tr16"] and (plan["bm"], plan["bn"]) == (bm, bn)
    assert plan["splitk"] == 4 and plan["kchunk"] == 384
    assert plan["ws_elems"] == 4 * M * N
    # one row of tiles pads z from 4 to 8: dead z blocks exist
    assert plan["grid_z"] == (8 if M == bm else 4)
    before = ops.float_atomic_launches()
    out = _tr_gemm(ext, bm, bn, M, N, A, B)
    torch.cuda.synchronize()
    assert ops.float_atomic_launches() == before
    want = (ref64[:M, :N].double() / 64).float()
    assert torch.equal(out.cpu(), want), \
        f"{int((out.cpu() != want).sum())} of {M * N} elements differ"


def _wgrad(x, dy, dw, implicit, G=1):
    ops.set_implicit_gemm(implicit)
    try:
        w = torch.zeros_like(dw)
        _y, cache = ops.conv2d_forward_ex(x, w, None, (1, 1), (1, 1), G)
        ops.conv2d_backward_weight_acc(x, cache[0], dy, dw, None, (1, 1),
                                       (1, 1), G)
    finally:
        ops.set_implicit_gemm(False)
    return dw


@pytest.mark.parametrize("implicit", [True, False],
                         ids=["implicit", "materialized"])
def test_conv_wgrad_exact(det, implicit):
    """N=2, C=16, 16x16, 3x3 pad 1, 32 outputs: K = 512 splits in two."""
    x8 = _ints((2, 16, 16, 16), -8, 8, 21)
    dy8 = _ints((2, 32, 16, 16), -8, 8, 22)
    base8 = _ints((32, 16, 3, 3), -40, 40, 23)
    ref = torch.nn.grad.conv2d_weight(x8.double() / 8, [32, 16, 3, 3],
                                      dy8.double() / 8, stride=1, padding=1)
    want = (base8.double() / 8 + ref).float()
    dw = (base8.float() / 8).to(DEV)
    before = ops.float_atomic_launches()
    _wgrad((x8.float() / 8).to(DEV, BF16), (dy8.float() / 8).to(DEV, BF16),
           dw, implicit)
    torch.cuda.synchronize()
    assert ops.float_atomic_launches() == before
    assert torch.equal(dw.cpu(), want), \
        f"{int((dw.cpu() != want).sum())} of {dw.numel()} elements differ"


def test_generic_workspace_split_exact(det):
    from poseidon_amd.ops._backend import load
    M = N = 64
    K = 6144
    plan = ops.gemm_plan(M, N, K, False, False, False)
    assert not plan["tr16"] and plan["splitk"] > 1
    assert plan["ws_elems"] == plan["splitk"] * M * N
    a8 = _ints((K, M), -8, 8, 31)
    b8 = _ints((K, N), -8, 8, 32)
    want = ((a8.t().long() @ b8.long()).double() / 64).float()
    before = ops.float_atomic_launches()
    out = load().gemm((a8.float() / 8).to(DEV), (b8.float() / 8).to(DEV), M, N,
                      K, False, False)
    torch.cuda.synchronize()
    assert ops.float_atomic_launches() == before
    assert torch.equal(out.cpu(), want)


# ---------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------
# one shape per route of the default launcher (tests/test_gpu_step_kernels.py
# _COLSUM_CASES names them): in deterministic mode all of them must be exact
COLSUM_CASES = [
    (50, 130, "banded-1blk"), (200, 130, "banded-3blk"),
    (200, 67, "banded-3blk"), (8, 512, "flat-ph1-1pass"),
    (2, 768, "flat-ph3-1pass"), (1023, 4096, "flat-ph1-multipass"),
    (1023, 6144, "flat-ph3-multipass"), (1023, 5120, "ph5-banded"),
]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("R,C,route", COLSUM_CASES,
                         ids=[f"{R}x{C}-{r}" for R, C, r in COLSUM_CASES])
def test_colsum_acc_exact(det, R, C, route, dtype):
    x8, sum8 = _eighths(R, C)
    assert 4 * R + 4 < 2 ** 21
    x = (x8.float() / 8).to(dtype).to(DEV)
    before = ops.float_atomic_launches()
    for pre8 in (_prefill8(C), torch.zeros(C, dtype=torch.int64)):
        arena = Arena([C])
        buf = arena.new()
        buf[arena.slices()[0]] = pre8.float() / 8
        want = buf.clone()
        want[arena.slices()[0]] = (pre8 + sum8).double().div(8).float()
        bufd = buf.to(DEV)
        ops.colsum_acc(x, arena.views(bufd)[0])
        torch.cuda.synchronize()
        assert torch.equal(bufd.cpu(), want), \
            f"{int((bufd.cpu() != want).sum())} of {C} columns differ"
    assert ops.float_atomic_launches() == before


def _colsum_mt_inputs(dtype, prefilled, exact=True):
    shapes = _COLSUM_MT[dtype]
    arena = Arena([s[1] for s in shapes])
    buf = arena.new()
    dys, sums, pres = [], [], []
    for (N, C, H, W), sl in zip(shapes, arena.slices()):
        if exact:
            x8, sum8 = _eighths(N * H * W, C)
            x = x8.float() / 8
        else:
            x = torch.randn(N * H * W, C, generator=_gen(C))
            sum8 = None
        dy = x.to(dtype).to(DEV).view(N, H, W, C)
        dys.append(dy.permute(0, 3, 1, 2))
        pre8 = _prefill8(C) if prefilled else torch.zeros(C, dtype=torch.int64)
        buf[sl] = pre8.float() / 8
        sums.append(sum8)
        pres.append(pre8)
    return arena, buf, dys, sums, pres


@pytest.mark.parametrize("prefilled", [True, False], ids=["prefilled", "zero"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
def test_colsum_mt_exact(det, dtype, prefilled):
    arena, buf, dys, sums, pres = _colsum_mt_inputs(dtype, prefilled)
    bufd = buf.to(DEV)
    mt = ops.colsum_mt_prepare(dys, arena.views(bufd))
    assert mt[2] == _COLSUM_MT_CHUNKS[dtype] and mt[4] == len(dys)
    assert mt[5].numel() == mt[2] * mt[3]
    before = ops.float_atomic_launches()
    for run in (1, 2):  # the second run accumulates onto the first
        ops.colsum_mt_run(mt, dtype is BF16)
        torch.cuda.synchronize()
        want = buf.clone()
        for sl, pre8, sum8 in zip(arena.slices(), pres, sums):
            want[sl] = (pre8 + run * sum8).double().div(8).float()
        assert torch.equal(bufd.cpu(), want), f"run {run}"
    assert ops.float_atomic_launches() == before


def test_colsum_mt_table_from_the_other_mode_is_refused():
    """A table prepared with the mode off has no scratch: running it with the
    mode on raises instead of adding atomically."""
    arena, buf, dys, _s, _p = _colsum_mt_inputs(F32, False)
    mt = ops.colsum_mt_prepare(dys, arena.views(buf.to(DEV)))
    assert mt[5].numel() == 0
    ops.set_deterministic(True)
    try:
        with pytest.raises(RuntimeError, match="prepare it again"):
            ops.colsum_mt_run(mt, False)
    finally:
        ops.set_deterministic(False)


# ---------------------------------------------------------------------------
# fused backward tails
# ---------------------------------------------------------------------------
TAIL_SHAPES = [(16, 7, 0), (24, 8, 1), (96, 8, 1)]


@functools.lru_cache(maxsize=None)
def _tail_block(C, hw, pad, dtype, exact):
    """Post-ReLU x (about half zeros), y = lrn(x), both pools' masks, and top
    diffs for the pool (dpool) and for the full map (dfull): eighths in
    [-4, 4] when exact, else N(0, 1)."""
    p = (pad, pad)
    cl = torch.channels_last
    x = torch.relu(torch.randn(2, C, hw, hw, generator=_gen(31))).to(
        DEV, dtype).contiguous(memory_format=cl)
    y, _sc = ops.lrn_forward(x, 5, 1.0, 0.75)
    ypool, mask = ops.pool_max_forward(y, K3, S2, p)
    _, xmask = ops.pool_max_forward(x, K3, S2, p)

    def diff(shape, seed):
        if exact:
            t = _ints(tuple(shape), -32, 32, seed).float() / 8
        else:
            t = torch.randn(*shape, generator=_gen(seed))
        return t.to(DEV, dtype).contiguous(memory_format=cl)

    return dict(x=x, y=y, mask=mask, xmask=xmask, p=p,
                dpool=diff(ypool.shape, 32), dfull=diff(x.shape, 33))


def _base8(C, prefill):
    return _prefill8(C) if prefill else torch.zeros(C, dtype=torch.int64)


def _tail_ops(d, db_of):
    """The three tail ops on block d as callables of no arguments returning
    (dx, db); db_of() makes a fresh db."""
    def lrn(alpha):
        db = db_of()
        dx = ops.lrn_backward_tail(d["x"], d["y"], d["dpool"], 5, alpha, 0.75,
                                   relu=True, db=db,
                                   pool=(d["mask"], K3, S2, d["p"]))
        return dx, db

    def pool():
        db = db_of()
        dx = ops.pool_max_backward_tail(d["dpool"], d["xmask"], d["x"], K3,
                                        S2, d["p"], db=db)
        return dx, db

    def relu():
        db = db_of()
        dy = d["dfull"].clone(memory_format=torch.preserve_format)
        dx = ops.relu_backward_bias(d["x"], dy, db)
        assert dx.data_ptr() == dy.data_ptr()
        return dx, db

    return dict(lrn=lambda: lrn(1.0), lrn0=lambda: lrn(0.0), pool=pool,
                relu=relu)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
@pytest.mark.parametrize("C,hw,pad", TAIL_SHAPES)
def test_tail_ops_exact(C, hw, pad, dtype):
    """dx equals the mode-off dx bit for bit; db equals base + the exact
    column sum of dx (pool and ReLU tails, and the LRN tail at alpha = 0,
    where it passes the pool gradient through), or lies within the recursive
    summation bound of it (the LRN tail proper)."""
    d = _tail_block(C, hw, pad, dtype, True)
    base8 = _base8(C, prefill=(hw == 8))
    tails = _tail_ops(d, lambda: (base8.float() / 8).to(DEV))
    off = {k: f() for k, f in tails.items()}
    torch.cuda.synchronize()
    ops.set_deterministic(True)
    try:
        before = ops.float_atomic_launches()
        on = {k: f() for k, f in tails.items()}
        torch.cuda.synchronize()
        assert ops.float_atomic_launches() == before
    finally:
        ops.set_deterministic(False)
    for k in tails:
        dx, db = on[k]
        assert torch.equal(dx, off[k][0]), f"{k}: dx differs from mode off"
        dx64 = dx.double().cpu()
        ref = base8.double() / 8 + dx64.sum(dim=(0, 2, 3))
        got = db.double().cpu()
        eighths = bool(((dx64 * 8) == (dx64 * 8).round()).all())
        # pool: sums of at most 4 eighths; relu: dy itself
        assert eighths or k.startswith("lrn"), f"{k}: dx is not exact"
        if not eighths:
            rows = dx64.numel() // C
            bound = rows * U * (dx64.abs().sum(dim=(0, 2, 3))
                                + base8.double().abs() / 8)
            err = (got - ref).abs()
            print(f"{k} C={C}: db err/bound {(err / bound.clamp(min=1e-300)).max():.3f}")
            assert bool((err <= bound).all()), f"{k}: db err {err.max():.3e}"
        else:
            # eighths: the fp64 reference is exact and f32 holds it
            assert torch.equal(got, ref), \
                f"{k}: {int((got != ref).sum())} of {C} db columns differ"


# ---------------------------------------------------------------------------
# softmax loss
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("C", [10, 1000])
@pytest.mark.parametrize("rows", [1, 5, 256, 1000])
def test_softmax_loss(rows, C):
    x = torch.randn(rows, C, generator=_gen(29)) * 2.0
    labels = torch.randint(0, C, (rows,), generator=_gen(30)).float()
    lp = torch.log_softmax(x.double(), dim=1)
    ref = -lp[torch.arange(rows), labels.long()].sum() / rows
    loss_off, prob_off = ops.softmax_loss_forward(x.to(DEV), labels.to(DEV))
    ops.set_deterministic(True)
    try:
        before = ops.float_atomic_launches()
        loss, prob = ops.softmax_loss_forward(x.to(DEV), labels.to(DEV))
        torch.cuda.synchronize()
        assert ops.float_atomic_launches() == before
    finally:
        ops.set_deterministic(False)
    assert torch.equal(prob, prob_off)
    # the tolerance of tests/test_gpu_ops.py::test_softmax_loss (close())
    err = abs(loss.item() - ref.item())
    rel = err / max(abs(ref.item()), 1.0)
    print(f"rows={rows} C={C}: loss {loss.item():.6f} err {err:.3e} "
          f"(mode off {abs(loss_off.item() - ref.item()):.3e})")
    assert rel <= 2e-4 or err <= 2e-4


# ---------------------------------------------------------------------------
# repeatability on inexact inputs
# ---------------------------------------------------------------------------
# name -> callable returning the op's float outputs; built once per name.
# Shapes: those at which 20 runs with the mode OFF gave more than one result
# on an MI355X (counts in profiles/deterministic_mode.md).

def repeat_ops():
    from poseidon_amd.ops._backend import load
    ext = load()
    out = {}

    bm, bn, M, N = 128, 128, 128, 192
    A = torch.randn(TR_K, M, generator=_gen(41)).to(DEV, BF16)
    B = torch.randn(TR_K, N, generator=_gen(42)).to(DEV, BF16)
    out["tr16_gemm"] = lambda: [_tr_gemm(ext, bm, bn, M, N, A, B)]

    x = torch.randn(2, 16, 16, 16, generator=_gen(43)).to(DEV, BF16)
    dy = torch.randn(2, 32, 16, 16, generator=_gen(44)).to(DEV, BF16)
    for name, implicit in (("wgrad_implicit", True), ("wgrad_colT", False)):
        out[name] = lambda implicit=implicit: [_wgrad(
            x, dy, torch.zeros(32, 16, 3, 3, device=DEV), implicit)]

    Ag = torch.randn(6144, 64, generator=_gen(45)).to(DEV)
    Bg = torch.randn(6144, 64, generator=_gen(46)).to(DEV)
    out["generic_gemm"] = lambda: [ext.gemm(Ag, Bg, 64, 64, 6144, False,
                                            False)]

    xc = torch.randn(1023, 4096, generator=_gen(47)).to(DEV)

    def colsum():
        db = torch.zeros(4096, device=DEV)
        ops.colsum_acc(xc, db)
        return [db]
    out["colsum_acc"] = colsum

    arena, buf, dys, _s, _p = _colsum_mt_inputs(F32, False, exact=False)
    state = {}

    def colsum_mt():
        key = ops.conv_policy_epoch()
        if state.get("key") != key:  # prepared in the mode it runs in
            state["key"] = key
            state["buf"] = buf.to(DEV)
            state["mt"] = ops.colsum_mt_prepare(dys, arena.views(state["buf"]))
        state["buf"].copy_(buf)
        ops.colsum_mt_run(state["mt"], False)
        return [state["buf"]]
    out["colsum_mt"] = colsum_mt

    d = _tail_block(96, 8, 1, F32, False)
    tails = _tail_ops(d, lambda: torch.zeros(96, device=DEV))
    for k in ("lrn", "pool", "relu"):
        out[k + "_tail"] = lambda k=k: list(tails[k]())

    xs = (torch.randn(1000, 1000, generator=_gen(48)) * 2.0).to(DEV)
    ls = torch.randint(0, 1000, (1000,), generator=_gen(49)).float().to(DEV)
    out["softmax_loss"] = lambda: [ops.softmax_loss_forward(xs, ls)[0]]
    return out


REPEAT_NAMES = ["tr16_gemm", "wgrad_implicit", "wgrad_colT", "generic_gemm",
                "colsum_acc", "colsum_mt", "lrn_tail", "pool_tail",
                "relu_tail", "softmax_loss"]


@functools.lru_cache(maxsize=1)
def _repeat_ops():
    return repeat_ops()


@pytest.mark.parametrize("name", REPEAT_NAMES)
def test_twenty_runs_one_result(det, name):
    f = _repeat_ops()[name]
    first = [t.clone() for t in f()]
    for run in range(1, 20):
        for a, b in zip(first, f()):
            assert torch.equal(a, b), \
                f"{name}: run {run} differs in {int((a != b).sum())} elements"
