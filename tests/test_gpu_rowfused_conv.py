"""Row-fused small-channel first-layer convolution (conv_rowfused.hip: forward
and weight gradient from staged input rows, no column matrix) beside the
materialized path and against torch's CPU convolution.

Every test forces the path with the switch and threshold 0 and puts back
what it found (the switch is on by default, PS_ROWFUSED_CONV=0 turns it off). The forward runs the same MFMA, k order and epilogue as the
materialized im2col + GEMM, so it must be bit-identical (torch.equal). The
weight gradients sum the same fp32 products in different orders, so they may
differ by the reassociation bound 2 * NP * 2^-24 * (|dy|^T |col|) per element
(tests/test_gpu_packed_conv.py). Against the CPU fp32 reference both get the
bound of tests/test_gpu_bf16.py::test_conv_bf16: close_bf16, rtol = atol =
1e-2. References are computed once per case."""

import functools

import pytest
import torch
import torch.nn.functional as F

import poseidon_amd as pa
from poseidon_amd.ops import functional as ops
from test_gpu_bf16 import close_bf16
from test_gpu_packed_conv import _CASES as _PACKED_CASES, _q, _rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (name, N, C, H, W, Co, kh, kw, stride, pad)
_EXTRA = [
    # Wo = 130 exceeds the 128-position tile: Wo-segment mode, ragged second
    # segment
    ("3x3-s1-p1-w130", 2, 3, 6, 130, 16, 3, 3, 1, 1),
    # 8 row strips per tile -> 80 tiles; with the grid capped at 3 blocks each
    # block walks 27 tiles (persistent loop, accumulate-across-tiles wgrad)
    ("3x3-n8-h80-w16", 8, 3, 80, 16, 16, 3, 3, 1, 1),
    # VGG conv1_1's plan at small size: Co = 64, ld_col = 64
    ("vgg-co64", 2, 3, 12, 20, 64, 3, 3, 1, 1),
    # Co = 128: the 8-fragment kernels (two k passes in the wgrad)
    ("7x7-co128", 2, 3, 21, 21, 128, 7, 7, 2, 3),
]
_CASES = list(_PACKED_CASES) + _EXTRA
_NAMES = [c[0] for c in _CASES]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and CPU fp32 references of one case, computed once."""
    _, N, C, H, W, Co, kh, kw, s, p = next(c for c in _CASES if c[0] == name)
    x = _q(_rnd(N, C, H, W, seed=31))
    w = _q(_rnd(Co, C, kh, kw, seed=32, scale=0.2))
    b = _rnd(Co, seed=33)
    y_nobias = F.conv2d(x, w, None, stride=s, padding=p)
    dy = _q(_rnd(*y_nobias.shape, seed=34))
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=s, padding=p)
    dw_abs = torch.nn.grad.conv2d_weight(x.abs(), w.shape, dy.abs(),
                                         stride=s, padding=p)
    NP = N * y_nobias.shape[2] * y_nobias.shape[3]
    return dict(x=x, w=w, b=b, dy=dy, stride=(s, s), pad=(p, p),
                y_nobias=y_nobias,
                y_bias_relu=F.relu(y_nobias + b.view(1, -1, 1, 1)),
                dw=dw, dw_abs=dw_abs, NP=NP,
                bound=(2.0 * NP * 2.0 ** -24) * dw_abs + 1e-30)


class _rowfused:
    """The path forced on (threshold 0) or off; on leaving, the switch,
    threshold and grid cap are what they were on entering."""

    def __init__(self, on, blocks=0):
        self.on, self.blocks = on, blocks

    def __enter__(self):
        self.was = (ops.rowfused_conv(), ops.rowfused_threshold())
        ops.set_rowfused_conv(self.on)
        ops.set_rowfused_threshold(0)
        ops._set_rowfused_blocks(self.blocks)

    def __exit__(self, *exc):
        ops.set_rowfused_conv(self.was[0])
        ops.set_rowfused_threshold(self.was[1])
        ops._set_rowfused_blocks(0)


def _plan(c):
    return ops.conv_plan(c["x"].shape, c["w"].shape, c["stride"], c["pad"], 1,
                         True)


def _is_sentinel(slot):
    return slot.dim() == 2 and slot.shape[0] == 0


def _run(c, on, x=None, blocks=0, bias=True):
    """y without bias, y with bias + ReLU, the cache slot, dW and the khwc
    scratch of one path."""
    xg = c["x"].to(DEV, torch.bfloat16) if x is None else x
    wg, bg = c["w"].to(DEV), c["b"].to(DEV)
    dyg = c["dy"].to(DEV, torch.bfloat16)
    with _rowfused(on, blocks):
        y0, (slot, _) = ops.conv2d_forward_ex(xg, wg, None, c["stride"],
                                              c["pad"], 1)
        y1 = None
        if bias:
            y1, _ = ops.conv2d_forward_ex(xg, wg, bg, c["stride"], c["pad"],
                                          1, fuse_relu=True)
        dw = torch.zeros_like(wg)
        dwk = ops.conv2d_backward_weight_acc(xg, slot, dyg, dw, None,
                                             c["stride"], c["pad"], 1)
        torch.cuda.synchronize()
    return y0, y1, slot, dw, dwk


@functools.lru_cache(maxsize=None)
def _materialized(name):
    return _run(_case(name), False)


@pytest.mark.parametrize("name", _NAMES)
def test_forward_and_wgrad(name):
    c = _case(name)
    # the many-tiles case walks its 80 tiles on 3 blocks
    blocks = 3 if name == "3x3-n8-h80-w16" else 0
    y0, y1, slot, dw, dwk = _run(c, True, blocks=blocks)
    m0, m1, mslot, mdw, _ = _materialized(name)
    plan = _plan(c)
    assert _is_sentinel(slot), f"cache slot is {tuple(slot.shape)}"
    assert tuple(mslot.shape) == (plan["NP"], plan["ld_col"])
    assert y0.dtype == torch.bfloat16
    assert torch.equal(y0, m0), \
        f"fwd differs from the materialized path by " \
        f"{(y0.float() - m0.float()).abs().max():.3e}"
    assert torch.equal(y1, m1), \
        f"fwd bias+relu differs by {(y1.float() - m1.float()).abs().max():.3e}"
    close_bf16(y0, c["y_nobias"], rtol=1e-2, atol=1e-2, what=f"{name} fwd")
    close_bf16(y1, c["y_bias_relu"], rtol=1e-2, atol=1e-2,
               what=f"{name} fwd bias+relu")
    err = (dw - mdw).abs().cpu()
    print(f"{name}: max |dW_rowfused - dW_colT| = {err.max():.3e}, "
          f"bound min {c['bound'].min():.3e} max {c['bound'].max():.3e}")
    assert bool((err <= c["bound"]).all()), \
        f"max |dW_rowfused - dW_colT| = {err.max():.3e}"
    close_bf16(dw, c["dw"], rtol=1e-2, atol=1e-2, what=f"{name} dW")
    # pad columns of the khwc scratch are exact zeros
    assert tuple(dwk.shape) == (c["w"].shape[0], plan["wk_ld"])
    assert dwk[:, plan["Kcol"]:].abs().sum().item() == 0
    assert dwk[:, :plan["Kcol"]].abs().sum().item() > 0


@pytest.mark.parametrize("name", ["7x7-s2-p3-w14", "11x11-w19-h15",
                                  "c1-5x5-s2-p2", "c4-3x3-s2-w9"])
def test_input_layouts(name):
    """x is staged through its strides: NCHW, channels-last and a non-dense
    view give the same y and, within the bound, the same dW."""
    c = _case(name)
    xg = c["x"].to(DEV, torch.bfloat16)
    N, C, H, W = xg.shape
    wide = torch.full((N, C + 2, H, W + 6), float("nan"), device=DEV,
                      dtype=torch.bfloat16)
    wide[:, 1:C + 1, :, 3:W + 3] = xg
    y_ref, _, _, dw_ref, _ = _run(c, True, bias=False)
    for v in (xg.contiguous(memory_format=torch.channels_last),
              wide[:, 1:C + 1, :, 3:W + 3]):
        y, _, slot, dw, _ = _run(c, True, x=v, bias=False)
        assert _is_sentinel(slot)
        assert torch.equal(y, y_ref)
        assert bool(((dw - dw_ref).abs().cpu() <= c["bound"]).all())
        close_bf16(dw, c["dw"], rtol=1e-2, atol=1e-2, what=f"{name} dW")


def test_no_column_matrix_is_allocated():
    """A mid-size conv1 (colT 4*33*33*384*2 B = 3.3 MB) grows the allocator's
    peak by less than that column matrix when row-fused, and by at least it
    on the materialized path."""
    N, C, H, W, Co = 4, 3, 139, 139, 96
    x = _q(_rnd(N, C, H, W, seed=51)).to(DEV, torch.bfloat16)
    w = _q(_rnd(Co, C, 11, 11, seed=52, scale=0.2)).to(DEV)
    plan = ops.conv_plan(x.shape, w.shape, (4, 4), (0, 0), 1, True)
    col_bytes = plan["NP"] * plan["ld_col"] * 2
    growth = {}
    for on in (True, False):
        with _rowfused(on):
            ops.conv2d_forward_ex(x, w, None, (4, 4), (0, 0), 1)  # warm
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            y, (slot, _) = ops.conv2d_forward_ex(x, w, None, (4, 4), (0, 0), 1)
            torch.cuda.synchronize()
            growth[on] = torch.cuda.max_memory_allocated() - base
            assert _is_sentinel(slot) is on
            del y, slot
    print(f"colT {col_bytes} B; peak growth row-fused {growth[True]} B, "
          f"materialized {growth[False]} B")
    assert growth[True] < col_bytes
    assert growth[False] >= col_bytes


def test_wgrad_follows_the_forward_not_the_switch():
    c = _case("conv1-39-np256")
    xg = c["x"].to(DEV, torch.bfloat16)
    wg = c["w"].to(DEV)
    dyg = c["dy"].to(DEV, torch.bfloat16)
    was = ops.rowfused_conv()
    try:
        with _rowfused(True):
            _, (slot, _) = ops.conv2d_forward_ex(xg, wg, None, c["stride"],
                                                 c["pad"], 1)
            assert _is_sentinel(slot)
            ops.set_rowfused_conv(False)  # flipped between fwd and bwd
            dw = torch.zeros_like(wg)
            n0 = ops.float_atomic_launches()
            ops.conv2d_backward_weight_acc(xg, slot, dyg, dw, None,
                                           c["stride"], c["pad"], 1)
            assert ops.float_atomic_launches() == n0 + 1
        close_bf16(dw, c["dw"], rtol=1e-2, atol=1e-2,
                   what="dW after switch-off")
        with _rowfused(False):
            _, (colT, _) = ops.conv2d_forward_ex(xg, wg, None, c["stride"],
                                                 c["pad"], 1)
            assert colT.dim() == 2 and colT.shape[0] == c["NP"]
            ops.set_rowfused_conv(True)   # and the other way round
            dw = torch.zeros_like(wg)
            ops.conv2d_backward_weight_acc(xg, colT, dyg, dw, None,
                                           c["stride"], c["pad"], 1)
        close_bf16(dw, c["dw"], rtol=1e-2, atol=1e-2,
                   what="dW after switch-on")
    finally:
        ops.set_rowfused_conv(was)


@pytest.mark.parametrize("name", ["conv1-39-np256", "7x7-s2-p3-w14"])
def test_persistent_buffers_match_per_layer_route(name):
    """wk from repack_mt and dW from a persistent, pre-zeroed dwk through
    unpack_mt, two iterations running, against the per-layer kernels."""
    c = _case(name)
    xg = c["x"].to(DEV, torch.bfloat16)
    wg, bg = c["w"].to(DEV), c["b"].to(DEV)
    dyg = c["dy"].to(DEV, torch.bfloat16)
    Co, C, kh, kw = wg.shape
    with _rowfused(True):
        plan = _plan(c)
        assert plan["rowfused"] and not plan["packed"]
        y_l, (slot_l, _) = ops.conv2d_forward_ex(xg, wg, bg, c["stride"],
                                                 c["pad"], 1)
        dw_l = torch.zeros_like(wg)
        ops.conv2d_backward_weight_acc(xg, slot_l, dyg, dw_l, None,
                                       c["stride"], c["pad"], 1)
        wk = torch.zeros(Co, plan["wk_ld"], device=DEV, dtype=torch.bfloat16)
        wkT = torch.empty(kh * kw * C, Co, device=DEV, dtype=torch.bfloat16)
        dwk = torch.zeros(Co, plan["Kgw"], device=DEV)
        dw = torch.zeros_like(wg)
        layout = ops.khwc_layout(C, kw, False)
        assert layout == (plan["kw_ld"], plan["c_ld"])
        rmt = ops.repack_mt_prepare([wg], [wk], [wkT], [1], [layout[0]],
                                    [layout[1]])
        umt = ops.unpack_mt_prepare([dwk], [dw], [C], [kh], [kw],
                                    [layout[0]], [layout[1]])
        for it in range(2):
            ops.repack_mt_run(rmt)
            y, (slot, _) = ops.conv2d_forward_ex(xg, wg, bg, c["stride"],
                                                 c["pad"], 1,
                                                 cached=(wk, wkT))
            assert _is_sentinel(slot)
            assert torch.equal(y, y_l), f"iteration {it}: forward differs"
            dwk.zero_()
            dw.zero_()
            used = ops.conv2d_backward_weight_acc(
                xg, slot, dyg, dw, None, c["stride"], c["pad"], 1,
                dwk_buf=dwk, skip_unpack=True)
            assert used.data_ptr() == dwk.data_ptr()
            assert dw.abs().max().item() == 0  # unpack deferred
            ops.unpack_mt_run(umt)
            err = (dw - dw_l).abs().cpu()
            assert bool((err <= c["bound"]).all()), \
                f"iteration {it}: max |dW_mt - dW_layer| = {err.max():.3e}"
            close_bf16(dw, c["dw"], rtol=1e-2, atol=1e-2, what="dW via mt")


_NET = """
    name: "rowfused1"
    layers { name: "data" type: DUMMY_DATA top: "data" top: "label"
             dummy_data_param { num: 4 channels: 3 height: 19 width: 21
                 num: 4 channels: 1 height: 1 width: 1
                 data_filler { type: "gaussian" std: 1.0 }
                 data_filler { type: "constant" } } }
    layers { name: "c1" type: CONVOLUTION bottom: "data" top: "c1"
             convolution_param { num_output: 16 kernel_size: 5 stride: 2
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "r1" type: RELU bottom: "c1" top: "c1" }
    layers { name: "c2" type: CONVOLUTION bottom: "c1" top: "c2"
             convolution_param { num_output: 8 kernel_size: 3
                 weight_filler { type: "gaussian" std: 0.1 } } }
    layers { name: "ip" type: INNER_PRODUCT bottom: "c2" top: "ip"
             inner_product_param { num_output: 5
                 weight_filler { type: "gaussian" std: 0.1 } } }
    layers { name: "loss" type: SOFTMAX_LOSS bottom: "ip" bottom: "label"
             top: "loss" }
"""


def _net_inputs():
    data = _q(_rnd(4, 3, 19, 21, seed=41))
    labels = torch.tensor([0.0, 2.0, 4.0, 1.0]).view(4, 1, 1, 1)
    return data, labels


def test_net_runs_rowfused_first_layer():
    """Two iterations of conv(3 ch) -> relu -> conv -> ip -> loss with the
    path on and off: equal loss (the forward is bit-identical), param diffs
    within close_bf16."""
    from poseidon_amd.core.net import Net, TRAIN
    from poseidon_amd.proto import parse_text

    data, labels = _net_inputs()

    def run(on):
        with _rowfused(on):
            pa.init(device="cuda", seed=7, compute_dtype=torch.bfloat16)
            net = Net(parse_text("NetParameter", _NET), phase=TRAIN,
                      verbose=False)
            net.blobs["data"].data = data.to(DEV, torch.bfloat16)
            net.blobs["label"].data = labels.to(DEV)
            net.layers[0]._filled = True
            net.layers[0].refill = [False, False]
            convs = [l for l in net.layers if l.type_name == "CONVOLUTION"]
            n0 = ops.float_atomic_launches()
            for it in range(2):
                loss = net.forward()
                assert _is_sentinel(convs[0]._colT[0][0]) is on
                net.zero_param_diffs()
                net.backward()
                for l in convs:  # as the single-GPU solver runs them
                    l.defer_unpack = True
            torch.cuda.synchronize()
            c1 = convs[0]
            assert c1._dwk_packed is False and c1._dwk_layout == (5, 3)
            assert c1._wk_cache[0].shape[1] == 128
            assert c1._dwk_cache.shape[1] == 128
            assert ops.float_atomic_launches() > n0
            return loss, [p.blob.diff.clone() for p in net.learnable_params]

    try:
        loss_on, diffs_on = run(True)
        loss_off, diffs_off = run(False)
    finally:
        pa.init(device="cpu", compute_dtype=torch.float32)
    assert loss_on == loss_off
    for d_on, d_off in zip(diffs_on, diffs_off):
        close_bf16(d_on, d_off, rtol=1e-2, atol=1e-2, what="param diff")


def test_graphed_training_replays_to_the_eager_result():
    """The same net trained 6 steps by the solver, eager and under graph
    capture, both row-fused: the captured step allocates and queries what
    the warm-up did, and replays to eager's parameters within close_bf16
    (conv1's atomic wgrad fixes no summation order)."""
    from poseidon_amd.proto import Message, parse_text
    from poseidon_amd.solver.solver import SGDSolver

    data, labels = _net_inputs()

    def train(graphed):
        with _rowfused(True):
            pa.init(device="cuda", seed=7, compute_dtype=torch.bfloat16)
            sp = Message("SolverParameter", base_lr=0.01, lr_policy="fixed",
                         momentum=0.9, weight_decay=0.0005, max_iter=100,
                         display=0, snapshot=0)
            sp.net_param = parse_text("NetParameter", _NET)
            s = SGDSolver(sp, verbose=False)
            s.net.blobs["data"].data = data.to(DEV, torch.bfloat16)
            s.net.blobs["label"].data = labels.to(DEV)
            s.net.layers[0]._filled = True
            s.net.layers[0].refill = [False, False]
            if graphed:
                assert s.enable_graph() is True
            s.step(4)
            s.step(2)
            torch.cuda.synchronize()
            if graphed:
                assert s._use_graph and s._graph is not None
            plan = ops.conv_plan((4, 3, 19, 21), (16, 3, 5, 5), (2, 2),
                                 (0, 0), 1, True)
            assert plan["rowfused"]
            return [p.blob.data.detach().cpu().clone()
                    for p in s.net.learnable_params]

    try:
        eager = train(False)
        graph = train(True)
    finally:
        pa.init(device="cpu", compute_dtype=torch.float32)
    for k, (pg, pe) in enumerate(zip(graph, eager)):
        close_bf16(pg, pe, rtol=1e-2, atol=1e-2, what=f"param {k}")


def test_deterministic_mode_keeps_the_column_matrix():
    c = _case("conv1-39-np256")
    xg = c["x"].to(DEV, torch.bfloat16)
    wg = c["w"].to(DEV)
    dyg = c["dy"].to(DEV, torch.bfloat16)
    was = ops.deterministic()
    try:
        with _rowfused(True):
            ops.set_deterministic(True)
            plan = _plan(c)
            assert not plan["rowfused"]
            ops.float_atomic_launches(reset=True)
            _, (slot, _) = ops.conv2d_forward_ex(xg, wg, None, c["stride"],
                                                 c["pad"], 1)
            assert tuple(slot.shape) == (plan["NP"], plan["ld_col"])
            dw = torch.zeros_like(wg)
            ops.conv2d_backward_weight_acc(xg, slot, dyg, dw, None,
                                           c["stride"], c["pad"], 1)
            torch.cuda.synchronize()
            assert ops.float_atomic_launches() == 0
        close_bf16(dw, c["dw"], rtol=1e-2, atol=1e-2, what="deterministic dW")
    finally:
        ops.set_deterministic(was)


def test_defaults():
    """At the default threshold the small shapes keep their column matrix
    (the existing tests read it) whatever the switch says, and AlexNet
    conv1's shape is row-fused exactly when the switch is on -- from the plan
    alone, nothing is launched. The switch itself starts as
    PS_ROWFUSED_CONV says, on when unset."""
    import os
    env = os.environ.get("PS_ROWFUSED_CONV")
    assert ops.rowfused_conv() is (env is None or env.strip() not in ("", "0"))
    assert ops.rowfused_threshold() == ops.ROWFUSED_THRESHOLD_DEFAULT
    shape = ((256, 3, 227, 227), (96, 3, 11, 11), (4, 4), (0, 0), 1)
    was = ops.rowfused_conv()
    try:
        for on in (True, False):
            ops.set_rowfused_conv(on)
            for name in _NAMES:
                assert not _plan(_case(name))["rowfused"], name
            alex = ops.conv_plan(*shape, True)
            assert alex["rowfused"] is on
            assert not alex["packed"] and not alex["implicit"]
            assert alex["wk_ld"] == 384 and alex["Kgw"] == 384
            assert not ops.conv_plan(*shape, False)["rowfused"]  # fp32
    finally:
        ops.set_rowfused_conv(was)
