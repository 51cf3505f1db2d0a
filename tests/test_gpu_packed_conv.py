"""Packed small-channel first-layer convolution (no column matrix; behind
set_packed_conv, default off) against torch's CPU convolution, beside the
materialized path, whose rowstage im2col reads x in any layout.

Both GPU paths see the same bf16-rounded x / w / dy and accumulate the same
products in fp32, so both get the bound tests/test_gpu_bf16.py::test_conv_bf16
allows the conv forward, wgrad and bias gradient: close_bf16 with rtol = atol
= 1e-2. The references are computed once per case, in fp32 on the CPU.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

import poseidon_amd as pa
from poseidon_amd.ops import functional as ops
from test_gpu_bf16 import close_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (name, N, C, H, W, Co, kh, kw, stride, pad)
_CASES = [
    # AlexNet conv1's kernel on a small image; NP = 2*7*7 = 98 is no multiple
    # of 64, so the wgrad takes the generic gather GEMM
    ("conv1-35-n2", 2, 3, 35, 35, 96, 11, 11, 4, 0),
    # the same image at N = 4 (NP = 196) ...
    ("conv1-35-n4", 4, 3, 35, 35, 96, 11, 11, 4, 0),
    # ... and the size at which N = 4 gives NP = 4*8*8 = 256, a multiple of
    # 64: the tr16 gather wgrad runs (M0 = 96 -> bm = 32)
    ("conv1-39-np256", 4, 3, 39, 39, 96, 11, 11, 4, 0),
    # M edges of the tr16 wgrad: 16 is the smallest M0, 80 gives bm = 16
    ("conv1-39-co16", 4, 3, 39, 39, 16, 11, 11, 4, 0),
    ("conv1-39-co80", 4, 3, 39, 39, 80, 11, 11, 4, 0),
    # the host program's geometries (tests/packed_conv_host.cpp)
    ("11x11-w19-h15", 2, 3, 15, 19, 24, 11, 11, 4, 0),   # odd W, odd kw
    ("7x7-s2-p3-w14", 2, 3, 14, 14, 16, 7, 7, 2, 3),     # odd pw, even W
    ("4x4-s2-p1", 2, 3, 10, 10, 16, 4, 4, 2, 1),         # even kw
    ("c1-5x5-s2-p2", 3, 1, 11, 11, 16, 5, 5, 2, 2),
    ("c4-3x3-s2-w9", 2, 4, 9, 9, 16, 3, 3, 2, 0),        # reaches last pixel
]


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _q(t):  # what the bf16 kernels see, as fp32
    return t.to(torch.bfloat16).float()


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
    # |dy|^T |col|: scales the fp32 reassociation bound between two GPU runs
    dw_abs = torch.nn.grad.conv2d_weight(x.abs(), w.shape, dy.abs(),
                                         stride=s, padding=p)
    return dict(x=x, w=w, b=b, dy=dy, stride=(s, s), pad=(p, p),
                y_nobias=y_nobias, y_bias_relu=F.relu(y_nobias + b.view(1, -1, 1, 1)),
                dw=dw, db=dy.sum(dim=(0, 2, 3)), dw_abs=dw_abs,
                NP=N * y_nobias.shape[2] * y_nobias.shape[3])


class _packed:
    """The packed switch on or off; back to its default (off) after."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        ops.set_packed_conv(self.on)

    def __exit__(self, *exc):
        ops.set_packed_conv(False)


def _plan(c):
    return ops.conv_plan(c["x"].shape, c["w"].shape, c["stride"], c["pad"], 1,
                         True)


def _check_slot(c, slot, packed):
    plan = _plan(c)
    N, _, H, _ = c["x"].shape
    if packed:
        # the packed input, not a column matrix
        assert plan["packed"] and not plan["implicit"]
        assert slot.dim() == 4
        assert tuple(slot.shape) == (N, H, plan["pk_W"], 8)
    else:
        assert not plan["packed"]
        assert tuple(slot.shape) == (plan["NP"], plan["ld_col"])


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "colT"])
@pytest.mark.parametrize("name", [c[0] for c in _CASES])
def test_forward_and_wgrad(name, packed):
    c = _case(name)
    xg = c["x"].to(DEV, torch.bfloat16)
    wg, bg = c["w"].to(DEV), c["b"].to(DEV)
    dyg = c["dy"].to(DEV, torch.bfloat16)
    with _packed(packed):
        y0, (slot, _) = ops.conv2d_forward_ex(xg, wg, None, c["stride"],
                                              c["pad"], 1)
        y1, _ = ops.conv2d_forward_ex(xg, wg, bg, c["stride"], c["pad"], 1,
                                      fuse_relu=True)
        _check_slot(c, slot, packed)
        dw = torch.zeros_like(wg)
        db = torch.zeros_like(bg)
        ops.conv2d_backward_weight_acc(xg, slot, dyg, dw, db, c["stride"],
                                       c["pad"], 1)
        torch.cuda.synchronize()
    assert y0.dtype == torch.bfloat16
    close_bf16(y0, c["y_nobias"], rtol=1e-2, atol=1e-2, what=f"{name} fwd")
    close_bf16(y1, c["y_bias_relu"], rtol=1e-2, atol=1e-2,
               what=f"{name} fwd bias+relu")
    close_bf16(dw, c["dw"], rtol=1e-2, atol=1e-2, what=f"{name} dW")
    close_bf16(db, c["db"], rtol=1e-2, atol=1e-2, what=f"{name} db")


def test_input_layouts():
    """The pack kernel reads x through its strides: NCHW, channels-last and
    a non-dense view give the same xp."""
    c = _case("7x7-s2-p3-w14")
    xg = c["x"].to(DEV, torch.bfloat16)
    wide = torch.zeros(2, 5, 14, 20, device=DEV, dtype=torch.bfloat16)
    wide[:, 1:4, :, 3:17] = xg
    with _packed(True):
        slots = [ops.conv2d_forward_ex(v, c["w"].to(DEV), None, c["stride"],
                                       c["pad"], 1)[1][0]
                 for v in (xg, xg.contiguous(memory_format=torch.channels_last),
                           wide[:, 1:4, :, 3:17])]
    assert torch.equal(slots[0], slots[1]) and torch.equal(slots[0], slots[2])
    # pad pixels, the unused channel slot and the right edge are zeros
    xp = slots[0].float().cpu()
    assert xp[..., 3].abs().max() == 0 and xp[..., 7].abs().max() == 0
    assert xp[:, :, 0, :].abs().max() == 0  # pw = 3: chunk 0 is padding
    assert xp[:, :, 1, :4].abs().max() == 0
    assert torch.equal(xp[:, :, 1, 4:7], c["x"][:, :, :, 0].permute(0, 2, 1))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("name", ["7x7-s2-p3-w14", "11x11-w19-h15",
                                  "c1-5x5-s2-p2"])
def test_rowstage_im2col_reads_any_layout(name, dtype):
    """The materialized path of a small-channel first layer stages x through
    its strides (no channels-last copy): NCHW, channels-last and a non-dense
    view give the same column matrix, pad columns zero."""
    c = _case(name)
    xg = c["x"].to(DEV, dtype)
    N, C, H, W = xg.shape
    wide = torch.zeros(N, C + 2, H, W + 6, device=DEV, dtype=dtype)
    wide[:, 1:C + 1, :, 3:W + 3] = xg
    with _packed(False):
        cols = [ops.conv2d_forward_ex(v, c["w"].to(DEV), None, c["stride"],
                                      c["pad"], 1)[1][0]
                for v in (xg, xg.contiguous(memory_format=torch.channels_last),
                          wide[:, 1:C + 1, :, 3:W + 3])]
    plan = ops.conv_plan(xg.shape, c["w"].shape, c["stride"], c["pad"], 1,
                         dtype == torch.bfloat16)
    assert tuple(cols[0].shape) == (plan["NP"], plan["ld_col"])
    assert torch.equal(cols[0], cols[1]) and torch.equal(cols[0], cols[2])
    # against torch's unfold (rows (n, oh, ow), columns (ky, kx, c))
    kh, kw = c["w"].shape[2:]
    ref = F.unfold(c["x"], (kh, kw), padding=c["pad"], stride=c["stride"])
    ref = ref.view(N, C, kh * kw, -1).permute(0, 3, 2, 1).reshape(
        plan["NP"], plan["Kcol"])
    got = cols[0].float().cpu()
    assert torch.equal(got[:, :plan["Kcol"]], ref)
    assert got[:, plan["Kcol"]:].abs().sum() == 0


def test_wgrad_follows_the_forward_not_the_switch():
    c = _case("conv1-39-np256")
    xg = c["x"].to(DEV, torch.bfloat16)
    wg = c["w"].to(DEV)
    dyg = c["dy"].to(DEV, torch.bfloat16)
    with _packed(True):
        _, (slot, _) = ops.conv2d_forward_ex(xg, wg, None, c["stride"],
                                             c["pad"], 1)
        assert slot.dim() == 4
        ops.set_packed_conv(False)  # flipped between forward and backward
        dw = torch.zeros_like(wg)
        ops.conv2d_backward_weight_acc(xg, slot, dyg, dw, None, c["stride"],
                                       c["pad"], 1)
    close_bf16(dw, c["dw"], rtol=1e-2, atol=1e-2, what="dW after switch-off")
    with _packed(False):
        _, (colT, _) = ops.conv2d_forward_ex(xg, wg, None, c["stride"],
                                             c["pad"], 1)
        assert colT.dim() == 2
        ops.set_packed_conv(True)   # and the other way round
        dw = torch.zeros_like(wg)
        ops.conv2d_backward_weight_acc(xg, colT, dyg, dw, None, c["stride"],
                                       c["pad"], 1)
    close_bf16(dw, c["dw"], rtol=1e-2, atol=1e-2, what="dW after switch-on")


@pytest.mark.parametrize("name", ["conv1-39-np256", "7x7-s2-p3-w14"])
def test_persistent_buffers_match_per_layer_route(name):
    """wk from repack_mt and dW from a persistent dwk through unpack_mt, two
    iterations running, against the per-layer kernels. The two routes sum
    the same fp32 products, in an order the split-K atomics do not fix:
    they may differ by the reassociation bound 2 * NP * 2^-24 * |dy|^T|col|
    per element, nothing more."""
    c = _case(name)
    xg = c["x"].to(DEV, torch.bfloat16)
    wg, bg = c["w"].to(DEV), c["b"].to(DEV)
    dyg = c["dy"].to(DEV, torch.bfloat16)
    Co, C, kh, kw = wg.shape
    bound = (2.0 * c["NP"] * 2.0 ** -24) * c["dw_abs"] + 1e-30
    with _packed(True):
        plan = _plan(c)
        assert plan["packed"]
        y_l, (slot_l, _) = ops.conv2d_forward_ex(xg, wg, bg, c["stride"],
                                                 c["pad"], 1)
        dw_l = torch.zeros_like(wg)
        ops.conv2d_backward_weight_acc(xg, slot_l, dyg, dw_l, None,
                                       c["stride"], c["pad"], 1)

        wk = torch.zeros(Co, plan["wk_ld"], device=DEV, dtype=torch.bfloat16)
        wkT = torch.empty(kh * kw * C, Co, device=DEV, dtype=torch.bfloat16)
        dwk = torch.zeros(Co, plan["Kgw"], device=DEV)
        dw = torch.zeros_like(wg)
        layout = ops.khwc_layout(C, kw, True)
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
            assert bool((err <= bound).all()), \
                f"iteration {it}: max |dW_mt - dW_layer| = {err.max():.3e}"
            close_bf16(dw, c["dw"], rtol=1e-2, atol=1e-2, what="dW via mt")


def test_net_runs_packed_first_layer():
    """Net-level plumbing: the persistent wk / dwk buffers and the
    multi-tensor repack / deferred unpack tables carry the packed layout,
    and the net computes what it computes with the switch off."""
    from poseidon_amd.core.net import Net, TRAIN
    from poseidon_amd.proto import parse_text

    text = """
        name: "packed1"
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
    data = _q(_rnd(4, 3, 19, 21, seed=41))
    labels = torch.tensor([0.0, 2.0, 4.0, 1.0]).view(4, 1, 1, 1)

    def run(packed):
        with _packed(packed):
            pa.init(device="cuda", seed=7, compute_dtype=torch.bfloat16)
            net = Net(parse_text("NetParameter", text), phase=TRAIN,
                      verbose=False)
            net.blobs["data"].data = data.to(DEV, torch.bfloat16)
            net.blobs["label"].data = labels.to(DEV)
            net.layers[0]._filled = True
            net.layers[0].refill = [False, False]
            convs = [l for l in net.layers if l.type_name == "CONVOLUTION"]
            for it in range(2):
                loss = net.forward()
                net.zero_param_diffs()
                net.backward()
                for l in convs:  # as the single-GPU solver runs them
                    l.defer_unpack = True
            torch.cuda.synchronize()
            c1 = convs[0]
            # 5x5 on 3 channels: the packed rows (5*3*8 = 120) and the plain
            # ones (75) both round up to 128 -- only the recorded layout
            # tells the two scratch formats apart
            assert c1._dwk_packed is packed
            assert c1._dwk_layout == ((6, 4) if packed else (5, 3))
            assert c1._wk_cache[0].shape[1] == 128
            assert c1._dwk_cache.shape[1] == 128
            assert convs[1]._dwk_packed is False
            return loss, [p.blob.diff.clone() for p in net.learnable_params]

    try:
        loss_p, diffs_p = run(True)
        loss_m, diffs_m = run(False)
    finally:
        pa.init(device="cpu", compute_dtype=torch.float32)
    close_bf16(torch.tensor(loss_p), torch.tensor(loss_m), rtol=1e-2,
               atol=1e-2, what="loss")
    for dp, dm in zip(diffs_p, diffs_m):
        close_bf16(dp, dm, rtol=1e-2, atol=1e-2, what="param diff")
