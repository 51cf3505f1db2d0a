"""Row-fused conv window staging on the GPU (conv_rowfused.hip: rf_load_x /
rf_store_x). A vector that runs over a row end is fetched with ONE 16 B load
that also brings in the neighbouring row's pixels -- or, at the ends of x,
with 8 two-byte loads from clamped pixels -- and a register mask zeroes what
lies outside the row. So x here is always a view into a larger NaN-filled
buffer: a NaN image before it and one after it, and NaN row padding where
the view has any. An element the mask lets through shows up as a NaN in y
and dW.

Every case forces the path as tests/test_gpu_rowfused_conv.py does (switch,
threshold and grid cap put back) and asserts its checks: the forward is
torch.equal to the materialized im2col + GEMM forward, dW is within the
reassociation bound 2 * NP * 2^-24 * (|dy|^T |col|) of the materialized dW,
and both pass close_bf16 (rtol = atol = 1e-2) against the CPU fp32
reference. References are computed once per case."""

import functools

import pytest
import torch
import torch.nn.functional as F

from poseidon_amd.ops import functional as ops
from test_gpu_bf16 import close_bf16
from test_gpu_packed_conv import _q, _rnd
from test_gpu_rowfused_conv import _is_sentinel, _rowfused

pytestmark = pytest.mark.gpu
DEV = "cuda"

# name: (N, C, H, W, Co, k, stride, pad, layout, blocks)
#   layout "nchw": rows of W; ("rows", S): rows of S > W elements;
#   "nhwc": channels-last. blocks: cap on the persistent grid (0 = auto)
_CASES = {
    # the right edge only, as AlexNet's conv1: 35 = 4 vectors + 3 pixels
    "11x11-s4-w35": (2, 3, 35, 35, 16, 11, 4, 0, "nchw", 0),
    # both edges, odd pad
    "7x7-s2-p3-w14": (2, 3, 14, 14, 16, 7, 2, 3, "nchw", 0),
    # one image: the first and the last vector of x's span
    "3x3-p1-n1-w13": (1, 3, 12, 13, 16, 3, 1, 1, "nchw", 0),
    # a row shorter than a vector, and one equal to a vector
    "3x3-p1-w6": (2, 3, 9, 6, 16, 3, 1, 1, "nchw", 0),
    "3x3-p1-w8": (2, 3, 9, 8, 16, 3, 1, 1, "nchw", 0),
    # segment mode: the second segment starts at pixel 127, not a multiple
    # of 8
    "3x3-p1-w130": (2, 3, 6, 130, 16, 3, 1, 1, "nchw", 0),
    # rows padded to 24 elements
    "3x3-p1-w20-rows24": (2, 3, 12, 20, 16, 3, 1, 1, ("rows", 24), 0),
    # channels-last: every vector takes the two-byte loads
    "11x11-s4-w19-nhwc": (2, 3, 15, 19, 16, 11, 4, 0, "nhwc", 0),
    # 80 tiles on 3 blocks, 27 tiles a block: the staging double buffer over
    # many tiles
    "3x3-p1-n8-h80-w16": (8, 3, 80, 16, 16, 3, 1, 1, "nchw", 3),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and CPU fp32 references of one case, computed once."""
    N, C, H, W, Co, k, s, p, layout, blocks = _CASES[name]
    x = _q(_rnd(N, C, H, W, seed=61))
    w = _q(_rnd(Co, C, k, k, seed=62, scale=0.2))
    b = _rnd(Co, seed=63)
    y_nobias = F.conv2d(x, w, None, stride=s, padding=p)
    dy = _q(_rnd(*y_nobias.shape, seed=64))
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=s, padding=p)
    dw_abs = torch.nn.grad.conv2d_weight(x.abs(), w.shape, dy.abs(),
                                         stride=s, padding=p)
    NP = N * y_nobias.shape[2] * y_nobias.shape[3]
    return dict(x=x, w=w, b=b, dy=dy, stride=(s, s), pad=(p, p),
                layout=layout, blocks=blocks, y_nobias=y_nobias,
                y_bias_relu=F.relu(y_nobias + b.view(1, -1, 1, 1)),
                dw=dw, bound=(2.0 * NP * 2.0 ** -24) * dw_abs + 1e-30)


def _nan_framed(x, layout):
    """x's values as a view into a NaN-filled buffer: one NaN image before
    and one after, NaN row padding for ("rows", S)."""
    N, C, H, W = x.shape
    xg = x.to(DEV, torch.bfloat16)
    if layout == "nhwc":
        buf = torch.full((N + 2, H, W, C), float("nan"), device=DEV,
                         dtype=torch.bfloat16)
        view = buf[1:N + 1].permute(0, 3, 1, 2)
    else:
        S = W if layout == "nchw" else layout[1]
        buf = torch.full((N + 2, C, H, S), float("nan"), device=DEV,
                         dtype=torch.bfloat16)
        view = buf[1:N + 1, :, :, :W]
    view.copy_(xg)
    assert torch.equal(view, xg) and bool(torch.isnan(buf[0]).all())
    assert bool(torch.isnan(buf[-1]).all())
    return view


def _run(c, on, x):
    """y without bias, y with bias + ReLU, the cache slot and dW of one
    path."""
    wg, bg = c["w"].to(DEV), c["b"].to(DEV)
    dyg = c["dy"].to(DEV, torch.bfloat16)
    with _rowfused(on, c["blocks"] if on else 0):
        y0, (slot, _) = ops.conv2d_forward_ex(x, wg, None, c["stride"],
                                              c["pad"], 1)
        y1, _ = ops.conv2d_forward_ex(x, wg, bg, c["stride"], c["pad"], 1,
                                      fuse_relu=True)
        dw = torch.zeros_like(wg)
        ops.conv2d_backward_weight_acc(x, slot, dyg, dw, None, c["stride"],
                                       c["pad"], 1)
        torch.cuda.synchronize()
    return y0, y1, slot, dw


@pytest.mark.parametrize("name", list(_CASES))
def test_staged_window_masks_its_neighbours(name):
    c = _case(name)
    x = _nan_framed(c["x"], c["layout"])
    # the materialized path on a dense copy of the same values
    m0, m1, mslot, mdw = _run(c, False, c["x"].to(DEV, torch.bfloat16))
    y0, y1, slot, dw = _run(c, True, x)
    assert _is_sentinel(slot) and not _is_sentinel(mslot)
    n_nan = int(torch.isnan(y0.float()).sum()) + int(torch.isnan(dw).sum())
    print(f"{name}: NaNs in y / dW {n_nan}, max |y - y_mat| "
          f"{(y0.float() - m0.float()).abs().max():.3e}")
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
