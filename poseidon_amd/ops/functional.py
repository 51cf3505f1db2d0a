"""Op dispatch: hand-written HIP/CDNA4 kernels on GPU, plain fp32 torch on CPU.

The CPU path is the numerics reference for every GPU kernel (tests compare
the two). The GPU path REQUIRES the compiled in-tree extension
(poseidon_amd/ops/_hip) -- it raises rather than silently falling back to
eager torch, so a GPU run that passes is running our CDNA4 kernels.

Semantics mirror the reference layer math:
  conv      /root/reference/src/caffe/layers/conv_layer.{cpp,cu}
  pooling   /root/reference/src/caffe/layers/pooling_layer.cu (Caffe ceil
            geometry + far-edge-clipped AVE pool_size)
  lrn       /root/reference/src/caffe/layers/lrn_layer.cu
  softmax   /root/reference/src/caffe/layers/softmax_layer.cu
  sgd       /root/reference/src/caffe/solver.cpp:815-892 (fused here)
"""

from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

_EXT = None
_EXT_ERR: Optional[str] = None


def _ext():
    global _EXT, _EXT_ERR
    if _EXT is None and _EXT_ERR is None:
        try:
            from . import _backend
            _EXT = _backend.load()
        except Exception as e:  # noqa: BLE001
            _EXT_ERR = str(e)
    if _EXT is None:
        raise RuntimeError(
            "poseidon_amd HIP extension is not built/loadable but a GPU op was "
            f"requested. Build it with `python setup.py build_ext --inplace` "
            f"(PYTORCH_ROCM_ARCH=gfx950). Original error: {_EXT_ERR}")
    return _EXT


def set_implicit_gemm(on: bool) -> None:
    """Toggle implicit-GEMM convolution (im2col gathered inside the MFMA
    GEMM staging; no column matrix). Default off: the materialized pipeline
    measures faster on current shapes."""
    _ext().set_implicit_gemm(bool(on))


def set_implicit_threshold(bytes_: int) -> None:
    """colT size above which a conv auto-selects implicit GEMM per layer."""
    if ext_available():
        _ext().set_implicit_threshold(int(bytes_))


# bumped by every setter that can change a conv's khwc weight layout: Net
# keys its persistent wk buffers on it
_conv_policy_epoch = 0


def set_packed_conv(on: bool) -> None:
    """Toggle the packed first-layer path (G==1, C<=4, even horizontal
    stride, bf16): forward and wgrad gather from a pair-packed copy of the
    input instead of building a column matrix. Default off (it measures
    slower on AlexNet conv1, docs/performance.md item 20); the environment
    variable PS_PACKED_CONV=0/1 sets it at import."""
    global _conv_policy_epoch
    _ext().set_packed_conv(bool(on))
    _conv_policy_epoch += 1


ROWFUSED_THRESHOLD_DEFAULT = 256 << 20


def set_rowfused_conv(on: bool) -> None:
    """Toggle the row-fused first-layer path (bf16, G==1, C % 8 != 0, not
    1x1): forward and wgrad build their MFMA operands from input rows staged
    in LDS, and no column matrix is written or read. Default on for layers
    whose column matrix reaches set_rowfused_threshold (AlexNet / CaffeNet
    conv1, docs/performance.md item 27); never taken in deterministic mode. The khwc weight layout is the materialized path's,
    so no persistent buffer changes. The environment variable
    PS_ROWFUSED_CONV=0/1 sets it at import."""
    if ext_available():
        _ext().set_rowfused_conv(bool(on))


def rowfused_conv() -> bool:
    return bool(_ext().rowfused_conv()) if ext_available() else False


def set_rowfused_threshold(bytes_: int) -> None:
    """Column-matrix size from which a first layer goes row-fused."""
    if ext_available():
        _ext().set_rowfused_threshold(int(bytes_))


def rowfused_threshold() -> int:
    return (int(_ext().rowfused_threshold()) if ext_available()
            else ROWFUSED_THRESHOLD_DEFAULT)


def _set_rowfused_blocks(n: int) -> None:
    """Tests only: cap on the row-fused kernels' persistent grid (0 = one
    block per CU), so that a small case walks several tiles per block."""
    if ext_available():
        _ext().set_rowfused_blocks(int(n))


def conv_policy_epoch() -> int:
    return _conv_policy_epoch


# Deterministic mode. The flag itself lives in the extension (one per
# process, initially PS_DETERMINISTIC=1); without the extension -- CPU only,
# where every reduction is ordered anyway -- it is kept here.
_deterministic_cpu = os.environ.get("PS_DETERMINISTIC", "0") not in ("", "0")


def set_deterministic(on: bool) -> None:
    """Opt-in bit-reproducible mode: every float reduction of the HIP kernels
    (split-K GEMMs, column sums, fused bias gradients, the softmax loss) runs
    in an order fixed by the problem shape and the plan instead of by block
    scheduling, so the same steps from the same seed on one GPU in one build
    leave identical bits, eager or graphed. No kernel takes an atomic-float
    path while it is on; a launch that has no ordered form raises. Toggling
    bumps conv_policy_epoch() so nets re-plan their cached tables."""
    global _deterministic_cpu, _conv_policy_epoch
    on = bool(on)
    if on == deterministic():
        return
    if ext_available():
        _ext().set_deterministic(on)
    _deterministic_cpu = on
    _conv_policy_epoch += 1
    from ..core.context import ctx
    ctx().deterministic = on


def deterministic() -> bool:
    if ext_available():
        return bool(_ext().deterministic())
    return _deterministic_cpu


# The fused weight tail (docs/architecture.md): fc weight gradients are
# written straight into the param diff, sole-owner diffs leave the zero
# table, and the SGD kernel writes the fc bf16 shadows. Off reproduces the
# accumulate / full-repack step bit for bit. Read at every step by the
# layers, the net and the solver, so it may be flipped between eager steps;
# a captured graph keeps what it was captured with.
_fused_weight_tail = os.environ.get("PS_WEIGHT_TAIL", "1") not in ("", "0")


def set_fused_weight_tail(on: bool) -> None:
    global _fused_weight_tail
    _fused_weight_tail = bool(on)


def fused_weight_tail() -> bool:
    return _fused_weight_tail


def gemm_plan(M: int, N: int, K: int, a_klast: bool, b_klast: bool,
              bf16: bool) -> dict:
    """The launch plan of the test GEMM entry for this shape right now:
    tr16, splitk, ws_elems, bm, bn, kchunk, grid_z."""
    return dict(_ext().gemm_plan(int(M), int(N), int(K), bool(a_klast),
                                 bool(b_klast), bool(bf16)))


def float_atomic_launches(reset: bool = False) -> int:
    """Launches so far of kernel instantiations that add floats atomically
    (LDS or global). A host-side counter bumped at launch time: nothing is
    read from the device. Stays put across any work done in deterministic
    mode. reset=True also sets it back to zero."""
    if not ext_available():
        return 0
    return int(_ext().float_atomic_launches(bool(reset)))


def khwc_layout(Cg: int, kw: int, packed: bool) -> Tuple[int, int]:
    """(tap-row width, channel slots) of a conv's khwc weight rows."""
    kw_ld, c_ld = _ext().khwc_layout(int(Cg), int(kw), bool(packed))
    return int(kw_ld), int(c_ld)


DGRAD_FWD_THRESHOLD_DEFAULT = 128 << 20


def set_dgrad_fwd_threshold(bytes_: int) -> None:
    """dcolT size above which a stride-1 conv dgrad runs as a forward conv
    of dy with rotated weights (no dcolT, no col2im)."""
    if ext_available():
        _ext().set_dgrad_fwd_threshold(int(bytes_))


def ext_available() -> bool:
    try:
        _ext()
        return True
    except RuntimeError:
        return False


# ---------------------------------------------------------------------------
# Geometry helpers (Caffe pooling/conv shape rules)
# ---------------------------------------------------------------------------

def conv_out_size(h: int, k: int, p: int, s: int) -> int:
    return (h + 2 * p - k) // s + 1


def pool_out_size(h: int, k: int, p: int, s: int) -> Tuple[int, bool]:
    """Caffe pooled size: ceil((h+2p-k)/s)+1, minus 1 when the last window
    would start in the padding (pooling_layer.cpp:64-77)."""
    out = int(math.ceil((h + 2 * p - k) / s)) + 1
    if p > 0 and (out - 1) * s >= h + p:
        out -= 1
    return out


# ---------------------------------------------------------------------------
# Convolution
# ---------------------------------------------------------------------------

def conv2d_forward_ex(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor],
                      stride: Tuple[int, int], pad: Tuple[int, int],
                      groups: int, fuse_relu: bool = False, cached=None):
    """Returns (y, colT_cache). colT is the im2col matrix on GPU (reused by
    the backward GEMMs) -- or, in its place, the empty implicit-GEMM
    sentinel or the 4-D packed input of a packed first layer, which tell
    the wgrad what the forward did; None on CPU. fuse_relu clamps the
    output in the GEMM epilogue (used by the Net-level conv+ReLU fusion
    pass)."""
    if x.is_cuda:
        wk_c, wkT_c = cached if cached is not None else (None, None)
        y, colT, wkT = _ext().conv2d_forward_ex(x, w, b, stride[0], stride[1],
                                                pad[0], pad[1], groups,
                                                fuse_relu, wk_c, wkT_c)
        return y, (colT, wkT)
    y = F.conv2d(x, w, b, stride=stride, padding=pad, groups=groups)
    if fuse_relu:
        y = F.relu(y)
    return y, None


def conv2d_backward_input(w: torch.Tensor, dy: torch.Tensor,
                          x_shape, stride, pad, groups: int,
                          wkT_cache=None, dx_out=None) -> torch.Tensor:
    if dy.is_cuda:
        return _ext().conv2d_backward_input(w, dy, list(x_shape), stride[0],
                                            stride[1], pad[0], pad[1], groups,
                                            wkT_cache, dx_out)
    return torch.nn.grad.conv2d_input(list(x_shape), w, dy, stride=stride,
                                      padding=pad, groups=groups)


def conv2d_backward_weight_acc(x: torch.Tensor, colT, dy: torch.Tensor,
                               dw: torch.Tensor, db: Optional[torch.Tensor],
                               stride, pad, groups: int,
                               dwk_buf: Optional[torch.Tensor] = None,
                               skip_unpack: bool = False,
                               skip_db: bool = False
                               ) -> Optional[torch.Tensor]:
    """Accumulates into dw (NCHW) and db. Returns the khwc dwk scratch used
    on GPU: hand it back as dwk_buf on later iterations (keeping it zeroed
    each iteration via the net-level zero table) to skip the per-GEMM
    split-K memset."""
    if dy.is_cuda:
        return _ext().conv2d_backward_weight_acc(
            x, colT, dy, dw, db, stride[0], stride[1], pad[0], pad[1],
            groups, dwk_buf, skip_unpack, skip_db)
    dw.add_(torch.nn.grad.conv2d_weight(x, list(dw.shape), dy, stride=stride,
                                        padding=pad, groups=groups))
    if db is not None:
        db.add_(dy.sum(dim=(0, 2, 3)))
    return None


# ---------------------------------------------------------------------------
# Inner product (FC): y[M,N] = x[M,K] @ w[N,K]^T + b
# ---------------------------------------------------------------------------

def linear_forward(x: torch.Tensor, w: torch.Tensor,
                   b: Optional[torch.Tensor],
                   fuse_relu: bool = False,
                   w_shadow: Optional[torch.Tensor] = None) -> torch.Tensor:
    if x.is_cuda:
        return _ext().linear_forward(x, w, b, fuse_relu, w_shadow)
    y = x.matmul(w.t())
    if b is not None:
        y = y + b
    if fuse_relu:
        y = F.relu(y)
    return y


def linear_backward(x: torch.Tensor, w: torch.Tensor, dy: torch.Tensor,
                    need_dx: bool, need_dw: bool, has_bias: bool,
                    w_shadow: Optional[torch.Tensor] = None,
                    dw_acc: Optional[torch.Tensor] = None,
                    dw_out: Optional[torch.Tensor] = None):
    """dw_acc: fp32 [N,K] buffer the weight grad is ACCUMULATED into
    (beta=1 GEMM). dw_out: fp32 contiguous [N,K] buffer the weight grad is
    WRITTEN into (beta=0; its old contents are never read). With either,
    the returned dw is None."""
    if dy.is_cuda:
        return _ext().linear_backward(x, w, dy, need_dx, need_dw, has_bias,
                                      w_shadow, dw_acc, dw_out)
    dx = dy.matmul(w) if need_dx else None
    dw = dy.t().matmul(x) if need_dw else None
    if dw is not None and dw_out is not None:
        dw_out.copy_(dw)
        dw = None
    elif dw is not None and dw_acc is not None:
        dw_acc.add_(dw)
        dw = None
    db = dy.sum(dim=0) if has_bias else None
    return dx, dw, db


def gemm_at_b(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a[M,N]^T-free outer-product GEMM used by SFB reconstruction:
    returns a^T @ b for a[B,N], b[B,K] -> [N,K]."""
    if a.is_cuda:
        return _ext().gemm_at_b(a, b)
    return a.t().matmul(b)


# ---------------------------------------------------------------------------
# Pooling
# ---------------------------------------------------------------------------

def _unfold_pad(x, k, s, p, pad_value: float, Ho: int, Wo: int):
    """Pad so that all Ho/Wo Caffe ceil-mode windows exist (the last window
    may extend past H+p), then unfold."""
    H, W = x.shape[2], x.shape[3]
    far_h = max(p[0], (Ho - 1) * s[0] + k[0] - H - p[0])
    far_w = max(p[1], (Wo - 1) * s[1] + k[1] - W - p[1])
    xp = F.pad(x, (p[1], far_w, p[0], far_h), value=pad_value)
    return xp.unfold(2, k[0], s[0]).unfold(3, k[1], s[1])


def pool_max_forward(x, k, s, p):
    if x.is_cuda:
        return _ext().pool_max_forward(x, k[0], k[1], s[0], s[1], p[0], p[1])
    N, C, H, W = x.shape
    Ho = pool_out_size(H, k[0], p[0], s[0])
    Wo = pool_out_size(W, k[1], p[1], s[1])
    win = _unfold_pad(x, k, s, p, float("-inf"), Ho, Wo)[:, :, :Ho, :Wo]
    flat = win.contiguous().view(N, C, Ho, Wo, -1)
    y, idx = flat.max(dim=-1)
    # map window-local argmax to bottom (unpadded) flat index h*W + w
    kh = idx // k[1]
    kw = idx % k[1]
    oh = torch.arange(Ho, device=x.device).view(1, 1, Ho, 1)
    ow = torch.arange(Wo, device=x.device).view(1, 1, 1, Wo)
    h = oh * s[0] - p[0] + kh
    wdx = ow * s[1] - p[1] + kw
    mask = (h * W + wdx).to(torch.int32)
    return y, mask


def pool_max_backward(dy, mask, x_shape, k=None, s_=None, p=None,
                      dx_out=None):
    if dy.is_cuda:
        return _ext().pool_max_backward(dy, mask, list(x_shape), k[0], k[1],
                                        s_[0], s_[1], p[0], p[1], dx_out)
    N, C, H, W = x_shape
    dx = torch.zeros(N, C, H * W, dtype=dy.dtype, device=dy.device)
    dx.scatter_add_(2, mask.view(N, C, -1).long(), dy.view(N, C, -1))
    return dx.view(N, C, H, W)


def _ave_pool_sizes(H, W, k, s, p, Ho, Wo, device):
    oh = torch.arange(Ho, device=device)
    ow = torch.arange(Wo, device=device)
    hstart = oh * s[0] - p[0]
    wstart = ow * s[1] - p[1]
    hend = torch.clamp(hstart + k[0], max=H + p[0])
    wend = torch.clamp(wstart + k[1], max=W + p[1])
    return ((hend - hstart).view(Ho, 1) * (wend - wstart).view(1, Wo)).float()


def pool_ave_forward(x, k, s, p):
    if x.is_cuda:
        return _ext().pool_ave_forward(x, k[0], k[1], s[0], s[1], p[0], p[1])
    N, C, H, W = x.shape
    Ho = pool_out_size(H, k[0], p[0], s[0])
    Wo = pool_out_size(W, k[1], p[1], s[1])
    win = _unfold_pad(x, k, s, p, 0.0, Ho, Wo)[:, :, :Ho, :Wo]
    ssum = win.contiguous().view(N, C, Ho, Wo, -1).sum(dim=-1)
    sizes = _ave_pool_sizes(H, W, k, s, p, Ho, Wo, x.device).to(x.dtype)
    return ssum / sizes


def pool_ave_backward(dy, x_shape, k, s, p):
    if dy.is_cuda:
        return _ext().pool_ave_backward(dy, list(x_shape), k[0], k[1],
                                        s[0], s[1], p[0], p[1])
    N, C, H, W = x_shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    sizes = _ave_pool_sizes(H, W, k, s, p, Ho, Wo, dy.device).to(dy.dtype)
    g = (dy / sizes).view(N * C, 1, Ho, Wo)
    # distribute each output's gradient over its (real-region) window = fold
    Hp = max(H + 2 * p[0], (Ho - 1) * s[0] + k[0])
    Wp = max(W + 2 * p[1], (Wo - 1) * s[1] + k[1])
    cols = g.expand(N * C, k[0] * k[1], Ho, Wo).reshape(N * C, k[0] * k[1], Ho * Wo)
    dxp = F.fold(cols, (Hp, Wp), (k[0], k[1]), stride=(s[0], s[1]))
    dx = dxp[:, :, p[0]:p[0] + H, p[1]:p[1] + W]
    return dx.reshape(N, C, H, W)


def pool_stoch_forward_train(x, k, s, p, rand=None):
    """Stochastic pooling (train): pick an element of each window with
    probability proportional to its value (pooling_layer.cu:81-120)."""
    if x.is_cuda:
        return _ext().pool_stoch_forward_train(x, k[0], k[1], s[0], s[1],
                                               p[0], p[1],
                                               int(torch.randint(0, 2**31 - 1, ()).item()))
    N, C, H, W = x.shape
    Ho = pool_out_size(H, k[0], p[0], s[0])
    Wo = pool_out_size(W, k[1], p[1], s[1])
    win = _unfold_pad(x, k, s, p, 0.0, Ho, Wo)[:, :, :Ho, :Wo]
    flat = win.contiguous().view(N, C, Ho, Wo, -1)
    csum = flat.cumsum(dim=-1)
    total = csum[..., -1:]
    if rand is None:
        rand = torch.rand(N, C, Ho, Wo, 1, device=x.device, dtype=x.dtype)
    thresh = rand * total
    idx = (csum < thresh).sum(dim=-1).clamp(max=k[0] * k[1] - 1)
    y = flat.gather(-1, idx.unsqueeze(-1)).squeeze(-1)
    kh = idx // k[1]
    kw = idx % k[1]
    oh = torch.arange(Ho, device=x.device).view(1, 1, Ho, 1)
    ow = torch.arange(Wo, device=x.device).view(1, 1, 1, Wo)
    h = (oh * s[0] - p[0] + kh).clamp(0, H - 1)
    wdx = (ow * s[1] - p[1] + kw).clamp(0, W - 1)
    mask = (h * W + wdx).to(torch.int32)
    return y, mask


def pool_stoch_forward_test(x, k, s, p):
    if x.is_cuda:
        return _ext().pool_stoch_forward_test(x, k[0], k[1], s[0], s[1], p[0], p[1])
    N, C, H, W = x.shape
    Ho = pool_out_size(H, k[0], p[0], s[0])
    Wo = pool_out_size(W, k[1], p[1], s[1])
    win = _unfold_pad(x, k, s, p, 0.0, Ho, Wo)[:, :, :Ho, :Wo]
    flat = win.contiguous().view(N, C, Ho, Wo, -1)
    num = (flat * flat).sum(-1)
    den = flat.sum(-1)
    return num / (den + torch.finfo(x.dtype).tiny)


# ---------------------------------------------------------------------------
# LRN (across channels)
# ---------------------------------------------------------------------------

def lrn_forward(x, size: int, alpha: float, beta: float):
    if x.is_cuda:
        return _ext().lrn_forward(x, size, alpha, beta)
    N, C, H, W = x.shape
    sq = (x * x).view(N, 1, C, H * W)
    pad = (size - 1) // 2
    # sliding sum over channel dim: conv with ones kernel
    kernel = torch.ones(1, 1, size, 1, dtype=x.dtype, device=x.device)
    ssum = F.conv2d(sq, kernel, padding=(size - 1 - pad, 0))
    ssum = ssum[:, :, :C, :].view(N, C, H, W)
    scale = 1.0 + (alpha / size) * ssum
    y = x * scale.pow(-beta)
    return y, scale


def lrn_backward(x, y, scale, dy, size: int, alpha: float, beta: float):
    if x.is_cuda:
        return _ext().lrn_backward(x, y, scale, dy, size, alpha, beta)
    N, C, H, W = x.shape
    pad = (size - 1) // 2
    ratio = (dy * y / scale).view(N, 1, C, H * W)
    kernel = torch.ones(1, 1, size, 1, dtype=x.dtype, device=x.device)
    acc = F.conv2d(ratio, kernel, padding=(pad, 0))[:, :, :C, :].view(N, C, H, W)
    return dy * scale.pow(-beta) - (2.0 * alpha * beta / size) * x * acc


# ---------------------------------------------------------------------------
# Fused backward tails of a conv block: conv -> relu -> [lrn] -> [max pool].
# One kernel writes the conv's top diff (already masked by the in-place
# ReLU) and adds its column sum into the conv's bias gradient. The CPU path
# is the composition of the ops above.
# ---------------------------------------------------------------------------

def lrn_v8_ok(C: int, size: int) -> bool:
    """Whether the GPU runs this LRN on its vec8 path (what the tails need)."""
    return bool(_ext().lrn_v8_ok(int(C), int(size)))


def set_bwd_tail_blocks(n: int) -> None:
    """Block cap of the tail kernels that sum a bias gradient (0 = default);
    tests lower it to make small tensors stride the grid."""
    _ext().set_bwd_tail_blocks(int(n))


def _bias_acc(dx, db) -> None:
    if db is not None:
        db += dx.sum(dim=(0, 2, 3)).to(db.dtype)


def lrn_backward_tail(x, y, dy, size: int, alpha: float, beta: float,
                      relu: bool = False, db=None, pool=None, dx_out=None):
    """LRN backward with its neighbours folded in. pool = (mask, k, s, p) of
    the MAX pool consuming this LRN's output: dy is then the POOL's top diff.
    relu: x is a post-ReLU conv output, dx is masked by x > 0. db: f32 [C],
    += the column sum of dx. GPU: the vec8 LRN path only (lrn_v8_ok)."""
    if x.is_cuda:
        mask, k, s, p = pool if pool is not None else (None, (0, 0), (0, 0),
                                                       (0, 0))
        return _ext().lrn_backward_tail(x, y, dy, size, alpha, beta, relu, db,
                                        mask, k[0], k[1], s[0], s[1], p[0],
                                        p[1], dx_out)
    if pool is not None:
        mask, k, s, p = pool
        dy = pool_max_backward(dy, mask, x.shape, k, s, p)
    _, scale = lrn_forward(x, size, alpha, beta)
    dx = lrn_backward(x, y, scale, dy, size, alpha, beta)
    if relu:
        dx = relu_backward(x, dx, 0.0)
    _bias_acc(dx, db)
    return dx


def pool_max_backward_tail(dy, mask, x, k, s, p, db=None, dx_out=None):
    """MAX pool backward whose bottom x is a post-ReLU conv output: dx is
    masked by x > 0 and its column sum is added into db (f32 [C])."""
    if dy.is_cuda:
        return _ext().pool_max_backward_tail(dy, mask, x, k[0], k[1], s[0],
                                             s[1], p[0], p[1], db, dx_out)
    dx = relu_backward(x, pool_max_backward(dy, mask, x.shape, k, s, p), 0.0)
    _bias_acc(dx, db)
    return dx


def relu_backward_bias(x, dy, db):
    """Slope-0 ReLU backward (in dy's buffer on the GPU) that also adds the
    column sum of dx into db (f32 [C]): the relu -> conv tail."""
    if x.is_cuda:
        return _ext().relu_backward_bias(x, dy, db)
    dx = relu_backward(x, dy, 0.0)
    _bias_acc(dx, db)
    return dx


# ---------------------------------------------------------------------------
# Softmax + losses
# ---------------------------------------------------------------------------

def softmax_forward(x: torch.Tensor) -> torch.Tensor:
    """Channel softmax per spatial position (softmax_layer.cu)."""
    if x.is_cuda:
        return _ext().softmax_forward(x)
    return F.softmax(x, dim=1)


def softmax_backward(y: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    if y.is_cuda:
        return _ext().softmax_backward(y, dy)
    dot = (dy * y).sum(dim=1, keepdim=True)
    return (dy - dot) * y


def softmax_loss_forward(logits: torch.Tensor, labels: torch.Tensor):
    """Returns (mean NLL over batch as 0-d tensor, probs)."""
    if logits.is_cuda:
        return _ext().softmax_loss_forward(logits, labels)
    prob = F.softmax(logits, dim=1)
    n = logits.shape[0]
    picked = prob[torch.arange(n), labels.long().view(-1)]
    loss = -torch.log(torch.clamp(picked, min=torch.finfo(prob.dtype).tiny)).sum() / n
    return loss, prob


def softmax_loss_backward(prob: torch.Tensor, labels: torch.Tensor,
                          loss_weight: float) -> torch.Tensor:
    if prob.is_cuda:
        return _ext().softmax_loss_backward(prob, labels, loss_weight)
    n = prob.shape[0]
    dx = prob.clone()
    dx[torch.arange(n), labels.long().view(-1)] -= 1.0
    return dx * (loss_weight / n)


# ---------------------------------------------------------------------------
# Elementwise / neuron ops
# ---------------------------------------------------------------------------

def relu_forward(x, negative_slope: float = 0.0):
    if x.is_cuda:
        return _ext().relu_forward(x, negative_slope)
    return F.leaky_relu(x, negative_slope)


def relu_backward(x, dy, negative_slope: float = 0.0,
                  in_place: bool = False):
    """in_place: write dx into dy's buffer (elementwise same-index safe).
    Keeps the grad identity stable for net-level batching."""
    if x.is_cuda:
        return _ext().relu_backward(x, dy, negative_slope, in_place)
    return torch.where(x > 0, dy, dy * negative_slope)


def sigmoid_forward(x):
    if x.is_cuda:
        return _ext().sigmoid_forward(x)
    return torch.sigmoid(x)


def sigmoid_backward(y, dy):
    if y.is_cuda:
        return _ext().sigmoid_backward(y, dy)
    return dy * y * (1 - y)


def tanh_forward(x):
    if x.is_cuda:
        return _ext().tanh_forward(x)
    return torch.tanh(x)


def tanh_backward(y, dy):
    if y.is_cuda:
        return _ext().tanh_backward(y, dy)
    return dy * (1 - y * y)


def bnll_forward(x):
    """log(1 + exp(x)), computed stably (bnll_layer.cu)."""
    if x.is_cuda:
        return _ext().bnll_forward(x)
    return F.softplus(x)


def bnll_backward(x, dy):
    if x.is_cuda:
        return _ext().bnll_backward(x, dy)
    return dy * torch.sigmoid(x)


def dropout_forward(x, ratio: float, seed: int, offset, offset_dev=None):
    """Train-mode dropout. Returns (y, mask) where mask is uint8 keep-mask;
    y = x * mask * 1/(1-ratio). On GPU, offset_dev (int64 device scalar)
    makes the op hipGraph-replayable (fresh mask per replay)."""
    if x.is_cuda:
        if offset_dev is not None:
            return _ext().dropout_forward_offdev(x, ratio, seed, offset_dev)
        return _ext().dropout_forward(x, ratio, seed, offset)
    scale = 1.0 / (1.0 - ratio)
    g = torch.Generator(device="cpu").manual_seed(seed + offset)
    mask = (torch.rand(x.shape, generator=g) >= ratio)
    return x * mask.to(x.dtype) * scale, mask


def dropout_backward(dy, mask, ratio: float):
    if dy.is_cuda:
        return _ext().dropout_backward(dy, mask, ratio)
    return dy * mask.to(dy.dtype) * (1.0 / (1.0 - ratio))


# ---------------------------------------------------------------------------
# Fused SGD update (solver.cpp:858-892 collapsed to one kernel)
#   hist = momentum*hist + local_rate*(grad + decay*w)
#   w   -= hist
# ---------------------------------------------------------------------------

def threshold_forward(x: torch.Tensor, thr: float) -> torch.Tensor:
    if x.is_cuda:
        return _ext().threshold_forward(x, float(thr))
    return (x > thr).to(x.dtype)


def eltwise_max(blobs) -> tuple:
    """Running pairwise max with a u8 argmax mask (ELTWISE MAX,
    eltwise_layer.cu:11 MaxForward semantics)."""
    if blobs[0].is_cuda:
        y = blobs[0].contiguous().clone()
        mask = torch.zeros(y.numel(), dtype=torch.uint8, device=y.device)
        for i, b in enumerate(blobs[1:], start=1):
            _ext().eltwise_max_step(y.view(-1), b.reshape(-1), mask, i)
        return y, mask.view(y.shape)
    stacked = torch.stack(list(blobs))
    y, idx = stacked.max(dim=0)
    return y, idx.to(torch.uint8)


def eltwise_max_backward(dy: torch.Tensor, mask: torch.Tensor,
                         idx: int) -> torch.Tensor:
    if dy.is_cuda:
        return _ext().eltwise_max_backward(dy.reshape(-1),
                                           mask.reshape(-1),
                                           idx).view(dy.shape)
    return dy * (mask == idx).to(dy.dtype)


def contrastive_terms(dist_sq: torch.Tensor, sim: torch.Tensor,
                      margin: float, legacy: bool) -> torch.Tensor:
    """Per-pair contrastive loss terms (contrastive_loss_layer.cu:49)."""
    if dist_sq.is_cuda:
        return _ext().contrastive_forward(dist_sq, sim, float(margin),
                                          bool(legacy))
    m = torch.clamp(margin - (dist_sq if legacy else dist_sq.sqrt()), min=0)
    return torch.where(sim != 0, dist_sq, m if legacy else m * m)


def sgd_update(w: torch.Tensor, grad: torch.Tensor, hist: torch.Tensor,
               local_rate: float, momentum: float, decay: float,
               lr_dev=None) -> None:
    if w.is_cuda:
        if lr_dev is not None:
            _ext().sgd_update_lrdev(w, grad, hist, local_rate, momentum,
                                    decay, lr_dev)
        else:
            _ext().sgd_update(w, grad, hist, local_rate, momentum, decay)
        return
    gw = grad if decay == 0.0 else grad + decay * w
    hist.mul_(momentum).add_(gw, alpha=local_rate)
    w.sub_(hist)


# -- multi-tensor apply: one launch for ALL params (GPU only) ---------------

def sgd_mt_prepare(ws, gs, hs, lr_mults, wds, shadows=None):
    """Build device-resident descriptor/chunk tables for sgd_mt_run. Shapes
    and tensor identities must stay fixed afterwards (they do: param blobs
    are allocated once at net build). shadows: per tensor, a bf16 buffer of
    the same element count that the update also writes the new weight to,
    or None."""
    d, c, n = _ext().sgd_mt_prepare(list(ws), list(gs), list(hs),
                                    [float(v) for v in lr_mults],
                                    [float(v) for v in wds],
                                    list(shadows) if shadows is not None
                                    else [])
    return d, c, int(n.item())


def sgd_mt_run(mt, lr: float, momentum: float, lr_dev=None) -> None:
    desc, chunk, nchunks = mt
    _ext().sgd_mt_run(desc, chunk, nchunks, float(lr), float(momentum),
                      lr_dev)


def conv_plan(x_shape, w_shape, stride, pad, groups: int, bf16: bool) -> dict:
    """The conv layout plan the bindings derive for this problem (column
    stride ld_col, padded weight width wk_ld, implicit / dgrad-as-forward
    choices, ...) under the current implicit-GEMM policy."""
    return _ext().conv_plan(list(x_shape), list(w_shape), list(stride),
                            list(pad), int(groups), bool(bf16))


def repack_mt_prepare(masters, wks, wkTs, Gs, kw_lds=(), c_lds=()):
    """kw_lds / c_lds: the plan's khwc layout per tensor (conv_plan's kw_ld,
    c_ld); empty means every shadow is plain khwc."""
    d, c, n = _ext().repack_mt_prepare(list(masters), list(wks), list(wkTs),
                                       [int(g) for g in Gs],
                                       [int(v) for v in kw_lds],
                                       [int(v) for v in c_lds])
    return d, c, int(n.item())


def repack_mt_run(mt) -> None:
    d, c, n = mt
    _ext().repack_mt_run(d, c, n)


def unpack_mt_prepare(dwks, dws, Cigs, khs, kws, kw_lds=(), c_lds=(),
                      overwrites=()):
    """kw_lds / c_lds: khwc_layout() of each dwk scratch; empty = plain.
    overwrites: per tensor, write dw instead of adding to it; empty = every
    tensor accumulates."""
    d, c, n = _ext().unpack_mt_prepare(list(dwks), list(dws), list(Cigs),
                                       list(khs), list(kws),
                                       [int(v) for v in kw_lds],
                                       [int(v) for v in c_lds],
                                       [bool(v) for v in overwrites])
    return d, c, int(n)


def unpack_mt_run(mt) -> None:
    d, c, n = mt
    _ext().unpack_mt_run(d, c, n)


def colsum_mt_prepare(dys, dbs):
    """(descs, chunks, nchunks, max C, tensors, scratch). The scratch holds
    deterministic mode's per-chunk partials and is sized only when the table
    is prepared with the mode on: prepare again after toggling it."""
    d, c, n, mc, nt, scratch = _ext().colsum_mt_prepare(list(dys), list(dbs))
    return d, c, int(n), int(mc), int(nt), scratch


def colsum_mt_run(mt, bf16: bool) -> None:
    d, c, n, mc, nt, scratch = mt
    _ext().colsum_mt_run(d, c, n, bf16, mc, nt, scratch)


def colsum_acc(dy, db) -> None:
    _ext().colsum_acc(dy, db)


def zero_mt_prepare(tensors):
    d, c, n = _ext().zero_mt_prepare(list(tensors))
    return d, c, int(n.item())


def zero_mt_run(mt) -> None:
    desc, chunk, nchunks = mt
    _ext().zero_mt_run(desc, chunk, nchunks)


# -- blob statistics (solver debug_info) -------------------------------------
# Per tensor: sum of |x| (NaN / Inf propagate), largest finite |x|, number of
# NaN / Inf elements. On the GPU one streaming pass per tensor stores block
# partials to a persistent scratch and blob_stats_finalize sums them in a
# fixed order (stats.hip): no float atomics, no host sync, capturable. The
# CPU path computes the same three numbers with torch, the sum in float64.

class BlobStatsBuffer:
    """The persistent buffers of nslots statistics records. records() is the
    one device-to-host copy."""

    def __init__(self, nslots: int, device) -> None:
        device = torch.device(device)
        self.nslots = int(nslots)
        self.is_cuda = device.type == "cuda"
        if self.is_cuda:
            mb = int(_ext().blob_stats_max_blocks())
            self.stats = torch.zeros(self.nslots, 4, dtype=torch.float32,
                                     device=device)
            self.scratch = torch.zeros(self.nslots, mb, 4,
                                       dtype=torch.float32, device=device)
            self.nblk = torch.zeros(self.nslots, dtype=torch.int32,
                                    device=device)
        else:
            self.stats = torch.zeros(self.nslots, 4, dtype=torch.float64)
            self.scratch = self.nblk = None

    def records(self):
        """[(asum, maxabs, nonfinite)] per slot, as Python numbers."""
        if self.is_cuda:
            host = self.stats.cpu()
            nf = host.view(torch.int32)[:, 2].tolist()
        else:
            host = self.stats
            nf = [int(v) for v in host[:, 2].tolist()]
        return list(zip(host[:, 0].tolist(), host[:, 1].tolist(), nf))


def _stats_dense(t: torch.Tensor) -> bool:
    """Non-overlapping and dense: some order of the dimensions walks the
    storage without gaps."""
    dims = sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1)
    expect = 1
    for st, sz in dims:
        if st != expect:
            return False
        expect *= sz
    return True


def _stats_check(t: torch.Tensor) -> None:
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("blob_stats: expected float32 or bfloat16")
    if not _stats_dense(t):
        raise ValueError("blob_stats: tensor must be non-overlapping and "
                         "dense (it is read in place, never copied)")


def _stats_cpu(t: torch.Tensor, out: BlobStatsBuffer, slot: int) -> None:
    a = t.detach().abs()
    fin = torch.isfinite(a)
    nf = int(a.numel() - int(fin.sum()))
    finite = a[fin]
    out.stats[slot, 0] = a.double().sum()
    out.stats[slot, 1] = float(finite.max()) if finite.numel() else 0.0
    out.stats[slot, 2] = nf
    out.stats[slot, 3] = 0.0


def blob_stats_plan(count: int, itemsize: int) -> Tuple[int, int]:
    """(blocks, longest serial add chain per accumulator) of the GPU pass
    over count elements of itemsize bytes."""
    blocks, chain = _ext().blob_stats_plan(int(count), int(itemsize))
    return int(blocks), int(chain)


def blob_stats_reduce_depth(blocks: int, itemsize: int) -> int:
    """Float adds between one accumulator and the record (vector, unroll,
    lane, wave and partial sums) for a launch of that many blocks."""
    return int(_ext().blob_stats_reduce_depth(int(blocks), int(itemsize)))


def blob_stats(t: torch.Tensor, out: BlobStatsBuffer, slot: int) -> None:
    """Statistics of one tensor into slot (GPU: its partials; the record is
    there after blob_stats_finalize). Everything goes as kernel arguments,
    so the launch is safe under graph capture for any tensor."""
    _stats_check(t)
    if not 0 <= slot < out.nslots:
        raise IndexError("blob_stats: slot out of range")
    if t.numel() == 0:
        return
    if t.is_cuda:
        _ext().blob_stats(t, out.scratch, out.nblk, int(slot))
    else:
        _stats_cpu(t, out, slot)


def blob_stats_mt_prepare(tensors, slots):
    """One table for a set of identity-stable tensors (all param diffs, all
    histories): blob_stats_mt_run covers them in a single launch. Rebuild it
    when a tensor's identity changes."""
    tensors, slots = list(tensors), [int(s) for s in slots]
    for t in tensors:
        _stats_check(t)
    if tensors and tensors[0].is_cuda:
        d, c, n, ms = _ext().blob_stats_mt_prepare(tensors, slots)
        return d, c, int(n), int(ms), tensors
    return None, None, 0, max(slots, default=0), list(zip(tensors, slots))


def blob_stats_mt_run(mt, out: BlobStatsBuffer) -> None:
    d, c, n, ms, held = mt
    if ms >= out.nslots:
        raise IndexError("blob_stats_mt_run: slot out of range")
    if d is not None:
        _ext().blob_stats_mt_run(d, c, n, ms, out.scratch, out.nblk)
        return
    for t, slot in held:
        _stats_cpu(t, out, slot)


def blob_stats_finalize(out: BlobStatsBuffer, slot0: int = 0,
                        nslots: Optional[int] = None) -> None:
    """Sum the partials of slots [slot0, slot0 + nslots) into their records:
    once per phase, after the phase's launches. Nothing to do on the CPU."""
    nslots = out.nslots - slot0 if nslots is None else nslots
    if slot0 < 0 or nslots < 0 or slot0 + nslots > out.nslots:
        raise IndexError("blob_stats_finalize: slot range out of bounds")
    if out.is_cuda and nslots:
        _ext().blob_stats_finalize(out.stats, out.scratch, out.nblk,
                                   int(slot0), int(nslots))


def blob_stats_launches(reset: bool = False) -> int:
    """Launches so far of the statistics kernels (single, multi-tensor and
    finalize): a host-side counter, like float_atomic_launches."""
    if not ext_available():
        return 0
    return int(_ext().blob_stats_launches(bool(reset)))


def nesterov_update(w, grad, hist, local_rate: float, momentum: float,
                    decay: float) -> None:
    """update = (1+mu)*h_new - mu*h_old (solver.cpp:1013-1120)."""
    if w.is_cuda:
        _ext().nesterov_update(w, grad, hist, local_rate, momentum, decay)
        return
    gw = grad if decay == 0.0 else grad + decay * w
    h_old = hist.clone()
    hist.mul_(momentum).add_(gw, alpha=local_rate)
    w.sub_((1 + momentum) * hist - momentum * h_old)


def adagrad_update(w, grad, hist, local_rate: float, delta: float,
                   decay: float) -> None:
    """hist += g^2 ; w -= lr * g / (sqrt(hist)+delta) (solver.cpp:1240-1364)."""
    if w.is_cuda:
        _ext().adagrad_update(w, grad, hist, local_rate, delta, decay)
        return
    gw = grad if decay == 0.0 else grad + decay * w
    hist.add_(gw * gw)
    w.sub_(local_rate * gw / (hist.sqrt() + delta))


# ---------------------------------------------------------------------------
# NHWC channel concat / slice (CONCAT + SLICE layers)
# ---------------------------------------------------------------------------

def concat_channels(tensors):
    if tensors[0].is_cuda and tensors[0].dim() == 4:
        return _ext().concat_channels(list(tensors))
    return torch.cat(tensors, dim=1)


def slice_channels(x, c_off: int, c_len: int):
    if x.is_cuda and x.dim() == 4:
        return _ext().slice_channels(x, c_off, c_len)
    return x.narrow(1, c_off, c_len).contiguous()


def split_channels(x, sizes, outs_cache=None, relu_masks=None):
    """All channel ranges in one go: up to 4 ranges per kernel launch
    (concat backward / slice forward over inception joins). outs_cache:
    persistent output tensors (keeps downstream grad identities stable
    for net-level batching). relu_masks: per-output post-relu activation
    tensors -- outputs are zeroed where the activation is zero, fusing
    the consumer ReLU's backward into the scatter."""
    if x.is_cuda and x.dim() == 4:
        return _ext().split_channels(x, [int(s) for s in sizes], outs_cache,
                                     relu_masks)
    out, off = [], 0
    for s in sizes:
        out.append(x.narrow(1, off, int(s)).contiguous())
        off += int(s)
    return out


# ---------------------------------------------------------------------------
# Data-layer transform (mean, crop, mirror, scale, cast) of raw uint8 records
# ---------------------------------------------------------------------------

MEAN_NONE, MEAN_SCALAR, MEAN_CHANNEL, MEAN_IMAGE = 0, 1, 2, 3


def data_transform(raw: torch.Tensor, params: torch.Tensor,
                   mean: Optional[torch.Tensor], mean_mode: int, scale: float,
                   out: torch.Tensor) -> None:
    """out[n,c,h,w] = (float(raw[n,c,h+h_off,ws]) - mean[c,h+h_off,ws]) * scale
    with (h_off, w_off, flip) = params[n] and ws = w_off + w, or
    w_off + Wo-1-w when flip: DataTransformer's arithmetic (one fp32
    subtract, one fp32 multiply, one rounding to out's dtype), written INTO
    out [N,C,Ho,Wo]. raw is uint8 [N,C,H,W], params int32 [N,3], mean fp32
    with 1 / C / C*H*W elements per mean_mode (MEAN_*)."""
    if raw.is_cuda:
        _ext().data_transform(raw, params, mean, int(mean_mode), float(scale),
                              out)
        return
    N, C, H, W = raw.shape
    Ho, Wo = int(out.shape[2]), int(out.shape[3])
    assert tuple(out.shape) == (N, C, Ho, Wo) and Ho <= H and Wo <= W
    x = raw.to(torch.float32)
    if mean_mode == MEAN_IMAGE:
        x = x - mean.reshape(1, C, H, W)
    elif mean_mode == MEAN_CHANNEL:
        x = x - mean.reshape(1, C, 1, 1)
    elif mean_mode == MEAN_SCALAR:
        x = x - mean.reshape(())
    p = params.long()
    h_off = p[:, 0:1].clamp(0, H - Ho)
    w_off = p[:, 1:2].clamp(0, W - Wo)
    w = torch.arange(Wo)
    hi = h_off + torch.arange(Ho)                                  # [N,Ho]
    wi = w_off + torch.where(p[:, 2:3] != 0, Wo - 1 - w, w)        # [N,Wo]
    g = x[torch.arange(N).view(N, 1, 1, 1), torch.arange(C).view(1, C, 1, 1),
          hi.view(N, 1, Ho, 1), wi.view(N, 1, 1, Wo)]
    out.copy_(g * torch.tensor(float(scale), dtype=torch.float32))


# ---------------------------------------------------------------------------
# Metrics
# ---------------------------------------------------------------------------

def accuracy(pred: torch.Tensor, labels: torch.Tensor, top_k: int = 1) -> torch.Tensor:
    n = pred.shape[0]
    flat = pred.reshape(n, -1)
    if top_k == 1:
        correct = (flat.argmax(dim=1) == labels.long().view(-1))
    else:
        topk = flat.topk(top_k, dim=1).indices
        correct = (topk == labels.long().view(-1, 1)).any(dim=1)
    return correct.to(torch.float32).sum() / n
