"""The 4-D SOFTMAX and the per-position ACCURACY on the GPU (softmax_heads.hip)
against float64 on the CPU, lane-group and wave-per-row, and both with the
two-top SOFTMAX_LOSS inside a small net against the same net on the CPU."""

import pytest
import torch

import poseidon_amd as pa
from poseidon_amd.ops import functional as ops
from test_gpu_softmax_dense import (BF16, DEV, FP32, RAGGED, SMALL, TILES, TOL,
                                    _run, close, inputs)
from test_softmax_heads_cpu import build

pytestmark = pytest.mark.gpu
# C == 2 G (the flipped order); a ragged third element at G = 1, 8, 64; None:
# the first C past the lane-group range
CS = [2, 8, 64, 3, 21, 150, None]
by_shape = pytest.mark.parametrize("nhw", [SMALL, RAGGED, TILES])
by_c = pytest.mark.parametrize("C", CS)
by_dtype = pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])


def on_device(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


@by_dtype
@by_shape
@by_c
def test_softmax_matches_float64(C, nhw, dtype):
    C = C or ops.softmax_dense_max_c() + 1
    x, _ = inputs(C, nhw, dtype)
    dy = torch.randn(x.shape, generator=torch.Generator().manual_seed(C)) \
        .to(dtype)
    y_ref = torch.softmax(x.double(), dim=1)
    xg, dyg = on_device(x), on_device(dy)
    was = ops.softmax_dense()
    try:
        for on in (True, False):
            ops.set_softmax_dense(on)
            n0 = ops.softmax_dense_launches()
            y = ops.softmax_forward(xg)
            dx = ops.softmax_backward(y, dyg)
            assert ops.softmax_dense_launches() - n0 == \
                (2 if on and C <= ops.softmax_dense_max_c() else 0)
            for t in (y, dx):
                assert t.shape == x.shape and t.dtype == dtype
                assert t.is_contiguous(memory_format=torch.channels_last)
            # the backward reads the rounded y the forward wrote
            yd, dyd = y.cpu().double(), dy.double()
            dx_ref = (dyd - (dyd * yd).sum(dim=1, keepdim=True)) * yd
            tag = f"C={C} {nhw} {dtype} on={on}"
            close(y, y_ref, TOL[dtype], f"y {tag}")
            close(dx, dx_ref, TOL[dtype], f"dx {tag}")
    finally:
        ops.set_softmax_dense(was)


def rank_count(x, labels, top_k):
    """float64: positions whose label has fewer than top_k channels ahead of
    it, greater or equal with a higher index."""
    c = x.shape[1]
    rows = x.permute(0, 2, 3, 1).reshape(-1, c).double()
    lbl = labels.long()
    ok = (lbl >= 0) & (lbl < c)
    lbl = lbl.clamp(0, c - 1).view(-1, 1)
    v = rows.gather(1, lbl)
    ahead = (rows > v) | ((rows == v) & (torch.arange(c).view(1, -1) > lbl))
    return int((ok & (ahead.sum(dim=1) < top_k)).sum())


@by_dtype
@by_shape
@by_c
def test_accuracy_counts_ranks_exactly(C, nhw, dtype):
    C = C or ops.softmax_dense_max_c() + 1
    x, labels = inputs(C, nhw, dtype)
    rows = labels.numel()
    g = torch.Generator().manual_seed(C + rows)
    ties = torch.randint(0, 5, x.shape, generator=g).to(dtype)
    no_class = labels.clone()
    no_class[3], no_class[5], no_class[rows - 1] = -1, C, C
    n0 = ops.softmax_dense_launches()
    launches = 0
    for xs, ls in ((x, labels), (ties, labels), (ties, no_class)):
        xg, lg = on_device(xs), ls.to(DEV)
        for top_k in sorted({1, min(3, C), C}):
            acc = ops.accuracy(xg, lg, top_k)
            again = ops.accuracy(xg, lg, top_k)
            launches += 2
            assert acc.shape == () and acc.dtype == FP32
            assert acc.view(torch.int32).item() == \
                again.view(torch.int32).item()
            want = rank_count(xs, ls, top_k)
            print(f"C={C} {nhw} top_k={top_k}: {acc.item() * rows:.3f} "
                  f"of {rows}, reference {want}")
            assert round(acc.item() * rows) == want
    assert ops.softmax_dense_launches() - n0 == \
        (launches if C <= ops.softmax_dense_max_c() else 0)


def test_heads_in_a_net_on_the_gpu_match_the_cpu_net():
    try:
        cpu = build("cpu")
        loss_c = _run(cpu)
        gpu = build("cuda")
        n0 = ops.softmax_dense_launches()
        loss_g = _run(gpu, like=cpu)
        # the loss and the softmax each way, and the accuracy
        assert ops.softmax_dense_launches() == n0 + 5
        print(f"loss gpu {loss_g:.6f} cpu {loss_c:.6f}")
        assert abs(loss_g - loss_c) <= TOL[FP32] * max(1.0, abs(loss_c))
        for name in ("loss", "fit", "prob", "sm"):
            close(gpu.blobs[name].data, cpu.blobs[name].data, TOL[FP32], name)
        assert round(gpu.blobs["acc"].data.item() * 84) == \
            round(cpu.blobs["acc"].data.item() * 84)
        close(gpu.learnable_params[0].blob.diff,
              cpu.learnable_params[0].blob.diff, TOL[FP32], "score dW")
        layer = gpu.layers[gpu.layer_names.index("loss")]
        assert gpu.blobs["prob"].data.data_ptr() == layer._prob.data_ptr()
    finally:
        pa.init(device="cpu", compute_dtype=FP32)
