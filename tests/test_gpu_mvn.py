"""The fused MVN kernels against a plain fp64 reference, and the MVN layer's
choice of path.

Tolerance, after tests/test_gpu_lrn_within.py: the project's fp32 one (2e-4
relative, denominator clamped at 1); bf16 adds 2^-8 relative, the most one
rounding to bf16 can cost, of the magnitude the value is rounded from -- |y|,
and for dx the sum of the magnitudes of its three terms times rstd. The
kernels compute in fp32 and round once. An fp32 evaluation on the CPU of the
same centred formulas on these very inputs stays below 0.05 of the fp32
bound, so the bound belongs to the method."""

import pytest
import torch

from poseidon_amd.ops import functional as ops

gpu = pytest.mark.gpu
DEV = "cuda"
BF16, FP32 = torch.bfloat16, torch.float32
OFFSET, PLAIN = (1.0, 0.05), (0.0, 1.0)  # x = offset + scale * randn
# (shape, forced blocks per slab or 0, (offset, scale))
CASES = [((2, 8, 16, 16), 0, OFFSET),  # one bf16 vector; the composite fails
         ((3, 24, 7, 9), 0, PLAIN),    # three vectors, odd pixels, H != W
         ((2, 3, 6, 6), 0, PLAIN),     # scalar form; bf16 rows misaligned
         ((3, 5, 3, 7), 0, PLAIN),     # odd row: every later row misaligned
         ((1, 16, 1, 1), 0, PLAIN),    # one pixel: variance exactly 0
         ((3, 101), 0, OFFSET),        # 2-D, misaligned rows
         ((4, 1000), 0, PLAIN),        # 2-D, aligned rows
         ((1, 8, 18, 18), 0, PLAIN),   # a whole block per slab, through LDS
         ((1, 8, 40, 40), 3, PLAIN),   # split: unequal chunks merged
         ((2, 64, 32, 32), 3, OFFSET)]


def rnd(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def reference(x, dy, across, norm_var):
    """fp64 (y, dx, the magnitude dx's bf16 ulp is taken on)."""
    shape = x.shape
    x, dy = (t.double().reshape(tuple(shape) + (1,) * (4 - t.dim()))
             for t in (x, dy))  # (N, K) reads as (N, K, 1, 1)
    dims = (1, 2, 3) if across else (2, 3)
    mean = x.mean(dims, keepdim=True)
    var = ((x - mean) ** 2).mean(dims, keepdim=True)
    rstd = 1 / (var + 1e-10).sqrt() if norm_var else torch.ones_like(var)
    y = (x - mean) * rstd
    mdy = dy.mean(dims, keepdim=True)
    spread = y * (dy * y).mean(dims, keepdim=True) if norm_var else 0 * y
    dx = (dy - mdy - spread) * rstd
    mag = (dy.abs() + mdy.abs() + spread.abs()) * rstd
    return y.reshape(shape), dx.reshape(shape), mag.reshape(shape)


def check(got, ref, mag, what):
    err = (got.detach().cpu().double() - ref).abs()
    tol = 2e-4 * ref.abs().clamp(min=1.0)
    if got.dtype == BF16:
        tol = tol + 2.0 ** -8 * mag
    worst = (err / tol).max().item()
    print(f"{what}: max err {err.max().item():.3e}, {worst:.3f} of the bound")
    assert got.shape == ref.shape and worst <= 1.0, what


@gpu
@pytest.mark.parametrize("shape,split,data", CASES,
                         ids=["x".join(map(str, c[0])) for c in CASES])
@pytest.mark.parametrize("norm_var", [True, False], ids=["nv", "mean"])
@pytest.mark.parametrize("across", [False, True], ids=["chan", "across"])
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
def test_op_against_fp64(dtype, across, norm_var, shape, split, data):
    x = (data[0] + data[1] * rnd(shape, 1)).to(dtype)
    dy = rnd(shape, 2).to(dtype)
    ref_y, ref_dx, mag = reference(x, dy, across, norm_var)
    ops._set_mvn_split(split)
    try:
        n0 = ops.mvn_launches()
        y, stats = ops.mvn_forward(x.to(DEV), across, norm_var)
        n1 = ops.mvn_launches()
        dx = ops.mvn_backward(x.to(DEV), dy.to(DEV), stats, across, norm_var)
        n2 = ops.mvn_launches()
    finally:
        ops._set_mvn_split(0)
    assert (n1 - n0, n2 - n1) == ((2, 2) if split else (1, 1))
    sets = shape[0] if across else shape[0] * shape[1]
    assert stats.dtype == FP32 and tuple(stats.shape) == (sets, 2)
    assert y.dtype == dtype and dx.dtype == dtype
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    check(y, ref_y, ref_y.abs(), "y")
    check(dx, ref_dx, mag, "dx")


@gpu
@pytest.mark.parametrize("dtype,fused,data", [(FP32, True, PLAIN),
                                              (FP32, False, PLAIN),
                                              (BF16, True, OFFSET)],
                         ids=["fp32-fused", "fp32-composite", "bf16-offset"])
def test_layer(dtype, fused, data):
    """An MVN layer built from prototxt text (default mvn_param) against the
    same layer in fp64 on the CPU. fp32: the switch picks the path, and the
    composite meets this bound on zero-mean data. bf16 on offset data is the
    case the composite turns into NaNs."""
    from poseidon_amd.core.blob import Blob
    from poseidon_amd.core.layer import create_layer
    from poseidon_amd.proto import parse_text
    shape = (2, 8, 16, 16)
    x = (data[0] + data[1] * rnd(shape, 3)).to(dtype)
    dy = rnd(shape, 4).to(dtype)
    runs = []
    ops.set_mvn_fused(fused)
    try:
        for xs, ds in ((x.double(), dy.double()), (x.to(DEV), dy.to(DEV))):
            layer = create_layer(
                parse_text("LayerParameter", 'name: "m" type: MVN'), 0)
            bottom, top = Blob(shape), Blob(name="top")
            bottom.data = xs
            layer.setup([bottom], [top])
            n0 = ops.mvn_launches()
            layer.forward([bottom], [top])
            n1 = ops.mvn_launches()
            top.diff = ds
            layer.backward([top], [True], [bottom])
            runs.append((top.data, bottom.diff, n1 - n0,
                         ops.mvn_launches() - n1))
    finally:
        ops.set_mvn_fused(True)
    (ref_y, ref_dx, _, _), (y, dx, fwd, bwd) = runs
    assert (fwd, bwd) == ((1, 1) if fused else (0, 0))
    assert (layer._std is None) == fused
    assert y.dtype == dtype and dx.dtype == dtype
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    check(y, ref_y, ref_y.abs(), "layer y")
    check(dx, ref_dx, reference(x, dy, False, True)[2], "layer dx")
