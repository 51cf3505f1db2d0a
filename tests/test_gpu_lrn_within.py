"""The fused WITHIN_CHANNEL LRN kernels against a plain fp64 reference, the
LRN layer's choice of path, and the cifar10_full model that needs them.

Tolerance: the project's fp32 one (close() of tests/test_gpu_ops.py: 2e-4
relative, denominator clamped at 1). bf16 adds one bf16 ulp (2^-8 relative)
of the reference value: the kernels compute in fp32 and round once, which
costs half of that. dx is a difference, so its ulp is taken on the sum of the
magnitudes of its two terms."""

import pytest
import torch
import torch.nn.functional as F

import poseidon_amd as pa
from poseidon_amd.ops import functional as ops

gpu = pytest.mark.gpu
DEV = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                                 ids=["bf16", "fp32"])
SEAMS = (1, 8, 8, 4)  # run with 3-row strips: strip seams, ring warm-up
SHAPES = [(3, 32, 8, 8),   # norm2: several images in one block
          (2, 24, 7, 9),   # three lanes per pixel, odd sides, H != W
          (1, 8, 3, 300),  # one image row spans several blocks
          (2, 3, 6, 6),    # one channel per lane
          (1, 16, 2, 2),   # window larger than the image
          SEAMS]


def rnd(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def reference(x, dy, size, alpha, beta):
    """fp64 (y, dx, the magnitude dx's bf16 ulp is taken on)."""
    x, dy = x.double(), dy.double()

    def box(t):  # window sum / size^2, zero padding counted
        return F.avg_pool2d(t, size, 1, (size - 1) // 2,
                            count_include_pad=True)
    s = 1 + alpha * box(x * x)
    direct = dy * s ** -beta
    spread = 2 * alpha * beta * x * box(dy * x * s ** (-beta - 1))
    return x * s ** -beta, direct - spread, direct.abs() + spread.abs()


def check(got, ref, mag, what):
    err = (got.detach().cpu().double() - ref).abs()
    tol = 2e-4 * ref.abs().clamp(min=1.0)
    if got.dtype == torch.bfloat16:
        tol = tol + 2.0 ** -8 * mag
    worst = (err / tol).max().item()
    print(f"{what}: max err {err.max().item():.3e}, {worst:.3f} of the bound")
    assert got.shape == ref.shape and worst <= 1.0, what


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.75), (0.3, 1.25)])
@pytest.mark.parametrize("size", [3, 5, 7])
@DTYPES
def test_op_against_fp64(dtype, size, alpha, beta, shape):
    """alpha = 1 turns a wrong halo into an O(1) error; beta = 1.25 takes the
    general pow path."""
    x, dy = rnd(shape, 1, dtype), rnd(shape, 2, dtype)
    ref_y, ref_dx, mag = reference(x, dy, size, alpha, beta)
    ops._set_lrn_within_strip(3 if shape == SEAMS else 0)
    try:
        before = ops.lrn_within_launches()
        y, scale = ops.lrn_within_forward(x.to(DEV), size, alpha, beta)
        dx = ops.lrn_within_backward(x.to(DEV), dy.to(DEV), size, alpha, beta)
    finally:
        ops._set_lrn_within_strip(0)
    assert scale is None and ops.lrn_within_launches() - before == 2
    assert y.dtype == dtype and dx.dtype == dtype
    check(y, ref_y, ref_y.abs(), "y")
    check(dx, ref_dx, mag, "dx")


def _run_layer(x, dy):
    """One forward and backward of a WITHIN_CHANNEL LRN layer built from
    prototxt text -> (y, dx, fused launches of the forward, of the
    backward, the layer)."""
    from poseidon_amd.core.blob import Blob
    from poseidon_amd.core.layer import create_layer
    from poseidon_amd.proto import parse_text
    layer = create_layer(parse_text("LayerParameter", """name: "n" type: LRN
        lrn_param { local_size: 3 alpha: 1.0 beta: 0.75
                    norm_region: WITHIN_CHANNEL }"""), 0)
    bottom, top = Blob(x.shape), Blob(name="top")
    bottom.data = x
    layer.setup([bottom], [top])
    n0 = ops.lrn_within_launches()
    layer.forward([bottom], [top])
    n1 = ops.lrn_within_launches()
    top.diff = dy
    layer.backward([top], [True], [bottom])
    return top.data, bottom.diff, n1 - n0, ops.lrn_within_launches() - n1, layer


@gpu
def test_layer_takes_the_fused_path():
    """fp32: with the switch off the layer runs the composite, which rounds
    every intermediate to the compute type and meets this bound in fp32
    only. The bf16 kernels are held to it by test_op_against_fp64."""
    x = rnd((2, 16, 5, 6), 3, torch.float32)
    dy = rnd((2, 16, 5, 6), 4, torch.float32)
    ref_y, ref_dx, _, _, _ = _run_layer(x.double(), dy.double())
    mag = reference(x, dy, 3, 1.0, 0.75)[2]
    try:
        for on in (True, False):
            ops.set_lrn_within(on)
            y, dx, fwd, bwd, layer = _run_layer(x.to(DEV), dy.to(DEV))
            assert (fwd, bwd) == ((1, 1) if on else (0, 0))
            assert (layer._scale is None and layer._y is None) == on
            check(y, ref_y, ref_y.abs(), f"layer y, fused {on}")
            check(dx, ref_dx, mag, f"layer dx, fused {on}")
    finally:
        ops.set_lrn_within(True)


def test_cifar10_full_builds_cpu():
    from poseidon_amd.core.net import Net, TRAIN
    from poseidon_amd.models import zoo
    pa.init(device="cpu", seed=3)
    net = Net(zoo.cifar10_full(batch=16, num_classes=4), phase=TRAIN,
              verbose=False)
    norms = [l for l in net.layers if hasattr(l, "region")]
    assert [(l.region, l.size) for l in norms] == [("WITHIN_CHANNEL", 3)] * 2
    assert net.blobs["norm2"].shape == (16, 32, 8, 8)
    assert net.blobs["ip1"].shape[:2] == (16, 4)
    assert torch.isfinite(torch.tensor(net.forward()))


@gpu
def test_cifar10_full_step_and_capture_gpu():
    """One bf16 forward and backward (after test_cifar_quick_step_gpu), both
    norms on the fused kernels, then a short graphed SGD run."""
    from poseidon_amd.core.net import Net, TRAIN
    from poseidon_amd.models import zoo
    from poseidon_amd.proto import Message
    from poseidon_amd.solver.solver import SGDSolver
    pa.init(device="cuda", seed=3, compute_dtype=torch.bfloat16)
    try:
        net = Net(zoo.cifar10_full(batch=16, num_classes=4), phase=TRAIN,
                  verbose=False)
        before = ops.lrn_within_launches()
        assert torch.isfinite(torch.tensor(net.forward()))
        net.zero_param_diffs()
        net.backward()
        assert ops.lrn_within_launches() - before == 4
        for ps_ in net.learnable_params:
            assert torch.isfinite(ps_.blob.diff).all(), ps_.blob.name
            assert float(ps_.blob.diff.abs().sum()) > 0, ps_.blob.name
        sp = Message("SolverParameter", base_lr=0.001, lr_policy="fixed",
                     momentum=0.9, weight_decay=0.004, max_iter=100,
                     display=0, snapshot=0)
        sp.net_param = zoo.cifar10_full(batch=16, num_classes=4)
        s = SGDSolver(sp, verbose=False)
        assert s.enable_graph() is True
        loss = s.step(4)
        torch.cuda.synchronize()
        assert s._use_graph and s._graph is not None and s.iter == 4
        assert torch.isfinite(torch.tensor(loss))
    finally:
        pa.init(device="cpu", compute_dtype=torch.float32)
