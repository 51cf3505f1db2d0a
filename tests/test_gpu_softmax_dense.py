"""Dense (per-position) SOFTMAX_LOSS on the GPU: the lane-group kernels
(softmax_dense.hip) and their wave-per-row A/B partner against the float64
definition evaluated on the CPU, the ordered deterministic reduction, and
the layer inside a small net against the same net on the CPU."""

import pytest
import torch

import poseidon_amd as pa
from poseidon_amd.ops import functional as ops
from test_softmax_dense_cpu import _NET, reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, FP32 = torch.bfloat16, torch.float32
TOL = {FP32: 2e-4, BF16: 3e-2}
SMALL, RAGGED, TILES = (2, 3, 5), (1, 7, 9), (3, 8, 11)  # 30, 63, 264 rows


def close(a, b, tol, what):
    """tests/test_gpu_ops.py's rule; prints what it saw."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    err = (a - b).abs()
    rel = (err / b.abs().clamp(min=1.0)).max().item()
    print(f"{what}: max abs {err.max().item():.3e} rel {rel:.3e}")
    assert rel <= tol or err.max().item() <= tol, what


def inputs(C, nhw, dtype):
    n, h, w = nhw
    g = torch.Generator().manual_seed(1000 * C + n * h * w)
    x = torch.randn(n, C, h, w, generator=g) * 4
    x[0, :, 0, 0] += 80
    x[-1, :, -1, -1] -= 80
    labels = torch.randint(0, C, (n * h * w,), generator=g).float()
    labels[1], labels[2] = 0, C - 1
    return x.to(dtype), labels


# (C, (N, H, W), cap of the forward's grid). C = None: the first C past the
# plan's lane-group range, which runs wave-per-row either way. At these sizes
# the plan gives every tile a block; the cap of 2 makes two blocks walk all
# tiles, as every block does once there are more tiles than the grid holds.
CASES = [(2, SMALL, 0), (2, TILES, 0), (3, RAGGED, 0), (5, SMALL, 0),
         (8, TILES, 0), (21, RAGGED, 0), (21, TILES, 0), (21, TILES, 2),
         (33, SMALL, 0), (64, RAGGED, 0), (64, TILES, 2), (150, RAGGED, 0),
         (150, TILES, 0), (None, SMALL, 0)]


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C,nhw,max_blocks", CASES)
def test_dense_loss_matches_float64(C, nhw, dtype, max_blocks):
    if C is None:
        C = ops.softmax_dense_max_c() + 1
    x, labels = inputs(C, nhw, dtype)
    lane_groups = C <= ops.softmax_dense_max_c()
    weight = 0.7
    # bf16: the loss is an fp32 sum over the rounded logits the kernel reads
    ref_loss, ref_prob, ref_dx = reference(x, labels, weight)
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last)
    lg = labels.to(DEV)
    was = ops.softmax_dense()
    try:
        for on in (True, False):
            ops.set_softmax_dense(on)
            n0 = ops.softmax_dense_launches()
            loss, prob = ops.softmax_loss_forward(xg, lg, max_blocks)
            dx = ops.softmax_loss_backward(prob, lg, weight)
            assert ops.softmax_dense_launches() - n0 == \
                (2 if on and lane_groups else 0)
            tag = f"C={C} {nhw} {dtype} on={on}"
            for t in (prob, dx):
                assert t.shape == x.shape and t.dtype == dtype
                assert t.is_contiguous(memory_format=torch.channels_last)
            close(loss, ref_loss, TOL[FP32], f"loss {tag}")
            close(prob, ref_prob, TOL[dtype], f"prob {tag}")
            close(dx, ref_dx, TOL[dtype], f"dx {tag}")
    finally:
        ops.set_softmax_dense(was)


@pytest.mark.parametrize("max_blocks", [0, 2])
def test_deterministic_loss_is_ordered_and_atomic_free(max_blocks):
    x, labels = inputs(21, TILES, FP32)
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last)
    lg = labels.to(DEV)
    ops.set_deterministic(True)
    try:
        a0, n0 = ops.float_atomic_launches(), ops.softmax_dense_launches()
        first, _ = ops.softmax_loss_forward(xg, lg, max_blocks)
        second, _ = ops.softmax_loss_forward(xg, lg, max_blocks)
        assert ops.softmax_dense_launches() == n0 + 2
        assert ops.float_atomic_launches() == a0
        assert first.view(torch.int32).item() == second.view(torch.int32).item()
        close(first, reference(x, labels)[0], TOL[FP32], "deterministic loss")
    finally:
        ops.set_deterministic(False)


def _net(device, lh, lw):
    from poseidon_amd.core.net import Net, TRAIN
    from poseidon_amd.proto import parse_text
    pa.init(device=device, seed=3, compute_dtype=FP32)
    return Net(parse_text("NetParameter", _NET % (lh, lw)), phase=TRAIN,
               verbose=False)


def _run(net, like=None):
    """forward + backward; like: the net whose data, labels and weights to
    take (the fillers draw from each device's own generator)."""
    if like is not None:
        for name in ("data", "label"):
            net.blobs[name].data = like.blobs[name].data.to(DEV)
        # DUMMY_DATA fills a top on its first forward (_filled) and again on
        # every forward whose filler is not constant (refill): keep ours
        net.layers[0]._filled = True
        net.layers[0].refill = [False, False]
        for p, q in zip(net.learnable_params, like.learnable_params):
            p.blob.data.copy_(q.blob.data)
    loss = net.forward()
    net.zero_param_diffs()
    net.backward()
    return loss


def test_layer_on_the_gpu_matches_the_cpu_net():
    try:
        cpu = _net("cpu", 6, 7)
        loss_c = _run(cpu)
        gpu = _net("cuda", 6, 7)
        n0 = ops.softmax_dense_launches()
        loss_g = _run(gpu, like=cpu)
        assert ops.softmax_dense_launches() == n0 + 2
        print(f"loss gpu {loss_g:.6f} cpu {loss_c:.6f}")
        assert abs(loss_g - loss_c) <= TOL[FP32] * max(1.0, abs(loss_c))
        close(gpu.learnable_params[0].blob.diff,
              cpu.learnable_params[0].blob.diff, TOL[FP32], "score dW")
        with pytest.raises(ValueError, match="label"):
            _net("cuda", 3, 7)
        # one label per image: the classifier path, bit for bit the 2-D op
        flat = _net("cuda", 1, 1)
        n0 = ops.softmax_dense_launches()
        loss_f = _run(flat)
        assert ops.softmax_dense_launches() == n0
        ref, _ = ops.softmax_loss_forward(
            flat.blobs["score"].data.reshape(2, -1),
            flat.blobs["label"].data.reshape(-1))
        assert loss_f == ref.item()
    finally:
        pa.init(device="cpu", compute_dtype=FP32)
