"""Halo-tile direct convolution (conv_halo.hip) through the public conv ops,
against an fp64 CPU convolution of the bf16-quantised inputs.

Bound, derived and not measured: |y - ref| <= 2^-8 |ref| + K 2^-22 S, with K
the reduction length and S the fp64 conv of |x| with |w| (plus |b|): one bf16
rounding of the output, and f32 accumulation of K products in any order with
4x slack for the MFMA's internal order. ReLU is applied to the reference."""

import functools

import pytest
import torch
import torch.nn.functional as F

import poseidon_amd as pa
from poseidon_amd.ops import functional as ops
from test_gpu_bf16 import close_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda"

# name: (N, Ci, H, W, Co, (kh, kw), (ph, pw), grid cap, dgrad eligible)
_CASES = {
    "tiny-5x5": (2, 64, 5, 5, 64, (3, 3), (1, 1), 0, True),
    # 3 x 2 ragged tiles an image, 2 blocks walking 6 tiles each across the
    # image boundary
    "ragged-p1": (2, 64, 19, 37, 64, (3, 3), (1, 1), 2, True),
    "ragged-p0": (2, 64, 19, 37, 64, (3, 3), (0, 0), 2, True),
    "ragged-p2": (2, 64, 19, 37, 64, (3, 3), (2, 2), 2, True),
    "cifar-5x5": (2, 32, 16, 16, 32, (5, 5), (2, 2), 0, True),
    # the largest bank that fits; its dgrad's (64 -> 32, K = 1600) does not
    "5x5-co64": (2, 32, 9, 33, 64, (5, 5), (2, 2), 0, False),
    # Co = 48: an unpaired last fragment; the dgrad's Ci = 48 is ineligible
    "3x1-co48": (2, 64, 9, 20, 48, (3, 1), (1, 0), 0, False),
}


def _q(t):
    return t.to(torch.bfloat16).to(torch.float64)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, fp64 references and bounds of one case, computed once."""
    N, Ci, H, W, Co, k, p, blocks, dgrad = _CASES[name]
    g = torch.Generator().manual_seed(5)
    x = _q(torch.randn(N, Ci, H, W, generator=g))
    w = _q(torch.randn(Co, Ci, *k, generator=g) * 0.1)
    b = torch.randn(Co, generator=g).to(torch.float64)
    y = F.relu(F.conv2d(x, w, b, padding=p))
    dy = _q(torch.randn(*y.shape, generator=g))
    eps = 2.0 ** -22
    return dict(
        x=x, w=w, b=b, dy=dy, pad=p, blocks=blocks, dgrad=dgrad, y=y,
        y_tol=2.0 ** -8 * y.abs() + k[0] * k[1] * Ci * eps *
        F.conv2d(x.abs(), w.abs(), b.abs(), padding=p),
        dx=torch.nn.grad.conv2d_input(x.shape, w, dy, padding=p),
        dx_tol=k[0] * k[1] * Co * eps *
        torch.nn.grad.conv2d_input(x.shape, w.abs(), dy.abs(), padding=p))


@pytest.fixture
def halo():
    # implicit GEMM, dgrad-as-forward and the halo path from 0 bytes
    was = (ops.halo_conv(), ops.halo_threshold())
    ops.set_halo_conv(True)
    ops.set_halo_threshold(0)
    ops.set_implicit_gemm(True)
    ops.set_dgrad_fwd_threshold(0)
    yield
    ops.set_halo_conv(was[0])
    ops.set_halo_threshold(was[1])
    ops._set_halo_blocks(0)
    ops.set_implicit_gemm(False)
    ops.set_dgrad_fwd_threshold(128 << 20)


def _within(got, ref, tol, what):
    err = (got.double().cpu() - ref).abs()
    print(f"{what}: max err {err.max():.3e}, err - tol {(err - tol).max():.3e}")
    assert (err <= tol).all(), what


@pytest.mark.parametrize("name", list(_CASES))
def test_forward_and_dgrad(halo, name):
    c = _case(name)
    ops._set_halo_blocks(c["blocks"])
    xg = c["x"].to(DEV, torch.bfloat16)
    wg = c["w"].to(DEV, torch.float32)
    dyg = c["dy"].to(DEV, torch.bfloat16)
    n0 = ops.halo_conv_launches()
    y, (slot, _) = ops.conv2d_forward_ex(xg, wg, c["b"].to(DEV, torch.float32),
                                         (1, 1), c["pad"], 1, fuse_relu=True)
    assert ops.halo_conv_launches() == n0 + 1
    assert slot.dim() == 1 and slot.numel() == 0  # the implicit sentinel
    _within(y, c["y"], c["y_tol"], "y")
    rise = 1 if c["dgrad"] else 0
    dx = ops.conv2d_backward_input(wg, dyg, xg.shape, (1, 1), c["pad"], 1)
    assert ops.halo_conv_launches() == n0 + 1 + rise
    tol = 2.0 ** -8 * c["dx"].abs() + c["dx_tol"]
    _within(dx, c["dx"], tol, "dx")
    out = torch.full_like(dx, float("nan"))
    got = ops.conv2d_backward_input(wg, dyg, xg.shape, (1, 1), c["pad"], 1,
                                    dx_out=out)
    assert got.data_ptr() == out.data_ptr()
    assert ops.halo_conv_launches() == n0 + 1 + 2 * rise
    _within(out, c["dx"], tol, "dx_out")


def test_stride_2_keeps_the_gather_gemm(halo):
    x = torch.randn(2, 64, 9, 9, device=DEV).to(torch.bfloat16)
    w = torch.randn(64, 64, 3, 3, device=DEV) * 0.1
    n0 = ops.halo_conv_launches()
    ops.conv2d_forward_ex(x, w, None, (2, 2), (1, 1), 1)
    assert ops.halo_conv_launches() == n0


def test_plan_of_vgg_conv1_2_at_defaults():
    shape = ((32, 64, 224, 224), (64, 64, 3, 3), (1, 1), (1, 1), 1)
    assert ops.halo_threshold() == ops.HALO_THRESHOLD_DEFAULT
    was = ops.halo_conv()
    try:
        for on in (True, False):
            ops.set_halo_conv(on)
            plan = ops.conv_plan(*shape, True)
            assert plan["implicit"] and plan["dgrad_as_fwd"]
            assert plan["halo_fwd"] is on and plan["halo_dgrad"] is on
            fp32 = ops.conv_plan(*shape, False)
            assert not fp32["halo_fwd"] and not fp32["halo_dgrad"]
    finally:
        ops.set_halo_conv(was)


_FILL = 'weight_filler { type: "gaussian" std: 0.05 }'
_NET = """
    layers { name: "data" type: DUMMY_DATA top: "data" top: "label"
      dummy_data_param { num: 2 channels: 64 height: 11 width: 35 num: 2
        channels: 1 height: 1 width: 1 data_filler { type: "gaussian" }
        data_filler { type: "constant" } } }
    layers { name: "c1" type: CONVOLUTION bottom: "data" top: "c1"
      convolution_param { num_output: 64 kernel_size: 3 pad: 1 %s
        bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "r1" type: RELU bottom: "c1" top: "c1" }
    layers { name: "c2" type: CONVOLUTION bottom: "c1" top: "c2"
      convolution_param { num_output: 32 kernel_size: 3 pad: 1 %s } }
    layers { name: "ip" type: INNER_PRODUCT bottom: "c2" top: "ip"
      inner_product_param { num_output: 5 %s } }
    layers { name: "loss" type: SOFTMAX_LOSS bottom: "ip" bottom: "label"
      top: "loss" }
""" % (_FILL, _FILL, _FILL)


def test_net_trains_through_the_halo_path(halo):
    """conv(64 -> 64) -> relu -> conv(64 -> 32) -> ip -> loss, two solver
    steps with the path on and off: per step the halo kernel runs both
    forwards and c2's dgrad, and loss and parameters agree with the gathered
    path within close_bf16. Six graphed steps (warm-up, capture, replays)
    leave the parameters of six eager ones."""
    from poseidon_amd.proto import Message, parse_text
    from poseidon_amd.solver.solver import SGDSolver

    g = torch.Generator().manual_seed(41)
    data = torch.randn(2, 64, 11, 35, generator=g)
    labels = torch.tensor([1.0, 3.0]).view(2, 1, 1, 1)

    def train(on, graphed, steps):
        ops.set_halo_conv(on)
        pa.init(device="cuda", seed=7, compute_dtype=torch.bfloat16)
        sp = Message("SolverParameter", base_lr=0.01, lr_policy="fixed",
                     momentum=0.9, max_iter=100, display=0, snapshot=0)
        sp.net_param = parse_text("NetParameter", _NET)
        s = SGDSolver(sp, verbose=False)
        s.net.blobs["data"].data = data.to(DEV, torch.bfloat16)
        s.net.blobs["label"].data = labels.to(DEV)
        s.net.layers[0]._filled = True
        s.net.layers[0].refill = [False, False]
        if graphed:
            assert s.enable_graph() is True
        n0 = ops.halo_conv_launches()
        s.step(1)
        if not graphed:  # a graphed first step also warms up and captures
            assert ops.halo_conv_launches() == n0 + (3 if on else 0)
        s.step(steps - 1)
        torch.cuda.synchronize()
        assert not graphed or (s._use_graph and s._graph is not None)
        params = [p.blob.data.detach().cpu().clone()
                  for p in s.net.learnable_params]
        return float(s.net.forward()), params

    try:
        loss_off, p_off = train(False, False, 2)
        loss_on, p_on = train(True, False, 2)
        _, p_eager = train(True, False, 6)
        _, p_graph = train(True, True, 6)
    finally:
        pa.init(device="cpu", compute_dtype=torch.float32)
    print(f"loss on {loss_on:.6f} off {loss_off:.6f}")
    assert abs(loss_on - loss_off) <= 1e-2 * max(1.0, abs(loss_off))
    for a, b in zip(p_on, p_off):
        close_bf16(a, b, rtol=1e-2, atol=1e-2, what="param on/off")
    for a, b in zip(p_graph, p_eager):
        close_bf16(a, b, rtol=1e-2, atol=1e-2, what="param graph/eager")
