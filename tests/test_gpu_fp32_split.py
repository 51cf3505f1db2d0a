"""Split-precision fp32 GEMMs (gemm_split.hip, ops.set_fp32_split): every
numerical case against an fp64 reference of the same fp32 inputs, held
element-wise to

    |got - ref| <= (2^-16 + K * 2^-22) * S   (+ 2^-24 |bias| with a bias)

with S = sum_k |a_k| |b_k| in fp64: |x - hi - lo| <= 2^-18 |x| per operand
and the dropped lo*lo term <= 2^-18 |a b| stay under 2^-16 per product, and
3K fp32 addends in any order give 3K * 2^-24 <= K * 2^-22. A kernel that
loses a cross term misses this 8x or more at K <= 264, so the cases that
judge the arithmetic stay there; the split-K cases have the K their plans
need (a wrong slice is off by orders of magnitude). The deterministic case
reads its K from the plan made in deterministic mode: the smallest K that
splits atomically does not split there."""

import pytest
import torch
import torch.nn.functional as F

import poseidon_amd as pa
from poseidon_amd.core.net import Net, TRAIN
from poseidon_amd.models import zoo
from poseidon_amd.ops import functional as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAYOUTS = {"nt": (True, True), "nn": (True, False), "tn": (False, False)}


@pytest.fixture(autouse=True)
def switches():
    ops.set_fp32_split(True)
    ops.fp32_split_launches(reset=True)
    yield
    ops.set_fp32_split(False)
    ops.set_implicit_gemm(False)
    ops.set_deterministic(False)


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def within(got, ref, S, K, extra=0.0, what=""):
    err = (got.detach().double().cpu() - ref).abs()
    bound = (2.0 ** -16 + K * 2.0 ** -22) * S + extra
    print(f"{what}: {(err / bound).max().item():.3f} of the bound")
    assert (err <= bound).all(), what


def gemm_case(M, N, K, layout):
    """ext.gemm on the split path against fp64, in one of the LAYOUTS"""
    ak, bk = LAYOUTS[layout]
    a, b = rnd(M, K, seed=1), rnd(K, N, seed=2)
    A = (a if ak else a.t()).contiguous().to(DEV)
    B = (b.t() if bk else b).contiguous().to(DEV)
    plan = ops.gemm_plan(M, N, K, ak, bk, False)
    assert plan["split3"] and not plan["tr16"]
    n0 = ops.fp32_split_launches()
    got = ops._ext().gemm(A, B, M, N, K, ak, bk)
    torch.cuda.synchronize()
    assert ops.fp32_split_launches() == n0 + 1
    within(got, a.double() @ b.double(), a.double().abs() @ b.double().abs(),
           K, what=f"{layout} {M}x{N}x{K}")
    return A, B, plan


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape", [(40, 72, 40), (130, 136, 264),
                                   (16, 200, 33)])
def test_plain_gemm(shape, layout):
    gemm_case(*shape, layout)


@pytest.fixture(scope="module")
def fc():
    """130x136x264 linear layer: inputs and fp64 references, made once"""
    x, w, b, dy = (rnd(130, 264, seed=3), rnd(136, 264, seed=4),
                   rnd(136, seed=5), rnd(130, 136, seed=6))
    xd, wd, dyd = x.double(), w.double(), dy.double()
    return dict(x=x, w=w, b=b, dy=dy, y=xd @ wd.t(),
                Sy=xd.abs() @ wd.abs().t(), dx=dyd @ wd,
                Sdx=dyd.abs() @ wd.abs(), dw=dyd.t() @ xd,
                Sdw=dyd.abs().t() @ xd.abs())


@pytest.mark.parametrize("epi", ["none", "bias", "bias_relu"])
def test_linear_forward(fc, epi):
    b = None if epi == "none" else fc["b"].to(DEV)
    y = ops.linear_forward(fc["x"].to(DEV), fc["w"].to(DEV), b,
                           fuse_relu=epi == "bias_relu")
    ref, extra = fc["y"], 0.0
    if b is not None:
        ref, extra = ref + fc["b"].double(), 2.0 ** -24 * fc["b"].double().abs()
    if epi == "bias_relu":
        # |relu(p) - relu(q)| <= |p - q|: the bound carries over
        ref = ref.clamp(min=0)
    assert ops.fp32_split_launches() == 1
    within(y, ref, fc["Sy"], 264, extra, f"linear forward {epi}")


def test_linear_backward(fc):
    dx, dw, _ = ops.linear_backward(fc["x"].to(DEV), fc["w"].to(DEV),
                                    fc["dy"].to(DEV), True, True, False)
    assert ops.fp32_split_launches() == 2
    within(dx, fc["dx"], fc["Sdx"], 136, what="linear dx")
    within(dw, fc["dw"], fc["Sdw"], 130, what="linear dW")


def first_split_k():
    """smallest K whose 64x64 plan, in the current mode, splits K"""
    for K in range(32, 16385, 32):
        if ops.gemm_plan(64, 64, K, False, False, False)["splitk"] > 1:
            return K
    raise AssertionError("no K up to 16384 splits a 64x64 output")


def test_splitk_atomic():
    n0 = ops.float_atomic_launches()
    _, _, plan = gemm_case(64, 64, first_split_k(), "tn")
    assert plan["splitk"] > 1 and plan["ws_elems"] == 0
    assert ops.float_atomic_launches() == n0 + 1


def test_splitk_deterministic():
    ops.set_deterministic(True)
    n0 = ops.float_atomic_launches()
    K = first_split_k()
    A, B, plan = gemm_case(64, 64, K, "tn")
    assert plan["splitk"] > 1 and plan["ws_elems"] > 0
    c1 = ops._ext().gemm(A, B, 64, 64, K, False, False)
    c2 = ops._ext().gemm(A, B, 64, 64, K, False, False)
    assert torch.equal(c1, c2)
    assert ops.float_atomic_launches() == n0


@pytest.mark.parametrize("groups,stride,K", [(1, 1, 72), (2, 2, 36)])
def test_implicit_conv(groups, stride, K):
    x, w, b = rnd(2, 8, 9, 9, seed=7), rnd(16, 8 // groups, 3, 3, seed=8), \
        rnd(16, seed=9)
    kw = dict(stride=stride, padding=1, groups=groups)
    xd, wd = x.double(), w.double()
    y_ref = F.conv2d(xd, wd, b.double(), **kw)
    dy = rnd(*y_ref.shape, seed=10)
    dyd = dy.double()
    st, pd = (stride, stride), (1, 1)
    ops.set_implicit_gemm(True)
    y, cache = ops.conv2d_forward_ex(x.to(DEV), w.to(DEV), b.to(DEV), st, pd,
                                     groups)
    assert ops.fp32_split_launches() >= 1
    within(y, y_ref, F.conv2d(xd.abs(), wd.abs(), None, **kw), K,
           (2.0 ** -24 * b.double().abs()).view(1, -1, 1, 1), "conv forward")
    dx = ops.conv2d_backward_input(w.to(DEV), dy.to(DEV), x.shape, st, pd,
                                   groups)
    within(dx, torch.nn.grad.conv2d_input(list(x.shape), wd, dyd, **kw),
           torch.nn.grad.conv2d_input(list(x.shape), wd.abs(), dyd.abs(), **kw),
           K, what="conv dgrad")
    dw = torch.zeros_like(w).to(DEV)
    ops.conv2d_backward_weight_acc(x.to(DEV), cache[0], dy.to(DEV), dw, None,
                                   st, pd, groups)
    within(dw, torch.nn.grad.conv2d_weight(xd, list(w.shape), dyd, **kw),
           torch.nn.grad.conv2d_weight(xd.abs(), list(w.shape), dyd.abs(),
                                       **kw), K, what="conv wgrad")


def lenet_step():
    net = Net(zoo.lenet(batch=8), phase=TRAIN, verbose=False)
    loss = net.forward()
    net.zero_param_diffs()
    net.backward()
    torch.cuda.synchronize()
    return float(loss)


def test_public_interface():
    ops.set_fp32_split(False)
    dtype0 = pa.ctx().compute_dtype
    try:
        pa.init(device="cuda", seed=1, compute_dtype=torch.float32,
                fp32_split=True)
        assert ops.fp32_split() and pa.ctx().fp32_split
        loss = lenet_step()
        assert ops.fp32_split_launches(reset=True) > 0
        assert loss == loss and abs(loss) != float("inf")
        pa.init(compute_dtype=torch.bfloat16)
        lenet_step()
        assert ops.fp32_split_launches() == 0
    finally:
        pa.init(compute_dtype=dtype0)
    epoch = ops.conv_policy_epoch()
    ops.set_fp32_split(False)
    assert ops.conv_policy_epoch() > epoch and not pa.ctx().fp32_split
    for ak, bk in LAYOUTS.values():
        assert not ops.gemm_plan(130, 136, 264, ak, bk, False)["split3"]
