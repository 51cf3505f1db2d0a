"""The gather GEMM's walked A staging (gemm.hip GatherWalk, ps_gather.h) at
the smallest conv shapes that reach each piece of it. Every shape has at
least one interior 128-row tile (the walk lives only there) and an edge
tile (which still decodes every address through gather_addr).

Forward: the gathered (implicit) result must be bit-equal to the
materialised result of the same build -- same tiles, same k order, the
column matrix only adds zero columns -- and within the bf16 tolerances of
tests/test_gpu_bf16.py of a CPU reference from bf16-quantised inputs.

dgrad-as-forward (forced with set_dgrad_fwd_threshold(0)): max abs error
against an fp64 reference from bf16-quantised inputs, held to 4x the error
the commit before the walk made on the same case (PARENT_DGRAD_ERR, measured
on an MI355X; the margin covers bf16 output rounding of values that sit near
a rounding boundary), the rule of tests/test_gpu_tr16_tiles.py.

The N-fitting tiles 128x96 and 128x48 (plain NT ext.gemm, ragged M): max abs
error against an fp64 reference from bf16-quantised inputs, held to 4x the
error of the parent's 128x128 / 64x64 tiles on the same shapes
(PARENT_TILE_ERR). tests/gather_walk_host.cpp checks that the planner gives
these shapes those tiles.

Remapped grids (plain NT ext.gemm, bf16 and one fp32): the planned 2D-XCD
rectangle and the linear XCD swizzle on more than 8 blocks, by the same
measure and rule; their PARENT_TILE_ERR entries are the commit before the
remaps moved into ps_gemm_plan.h (which gave bit-equal results).
tests/gemm_plan_host.cpp pins the plans of these shapes."""

import pytest
import torch
import torch.nn.functional as F

from poseidon_amd.ops import functional as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"

CASES = {
    # Cg = 48 wraps twice inside a 64-deep tile; Kg = 1200 leaves a 48-wide K
    # tail; M = 676; the dgrad has N = 48
    "conv2-like": dict(N=4, C=96, hw=13, Co=256, k=5, s=1, p=2, g=2),
    # Cg = 192 wraps every third tile; N = 192 forward and dgrad
    "conv4-like": dict(N=4, C=384, hw=13, Co=384, k=3, s=1, p=1, g=2),
    # Cg = 8 (re-decoded, not walked); Kg = 72 padded to 128; N = 96
    "small-Cg": dict(N=4, C=8, hw=16, Co=96, k=3, s=1, p=1, g=1),
    "strided": dict(N=8, C=64, hw=17, Co=128, k=3, s=2, p=1, g=1),
    "wide-kernel": dict(N=4, C=16, hw=12, Co=48, k=7, s=1, p=3, g=1),
    # Kg = 4608 takes the workspace split-K: slices start at k_begin != 0
    "split-K": dict(N=2, C=512, hw=8, Co=128, k=3, s=1, p=1, g=1),
    "small-Cg-f32": dict(N=4, C=8, hw=16, Co=96, k=3, s=1, p=1, g=1, f32=True),
}

# max abs error of the parent commit's dgrad-as-forward against the fp64
# reference, same inputs (three runs gave the same figure: no atomics on this
# path; the bf16 cases are half an ulp of dx values between 4 and 16). On
# the parent every forward case is bit-equal to the materialised result too.
PARENT_DGRAD_ERR = {
    "conv2-like": 6.212e-02,
    "conv4-like": 5.890e-02,
    "small-Cg": 2.997e-02,
    "wide-kernel": 5.748e-02,
    "split-K": 3.120e-02,
    "small-Cg-f32": 4.219e-06,
}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _dtype(c):
    return torch.float32 if c.get("f32") else torch.bfloat16


def _quant(t, c):
    return t.to(_dtype(c)).float()


def make_data():
    out = {}
    for name, c in CASES.items():
        x = rnd(c["N"], c["C"], c["hw"], c["hw"], seed=21)
        w = rnd(c["Co"], c["C"] // c["g"], c["k"], c["k"], seed=22, scale=0.1)
        b = rnd(c["Co"], seed=23)
        xq, wq = _quant(x, c), _quant(w, c)
        y_ref = F.conv2d(xq, wq, b, stride=c["s"], padding=c["p"],
                         groups=c["g"])
        d = dict(x=x, w=w, b=b, y_ref=y_ref)
        if c["s"] == 1:
            dy = rnd(*y_ref.shape, seed=24)
            d["dy"] = dy
            d["dx_ref"] = torch.nn.grad.conv2d_input(
                list(x.shape), wq.double(), _quant(dy, c).double(),
                stride=c["s"], padding=c["p"], groups=c["g"])
        out[name] = d
    return out


@pytest.fixture(scope="module")
def data():
    """Inputs and CPU references, made once and left unchanged."""
    return make_data()


def _forward(c, d, implicit):
    st, pd = (c["s"], c["s"]), (c["p"], c["p"])
    ops.set_implicit_gemm(implicit)
    try:
        y, _ = ops.conv2d_forward_ex(d["x"].to(DEV, _dtype(c)), d["w"].to(DEV),
                                     d["b"].to(DEV), st, pd, c["g"])
        torch.cuda.synchronize()
    finally:
        ops.set_implicit_gemm(False)
    return y


@pytest.mark.parametrize("name", list(CASES))
def test_gathered_forward_equals_materialised(data, name):
    c, d = CASES[name], data[name]
    y_mat = _forward(c, d, False)
    y_gat = _forward(c, d, True)
    assert y_gat.dtype == _dtype(c)
    diff = (y_gat.float() - y_mat.float()).abs().max().item()
    err = (y_gat.detach().cpu().float() - d["y_ref"]).abs()
    rel = (err / d["y_ref"].abs().clamp(min=1.0)).max().item()
    print(f"{name}: gathered vs materialised max abs {diff:.3e}; "
          f"vs CPU max abs {err.max().item():.3e} rel {rel:.3e}")
    assert torch.equal(y_gat, y_mat), \
        f"{name}: gathered != materialised, max abs {diff:.3e}"
    # tests/test_gpu_bf16.py: rtol = atol = 1e-2. The f32 case sums 72
    # products of O(0.1) terms in f32 either way: 1e-4 is ~100x its rounding
    tol = 1e-4 if c.get("f32") else 1e-2
    assert rel <= tol or err.max().item() <= tol, \
        f"{name}: max abs {err.max().item():.3e} rel {rel:.3e}"


def dgrad_error(name, c, d):
    """max abs error of the forced dgrad-as-forward against the fp64 ref"""
    st, pd = (c["s"], c["s"]), (c["p"], c["p"])
    ops.set_dgrad_fwd_threshold(0)
    try:
        dx = ops.conv2d_backward_input(d["w"].to(DEV),
                                       d["dy"].to(DEV, _dtype(c)),
                                       d["x"].shape, st, pd, c["g"])
        torch.cuda.synchronize()
    finally:
        ops.set_dgrad_fwd_threshold(ops.DGRAD_FWD_THRESHOLD_DEFAULT)
    assert dx.shape == d["x"].shape
    return (dx.detach().cpu().double() - d["dx_ref"]).abs().max().item()


@pytest.mark.parametrize("name", list(PARENT_DGRAD_ERR))
def test_dgrad_as_forward(data, name):
    c, d = CASES[name], data[name]
    err = dgrad_error(name, c, d)
    bound = 4.0 * PARENT_DGRAD_ERR[name]
    print(f"{name}: dgrad-as-forward max abs err {err:.3e} (bound "
          f"{bound:.3e}, parent {PARENT_DGRAD_ERR[name]:.3e})")
    assert err <= bound, \
        f"{name}: max abs {err:.3e} > 4 x parent {PARENT_DGRAD_ERR[name]:.3e}"


# (M, N, K) -> max abs error of the parent commit (f32 output: accumulation
# order only). K = 333 has rows that are not 16 B multiples (register
# staging), K = 320 is all direct-to-LDS tiles, K = 200 leaves an 8-wide tail.
N_FITTING = [(300, 96, 320), (300, 192, 333), (260, 48, 200)]
# Grids whose block -> tile remap (ps_gemm_plan.h) is more than the identity:
# the planned 2D-XCD rectangle, and the linear swizzle on more than 8 blocks.
# A fourth element "f32" runs the shape in fp32 (else bf16 in, f32 out).
XCD_GRIDS = [(2048, 4096, 64), (2048, 4096, 64, "f32"), (64, 32768, 64),
             (512, 512, 96)]
PARENT_TILE_ERR = {
    (300, 96, 320): 1.322e-06,    # 128x96
    (300, 192, 333): 1.561e-06,   # 128x96, two column tiles
    (260, 48, 200): 1.356e-06,    # 128x48
    (2048, 4096, 64): 5.933e-07,         # 128x128, rectangle 8x8
    (2048, 4096, 64, "f32"): 1.547e-06,  # the same plan on the fp32 MFMA
    (64, 32768, 64): 5.933e-07,          # 64x64, rectangle 1x64
    # 16 blocks, linear swizzle; one glds tile, then a 32-wide K tail
    (512, 512, 96): 5.355e-07,
}


def make_tile_data():
    out = {}
    for shape in PARENT_TILE_ERR:
        M, N, K = shape[:3]
        dt = torch.float32 if shape[3:] == ("f32",) else torch.bfloat16
        a = (rnd(M, K, seed=31) * 0.3).to(dt)
        b = (rnd(N, K, seed=32) * 0.3).to(dt)
        ref = a.double() @ b.double().t()
        out[shape] = (a, b, ref)
    return out


@pytest.fixture(scope="module")
def tile_data():
    return make_tile_data()


def tile_error(shape, t):
    from poseidon_amd.ops._backend import load
    M, N, K = shape[:3]
    a, b, ref = t  # already at the case's dtype
    out = load().gemm(a.to(DEV), b.to(DEV), M, N, K, True, True)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (M, N)
    return (out.cpu().double() - ref).abs().max().item()


def _check_tile(tile_data, shape):
    err = tile_error(shape, tile_data[shape])
    bound = 4.0 * PARENT_TILE_ERR[shape]
    print(f"gemm {shape}: max abs err {err:.3e} (bound {bound:.3e}, "
          f"parent {PARENT_TILE_ERR[shape]:.3e})")
    assert err <= bound, \
        f"gemm {shape}: max abs {err:.3e} > 4 x parent {PARENT_TILE_ERR[shape]:.3e}"


def _shape_id(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", N_FITTING, ids=_shape_id)
def test_n_fitting_tiles(tile_data, shape):
    _check_tile(tile_data, shape)


@pytest.mark.parametrize("shape", XCD_GRIDS, ids=_shape_id)
def test_remapped_grids(tile_data, shape):
    _check_tile(tile_data, shape)
