"""The tall tr16 TN tiles (96/128/192 rows, gemm.hip gemm_tn_tr_kernel) and
the ragged last N tile, at the smallest shapes that reach each piece. The
planner gives such small problems the 64-row tile (too few blocks to fill
the chip), so every case forces its tile through set_tr16_tune.

Tolerance: max abs error against an fp64 reference built from the
bf16-quantized inputs. PARENT_ERR is that same error measured for the 64-row
tiles of the commit before the tall tiles existed; the tall tiles get 4x it
(another split-K slicing changes the fp32 summation order), and never more
than the project's rtol = atol = 1e-2. Every element is held to the bound:
a dropped k-tile or a swapped sub-image moves whole 16x16 blocks by
O(sqrt(64) * sigma^2), orders of magnitude above it."""

import pytest
import torch

from poseidon_amd.ops import functional as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _ext():
    from poseidon_amd.ops._backend import load
    return load()


def _check(out, ref64, parent_err, what):
    err = (out.detach().cpu().double() - ref64).abs()
    bound = 4.0 * parent_err
    loose = 1e-2 * ref64.abs().clamp(min=1.0)   # rtol = atol = 1e-2
    print(f"{what}: max abs err {err.max().item():.3e} "
          f"(bound {bound:.3e}, parent {parent_err:.3e})")
    assert bool((err <= loose).all()), \
        f"{what}: max abs {err.max().item():.3e} beyond rtol=atol=1e-2"
    assert err.max().item() <= bound, \
        f"{what}: max abs {err.max().item():.3e} > 4 x parent {parent_err:.3e}"


# (M, N, K), forced tile, max abs error of the parent's 64-row path (worst
# of three runs on an MI355X: split-K atomics reorder the sum run to run)
TN_CASES = [
    # one 128x128 tile, two k-tiles, no split
    ((128, 128, 128), (128, 128), 6.16e-07),
    # ragged last N tile + split-K
    ((128, 192, 1024), (128, 128), 1.72e-06),
    # the 192-row tile (three 64-column sub-images), ragged N
    ((192, 320, 1024), (192, 128), 2.03e-06),
    # the 96-row tile (64 + 32 sub-images)
    ((96, 384, 2048), (96, 128), 2.70e-06),
    # three row tiles; split-K padded for the XCD clustering, so padded bz
    # blocks exit early
    ((384, 256, 4096), (128, 128), 5.36e-06),
    # N smaller than BN: the whole second half is dead
    ((128, 64, 512), (128, 128), 1.10e-06),
]


@pytest.fixture(scope="module")
def tn_data():
    out = {}
    for (M, N, K), _tile, _e in TN_CASES:
        opA = rnd(M, K, seed=5) * 0.3
        opB = rnd(K, N, seed=6) * 0.3
        ref = opA.to(torch.bfloat16).double() @ opB.to(torch.bfloat16).double()
        out[(M, N, K)] = (opA, opB, ref)
    return out


@pytest.mark.parametrize("shape,tile,parent_err", TN_CASES,
                         ids=[f"{s[0]}x{s[1]}x{s[2]}" for s, _, _ in TN_CASES])
def test_tn_tall_tiles(tn_data, shape, tile, parent_err):
    ext = _ext()
    M, N, K = shape
    opA, opB, ref = tn_data[shape]
    A = opA.t().contiguous().to(DEV, torch.bfloat16)  # [K, M] K-major
    B = opB.contiguous().to(DEV, torch.bfloat16)      # [K, N] K-major
    ext.set_tr16_tune(tile[0], tile[1], 0)
    try:
        out = ext.gemm(A, B, M, N, K, False, False)
        torch.cuda.synchronize()
    finally:
        ext.set_tr16_tune(0, 0, 0)
    assert out.dtype == torch.float32
    _check(out, ref, parent_err, f"tn {tile[0]}x{tile[1]} at {M}x{N}x{K}")


# implicit-gather wgrads: batch 4, 3x3 / stride 1 / pad 1 on 8x8 (K = 256),
# Kg = 144 -> N = 192: ragged, with pad columns beyond kg_max. Parent error:
# (into a zero dw, into a pre-filled dw).
WGRAD_CASES = [
    (dict(C=32, G=2, Co=256), (128, 128), (1.08e-05, 1.26e-05)),   # M = 128
    (dict(C=32, G=2, Co=384), (192, 128), (1.32e-05, 1.49e-05)),   # M = 192
    (dict(C=16, G=1, Co=96), (96, 128), (1.04e-05, 1.06e-05)),     # M = 96
]


@pytest.fixture(scope="module")
def wgrad_data():
    out = {}
    for cfg, _tile, _e in WGRAD_CASES:
        C, G, Co = cfg["C"], cfg["G"], cfg["Co"]
        x = rnd(4, C, 8, 8, seed=21)
        dy = rnd(4, Co, 8, 8, seed=22)
        dw0 = rnd(Co, C // G, 3, 3, seed=23)
        xq = x.to(torch.bfloat16).double()
        dyq = dy.to(torch.bfloat16).double()
        ref = torch.nn.grad.conv2d_weight(xq, list(dw0.shape), dyq, stride=1,
                                          padding=1, groups=G)
        out[Co] = (x, dy, dw0, ref)
    return out


@pytest.mark.parametrize("prefill", [False, True], ids=["zero", "prefilled"])
@pytest.mark.parametrize("cfg,tile,parent_err", WGRAD_CASES,
                         ids=[f"Co{c['Co']}" for c, _, _ in WGRAD_CASES])
def test_implicit_wgrad_tall_tiles(wgrad_data, cfg, tile, parent_err, prefill):
    ext = _ext()
    C, G, Co = cfg["C"], cfg["G"], cfg["Co"]
    x, dy, dw0, ref = wgrad_data[Co]
    xg = x.to(DEV, torch.bfloat16)
    w = torch.zeros(Co, C // G, 3, 3, device=DEV)
    # the unpack ACCUMULATES into dw: a non-zero dw must survive
    base = dw0 if prefill else torch.zeros_like(dw0)
    dw = base.clone().to(DEV)
    ops.set_implicit_gemm(True)
    ext.set_tr16_tune(tile[0], tile[1], 0)
    try:
        _y, cache = ops.conv2d_forward_ex(xg, w, None, (1, 1), (1, 1), G)
        colT, _wkT = cache
        ops.conv2d_backward_weight_acc(xg, colT, dy.to(DEV, torch.bfloat16),
                                       dw, None, (1, 1), (1, 1), G)
        torch.cuda.synchronize()
    finally:
        ext.set_tr16_tune(0, 0, 0)
        ops.set_implicit_gemm(False)
    _check(dw, ref + base.double(), parent_err[1 if prefill else 0],
           f"implicit wgrad {tile[0]}x{tile[1]} Co={Co} prefill={prefill}")
