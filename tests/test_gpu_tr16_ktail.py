"""K-tail of the tr16 TN kernel (gemm.hip gemm_tn_tr_kernel<KT>): K % 64 != 0
at the smallest shapes that reach each tail site. Scheme of
test_gpu_tr16_tiles.py: fp64 reference of the bf16-quantized inputs, every
element within rtol = atol = 1e-2, max abs error within 4x the parent commit's
(its generic kernel, worst of three runs on an MI355X, listed per case)."""

import functools

import pytest
import torch

from poseidon_amd.ops import functional as ops
from poseidon_amd.ops._backend import load

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(autouse=True)
def ktail_on():
    was = ops.tr16_ktail()
    ops.set_tr16_ktail(True)
    yield
    ops.set_tr16_ktail(was)
    load().set_tr16_tune(0, 0, 0)
    ops.set_implicit_gemm(False)
    ops.set_deterministic(False)


def _check(out, ref64, parent_err, what):
    err = (out.detach().cpu().double() - ref64).abs()
    print(f"{what}: max abs err {err.max().item():.3e} "
          f"(parent {parent_err:.3e})")
    assert bool((err <= 1e-2 * ref64.abs().clamp(min=1.0)).all()), what
    assert err.max().item() <= 4.0 * parent_err, what


# (M, N, K): (forced tile and split-K block target, parent max abs error)
TN_CASES = {
    (64, 64, 96): ((64, 64, 0), 3.13e-07),    # full tile + 32-row tail
    (64, 64, 129): ((64, 64, 0), 5.56e-07),   # 1-row tail
    # 4 slices of 256, the last of 8 rows: the prologue stages the tail
    (64, 64, 776): ((64, 64, 0), 1.84e-06),
    # GoogLeNet's K, tall tile, ragged last N tile; 4 slices of 448
    (128, 192, 1568): ((128, 128, 8), 2.18e-06),
    (96, 384, 1000): ((96, 128, 0), 1.71e-06),    # 64 + 32 sub-images
    (384, 256, 4136): ((128, 128, 0), 5.26e-06),  # padded bz blocks exit
}


@functools.lru_cache(maxsize=None)
def tn_operands(shape):
    M, N, K = shape
    a, b = rnd(M, K, seed=5) * 0.3, rnd(K, N, seed=6) * 0.3
    ref = a.to(torch.bfloat16).double() @ b.to(torch.bfloat16).double()
    return (a.t().contiguous().to(DEV, torch.bfloat16),
            b.contiguous().to(DEV, torch.bfloat16), ref)


def run_tn(shape, det):
    tune, parent_err = TN_CASES[shape]
    A, B, ref = tn_operands(shape)
    ops.set_deterministic(det)
    load().set_tr16_tune(*tune)
    plan = ops.gemm_plan(*shape, False, False, True)
    assert plan["tr16"] and (plan["bm"], plan["bn"]) == tune[:2], plan
    if shape == (64, 64, 776):
        assert plan["splitk"] == 4 and plan["kchunk"] == 256, plan
        assert (plan["ws_elems"] > 0) == det, plan
    outs = [load().gemm(A, B, *shape, False, False) for _ in range(2)]
    torch.cuda.synchronize()
    assert not det or torch.equal(outs[0], outs[1])
    _check(outs[0], ref, parent_err, f"tn {tune} at {shape} det={det}")


@pytest.mark.parametrize("shape", TN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_tn_ktail(shape):
    run_tn(shape, det=False)


def test_tn_ktail_deterministic():
    run_tn((64, 64, 776), det=True)


def test_switch_off_keeps_the_generic_plan():
    ops.set_tr16_ktail(False)
    assert not ops.gemm_plan(128, 832, 1568, False, False, True)["tr16"]


# conv wgrads: batch 4, 3x3 / stride 1 / pad 1 on 7x7: K = 196 (a tail of 4),
# Kg = 144 -> N = 192 ragged with pad columns. Parent error by prefill (the
# implicit and the materialized path gave the same figures).
WGRAD_CASES = [((16, 1, 64), (0, 0), (6.01e-06, 6.82e-06)),
               ((32, 2, 256), (128, 128), (1.16e-05, 1.28e-05))]


@functools.lru_cache(maxsize=None)
def wgrad_operands(C, G, Co):
    x, dy = rnd(4, C, 7, 7, seed=21), rnd(4, Co, 7, 7, seed=22)
    dw0 = rnd(Co, C // G, 3, 3, seed=23)
    ref = torch.nn.grad.conv2d_weight(
        x.to(torch.bfloat16).double(), list(dw0.shape),
        dy.to(torch.bfloat16).double(), stride=1, padding=1, groups=G)
    return x, dy, dw0, ref


@pytest.mark.parametrize("prefill", [False, True], ids=["zero", "prefilled"])
@pytest.mark.parametrize("implicit", [True, False],
                         ids=["implicit", "materialized"])
@pytest.mark.parametrize("cfg,tile,parent_err", WGRAD_CASES,
                         ids=[f"Co{c[2]}" for c, _, _ in WGRAD_CASES])
def test_wgrad_ktail(cfg, tile, parent_err, implicit, prefill):
    C, G, Co = cfg
    x, dy, dw0, ref = wgrad_operands(*cfg)
    base = dw0 if prefill else torch.zeros_like(dw0)
    xg = x.to(DEV, torch.bfloat16)
    dw = base.clone().to(DEV)  # the unpack ACCUMULATES into dw
    ops.set_implicit_gemm(implicit)
    load().set_tr16_tune(*tile, 0)
    _y, cache = ops.conv2d_forward_ex(
        xg, torch.zeros(Co, C // G, 3, 3, device=DEV), None, (1, 1), (1, 1), G)
    ops.conv2d_backward_weight_acc(xg, cache[0], dy.to(DEV, torch.bfloat16),
                                   dw, None, (1, 1), (1, 1), G)
    torch.cuda.synchronize()
    _check(dw, ref + base.double(), parent_err[prefill],
           f"wgrad {cfg} implicit={implicit} prefill={prefill}")
