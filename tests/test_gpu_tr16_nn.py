"""NN tr16 GEMM (gemm.hip gemm_nn_tr_kernel) at the smallest shapes that reach
each of its sites. fp64 reference of the bf16-quantized inputs; every element
within rtol = atol = 1e-2 and the max abs error within 4x that of the same
call with the switch off (the generic kernel; test_gpu_tr16_tiles.py's margin
for another f32 summation order), floored at one f32 ulp of the largest value."""

import functools
import math

import pytest
import torch

from poseidon_amd.ops import functional as ops
from poseidon_amd.ops._backend import load

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def nn_on():
    was, skinny = ops.tr16_nn(), ops.skinny_splitk()
    ops.set_tr16_nn(True)
    yield
    ops.set_tr16_nn(was)
    ops.set_skinny_splitk(skinny)
    ops.set_deterministic(False)


@functools.lru_cache(maxsize=None)
def operands(M, N, K, dtype=torch.bfloat16):
    gen = torch.Generator().manual_seed(1000 * M + N + K)
    a = (torch.randn(M, K, generator=gen) * 0.3).to(dtype)
    b = (torch.randn(K, N, generator=gen) * 0.3).to(dtype)
    return a.to(DEV), b.to(DEV), a.double() @ b.double()


def close(out, ref):
    err = (out.cpu().double() - ref).abs()
    return bool((err <= 1e-2 + 1e-2 * ref.abs()).all()), err.max().item()


def check(run, ref, what):
    ops.set_tr16_nn(False)
    _, off_err = close(run(), ref)
    ops.set_tr16_nn(True)
    before = ops.tr16_nn_launches()
    on = run()
    assert ops.tr16_nn_launches() > before, what
    ok, err = close(on, ref)
    ulp = 2.0 ** (math.floor(math.log2(ref.abs().max().item())) - 23)
    print(f"{what}: max abs err {err:.3e} (switch off {off_err:.3e})")
    assert ok and err <= 4.0 * max(off_err, ulp), what
    return on


# (M, N, K): the skinny override (kmin, bm, bn, splitk) or None
GEMM_CASES = {
    (64, 64, 64): (0, 64, 64, 0),         # one tile, one k-step
    (128, 128, 128): (0, 128, 128, 0),    # the double-buffer flip
    (50, 64, 128): None,                  # clamped A rows, guarded stores
    (1, 64, 64): None,                    # the extreme ragged M
    (64, 64, 96): None,                   # 32-row tail
    (64, 64, 72): None,                   # one 16 B chunk of tail, prefetched
    (64, 192, 64): (0, 128, 128, 0),      # dead sub-image, dead waves
    (64, 64, 1096): (64, 64, 64, 4),      # slabs, ragged last slice, reduce
}


def run_gemm(shape, det=False):
    tune, (A, B, ref) = GEMM_CASES[shape], operands(*shape)
    ops.set_deterministic(det)
    if tune:
        ops.set_skinny_splitk(True, *tune)
    plan = ops.gemm_plan(*shape, True, False, True)
    assert plan["tr16_nn"], plan
    assert not tune or (plan["bm"], plan["bn"]) == tune[1:3], plan
    if tune and tune[3]:
        assert plan["splitk"] == tune[3] and plan["kchunk"] == 320, plan
        assert plan["ws_elems"] == tune[3] * shape[0] * shape[1], plan
    return check(lambda: load().gemm(A, B, *shape, True, False), ref,
                 f"nn {shape} det={det}")


@pytest.mark.parametrize("shape", GEMM_CASES, ids=str)
def test_nn_gemm(shape):
    run_gemm(shape)


def test_nn_gemm_deterministic():
    shape, atomics = (64, 64, 1096), ops.float_atomic_launches()
    first = run_gemm(shape, det=True)
    again = load().gemm(*operands(*shape)[:2], *shape, True, False)
    assert torch.equal(first, again)
    assert ops.float_atomic_launches() == atomics


# batch, Kin, Nout: ragged M with an 8-row K-tail; the fc8 contraction
@pytest.mark.parametrize("batch,kin,nout", [(50, 192, 136), (256, 128, 1000)])
def test_linear_backward_dx(batch, kin, nout):
    dy, w, ref = operands(batch, kin, nout)
    assert ops.gemm_plan(batch, kin, nout, True, False, True, False)["tr16_nn"]
    x = torch.zeros(batch, kin, device=DEV, dtype=torch.bfloat16)
    dx = check(lambda: ops.linear_backward(x, w.float(), dy, True, False,
                                           False)[0],
               ref, f"linear_backward dx {batch}x{kin}x{nout}")
    assert dx.dtype == torch.bfloat16 and dx.shape == (batch, kin)


@pytest.mark.parametrize("shape,bf16", [((64, 100, 64), True),
                                        ((64, 64, 68), True),
                                        ((64, 64, 64), False)], ids=str)
def test_ineligible_gemms_keep_the_generic_kernel(shape, bf16):
    A, B, ref = operands(*shape, torch.bfloat16 if bf16 else torch.float32)
    assert not ops.gemm_plan(*shape, True, False, bf16)["tr16_nn"]
    before = ops.tr16_nn_launches()
    assert close(load().gemm(A, B, *shape, True, False), ref)[0]
    assert ops.tr16_nn_launches() == before
    ops.set_tr16_nn(False)  # and off, what was eligible is not
    assert not ops.gemm_plan(128, 128, 128, True, False, True)["tr16_nn"]
