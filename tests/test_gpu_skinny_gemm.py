"""Skinny split-K GEMMs: the fc forward and data-gradient GEMMs at batch-sized
M, whose plan picks tile and split depth together so that the grid fills the
chip (ps_gemm_plan.h ps_skinny_plan); the split is reduced in slice order by
the reduce launch.

Every case runs through ops.linear_forward / ops.linear_backward(need_dx) on
a GEMM of the listed M x N x K -- forward with K-last B, dx with K-major B --
and is held to a bound that comes from the arithmetic alone, against an fp64
matmul of the (bf16-rounded) inputs:

    K * 2^-24 * sum_k |a_k b_k|       fp32 accumulation, any order
  + half a bf16 ulp of the result     where the output is bf16

(half an ulp of a bf16 y is 2^(floor(log2 |y|) - 8), between 2^-9 |y| and
2^-8 |y|; it is taken at |y_ref| plus the first term, the largest fp32 value
the rounding can have seen). The new path and the parent path (switch off)
must both hold it. References are computed once per shape and shared."""

import functools

import pytest
import torch

from poseidon_amd.ops import functional as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}

#  M    N     K     what it probes
SHAPES = [
    (8, 72, 1000),      # M and N under a tile, K tail
    (200, 1000, 1536),  # ragged M and N
    (256, 136, 4096),   # deepest split
    (32, 256, 2112),    # 33 staged bf16 tiles: no depth divides them evenly
]
EPILOGUES = {"bias_relu": (True, True), "bias": (True, False),
             "none": (False, False)}
# a forced depth on top of the planner's own: 2112 = 33 staged bf16 tiles on 8
# slices is 7 slices of 5, 5, 5, 5, 5, 5, 3 (the planner never leaves one
# empty; fp32 stages 16 columns, so it does get 8 slices of 17, ..., 13)
FORCED = {(32, 256, 2112): 8}


@pytest.fixture
def skinny_switch():
    """Leaves the process-wide switch on, its tune cleared."""
    yield
    ops.set_skinny_splitk(True)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _forward_case(M, N, K, dtype_name):
    """Inputs (CPU), fp64 reference before bias and the accumulation bound of
    y[M,N] = x[M,K] @ w[N,K]^T."""
    dtype = DTYPES[dtype_name]
    x = torch.randn(M, K, generator=_gen(M + N + K)).to(dtype)
    w = torch.randn(N, K, generator=_gen(M + N + K + 1))
    b = torch.randn(N, generator=_gen(M + N + K + 2))
    xr, wr = x.double(), w.to(dtype).double()
    ref = xr @ wr.t()
    acc = K * 2.0 ** -24 * (xr.abs() @ wr.abs().t())
    return x, w, b, ref, acc


@functools.lru_cache(maxsize=None)
def _dx_case(M, N, K, dtype_name):
    """dx[M,N] = dy[M,K] @ w[K,N]: the GEMM contracts the layer's outputs."""
    dtype = DTYPES[dtype_name]
    dy = torch.randn(M, K, generator=_gen(M + N + K + 3)).to(dtype)
    w = torch.randn(K, N, generator=_gen(M + N + K + 4))
    x = torch.zeros(M, N).to(dtype)
    dyr, wr = dy.double(), w.to(dtype).double()
    ref = dyr @ wr
    acc = K * 2.0 ** -24 * (dyr.abs() @ wr.abs())
    return x, w, dy, ref, acc


def _bound(ref, acc, dtype_name):
    if dtype_name == "fp32":
        return acc
    top = (ref.abs() + acc).clamp_min(2.0 ** -126)
    return acc + torch.exp2(torch.floor(torch.log2(top)) - 8)


def _check(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, "
          f"max err/bound {worst:.3f}")
    assert torch.isfinite(got).all(), what
    assert (err <= bound).all(), f"{what}: err/bound {worst:.3f}"


def _fwd_plan(M, N, K, dtype_name, bias):
    bf16 = dtype_name == "bf16"
    return ops.gemm_plan(M, N, K, True, True, bf16, out_f32=not bf16,
                         bias=bias)


def _dx_plan(M, N, K, dtype_name):
    bf16 = dtype_name == "bf16"
    return ops.gemm_plan(M, N, K, True, False, bf16, out_f32=not bf16)


def _atomic_c(dtype_name, bias, relu):
    # an fp32 C with nothing else landing in it keeps its atomic split
    return dtype_name == "fp32" and not bias and not relu


def _forward(case, bias, relu):
    x, w, b = case[0].to(DEV), case[1].to(DEV), case[2].to(DEV)
    return ops.linear_forward(x, w, b if bias else None, fuse_relu=relu)


def _dx(case):
    x, w, dy = case[0].to(DEV), case[1].to(DEV), case[2].to(DEV)
    return ops.linear_backward(x, w, dy, True, False, False)[0]


@pytest.mark.parametrize("epilogue", list(EPILOGUES))
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_holds_the_fp64_bound(shape, dtype_name, epilogue,
                                      skinny_switch):
    M, N, K = shape
    bias, relu = EPILOGUES[epilogue]
    case = _forward_case(M, N, K, dtype_name)
    ref = case[3] + (case[2].double() if bias else 0.0)
    if relu:
        ref = ref.clamp_min(0.0)
    # the bias is one more fp32 addend
    acc = case[4] + (2.0 ** -24 * case[2].double().abs() if bias else 0.0)
    bound = _bound(ref, acc, dtype_name)

    ops.set_skinny_splitk(True)
    plan = _fwd_plan(M, N, K, dtype_name, bias)
    if _atomic_c(dtype_name, bias, relu):
        assert not plan["skinny"] and plan["ws_elems"] == 0, plan
    else:
        assert plan["skinny"] and plan["splitk"] > 1, plan
        assert plan["ws_elems"] == plan["splitk"] * M * N, plan
    _check(_forward(case, bias, relu), ref, bound, f"new {plan}")

    depth = FORCED.get(shape)
    if depth and not _atomic_c(dtype_name, bias, relu):
        ops.set_skinny_splitk(True, splitk=depth)
        forced = _fwd_plan(M, N, K, dtype_name, bias)
        assert forced["skinny"] and forced["splitk"] > plan["splitk"]
        _check(_forward(case, bias, relu), ref, bound, f"forced {forced}")

    ops.set_skinny_splitk(False)
    parent = _fwd_plan(M, N, K, dtype_name, bias)
    assert not parent["skinny"], parent
    _check(_forward(case, bias, relu), ref, bound, f"parent {parent}")


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dx_holds_the_fp64_bound(shape, dtype_name, skinny_switch):
    M, N, K = shape
    case = _dx_case(M, N, K, dtype_name)
    ref, bound = case[3], _bound(case[3], case[4], dtype_name)

    ops.set_skinny_splitk(True)
    plan = _dx_plan(M, N, K, dtype_name)
    if dtype_name == "fp32":
        assert not plan["skinny"] and plan["ws_elems"] == 0, plan
    else:
        assert plan["skinny"] and plan["splitk"] > 1, plan
    _check(_dx(case), ref, bound, f"new {plan}")

    depth = FORCED.get(shape)
    if depth and dtype_name == "bf16":
        ops.set_skinny_splitk(True, splitk=depth)
        forced = _dx_plan(M, N, K, dtype_name)
        assert forced["skinny"] and forced["splitk"] > plan["splitk"]
        _check(_dx(case), ref, bound, f"forced {forced}")

    ops.set_skinny_splitk(False)
    parent = _dx_plan(M, N, K, dtype_name)
    assert not parent["skinny"], parent
    _check(_dx(case), ref, bound, f"parent {parent}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_five_calls_give_the_same_bits(shape, skinny_switch):
    M, N, K = shape
    ops.set_skinny_splitk(True)
    assert _fwd_plan(M, N, K, "bf16", True)["skinny"]
    assert _dx_plan(M, N, K, "bf16")["skinny"]
    assert _fwd_plan(M, N, K, "fp32", True)["skinny"]
    fwd, dx = _forward_case(M, N, K, "bf16"), _dx_case(M, N, K, "bf16")
    f32 = _forward_case(M, N, K, "fp32")
    first = (_forward(fwd, True, True), _dx(dx), _forward(f32, True, False))
    for _ in range(4):
        again = (_forward(fwd, True, True), _dx(dx),
                 _forward(f32, True, False))
        for a, b in zip(first, again):
            assert torch.equal(a, b)


def _two_gemms():
    """Two different skinny GEMMs: a forward with bias and ReLU and a dx."""
    (M1, N1, K1), (M2, N2, K2) = SHAPES[2], SHAPES[1]
    assert _fwd_plan(M1, N1, K1, "bf16", True)["splitk"] > 1
    assert _dx_plan(M2, N2, K2, "bf16")["splitk"] > 1
    fwd = [t.to(DEV) for t in _forward_case(M1, N1, K1, "bf16")[:3]]
    dx = [t.to(DEV) for t in _dx_case(M2, N2, K2, "bf16")[:3]]
    run_fwd = lambda: ops.linear_forward(fwd[0], fwd[1], fwd[2],
                                         fuse_relu=True)
    run_dx = lambda: ops.linear_backward(dx[0], dx[1], dx[2], True, False,
                                         False)[0]
    return run_fwd, run_dx


def test_graph_replays_match_eager(skinny_switch):
    """Five replays of a graph holding two skinny GEMMs back to back, each
    with its workspace and reduce launch, leave the eager bits every time."""
    ops.set_skinny_splitk(True)
    run_fwd, run_dx = _two_gemms()
    y_eager, dx_eager = run_fwd(), run_dx()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream
        run_fwd(), run_dx()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        y, dx = run_fwd(), run_dx()
    for _ in range(5):
        y.fill_(float("nan"))
        dx.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, y_eager) and torch.equal(dx, dx_eager)
    # and eager still gives them after the replays
    assert torch.equal(run_fwd(), y_eager)
    assert torch.equal(run_dx(), dx_eager)


def test_two_streams_match_one(skinny_switch):
    """Two skinny GEMMs issued on two streams at once, joined by events, each
    leave their single-stream bits: nothing of a split is shared between
    launches."""
    ops.set_skinny_splitk(True)
    run_fwd, run_dx = _two_gemms()
    y_one, dx_one = run_fwd(), run_dx()
    cur = torch.cuda.current_stream()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(5):
        start = torch.cuda.Event()
        start.record(cur)
        with torch.cuda.stream(s1):
            s1.wait_event(start)
            y = run_fwd()
            done1 = torch.cuda.Event()
            done1.record(s1)
        with torch.cuda.stream(s2):
            s2.wait_event(start)
            dx = run_dx()
            done2 = torch.cuda.Event()
            done2.record(s2)
        cur.wait_event(done1)
        cur.wait_event(done2)
        y.record_stream(cur)
        dx.record_stream(cur)
        assert torch.equal(y, y_one) and torch.equal(dx, dx_one)


def test_deterministic_mode_keeps_its_plans(skinny_switch):
    ops.set_skinny_splitk(True)
    was = ops.deterministic()
    try:
        ops.set_deterministic(True)
        for M, N, K in SHAPES + [(256, 4096, 9216)]:
            assert not _fwd_plan(M, N, K, "bf16", True)["skinny"]
            assert not _dx_plan(M, N, K, "bf16")["skinny"]
    finally:
        ops.set_deterministic(was)
