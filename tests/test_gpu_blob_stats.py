"""The blob-statistics kernels (ops.blob_stats / blob_stats_mt_* /
blob_stats_finalize): sum of |x|, largest finite |x| and the NaN / Inf count
of a dense tensor in one pass.

Exactness: values are drawn from {0, +-0.25, +-0.5, +-1, +-2} and every
tensor's sum of magnitudes stays below 2^22, so every partial sum in any
order is a multiple of 0.25 below 2^22 -- exact in fp32 -- and asum must
equal the float64 reference bit for bit. For a count n the largest magnitude
allowed is the largest of {2, 1, 0.5, 0.25} with n * vmax < 2^22; the value
set shrinks accordingly for the largest sizes.

General values (random normal) are held to the bound of the kernel's own
summation order: every add of non-negative terms loses at most 2^-24
relative, and a value passes through (longest serial chain per accumulator +
the depth of the tree over vector elements, accumulators, lanes, waves and
partials) adds, both taken from the planner."""

import functools
import math

import pytest
import torch

from poseidon_amd.ops import functional as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]


def _name(dtype):
    return "bf16" if dtype is BF16 else "f32"


def _values(n, dtype, seed, storage_offset=0):
    """n exact values as a view at storage_offset into a larger buffer."""
    vmax = next(v for v in (2.0, 1.0, 0.5, 0.25) if n * v < 2 ** 22)
    table = torch.tensor([v for v in (0, .25, -.25, .5, -.5, 1, -1, 2, -2)
                          if abs(v) <= vmax], dtype=torch.float32)
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, table.numel(), (n + storage_offset,), generator=g)
    buf = table[idx].to(DEV, dtype)
    return buf[storage_offset:]


def _stat(t, slot=1, nslots=3):
    out = ops.BlobStatsBuffer(nslots, DEV)
    ops.blob_stats(t, out, slot)
    ops.blob_stats_finalize(out)
    recs = out.records()
    assert all(r == (0.0, 0.0, 0) for i, r in enumerate(recs) if i != slot)
    return recs[slot]


def _ref(t):
    a = t.detach().abs().double()
    fin = torch.isfinite(a)
    m = float(a[fin].max()) if bool(fin.any()) else 0.0
    return float(a.sum()), m, int((~fin).sum())


@functools.lru_cache(maxsize=None)
def _big_count(itemsize):
    """A count that takes more than one grid-stride trip with the block
    count at its cap: more loads per thread than it has accumulators."""
    n = 1 << 16
    while ops.blob_stats_plan(n, itemsize)[1] < 3:
        n += n // 4  # small steps: the count must also keep n / 4 < 2^22
    n += 77
    blocks, chain = ops.blob_stats_plan(n, itemsize)
    assert chain >= 3 and blocks == ops.blob_stats_plan(16 * n, itemsize)[0]
    return n


def test_plan():
    for itemsize in (2, 4):
        assert ops.blob_stats_plan(1, itemsize) == (1, 1)
        b_small, _ = ops.blob_stats_plan(1000, itemsize)
        b_mid, _ = ops.blob_stats_plan(1 << 20, itemsize)
        b_big, c_big = ops.blob_stats_plan(_big_count(itemsize), itemsize)
        assert b_small == 1 < b_mid < b_big
        # proportional to bytes below the cap
        assert ops.blob_stats_plan(1 << 21, itemsize)[0] == 2 * b_mid
        assert c_big >= 3


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [1, 7, 8, 9, 255, 256, 257, 2049, 65537, "big"])
def test_exact_sizes(n, dtype):
    if n == "big":
        n = _big_count(dtype.itemsize)
    t = _values(n, dtype, seed=n)
    asum, maxabs, nf = _stat(t)
    want = _ref(t)
    assert want[0] < 2 ** 22
    assert (asum, maxabs, nf) == want


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("n", [5, 2049, 65537])
def test_storage_offsets(n, off, dtype):
    t = _values(n, dtype, seed=3 * n + off, storage_offset=off)
    assert t.storage_offset() == off
    assert _stat(t) == _ref(t)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_channels_last(dtype):
    t = _values(5 * 3 * 7 * 9, dtype, seed=4).view(5, 7, 9, 3).permute(
        0, 3, 1, 2)
    assert t.shape[1] == 3 and not t.is_contiguous()
    assert t.is_contiguous(memory_format=torch.channels_last)
    assert _stat(t) == _ref(t)
    # a permutation that is dense in no standard format
    assert _stat(t.permute(2, 0, 3, 1)) == _ref(t)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("off", [0, 1])
def test_nonfinite(off, dtype):
    n = 2049
    t = _values(n, dtype, seed=9, storage_offset=off)
    t[100] = 2.0  # the largest finite value, whatever the seed drew
    es = t.element_size()
    # first element at a 16-byte boundary after the start
    k = next(i for i in range(1, 16) if (t.data_ptr() + i * es) % 16 == 0)
    inf, nan = float("inf"), float("nan")
    only_inf = t.clone() if off == 0 else None
    t[0], t[n - 1], t[k - 1], t[k] = nan, inf, -inf, nan
    where = {0, n - 1, k - 1, k}
    asum, maxabs, nf = _stat(t)
    assert nf == len(where) and maxabs == 2.0 and math.isnan(asum)
    assert math.isnan(float(t.abs().sum()))
    if only_inf is not None:
        only_inf[0], only_inf[n - 1] = inf, -inf
        only_inf[k - 1], only_inf[k] = -inf, inf
        asum, maxabs, nf = _stat(only_inf)
        assert asum == inf == float(only_inf.abs().sum())
        assert nf == len(where) and maxabs == 2.0
    # nothing finite at all
    assert _stat(torch.full((9,), nan, device=DEV, dtype=dtype))[1:] == (0.0, 9)


def _five(seed):
    sizes = [(1, F32), (2049, BF16), (65537, F32), (255, BF16), (300000, BF16)]
    return [_values(n, dt, seed=seed + i, storage_offset=i % 2)
            for i, (n, dt) in enumerate(sizes)]


def test_multi_tensor_matches_single_launches():
    slots = [4, 0, 2, 5, 1]  # slot 3 stays unused
    for seed in (20, 40):  # second round: new tensors, a rebuilt table
        ts = _five(seed)
        single = ops.BlobStatsBuffer(6, DEV)
        for t, s in zip(ts, slots):
            ops.blob_stats(t, single, s)
        ops.blob_stats_finalize(single)
        multi = ops.BlobStatsBuffer(6, DEV)
        mt = ops.blob_stats_mt_prepare(ts, slots)
        before = ops.blob_stats_launches()
        ops.blob_stats_mt_run(mt, multi)
        assert ops.blob_stats_launches() == before + 1
        ops.blob_stats_finalize(multi)
        assert torch.equal(single.stats, multi.stats)
        recs = multi.records()
        assert recs[3] == (0.0, 0.0, 0)
        for t, s in zip(ts, slots):
            assert recs[s] == _ref(t)


def test_finalize_ranges_are_independent():
    out = ops.BlobStatsBuffer(4, DEV)
    ts = [_values(n, F32, seed=n) for n in (9, 2049, 257, 65537)]
    for s, t in enumerate(ts):
        ops.blob_stats(t, out, s)
    ops.blob_stats_finalize(out, 1, 2)
    recs = out.records()
    assert recs[0] == recs[3] == (0.0, 0.0, 0)
    assert recs[1] == _ref(ts[1]) and recs[2] == _ref(ts[2])
    with pytest.raises(IndexError):
        ops.blob_stats_finalize(out, 3, 2)
    with pytest.raises(IndexError):
        ops.blob_stats(ts[0], out, 4)


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
def test_same_bits_and_no_float_atomics(det):
    g = torch.Generator().manual_seed(1)
    ts = [torch.randn(300001, generator=g).to(DEV, dt) for dt in DTYPES]
    ops.set_deterministic(det)
    try:
        before = ops.float_atomic_launches()
        runs = []
        for _ in range(2):
            out = ops.BlobStatsBuffer(2, DEV)
            for s, t in enumerate(ts):
                ops.blob_stats(t, out, s)
            ops.blob_stats_finalize(out)
            runs.append(out.stats.clone())
        mt_out = ops.BlobStatsBuffer(2, DEV)
        ops.blob_stats_mt_run(ops.blob_stats_mt_prepare(ts, [0, 1]), mt_out)
        ops.blob_stats_finalize(mt_out)
        torch.cuda.synchronize()
        assert ops.float_atomic_launches() == before
    finally:
        ops.set_deterministic(False)
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    assert torch.equal(runs[0].view(torch.int32), mt_out.stats.view(torch.int32))


def test_bad_input_raises():
    out = ops.BlobStatsBuffer(1, DEV)
    t = torch.zeros(8, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.blob_stats(t[:, ::2], out, 0)      # gaps
    with pytest.raises(ValueError):
        ops.blob_stats(t[:, :4], out, 0)       # a column block
    with pytest.raises(ValueError):
        ops.blob_stats(t[0].expand(4, 8), out, 0)  # overlapping
    with pytest.raises(TypeError):
        ops.blob_stats(t.half(), out, 0)
    with pytest.raises(ValueError):
        ops.blob_stats_mt_prepare([t, t[:, ::2]], [0, 0])
    # the extension checks on its own as well
    with pytest.raises(RuntimeError):
        ops._ext().blob_stats(t[:, ::2], out.scratch, out.nblk, 0)
    with pytest.raises(RuntimeError):
        ops._ext().blob_stats(t, out.scratch, out.nblk, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_general_values_within_the_plan_bound(dtype):
    n = 1 << 20
    t = torch.randn(n, generator=torch.Generator().manual_seed(2)).to(DEV, dtype)
    asum, maxabs, nf = _stat(t)
    want, want_max, _ = _ref(t)
    blocks, chain = ops.blob_stats_plan(n, t.element_size())
    adds = chain + ops.blob_stats_reduce_depth(blocks, t.element_size())
    rel = abs(asum - want) / want
    print(f"{_name(dtype)}: blocks {blocks} chain {chain} adds {adds} "
          f"rel err {rel:.3e} bound {adds * 2.0 ** -24:.3e}")
    assert rel <= adds * 2.0 ** -24
    assert maxabs == want_max and nf == 0
