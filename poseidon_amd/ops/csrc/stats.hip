// Blob statistics for solver debug_info: one read-only streaming pass per
// tensor gives the fp32 sum of |x|, the largest finite |x| and the number of
// NaN / Inf elements. The result does not depend on element order, so any
// dense layout (NCHW, channels-last, a view at an odd offset) is read as the
// flat storage it is.
//
// Block b of a tensor's launch stores its partial to scratch[slot][b]; a
// finalize kernel, launched once per phase, sums every slot's partials in a
// fixed order. No float atomics, no cross-block hand-off: the same input
// gives the same bits on every run, eager or graph-replayed.
#include <cfloat>

#include <atomic>

#include "ps_api.h"
#include "ps_common.h"
#include "ps_mt.h"

namespace {

using namespace ps;

struct Acc {
  float s;
  float m;
  uint32_t nf;
};

// |x| of one element into a: the sum takes every value (NaN and Inf
// propagate), the max and the count split on finiteness
__device__ __forceinline__ void acc_abs(Acc& a, float ax, float& s) {
  s = ax;
  const bool fin = ax <= FLT_MAX;  // false for Inf and NaN
  a.m = fin ? fmaxf(a.m, ax) : a.m;
  a.nf += fin ? 0u : 1u;
}

// one 16-byte vector: the element magnitudes are tree-summed, then added to
// the accumulator once
template <bool BF16>
__device__ __forceinline__ void acc_vec(Acc& a, const uint4 r) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
  if (BF16) {
    float e[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // a bf16 is the high half of the fp32 with the same value
      acc_abs(a, fabsf(__uint_as_float(w[k] << 16)), e[2 * k]);
      acc_abs(a, fabsf(__uint_as_float(w[k] & 0xffff0000u)), e[2 * k + 1]);
    }
    a.s += ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
  } else {
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc_abs(a, fabsf(__uint_as_float(w[k])), e[k]);
    a.s += (e[0] + e[1]) + (e[2] + e[3]);
  }
}

template <bool BF16>
__device__ __forceinline__ float load_elem(const void* p, int64_t i) {
  if (BF16)
    return __uint_as_float((uint32_t)((const uint16_t*)p)[i] << 16);
  return ((const float*)p)[i];
}

__device__ __forceinline__ void merge(Acc& a, const Acc& b) {
  a.s += b.s;
  a.m = fmaxf(a.m, b.m);
  a.nf += b.nf;
}

// Block b of nb over n elements at p -> out[b]. Every read is inside
// [p, p + n): the head stops at n, vector i < nvec ends at element
// head + (i + 1) * VE <= head + nvec * VE <= n, the tail starts there.
template <bool BF16>
__device__ void stats_block(const void* p, int64_t n, int b, int nb,
                            StatsRec* out) {
  constexpr int ES = BF16 ? 2 : 4;
  constexpr int VE = STATS_VEC_BYTES / ES;
  const int tid = threadIdx.x;
  // scalar head up to the first 16-byte boundary of the data pointer (the
  // pointer itself is only element-aligned: blobs are views, params sit in
  // packed tables)
  int64_t head = (int64_t)((16 - ((uintptr_t)p & 15)) & 15) / ES;
  if (head > n) head = n;
  const int64_t nvec = (n - head) / VE;
  const int64_t tail0 = head + nvec * VE;
  const uint4* v = (const uint4*)((const char*)p + head * ES);

  Acc a[STATS_UNROLL];
#pragma unroll
  for (int u = 0; u < STATS_UNROLL; ++u) a[u] = {0.f, 0.f, 0u};

  const int64_t stride = (int64_t)nb * STATS_THREADS;
  int64_t i = (int64_t)b * STATS_THREADS + tid;
  for (; i + (STATS_UNROLL - 1) * stride < nvec; i += STATS_UNROLL * stride) {
    uint4 r[STATS_UNROLL];
#pragma unroll
    for (int u = 0; u < STATS_UNROLL; ++u) r[u] = v[i + u * stride];
#pragma unroll
    for (int u = 0; u < STATS_UNROLL; ++u) acc_vec<BF16>(a[u], r[u]);
  }
  // fewer than STATS_UNROLL loads left: one per accumulator, so no chain
  // grows by more than one
#pragma unroll
  for (int u = 0; u < STATS_UNROLL - 1; ++u) {
    if (i < nvec) {
      acc_vec<BF16>(a[u], v[i]);
      i += stride;
    }
  }
  if (b == 0) {
    float e;
    if (tid < head) {
      acc_abs(a[STATS_UNROLL - 1], fabsf(load_elem<BF16>(p, tid)), e);
      a[STATS_UNROLL - 1].s += e;
    } else if (tid - head < n - tail0) {
      // (a thread is in the head or in the tail, never both: both are
      // shorter than a vector)
      acc_abs(a[STATS_UNROLL - 1],
              fabsf(load_elem<BF16>(p, tail0 + (tid - head))), e);
      a[STATS_UNROLL - 1].s += e;
    }
  }

  // accumulators (tree), lanes (butterfly), waves (LDS, in wave order)
#pragma unroll
  for (int w = STATS_UNROLL / 2; w >= 1; w >>= 1)
#pragma unroll
    for (int u = 0; u < w; ++u) merge(a[u], a[u + w]);
  Acc t = a[0];
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) {
    Acc o;
    o.s = __shfl_xor(t.s, off);
    o.m = __shfl_xor(t.m, off);
    o.nf = (uint32_t)__shfl_xor((int)t.nf, off);
    merge(t, o);
  }
  constexpr int NW = STATS_THREADS / kWave;
  __shared__ StatsRec wave_part[NW];
  if ((tid & (kWave - 1)) == 0) wave_part[tid / kWave] = {t.s, t.m, t.nf, 0u};
  __syncthreads();
  if (tid == 0) {
    StatsRec r = wave_part[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      r.asum += wave_part[w].asum;
      r.maxabs = fmaxf(r.maxabs, wave_part[w].maxabs);
      r.nonfinite += wave_part[w].nonfinite;
    }
    out[b] = r;
  }
}

__device__ __forceinline__ void stats_dispatch(const void* p, int64_t n,
                                               int bf16, int slot, int b,
                                               int nb, StatsRec* scratch,
                                               int* nblk) {
  StatsRec* out = scratch + (int64_t)slot * STATS_MAX_BLOCKS;
  if (b == 0 && threadIdx.x == 0) nblk[slot] = nb;
  if (bf16)
    stats_block<true>(p, n, b, nb, out);
  else
    stats_block<false>(p, n, b, nb, out);
}

// single tensor: everything is a kernel argument, no table is read, so the
// launch is capturable whatever tensor it is given
__global__ void __launch_bounds__(STATS_THREADS)
blob_stats_k(const void* __restrict__ p, int64_t n, int bf16, int slot,
             StatsRec* __restrict__ scratch, int* __restrict__ nblk) {
  stats_dispatch(p, n, bf16, slot, blockIdx.x, gridDim.x, scratch, nblk);
}

__global__ void __launch_bounds__(STATS_THREADS)
blob_stats_mt_k(const StatsDesc* __restrict__ descs,
                const MTChunk* __restrict__ chunks,
                StatsRec* __restrict__ scratch, int* __restrict__ nblk) {
  const MTChunk ck = chunks[blockIdx.x];
  const StatsDesc d = descs[ck.t];
  stats_dispatch(d.p, d.n, d.bf16, d.slot, (int)ck.off, d.blocks, scratch,
                 nblk);
}

// one wave per slot: lane l adds partials l, l + 64, ... in index order,
// then the lanes combine in a butterfly. A slot nothing was launched for
// since the buffers were made (nblk 0) gets a zero record.
__global__ void __launch_bounds__(STATS_FINAL_LANES)
blob_stats_finalize_k(const StatsRec* __restrict__ scratch,
                      const int* __restrict__ nblk,
                      StatsRec* __restrict__ stats, int slot0) {
  const int slot = slot0 + blockIdx.x;
  const StatsRec* part = scratch + (int64_t)slot * STATS_MAX_BLOCKS;
  int nb = nblk[slot];
  if (nb > STATS_MAX_BLOCKS) nb = STATS_MAX_BLOCKS;
  Acc t = {0.f, 0.f, 0u};
  for (int j = threadIdx.x; j < nb; j += STATS_FINAL_LANES) {
    const StatsRec r = part[j];
    t.s += r.asum;
    t.m = fmaxf(t.m, r.maxabs);
    t.nf += r.nonfinite;
  }
#pragma unroll
  for (int off = STATS_FINAL_LANES / 2; off >= 1; off >>= 1) {
    Acc o;
    o.s = __shfl_xor(t.s, off);
    o.m = __shfl_xor(t.m, off);
    o.nf = (uint32_t)__shfl_xor((int)t.nf, off);
    merge(t, o);
  }
  if (threadIdx.x == 0) stats[slot] = {t.s, t.m, t.nf, 0u};
}

std::atomic<int64_t> g_stats_launches{0};

}  // namespace

extern "C" {

void ps_blob_stats(const void* p, int64_t n, int bf16, int slot,
                   void* scratch, int* nblk, hipStream_t s) {
  if (n <= 0) return;
  const StatsPlan plan = stats_plan(n, bf16 ? 2 : 4);
  g_stats_launches.fetch_add(1, std::memory_order_relaxed);
  blob_stats_k<<<dim3((unsigned)plan.blocks), STATS_THREADS, 0, s>>>(
      p, n, bf16, slot, (StatsRec*)scratch, nblk);
}

void ps_blob_stats_mt(const void* descs, const void* chunks, int nchunks,
                      void* scratch, int* nblk, hipStream_t s) {
  if (nchunks <= 0) return;
  g_stats_launches.fetch_add(1, std::memory_order_relaxed);
  blob_stats_mt_k<<<dim3((unsigned)nchunks), STATS_THREADS, 0, s>>>(
      (const StatsDesc*)descs, (const MTChunk*)chunks, (StatsRec*)scratch,
      nblk);
}

void ps_blob_stats_finalize(const void* scratch, const int* nblk, void* stats,
                            int slot0, int nslots, hipStream_t s) {
  if (nslots <= 0) return;
  g_stats_launches.fetch_add(1, std::memory_order_relaxed);
  blob_stats_finalize_k<<<dim3((unsigned)nslots), STATS_FINAL_LANES, 0, s>>>(
      (const StatsRec*)scratch, nblk, (StatsRec*)stats, slot0);
}

int64_t ps_blob_stats_launches(int reset) {
  return reset ? g_stats_launches.exchange(0) : g_stats_launches.load();
}

}  // extern "C"
