// Device helpers shared by the fused backward tails of a conv block
// (conv -> relu -> [lrn] -> [max pool]): the max-pool gradient gather and the
// bias-gradient block reduction. The LRN, pool and ReLU backward kernels pull
// them in behind compile-time flags so that one pass over the conv output
// produces dx (masked by the ReLU) and the conv's bias gradient.
//
// Every value rounds where the unfused chain of kernels rounded it: the pool
// sum to the storage type, then the consumer's dx to the storage type, then
// the ReLU mask -- so the fused dx is bit-identical to the chain's.
#pragma once

#include <cstdlib>

#include "ps_common.h"
#include "ps_api.h"

namespace ps {

// Gradient of one max-pool INPUT pixel (n, h, w), channels [c0, c0 + V):
// scans the covering windows in (oh, ow) order, sums dy where the stored
// window-local argmax points at this pixel (f32), and returns the sum rounded
// to the storage type T. This IS maxpool_bwd_k's body.
template <typename T, int V>
__device__ inline void maxpool_gather(const T* __restrict__ dy,
                                      const uint8_t* __restrict__ mask,
                                      const PoolGeom& g, int n, int h, int w,
                                      int c0, float* out) {
  typedef T vec_t __attribute__((ext_vector_type(V)));
  typedef uint8_t mvec_t __attribute__((ext_vector_type(V)));
  int oh0 = (h + g.ph < g.kh) ? 0 : (h + g.ph - g.kh) / g.sh + 1;
  int oh1 = min((h + g.ph) / g.sh + 1, g.Ho);
  int ow0 = (w + g.pw < g.kw) ? 0 : (w + g.pw - g.kw) / g.sw + 1;
  int ow1 = min((w + g.pw) / g.sw + 1, g.Wo);
  float acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = 0.f;
  for (int oh = oh0; oh < oh1; ++oh)
    for (int ow = ow0; ow < ow1; ++ow) {
      int64_t oi = ((((int64_t)n * g.Ho + oh) * g.Wo + ow) * g.C) + c0;
      int local = (h - (oh * g.sh - g.ph)) * g.kw + (w - (ow * g.sw - g.pw));
      mvec_t mv = *reinterpret_cast<const mvec_t*>(&mask[oi]);
      vec_t dv = *reinterpret_cast<const vec_t*>(&dy[oi]);
#pragma unroll
      for (int e = 0; e < V; ++e)
        if ((int)mv[e] == local) acc[e] += to_f32(dv[e]);
    }
#pragma unroll
  for (int e = 0; e < V; ++e) {
    T o;
    from_f32(acc[e], o);
    out[e] = to_f32(o);
  }
}

// ReLU backward of an already rounded gradient by the post-ReLU activation:
// what relu_bwd_k computes at slope 0 (g * 0 keeps its sign bit).
__device__ inline float relu_mask(float x, float g) {
  return x > 0.f ? g : g * 0.f;
}

// Bias-gradient epilogue. Each thread accumulated acc[V] over pixels for the
// FIXED channels [c0, c0 + V) (its channel chunk never changes across the
// grid-stride loop). part is C floats of LDS: bias_sum_init zeroes it, the
// flush folds every thread's registers into it with LDS atomics and issues
// ONE global atomicAdd per (block, column). Both contain a barrier: every
// thread of the block must reach them.
__device__ inline void bias_sum_init(float* part, int C) {
  for (int c = threadIdx.x; c < C; c += blockDim.x) part[c] = 0.f;
  __syncthreads();
}

template <int V>
__device__ inline void bias_sum_flush(float* part, const float* acc, int c0,
                                      bool owns, float* __restrict__ db,
                                      int C) {
  if (owns) {
#pragma unroll
    for (int j = 0; j < V; ++j) atomicAdd(&part[c0 + j], acc[j]);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) atomicAdd(&db[c], part[c]);
}

// Host side of a launch that ends in bias_sum_flush (db != null): counted as
// an atomic-float launch. Deterministic mode has no such launch -- the
// bindings run the tail without db and sum the stored dx with the ordered
// colsum instead -- so reaching here with the mode on is fatal.
static inline void bias_flush_launch(const float* db, const char* what) {
  if (!db) return;
  if (ps_deterministic()) {
    fprintf(stderr, "%s: atomic bias flush in deterministic mode\n", what);
    abort();
  }
  ps_count_float_atomic();
}

// Grid of a flat grid-stride kernel over nvec V-wide chunks (CV per row)
// whose threads must keep their channel chunk: blocks * 256 is a multiple of
// CV, or no thread runs a second iteration at all.
static inline unsigned bias_flat_blocks(int64_t nvec, int CV, int max_blocks) {
  int64_t need = cdiv64(nvec, 256);
  if (need <= max_blocks) return (unsigned)need;
  int a = CV, b = 256;
  while (b) { int t = a % b; a = b; b = t; }
  const int m = CV / a;  // blocks must be a multiple of m
  int64_t blocks = (int64_t)max_blocks / m * m;
  if (blocks == 0) blocks = m;
  return (unsigned)(blocks < need ? blocks : need);
}

}  // namespace ps
