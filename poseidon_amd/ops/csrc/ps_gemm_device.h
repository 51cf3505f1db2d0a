// Device code shared by the GEMM translation units (gemm.hip's generic tiles
// and gemm_split.hip's split-precision tiles): the implicit-GEMM address, the
// epilogue of a 16x16-fragment accumulator tile and the split-K reduce.
#pragma once
#include <type_traits>

#include "ps_common.h"
#include "ps_gather.h"

namespace ps {

// Implicit-GEMM address: row = im2col row (n,oh,ow), k = column within the
// group slice (khw*Cg + cg). Returns the NHWC x address of k's element run
// (contiguous along cg), or the zero page for padding. Valid for vector
// loads that stay inside one cg-run (callers guarantee k%VEC==0, Cg%VEC==0).
// The integer logic lives in ps_gather.h.
template <typename T>
__device__ inline const T* gather_addr(const GatherDesc& ga, int64_t row, int k) {
  if (k >= ga.kg_max) return (const T*)ga.zero;  // padded columns
  const GatherRow r = ps_gather_row(ga, (int)row);
  const GatherTap t = ps_gather_tap(ga, k);
  if (ps_gather_oob(ga, r, t, k)) return (const T*)ga.zero;
  return (const T*)ga.x + ps_gather_offset(r, t);
}

// Epilogue: C/D fragment map for 16x16 shapes: col = lane&15,
// row = (lane>>4)*4 + r (guide §3; dtype-independent on gfx950).
// bz is the split-K slice (the workspace slab it writes).
template <typename OUT, int FM, int FN, bool HAS_BIAS, bool SPLITK>
__device__ inline void gemm_epilogue(const f32x4 (&acc)[FM][FN],
                                     OUT* __restrict__ C,
                                     const float* __restrict__ bias,
                                     float* __restrict__ ws, int M, int N,
                                     int64_t ldc, float alpha, float beta,
                                     bool relu, int bz, int m0, int n0,
                                     int wm, int wn, int lane) {
#pragma unroll
  for (int fm = 0; fm < FM; ++fm) {
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      int col = n0 + wn + fn * 16 + (lane & 15);
      if (col >= N) continue;
      float bv = HAS_BIAS ? bias[col] : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wm + fm * 16 + (lane >> 4) * 4 + r;
        if (row >= M) continue;
        if (SPLITK) {
          if (ws) {
            // raw partial; alpha/beta/bias applied by the reduce kernel
            ws[((int64_t)bz * M + row) * N + col] = acc[fm][fn][r];
          } else if constexpr (std::is_same<OUT, float>::value) {
            // atomic split-K: accumulate straight into zeroed f32 C --
            // no workspace round-trip, no reduce kernel; lets the launcher
            // split K much deeper (wgrad tiles are tiny: M=Cout)
            atomicAdd(&C[(int64_t)row * ldc + col], alpha * acc[fm][fn][r]);
          }
        } else {
          int64_t idx = (int64_t)row * ldc + col;
          float v = alpha * acc[fm][fn][r] + bv;
          if (beta != 0.0f) v += beta * to_f32(C[idx]);
          if (relu && v < 0.0f) v = 0.0f;  // fused in-place ReLU epilogue
          from_f32(v, C[idx]);
        }
      }
    }
  }
}

// combine split-K partial slabs: C = alpha*sum_s ws[s] + bias + beta*C
template <typename OUT, bool HAS_BIAS>
__global__ void splitk_reduce_k(const float* __restrict__ ws,
                                OUT* __restrict__ C,
                                const float* __restrict__ bias,
                                int M, int N, int64_t ldc, int splitk,
                                float alpha, float beta, bool relu) {
  int64_t MN = (int64_t)M * N;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < MN;
       i += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    for (int s = 0; s < splitk; ++s) v += ws[s * MN + i];
    int row = i / N, col = i % N;
    v *= alpha;
    if (HAS_BIAS) v += bias[col];
    int64_t idx = (int64_t)row * ldc + col;
    if (beta != 0.0f) v += beta * to_f32(C[idx]);
    if (relu && v < 0.0f) v = 0.0f;
    from_f32(v, C[idx]);
  }
}

}  // namespace ps
