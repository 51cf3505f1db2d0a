// Device helpers of the lane-group softmax kernels (softmax_dense.hip,
// softmax_heads.hip): tile staging in 16-byte vectors, the element a lane
// holds in a slot, and max / sum inside a group of G lanes. Layout and plan:
// ps_softmax_dense_plan.h.
#pragma once

#include "ps_common.h"
#include "ps_softmax_dense_plan.h"

namespace ps {

namespace {

// global -> LDS (or back) of n elements: 16-byte vectors, then the last
// tile's ragged end by elements. Both sides are 16-byte aligned.
template <typename T>
__device__ inline void sd_copy(T* __restrict__ dst, const T* __restrict__ src,
                               int n) {
  constexpr int VN = 16 / (int)sizeof(T);
  const int nv = n / VN;
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  for (int v = threadIdx.x; v < nv; v += SD_THREADS) d4[v] = s4[v];
  for (int e = nv * VN + threadIdx.x; e < n; e += SD_THREADS) dst[e] = src[e];
}

// element of the row that lane j of a group holds in slot k
template <int G>
__device__ inline int sd_elem(int j, int k, int flip) {
  return j + ((k < 2 ? k ^ flip : k) * G);
}

// The value of the lane `OFF` away in a butterfly whose lower steps are done
// (every aligned run of OFF lanes already agrees). Inside a row of 16 lanes
// that is a DPP move on the VALU -- quad permutes for 1 and 2, and because
// the runs agree a half-row mirror stands in for 4 and a row mirror for 8;
// 16 and 32 cross rows and go through ds_bpermute. All lanes must be active.
template <int OFF>
__device__ inline float butterfly(float v) {
  if constexpr (OFF >= 16) {
    return __shfl_xor(v, OFF, 64);
  } else {
    constexpr int ctrl = OFF == 1 ? 0xB1     // quad_perm [1, 0, 3, 2]
                         : OFF == 2 ? 0x4E   // quad_perm [2, 3, 0, 1]
                         : OFF == 4 ? 0x141  // row_half_mirror
                                    : 0x140; // row_mirror
    const int i = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(i, i, ctrl, 0xF, 0xF, false));
  }
}

// max / sum over aligned groups of G lanes, every lane gets the result; the
// order of the additions is fixed by G alone
template <int G>
__device__ inline float group_max(float v) {
  if constexpr (G > 1) v = fmaxf(v, butterfly<1>(v));
  if constexpr (G > 2) v = fmaxf(v, butterfly<2>(v));
  if constexpr (G > 4) v = fmaxf(v, butterfly<4>(v));
  if constexpr (G > 8) v = fmaxf(v, butterfly<8>(v));
  if constexpr (G > 16) v = fmaxf(v, butterfly<16>(v));
  if constexpr (G > 32) v = fmaxf(v, butterfly<32>(v));
  return v;
}

template <int G>
__device__ inline float group_sum(float v) {
  if constexpr (G > 1) v += butterfly<1>(v);
  if constexpr (G > 2) v += butterfly<2>(v);
  if constexpr (G > 4) v += butterfly<4>(v);
  if constexpr (G > 8) v += butterfly<8>(v);
  if constexpr (G > 16) v += butterfly<16>(v);
  if constexpr (G > 32) v += butterfly<32>(v);
  return v;
}

// the tile's labels -> LDS, behind the tile itself
template <typename T>
__device__ inline float* sd_stage_labels(T* tile, const float* labels, int TR,
                                         int C, int nr) {
  float* lab = reinterpret_cast<float*>(
      reinterpret_cast<char*>(tile) + sd_tile_bytes(TR, C, (int)sizeof(T)));
  for (int i = threadIdx.x; i < nr; i += SD_THREADS) lab[i] = labels[i];
  return lab;
}

}  // namespace

// fn<T, G>(args) for the plan's G
#define SD_DISPATCH_G(G_, fn, ...)              \
  switch (G_) {                                 \
    case 1: fn<T, 1>(__VA_ARGS__); break;       \
    case 2: fn<T, 2>(__VA_ARGS__); break;       \
    case 4: fn<T, 4>(__VA_ARGS__); break;       \
    case 8: fn<T, 8>(__VA_ARGS__); break;       \
    case 16: fn<T, 16>(__VA_ARGS__); break;     \
    case 32: fn<T, 32>(__VA_ARGS__); break;     \
    default: fn<T, 64>(__VA_ARGS__); break;     \
  }

}  // namespace ps
