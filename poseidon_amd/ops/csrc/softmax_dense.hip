// Dense (per-position) softmax-with-loss: rows = N*H*W of a channels-last
// blob, C logits contiguous per row, one label per row -- the reference's
// SOFTMAX_LOSS over spatial_dim > 1 (softmax_loss_layer.cpp:46-55, :76-85).
// softmax.hip's wave-per-row kernels idle most lanes at the C of a
// segmentation net and read a row three times; these kernels give a row to a
// group of G lanes that keeps it in registers, and move whole tiles of rows
// through LDS in 16-byte vectors. Plan and LDS layout: ps_softmax_dense_plan.h.
//
//   forward   tile and its labels -> LDS; per row: max and sum inside the lane group by
//             shuffles, exp once, prob written back into the tile, the
//             label's lane adds -(x[label] - max - log sum); LDS -> prob;
//             next tile of the block. Then wave sums by shuffles, four wave
//             sums added in order and scaled by 1 / rows, and one atomicAdd
//             per block or (deterministic) partial[block]
//   backward  prob tile and its labels -> LDS; per row (p - onehot) * w in
//             place; LDS -> dx

#include <atomic>

#include "ps_common.h"
#include "ps_api.h"
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

// out: PARTIAL ? partial[gridDim.x] : loss[0] (pre-zeroed, added atomically);
// scale: what a block's sum of terms is multiplied by on its way out
template <typename T, int G, bool PARTIAL>
__global__ __launch_bounds__(SD_THREADS) void softmax_dense_fwd_k(
    const T* __restrict__ x, const float* __restrict__ labels,
    T* __restrict__ prob, float* __restrict__ out, int64_t rows, int C,
    int TR, int flip_on, float scale) {
  extern __shared__ uint4 sd_lds[];
  __shared__ float wave_nll[SD_THREADS / 64];
  T* tile = reinterpret_cast<T*>(sd_lds);
  constexpr int RB = SD_THREADS / G;  // rows of one pass
  const int tid = threadIdx.x;
  const int g = tid / G, j = tid & (G - 1);
  const int flip = flip_on ? sd_flip(tid & 63) : 0;
  float nll = 0.f;

  // a block walks tiles blockIdx.x, + gridDim.x, ...: its loss terms leave
  // it once, and a same-address atomic costs about what a tile does
  for (int64_t row0 = (int64_t)blockIdx.x * TR; row0 < rows;
       row0 += (int64_t)gridDim.x * TR) {
  const int nr = (int)(rows - row0 < TR ? rows - row0 : TR);
  sd_copy(tile, x + row0 * C, nr * C);
  const float* lab = sd_stage_labels(tile, labels + row0, TR, C, nr);
  __syncthreads();
  // uniform trip count: the shuffles below want whole waves
  for (int r0 = 0; r0 < nr; r0 += RB) {
    const int r = r0 + g;
    const bool live = r < nr;
    T* tr = tile + r * C;
    float xv[SD_MAX_PER_LANE];
    float m = -3.4e38f;
#pragma unroll
    for (int k = 0; k < SD_MAX_PER_LANE; ++k) {
      const int c = sd_elem<G>(j, k, flip);
      xv[k] = (live && c < C) ? to_f32(tr[c]) : -3.4e38f;
      m = fmaxf(m, xv[k]);
    }
    m = group_max<G>(m);
    float ev[SD_MAX_PER_LANE];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < SD_MAX_PER_LANE; ++k) {
      const int c = sd_elem<G>(j, k, flip);
      ev[k] = (live && c < C) ? __expf(xv[k] - m) : 0.f;
      sum += ev[k];
    }
    sum = group_sum<G>(sum);
    if (live) {
      const float inv = 1.0f / sum;
      int lbl = (int)lab[r];
      lbl = min(max(lbl, 0), C - 1);
      const float lse = m + __logf(sum);
#pragma unroll
      for (int k = 0; k < SD_MAX_PER_LANE; ++k) {
        const int c = sd_elem<G>(j, k, flip);
        if (c < C) {
          from_f32(ev[k] * inv, tr[c]);
          if (c == lbl) nll += lse - xv[k];
        }
      }
    }
  }
  __syncthreads();  // the tile now holds prob
  sd_copy(prob + row0 * C, tile, nr * C);
  __syncthreads();  // ... until the next one is staged over it
  }
  // every lane's terms -> the wave's, in the fixed order of the butterfly
  nll = group_sum<64>(nll);
  if ((tid & 63) == 0) wave_nll[tid >> 6] = nll;
  __syncthreads();
  if (tid == 0) {
    float v = wave_nll[0];
#pragma unroll
    for (int w = 1; w < SD_THREADS / 64; ++w) v += wave_nll[w];
    v *= scale;
    if (PARTIAL) out[blockIdx.x] = v;
    else atomicAdd(out, v);
  }
}

// dx = (prob - onehot(label)) * w; a label outside [0, C) matches nothing
template <typename T, int G>
__global__ __launch_bounds__(SD_THREADS) void softmax_dense_bwd_k(
    const T* __restrict__ prob, const float* __restrict__ labels,
    T* __restrict__ dx, int64_t rows, int C, int TR, int flip_on, float w) {
  extern __shared__ uint4 sd_lds[];
  T* tile = reinterpret_cast<T*>(sd_lds);
  constexpr int RB = SD_THREADS / G;
  const int64_t row0 = (int64_t)blockIdx.x * TR;
  const int nr = (int)(rows - row0 < TR ? rows - row0 : TR);
  const int tid = threadIdx.x;
  const int g = tid / G, j = tid & (G - 1);
  const int flip = flip_on ? sd_flip(tid & 63) : 0;

  sd_copy(tile, prob + row0 * C, nr * C);
  const float* lab = sd_stage_labels(tile, labels + row0, TR, C, nr);
  __syncthreads();
  for (int r = g; r < nr; r += RB) {
    T* tr = tile + r * C;
    const int lbl = (int)lab[r];
#pragma unroll
    for (int k = 0; k < SD_MAX_PER_LANE; ++k) {
      const int c = sd_elem<G>(j, k, flip);
      if (c < C)
        from_f32((to_f32(tr[c]) - (c == lbl ? 1.0f : 0.0f)) * w, tr[c]);
    }
  }
  __syncthreads();
  sd_copy(dx + row0 * C, tile, nr * C);
}

namespace {

std::atomic<int64_t> g_sd_launches{0};

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

SoftmaxDensePlan sd_checked_plan(int64_t rows, int C, int itemsize,
                                 int max_blocks, const void* a,
                                 const void* b) {
  const SoftmaxDensePlan p = sd_plan(rows, C, itemsize, max_blocks);
  if (p.G == 0 || p.tiles >= (int64_t)1 << 31 ||
      (((uintptr_t)a | (uintptr_t)b) & 15) != 0) {
    fprintf(stderr, "softmax dense: rows=%lld C=%d is outside the lane-group "
            "kernels (C <= %d, 16-byte aligned tensors)\n", (long long)rows, C,
            SD_MAX_C);
    abort();
  }
  return p;
}

template <typename T, int G>
void sd_fwd_g(const SoftmaxDensePlan& p, const T* x, const float* labels,
              T* prob, float* loss, float* partial, int64_t rows, int C,
              hipStream_t s) {
  const dim3 grid((unsigned)p.blocks);
  const float scale = (float)(1.0 / (double)rows);
  if (partial) {
    softmax_dense_fwd_k<T, G, true><<<grid, SD_THREADS, p.lds, s>>>(x, labels, prob, partial, rows, C, p.TR, p.flip, scale);
  } else {
    softmax_dense_fwd_k<T, G, false><<<grid, SD_THREADS, p.lds, s>>>(x, labels, prob, loss, rows, C, p.TR, p.flip, scale);
  }
}

template <typename T, int G>
void sd_bwd_g(const SoftmaxDensePlan& p, const T* prob, const float* labels,
              T* dx, int64_t rows, int C, float w, hipStream_t s) {
  const dim3 grid((unsigned)p.tiles);
  softmax_dense_bwd_k<T, G><<<grid, SD_THREADS, p.lds, s>>>(prob, labels, dx, rows, C, p.TR, p.flip, w);
}

template <typename T>
void sd_fwd(const T* x, const float* labels, T* prob, float* loss,
            float* partial, int64_t rows, int C, int max_blocks,
            hipStream_t s) {
  const SoftmaxDensePlan p =
      sd_checked_plan(rows, C, sizeof(T), max_blocks, x, prob);
  if (partial == nullptr) {
    if (ps_deterministic()) {
      fprintf(stderr, "softmax dense: deterministic mode needs partials\n");
      abort();
    }
    ps_count_float_atomic();
  }
  SD_DISPATCH_G(p.G, sd_fwd_g, p, x, labels, prob, loss, partial, rows, C, s);
  g_sd_launches.fetch_add(1, std::memory_order_relaxed);
  if (partial) ps_loss_sum(partial, loss, p.blocks, s);
}

template <typename T>
void sd_bwd(const T* prob, const float* labels, T* dx, int64_t rows, int C,
            float w, hipStream_t s) {
  const SoftmaxDensePlan p = sd_checked_plan(rows, C, sizeof(T), 0, prob, dx);
  SD_DISPATCH_G(p.G, sd_bwd_g, p, prob, labels, dx, rows, C, w, s);
  g_sd_launches.fetch_add(1, std::memory_order_relaxed);
}

}  // namespace

extern "C" {

int ps_softmax_dense_ok(int64_t rows, int64_t C, int itemsize) {
  return sd_lane_group_ok(rows, C, itemsize) ? 1 : 0;
}
int ps_softmax_dense_max_c() { return SD_MAX_C; }
int64_t ps_softmax_dense_blocks(int64_t rows, int C, int itemsize,
                                int max_blocks) {
  return sd_plan(rows, C, itemsize, max_blocks).blocks;
}
void ps_softmax_dense_fwd_f32(const float* x, const float* labels, float* prob,
                              float* loss, float* partial, int64_t rows, int C,
                              int max_blocks, hipStream_t s) {
  sd_fwd<float>(x, labels, prob, loss, partial, rows, C, max_blocks, s);
}
void ps_softmax_dense_fwd_bf16(const void* x, const float* labels, void* prob,
                               float* loss, float* partial, int64_t rows,
                               int C, int max_blocks, hipStream_t s) {
  sd_fwd<__bf16>((const __bf16*)x, labels, (__bf16*)prob, loss, partial, rows,
                 C, max_blocks, s);
}
void ps_softmax_dense_bwd_f32(const float* prob, const float* labels,
                              float* dx, int64_t rows, int C, float w,
                              hipStream_t s) {
  sd_bwd<float>(prob, labels, dx, rows, C, w, s);
}
void ps_softmax_dense_bwd_bf16(const void* prob, const float* labels, void* dx,
                               int64_t rows, int C, float w, hipStream_t s) {
  sd_bwd<__bf16>((const __bf16*)prob, labels, (__bf16*)dx, rows, C, w, s);
}
int64_t ps_softmax_dense_launches(int reset) {
  return reset ? g_sd_launches.exchange(0) : g_sd_launches.load();
}

}  // extern "C"

}  // namespace ps
