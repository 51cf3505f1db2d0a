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
#include "ps_softmax_dense_dev.h"  // sd_copy, sd_elem, group_max / group_sum

namespace ps {

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
void ps_softmax_dense_count_launch() {
  g_sd_launches.fetch_add(1, std::memory_order_relaxed);
}

}  // extern "C"

}  // namespace ps
