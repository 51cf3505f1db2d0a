// What a fully-convolutional net puts after its scores besides the loss: the
// plain SOFTMAX layer over the channels of every position, both ways, and the
// per-position ACCURACY. Rows = N*H*W of a channels-last blob, C contiguous
// elements each, fp32 or bf16 with fp32 arithmetic. The lane-group kernels
// share softmax_dense.hip's design (ps_softmax_dense_plan.h: G lanes a row,
// lane j owns elements j, j + G, j + 2G, whole tiles global <-> LDS in
// 16-byte vectors; helpers in ps_softmax_dense_dev.h).
//
//   forward   x tile -> LDS; per row max and sum inside the lane group, exp
//             once, y written back into the tile; LDS -> y. One tile a
//             block: nothing leaves a block but its tile.
//   backward  dx = (dy - sum_c dy * y) * y. Two tiles, y and dy, share the
//             block's LDS (sd_plan_streams(.., 2): about half the rows of the
//             forward's tile); the dot product is a group_sum; dx overwrites
//             the dy tile, each element by the lane that read it; LDS -> dx.
//   accuracy  row r with label l and v = x[r][l] is a hit iff fewer than
//             top_k elements rank ahead of l:
//               #{c : x[c] > v or (x[c] == v and c > l)} < top_k
//             -- the reference's partial_sort by std::greater<pair<value,
//             index>> (accuracy_layer.cpp:51-58) without the sort, ties going
//             to the higher index. l outside [0, C) or v NaN: a miss. The
//             lane group reads v from LDS (one address: a broadcast), every
//             lane counts over its own elements, group_sum, then wave and
//             block sums and ONE integer atomicAdd per block; blocks walk
//             tiles as the loss forward's do. Integer adds commute, so the
//             count is the same bits on every run and deterministic mode
//             needs nothing else. C > SD_MAX_C: one wave per row, lanes
//             stride over C, four rows a block pass, same counter.
//             accuracy = count / rows by a one-lane kernel: no host copy.
//
// From the gfx950 compile (hipcc -O3, -Rpass-analysis=kernel-resource-usage),
// over G = 1 .. 64: no scratch and no AGPRs anywhere, 8 waves a SIMD.
//   softmax_heads_fwd_k  58 VGPRs fp32, 59 bf16; dynamic LDS: the tile
//   softmax_heads_bwd_k  58 VGPRs fp32, 59 bf16; dynamic LDS: two tiles
//   accuracy_dense_k     46 .. 63 VGPRs fp32, 48 .. 64 bf16; dynamic LDS: the
//                        tile and its labels, and 16 bytes static
//   accuracy_rows_k      34 VGPRs fp32, 37 bf16; 16 bytes of static LDS
// Dynamic LDS is at most SD_TILE_BYTES = 16 KiB a block in every case.

#include "ps_common.h"
#include "ps_api.h"
#include "ps_softmax_dense_plan.h"
#include "ps_softmax_dense_dev.h"

namespace ps {

template <typename T, int G>
__global__ __launch_bounds__(SD_THREADS) void softmax_heads_fwd_k(
    const T* __restrict__ x, T* __restrict__ y, int64_t rows, int C, int TR,
    int flip_on) {
  extern __shared__ uint4 sh_lds[];
  T* tile = reinterpret_cast<T*>(sh_lds);
  constexpr int RB = SD_THREADS / G;  // rows of one pass
  const int64_t row0 = (int64_t)blockIdx.x * TR;
  const int nr = (int)(rows - row0 < TR ? rows - row0 : TR);
  const int tid = threadIdx.x;
  const int g = tid / G, j = tid & (G - 1);
  const int flip = flip_on ? sd_flip(tid & 63) : 0;

  sd_copy(tile, x + row0 * C, nr * C);
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
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < SD_MAX_PER_LANE; ++k) {
      const int c = sd_elem<G>(j, k, flip);
      xv[k] = (live && c < C) ? __expf(xv[k] - m) : 0.f;
      sum += xv[k];
    }
    sum = group_sum<G>(sum);
    if (live) {
      const float inv = 1.0f / sum;
#pragma unroll
      for (int k = 0; k < SD_MAX_PER_LANE; ++k) {
        const int c = sd_elem<G>(j, k, flip);
        if (c < C) from_f32(xv[k] * inv, tr[c]);
      }
    }
  }
  __syncthreads();  // the tile now holds y
  sd_copy(y + row0 * C, tile, nr * C);
}

template <typename T, int G>
__global__ __launch_bounds__(SD_THREADS) void softmax_heads_bwd_k(
    const T* __restrict__ y, const T* __restrict__ dy, T* __restrict__ dx,
    int64_t rows, int C, int TR, int flip_on) {
  extern __shared__ uint4 sh_lds[];
  T* ty = reinterpret_cast<T*>(sh_lds);
  T* td = reinterpret_cast<T*>(reinterpret_cast<char*>(sh_lds) +
                               sd_tile_bytes(TR, C, (int)sizeof(T)));
  constexpr int RB = SD_THREADS / G;
  const int64_t row0 = (int64_t)blockIdx.x * TR;
  const int nr = (int)(rows - row0 < TR ? rows - row0 : TR);
  const int tid = threadIdx.x;
  const int g = tid / G, j = tid & (G - 1);
  const int flip = flip_on ? sd_flip(tid & 63) : 0;

  sd_copy(ty, y + row0 * C, nr * C);
  sd_copy(td, dy + row0 * C, nr * C);
  __syncthreads();
  for (int r0 = 0; r0 < nr; r0 += RB) {  // uniform, as in the forward
    const int r = r0 + g;
    const bool live = r < nr;
    const T* yr = ty + r * C;
    T* dr = td + r * C;
    float yv[SD_MAX_PER_LANE], dv[SD_MAX_PER_LANE];
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < SD_MAX_PER_LANE; ++k) {
      const int c = sd_elem<G>(j, k, flip);
      const bool in = live && c < C;
      yv[k] = in ? to_f32(yr[c]) : 0.f;
      dv[k] = in ? to_f32(dr[c]) : 0.f;
      dot += dv[k] * yv[k];
    }
    dot = group_sum<G>(dot);
    if (live) {
#pragma unroll
      for (int k = 0; k < SD_MAX_PER_LANE; ++k) {
        const int c = sd_elem<G>(j, k, flip);
        if (c < C) from_f32((dv[k] - dot) * yv[k], dr[c]);
      }
    }
  }
  __syncthreads();  // the dy tile now holds dx
  sd_copy(dx + row0 * C, td, nr * C);
}

namespace {

// a label as the layers store it, a float: its class if that is one of C
__device__ inline bool acc_label(float lf, int C, int* lbl) {
  const bool ok = lf > -1.0f && lf < (float)C;  // false for NaN
  *lbl = ok ? (int)lf : 0;
  return ok;
}

// the block's hits -> count[0], one atomic (none for a block without hits)
__device__ inline void acc_block_add(int wave_total, int* wave_hits,
                                     int* __restrict__ count) {
  if ((threadIdx.x & 63) == 0) wave_hits[threadIdx.x >> 6] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < SD_THREADS / 64; ++w) n += wave_hits[w];
    if (n) atomicAdd(count, n);
  }
}

}  // namespace

template <typename T, int G>
__global__ __launch_bounds__(SD_THREADS) void accuracy_dense_k(
    const T* __restrict__ x, const float* __restrict__ labels,
    int* __restrict__ count, int64_t rows, int C, int TR, int flip_on,
    int top_k) {
  extern __shared__ uint4 sh_lds[];
  __shared__ int wave_hits[SD_THREADS / 64];
  T* tile = reinterpret_cast<T*>(sh_lds);
  constexpr int RB = SD_THREADS / G;
  const int tid = threadIdx.x;
  const int g = tid / G, j = tid & (G - 1);
  const int flip = flip_on ? sd_flip(tid & 63) : 0;
  // whole numbers kept as floats for the butterflies, and exact: a wave's
  // total is at most its share of the rows, 2^31 / (SD_MAX_BLOCKS * 4) =
  // 2^19 once the grid is capped and less than that before
  float hits = 0.f;

  for (int64_t row0 = (int64_t)blockIdx.x * TR; row0 < rows;
       row0 += (int64_t)gridDim.x * TR) {
    const int nr = (int)(rows - row0 < TR ? rows - row0 : TR);
    sd_copy(tile, x + row0 * C, nr * C);
    const float* lab = sd_stage_labels(tile, labels + row0, TR, C, nr);
    __syncthreads();
    for (int r0 = 0; r0 < nr; r0 += RB) {  // uniform, for the shuffles
      const int r = r0 + g;
      const T* tr = tile + r * C;
      int lbl;
      const bool ok = acc_label(r < nr ? lab[r] : -1.0f, C, &lbl);
      const float v = ok ? to_f32(tr[lbl]) : 0.f;  // one address a group
      float ahead = 0.f;
#pragma unroll
      for (int k = 0; k < SD_MAX_PER_LANE; ++k) {
        const int c = sd_elem<G>(j, k, flip);
        if (ok && c < C) {
          const float xc = to_f32(tr[c]);
          ahead += (xc > v || (xc == v && c > lbl)) ? 1.f : 0.f;
        }
      }
      ahead = group_sum<G>(ahead);
      if (ok && j == 0 && v == v && ahead < (float)top_k) hits += 1.f;
    }
    __syncthreads();  // before the next tile is staged over this one
  }
  hits = group_sum<64>(hits);
  acc_block_add((int)hits, wave_hits, count);
}

// C beyond the lane-group range: a wave a row, blocks stride over the rows
constexpr int ACC_ROWS_MAX_BLOCKS = 2048;

template <typename T>
__global__ __launch_bounds__(SD_THREADS) void accuracy_rows_k(
    const T* __restrict__ x, const float* __restrict__ labels,
    int* __restrict__ count, int64_t rows, int C, int top_k) {
  __shared__ int wave_hits[SD_THREADS / 64];
  const int lane = threadIdx.x & 63;
  int hits = 0;
  // the row is the wave's, so every lane of a wave takes the same trips
  for (int64_t row = (int64_t)blockIdx.x * (SD_THREADS / 64) +
                     (threadIdx.x >> 6);
       row < rows; row += (int64_t)gridDim.x * (SD_THREADS / 64)) {
    const T* xr = x + row * C;
    int lbl;
    const bool ok = acc_label(labels[row], C, &lbl);
    const float v = to_f32(xr[lbl]);
    int ahead = 0;
    for (int c = lane; c < C; c += 64) {
      const float xc = to_f32(xr[c]);
      ahead += (xc > v || (xc == v && c > lbl)) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ahead += __shfl_xor(ahead, off, 64);
    if (ok && v == v && ahead < top_k) ++hits;
  }
  acc_block_add(hits, wave_hits, count);
}

__global__ void accuracy_ratio_k(const int* __restrict__ count,
                                 float* __restrict__ acc, float rows) {
  acc[0] = (float)count[0] / rows;
}

namespace {

SoftmaxDensePlan sh_checked_plan(int64_t rows, int C, int itemsize,
                                 int streams, const void* a, const void* b,
                                 const void* c) {
  const SoftmaxDensePlan p = sd_plan_streams(rows, C, itemsize, streams);
  if (p.G == 0 || p.tiles >= (int64_t)1 << 31 ||
      (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) != 0) {
    fprintf(stderr, "softmax heads: rows=%lld C=%d is outside the lane-group "
            "kernels (C <= %d, 16-byte aligned tensors)\n", (long long)rows, C,
            SD_MAX_C);
    abort();
  }
  return p;
}

// the softmax kernels stage no labels: their LDS is the tiles alone
size_t sh_tiles_lds(const SoftmaxDensePlan& p) {
  return p.lds - 4 * (size_t)p.TR;
}

template <typename T, int G>
void sh_fwd_g(const SoftmaxDensePlan& p, const T* x, T* y, int64_t rows, int C,
              hipStream_t s) {
  softmax_heads_fwd_k<T, G><<<dim3((unsigned)p.tiles), SD_THREADS, sh_tiles_lds(p), s>>>(x, y, rows, C, p.TR, p.flip);
}

template <typename T, int G>
void sh_bwd_g(const SoftmaxDensePlan& p, const T* y, const T* dy, T* dx,
              int64_t rows, int C, hipStream_t s) {
  softmax_heads_bwd_k<T, G><<<dim3((unsigned)p.tiles), SD_THREADS, sh_tiles_lds(p), s>>>(y, dy, dx, rows, C, p.TR, p.flip);
}

template <typename T, int G>
void sh_acc_g(const SoftmaxDensePlan& p, const T* x, const float* labels,
              int* count, int64_t rows, int C, int top_k, hipStream_t s) {
  accuracy_dense_k<T, G><<<dim3((unsigned)p.blocks), SD_THREADS, p.lds, s>>>(x, labels, count, rows, C, p.TR, p.flip, top_k);
}

template <typename T>
void sh_fwd(const T* x, T* y, int64_t rows, int C, hipStream_t s) {
  const SoftmaxDensePlan p =
      sh_checked_plan(rows, C, sizeof(T), 1, x, y, nullptr);
  SD_DISPATCH_G(p.G, sh_fwd_g, p, x, y, rows, C, s);
  ps_softmax_dense_count_launch();
}

template <typename T>
void sh_bwd(const T* y, const T* dy, T* dx, int64_t rows, int C,
            hipStream_t s) {
  const SoftmaxDensePlan p = sh_checked_plan(rows, C, sizeof(T), 2, y, dy, dx);
  SD_DISPATCH_G(p.G, sh_bwd_g, p, y, dy, dx, rows, C, s);
  ps_softmax_dense_count_launch();
}

template <typename T>
void sh_accuracy(const T* x, const float* labels, int* count, float* acc,
                 int64_t rows, int C, int top_k, int lane_groups,
                 hipStream_t s) {
  if (rows < 1 || rows >= (int64_t)1 << 31 || C < 1 || top_k < 1 ||
      top_k > C) {
    fprintf(stderr, "accuracy: rows=%lld C=%d top_k=%d is outside the "
            "kernels (1 <= top_k <= C, rows < 2^31)\n", (long long)rows, C,
            top_k);
    abort();
  }
  if (lane_groups && sd_lane_group_ok(rows, C, sizeof(T))) {
    const SoftmaxDensePlan p =
        sh_checked_plan(rows, C, sizeof(T), 1, x, nullptr, nullptr);
    SD_DISPATCH_G(p.G, sh_acc_g, p, x, labels, count, rows, C, top_k, s);
    ps_softmax_dense_count_launch();
  } else {
    const int64_t blocks = cdiv64(rows, SD_THREADS / 64);
    const dim3 grid((unsigned)(blocks < ACC_ROWS_MAX_BLOCKS
                                   ? blocks : ACC_ROWS_MAX_BLOCKS));
    accuracy_rows_k<T><<<grid, SD_THREADS, 0, s>>>(x, labels, count, rows, C, top_k);
  }
  accuracy_ratio_k<<<1, 1, 0, s>>>(count, acc, (float)rows);
}

}  // namespace

extern "C" {

void ps_softmax_heads_fwd_f32(const float* x, float* y, int64_t rows, int C,
                              hipStream_t s) {
  sh_fwd<float>(x, y, rows, C, s);
}
void ps_softmax_heads_fwd_bf16(const void* x, void* y, int64_t rows, int C,
                               hipStream_t s) {
  sh_fwd<__bf16>((const __bf16*)x, (__bf16*)y, rows, C, s);
}
void ps_softmax_heads_bwd_f32(const float* y, const float* dy, float* dx,
                              int64_t rows, int C, hipStream_t s) {
  sh_bwd<float>(y, dy, dx, rows, C, s);
}
void ps_softmax_heads_bwd_bf16(const void* y, const void* dy, void* dx,
                               int64_t rows, int C, hipStream_t s) {
  sh_bwd<__bf16>((const __bf16*)y, (const __bf16*)dy, (__bf16*)dx, rows, C, s);
}
void ps_accuracy_rows_f32(const float* x, const float* labels, int* count,
                          float* acc, int64_t rows, int C, int top_k,
                          int lane_groups, hipStream_t s) {
  sh_accuracy<float>(x, labels, count, acc, rows, C, top_k, lane_groups, s);
}
void ps_accuracy_rows_bf16(const void* x, const float* labels, int* count,
                           float* acc, int64_t rows, int C, int top_k,
                           int lane_groups, hipStream_t s) {
  sh_accuracy<__bf16>((const __bf16*)x, labels, count, acc, rows, C, top_k,
                      lane_groups, s);
}

}  // extern "C"

}  // namespace ps
