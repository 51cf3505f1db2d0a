// Row softmax + fused softmax-with-loss, one wave per row with shuffle
// reductions (vs the reference's 6-pass kernel chain, softmax_layer.cu:14-84,
// and its CPU-fallback loss layer, softmax_loss_layer.cu:12-22).
// Rows = N*H*W (NHWC spatial softmax) or batch (classifier logits);
// the reduced dim (channels/classes) is contiguous.

#include <cstdlib>

#include "ps_common.h"
#include "ps_api.h"

namespace ps {

__device__ inline float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_down(v, off, 64));
  return __shfl(v, 0, 64);
}

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

// 4 waves per block, one row per wave
template <typename T>
__global__ void softmax_rows_k(const T* x, T* y, int64_t rows, int C) {
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  int lane = threadIdx.x & 63;
  const T* xr = x + row * C;
  T* yr = y + row * C;
  float m = -3.4e38f;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, to_f32(xr[c]));
  m = wave_max(m);
  float sum = 0.f;
  for (int c = lane; c < C; c += 64) sum += __expf(to_f32(xr[c]) - m);
  sum = wave_sum(sum);
  float inv = 1.0f / sum;
  for (int c = lane; c < C; c += 64)
    from_f32(__expf(to_f32(xr[c]) - m) * inv, yr[c]);
}

// dx = (dy - sum_c(dy*y)) * y per row
template <typename T>
__global__ void softmax_bwd_rows_k(const T* y, const T* dy, T* dx,
                                   int64_t rows, int C) {
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  int lane = threadIdx.x & 63;
  const T* yr = y + row * C;
  const T* dyr = dy + row * C;
  T* dxr = dx + row * C;
  float dot = 0.f;
  for (int c = lane; c < C; c += 64) dot += to_f32(dyr[c]) * to_f32(yr[c]);
  dot = wave_sum(dot);
  for (int c = lane; c < C; c += 64)
    from_f32((to_f32(dyr[c]) - dot) * to_f32(yr[c]), dxr[c]);
}

// fused: prob + per-row NLL, loss accumulated into loss_out[0] (pre-zeroed),
// final normalization by batch on the host side wrapper (adds /n).
// ROWS (deterministic mode): loss_out is a rows-long buffer and row r's term
// is stored at loss_out[r]; loss_sum_k adds them up in a fixed order.
template <typename T, typename LT, bool ROWS = false>
__global__ void softmax_loss_fwd_k(const T* x, const LT* labels, T* prob,
                                   float* loss_out, int64_t rows, int C) {
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  int lane = threadIdx.x & 63;
  const T* xr = x + row * C;
  T* pr = prob + row * C;
  float m = -3.4e38f;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, to_f32(xr[c]));
  m = wave_max(m);
  float sum = 0.f;
  for (int c = lane; c < C; c += 64) sum += __expf(to_f32(xr[c]) - m);
  sum = wave_sum(sum);
  float inv = 1.0f / sum;
  for (int c = lane; c < C; c += 64)
    from_f32(__expf(to_f32(xr[c]) - m) * inv, pr[c]);
  if (lane == 0) {
    int lbl = (int)to_f32(labels[row]);
    lbl = min(max(lbl, 0), C - 1);
    float logp = to_f32(xr[lbl]) - m - __logf(sum);
    if (ROWS) loss_out[row] = -logp;
    else atomicAdd(loss_out, -logp);
  }
}

// One block: loss[0] += sum of row_loss[0 .. rows). Thread t adds rows t,
// t + 256, ... in ascending order, then a fixed LDS tree joins the 256
// partials -- the same order on every run.
__global__ void loss_sum_k(const float* __restrict__ row_loss,
                           float* __restrict__ loss, int64_t rows) {
  __shared__ float part[256];
  float v = 0.f;
  for (int64_t r = threadIdx.x; r < rows; r += 256) v += row_loss[r];
  part[threadIdx.x] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] += part[0];
}

template <typename T>
static void softmax_loss_fwd(const T* x, const float* labels, T* prob,
                             float* loss, float* row_loss, int64_t rows,
                             int C, hipStream_t s) {
  if (row_loss) {
    softmax_loss_fwd_k<T, float, true><<<cdiv64(rows, 4), 256, 0, s>>>(
        x, labels, prob, row_loss, rows, C);
    loss_sum_k<<<1, 256, 0, s>>>(row_loss, loss, rows);
    return;
  }
  if (ps_deterministic()) {
    fprintf(stderr, "softmax loss: deterministic mode needs row_loss\n");
    abort();
  }
  ps_count_float_atomic();
  softmax_loss_fwd_k<T, float><<<cdiv64(rows, 4), 256, 0, s>>>(
      x, labels, prob, loss, rows, C);
}

// dx = (prob - onehot) * w  (w = loss_weight / batch)
template <typename T, typename LT>
__global__ void softmax_loss_bwd_k(const T* prob, const LT* labels, T* dx,
                                   int64_t rows, int C, float w) {
  int64_t total = rows * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t row = i / C;
    int c = i % C;
    int lbl = (int)to_f32(labels[row]);
    float p = to_f32(prob[i]);
    from_f32((p - (c == lbl ? 1.0f : 0.0f)) * w, dx[i]);
  }
}

extern "C" {

void ps_softmax_rows_f32(const float* x, float* y, int64_t rows, int C,
                         hipStream_t s) {
  softmax_rows_k<float><<<cdiv64(rows, 4), 256, 0, s>>>(x, y, rows, C);
}
void ps_softmax_rows_bf16(const void* x, void* y, int64_t rows, int C,
                          hipStream_t s) {
  softmax_rows_k<__bf16><<<cdiv64(rows, 4), 256, 0, s>>>(
      (const __bf16*)x, (__bf16*)y, rows, C);
}
void ps_softmax_bwd_rows_f32(const float* y, const float* dy, float* dx,
                             int64_t rows, int C, hipStream_t s) {
  softmax_bwd_rows_k<float><<<cdiv64(rows, 4), 256, 0, s>>>(y, dy, dx, rows, C);
}
void ps_softmax_bwd_rows_bf16(const void* y, const void* dy, void* dx,
                              int64_t rows, int C, hipStream_t s) {
  softmax_bwd_rows_k<__bf16><<<cdiv64(rows, 4), 256, 0, s>>>(
      (const __bf16*)y, (const __bf16*)dy, (__bf16*)dx, rows, C);
}
void ps_softmax_loss_fwd_f32(const float* x, const float* labels, float* prob,
                             float* loss_out, float* row_loss, int64_t rows,
                             int C, hipStream_t s) {
  softmax_loss_fwd<float>(x, labels, prob, loss_out, row_loss, rows, C, s);
}
void ps_softmax_loss_fwd_bf16(const void* x, const float* labels, void* prob,
                              float* loss_out, float* row_loss, int64_t rows,
                              int C, hipStream_t s) {
  // labels stay fp32: class indices above 256 are not exactly representable
  // in bf16's 8-bit mantissa
  softmax_loss_fwd<__bf16>((const __bf16*)x, labels, (__bf16*)prob, loss_out,
                           row_loss, rows, C, s);
}
void ps_softmax_loss_bwd_f32(const float* prob, const float* labels, float* dx,
                             int64_t rows, int C, float w, hipStream_t s) {
  softmax_loss_bwd_k<float, float><<<ew_grid(rows * C), 256, 0, s>>>(
      prob, labels, dx, rows, C, w);
}
void ps_softmax_loss_bwd_bf16(const void* prob, const float* labels, void* dx,
                              int64_t rows, int C, float w, hipStream_t s) {
  softmax_loss_bwd_k<__bf16, float><<<ew_grid(rows * C), 256, 0, s>>>(
      (const __bf16*)prob, labels, (__bf16*)dx, rows, C, w);
}

}  // extern "C"

}  // namespace ps
