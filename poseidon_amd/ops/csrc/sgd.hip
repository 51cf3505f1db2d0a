// Fused optimizer updates: one kernel per (param, iteration) replaces the
// reference's 4-6 cuBLAS axpy/scal call sequence per param
// (solver.cpp:858-892 SGD, :1013-1120 Nesterov, :1240-1364 AdaGrad).
// Params and history are fp32 master copies; float4-vectorized.

#include "ps_common.h"
#include "ps_mt.h"

namespace ps {

__global__ void u64_inc_k(unsigned long long* p) { *p += 1; }

// hist = mom*hist + lr*(g + wd*w); w -= hist. LRDEV reads lr from device
// memory so a hipGraph replay can see per-iteration learning rates.
template <bool LRDEV>
__global__ void sgd_update_k(float* __restrict__ w, const float* __restrict__ g,
                             float* __restrict__ h, int64_t n, float lr_or_mult,
                             float mom, float wd, const float* __restrict__ lr_dev) {
  const float lr = LRDEV ? lr_dev[0] * lr_or_mult : lr_or_mult;
  int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (; i + 4 <= n; i += stride) {
    f32x4 wv = *(f32x4*)&w[i];
    f32x4 gv = *(const f32x4*)&g[i];
    f32x4 hv = *(f32x4*)&h[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      hv[j] = mom * hv[j] + lr * (gv[j] + wd * wv[j]);
      wv[j] -= hv[j];
    }
    *(f32x4*)&w[i] = wv;
    *(f32x4*)&h[i] = hv;
  }
}

template <bool LRDEV>
__global__ void sgd_update_tail_k(float* w, const float* g, float* h,
                                  int64_t start, int64_t n, float lr_or_mult,
                                  float mom, float wd, const float* lr_dev) {
  const float lr = LRDEV ? lr_dev[0] * lr_or_mult : lr_or_mult;
  int64_t i = start + threadIdx.x;
  if (i < n) {
    float hv = mom * h[i] + lr * (g[i] + wd * w[i]);
    h[i] = hv;
    w[i] -= hv;
  }
}

// update = (1+mom)*h_new - mom*h_old
__global__ void nesterov_update_k(float* w, const float* g, float* h,
                                  int64_t n, float lr, float mom, float wd) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float h_old = h[i];
    float h_new = mom * h_old + lr * (g[i] + wd * w[i]);
    h[i] = h_new;
    w[i] -= (1.0f + mom) * h_new - mom * h_old;
  }
}

// hist += g^2; w -= lr * g / (sqrt(hist) + delta)
__global__ void adagrad_update_k(float* w, const float* g, float* h,
                                 int64_t n, float lr, float delta, float wd) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gv = g[i] + wd * w[i];
    float hv = h[i] + gv * gv;
    h[i] = hv;
    w[i] -= lr * gv / (sqrtf(hv) + delta);
  }
}

// ---------------------------------------------------------------------------
// Multi-tensor apply: GoogLeNet has ~116 param tensors, so per-param update
// and zero launches cost more than the math (128 sgd_update_k + 116 zero_
// launches/iter in the profile). One launch covers every param via a
// device-resident (tensor-descriptor, chunk) table built once at solver
// setup -- shapes are static so the table never changes. Table layouts:
// ps_mt.h.
// ---------------------------------------------------------------------------

typedef __bf16 bf16x4v __attribute__((ext_vector_type(4)));

// A desc with a shadow also stores the new weight as bf16, with the cast of
// repack_mt_k's straight-cast branch: the fc forward of the next step reads
// the same bits that repack would write, without the pass that re-reads w.
template <bool LRDEV>
__global__ void sgd_mt_k(const MTDesc* __restrict__ descs,
                         const MTChunk* __restrict__ chunks, float lr_scalar,
                         float mom, const float* __restrict__ lr_dev) {
  const MTChunk ck = chunks[blockIdx.x];
  const MTDesc d = descs[ck.t];
  const float lr = (LRDEV ? lr_dev[0] : lr_scalar) * d.lr_mult;
  const float wd = d.wd;
  __bf16* const sh = (__bf16*)d.shadow;
  int64_t i = ck.off + (int64_t)threadIdx.x * 4;
#pragma unroll
  for (int it = 0; it < MT_CHUNK / (256 * 4); ++it, i += 256 * 4) {
    if (i + 4 <= d.n) {
      f32x4 wv = *(f32x4*)&d.w[i];
      f32x4 gv = *(const f32x4*)&d.g[i];
      f32x4 hv = *(f32x4*)&d.h[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        hv[j] = mom * hv[j] + lr * (gv[j] + wd * wv[j]);
        wv[j] -= hv[j];
      }
      *(f32x4*)&d.w[i] = wv;
      *(f32x4*)&d.h[i] = hv;
      if (sh) {
        bf16x4v o = {(__bf16)wv[0], (__bf16)wv[1], (__bf16)wv[2],
                     (__bf16)wv[3]};
        *(bf16x4v*)(sh + i) = o;
      }
    } else if (i < d.n) {
      for (int64_t k = i; k < d.n; ++k) {
        float hv = mom * d.h[k] + lr * (d.g[k] + wd * d.w[k]);
        d.h[k] = hv;
        const float wn = d.w[k] - hv;
        d.w[k] = wn;
        if (sh) sh[k] = (__bf16)wn;
      }
    }
  }
}

// Multi-tensor conv weight repack: one launch refreshes EVERY conv's bf16
// khwc shadow + per-group dgrad transpose from the fp32 masters
// (GoogLeNet: 2 launches instead of 68 x ~5 us repack kernels per step).
__global__ void repack_mt_k(const MTRepackDesc* __restrict__ descs,
                            const MTChunk* __restrict__ chunks) {
  const MTChunk ck = chunks[blockIdx.x];
  const MTRepackDesc d = descs[ck.t];
  const int Cog = d.Co / d.G;
  const int Kg = d.kh * d.kw * d.Cig;
  const int KW = d.kw, KH = d.kh, Cig = d.Cig;
  if (KW == 1 && KH == 1 && d.G == 1 && !d.wkT && d.ldk == Cig) {
    // fc shadows: khwc degenerates to a straight cast -- skip the
    // per-element divides (VGG: 102M of 138M repacked elements)
    int64_t i = ck.off + (int64_t)threadIdx.x * 4;
#pragma unroll
    for (int it = 0; it < MT_CHUNK / (256 * 4); ++it, i += 256 * 4) {
      if (i + 4 <= d.n) {
        f32x4 v = *(const f32x4*)&d.src[i];
        bf16x4v o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        *(bf16x4v*)((__bf16*)d.wk + i) = o;
      } else if (i < d.n) {
        for (int64_t k = i; k < d.n; ++k)
          ((__bf16*)d.wk)[k] = (__bf16)d.src[k];
      }
    }
    return;
  }
  for (int64_t i = ck.off + threadIdx.x;
       i < ck.off + MT_CHUNK && i < d.n; i += 256) {
    int kkw = (int)(i % KW);
    int64_t t = i / KW;
    int kkh = (int)(t % KH); t /= KH;
    int ci = (int)(t % Cig);
    int co = (int)(t / Cig);
    const float v = d.src[i];
    const int kg = (kkh * KW + kkw) * Cig + ci;
    ((__bf16*)d.wk)[(int64_t)co * d.ldk +
                    ps_khwc_col(kkh, kkw, ci, d.kw_ld, d.c_ld)] = (__bf16)v;
    if (d.wkT)  // IP shadows need only the row-major form
      ((__bf16*)d.wkT)[((int64_t)(co / Cog) * Kg + kg) * Cog + co % Cog] =
          (__bf16)v;
  }
}

// inverse of repack_mt_k for GRADIENTS: khwc fp32 wgrad scratch -> NCHW
// fp32 param diff, accumulating (beta=1) unless the desc says overwrite
// (a diff with this one writer, which then nobody has to zero). One launch
// covers every conv's unpack at the end of backward (GoogLeNet: 57
// weight_from_khwc launches -> 1) -- single-GPU mode only; DWBP needs
// per-layer grads final.
__global__ void unpack_mt_k(const MTUnpackDesc* __restrict__ descs,
                            const MTChunk* __restrict__ chunks) {
  const MTChunk ck = chunks[blockIdx.x];
  const MTUnpackDesc d = descs[ck.t];
  const int KW = d.kw, KH = d.kh, Cig = d.Cig;
  for (int64_t i = ck.off + threadIdx.x;
       i < ck.off + MT_CHUNK && i < d.n; i += 256) {
    int kkw = (int)(i % KW);
    int64_t t = i / KW;
    int kkh = (int)(t % KH); t /= KH;
    int ci = (int)(t % Cig);
    int co = (int)(t / Cig);
    const float v = d.dwk[(int64_t)co * d.ldk +
                          ps_khwc_col(kkh, kkw, ci, d.kw_ld, d.c_ld)];
    d.dw[i] = d.overwrite ? v : d.dw[i] + v;
  }
}

__global__ void zero_mt_k(const MTZeroDesc* __restrict__ descs,
                          const MTChunk* __restrict__ chunks) {
  const MTChunk ck = chunks[blockIdx.x];
  const MTZeroDesc d = descs[ck.t];
  int64_t i = ck.off + (int64_t)threadIdx.x * 4;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int it = 0; it < MT_CHUNK / (256 * 4); ++it, i += 256 * 4) {
    if (i + 4 <= d.n)
      *(f32x4*)&d.p[i] = z;
    else if (i < d.n)
      for (int64_t k = i; k < d.n; ++k) d.p[k] = 0.f;
  }
}

// fp32 master -> bf16 shadow copy (for the bf16 compute path)
__global__ void f32_to_bf16_k(const float* src, __bf16* dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = (__bf16)src[i];
}

extern "C" {

void ps_sgd_update(float* w, const float* g, float* h, int64_t n, float lr,
                   float mom, float wd, hipStream_t s) {
  int64_t nv = n / 4;
  if (nv > 0)
    sgd_update_k<false><<<ew_grid(nv), 256, 0, s>>>(w, g, h, nv * 4, lr, mom,
                                                    wd, nullptr);
  if (n % 4)
    sgd_update_tail_k<false><<<1, 4, 0, s>>>(w, g, h, n & ~3LL, n, lr, mom,
                                             wd, nullptr);
}

// lr = lr_dev[0] * lr_mult (lr_mult folds the per-param blobs_lr)
void ps_sgd_update_lrdev(float* w, const float* g, float* h, int64_t n,
                         float lr_mult, float mom, float wd,
                         const float* lr_dev, hipStream_t s) {
  int64_t nv = n / 4;
  if (nv > 0)
    sgd_update_k<true><<<ew_grid(nv), 256, 0, s>>>(w, g, h, nv * 4, lr_mult,
                                                   mom, wd, lr_dev);
  if (n % 4)
    sgd_update_tail_k<true><<<1, 4, 0, s>>>(w, g, h, n & ~3LL, n, lr_mult,
                                            mom, wd, lr_dev);
}

void ps_u64_inc(void* p, hipStream_t s) {
  u64_inc_k<<<1, 1, 0, s>>>((unsigned long long*)p);
}

void ps_sgd_mt(const void* descs, const void* chunks, int nchunks, float lr,
               float mom, const float* lr_dev, hipStream_t s) {
  if (nchunks <= 0) return;
  if (lr_dev)
    sgd_mt_k<true><<<dim3((unsigned)nchunks), 256, 0, s>>>(
        (const MTDesc*)descs, (const MTChunk*)chunks, lr, mom, lr_dev);
  else
    sgd_mt_k<false><<<dim3((unsigned)nchunks), 256, 0, s>>>(
        (const MTDesc*)descs, (const MTChunk*)chunks, lr, mom, nullptr);
}

void ps_repack_mt(const void* descs, const void* chunks, int nchunks,
                  hipStream_t s) {
  if (nchunks <= 0) return;
  repack_mt_k<<<dim3((unsigned)nchunks), 256, 0, s>>>(
      (const MTRepackDesc*)descs, (const MTChunk*)chunks);
}

void ps_unpack_mt(const void* descs, const void* chunks, int nchunks,
                  hipStream_t s) {
  if (nchunks <= 0) return;
  unpack_mt_k<<<dim3((unsigned)nchunks), 256, 0, s>>>(
      (const MTUnpackDesc*)descs, (const MTChunk*)chunks);
}

void ps_zero_mt(const void* descs, const void* chunks, int nchunks,
                hipStream_t s) {
  if (nchunks <= 0) return;
  zero_mt_k<<<dim3((unsigned)nchunks), 256, 0, s>>>(
      (const MTZeroDesc*)descs, (const MTChunk*)chunks);
}

void ps_nesterov_update(float* w, const float* g, float* h, int64_t n,
                        float lr, float mom, float wd, hipStream_t s) {
  nesterov_update_k<<<ew_grid(n), 256, 0, s>>>(w, g, h, n, lr, mom, wd);
}

void ps_adagrad_update(float* w, const float* g, float* h, int64_t n,
                       float lr, float delta, float wd, hipStream_t s) {
  adagrad_update_k<<<ew_grid(n), 256, 0, s>>>(w, g, h, n, lr, delta, wd);
}

void ps_f32_to_bf16(const float* src, void* dst, int64_t n, hipStream_t s) {
  f32_to_bf16_k<<<ew_grid(n), 256, 0, s>>>(src, (__bf16*)dst, n);
}

}  // extern "C"

}  // namespace ps
