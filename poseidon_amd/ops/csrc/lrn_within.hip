// LRN, norm_region WITHIN_CHANNEL, NHWC layout: one forward and one backward
// kernel. Channels are independent; the window is size x size pixels of one
// channel, stride 1, centred, and the divisor is always size^2 (zero padding
// counts). With R = (size - 1) / 2 and a = alpha / size^2:
//
//   s(p)  = 1 + a * sum_{q in win(p)} x(q)^2
//   y(p)  = x(p) * s(p)^-beta
//   r(q)  = dy(q) * x(q) * s(q)^(-beta-1)
//   dx(p) = dy(p) * s(p)^-beta - 2*a*beta * x(p) * sum_{q in win(p)} r(q)
//
// A lane owns one 16-byte channel vector (V channels) of one pixel column
// and walks down a strip of rows. Its neighbours along W sit cvb lanes away
// in the same block, so the horizontal part of a box sum is an exchange
// through an LDS row buffer; its neighbours along H are itself one row
// later, so the vertical part is a register ring of 2R + 1 partial window
// sums. Both halves are separable sums: every x is loaded once per strip
// (plus halo rows and columns, recomputed by the neighbouring blocks).
//
// Lanes are laid out (segment, pixel slot, channel vector), ps_lrn_within_
// plan.h: a segment is the pixels one block emits of one image row plus
// halo slots each side, and narrow images put segments of several images in
// one block. Nothing travels by wave shuffles -- a segment may straddle a
// wave. Pixels outside the image and idle lanes load nothing and exchange
// zeros, which is exactly the zero padding.
//
// The backward keeps no scale tensor: it recomputes s with the same walk
// and chains a second box filter over r behind it.

#include <atomic>

#include "ps_common.h"
#include "ps_lrn_within_plan.h"

// This file's device code is built without the packed fp32 VALU forms
// (v_pk_*_f32): the same as -target-feature -packed-fp32-ops, which the
// extension build cannot pass to one source alone.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace ps {
namespace {

// sc^-beta (pw) and 1/sc (inv); lrn.hip's rsqrt forms for beta = 0.75
__device__ __forceinline__ void lrnw_pow(float sc, float beta, float& pw,
                                         float& inv) {
  const float r = rsqrtf(sc);
  inv = r * r;
  pw = (beta == 0.75f) ? r * sqrtf(r) : __powf(sc, -beta);
}

// Global I/O of one lane's V channels: one 16-byte access (V = 8 bf16, 4
// fp32) or one element (V = 1).
template <typename T, int V>
struct LrnwIO {
  typedef T raw_t __attribute__((ext_vector_type(V)));
  __device__ static __forceinline__ raw_t zero() {
    raw_t r;
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = (T)0.f;
    return r;
  }
  __device__ static __forceinline__ void unpack(const raw_t& r, float* v) {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = (float)r[j];
  }
  __device__ static __forceinline__ raw_t pack(const float* v) {
    raw_t r;
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = (T)v[j];
    return r;
  }
};

// LDS row buffer: one fp32 vector per lane, stored as V / 4 planes of
// [256] f32x4 (V = 1: one plane of floats), so a wave's accesses are
// contiguous and conflict-free.
template <int V>
struct LrnwLds {
  static constexpr int NP = V / 4;
  typedef f32x4 vec_t;
  static constexpr int ROW = NP * LRNW_THREADS;  // vec_t per row buffer
  __device__ static __forceinline__ void put(vec_t* row, int t,
                                             const float* v) {
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) {
      f32x4 q;
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = v[4 * pl + j];
      row[pl * LRNW_THREADS + t] = q;
    }
  }
  __device__ static __forceinline__ void add(const vec_t* row, int t,
                                             float* acc) {
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) {
      const f32x4 q = row[pl * LRNW_THREADS + t];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[4 * pl + j] += q[j];
    }
  }
};
template <>
struct LrnwLds<1> {
  static constexpr int NP = 1;
  typedef float vec_t;
  static constexpr int ROW = LRNW_THREADS;
  __device__ static __forceinline__ void put(vec_t* row, int t,
                                             const float* v) {
    row[t] = v[0];
  }
  __device__ static __forceinline__ void add(const vec_t* row, int t,
                                             float* acc) {
    acc[0] += row[t];
  }
};

// What one lane is, decoded once from the block and lane index.
struct LrnwLane {
  int t, px, sp, nbr;  // lane, pixel slot, slots per segment, lanes per slot
  bool active;         // has a slot of a segment of an image
  bool col_ok;         // ... that is a pixel and a channel vector: may load
  bool out_ok;         // ... and is not a halo slot: emits
  int h0, h1, H;       // the strip [h0, h1)
  int64_t base;        // element offset of (n, row 0, w, first channel)
  int64_t row_stride;  // W * C

  __device__ LrnwLane(const LrnWithinPlan& p, int N, int C, int H_, int W) {
    unsigned b = blockIdx.x;
    const int cg = b % p.cgroups;
    b /= p.cgroups;
    const int colg = b % p.colgroups;
    b /= p.colgroups;
    const int st = b % p.strips;
    const int img = b / p.strips;
    t = threadIdx.x;
    sp = p.sp;
    nbr = p.cvb;
    const int cvl = t % p.cvb, slot = t / p.cvb;
    px = slot % p.sp;
    const int seg = slot / p.sp;
    const int n = img * p.segs + seg;
    const int w = colg * p.pw + px - p.halo;
    const int cvi = cg * p.cvb + cvl;
    active = seg < p.segs && n < N;
    col_ok = active && w >= 0 && w < W && cvi < p.cv;
    out_ok = col_ok && px >= p.halo && px < p.halo + p.pw;
    H = H_;
    h0 = st * p.strip;
    h1 = min(h0 + p.strip, H_);
    row_stride = (int64_t)W * C;
    base = col_ok ? ((int64_t)n * H_ * W + w) * C + (int64_t)cvi * p.V : 0;
  }
  // row h of this lane's column; zeros outside the image
  template <typename IO, typename T>
  __device__ __forceinline__ typename IO::raw_t load(const T* g, int h) const {
    typedef typename IO::raw_t raw_t;
    if (col_ok && (unsigned)h < (unsigned)H)
      return *(const raw_t*)(g + base + h * row_stride);
    return IO::zero();
  }
  template <typename IO, typename T>
  __device__ __forceinline__ void store(T* g, int h,
                                        const typename IO::raw_t& v) const {
    *(typename IO::raw_t*)(g + base + h * row_stride) = v;
  }
};

// out = own + the R slots each side of this lane's, read from the row
// buffer; slots past the segment's ends count as zero
template <int V, int R>
__device__ __forceinline__ void lrnw_hsum(
    const typename LrnwLds<V>::vec_t* row, const LrnwLane& L,
    const float* own, float* out) {
#pragma unroll
  for (int j = 0; j < V; ++j) out[j] = own[j];
#pragma unroll
  for (int d = 1; d <= R; ++d) {
    if (L.active && L.px - d >= 0) LrnwLds<V>::add(row, L.t - d * L.nbr, out);
    if (L.active && L.px + d < L.sp)
      LrnwLds<V>::add(row, L.t + d * L.nbr, out);
  }
}

// Vertical half of the box sum. acc[k] is the partial window sum of the row
// k below the oldest unfinished one: a new row's horizontal sum joins all
// 2R + 1 of them, acc[0] is then complete (the row R behind the new one)
// and leaves, the rest move up.
template <int V, int R>
__device__ __forceinline__ void lrnw_ring(float (&acc)[2 * R + 1][V],
                                          const float* h, float* done) {
#pragma unroll
  for (int j = 0; j < V; ++j) {
    done[j] = acc[0][j] + h[j];
#pragma unroll
    for (int k = 0; k < 2 * R; ++k) acc[k][j] = acc[k + 1][j] + h[j];
    acc[2 * R][j] = 0.f;
  }
}

// Forward. Front row f runs from R above the strip to R below it; row
// f - R is emitted once f >= h0 + R. One barrier per row: the row buffer is
// double-buffered, so a wave may write row f + 1 while others still read
// row f, and nobody reaches row f + 2 before all have passed barrier f + 1.
template <typename T, int V, int R>
__global__ void __launch_bounds__(LRNW_THREADS)
lrnw_fwd_k(const T* __restrict__ x, T* __restrict__ y, const LrnWithinPlan p,
           int N, int C, int H, int W, float a, float beta) {
  typedef LrnwIO<T, V> IO;
  typedef typename IO::raw_t raw_t;
  typedef LrnwLds<V> Lds;
  __shared__ typename Lds::vec_t lds[2 * Lds::ROW];
  const LrnwLane L(p, N, C, H, W);
  float acc[2 * R + 1][V] = {};
  raw_t xd[R + 1];  // x of rows f .. f - R, as loaded
#pragma unroll
  for (int k = 0; k <= R; ++k) xd[k] = IO::zero();
  raw_t nxt = L.template load<IO>(x, L.h0 - R);
  int buf = 0;
  for (int f = L.h0 - R; f < L.h1 + R; ++f, buf ^= 1) {
#pragma unroll
    for (int k = R; k > 0; --k) xd[k] = xd[k - 1];
    xd[0] = nxt;
    nxt = L.template load<IO>(x, f + 1);  // in flight across the barrier
    float xv[V], sq[V], hx[V], ss[V];
    IO::unpack(xd[0], xv);
#pragma unroll
    for (int j = 0; j < V; ++j) sq[j] = xv[j] * xv[j];
    typename Lds::vec_t* row = lds + buf * Lds::ROW;
    Lds::put(row, L.t, sq);
    __syncthreads();
    lrnw_hsum<V, R>(row, L, sq, hx);
    lrnw_ring<V, R>(acc, hx, ss);
    const int o = f - R;
    if (L.out_ok && o >= L.h0) {
      float out[V];
      IO::unpack(xd[R], xv);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float pw, inv;
        lrnw_pow(1.0f + a * ss[j], beta, pw, inv);
        out[j] = xv[j] * pw;
      }
      L.template store<IO>(y, o, IO::pack(out));
    }
  }
}

// Backward: two chained box filters in one walk. At front row f
//   - x(f)^2 and r(f - 1 - R), the latter computed in the previous trip, go
//     into their row buffers; one barrier serves both exchanges
//   - ring A completes s of row q = f - R, ring B the r-sum of row
//     p = f - 1 - 2R, which is emitted
//   - r(q) and t(q) = dy(q) * s(q)^-beta follow from s(q); t waits R + 1
//     trips in a register delay line for its row's r-sum
// x(q) comes out of a delay line of the loaded vectors; x(p) is read again
// (it was loaded 2R + 1 trips ago by this very lane: an L2 hit) rather than
// held for that long. The strip needs r of R rows each side and those need
// x of R more: f runs from 2R above the strip to 2R + 1 below it.
template <typename T, int V, int R>
__global__ void __launch_bounds__(LRNW_THREADS)
lrnw_bwd_k(const T* __restrict__ x, const T* __restrict__ dy,
           T* __restrict__ dx, const LrnWithinPlan p, int N, int C, int H,
           int W, float a, float c2, float beta) {
  typedef LrnwIO<T, V> IO;
  typedef typename IO::raw_t raw_t;
  typedef LrnwLds<V> Lds;
  __shared__ typename Lds::vec_t lds[4 * Lds::ROW];  // [x^2 | r] x 2
  const LrnwLane L(p, N, C, H, W);
  float accA[2 * R + 1][V] = {}, accB[2 * R + 1][V] = {};
  float td[R + 1][V] = {};  // t of rows q - 1 .. q - 1 - R
  float rq[V] = {};         // r of row q - 1
  raw_t xd[R + 1];          // x of rows f .. q, as loaded
#pragma unroll
  for (int k = 0; k <= R; ++k) xd[k] = IO::zero();
  const int f0 = L.h0 - 2 * R;
  raw_t nx = L.template load<IO>(x, f0);
  raw_t nd = L.template load<IO>(dy, f0 - R);
  raw_t np = L.template load<IO>(x, f0 - 1 - 2 * R);
  int buf = 0;
  for (int f = f0; f <= L.h1 + 2 * R; ++f, buf ^= 1) {
#pragma unroll
    for (int k = R; k > 0; --k) xd[k] = xd[k - 1];
    xd[0] = nx;
    const raw_t dq_raw = nd, xp_raw = np;
    nx = L.template load<IO>(x, f + 1);
    nd = L.template load<IO>(dy, f + 1 - R);
    np = L.template load<IO>(x, f - 2 * R);
    float xv[V], sq[V], hx[V], hr[V], ss[V], rs[V];
    IO::unpack(xd[0], xv);
#pragma unroll
    for (int j = 0; j < V; ++j) sq[j] = xv[j] * xv[j];
    typename Lds::vec_t* rowA = lds + (2 * buf) * Lds::ROW;
    typename Lds::vec_t* rowB = rowA + Lds::ROW;
    Lds::put(rowA, L.t, sq);
    Lds::put(rowB, L.t, rq);
    __syncthreads();
    lrnw_hsum<V, R>(rowA, L, sq, hx);
    lrnw_ring<V, R>(accA, hx, ss);
    lrnw_hsum<V, R>(rowB, L, rq, hr);
    lrnw_ring<V, R>(accB, hr, rs);
    const int o = f - 1 - 2 * R;
    if (L.out_ok && o >= L.h0) {
      float out[V];
      IO::unpack(xp_raw, xv);
#pragma unroll
      for (int j = 0; j < V; ++j) out[j] = td[R][j] - c2 * xv[j] * rs[j];
      L.template store<IO>(dx, o, IO::pack(out));
    }
    float dv[V];
    IO::unpack(xd[R], xv);
    IO::unpack(dq_raw, dv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float pw, inv;
      lrnw_pow(1.0f + a * ss[j], beta, pw, inv);
#pragma unroll
      for (int k = R; k > 0; --k) td[k][j] = td[k - 1][j];
      td[0][j] = dv[j] * pw;
      rq[j] = td[0][j] * xv[j] * inv;
    }
  }
}

std::atomic<int64_t> g_lrnw_launches{0};
std::atomic<int> g_lrnw_strip{0};  // 0 = the plan's own

template <typename T>
bool lrnw_aligned(const T* a, const T* b, const T* c) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

template <typename T, int V>
void lrnw_fwd_r(const LrnWithinPlan& p, int R, const T* x, T* y, int N, int C,
                int H, int W, float a, float beta, hipStream_t s) {
  const dim3 grid((unsigned)p.blocks);
  switch (R) {
    case 1: lrnw_fwd_k<T, V, 1><<<grid, LRNW_THREADS, 0, s>>>(x, y, p, N, C, H, W, a, beta); break;
    case 2: lrnw_fwd_k<T, V, 2><<<grid, LRNW_THREADS, 0, s>>>(x, y, p, N, C, H, W, a, beta); break;
    default: lrnw_fwd_k<T, V, 3><<<grid, LRNW_THREADS, 0, s>>>(x, y, p, N, C, H, W, a, beta); break;
  }
}

template <typename T, int V>
void lrnw_bwd_r(const LrnWithinPlan& p, int R, const T* x, const T* dy, T* dx,
                int N, int C, int H, int W, float a, float c2, float beta,
                hipStream_t s) {
  const dim3 grid((unsigned)p.blocks);
  switch (R) {
    case 1: lrnw_bwd_k<T, V, 1><<<grid, LRNW_THREADS, 0, s>>>(x, dy, dx, p, N, C, H, W, a, c2, beta); break;
    case 2: lrnw_bwd_k<T, V, 2><<<grid, LRNW_THREADS, 0, s>>>(x, dy, dx, p, N, C, H, W, a, c2, beta); break;
    default: lrnw_bwd_k<T, V, 3><<<grid, LRNW_THREADS, 0, s>>>(x, dy, dx, p, N, C, H, W, a, c2, beta); break;
  }
}

// dy == nullptr: forward into out; else backward into out
template <typename T>
void lrnw_launch(const T* x, const T* dy, T* out, int N, int C, int H, int W,
                 int size, float alpha, float beta, hipStream_t s) {
  if (!lrn_within_ok(C, size, (int)sizeof(T))) {
    fprintf(stderr, "lrn_within: unsupported C=%d size=%d\n", C, size);
    abort();
  }
  if ((int64_t)N * C * H * W == 0) return;
  const int R = (size - 1) / 2;
  const bool bwd = dy != nullptr;
  const LrnWithinPlan p =
      lrn_within_plan(N, C, H, W, (int)sizeof(T), R, bwd,
                      lrnw_aligned(x, bwd ? dy : x, out), g_lrnw_strip.load());
  if (p.blocks >= (int64_t)1 << 31) {
    fprintf(stderr, "lrn_within: grid of %lld blocks\n", (long long)p.blocks);
    abort();
  }
  constexpr int VN = 16 / (int)sizeof(T);
  const float a = alpha / (float)(size * size);
  const float c2 = 2.0f * alpha * beta / (float)(size * size);
  g_lrnw_launches.fetch_add(1, std::memory_order_relaxed);
  if (bwd) {
    if (p.V == 1) lrnw_bwd_r<T, 1>(p, R, x, dy, out, N, C, H, W, a, c2, beta, s);
    else lrnw_bwd_r<T, VN>(p, R, x, dy, out, N, C, H, W, a, c2, beta, s);
  } else {
    if (p.V == 1) lrnw_fwd_r<T, 1>(p, R, x, out, N, C, H, W, a, beta, s);
    else lrnw_fwd_r<T, VN>(p, R, x, out, N, C, H, W, a, beta, s);
  }
}

}  // namespace

extern "C" {

int ps_lrn_within_ok(int C, int size, int itemsize) {
  return lrn_within_ok(C, size, itemsize) ? 1 : 0;
}

void ps_lrn_within_fwd_f32(const float* x, float* y, int N, int C, int H,
                           int W, int size, float alpha, float beta,
                           hipStream_t s) {
  lrnw_launch<float>(x, nullptr, y, N, C, H, W, size, alpha, beta, s);
}
void ps_lrn_within_fwd_bf16(const void* x, void* y, int N, int C, int H,
                            int W, int size, float alpha, float beta,
                            hipStream_t s) {
  lrnw_launch<__bf16>((const __bf16*)x, nullptr, (__bf16*)y, N, C, H, W, size,
                      alpha, beta, s);
}
void ps_lrn_within_bwd_f32(const float* x, const float* dy, float* dx, int N,
                           int C, int H, int W, int size, float alpha,
                           float beta, hipStream_t s) {
  lrnw_launch<float>(x, dy, dx, N, C, H, W, size, alpha, beta, s);
}
void ps_lrn_within_bwd_bf16(const void* x, const void* dy, void* dx, int N,
                            int C, int H, int W, int size, float alpha,
                            float beta, hipStream_t s) {
  lrnw_launch<__bf16>((const __bf16*)x, (const __bf16*)dy, (__bf16*)dx, N, C,
                      H, W, size, alpha, beta, s);
}

void ps_lrn_within_set_strip(int n) { g_lrnw_strip = n > 0 ? n : 0; }

int64_t ps_lrn_within_launches(int reset) {
  return reset ? g_lrnw_launches.exchange(0) : g_lrnw_launches.load();
}

}  // extern "C"

}  // namespace ps

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
