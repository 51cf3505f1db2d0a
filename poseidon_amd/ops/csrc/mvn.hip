// MVN (mean-variance normalisation) on channels-last tensors, forward and
// backward, fp32 or bf16 in and out, all arithmetic in fp32:
//
//   mean = E[x],  var = E[(x - mean)^2],  rstd = 1 / sqrt(var + eps)
//   y    = (x - mean) * rstd                      (normalize_variance)
//   y    = x - mean,  rstd = 1                    (otherwise)
//   dx   = (dy - E[dy] - y * E[dy * y]) * rstd    (the y term only with
//                                                  normalize_variance)
//
// over one of two reduction sets: each (image, channel) over its pixels, or
// each image over all its elements. The variance always comes from centred
// values -- a second sweep over data the group still holds, or per-chunk
// (mean, M2) pairs merged with Chan's formula -- never from E[x^2] - mean^2,
// which cancels to nothing (or below zero) once |mean| >> std.
//
// ps_mvn_plan.h lays both geometries out the same way: a group of lanes
// (slot, channel vector) reduces one slab, a lane owns the items of its
// slot. So one set of kernels serves both; ROWS only says whether a lane's V
// elements belong to one statistic (across) or to V of them (per channel).
//
// Regimes:
//   wave  a group is a wave, a lane's items stay in registers, slots combine
//         by cross-lane exchange alone; four slabs share a block
//   lds   a group is a block, a lane parks its items (raw 16-byte vectors)
//         in LDS and reads back only its own, so the staging needs no
//         barrier; slots combine by cross-lane exchange, waves through LDS
//   split S blocks per slab run the lds kernel on a chunk each and write
//         partials, (mean, M2) forward and (sum dy, sum dy*y) backward; a
//         second launch merges the S partials of its sets in a fixed order
//         and streams its chunk again. No atomics and no finishing block:
//         every result is a fixed tree of additions, the same every run.
//
// The backward recomputes y from x and the forward's (mean, rstd).

#include <atomic>

#include "ps_common.h"
#include "ps_mvn_plan.h"

namespace ps {
namespace {

constexpr int MVN_WAVES = MVN_THREADS / kWave;
// cross-wave exchange: per wave, cvb lanes x values per lane <= 128 floats
// (V = 8: 8 lanes x 16, V = 4: 8 x 8, V = 1: 64 x 2)
constexpr int MVN_RED = MVN_WAVES * 128;

// Global I/O of one lane's item: one 16-byte access or one element.
template <typename T, int V>
struct MvnIO {
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

// What one lane is: lane l of group g, a group being G lanes.
template <int V, bool ROWS, int G>
struct MvnLane {
  int64_t base;    // element offset of its first item
  int64_t stride;  // elements from one of its items to the next
  int64_t set;     // its first (per channel: of V) statistic
  int cnt;         // items it owns
  int len;         // items of the group's chunk
  int s;           // which chunk of the slab
  int cvb, cvl;    // lanes per slot, this lane's place among them
  bool active;     // has channels
  bool owner;      // ... and slot 0: writes its sets' results
  __device__ MvnLane(const MvnPlan& p, int64_t g, int l) {
    const int64_t slab = g / p.split;
    s = (int)(g - slab * p.split);
    const int cg = (int)(slab % p.cgroups);
    const int64_t n = slab / p.cgroups;
    cvb = p.cvb;
    cvl = l % cvb;
    const int slot = l / cvb, slots = G / cvb;
    const int cvi = cg * cvb + cvl;
    const int i0 = s * p.chunk;
    len = min(p.chunk, p.items - i0);
    active = cvi < p.cv;
    owner = active && slot == 0;
    cnt = (active && slot < len) ? (len - slot + slots - 1) / slots : 0;
    base = (n * p.items + i0 + slot) * p.C + (int64_t)cvi * V;
    stride = (int64_t)slots * p.C;
    set = ROWS ? n : n * p.C + (int64_t)cvi * V;
  }
};

// Where a lane keeps LAYERS raw vectors per item between sweeps: registers
// (wave regime; every index is a compile-time constant once MVN_EACH is
// unrolled) or its own column of the block's dynamic LDS.
template <typename raw_t, bool WAVE, int LAYERS>
struct MvnHold {
  raw_t r[LAYERS][MVN_WAVE_ITEMS];
  __device__ explicit MvnHold(void*, int) {}
  __device__ __forceinline__ void put(int layer, int k, const raw_t& v) {
    r[layer][k] = v;
  }
  __device__ __forceinline__ raw_t get(int layer, int k) const {
    return r[layer][k];
  }
};
template <typename raw_t, int LAYERS>
struct MvnHold<raw_t, false, LAYERS> {
  raw_t* col;
  __device__ MvnHold(void* smem, int t) : col((raw_t*)smem + t) {}
  __device__ __forceinline__ void put(int layer, int k, const raw_t& v) {
    col[(k * LAYERS + layer) * MVN_THREADS] = v;
  }
  __device__ __forceinline__ raw_t get(int layer, int k) const {
    return col[(k * LAYERS + layer) * MVN_THREADS];
  }
};

// the items of a lane: a fully unrolled, guarded loop in the wave regime
#define MVN_EACH(k, cnt)                                                  \
  _Pragma("unroll") for (int k = 0; k < (WAVE ? MVN_WAVE_ITEMS : (cnt)); \
                         ++k) if (k < (cnt))

// ROWS: a lane's V partial sums are one statistic's
template <int V, bool ROWS>
__device__ __forceinline__ void mvn_fold(float* v) {
  if (ROWS) {
#pragma unroll
    for (int j = 1; j < V; ++j) v[0] += v[j];
  }
}

// Sum v[0 .. NVAL) over the lanes of the group that share this lane's place
// among the cvb: a butterfly over lane distances cvb .. 32, then (block
// groups) the waves' results through LDS, added in wave order. Every lane of
// the group calls it and every lane gets the same bits.
template <int NVAL, bool WAVE>
__device__ __forceinline__ void mvn_reduce(float* v, int cvb, float* red) {
  for (int off = cvb; off < kWave; off <<= 1) {
#pragma unroll
    for (int j = 0; j < NVAL; ++j) v[j] += __shfl_xor(v[j], off, kWave);
  }
  if (!WAVE) {
    const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if (lane < cvb) {
#pragma unroll
      for (int j = 0; j < NVAL; ++j) red[(w * cvb + lane) * NVAL + j] = v[j];
    }
    __syncthreads();
    const int cvl = lane % cvb;
#pragma unroll
    for (int j = 0; j < NVAL; ++j) {
      float a = red[cvl * NVAL + j];
#pragma unroll
      for (int ww = 1; ww < MVN_WAVES; ++ww)
        a += red[(ww * cvb + cvl) * NVAL + j];
      v[j] = a;
    }
    __syncthreads();  // red is free again
  }
}

// Forward of one group's chunk: load and hold, sum -> mean, centred sweep ->
// M2, then either normalise and write (y, stats) or, with part, leave the
// chunk's (mean, M2) for mvn_apply_k.
template <typename T, int V, bool ROWS, bool WAVE>
__global__ void __launch_bounds__(MVN_THREADS)
mvn_fwd_k(const T* __restrict__ x, T* __restrict__ y,
          float* __restrict__ stats, float* __restrict__ part,
          const MvnPlan p, float eps, int nv) {
  typedef MvnIO<T, V> IO;
  typedef typename IO::raw_t raw_t;
  constexpr int NS = ROWS ? 1 : V;
  extern __shared__ __attribute__((aligned(16))) unsigned char mvn_smem[];
  __shared__ float red[WAVE ? 1 : MVN_RED];
  const int t = threadIdx.x;
  const int64_t g =
      WAVE ? (int64_t)blockIdx.x * MVN_WAVES + t / kWave : blockIdx.x;
  if (WAVE && g >= p.groups) return;  // a whole wave; no barrier follows
  const MvnLane<V, ROWS, WAVE ? kWave : MVN_THREADS> L(p, g,
                                                       WAVE ? t % kWave : t);
  MvnHold<raw_t, WAVE, 1> h(mvn_smem, t);
  const float n = (float)L.len * (ROWS ? V : 1);
  float acc[V] = {}, mean[NS], m2[NS] = {}, rstd[NS];
  MVN_EACH(k, L.cnt) {
    const raw_t r = *(const raw_t*)(x + L.base + k * L.stride);
    h.put(0, k, r);
    float v[V];
    IO::unpack(r, v);
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] += v[j];
  }
  mvn_fold<V, ROWS>(acc);
  mvn_reduce<NS, WAVE>(acc, L.cvb, red);
#pragma unroll
  for (int j = 0; j < NS; ++j) mean[j] = acc[j] / n;
  if (nv) {
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    MVN_EACH(k, L.cnt) {
      float v[V];
      IO::unpack(h.get(0, k), v);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d = v[j] - mean[ROWS ? 0 : j];
        acc[j] += d * d;
      }
    }
    mvn_fold<V, ROWS>(acc);
    mvn_reduce<NS, WAVE>(acc, L.cvb, red);
#pragma unroll
    for (int j = 0; j < NS; ++j) m2[j] = acc[j];
  }
  if (part != nullptr) {
    if (L.owner) {
      float* o = part + ((int64_t)L.s * p.sets + L.set) * 2;
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        o[2 * j] = mean[j];
        o[2 * j + 1] = m2[j];
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NS; ++j)
    rstd[j] = nv ? 1.0f / sqrtf(m2[j] / n + eps) : 1.0f;
  MVN_EACH(k, L.cnt) {
    float v[V];
    IO::unpack(h.get(0, k), v);
#pragma unroll
    for (int j = 0; j < V; ++j)
      v[j] = (v[j] - mean[ROWS ? 0 : j]) * rstd[ROWS ? 0 : j];
    *(raw_t*)(y + L.base + k * L.stride) = IO::pack(v);
  }
  if (L.owner) {
    float* o = stats + L.set * 2;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      o[2 * j] = mean[j];
      o[2 * j + 1] = rstd[j];
    }
  }
}

// Backward of one group's chunk: one sweep loads and holds x and dy and sums
// dy and dy * y, then either dx is written or, with part, the two sums are
// left for mvn_apply_k. Without normalize_variance x is not read at all.
template <typename T, int V, bool ROWS, bool WAVE>
__global__ void __launch_bounds__(MVN_THREADS)
mvn_bwd_k(const T* __restrict__ x, const T* __restrict__ dy,
          T* __restrict__ dx, const float* __restrict__ stats,
          float* __restrict__ part, const MvnPlan p, int nv) {
  typedef MvnIO<T, V> IO;
  typedef typename IO::raw_t raw_t;
  constexpr int NS = ROWS ? 1 : V;
  extern __shared__ __attribute__((aligned(16))) unsigned char mvn_smem[];
  __shared__ float red[WAVE ? 1 : MVN_RED];
  const int t = threadIdx.x;
  const int64_t g =
      WAVE ? (int64_t)blockIdx.x * MVN_WAVES + t / kWave : blockIdx.x;
  if (WAVE && g >= p.groups) return;
  const MvnLane<V, ROWS, WAVE ? kWave : MVN_THREADS> L(p, g,
                                                       WAVE ? t % kWave : t);
  MvnHold<raw_t, WAVE, 2> h(mvn_smem, t);
  const float n = (float)L.len * (ROWS ? V : 1);
  float mean[NS], rstd[NS], a[V] = {}, b[V] = {};
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    mean[j] = L.active ? stats[(L.set + j) * 2] : 0.f;
    rstd[j] = L.active ? stats[(L.set + j) * 2 + 1] : 0.f;
  }
  MVN_EACH(k, L.cnt) {
    const raw_t rd = *(const raw_t*)(dy + L.base + k * L.stride);
    const raw_t rx =
        nv ? *(const raw_t*)(x + L.base + k * L.stride) : IO::zero();
    h.put(0, k, rx);
    h.put(1, k, rd);
    float xv[V], dv[V];
    IO::unpack(rx, xv);
    IO::unpack(rd, dv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      a[j] += dv[j];
      b[j] += dv[j] * ((xv[j] - mean[ROWS ? 0 : j]) * rstd[ROWS ? 0 : j]);
    }
  }
  mvn_fold<V, ROWS>(a);
  mvn_fold<V, ROWS>(b);
  float ab[2 * NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    ab[j] = a[j];
    ab[NS + j] = b[j];
  }
  mvn_reduce<2 * NS, WAVE>(ab, L.cvb, red);
  if (part != nullptr) {
    if (L.owner) {
      float* o = part + ((int64_t)L.s * p.sets + L.set) * 2;
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        o[2 * j] = ab[j];
        o[2 * j + 1] = ab[NS + j];
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    ab[j] /= n;
    ab[NS + j] = nv ? ab[NS + j] / n : 0.f;
  }
  MVN_EACH(k, L.cnt) {
    float xv[V], dv[V];
    IO::unpack(h.get(0, k), xv);
    IO::unpack(h.get(1, k), dv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int q = ROWS ? 0 : j;
      const float yh = (xv[j] - mean[q]) * rstd[q];
      dv[j] = (dv[j] - ab[q] - yh * ab[NS + q]) * rstd[q];
    }
    *(raw_t*)(dx + L.base + k * L.stride) = IO::pack(dv);
  }
}

// Second launch of the split regime, same grid and chunks as the first. The
// block's first lanes each merge the S partials of one of its sets -- Chan's
// pairwise update forward, plain sums backward, chunk 0 first -- and hand
// the result round through LDS; then every lane streams its items once
// more. Chunk 0's block also writes the forward's stats.
template <typename T, int V, bool ROWS, bool BWD>
__global__ void __launch_bounds__(MVN_THREADS)
mvn_apply_k(const T* __restrict__ x, const T* __restrict__ dy,
            T* __restrict__ out, float* __restrict__ stats,
            const float* __restrict__ part, const MvnPlan p, float eps,
            int nv) {
  typedef MvnIO<T, V> IO;
  typedef typename IO::raw_t raw_t;
  constexpr int NS = ROWS ? 1 : V;
  __shared__ float st[2][kWave];
  const int t = threadIdx.x;
  const MvnLane<V, ROWS, MVN_THREADS> L(p, blockIdx.x, t);
  const int64_t slab = blockIdx.x / p.split;
  const int c = ROWS ? 0 : (int)(slab % p.cgroups) * p.cvb * V + t;
  if (t < (ROWS ? 1 : p.cvb * V) && c < p.C) {
    const int64_t set = ROWS ? slab : (slab / p.cgroups) * p.C + c;
    const float per = ROWS ? V : 1;
    const float* q = part + set * 2;
    if (!BWD) {
      float na = 0.f, mean = 0.f, m2 = 0.f;
      for (int s = 0; s < p.split; ++s, q += p.sets * 2) {
        const float nb = (float)min(p.chunk, p.items - s * p.chunk) * per;
        const float nt = na + nb, delta = q[0] - mean;
        mean += delta * (nb / nt);
        m2 += q[1] + delta * delta * (na * nb / nt);
        na = nt;
      }
      const float rstd = nv ? 1.0f / sqrtf(m2 / na + eps) : 1.0f;
      st[0][t] = mean;
      st[1][t] = rstd;
      if (L.s == 0) {
        stats[set * 2] = mean;
        stats[set * 2 + 1] = rstd;
      }
    } else {
      float a = 0.f, b = 0.f;
      for (int s = 0; s < p.split; ++s, q += p.sets * 2) {
        a += q[0];
        b += q[1];
      }
      const float n = (float)p.items * per;
      st[0][t] = a / n;
      st[1][t] = nv ? b / n : 0.f;
    }
  }
  __syncthreads();
  float m0[NS], m1[NS], mean[NS], rstd[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    m0[j] = st[0][ROWS ? 0 : L.cvl * V + j];
    m1[j] = st[1][ROWS ? 0 : L.cvl * V + j];
    mean[j] = (BWD && L.active) ? stats[(L.set + j) * 2] : 0.f;
    rstd[j] = (BWD && L.active) ? stats[(L.set + j) * 2 + 1] : 0.f;
  }
#pragma unroll 4
  for (int k = 0; k < L.cnt; ++k) {
    const int64_t at = L.base + k * L.stride;
    float xv[V], dv[V];
    IO::unpack((!BWD || nv) ? *(const raw_t*)(x + at) : IO::zero(), xv);
    if (BWD) IO::unpack(*(const raw_t*)(dy + at), dv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int q = ROWS ? 0 : j;
      if (BWD) {
        const float yh = (xv[j] - mean[q]) * rstd[q];
        xv[j] = (dv[j] - m0[q] - yh * m1[q]) * rstd[q];
      } else {
        xv[j] = (xv[j] - m0[q]) * m1[q];
      }
    }
    *(raw_t*)(out + at) = IO::pack(xv);
  }
}

std::atomic<int64_t> g_mvn_launches{0};
std::atomic<int> g_mvn_split{0};  // 0 = the plan's own

template <typename T, int V, bool ROWS>
void mvn_run(const MvnPlan& p, const T* x, const T* dy, T* out, float* stats,
             float* ws, int nv, hipStream_t s) {
  const float eps = 1e-10f;
  const dim3 grid((unsigned)p.blocks);
  const bool bwd = dy != nullptr;
  if (p.regime == MVN_WAVE) {
    if (bwd) {
      mvn_bwd_k<T, V, ROWS, true><<<grid, MVN_THREADS, 0, s>>>(x, dy, out, stats, nullptr, p, nv);
    } else {
      mvn_fwd_k<T, V, ROWS, true><<<grid, MVN_THREADS, 0, s>>>(x, out, stats, nullptr, p, eps, nv);
    }
    g_mvn_launches.fetch_add(1, std::memory_order_relaxed);
    return;
  }
  float* part = p.split > 1 ? ws : nullptr;
  if (bwd) {
    mvn_bwd_k<T, V, ROWS, false><<<grid, MVN_THREADS, p.lds, s>>>(x, dy, out, stats, part, p, nv);
  } else {
    mvn_fwd_k<T, V, ROWS, false><<<grid, MVN_THREADS, p.lds, s>>>(x, out, stats, part, p, eps, nv);
  }
  g_mvn_launches.fetch_add(1, std::memory_order_relaxed);
  if (part == nullptr) return;
  if (bwd) {
    mvn_apply_k<T, V, ROWS, true><<<grid, MVN_THREADS, 0, s>>>(x, dy, out, stats, part, p, eps, nv);
  } else {
    mvn_apply_k<T, V, ROWS, false><<<grid, MVN_THREADS, 0, s>>>(x, nullptr, out, stats, part, p, eps, nv);
  }
  g_mvn_launches.fetch_add(1, std::memory_order_relaxed);
}

// dy == nullptr: forward (x -> out, stats written); else backward (stats
// read). ws: mvn_ws_floats() floats, needed only by a split plan.
template <typename T>
void mvn_launch(const T* x, const T* dy, T* out, float* stats, float* ws,
                int64_t N, int64_t C, int64_t P, int across, int nv, int vec,
                hipStream_t s) {
  if (!mvn_ok(N, C, P, (int)sizeof(T))) {
    fprintf(stderr, "mvn: unsupported N=%lld C=%lld P=%lld\n", (long long)N,
            (long long)C, (long long)P);
    abort();
  }
  if (N == 0) return;
  const MvnPlan p = mvn_plan(N, (int)C, P, (int)sizeof(T), across != 0,
                             dy != nullptr, vec != 0, g_mvn_split.load());
  if (p.blocks >= (int64_t)1 << 31 || p.lds > (size_t)MVN_LDS_BYTES ||
      (p.regime == MVN_WAVE && p.per_lane > MVN_WAVE_ITEMS) ||
      (p.split > 1 && ws == nullptr)) {
    fprintf(stderr, "mvn: bad plan (%lld blocks, %zu B of LDS, split %d)\n",
            (long long)p.blocks, p.lds, p.split);
    abort();
  }
  constexpr int VN = 16 / (int)sizeof(T);
  if (p.rows) {
    if (p.V == 1) mvn_run<T, 1, true>(p, x, dy, out, stats, ws, nv, s);
    else mvn_run<T, VN, true>(p, x, dy, out, stats, ws, nv, s);
  } else {
    if (p.V == 1) mvn_run<T, 1, false>(p, x, dy, out, stats, ws, nv, s);
    else mvn_run<T, VN, false>(p, x, dy, out, stats, ws, nv, s);
  }
}

}  // namespace

extern "C" {

int64_t ps_mvn_ws_floats(int64_t N, int64_t C, int64_t P, int itemsize,
                         int across, int backward, int vec) {
  if (!mvn_ok(N, C, P, itemsize) || N == 0) return 0;
  return mvn_ws_floats(mvn_plan(N, (int)C, P, itemsize, across != 0,
                                backward != 0, vec != 0, g_mvn_split.load()));
}

void ps_mvn_fwd_f32(const float* x, float* y, float* stats, float* ws,
                    int64_t N, int64_t C, int64_t P, int across, int norm_var,
                    int vec, hipStream_t s) {
  mvn_launch<float>(x, nullptr, y, stats, ws, N, C, P, across, norm_var, vec,
                    s);
}
void ps_mvn_fwd_bf16(const void* x, void* y, float* stats, float* ws,
                     int64_t N, int64_t C, int64_t P, int across, int norm_var,
                     int vec, hipStream_t s) {
  mvn_launch<__bf16>((const __bf16*)x, nullptr, (__bf16*)y, stats, ws, N, C, P,
                     across, norm_var, vec, s);
}
void ps_mvn_bwd_f32(const float* x, const float* dy, float* dx, float* stats,
                    float* ws, int64_t N, int64_t C, int64_t P, int across,
                    int norm_var, int vec, hipStream_t s) {
  mvn_launch<float>(x, dy, dx, stats, ws, N, C, P, across, norm_var, vec, s);
}
void ps_mvn_bwd_bf16(const void* x, const void* dy, void* dx, float* stats,
                     float* ws, int64_t N, int64_t C, int64_t P, int across,
                     int norm_var, int vec, hipStream_t s) {
  mvn_launch<__bf16>((const __bf16*)x, (const __bf16*)dy, (__bf16*)dx, stats,
                     ws, N, C, P, across, norm_var, vec, s);
}

void ps_mvn_set_split(int n) { g_mvn_split = n > 0 ? n : 0; }

int64_t ps_mvn_launches(int reset) {
  return reset ? g_mvn_launches.exchange(0) : g_mvn_launches.load();
}

}  // extern "C"

}  // namespace ps
