// Row-fused first-layer convolution for gfx950: forward and weight gradient of
// a small-channel bf16 conv (G == 1, C % 8 != 0) straight from staged input
// rows. The column matrix im2col_rowstage_k writes -- 7.5x the input for
// AlexNet conv1, written once and read twice per step -- never exists: both
// kernels stage a tile's input window in LDS as that kernel does, and build
// their MFMA operands from it with 2-byte LDS reads.
//
// Tile walk, staged addressing and LDS layout: ps_rowfused.h (checked on the
// host by tests/rowfused_plan_host.cpp). Both kernels are persistent -- about
// one 512-thread block per CU, each walking a run of consecutive tiles -- and
// split their waves by role: waves 4-7 stage tile i + 1 (x through its
// element strides, any layout; dy for the wgrad) into one LDS buffer while
// waves 0-3 run the MFMAs of tile i from the other; one barrier per tile.
//
// A dead position (past the tile's live count) or a pad column k >= Kcol
// reads the zero header of the staged image (ps_rf_addr), so its operand
// element is an exact zero whatever the staged rows hold.
//
// Forward: the whole khwc weight shadow wk [Co][Kpad] sits in LDS for the
//   launch. A wave owns 32 positions x all Co columns; its A fragments are 8
//   consecutive k of one position, gathered through a k -> staged-offset
//   table. v_mfma_f32_16x16x32_bf16 with GemmTraits<__bf16>::load_frag's
//   k -> (k-step, lane group, element) map, k-steps ascending from a zero
//   accumulator, gemm_epilogue's arithmetic: bit-identical to the
//   materialized im2col + gemm_kernel path.
// Wgrad: dwk[co][k] += sum_p dy[p][co] * col[p][k]. A wave owns KF 16-column
//   k fragments x all Co rows and keeps them in registers across all tiles of
//   its block; the col operand of a lane is 8 consecutive positions at one k,
//   the dy operand comes from the LDS dy tile through ds_read_b64_tr_b16 (as
//   gemm_tn_tr_kernel reads its A image). One atomicAdd flush per block.

#include "ps_common.h"
#include "ps_api.h"
#include "ps_rowfused.h"

#include <atomic>
#include <mutex>

namespace ps {
namespace {

constexpr int RF_THREADS = PS_RF_THREADS;
constexpr int RF_STAGERS = 256;  // the forward's waves 4-7

typedef __attribute__((ext_vector_type(4))) __bf16 rf_bf16x4;
typedef __attribute__((ext_vector_type(4))) int rf_i32x4;

// x: its first element and how to walk it (strides in elements, span)
struct RfX {
  const __bf16* x;
  RowFusedX g;
};

// one staged bf16 at byte offset pbase + koff of the image (zero header for
// a dead position / pad column)
__device__ inline __bf16 rf_read(const char* img, int pbase, int koff) {
  return *reinterpret_cast<const __bf16*>(img + max(pbase + koff, 0));
}

// A tile's input window, global -> registers -> LDS, in two halves so that a
// caller can leave the loads in flight across other work. The image is
// channel-planar (ps_rowfused.h): its 16 B vector idx is 8 pixels of one
// channel of one staged row. ps_rf_vec decides per vector: nothing to load
// (ZERO), ONE 2-byte-aligned 16 B load that may run over a row end into the
// neighbouring row of the same tensor (WIDE), or 8 two-byte loads from
// pixels clamped into the row (NARROW: the ends of x's span, layouts with
// sw != 1). rf_load_x only issues loads -- no loaded value is used, so no
// wait stands between them; rf_store_x packs the NARROW elements, zeroes
// what lies outside the row with a register mask and writes the vector.
// Thread tid of NT holds vectors tid, tid + NT, ... (NV of them).
typedef unsigned rf_u32x4a2 __attribute__((ext_vector_type(4), aligned(2)));
typedef unsigned rf_u32x4 __attribute__((ext_vector_type(4)));

// a vector in flight. WIDE: the 16 B in w; NARROW: element j, zero-extended,
// in e[j]. The two kinds keep registers of their own, so that neither load
// has to be merged with the other's result before the store.
// m = kind | lo << 2 | hi << 6
struct RfRaw {
  unsigned w[4];
  unsigned e[8];
  int m;
};

// the tile-invariant half of the decision (ps_rf_vec_pos), packed:
// sc = sr << 16 | col, negative past the window
struct RfPos {
  int rel, sc;
};

template <int NV, int NT>
__device__ inline void rf_positions(RfPos (&pos)[NV], const RowFusedTiling& t,
                                    const RfX& X, int tid, int first) {
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const RowFusedVecPos p = ps_rf_vec_pos(t, X.g, first + tid + v * NT);
    pos[v].rel = p.rel;
    pos[v].sc = p.live ? p.sr << 16 | p.col : -1;
  }
}

template <int NV>
__device__ inline void rf_load_x(RfRaw (&xr)[NV], const RfPos (&pos)[NV],
                                 const RowFusedTiling& t,
                                 const RowFusedTile& tl, const RfX& X) {
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const RowFusedVecPos p = {pos[v].sc >> 16, pos[v].sc & 0xffff, pos[v].rel,
                              pos[v].sc >= 0};
    const RowFusedVec d = ps_rf_vec_at(t, tl, X.g, p);
    xr[v].m = d.kind | d.lo << 2 | d.hi << 6;
#pragma unroll
    for (int j = 0; j < 4; ++j) xr[v].w[j] = 0u;
    // e is read only where the kind is NARROW; starting it from a value the
    // compiler cannot fold keeps the packing shifts out of the branch below
    // (and with them a wait per vector). This steers code generation and a
    // compiler update can undo it. What to look for in the ISA of
    // conv_rowfused_fwd_k<6>: the six slots of a chunk are
    // global_load_dwordx4, 8 x global_load_ushort, six times, with no
    // s_waitcnt vmcnt between them. If waits come back they sit inside the
    // NARROW branch: layouts with sw != 1 then stage one vector at a time;
    // the w-contiguous data blob, which hardly has NARROW vectors, loses
    // nothing
#pragma unroll
    for (int j = 0; j < 8; ++j) xr[v].e[j] = (unsigned)xr[v].m;
    if (d.kind == PS_RF_WIDE) {
      const rf_u32x4a2 w = *reinterpret_cast<const rf_u32x4a2*>(X.x + d.off);
#pragma unroll
      for (int j = 0; j < 4; ++j) xr[v].w[j] = w[j];
    }
    if (d.kind == PS_RF_NARROW) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        xr[v].e[j] = *reinterpret_cast<const unsigned short*>(
            X.x + ps_rf_narrow_off(t, d, X.g.sw, j));
    }
  }
}

template <int NV, int NT>
__device__ inline void rf_store_x(char* img, const RfRaw (&xr)[NV],
                                  const RowFusedTiling& t, int tid,
                                  int first) {
  const int total = t.srows * t.C * (t.rsw_ld / 8);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int idx = first + tid + v * NT;
    const int m = xr[v].m;
    const bool narrow = (m & 3) == PS_RF_NARROW;
    const unsigned em = ps_rf_elem_mask((m >> 2) & 15, m >> 6);
    rf_u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned w = narrow ? xr[v].e[2 * i] | xr[v].e[2 * i + 1] << 16
                                : xr[v].w[i];
      const unsigned keep = ((em >> (2 * i) & 1u) ? 0x0000ffffu : 0u) |
                            ((em >> (2 * i + 1) & 1u) ? 0xffff0000u : 0u);
      o[i] = w & keep;
    }
    if (idx < total)
      *reinterpret_cast<rf_u32x4*>(img + PS_RF_HDR + idx * 16) = o;
  }
}

// the forward's waves 4-7 stage a whole window, RF_FV vectors per thread in
// flight at a time. ptid: 0..RF_STAGERS-1
constexpr int RF_FV = 6;
__device__ inline void rf_stage_x(char* img, const RowFusedTiling& t,
                                  const RowFusedTile& tl, const RfX& X,
                                  int ptid) {
  const int total = t.srows * t.C * (t.rsw_ld / 8);
  for (int first = 0; first < total; first += RF_FV * RF_STAGERS) {
    RfPos pos[RF_FV];
    RfRaw xr[RF_FV];
    rf_positions<RF_FV, RF_STAGERS>(pos, t, X, ptid, first);
    rf_load_x<RF_FV>(xr, pos, t, tl, X);
    rf_store_x<RF_FV, RF_STAGERS>(img, xr, t, ptid, first);
  }
}

__device__ inline void rf_zero_headers(char* xs0, int xs_bytes, int tid) {
  if (tid < 4) reinterpret_cast<int*>(xs0)[tid] = 0;
  else if (tid < 8) reinterpret_cast<int*>(xs0 + xs_bytes)[tid - 4] = 0;
}

template <int FN>
__global__ __launch_bounds__(RF_THREADS)
void conv_rowfused_fwd_k(RowFusedTiling t, RfX X,
                         const __bf16* __restrict__ wk,
                         const float* __restrict__ bias,
                         __bf16* __restrict__ y, int relu, float alpha,
                         int tpb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* wl = reinterpret_cast<__bf16*>(smem);
  int* kofft = reinterpret_cast<int*>(smem + t.fwd_koff_off);
  char* xs0 = smem + t.fwd_xs_off;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = lane & 15, q = lane >> 4;
  const int64_t t0 = (int64_t)blockIdx.x * tpb;
  const int64_t t1 = t0 + tpb < t.tiles ? t0 + tpb : t.tiles;
  if (t0 >= t1) return;

  // weights: Cop rows of Kpad, rows past Co zero
  {
    const int vpr = t.Kpad / 8;
    for (int i = tid; i < t.Cop * vpr; i += RF_THREADS) {
      const int co = i / vpr;
      const int kv = (i - co * vpr) * 8;
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.0f;
      if (co < t.Co)
        v = *reinterpret_cast<const bf16x8*>(&wk[(int64_t)co * t.Kpad + kv]);
      *reinterpret_cast<bf16x8*>(&wl[co * t.w_ld + kv]) = v;
    }
    for (int k = tid; k < t.Kpad; k += RF_THREADS) kofft[k] = ps_rf_koff(t, k);
    rf_zero_headers(xs0, t.xs_bytes, tid);
  }
  if (wid >= 4)
    rf_stage_x(xs0, t, ps_rf_tile(t, t0), X, tid - RF_STAGERS);
  // the two fragments' positions and their staged bases: tile-invariant
  int pf[2], pbf[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    pf[f] = (wid & 3) * 32 + f * 16 + l;
    pbf[f] = ps_rf_pbase(t, pf[f]);
  }
  // the lane's bias values, once per launch and waited for here: a load
  // still pending when the tile loop is entered (or one inside the epilogue)
  // makes the compiler put a vmcnt(0) -- a drain of every store before it --
  // in front of each of the epilogue's conditional stores. The empty asm
  // below only forces that wait, and a compiler update can undo it. What to
  // look for in the ISA of conv_rowfused_fwd_k<6>: the epilogue's
  // global_store_short come 12 in a row with no s_waitcnt vmcnt between
  // them. If the waits come back, AlexNet's conv1 forward goes from about
  // 193 us back to about 324 us (profiles/first_layer_rowfused.md)
  float bvf[FN];
#pragma unroll
  for (int fn = 0; fn < FN; ++fn)
    bvf[fn] = bias && fn * 16 + l < t.Co ? bias[fn * 16 + l] : 0.0f;
#pragma unroll
  for (int fn = 0; fn < FN; ++fn) asm volatile("" : "+v"(bvf[fn]));
  __syncthreads();

  for (int64_t ti = t0; ti < t1; ++ti) {
    const int cur = (int)(ti - t0) & 1;
    if (wid >= 4) {
      if (ti + 1 < t1)
        rf_stage_x(xs0 + (cur ^ 1) * t.xs_bytes, t, ps_rf_tile(t, ti + 1), X,
                   tid - RF_STAGERS);
    } else {
      const RowFusedTile tl = ps_rf_tile(t, ti);
      if (wid * 32 < tl.nlive) {
        const char* img = xs0 + cur * t.xs_bytes;
        int pb[2];
#pragma unroll
        for (int f = 0; f < 2; ++f)
          pb[f] = pf[f] < tl.nlive ? pbf[f] : PS_RF_NEG;
        f32x4 acc[2][FN] = {};
        // one k-step per trip: table reads, 16 two-byte staged reads, then
        // the 12 MFMAs. Nothing of step s + 1 is issued under step s's MFMAs
        // (an unroll pragma here changed nothing: the compiler keeps the
        // steps apart), and with one computing wave per SIMD nothing else
        // hides the LDS latency -- the next thing to work on
        // (profiles/first_layer_rowfused.md)
        for (int ks = 0; ks < t.Kpad; ks += 32) {
          const rf_i32x4 k0 =
              *reinterpret_cast<const rf_i32x4*>(&kofft[ks + q * 8]);
          const rf_i32x4 k1 =
              *reinterpret_cast<const rf_i32x4*>(&kofft[ks + q * 8 + 4]);
          bf16x8 bfr[FN];
#pragma unroll
          for (int fn = 0; fn < FN; ++fn)
            bfr[fn] = *reinterpret_cast<const bf16x8*>(
                &wl[(fn * 16 + l) * t.w_ld + ks + q * 8]);
          bf16x8 af[2];
#pragma unroll
          for (int f = 0; f < 2; ++f) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              af[f][e] = rf_read(img, pb[f], k0[e]);
              af[f][4 + e] = rf_read(img, pb[f], k1[e]);
            }
          }
#pragma unroll
          for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int fn = 0; fn < FN; ++fn)
              acc[f][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  af[f], bfr[fn], acc[f][fn], 0, 0, 0);
        }
        // gemm_epilogue's arithmetic; C/D map: col = lane & 15,
        // row = (lane >> 4) * 4 + r
#pragma unroll
        for (int f = 0; f < 2; ++f) {
#pragma unroll
          for (int fn = 0; fn < FN; ++fn) {
            const int col = fn * 16 + l;
            if (col >= t.Co) continue;
            const float bv = bvf[fn];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int p = wid * 32 + f * 16 + q * 4 + r;
              if (p >= tl.nlive) continue;
              float v = alpha * acc[f][fn][r] + bv;
              if (relu && v < 0.0f) v = 0.0f;
              from_f32(v, y[(tl.pos0 + p) * t.Co + col]);
            }
          }
        }
      }
    }
    __syncthreads();
  }
}

// the two transpose-reads of one dy^T fragment, issued without waiting (the
// caller drains them with rf_tr_wait): lane l of a 16-lane group points at
// row kk + l/4 (+4), columns cb + 4*(l%4)..+3 of the [position][co] image and
// receives the 8-position run of column cb + l (gemm.hip, tr_frag)
__device__ inline bf16x8 rf_tr_frag(unsigned base, int kk, int cb, int l,
                                    int ld) {
  const unsigned a1 =
      base + (unsigned)(((kk + (l >> 2)) * ld + cb + 4 * (l & 3)) * 2);
  const unsigned a2 = a1 + (unsigned)(4 * ld * 2);
  rf_bf16x4 v1, v2;
  asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
               "ds_read_b64_tr_b16 %1, %3"
               : "=&v"(v1), "=&v"(v2) : "v"(a1), "v"(a2));
  bf16x8 f;
#pragma unroll
  for (int i = 0; i < 4; ++i) { f[i] = v1[i]; f[4 + i] = v2[i]; }
  return f;
}

template <int N>
__device__ inline void rf_tr_wait(bf16x8 (&a)[N]) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+v"(a[i]));
}

template <int FN, int KF>
__global__ __launch_bounds__(RF_THREADS)
void conv_rowfused_wgrad_k(RowFusedTiling t, RfX X,
                           const __bf16* __restrict__ dy,
                           float* __restrict__ dwk, int tpb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* ptab = reinterpret_cast<int*>(smem);  // [2][TM] staged bases
  __bf16* dyl0 = reinterpret_cast<__bf16*>(smem + t.wg_dy_off);
  char* xs0 = smem + t.wg_xs_off;
  const int dy_tile = PS_RF_TM * t.dy_ld;  // elements per dy buffer
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = lane & 15, q = lane >> 4;
  const int64_t t0 = (int64_t)blockIdx.x * tpb;
  const int64_t t1 = t0 + tpb < t.tiles ? t0 + tpb : t.tiles;
  if (t0 >= t1) return;
  rf_zero_headers(xs0, t.xs_bytes, tid);

  // a tile's x window, dy rows (dead rows and columns past Co zero) and its
  // positions' staged bases (dead ones -> the zero header): loaded into
  // registers ahead of the previous tile's MFMAs, stored to LDS after them
  const int my_pb = tid < PS_RF_TM ? ps_rf_pbase(t, tid) : 0;
  const int cv8 = t.Cop / 8;
  RfPos xpos[PS_RF_XV];
  rf_positions<PS_RF_XV, RF_THREADS>(xpos, t, X, tid, 0);
  // dy vector v of this thread: position and first column, tile-invariant
  int dyp[PS_RF_DV], dyc[PS_RF_DV];
#pragma unroll
  for (int v = 0; v < PS_RF_DV; ++v) {
    const int idx = tid + v * RF_THREADS;
    dyp[v] = idx / cv8;
    dyc[v] = (idx - dyp[v] * cv8) * 8;
  }
  RfRaw xr[PS_RF_XV];
  bf16x8 dv[PS_RF_DV];
  auto load = [&](int64_t ti) {
    const RowFusedTile tl = ps_rf_tile(t, ti);
    rf_load_x<PS_RF_XV>(xr, xpos, t, tl, X);
#pragma unroll
    for (int v = 0; v < PS_RF_DV; ++v) {
      const int p = dyp[v];
      const int cv = dyc[v];
#pragma unroll
      for (int j = 0; j < 8; ++j) dv[v][j] = (__bf16)0.0f;
      if (p < tl.nlive && cv < t.Co)
        dv[v] = *reinterpret_cast<const bf16x8*>(
            &dy[(tl.pos0 + p) * t.Co + cv]);
    }
  };
  auto store = [&](int buf, int64_t ti) {
    const RowFusedTile tl = ps_rf_tile(t, ti);
    rf_store_x<PS_RF_XV, RF_THREADS>(xs0 + buf * t.xs_bytes, xr, t, tid,
                                     0);
    __bf16* dyl = dyl0 + buf * dy_tile;
#pragma unroll
    for (int v = 0; v < PS_RF_DV; ++v) {
      const int p = dyp[v];
      const int cv = dyc[v];
      if (p < PS_RF_TM)
        *reinterpret_cast<bf16x8*>(&dyl[p * t.dy_ld + cv]) = dv[v];
    }
    if (tid < PS_RF_TM)
      ptab[buf * PS_RF_TM + tid] = tid < tl.nlive ? my_pb : PS_RF_NEG;
  };
  load(t0);
  store(0, t0);

  // this wave's k fragments: (by*KF + i)*8 + wave, 16 columns each; the
  // lane's column is B-operand row l
  const int by = blockIdx.y;
  int kofs[KF];
  bool klive[KF];
#pragma unroll
  for (int i = 0; i < KF; ++i) {
    const int kf = (by * KF + i) * 8 + wid;
    klive[i] = kf * 16 < t.Kpad;  // wave-uniform
    kofs[i] = klive[i] ? ps_rf_koff(t, kf * 16 + l) : PS_RF_NEG;
  }
  f32x4 acc[FN][KF] = {};
  __syncthreads();

  for (int64_t ti = t0; ti < t1; ++ti) {
    const int cur = (int)(ti - t0) & 1;
    if (ti + 1 < t1) load(ti + 1);
    {
      const RowFusedTile tl = ps_rf_tile(t, ti);
      const char* img = xs0 + cur * t.xs_bytes;
      const int* pt = ptab + cur * PS_RF_TM;
      const unsigned dyb = (unsigned)(unsigned long long)(
          __attribute__((address_space(3))) __bf16*)(dyl0 + cur * dy_tile);
      for (int p0 = 0; p0 < tl.nlive; p0 += 32) {
        const rf_i32x4 pa =
            *reinterpret_cast<const rf_i32x4*>(&pt[p0 + q * 8]);
        const rf_i32x4 pb =
            *reinterpret_cast<const rf_i32x4*>(&pt[p0 + q * 8 + 4]);
        bf16x8 af[FN];
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          af[fn] = rf_tr_frag(dyb, p0 + q * 8, fn * 16, l, t.dy_ld);
        rf_tr_wait(af);
#pragma unroll
        for (int i = 0; i < KF; ++i) {
          if (klive[i]) {
            bf16x8 bfr;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              bfr[e] = rf_read(img, pa[e], kofs[i]);
              bfr[4 + e] = rf_read(img, pb[e], kofs[i]);
            }
#pragma unroll
            for (int fn = 0; fn < FN; ++fn)
              acc[fn][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  af[fn], bfr, acc[fn][i], 0, 0, 0);
          }
        }
      }
    }
    if (ti + 1 < t1) store(cur ^ 1, ti + 1);
    __syncthreads();
  }
  // D map: col = lane & 15 is the k column, row = (lane >> 4)*4 + r the co.
  // Pad columns hold exact zeros and are left as they are.
#pragma unroll
  for (int fn = 0; fn < FN; ++fn)
#pragma unroll
    for (int i = 0; i < KF; ++i) {
      if (!klive[i]) continue;
      const int k = ((by * KF + i) * 8 + wid) * 16 + l;
      if (k >= t.Kcol) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = fn * 16 + q * 4 + r;
        if (co < t.Co)
          atomicAdd(&dwk[(int64_t)co * t.Kpad + k], acc[fn][i][r]);
      }
    }
}

// tests / tuning: cap on the persistent grid (0 = one block per CU)
std::atomic<int> g_rf_blocks{0};

// CU count and the kernels' LDS attribute, set up once by
// ps_rowfused_prepare (the bindings call it when a plan comes out row-fused,
// so ahead of any launch or capture)
std::atomic<int> g_rf_cus{0};
std::once_flag g_rf_once;

int rf_cu_count() {
  const int n = g_rf_cus.load();
  return n > 0 ? n : 256;
}

// grid.x and tiles per block: consecutive tiles per block
void rf_grid(const RowFusedTiling& t, int* blocks, int* tpb) {
  const int cap = g_rf_blocks.load();
  int64_t b = cap > 0 ? cap : rf_cu_count();
  if (b > t.tiles) b = t.tiles;
  *tpb = (int)((t.tiles + b - 1) / b);
  *blocks = (int)((t.tiles + *tpb - 1) / *tpb);
}

// dynamic LDS above 64 KB needs the attribute on each instantiation
template <typename K>
bool rf_allow_lds(K kernel) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             PS_RF_LDS_MAX) == hipSuccess;
}

template <int FN>
void rf_launch_fwd(const RowFusedTiling& t, const RfX& X, const void* wk,
                   const float* bias, void* y, int relu, hipStream_t s) {
  int blocks, tpb;
  rf_grid(t, &blocks, &tpb);
  conv_rowfused_fwd_k<FN><<<dim3((unsigned)blocks), RF_THREADS, t.fwd_lds,
                            s>>>(t, X, (const __bf16*)wk, bias, (__bf16*)y,
                                 relu, 1.0f, tpb);
}

template <int FN, int KF>
void rf_launch_wgrad(const RowFusedTiling& t, const RfX& X, const void* dy,
                     float* dwk, hipStream_t s) {
  int blocks, tpb;
  rf_grid(t, &blocks, &tpb);
  // a block covers 8 waves x KF fragments of 16 k columns
  const int gy = (t.Kpad / 16 + 8 * KF - 1) / (8 * KF);
  conv_rowfused_wgrad_k<FN, KF><<<dim3((unsigned)blocks, (unsigned)gy),
                                  RF_THREADS, t.wg_lds, s>>>(
      t, X, (const __bf16*)dy, dwk, tpb);
}

}  // namespace
}  // namespace ps

extern "C" {

void ps_rowfused_set_blocks(int n) { ps::g_rf_blocks.store(n < 0 ? 0 : n); }

// Once per process, at plan time: the device's CU count (the persistent
// grids' size) and the LDS attribute of every instantiation. Returns 0
// without a usable device; the launchers must not be called then.
int ps_rowfused_prepare() {
  using namespace ps;
  std::call_once(g_rf_once, [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess || n <= 0)
      return;
    const bool ok =
        rf_allow_lds(conv_rowfused_fwd_k<1>) &&
        rf_allow_lds(conv_rowfused_fwd_k<2>) &&
        rf_allow_lds(conv_rowfused_fwd_k<4>) &&
        rf_allow_lds(conv_rowfused_fwd_k<6>) &&
        rf_allow_lds(conv_rowfused_fwd_k<8>) &&
        rf_allow_lds(conv_rowfused_wgrad_k<1, 3>) &&
        rf_allow_lds(conv_rowfused_wgrad_k<2, 3>) &&
        rf_allow_lds(conv_rowfused_wgrad_k<4, 3>) &&
        rf_allow_lds(conv_rowfused_wgrad_k<6, 3>) &&
        rf_allow_lds(conv_rowfused_wgrad_k<8, 2>);
    if (ok) g_rf_cus.store(n);
  });
  return g_rf_cus.load() > 0 ? 1 : 0;
}

// y[NP][Co] = relu?(col @ wk^T + bias), col never materialized. x bf16 read
// through its element strides; wk the bf16 khwc shadow [Co][t->Kpad].
void ps_conv_rowfused_fwd(const RowFusedTiling* t, const void* x, int64_t sn,
                          int64_t sc, int64_t sh, int64_t sw, int64_t span,
                          const void* wk, const float* bias, void* y,
                          int relu, hipStream_t s) {
  const ps::RfX X = {(const __bf16*)x,
                     {sn, (int)sc, (int)sh, (int)sw, span}};
  const int fn = t->Cop / 16;
  if (fn <= 1) ps::rf_launch_fwd<1>(*t, X, wk, bias, y, relu, s);
  else if (fn <= 2) ps::rf_launch_fwd<2>(*t, X, wk, bias, y, relu, s);
  else if (fn <= 4) ps::rf_launch_fwd<4>(*t, X, wk, bias, y, relu, s);
  else if (fn <= 6) ps::rf_launch_fwd<6>(*t, X, wk, bias, y, relu, s);
  else ps::rf_launch_fwd<8>(*t, X, wk, bias, y, relu, s);
}

// dwk[Co][t->Kpad] (f32) += dy^T @ col. Adds atomically: dwk must be zero on
// entry (prezeroed), else it is cleared here first.
void ps_conv_rowfused_wgrad(const RowFusedTiling* t, const void* x,
                            int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                            int64_t span, const void* dy, float* dwk,
                            int prezeroed, hipStream_t s) {
  const ps::RfX X = {(const __bf16*)x,
                     {sn, (int)sc, (int)sh, (int)sw, span}};
  if (!prezeroed)
    PS_HIP_CHECK(hipMemsetAsync(
        dwk, 0, (size_t)t->Co * t->Kpad * sizeof(float), s));
  ps_count_float_atomic();
  const int fn = t->Cop / 16;
  if (fn <= 1) ps::rf_launch_wgrad<1, 3>(*t, X, dy, dwk, s);
  else if (fn <= 2) ps::rf_launch_wgrad<2, 3>(*t, X, dy, dwk, s);
  else if (fn <= 4) ps::rf_launch_wgrad<4, 3>(*t, X, dy, dwk, s);
  else if (fn <= 6) ps::rf_launch_wgrad<6, 3>(*t, X, dy, dwk, s);
  else ps::rf_launch_wgrad<8, 2>(*t, X, dy, dwk, s);  // <8, 3> spills
}

}  // extern "C"
