// Split-precision fp32 GEMM for gfx950 (CDNA4): fp32 operands, bf16 MFMAs.
//
// C[M,N] = alpha * op(A) @ op(B) + beta * C (+ bias[N])(, relu), A, B and C
// fp32, in the layouts fp32 training reaches (gemm.hip, dispatch_tiles):
// K-last x K-last (bias, ReLU, gathered A), K-last x K-major, K-major x
// K-major (gathered B); split-K atomically or through the f32 workspace.
//
// Every fp32 value x is written as hi + lo with hi = bf16(x) (round to
// nearest even) and lo = bf16(x - float(hi)); the subtraction is exact in
// fp32, so |x - hi - lo| <= 2^-18 |x|. A product a * b becomes three
// v_mfma_f32_16x16x32_bf16 into one fp32 accumulator: a_lo * b_hi, then
// a_hi * b_lo, then a_hi * b_hi, smallest terms first; lo * lo (<= 2^-18
// |a b|) is dropped. Arithmetic ceiling: a third of the bf16 MFMA rate,
// against v_mfma_f32_16x16x4_f32's vector-rate ceiling on the exact path.
//
// One kernel, gemm_split_kernel: 256 threads = 4 waves, each owning FM x FN
// fragments of 16x16, on the six square-menu tiles of PS_GEMM_TILE_LIST, so
// pick_gemm_tile and the split-K planner serve it unchanged (GemmShape::bk =
// PS_SPLIT3_BK, nt = false).
//
// Staging is through registers, always: the split is VALU work. Guarded
// 16 B f32x4 loads, zero-filled out of range, run one tile ahead of the
// MFMAs (write after the barrier, re-issue at once). The staged K tile is 32
// fp32 elements. At write time a thread splits 8 consecutive k of one row
// and stores one 16 B chunk into each of the operand's TWO LDS images, hi
// and lo, each [rows][32 k] bf16 = 64 B rows, unpadded: a 128x128 tile holds
// 2 operands x 2 images x 128 rows x 64 B x 2 buffers = 64 KiB, two blocks
// to a CU.
//
// LDS layout of an image (s3_off). Logical (row, chunk c = k / 8) lives at
//   physical row  (row & ~3) | ((row + (row >> 4)) & 3)
//   physical slot c ^ ((row >> 2) & 3)
// i.e. rows rotate within their aligned group of 4 by the index of their
// 16-row fragment, and the four 16 B slots of a row are XORed with the row's
// group-of-4 index. Paper conflict counts, for 64 banks x 4 B and a 128-bit
// LDS access served 16 lanes at a time (16 lanes x 16 B = one pass over all
// banks when conflict-free); a 16 B slot's bank group is (physical row & 3)
// * 4 + physical slot:
//   - fragment read (one ds_read_b128 per fragment and image): lane l reads
//     row l & 15 of the fragment at chunk l >> 4. 16 lanes = 16 rows, one
//     chunk: row & 3 (rotated by a constant) takes 4 values, for each of
//     which the XOR with (row >> 2) & 3 takes 4 slots -> 16 bank groups, 0
//     conflicts. Unswizzled 64 B rows would be 4-way (rows r, r + 4, r + 8,
//     r + 12 on the same 4 banks).
//   - K-last write: thread t owns chunk t & 3 of row t >> 2; 16 lanes cover 4
//     whole rows of one aligned group, a permutation of 256 contiguous
//     bytes -> 0 conflicts.
//   - K-major write: a thread loads 8 k-rows of 4 consecutive rows (f32x4
//     along the contiguous dimension, 32+ lanes side by side: coalesced) and
//     transposes the 4 x 8 block in registers into 4 chunks, one per row,
//     written by 4 instructions. In instruction j, 16 lanes hold rows j, j +
//     4, ..., j + 60 at one chunk: naively one bank group, 16-way. Here the
//     row's fragment index (4 values) rotates the physical row and its
//     group-of-4 index (4 values) XORs the slot -> 16 bank groups, 0
//     conflicts for tiles sides of 64 and 128 rows. A 32-row side has 8 such
//     rows per chunk and two chunks per 16 lanes: 2-way; a 16-row side 4-way
//     (4 rows x 4 chunks onto 4 bank groups). Those sides stage 1/4 and 1/8
//     of a 128-row side's bytes.
// Measured (profiles/fp32_split.md): the LDS bank-conflict counter reads 2.67
// conflict cycles per LDS instruction, a third of the LDS-active cycles, on
// the 4096^3 launches of BOTH layouts -- not the 0 of this model. 64 cycles a
// wave and tile is 4 per fragment read or 8 per write; which of the two the
// 16-consecutive-lanes model gets wrong is open (docs/ROADMAP.md).
//
// MFMA loop: per staged tile, FM + FN fragment reads per image (a_hi, a_lo,
// b_hi, b_lo), then the term loop OUTERMOST with the FM x FN nest inside, so
// the three MFMAs that feed one accumulator are FM * FN issues apart.
//
// Non-finite values: operands beyond bf16's largest finite value round hi to
// infinity and an infinite operand can give NaN (inf * 0 in a cross term)
// where exact fp32 gives infinity. Non-finite in, non-finite out; which kind
// is not defined.

// This file's device code is built without packed f32 arithmetic (the split's
// subtractions and the epilogue): a per-file switch, since the extension's
// sources share one set of compiler flags. It comes BEFORE the includes: a
// function without the attribute is never inlined into one that has it, and
// the kernel must not call its barrier, its epilogue or its address decode
// out of line.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "ps_common.h"
#include "ps_api.h"
#include "ps_gather.h"
#include "ps_gemm_device.h"  // gather_addr, gemm_epilogue, splitk_reduce_k

namespace ps {
namespace {

constexpr int S3_BK = PS_SPLIT3_BK;  // fp32 k per staged tile = bf16 k per MFMA
constexpr int S3_CH = S3_BK / 8;     // 16 B chunks of 8 bf16 per image row

// element offset of logical (row, chunk) in a [rows][32] bf16 image
__device__ inline int s3_off(int row, int chunk) {
  const int prow = (row & ~3) | ((row + (row >> 4)) & 3);
  return prow * S3_BK + ((chunk ^ (row >> 2)) & (S3_CH - 1)) * 8;
}

// x -> hi + lo, 8 values at a time (v_cvt_pk_bf16_f32, round to nearest even)
__device__ inline void s3_split(const float (&x)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const __bf16 h = (__bf16)x[e];
    hi[e] = h;
    lo[e] = (__bf16)(x[e] - (float)h);
  }
}

// One operand's side of a staged tile, [ROWS x 32 k] fp32, split into {issue
// global loads -> regs} and {split, write regs -> the two LDS images}.
// K-last: 16 B chunk c = row * 4 + k / 8 belongs to thread c % 256, two f32x4
// loads each. K-major: 4-row x 8-k block c = (k / 8) * (ROWS / 4) + row / 4
// belongs to thread c (operand A) or c + 128 (operand B, so that a 128-row A
// and B do not both land on the first two waves); ROWS <= 128 blocks, one per
// thread at most.
template <int ROWS, bool KLAST, bool GATHER, bool IS_B>
struct SplitStager {
  static constexpr int NCH = ROWS * S3_CH;
  static constexpr int NV = (NCH + 255) / 256;
  static constexpr int BLK_M = ROWS / 4;
  static constexpr int NB = BLK_M * S3_CH;
  static_assert(NB <= 128, "one K-major block per thread, B offset by 128");
  f32x4 v[KLAST ? 2 * NV : 8];

  __device__ static inline int block_of(int tid) {
    return IS_B ? (tid + 128) & 255 : tid;
  }

  __device__ inline void load(const float* src, int64_t ld, int row0,
                              int rows_max, int k0, int K, int tid,
                              const GatherDesc* ga) {
    if (KLAST) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = tid + i * 256;
        if (c >= NCH) break;
        const int gr = row0 + c / S3_CH;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int gk = k0 + (c % S3_CH) * 8 + h * 4;
          f32x4 val = {};
          if (gr < rows_max && gk < K) {
            if (GATHER) {
              // implicit im2col: bindings guarantee Cg % 4 == 0, so a run of
              // 4 k stays inside one cg run
              val = *reinterpret_cast<const f32x4*>(
                  gather_addr<float>(*ga, gr, gk));
            } else if (gk + 4 <= K) {
              val = *reinterpret_cast<const f32x4*>(&src[(int64_t)gr * ld + gk]);
            } else {
              for (int j = 0; j < 4; ++j)
                if (gk + j < K) val[j] = src[(int64_t)gr * ld + gk + j];
            }
          }
          v[2 * i + h] = val;
        }
      }
    } else {
      const int c = block_of(tid);
      if (c < NB) {
        const int gm = row0 + (c % BLK_M) * 4;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int gk = k0 + (c / BLK_M) * 8 + j;
          f32x4 val = {};
          if (gk < K && gm < rows_max) {
            // gathered (conv wgrad B = im2col): rows are im2col columns kg,
            // k is the im2col row
            if (gm + 4 <= rows_max) {
              val = *reinterpret_cast<const f32x4*>(
                  GATHER ? gather_addr<float>(*ga, gk, gm)
                         : &src[(int64_t)gk * ld + gm]);
            } else {
              for (int e = 0; e < 4; ++e)
                if (gm + e < rows_max)
                  val[e] = GATHER ? *gather_addr<float>(*ga, gk, gm + e)
                                  : src[(int64_t)gk * ld + gm + e];
            }
          }
          v[j] = val;
        }
      }
    }
  }

  __device__ inline void write(__bf16* hi_img, __bf16* lo_img, int tid) {
    if (KLAST) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = tid + i * 256;
        if (c >= NCH) break;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = v[2 * i + (e >> 2)][e & 3];
        bf16x8 hi, lo;
        s3_split(x, hi, lo);
        const int off = s3_off(c / S3_CH, c % S3_CH);
        *reinterpret_cast<bf16x8*>(&hi_img[off]) = hi;
        *reinterpret_cast<bf16x8*>(&lo_img[off]) = lo;
      }
    } else {
      const int c = block_of(tid);
      if (c < NB) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // j: row within the block
          float x[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = v[e][j];
          bf16x8 hi, lo;
          s3_split(x, hi, lo);
          const int off = s3_off((c % BLK_M) * 4 + j, c / BLK_M);
          *reinterpret_cast<bf16x8*>(&hi_img[off]) = hi;
          *reinterpret_cast<bf16x8*>(&lo_img[off]) = lo;
        }
      }
    }
  }
};

// One staged tile into the accumulators: a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
template <int FM, int FN>
__device__ inline void split_mma(const __bf16* a_hi, const __bf16* a_lo,
                                 const __bf16* b_hi, const __bf16* b_lo,
                                 int wm, int wn, int lane,
                                 f32x4 (&acc)[FM][FN]) {
  bf16x8 ah[FM], al[FM], bh[FN], bl[FN];
#pragma unroll
  for (int f = 0; f < FM; ++f) {
    const int off = s3_off(wm + f * 16 + (lane & 15), lane >> 4);
    ah[f] = *reinterpret_cast<const bf16x8*>(&a_hi[off]);
    al[f] = *reinterpret_cast<const bf16x8*>(&a_lo[off]);
  }
#pragma unroll
  for (int f = 0; f < FN; ++f) {
    const int off = s3_off(wn + f * 16 + (lane & 15), lane >> 4);
    bh[f] = *reinterpret_cast<const bf16x8*>(&b_hi[off]);
    bl[f] = *reinterpret_cast<const bf16x8*>(&b_lo[off]);
  }
#pragma unroll
  for (int term = 0; term < 3; ++term)
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            term == 0 ? al[fm] : ah[fm], term == 1 ? bl[fn] : bh[fn],
            acc[fm][fn], 0, 0, 0);
}

// xcd2d: the plan's 2D-XCD rectangle as (ry << 16) | cx, 0 for none
template <int BM, int BN, int WGM, int WGN, bool A_KLAST, bool B_KLAST,
          bool HAS_BIAS, bool SPLITK, bool GA, bool GB>
__global__ __launch_bounds__(256)
void gemm_split_kernel(const float* __restrict__ A,
                       const float* __restrict__ B, float* __restrict__ C,
                       const float* __restrict__ bias, int M, int N, int K,
                       int64_t lda, int64_t ldb, int64_t ldc, float alpha,
                       float beta, float* __restrict__ ws, int kchunk,
                       GatherDesc ga_a, GatherDesc ga_b, bool relu,
                       int xcd2d) {
  constexpr int BK = S3_BK;
  constexpr int FM = BM / WGM / 16, FN = BN / WGN / 16;
  static_assert(WGM * WGN == 4, "4 waves per block");

  const GemmBlock blk =
      xcd2d != 0 ? ps_remap_rect(gridDim.x, xcd2d >> 16, xcd2d & 0xFFFF,
                                 blockIdx.x, blockIdx.y)
                 : ps_remap_linear(gridDim.x, gridDim.y, gridDim.z,
                                   blockIdx.x, blockIdx.y, blockIdx.z);

  // [buffer][hi, lo][rows * 32]
  __shared__ __attribute__((aligned(16))) __bf16 a_lds[2][2][BM * BK];
  __shared__ __attribute__((aligned(16))) __bf16 b_lds[2][2][BN * BK];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = (wid / WGN) * (BM / WGM);
  const int wn = (wid % WGN) * (BN / WGN);
  const int m0 = blk.by * BM;
  const int n0 = blk.bx * BN;
  int k_begin = 0, k_end = K;
  if (SPLITK) {
    k_begin = blk.bz * kchunk;
    k_end = min(K, k_begin + kchunk);
  }

  f32x4 acc[FM][FN] = {};

  SplitStager<BM, A_KLAST, GA, false> sa;
  SplitStager<BN, B_KLAST, GB, true> sb;
  // prologue: tile 0 -> LDS[0]; issue tile 1 loads
  sa.load(A, lda, m0, M, k_begin, k_end, tid, &ga_a);
  sb.load(B, ldb, n0, N, k_begin, k_end, tid, &ga_b);
  sa.write(a_lds[0][0], a_lds[0][1], tid);
  sb.write(b_lds[0][0], b_lds[0][1], tid);
  if (k_begin + BK < k_end) {
    sa.load(A, lda, m0, M, k_begin + BK, k_end, tid, &ga_a);
    sb.load(B, ldb, n0, N, k_begin + BK, k_end, tid, &ga_b);
  }
  __syncthreads();

  int cur = 0;
  for (int k0 = k_begin; k0 < k_end; k0 += BK) {
    // regs hold tile t+1: split and write it into the other buffer, then
    // issue tile t+2's loads so they fly during this tile's MFMA phase
    if (k0 + BK < k_end) {
      sa.write(a_lds[cur ^ 1][0], a_lds[cur ^ 1][1], tid);
      sb.write(b_lds[cur ^ 1][0], b_lds[cur ^ 1][1], tid);
      if (k0 + 2 * BK < k_end) {
        sa.load(A, lda, m0, M, k0 + 2 * BK, k_end, tid, &ga_a);
        sb.load(B, ldb, n0, N, k0 + 2 * BK, k_end, tid, &ga_b);
      }
    }
    split_mma<FM, FN>(a_lds[cur][0], a_lds[cur][1], b_lds[cur][0],
                      b_lds[cur][1], wm, wn, lane, acc);
    __syncthreads();
    cur ^= 1;
  }
  gemm_epilogue<float, FM, FN, HAS_BIAS, SPLITK>(acc, C, bias, ws, M, N, ldc,
                                                 alpha, beta, relu, blk.bz,
                                                 m0, n0, wm, wn, lane);
}

// ---------------------------------------------------------------------------
// launching as planned
// ---------------------------------------------------------------------------

std::atomic<int> g_fp32_split{[] {
  const char* e = getenv("PS_FP32_SPLIT");
  return e && *e && strcmp(e, "0") != 0 ? 1 : 0;
}()};
std::atomic<int64_t> g_split_launches{0};

template <typename F>
void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

template <int BM, int BN, int WGM, int WGN, bool AK, bool BK_, bool HB,
          bool GA, bool GB>
void launch_tile(const GemmArgs& g, const GemmPlan& p, float* ws,
                 hipStream_t s) {
  GatherDesc da = GA ? *g.gather_a : GatherDesc{};
  GatherDesc db = GB ? *g.gather_b : GatherDesc{};
  dim3 grid(cdiv(g.N, BN), cdiv(g.M, BM), p.splitk);
  with_bool(p.splitk > 1, [&](auto sk) {
    gemm_split_kernel<BM, BN, WGM, WGN, AK, BK_, HB, decltype(sk)::value, GA,
                      GB><<<grid, 256, 0, s>>>(
        (const float*)g.A, (const float*)g.B, (float*)g.C, g.bias, g.M, g.N,
        g.K, g.lda, g.ldb, g.ldc, g.alpha, g.beta, ws, p.kchunk, da, db,
        g.relu, (p.ry << 16) | p.cx);
  });
  if (p.splitk == 1 || !ws) return;  // atomic split-K accumulated into C
  int64_t rb = cdiv64((int64_t)g.M * g.N, 256);
  if (rb > 2048) rb = 2048;
  splitk_reduce_k<float, HB><<<dim3((unsigned)rb), 256, 0, s>>>(
      ws, (float*)g.C, g.bias, g.M, g.N, g.ldc, p.splitk, g.alpha, g.beta,
      g.relu);
}

[[noreturn]] void die(const GemmArgs& g, const GemmPlan& p, const char* what) {
  fprintf(stderr,
          "split gemm: %s: %dx%d tile, %s in, A %s%s, B %s%s%s is not built\n",
          what, p.bm, p.bn, g.in_bf16 ? "bf16" : "f32",
          g.a_klast ? "K-last" : "K-major", g.gather_a ? " gathered" : "",
          g.b_klast ? "K-last" : "K-major", g.gather_b ? " gathered" : "",
          g.bias ? ", bias" : "");
  abort();
}

// the six square-menu tiles of PS_GEMM_TILE_LIST; the N-fitting tiles are
// not built for this path and never planned (GemmShape::nt = false)
template <bool AK, bool BK_, bool HB, bool GA, bool GB>
void dispatch_tiles(const GemmArgs& g, const GemmPlan& p, float* ws,
                    hipStream_t s) {
#define PS_SPLIT_CASE(BM_, BN_, WGM_, WGN_, NARROW_)                        \
  if constexpr (!NARROW_)                                                   \
    if (p.bm == BM_ && p.bn == BN_)                                         \
      return launch_tile<BM_, BN_, WGM_, WGN_, AK, BK_, HB, GA, GB>(g, p,   \
                                                                    ws, s);
  PS_GEMM_TILE_LIST(PS_SPLIT_CASE)
#undef PS_SPLIT_CASE
  die(g, p, "tile");
}

}  // namespace

extern "C" {

void ps_set_fp32_split(int on) { g_fp32_split.store(on ? 1 : 0); }
int ps_fp32_split() { return g_fp32_split.load(); }
int64_t ps_fp32_split_launches(int reset) {
  return reset ? g_split_launches.exchange(0) : g_split_launches.load();
}

void ps_gemm_split_run(const GemmArgs* gp, const GemmPlan* plan, float* ws,
                       hipStream_t s) {
  const GemmArgs& g = *gp;
  const GemmPlan& p = *plan;
  const bool nt = g.a_klast && g.b_klast;
  if (g.in_bf16 || !g.out_f32 || (!g.a_klast && g.b_klast) ||
      ((g.bias || g.gather_a) && !nt) ||
      (g.gather_b && (g.a_klast || g.b_klast)))
    die(g, p, "dtype x layout x epilogue");
  g_split_launches.fetch_add(1);
  if (nt) {
    with_bool(g.bias != nullptr, [&](auto hb) {
      with_bool(g.gather_a != nullptr, [&](auto ga) {
        dispatch_tiles<true, true, decltype(hb)::value, decltype(ga)::value,
                       false>(g, p, ws, s);
      });
    });
  } else if (g.a_klast) {
    dispatch_tiles<true, false, false, false, false>(g, p, ws, s);
  } else {
    with_bool(g.gather_b != nullptr, [&](auto gb) {
      dispatch_tiles<false, false, false, false, decltype(gb)::value>(g, p,
                                                                      ws, s);
    });
  }
}

}  // extern "C"

}  // namespace ps

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
