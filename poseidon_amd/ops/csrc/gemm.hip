// MFMA GEMM for gfx950 (CDNA4): the single compute primitive behind
// InnerProduct, implicit-GEMM convolution (over im2col tiles), and the SFB
// outer-product reconstruction.
//
// C[M,N] = alpha * op(A) @ op(B) + beta * C (+ bias[N])
//   - op(A) is [M,K]: stored K-last ([M][lda], lda>=K) or K-major
//     ([K][lda], lda>=M; staged with an on-the-fly transpose into LDS)
//   - op(B) is [K,N]: stored as [N][ldb] K-last (the natural NT form) or
//     [K][ldb] K-major (staged transposed)
//   - A (K-last) or B (K-major) may be GATHERED from an NHWC activation
//     instead of read from a matrix (implicit im2col, ps_gather.h)
//
// Every launch decision -- path, tile, split-K, K slice, XCD placement -- is
// made once by ps_gemm_plan (policy in ps_gemm_plan.h, checked on the host by
// tests/gemm_plan_host.cpp); ps_gemm_run executes that plan. Two kernels:
//
// gemm_kernel, the generic tiles (PS_GEMM_TILE_LIST): every forward, every
//   dgrad, every fp32 GEMM and whatever tr16 does not take. 256 threads = 4
//   waves, each owning a sub-tile of 16x16 fragments of
//   v_mfma_f32_16x16x32_bf16 (bf16, K step 32) or v_mfma_f32_16x16x4_f32
//   (fp32, K step 4, exact f32 at the 155 TF vector-rate ceiling); LDS is
//   double-buffered. A block picks one of two main loops:
//   - glds: interior tiles of K-last x K-last operands with 16 B-aligned
//     rows stage by global_load_lds, 16 B per lane straight into a linear,
//     source-swizzled LDS image; a gathered A walks its addresses
//     (GatherWalk); a K % BK tail is staged by guarded scalar writes.
//   - register-staged: everything else (edge tiles, K-major operands,
//     unaligned rows). Guarded vector loads into registers, written to LDS
//     rows padded by 16 B (K-last) or block-transposed and XOR-swizzled
//     (K-major), one tile ahead of the MFMAs.
//   Split-K slices either store raw partials to a workspace that
//   splitk_reduce_k combines, or add atomically into a zeroed f32 C.
//
// gemm_tn_tr_kernel, the tr16 tiles (PS_TR_TILE_LIST): bf16 in / f32 out with
//   both operands K-major -- the weight gradients. Natural [k][col] images
//   staged by glds and read through ds_read_b64_tr_b16. Covers the 16 x 64
//   aligned interior; edge strips run as unsplit generic sub-problems.
//
// Replaces the reference's cuBLAS call sites (math_functions.cu:16-65,
// conv_layer.cu:25-121, inner_product_layer.cu:18-63).

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "ps_common.h"
#include "ps_api.h"
#include "ps_gather.h"

namespace ps {

template <typename T> struct GemmTraits;

template <> struct GemmTraits<float> {
  static constexpr int BK = 16;      // K elems per LDS tile
  static constexpr int KSTEP = 4;    // K per MFMA
  static constexpr int VEC = 4;      // elems per staging vector load
  static constexpr int RS = BK + 4;  // padded LDS row stride (elems)
  static constexpr int GSH = 2;      // log2(VEC): k-group shift for swizzle
  using vec_t = f32x4;
  using frag_t = float;  // one A/B element per lane
  __device__ static inline f32x4 mfma(frag_t a, frag_t b, f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  __device__ static inline frag_t load_frag(const float* lds_row, int kk, int lane) {
    return lds_row[kk + (lane >> 4)];
  }
};

template <> struct GemmTraits<__bf16> {
  static constexpr int BK = 64;
  static constexpr int KSTEP = 32;
  static constexpr int VEC = 8;
  static constexpr int RS = BK + 8;  // 144 B rows: 16B-aligned, conflict-spread
  static constexpr int GSH = 3;      // log2(VEC)
  typedef __attribute__((ext_vector_type(8))) __bf16 vec_t;
  using frag_t = bf16x8;
  __device__ static inline f32x4 mfma(frag_t a, frag_t b, f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }
  __device__ static inline frag_t load_frag(const __bf16* lds_row, int kk, int lane) {
    return *reinterpret_cast<const frag_t*>(&lds_row[kk + (lane >> 4) * 8]);
  }
};

// Implicit-GEMM address: row = im2col row (n,oh,ow), k = column within the
// group slice (khw*Cg + cg). Returns the NHWC x address of k's element run
// (contiguous along cg), or the zero page for padding. Valid for vector
// loads that stay inside one cg-run (callers guarantee k%VEC==0, Cg%VEC==0).
// The integer logic lives in ps_gather.h.
template <typename T>
__device__ inline const T* gather_addr(const GatherDesc& ga, int64_t row, int k) {
  if (k >= ga.kg_max) return (const T*)ga.zero;  // padded columns
  const GatherRow r = ps_gather_row(ga, (int)row);
  const GatherTap t = ps_gather_tap(ga, k);
  if (ps_gather_oob(ga, r, t, k)) return (const T*)ga.zero;
  return (const T*)ga.x + ps_gather_offset(r, t);
}

// Direct global->LDS staging (glds): each wave-instruction moves 1 KiB
// (64 lanes x 16 B) HBM -> LDS without a VGPR round trip
// (__builtin_amdgcn_global_load_lds, width 16 -- guide §5 step 3: the
// +67% width-4 -> width-16 lever). The LDS image is LINEAR [row][BK]
// (the builtin writes wave-uniform-base + lane*16), so this path is used
// for interior tiles of K-last operands only; fragment reads use the
// unpadded BK stride.
template <typename T, int ROWS>
struct GldsMap {
  using TR = GemmTraits<T>;
  static constexpr int EPB = 16 / (int)sizeof(T);  // elems per 16B lane-load
  static constexpr int LPR = TR::BK / EPB;         // lanes per row
  static constexpr int RPC = 64 / LPR;             // rows per 1KB chunk
  static constexpr int CHUNKS = ROWS / RPC;
  static constexpr int CPL = (CHUNKS + 3) / 4;     // chunks per lane
  // Wave wid stages chunks wid, wid + 4, ...: all CPL of them when CHUNKS is
  // a multiple of 4. Saying so at compile time matters: wid comes from
  // threadIdx, so a run-time `ci < CHUNKS` is a per-lane compare and wraps
  // every load after the first in exec-mask save/restore and a branch.
  __device__ static inline bool live(int ci) {
    return CHUNKS % 4 == 0 || ci < CHUNKS;
  }
  // rule 21: the LDS image is XOR-swizzled by swizzling the SOURCE
  // address per lane (glds writes lane-linear); reads apply the same XOR.
  // ONE-bit (32 B-pair) swizzle, the 8-phase template's st_16x32 form:
  // full-slot permutations also kill bank conflicts but destroy the
  // request coalescer's lane-order contiguity (13x slower at L3-resident
  // sizes); the pair swap keeps 32 B runs contiguous and still cuts
  // ds_read_b128 conflicts 8-way -> 4-way. (A 2-bit slot swizzle keyed
  // on row bits 1-2 makes the fragment reads fully conflict-free on
  // paper, but flipping slot bit 0 reorders 16 B chunks within 32 B
  // pairs on the WRITE side and measured -5%% end-to-end on AlexNet/VGG
  // -- the global request coalescer penalty outweighs the LDS win.)
  // The swizzle bit is row bit 2 and a chunk is a multiple of 8 rows, so a
  // lane has ONE k column for all of its chunks.
  static_assert(RPC % 8 == 0, "swizzle bit must not depend on the chunk");
  __device__ static inline int r_in(int lane) { return lane / LPR; }
  __device__ static inline int kc(int lane) {
    const int swb = (r_in(lane) >> 2) & 1;
    return ((lane % LPR) ^ (swb << 1)) * EPB;
  }
  __device__ static inline void load(T* lds, int ci, const void* g) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)g,
        (__attribute__((address_space(3))) void*)(lds + ci * (1024 / (int)sizeof(T))),
        16, 0, 0);
  }
};

template <typename T, int ROWS>
__device__ inline void stage_glds(T* lds, const T* __restrict__ src,
                                  int64_t lda, int row0, int k0, int wid,
                                  int lane) {
  using MP = GldsMap<T, ROWS>;
  const int r_in = MP::r_in(lane), kc = MP::kc(lane);
#pragma unroll
  for (int i = 0; i < MP::CPL; ++i) {
    const int ci = wid + 4 * i;
    if (!MP::live(ci)) break;
    const int row = ci * MP::RPC + r_in;
    MP::load(lds, ci, src + (int64_t)(row0 + row) * lda + k0 + kc);
  }
}

// The same staging for a GATHERED A (implicit im2col): identical bytes into
// identical LDS slots, the addresses walked instead of decoded. A lane
// stages the same rows and the same column-within-the-tile for every k-tile,
// so it decodes its rows (two divisions each) and its tap ONCE, keeps a byte
// pointer to each row's window origin, and per tile pays two adds and two
// unsigned compares for the padding test, one 64-bit add and one select per
// chunk, plus one tap advance (ps_gather.h). The per-tile decode this
// replaces was 181 VALU per tile against 51 for a plain A.
template <typename T, int ROWS>
struct GatherWalk {
  using MP = GldsMap<T, ROWS>;
  static constexpr int CPL = MP::CPL;
  const char* rowp[CPL];  // x + row base, in bytes (see GatherRow::base)
  int ih0[CPL], iw0[CPL];
  GatherTap tap;
  int k;  // the tap's column

  __device__ inline void init(const GatherDesc& ga, int row0, int k0, int wid,
                              int lane) {
    const int r_in = MP::r_in(lane);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int ci = wid + 4 * i;
      if (!MP::live(ci)) break;
      const GatherRow r = ps_gather_row(ga, row0 + ci * MP::RPC + r_in);
      rowp[i] = (const char*)ga.x + r.base * (int64_t)sizeof(T);
      ih0[i] = r.ih0;
      iw0[i] = r.iw0;
    }
    k = k0 + MP::kc(lane);
    tap = ps_gather_tap(ga, k);
  }

  // stage the tile at the tap's column, then move the tap one tile on
  __device__ inline void stage(T* lds, const GatherDesc& ga, int wid) {
    const bool dead = k >= ga.kg_max;
    const int64_t tapb = (int64_t)tap.off * (int64_t)sizeof(T);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int ci = wid + 4 * i;
      if (!MP::live(ci)) break;
      const bool oob = dead | ps_gather_pad(ga, ih0[i], iw0[i], tap);
      const char* g = rowp[i] + tapb;
      MP::load(lds, ci, oob ? (const char*)ga.zero : g);
    }
    ps_gather_tap_advance(ga, tap, k, GemmTraits<T>::BK);
    k += GemmTraits<T>::BK;
  }
};

// matching read-side XOR for glds-staged tiles: element offset within a
// linear [row][BK] image whose 16 B slots are swizzled by row
template <typename T>
__device__ inline int glds_col(int row, int col) {
  constexpr int EPB = 16 / (int)sizeof(T);
  int slot = col / EPB;
  return (slot ^ (((row >> 2) & 1) << 1)) * EPB + (col % EPB);
}

// Guarded scalar staging of a PARTIAL final K-tile into the glds-layout
// image (zero-filled beyond k_end): lets a GEMM whose K is not a BK
// multiple still take the glds path for the full tiles (AlexNet conv2's
// implicit fwd at K=1200 was otherwise stuck on the guarded register
// pipeline for every tile: 674 us -> glds + this tail).
template <typename T, int ROWS, bool GATHER = false>
__device__ inline void stage_tail_linear(T* lds, const T* __restrict__ src,
                                         int64_t lda, int row0, int k0,
                                         int k_end, int tid,
                                         const GatherDesc* ga = nullptr) {
  using TR = GemmTraits<T>;
  constexpr int BK = TR::BK;
  const int rem = k_end - k0;
  for (int i = tid; i < ROWS * BK; i += 256) {
    const int row = i / BK, col = i - row * BK;
    T v = (T)0.0f;
    if (col < rem) {
      if (GATHER)
        v = gather_addr<T>(*ga, row0 + row, k0 + (col & ~(TR::VEC - 1)))
                [col & (TR::VEC - 1)];
      else
        v = src[(int64_t)(row0 + row) * lda + k0 + col];
    }
    lds[row * BK + glds_col<T>(row, col)] = v;
  }
}

// Column offset inside an LDS tile row. K-major-staged tiles XOR the
// k-group index with the row band so the block-transposed vector writes
// spread across banks (write lanes hit 8 distinct banks instead of 1);
// fragment reads apply the same XOR. K-last tiles stay linear.
template <typename T, bool SWZ>
__device__ inline int lds_col(int row, int kk) {
  using TR = GemmTraits<T>;
  if (!SWZ) return kk;
  constexpr int GM = (TR::BK / TR::VEC) - 1;  // k-group mask
  int kg = kk >> TR::GSH;
  return (((kg ^ (row >> TR::GSH)) & GM) << TR::GSH) | (kk & (TR::VEC - 1));
}

// The three column layouts of a staged tile; fragment reads undo them.
enum ColMap {
  COL_PADDED,  // register-staged K-last: linear, rows padded to RS
  COL_KMAJOR,  // register-staged K-major: lds_col swizzle, rows padded to RS
  COL_GLDS,    // glds: glds_col swizzle, unpadded BK rows
};
template <typename T, ColMap MAP>
__device__ inline int tile_col(int row, int col) {
  if (MAP == COL_GLDS) return glds_col<T>(row, col);
  return lds_col<T, MAP == COL_KMAJOR>(row, col);
}

// Staging, split into {issue global loads -> regs} and {write regs -> LDS}
// halves so the next tile's HBM latency hides under the current tile's MFMA
// phase (guide T14 / Guideline 15: write AFTER the barrier, re-issue at
// once). A [ROWS x BK] tile is ROWS*BK/(256*VEC) vectors per thread.
// Guarded, zero-filled out of range.
template <typename T, int ROWS, bool KLAST, bool GATHER = false,
          bool FASTI = false>
struct Stager {
  using TR = GemmTraits<T>;
  using vec_t = typename TR::vec_t;
  static constexpr int TV = ROWS * TR::BK / TR::VEC;  // total vectors in tile
  static constexpr int NV = (TV + 255) / 256;         // per-thread (>=1)
  // K-major path: VEC x VEC blocks, VEC vectors each
  static constexpr int TB = ROWS * TR::BK / (TR::VEC * TR::VEC);
  static constexpr int NVB = (TB + 255) / 256;
  vec_t v[KLAST ? NV : NVB * TR::VEC];

  __device__ inline void load(const T* src, int64_t lda, int row0,
                              int rows_max, int k0, int K, int tid,
                              const GatherDesc* ga = nullptr) {
    // Interior tiles of K-MAJOR operands take a branch with NO per-vector
    // guards: the guarded form makes the compiler wrap EVERY 16 B load in
    // s_and_saveexec exec-mask juggling plus a scalarized edge clone --
    // measured as the dominant cost of the TN/NN staging path. The code
    // duplication costs ~36 VGPRs, which pushes the NON-split-K 128x128
    // bf16 instantiation over the 256-VGPR occupancy cliff (224 -> 260,
    // -30% at 4096^3), so FASTI (= SPLITK at the launch site, 200 VGPR)
    // gates it to the split-K kernels where it measures +9%.
    const bool interior = FASTI &&
        (row0 + ROWS <= rows_max) && (k0 + TR::BK <= K);
    if (KLAST) {
      constexpr int CK = TR::BK / TR::VEC;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        int c = tid + i * 256;
        if (c >= TV) break;
        int r = c / CK, kc = c % CK;
        int gr = row0 + r, gk = k0 + kc * TR::VEC;
        vec_t val = {};
        if (gr < rows_max && gk < K) {
          if (GATHER) {
            // implicit im2col: one VEC run per (row, k-chunk); bindings
            // guarantee Cg % VEC == 0 so the run is contiguous
            val = *reinterpret_cast<const vec_t*>(
                gather_addr<T>(*ga, gr, gk));
          } else if (gk + TR::VEC <= K) {
            val = *reinterpret_cast<const vec_t*>(&src[(int64_t)gr * lda + gk]);
          } else {
            for (int j = 0; j < TR::VEC; ++j)
              if (gk + j < K) val[j] = src[(int64_t)gr * lda + gk + j];
          }
        }
        v[i] = val;
      }
    } else if (GATHER) {
      // K-major gather (conv wgrad B = im2col): rows dim is Kg (contiguous
      // within cg runs), K dim is NP (im2col rows)
      constexpr int BLK_M = ROWS / TR::VEC;
#pragma unroll
      for (int i = 0; i < NVB; ++i) {
        int c = tid + i * 256;
        if (c >= TB) break;
        int kb = c / BLK_M, mb = c % BLK_M;
        int gm = row0 + mb * TR::VEC;  // kg (column of im2col)
#pragma unroll
        for (int j = 0; j < TR::VEC; ++j) {
          int gk = k0 + kb * TR::VEC + j;  // np (im2col row)
          vec_t val = {};
          if (gk < K && gm + TR::VEC <= rows_max)
            val = *reinterpret_cast<const vec_t*>(
                gather_addr<T>(*ga, gk, gm));
          else if (gk < K && gm < rows_max) {
            for (int e = 0; e < TR::VEC; ++e)
              if (gm + e < rows_max)
                val[e] = *gather_addr<T>(*ga, gk, gm + e);
          }
          v[i * TR::VEC + j] = val;
        }
      }
    } else if (interior) {
      // K-major interior: VEC unguarded row-vector loads per block
      constexpr int BLK_M = ROWS / TR::VEC;
#pragma unroll
      for (int i = 0; i < NVB; ++i) {
        int c = tid + i * 256;
        if (c >= TB) break;
        int kb = c / BLK_M, mb = c % BLK_M;
        const T* base = &src[(int64_t)(k0 + kb * TR::VEC) * lda
                             + row0 + mb * TR::VEC];
#pragma unroll
        for (int j = 0; j < TR::VEC; ++j)
          v[i * TR::VEC + j] =
              *reinterpret_cast<const vec_t*>(base + (int64_t)j * lda);
      }
    } else {
      // K-major: each thread owns a VEC x VEC block (k-block kb, m-block mb)
      // and loads VEC row-vectors along the contiguous m dim (coalesced
      // across lanes: consecutive threads -> consecutive m-blocks)
      constexpr int BLK_M = ROWS / TR::VEC;
#pragma unroll
      for (int i = 0; i < NVB; ++i) {
        int c = tid + i * 256;
        if (c >= TB) break;
        int kb = c / BLK_M, mb = c % BLK_M;
        int gm = row0 + mb * TR::VEC;
#pragma unroll
        for (int j = 0; j < TR::VEC; ++j) {
          int gk = k0 + kb * TR::VEC + j;
          vec_t val = {};
          if (gk < K && gm < rows_max) {
            if (gm + TR::VEC <= rows_max) {
              val = *reinterpret_cast<const vec_t*>(&src[(int64_t)gk * lda + gm]);
            } else {
              for (int e = 0; e < TR::VEC; ++e)
                if (gm + e < rows_max) val[e] = src[(int64_t)gk * lda + gm + e];
            }
          }
          v[i * TR::VEC + j] = val;
        }
      }
    }
  }

  __device__ inline void write(T* lds, int tid) {
    if (KLAST) {
      constexpr int CK = TR::BK / TR::VEC;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        int c = tid + i * 256;
        if (c >= TV) break;
        int r = c / CK, kc = c % CK;
        *reinterpret_cast<vec_t*>(&lds[r * TR::RS + kc * TR::VEC]) = v[i];
      }
    } else {
      // register-transpose the VEC x VEC block, then VEC aligned vector
      // writes to swizzled columns (conflict-free within the lane group)
      constexpr int BLK_M = ROWS / TR::VEC;
#pragma unroll
      for (int i = 0; i < NVB; ++i) {
        int c = tid + i * 256;
        if (c >= TB) break;
        int kb = c / BLK_M, mb = c % BLK_M;
#pragma unroll
        for (int j = 0; j < TR::VEC; ++j) {  // j: m within the block
          vec_t out;
#pragma unroll
          for (int e = 0; e < TR::VEC; ++e) out[e] = v[i * TR::VEC + e][j];
          int row = mb * TR::VEC + j;
          *reinterpret_cast<vec_t*>(
              &lds[row * TR::RS + lds_col<T, true>(row, kb * TR::VEC)]) = out;
        }
      }
    }
  }
};

// Tile geometry: BM x BN block tile, 4 waves arranged WGM x WGN, each wave
// owns a (BM/WGM) x (BN/WGN) sub-tile as FM x FN fragments of 16x16.
// (m0, n0) is the block tile's origin, (wm, wn) the wave sub-tile's origin
// inside it. The parts below take these as plain ints: gathered into a
// struct, the compiler staged K-last operands differently from the kernel
// they were cut from (profiles/gemm_refactor.md).

// One staged K-tile into the accumulators: per MFMA k-step, FM + FN fragment
// reads and the FM x FN MFMA nest. RS is the images' row stride, MAPA / MAPB
// their column layouts.
template <typename T, int FM, int FN, int RS, ColMap MAPA, ColMap MAPB>
__device__ inline void tile_mma(const T* al, const T* bl, int wm, int wn,
                                int lane, f32x4 (&acc)[FM][FN]) {
  using TR = GemmTraits<T>;
#pragma unroll
  for (int kk = 0; kk < TR::BK; kk += TR::KSTEP) {
    typename TR::frag_t a_frag[FM], b_frag[FN];
#pragma unroll
    for (int f = 0; f < FM; ++f) {
      int row = wm + f * 16 + (lane & 15);
      int col = kk + (lane >> 4) * (TR::KSTEP / 4);
      a_frag[f] = *reinterpret_cast<const typename TR::frag_t*>(
          &al[row * RS + tile_col<T, MAPA>(row, col)]);
    }
#pragma unroll
    for (int f = 0; f < FN; ++f) {
      int row = wn + f * 16 + (lane & 15);
      int col = kk + (lane >> 4) * (TR::KSTEP / 4);
      b_frag[f] = *reinterpret_cast<const typename TR::frag_t*>(
          &bl[row * RS + tile_col<T, MAPB>(row, col)]);
    }
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        acc[fm][fn] = TR::mfma(a_frag[fm], b_frag[fn], acc[fm][fn]);
  }
}

// glds main loop: full BK tiles via glds, one tile ahead of the MFMAs; a
// partial final tile (K % BK != 0) is staged by guarded scalar writes into
// the same swizzled image. a_lds / b_lds hold two buffers of BUF_A / BUF_B
// elements each.
template <typename T, int BM, int BN, int FM, int FN, bool GA, int BUF_A,
          int BUF_B>
__device__ inline void mainloop_glds(const T* A, const T* B, int64_t lda,
                                     int64_t ldb, const GatherDesc& ga_a,
                                     T* a_lds, T* b_lds, int m0, int n0,
                                     int k_begin, int k_end, int tid,
                                     int lane, int wid, int wm, int wn,
                                     f32x4 (&acc)[FM][FN]) {
  constexpr int BK = GemmTraits<T>::BK;
  const int k_full = k_begin + ((k_end - k_begin) / BK) * BK;
  T* a_lin0 = a_lds;
  T* b_lin0 = b_lds;
  T* a_lin1 = a_lds + BUF_A;
  T* b_lin1 = b_lds + BUF_B;
  GatherWalk<T, BM> walk;  // GA only
  if constexpr (GA) {
    walk.init(ga_a, m0, k_begin, wid, lane);
    walk.stage(a_lin0, ga_a, wid);
  } else {
    stage_glds<T, BM>(a_lin0, A, lda, m0, k_begin, wid, lane);
  }
  stage_glds<T, BN>(b_lin0, B, ldb, n0, k_begin, wid, lane);
  __syncthreads();  // drains the in-flight glds (vmcnt 0) + barrier
  int cur = 0;
  for (int k0 = k_begin; k0 < k_end; k0 += BK) {
    if (k0 + BK < k_full) {
      // consecutive full tiles: the walk's tap sits at k0 + BK
      if constexpr (GA)
        walk.stage(cur ? a_lin0 : a_lin1, ga_a, wid);
      else
        stage_glds<T, BM>(cur ? a_lin0 : a_lin1, A, lda, m0, k0 + BK, wid,
                          lane);
      stage_glds<T, BN>(cur ? b_lin0 : b_lin1, B, ldb, n0, k0 + BK, wid,
                        lane);
    } else if (k0 + BK < k_end) {
      stage_tail_linear<T, BM, GA>(cur ? a_lin0 : a_lin1, A, lda, m0,
                                   k0 + BK, k_end, tid, &ga_a);
      stage_tail_linear<T, BN, false>(cur ? b_lin0 : b_lin1, B, ldb, n0,
                                      k0 + BK, k_end, tid, nullptr);
    }
    tile_mma<T, FM, FN, BK, COL_GLDS, COL_GLDS>(
        cur ? a_lin1 : a_lin0, cur ? b_lin1 : b_lin0, wm, wn, lane, acc);
    __syncthreads();
    cur ^= 1;
  }
}

// Epilogue: C/D fragment map for 16x16 shapes: col = lane&15,
// row = (lane>>4)*4 + r (guide §3; dtype-independent on gfx950).
// bz is the split-K slice (the workspace slab it writes).
template <typename OUT, int FM, int FN, bool HAS_BIAS, bool SPLITK>
__device__ inline void gemm_epilogue(const f32x4 (&acc)[FM][FN],
                                     OUT* __restrict__ C,
                                     const float* __restrict__ bias,
                                     float* __restrict__ ws, int M, int N,
                                     int64_t ldc, float alpha, float beta,
                                     bool relu, int bz, int m0, int n0,
                                     int wm, int wn, int lane) {
#pragma unroll
  for (int fm = 0; fm < FM; ++fm) {
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      int col = n0 + wn + fn * 16 + (lane & 15);
      if (col >= N) continue;
      float bv = HAS_BIAS ? bias[col] : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wm + fm * 16 + (lane >> 4) * 4 + r;
        if (row >= M) continue;
        if (SPLITK) {
          if (ws) {
            // raw partial; alpha/beta/bias applied by the reduce kernel
            ws[((int64_t)bz * M + row) * N + col] = acc[fm][fn][r];
          } else if constexpr (std::is_same<OUT, float>::value) {
            // atomic split-K: accumulate straight into zeroed f32 C --
            // no workspace round-trip, no reduce kernel; lets the launcher
            // split K much deeper (wgrad tiles are tiny: M=Cout)
            atomicAdd(&C[(int64_t)row * ldc + col], alpha * acc[fm][fn][r]);
          }
        } else {
          int64_t idx = (int64_t)row * ldc + col;
          float v = alpha * acc[fm][fn][r] + bv;
          if (beta != 0.0f) v += beta * to_f32(C[idx]);
          if (relu && v < 0.0f) v = 0.0f;  // fused in-place ReLU epilogue
          from_f32(v, C[idx]);
        }
      }
    }
  }
}

// xcd2d: the plan's 2D-XCD rectangle as (ry << 16) | cx, 0 for none
template <typename T, typename OUT, int BM, int BN, int WGM, int WGN,
          bool A_KLAST, bool B_KLAST, bool HAS_BIAS, bool SPLITK,
          bool GA = false, bool GB = false>
__global__ __launch_bounds__(256)
void gemm_kernel(const T* __restrict__ A, const T* __restrict__ B,
                 OUT* __restrict__ C, const float* __restrict__ bias,
                 int M, int N, int K,
                 int64_t lda, int64_t ldb, int64_t ldc,
                 float alpha, float beta,
                 float* __restrict__ ws, int kchunk,
                 GatherDesc ga_a = {}, GatherDesc ga_b = {},
                 bool relu = false, int xcd2d = 0) {
  using TR = GemmTraits<T>;
  constexpr int BK = TR::BK, RS = TR::RS;
  constexpr int FM = BM / WGM / 16, FN = BN / WGN / 16;
  static_assert(WGM * WGN == 4, "4 waves per block");

  const GemmBlock blk =
      xcd2d != 0 ? ps_remap_rect(gridDim.x, xcd2d >> 16, xcd2d & 0xFFFF,
                                 blockIdx.x, blockIdx.y)
                 : ps_remap_linear(gridDim.x, gridDim.y, gridDim.z,
                                   blockIdx.x, blockIdx.y, blockIdx.z);

  __shared__ __attribute__((aligned(16))) T a_lds[2][BM * RS];
  __shared__ __attribute__((aligned(16))) T b_lds[2][BN * RS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = (wid / WGN) * (BM / WGM);  // wave row offset in block tile
  const int wn = (wid % WGN) * (BN / WGN);
  const int m0 = blk.by * BM;
  const int n0 = blk.bx * BN;
  // split-K: grid.z indexes the K slice
  int k_begin = 0, k_end = K;
  if (SPLITK) {
    k_begin = blk.bz * kchunk;
    k_end = min(K, k_begin + kchunk);
  }

  f32x4 acc[FM][FN] = {};

  // glds fast path: interior tile, K-span a multiple of BK, vector-aligned
  // rows (guide §5: direct-to-LDS staging removes the VGPR round trip and
  // its VALU address work; edge tiles keep the guarded register pipeline)
  constexpr int EPB = 16 / (int)sizeof(T);
  bool glds_ok = A_KLAST && B_KLAST && (m0 + BM <= M) &&
                 (n0 + BN <= N) && k_end - k_begin >= BK &&
                 (ldb % EPB) == 0 && (k_begin % EPB) == 0 &&
                 (((uintptr_t)B & 15) == 0);
  if (GA) {
    // gathered A: every 16 B lane chunk must stay inside one cg run
    // (chunk starts are EPB-aligned, so Cg % EPB suffices -- the old
    // Cg % BK gate was overly strict and pushed grouped convs like
    // AlexNet conv2 (Cg=48) onto the guarded register-gather path)
    glds_ok = glds_ok && (ga_a.Cg % EPB) == 0 && (ga_a.C % EPB) == 0 &&
              (ga_a.c0 % EPB) == 0;
  } else {
    glds_ok = glds_ok && (lda % EPB) == 0 && (((uintptr_t)A & 15) == 0);
  }
  if (glds_ok) {
    mainloop_glds<T, BM, BN, FM, FN, GA, BM * RS, BN * RS>(
        A, B, lda, ldb, ga_a, a_lds[0], b_lds[0], m0, n0, k_begin, k_end, tid,
        lane, wid, wm, wn, acc);
  } else {
    // Register-staged main loop: guarded loads for every tile the glds loop
    // cannot take (edge tiles, K-major operands, unaligned rows). It stays
    // in the kernel body: as a function of its own the compiler merges two of
    // the three staging-load sites of the K-major kernels and drains them
    // with more waits (fp32 4096x9216x256 K-major x K-major: 95 -> 80 TF/s,
    // profiles/gemm_refactor.md).
    Stager<T, BM, A_KLAST, GA, SPLITK> sa;
    Stager<T, BN, B_KLAST, GB, SPLITK> sb;
    // prologue: tile 0 -> LDS[0]; issue tile 1 loads
    sa.load(A, lda, m0, M, k_begin, k_end, tid, &ga_a);
    sb.load(B, ldb, n0, N, k_begin, k_end, tid, &ga_b);
    sa.write(a_lds[0], tid);
    sb.write(b_lds[0], tid);
    if (k_begin + BK < k_end) {
      sa.load(A, lda, m0, M, k_begin + BK, k_end, tid, &ga_a);
      sb.load(B, ldb, n0, N, k_begin + BK, k_end, tid, &ga_b);
    }
    __syncthreads();

    int cur = 0;
    for (int k0 = k_begin; k0 < k_end; k0 += BK) {
      // regs hold tile t+1: write it into the other LDS buffer, then issue
      // tile t+2's loads so they fly during this tile's MFMA phase
      if (k0 + BK < k_end) {
        sa.write(a_lds[cur ^ 1], tid);
        sb.write(b_lds[cur ^ 1], tid);
        if (k0 + 2 * BK < k_end) {
          sa.load(A, lda, m0, M, k0 + 2 * BK, k_end, tid, &ga_a);
          sb.load(B, ldb, n0, N, k0 + 2 * BK, k_end, tid, &ga_b);
        }
      }
      tile_mma<T, FM, FN, RS, A_KLAST ? COL_PADDED : COL_KMAJOR,
               B_KLAST ? COL_PADDED : COL_KMAJOR>(a_lds[cur], b_lds[cur], wm,
                                                  wn, lane, acc);
      __syncthreads();
      cur ^= 1;
    }
  }
  gemm_epilogue<OUT, FM, FN, HAS_BIAS, SPLITK>(acc, C, bias, ws, M, N, ldc,
                                               alpha, beta, relu, blk.bz, m0,
                                               n0, wm, wn, lane);
}

// combine split-K partial slabs: C = alpha*sum_s ws[s] + bias + beta*C
template <typename OUT, bool HAS_BIAS>
__global__ void splitk_reduce_k(const float* __restrict__ ws,
                                OUT* __restrict__ C,
                                const float* __restrict__ bias,
                                int M, int N, int64_t ldc, int splitk,
                                float alpha, float beta, bool relu) {
  int64_t MN = (int64_t)M * N;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < MN;
       i += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    for (int s = 0; s < splitk; ++s) v += ws[s * MN + i];
    int row = i / N, col = i % N;
    v *= alpha;
    if (HAS_BIAS) v += bias[col];
    int64_t idx = (int64_t)row * ldc + col;
    if (beta != 0.0f) v += beta * to_f32(C[idx]);
    if (relu && v < 0.0f) v = 0.0f;
    from_f32(v, C[idx]);
  }
}


// ---------------------------------------------------------------------------
// TN fast path: both operands K-major, staged by glds in their NATURAL
// [BK][cols] row-major-in-k images and consumed through gfx950's
// ds_read_b64_tr_b16 hardware transpose-read (guide T10). Replaces the
// register block-transpose staging (59.5% wave-parked, 5.5 VALU per MFMA
// -- profiles/r01_tn_gemm_pmc.md) for eligible tiles: measured 46 -> 246
// TF/s on the VGG conv1_2 wgrad shape (64x576x1.6M), +14..40% on other
// wgrad shapes. Semantics probe: experiments/tr16_probe.hip -- within a
// 16-lane group, lane l loads 4 contiguous bf16 at its own 8B-aligned
// address and lane j receives element j of each 16-element chunk of the
// group's concatenated loads; pointing lane l at row kk+l/4, col
// cb+4*(l%4) of the [k][col] image hands lane j the k-run of col cb+j.
// Eligibility (checked by the launcher): M,N,K % 64 == 0, lda/ldb % 8 == 0,
// 16B-aligned bases, bf16 in / f32 out, no gathers, no bias, beta == 0.
// ---------------------------------------------------------------------------

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// Row-dependent 16 B-chunk XOR for the tr16 LDS image. Without it the
// ds_read_b64_tr_b16 lane groups put 4 lanes on each dword bank (rows r
// and r+2 / r+8 alias at row-stride COLS*2 B mod 256 B): measured 6.0
// LDS bank-conflict cycles per LDS instruction, 58.8%% of wave cycles
// parked. The XOR spreads the 8 rows a lane group touches across disjoint
// 16 B bands -> conflict-free reads. Writers permute the SOURCE lane
// (global_load_lds writes lane-linear), readers apply the same XOR.
template <int COLS>
__device__ inline int tr_swz(int row, int chunk) {
  constexpr int MASK = (COLS / 8) - 1;  // chunks per row
  const int p = (((row >> 1) & 1) << 1) ^ (((row >> 3) & 1) << 2);
  return chunk ^ (p & MASK);
}

template <int COLS, bool GATHER = false, bool NT = false>
__device__ inline void stage_kmaj_tr(__bf16* lds, const __bf16* src,
                                     int64_t ld, int k0, int c0, int wid,
                                     int lane,
                                     const GatherDesc* ga = nullptr) {
  // [BK=64 rows][COLS cols]: COLS*2 B rows, 16 B lane chunks. GATHER:
  // the operand is the im2col matrix gathered on the fly from NHWC x
  // (row = im2col row np, col = kg) -- implicit wgrad without a colT.
  constexpr int LPR = COLS / 8;       // lanes per row
  constexpr int RPC = 64 / LPR;       // rows per 1 KB chunk
  constexpr int CHUNKS = 64 / RPC;
  const int r_in = lane / LPR;
  const int slot = lane % LPR;
  // gather: the column decode (kg -> kh,kw,cg) depends on the swizzled
  // source chunk, which takes one of 4 values per lane -- precompute all
  // 4 decodes so the chunk loop still runs decode-free.
  int kkh[4], kkw[4], cg[4];
  if (GATHER) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int sl = slot ^ ((p << 1) & (LPR - 1));
      int khw = ps_fdiv_fix(c0 + sl * 8, ga->Cg, ga->inv_Cg, cg[p]);
      kkh[p] = ps_fdiv_fix(khw, ga->kw, ga->inv_kw, kkw[p]);
    }
  }
#pragma unroll
  for (int ci = wid; ci < CHUNKS; ci += 4) {
    const int row = ci * RPC + r_in;
    const int pi = ((row >> 1) & 1) | (((row >> 3) & 1) << 1);
    const int sslot = tr_swz<COLS>(row, slot);
    const __bf16* g2;
    if (GATHER) {
      int ow, oh;
      const int t2 = ps_fdiv_fix(k0 + row, ga->Wo, ga->inv_Wo, ow);
      const int n2 = ps_fdiv_fix(t2, ga->Ho, ga->inv_Ho, oh);
      const int ih = oh * ga->sh - ga->ph + kkh[pi];
      const int iw = ow * ga->sw - ga->pw + kkw[pi];
      g2 = (ih < 0 || ih >= ga->H || iw < 0 || iw >= ga->W)
               ? (const __bf16*)ga->zero
               : (const __bf16*)ga->x +
                     (((int64_t)n2 * ga->H + ih) * ga->W + iw) * ga->C +
                     ga->c0 + cg[pi];
    } else {
      g2 = src + (int64_t)(k0 + row) * ld + c0 + sslot * 8;
    }
    // NT (aux=2): the B stream is read by exactly ONE block; keep it from
    // evicting the XCD-L2-resident A slice the clustered tiles share
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)g2,
        (__attribute__((address_space(3))) void*)(lds + ci * 512), 16, 0,
        NT ? 2 : 0);
  }
}

// Issues the two transpose-reads WITHOUT waiting -- the caller batches all
// fragment reads of a k-step behind one s_waitcnt (tr_wait) so the LDS
// latency of 16 reads overlaps instead of serializing.
template <int COLS>
__device__ inline bf16x8 tr_frag(unsigned lds_base, int kk, int cb, int l,
                                 int ldt) {
  const int r1 = kk + (l >> 2), r2 = r1 + 4;
  const int c = cb + 4 * (l & 3);
  const int c1 = (tr_swz<COLS>(r1, c >> 3) << 3) | (c & 7);
  const int c2 = (tr_swz<COLS>(r2, c >> 3) << 3) | (c & 7);
  const unsigned a1 = lds_base + (unsigned)((r1 * ldt + c1) * 2);
  const unsigned a2 = lds_base + (unsigned)((r2 * ldt + c2) * 2);
  bf16x4 v1, v2;
  // "=&v" early-clobber: insn 1 writes v1 before insn 2 consumes a2
  asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
               "ds_read_b64_tr_b16 %1, %3"
               : "=&v"(v1), "=&v"(v2) : "v"(a1), "v"(a2));
  bf16x8 f;
#pragma unroll
  for (int i = 0; i < 4; ++i) { f[i] = v1[i]; f[4 + i] = v2[i]; }
  return f;
}

// drain the outstanding tr reads, then pin EVERY fragment behind the wait
// with an empty volatile asm (volatile asms are ordered against each
// other; a bare clobber would let the compiler hoist register uses)
template <int NA, int NB>
__device__ inline void tr_wait(bf16x8 (&a)[NA], bf16x8 (&b)[NB]) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int i = 0; i < NA; ++i) asm volatile("" : "+v"(a[i]));
#pragma unroll
  for (int i = 0; i < NB; ++i) asm volatile("" : "+v"(b[i]));
}

// A panel of W > 64 columns is staged as 64-column sub-images (96 = 64 +
// 32), each a [64][COLS] image with its OWN tr_swz, laid one after the
// other; a fragment (16 columns) never straddles two of them. Two reasons:
// stage_kmaj_tr needs COLS / 8 to divide 64 (96, 192), and a 128-column
// image has 256 B rows -- every row starts on bank 0 and tr_swz's two row
// bits leave a 4-way conflict (measured 2-4 conflict cycles per MFMA on the
// 32x128 / 64x128 tiles against 0.0 on 64x64), which 128 B rows do not have.
// A sub-image that starts at or past cmax (ragged last N tile,
// ps_tr_sub_live) is not staged at all: only dead waves would read it.
template <int W, bool GATHER = false, bool NT = false>
__device__ inline void stage_panel_tr(__bf16* lds, const __bf16* src,
                                      int64_t ld, int k0, int c0, int cmax,
                                      int wid, int lane,
                                      const GatherDesc* ga = nullptr) {
  if constexpr (W <= 64) {
    stage_kmaj_tr<W, GATHER, NT>(lds, src, ld, k0, c0, wid, lane, ga);
  } else {
#pragma unroll
    for (int i = 0; i < W / 64; ++i)
      if (ps_tr_sub_live(c0, i, cmax))
        stage_kmaj_tr<64, GATHER, NT>(lds + i * 64 * 64, src, ld, k0,
                                      c0 + i * 64, wid, lane, ga);
    if constexpr (W % 64 != 0)
      stage_kmaj_tr<W % 64, GATHER, NT>(lds + (W / 64) * 64 * 64, src, ld,
                                        k0, c0 + (W / 64) * 64, wid, lane,
                                        ga);
  }
}

template <int W>
__device__ inline bf16x8 tr_panel_frag(unsigned lds_base, int kk, int cb,
                                       int l) {
  if constexpr (W <= 64) {
    return tr_frag<W>(lds_base, kk, cb, l, W);
  } else if constexpr (W % 64 == 0) {
    return tr_frag<64>(lds_base + (unsigned)(cb >> 6) * (64 * 64 * 2), kk,
                       cb & 63, l, 64);
  } else {
    constexpr int FULL = W / 64 * 64;  // columns in whole sub-images
    if (cb < FULL)
      return tr_frag<64>(lds_base + (unsigned)(cb >> 6) * (64 * 64 * 2), kk,
                         cb & 63, l, 64);
    return tr_frag<W % 64>(lds_base + FULL * 64 * 2, kk, cb - FULL, l,
                           W % 64);
  }
}

// SPLITK: how a block's K slice reaches C.
//   TR_NOSPLIT  one block per tile, plain stores of alpha * acc
//   TR_ATOMIC   atomicAdd of alpha * acc into the zeroed C
//   TR_WS       deterministic mode: C is the f32 workspace [splitk][M][N] and
//               the block stores its raw partial into slab bz (ldC unused);
//               splitk_reduce_tr_k sums the slabs in order and applies alpha.
//               Padded bz blocks and dead waves store nothing, so only slabs
//               < splitk and columns < N are ever read back.
enum { TR_NOSPLIT = 0, TR_ATOMIC = 1, TR_WS = 2 };

template <int BM2, int BN2, int WGM2, int WGN2, int SPLITK,
          bool GB2 = false>
__global__ __launch_bounds__(256)
void gemm_tn_tr_kernel(const __bf16* __restrict__ A,
                       const __bf16* __restrict__ B, float* __restrict__ C,
                       int M, int N, int K, int64_t ldA, int64_t ldB,
                       int64_t ldC, float alpha, int kchunk,
                       GatherDesc ga_b = {}) {
  constexpr int FM2 = BM2 / WGM2 / 16, FN2 = BN2 / WGN2 / 16;
  static_assert(WGM2 * WGN2 == 4, "4 waves");
  __shared__ __attribute__((aligned(16))) __bf16 a_lds[2][64 * BM2];
  __shared__ __attribute__((aligned(16))) __bf16 b_lds[2][64 * BN2];
  // (by, bz) groups clustered per XCD when split, else the linear swizzle;
  // a padded bz exits via the k_begin >= k_end guard below
  const GemmBlock blk = ps_remap_tr(SPLITK != TR_NOSPLIT, gridDim.x,
                                    gridDim.y, gridDim.z,
                                    blockIdx.x, blockIdx.y, blockIdx.z);
  const int bx = blk.bx, by = blk.by, bz = blk.bz;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = WGM2 == 1 ? 0 : (wid / WGN2) * (BM2 / WGM2);
  const int wn = (wid % WGN2) * (BN2 / WGN2);
  const int m0 = by * BM2;
  const int n0 = bx * BN2;
  // ragged last N tile (N % 64 == 0, grid.x = ceil(N / BN2)): a dead wave
  // skips fragment reads, MFMAs and stores but reaches every barrier
  const bool live = BN2 > 64 ? ps_tr_wave_live(n0, wn, N) : true;
  int k_begin = 0, k_end = K;
  if (SPLITK) {
    k_begin = bz * kchunk;
    k_end = min(K, k_begin + kchunk);
    if (k_begin >= k_end) return;
  }
  const int l = lane & 15, q = lane >> 4;

  f32x4 acc[FM2][FN2] = {};
  // NT-stream B only when: one row of tiles (each B byte read once), B is
  // a materialized operand (a gather re-reads warm x kh*kw-fold -- nt
  // would push every re-read to HBM), and the stream is too big to be
  // cache-resident anyway (small colT matrices are L2/L3-HOT from the
  // im2col that just wrote them; nt measured -4% on AlexNet/GoogLeNet)
  const bool ntb = SPLITK != TR_NOSPLIT && gridDim.y == 1 && !GB2 &&
                   (int64_t)K * N * 2 > (192LL << 20);
  if (ntb)
    stage_panel_tr<BN2, GB2, true>(b_lds[0], B, ldB, k_begin, n0, N, wid,
                                   lane, &ga_b);
  else
    stage_panel_tr<BN2, GB2, false>(b_lds[0], B, ldB, k_begin, n0, N, wid,
                                    lane, &ga_b);
  stage_panel_tr<BM2>(a_lds[0], A, ldA, k_begin, m0, M, wid, lane);
  __syncthreads();
  unsigned ab[2], bb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    ab[i] = (unsigned)(unsigned long long)(
        __attribute__((address_space(3))) __bf16*)a_lds[i];
    bb[i] = (unsigned)(unsigned long long)(
        __attribute__((address_space(3))) __bf16*)b_lds[i];
  }
  int cur = 0;
  for (int k0 = k_begin; k0 < k_end; k0 += 64) {
    if (k0 + 64 < k_end) {
      stage_panel_tr<BM2>(a_lds[cur ^ 1], A, ldA, k0 + 64, m0, M, wid,
                          lane);
      if (ntb)
        stage_panel_tr<BN2, GB2, true>(b_lds[cur ^ 1], B, ldB, k0 + 64, n0,
                                       N, wid, lane, &ga_b);
      else
        stage_panel_tr<BN2, GB2, false>(b_lds[cur ^ 1], B, ldB, k0 + 64, n0,
                                        N, wid, lane, &ga_b);
    }
    // DEEP=2: both 32-k halves' transpose-reads go out before ONE wait,
    // doubling the MFMA burst per s_waitcnt (the 4-MFMA burst cannot hide
    // 8 ds_read_b64_tr latencies). Register cost doubles the fragment set,
    // so only tiles with FM2+FN2 <= 4 take it.
    constexpr int DEEP = (FM2 + FN2 <= 4) ? 2 : 1;
    if (live) {
#pragma unroll
    for (int kk = 0; kk < 64; kk += 32 * DEEP) {
      bf16x8 af[DEEP][FM2], bfr[DEEP][FN2];
#pragma unroll
      for (int d = 0; d < DEEP; ++d) {
#pragma unroll
        for (int f = 0; f < FM2; ++f)
          af[d][f] = tr_panel_frag<BM2>(ab[cur], kk + d * 32 + q * 8,
                                        wm + f * 16, l);
#pragma unroll
        for (int f = 0; f < FN2; ++f)
          bfr[d][f] = tr_panel_frag<BN2>(bb[cur], kk + d * 32 + q * 8,
                                         wn + f * 16, l);
      }
      tr_wait(af[0], bfr[0]);
      if (DEEP == 2) tr_wait(af[DEEP - 1], bfr[DEEP - 1]);
#pragma unroll
      for (int d = 0; d < DEEP; ++d)
#pragma unroll
        for (int fm = 0; fm < FM2; ++fm)
#pragma unroll
          for (int fn = 0; fn < FN2; ++fn)
            acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[d][fm], bfr[d][fn], acc[fm][fn], 0, 0, 0);
    }
    }
    __syncthreads();
    cur ^= 1;
  }
  if (!live) return;  // past the last barrier
#pragma unroll
  for (int fm = 0; fm < FM2; ++fm)
#pragma unroll
    for (int fn = 0; fn < FN2; ++fn) {
      const int col = n0 + wn + fn * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + fm * 16 + (lane >> 4) * 4 + r;
        if (SPLITK == TR_WS)
          C[((int64_t)bz * M + row) * N + col] = acc[fm][fn][r];
        else if (SPLITK == TR_ATOMIC)
          atomicAdd(&C[(int64_t)row * ldC + col], alpha * acc[fm][fn][r]);
        else
          C[(int64_t)row * ldC + col] = alpha * acc[fm][fn][r];
      }
    }
}

// Ordered combine of the TR_WS slabs: C[row][col] = alpha * (ws[0] + ws[1] +
// ... + ws[splitk - 1]) over the M x N interior, slabs added in ascending
// order whatever order their blocks ran in. N % 64 == 0, so the slabs are
// read as float4; C is stored as float4 when its rows allow (VST).
template <bool VST>
__global__ void splitk_reduce_tr_k(const float* __restrict__ ws,
                                   float* __restrict__ C, int M, int N,
                                   int64_t ldc, int splitk, float alpha) {
  const int N4 = N / 4;
  const int64_t MN4 = (int64_t)M * N4;
  const f32x4* ws4 = (const f32x4*)ws;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < MN4;
       i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 v = ws4[i];
    for (int s = 1; s < splitk; ++s) v += ws4[s * MN4 + i];
    v *= alpha;
    const int64_t row = i / N4;
    const int col = (int)(i - row * N4) * 4;
    float* out = C + row * ldc + col;
    if (VST) {
      *(f32x4*)out = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) out[e] = v[e];
    }
  }
}

// ---------------------------------------------------------------------------
// planning (ps_gemm_plan) and launching as planned (ps_gemm_run)
// ---------------------------------------------------------------------------

// Atomic split-K adds into C, which the launcher zeroes as ONE contiguous
// M*N block: only when nothing else lands in C and its rows are dense.
static bool atomic_splitk_ok(const GemmArgs& g) {
  return g.out_f32 && g.bias == nullptr && g.beta == 0.0f && !g.relu &&
         g.ldc == g.N;
}

// Operand eligibility for the tr16 TN path: what ps_gemm_plan.h cannot see
// from the shape alone (dtypes, layouts, alignment, epilogue).
static bool tn_tr_operands_ok(const GemmArgs& g) {
  if (!g.in_bf16 || !g.out_f32) return false;
  if (g.a_klast || g.b_klast || g.gather_a) return false;
  if (g.bias || g.relu || g.beta != 0.0f) return false;
  if (g.lda % 8) return false;
  if ((uintptr_t)g.A & 15) return false;
  if (g.gather_b) {
    const GatherDesc& gb = *g.gather_b;
    if (gb.Cg % 8 || gb.C % 8 || gb.c0 % 8) return false;
  } else {
    if (g.ldb % 8 || ((uintptr_t)g.B & 15)) return false;
  }
  return true;
}

static GemmShape gemm_shape(const GemmArgs& g) {
  GemmShape sh;
  sh.M = g.M;
  sh.N = g.N;
  sh.K = g.K;
  sh.esize = g.in_bf16 ? (int)sizeof(__bf16) : (int)sizeof(float);
  sh.bk = g.in_bf16 ? GemmTraits<__bf16>::BK : GemmTraits<float>::BK;
  sh.atomic_ok = atomic_splitk_ok(g);
  sh.tr_ok = tn_tr_operands_ok(g);
  sh.gather_b = g.gather_b != nullptr;
  sh.nt = g.a_klast && g.b_klast;
  sh.only128 = !g.a_klast && g.b_klast;
  sh.deterministic = ps_deterministic() != 0;
  return sh;
}

// Deterministic mode (ps_set_deterministic) and the count of launches that
// add floats atomically (ps_float_atomic_launches): process-wide, shared by
// every translation unit's launchers.
static std::atomic<int> g_deterministic{[] {
  const char* e = getenv("PS_DETERMINISTIC");
  return e && *e && strcmp(e, "0") != 0 ? 1 : 0;
}()};
static std::atomic<int64_t> g_float_atomic_launches{0};

// a launcher about to take an atomic-float path: counted, and fatal in
// deterministic mode (the bindings raise before it comes to this)
static void float_atomic_launch(const char* what) {
  if (ps_deterministic()) {
    fprintf(stderr, "%s: atomic float path taken in deterministic mode\n",
            what);
    abort();
  }
  ps_count_float_atomic();
}

// tests / tuning only (ps_gemm_set_tr_tune); all zero in the training path
static TrTune g_tr_tune = {0, 0, 0};

// Atomic split-K accumulates into C: zero it here, once, unless the caller
// owns a buffer that the net-level zero_mt launch already zeroed this
// iteration (GoogLeNet: ~57 fillBuffer launches/step eliminated).
// atomic_splitk_ok guarantees C is one dense M*N block.
static void zero_c_for_atomics(const GemmArgs& g, hipStream_t s) {
  if (!g.c_prezeroed)
    (void)hipMemsetAsync(g.C, 0, (size_t)g.M * g.N * sizeof(float), s);
}

// run-time bool -> template argument: f(std::true_type{} / std::false_type{})
template <typename F>
static void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// The launchers decide nothing: grid and kernel arguments come from the plan.
template <typename T, typename OUT, int BM, int BN, int WGM, int WGN,
          bool AK, bool BK_, bool HB, bool GA, bool GB>
static void launch_tile(const GemmArgs& g, const GemmPlan& p, float* ws,
                        hipStream_t s) {
  GatherDesc da = GA ? *g.gather_a : GatherDesc{};
  GatherDesc db = GB ? *g.gather_b : GatherDesc{};
  dim3 grid(cdiv(g.N, BN), cdiv(g.M, BM), p.splitk);
  with_bool(p.splitk > 1, [&](auto sk) {
    gemm_kernel<T, OUT, BM, BN, WGM, WGN, AK, BK_, HB, decltype(sk)::value,
                GA, GB><<<grid, 256, 0, s>>>(
        (const T*)g.A, (const T*)g.B, (OUT*)g.C, g.bias, g.M, g.N, g.K,
        g.lda, g.ldb, g.ldc, g.alpha, g.beta, ws, p.kchunk, da, db, g.relu,
        (p.ry << 16) | p.cx);
  });
  if (p.splitk == 1 || !ws) return;  // atomic split-K accumulated into C
  int64_t rb = cdiv64((int64_t)g.M * g.N, 256);
  if (rb > 2048) rb = 2048;
  splitk_reduce_k<OUT, HB><<<dim3((unsigned)rb), 256, 0, s>>>(
      ws, (OUT*)g.C, g.bias, g.M, g.N, g.ldc, p.splitk, g.alpha, g.beta,
      g.relu);
}

static const char* dtype_name(bool bf16) { return bf16 ? "bf16" : "f32"; }

static void die_not_built(const GemmArgs& g, const char* what) {
  fprintf(stderr,
          "gemm: %s: %s in, %s out, A %s%s, B %s%s%s is not instantiated\n",
          what, dtype_name(g.in_bf16), dtype_name(!g.out_f32),
          g.a_klast ? "K-last" : "K-major", g.gather_a ? " gathered" : "",
          g.b_klast ? "K-last" : "K-major", g.gather_b ? " gathered" : "",
          g.bias ? ", bias" : "");
  abort();
}

// which tiles of PS_GEMM_TILE_LIST a layout is built for: the N-fitting
// tiles for K-last x K-last only; A K-major x B K-last (test entry only)
// for 128x128 only
constexpr bool tile_built(int bm, int bn, bool narrow_only, bool ak,
                          bool bk) {
  return (!narrow_only || (ak && bk)) && (ak || !bk || (bm == 128 && bn == 128));
}

// WHAT IS INSTANTIATED follows what the run_gemm call sites in bindings.cpp
// can produce. C has the input dtype in every forward and data-gradient
// GEMM and is f32 in every weight gradient and in the test entry ext.gemm
// (which has no bias and no gather). So:
//   - a bias or a gathered A (forward / dgrad-as-forward) comes only with
//     OUT == T;
//   - a K-major A (weight gradients and gemm_at_b, gathered B included; the
//     test entry) comes only with f32 out.
// f32 x f32 satisfies both, bf16 -> bf16 and bf16 -> f32 one each. Anything
// else aborts by name; so does a planned tile the layout is not built for.
template <typename T, typename OUT, bool AK, bool BK_, bool HB, bool GA,
          bool GB>
static void dispatch_tiles(const GemmArgs& g, const GemmPlan& p, float* ws,
                           hipStream_t s) {
  constexpr bool same = std::is_same<T, OUT>::value;
  constexpr bool f32out = std::is_same<OUT, float>::value;
  if constexpr (((HB || GA) && !same) || (!AK && !f32out)) {
    die_not_built(g, "dtype x layout x epilogue");
  } else {
#define PS_GEMM_CASE(BM_, BN_, WGM_, WGN_, NARROW_)                         \
  if constexpr (tile_built(BM_, BN_, NARROW_, AK, BK_))                     \
    if (p.bm == BM_ && p.bn == BN_)                                         \
      return launch_tile<T, OUT, BM_, BN_, WGM_, WGN_, AK, BK_, HB, GA, GB>( \
          g, p, ws, s);
    PS_GEMM_TILE_LIST(PS_GEMM_CASE)
#undef PS_GEMM_CASE
    fprintf(stderr, "gemm: no %dx%d tile\n", p.bm, p.bn);
    die_not_built(g, "tile");
  }
}

template <typename T, typename OUT>
static void gemm_dispatch(const GemmArgs& g, const GemmPlan& p, float* ws,
                          hipStream_t s) {
  const bool nt = g.a_klast && g.b_klast;
  // bias and gathered A exist for K-last x K-last, gathered B for K-major x
  // K-major
  if (((g.bias || g.gather_a) && !nt) ||
      (g.gather_b && (g.a_klast || g.b_klast)))
    die_not_built(g, "layout");
  if (nt) {
    // forward GEMMs; gathered A: implicit-GEMM conv forward
    with_bool(g.bias != nullptr, [&](auto hb) {
      with_bool(g.gather_a != nullptr, [&](auto ga) {
        dispatch_tiles<T, OUT, true, true, decltype(hb)::value,
                       decltype(ga)::value, false>(g, p, ws, s);
      });
    });
  } else if (g.a_klast) {
    dispatch_tiles<T, OUT, true, false, false, false, false>(g, p, ws, s);
  } else if (g.b_klast) {
    // unused in the framework (kept for the generic test entry)
    dispatch_tiles<T, OUT, false, true, false, false, false>(g, p, ws, s);
  } else {
    // gathered B: implicit-GEMM conv wgrad, K-major B gathered from x
    with_bool(g.gather_b != nullptr, [&](auto gb) {
      dispatch_tiles<T, OUT, false, false, false, false,
                     decltype(gb)::value>(g, p, ws, s);
    });
  }
}

static void run_gemm_generic(const GemmArgs& g, const GemmPlan& p, float* ws,
                             hipStream_t s) {
  if (p.ws_elems == 0) ws = nullptr;
  if (p.splitk > 1 && !ws) {
    float_atomic_launch("gemm split-K");
    zero_c_for_atomics(g, s);
  }
  if (!g.in_bf16) gemm_dispatch<float, float>(g, p, ws, s);
  else if (g.out_f32) gemm_dispatch<__bf16, float>(g, p, ws, s);
  else gemm_dispatch<__bf16, __bf16>(g, p, ws, s);
}

// run-time tr16 split mode -> template argument
template <typename F>
static void with_tr_mode(int mode, F&& f) {
  if (mode == TR_WS) f(std::integral_constant<int, TR_WS>{});
  else if (mode == TR_ATOMIC) f(std::integral_constant<int, TR_ATOMIC>{});
  else f(std::integral_constant<int, TR_NOSPLIT>{});
}

static void run_gemm_tn_tr(const GemmArgs& g, const GemmPlan& p, float* ws,
                           hipStream_t s) {
  const int M0 = p.M0, N0 = p.N0;
  const int mode = p.splitk == 1  ? TR_NOSPLIT
                   : p.ws_elems > 0 ? TR_WS
                                    : TR_ATOMIC;
  if (mode == TR_WS && !ws) {
    fprintf(stderr, "tr16 gemm: the plan's split-K workspace is missing\n");
    abort();
  }
  if (mode == TR_ATOMIC) {
    float_atomic_launch("tr16 gemm split-K");
    zero_c_for_atomics(g, s);
  }
  // TR_WS: the kernel writes slabs, the reduce below overwrites C's interior
  float* out = mode == TR_WS ? ws : (float*)g.C;
  // ceil: a bn = 128 grid runs its last column tile ragged (N0 % 64 == 0);
  // grid.z padded: enables L2 clustering
  dim3 grid((N0 + p.bn - 1) / p.bn, M0 / p.bm, ps_tr_grid_z(p));
  GatherDesc gb = g.gather_b ? *g.gather_b : GatherDesc{};
#define PS_TR_CASE(BM_, BN_, WGM_, WGN_)                                    \
  if (p.bm == BM_ && p.bn == BN_)                                           \
    with_tr_mode(mode, [&](auto sk) {                                       \
      with_bool(g.gather_b != nullptr, [&](auto gat) {                      \
        gemm_tn_tr_kernel<BM_, BN_, WGM_, WGN_, decltype(sk)::value,        \
                          decltype(gat)::value><<<grid, 256, 0, s>>>(       \
            (const __bf16*)g.A, (const __bf16*)g.B, out, M0, N0,            \
            g.K, g.lda, g.ldb, g.ldc, g.alpha, p.kchunk, gb);               \
      });                                                                   \
    });                                                                     \
  else
  PS_TR_TILE_LIST(PS_TR_CASE) {
    fprintf(stderr, "tr16 gemm: no %dx%d tile\n", p.bm, p.bn);
    abort();
  }
#undef PS_TR_CASE
  if (mode == TR_WS) {
    int64_t rb = cdiv64((int64_t)M0 * N0 / 4, 256);
    if (rb > 2048) rb = 2048;
    float* c = (float*)g.C;
    if (g.ldc % 4 == 0 && ((uintptr_t)c & 15) == 0)
      splitk_reduce_tr_k<true><<<dim3((unsigned)rb), 256, 0, s>>>(
          ws, c, M0, N0, g.ldc, p.splitk, g.alpha);
    else
      splitk_reduce_tr_k<false><<<dim3((unsigned)rb), 256, 0, s>>>(
          ws, c, M0, N0, g.ldc, p.splitk, g.alpha);
  }
  // edge strips [0,M) x [N0,N) and [M0,M) x [0,N0): unsplit generic
  // sub-problems (plain stores over the zeroed C)
  auto strip = [&](GemmArgs gt) {
    GemmPlan sp;
    ps_generic_plan(gemm_shape(gt), &sp, /*may_split=*/false);
    run_gemm_generic(gt, sp, nullptr, s);
  };
  if (N0 != g.N) {
    GemmArgs gt = g;
    gt.N = g.N - N0;
    gt.B = (const void*)((const __bf16*)g.B + N0);
    gt.C = (void*)((float*)g.C + N0);
    strip(gt);
  }
  if (M0 != g.M) {
    GemmArgs gt = g;
    gt.M = g.M - M0; gt.N = N0;
    gt.A = (const void*)((const __bf16*)g.A + M0);
    gt.C = (void*)((float*)g.C + (int64_t)M0 * g.ldc);
    strip(gt);
  }
}

extern "C" {

// tr16 plan first (bf16 in, fp32 out only), else the generic plan
void ps_gemm_plan(const GemmArgs* g, GemmPlan* plan) {
  const GemmShape sh = gemm_shape(*g);
  if (!ps_tn_tr_plan(sh, g_tr_tune, plan)) ps_generic_plan(sh, plan);
}

void ps_set_deterministic(int on) { g_deterministic.store(on ? 1 : 0); }
int ps_deterministic() { return g_deterministic.load(); }
void ps_count_float_atomic() { g_float_atomic_launches.fetch_add(1); }
int64_t ps_float_atomic_launches(int reset) {
  return reset ? g_float_atomic_launches.exchange(0)
               : g_float_atomic_launches.load();
}

void ps_gemm_set_tr_tune(int bm, int bn, int target) {
  g_tr_tune = {bm, bn, target};
}

// ws: plan->ws_elems floats (null when the plan asks for none)
void ps_gemm_run(const GemmArgs* g, const GemmPlan* plan, float* ws,
                 hipStream_t s) {
  if (plan->tr16) return run_gemm_tn_tr(*g, *plan, ws, s);
  run_gemm_generic(*g, *plan, ws, s);
}

}  // extern "C"

}  // namespace ps
