// GEMM plan: every launch decision for one GEMM -- path, tile, split-K, K
// slice, XCD placement -- derived ONCE from the problem shape (ps_gemm_plan
// in gemm.hip fills a GemmShape from its GemmArgs and calls in here; the
// launchers decide nothing). Also the block-index remaps the kernels apply.
// Plain C++ (no torch / HIP includes) so it also compiles into a stand-alone
// host program (tests/gemm_plan_host.cpp).
#pragma once
#include <cstdint>

#include "ps_conv_plan.h"  // PS_HD

// How ps_gemm_run will execute a GemmArgs: made once by ps_gemm_plan, which
// owns path choice and split-K policy. Split-K (small-tile huge-K GEMMs,
// e.g. conv wgrad) either accumulates atomically into C -- the launcher
// zeroes C itself unless c_prezeroed -- or, when ws_elems > 0, stores
// partials into a caller-allocated f32 workspace of that many elements and
// reduces. A workspace is only consumed by the path that sized it. The tr16
// path plans a workspace in deterministic mode only: [splitk][M0][N0] slabs
// that a second kernel sums in slice order.
struct GemmPlan {
  bool tr16;         // bf16 TN ds_read_b64_tr_b16 path (else generic tiles)
  int splitk;        // 1: no split
  int64_t ws_elems;  // f32 workspace to pass to ps_gemm_run (0: none)
  int bm, bn;        // block tile
  int kchunk;        // K per grid.z slice, a multiple of the staged K tile
  int M0, N0;        // tr16 only: interior extent (edge strips run generic)
  int ry, cx;        // generic only: 2D-XCD rectangle in tiles (0: none)
};

// What planning needs to know of a GEMM (no pointers: the caller folds
// dtype, layout and alignment eligibility into tr_ok).
struct GemmShape {
  int M, N, K;
  int esize;       // bytes per A/B element
  int bk;          // K elements per staged LDS tile of that type
  bool atomic_ok;  // atomic split-K may add into C (atomic_splitk_ok)
  bool tr_ok;      // operands can take the tr16 TN kernel at all
  bool gather_b;   // B is gathered (implicit wgrad): no edge strips
  bool nt;         // both operands K-last: the N-fitting tiles exist
  bool only128;    // A K-major x B K-last (test entry only): 128x128 only
  // deterministic mode: no plan may add into C atomically. A split takes
  // the f32 workspace + ordered reduce (ws_elems > 0), or does not happen.
  bool deterministic = false;
};

// Manual override of the tr16 tile and split-K block target, 0 = planner's
// choice. For tests (reach a tile at a shape the planner would not give it)
// and for tuning runs; never set in the training path.
struct TrTune {
  int bm, bn, target;
};

// ---------------------------------------------------------------------------
// tr16 tiles: the ONE list both the launcher (gemm.hip PS_TR_CASE) and the
// planner draw from. X(bm, bn, wave rows, wave cols); 4 waves per block, the
// per-wave sub-tile is (bm / wgm) x (bn / wgn).
// ---------------------------------------------------------------------------
#define PS_TR_TILE_LIST(X)                                                  \
  X(16, 64, 1, 4) X(16, 128, 1, 4) X(32, 64, 1, 4) X(32, 128, 1, 4)         \
  X(64, 64, 2, 2) X(64, 128, 2, 2) X(96, 128, 1, 4) X(128, 128, 2, 2)       \
  X(192, 128, 2, 2)

struct TrTile {
  int bm, bn, wgm, wgn;
};

inline const TrTile* ps_tr_tile(int bm, int bn) {
#define PS_TR_ROW(BM_, BN_, WGM_, WGN_) {BM_, BN_, WGM_, WGN_},
  static const TrTile tiles[] = {PS_TR_TILE_LIST(PS_TR_ROW)};
#undef PS_TR_ROW
  for (const TrTile& t : tiles)
    if (t.bm == bm && t.bn == bn) return &t;
  return nullptr;
}

// split-K workspaces (generic and tr16) stay under this many bytes
constexpr int64_t PS_WS_CAP_BYTES = 256LL << 20;

constexpr int PS_TR_BK = 64;                 // k rows per staged tile
constexpr int PS_LDS_PER_CU = 160 * 1024;    // gfx950
constexpr int PS_NUM_CUS = 256;

// double-buffered [BK][bm] + [BK][bn] bf16 images
inline int ps_tr_lds_bytes(int bm, int bn) {
  return 2 * (bm + bn) * PS_TR_BK * 2;
}
// blocks per CU the split-K sizing assumes for a tile
inline int ps_tr_blocks_per_cu(int bm, int bn) {
  const int fit = PS_LDS_PER_CU / ps_tr_lds_bytes(bm, bn);
  return fit < 2 ? fit : 2;
}

// Ragged last N tile. N is a multiple of 64 but a bn = 128 grid covers
// ceil(N / 128) column tiles; a wave owns the columns
// [n0 + wn, n0 + wn + bn / wgn) and is LIVE iff they start inside N (its
// span is 32 or 64 wide and 32/64-aligned, so it never straddles N). A dead
// wave issues no fragment reads, no MFMAs and no stores, but still reaches
// every barrier. The kernel and the host test both ask this function.
PS_HD inline bool ps_tr_wave_live(int n0, int wn, int N) {
  return n0 + wn < N;
}
// The staging side of the same rule: panels wider than 64 columns are
// staged as 64-column sub-images, and sub-image i of the panel at column c0
// is staged iff it starts inside the operand's cmax columns. A live wave's
// columns always lie in a live sub-image; a dead sub-image is never read.
PS_HD inline bool ps_tr_sub_live(int c0, int i, int cmax) {
  return c0 + 64 * i < cmax;
}

// Tile selection shared by the generic launcher (grid) and the split-K
// plan. Cost model: MFMA time on the PADDED output plus LDS staging traffic
// (each A panel is re-staged once per N-tile and vice versa). ALPHA ~= MACs
// the matrix cores retire per element the memory system delivers (bf16:
// ~1.25e15 MAC/s vs ~3.2e12 elem/s -> ~400).
// `narrow` (both operands K-last, the only layout they are built for) adds
// the N-fitting tiles 128x96 (2x2 waves of 64x48) and 128x48 (4x1 waves of
// 32x48). They are taken only where they cut the padded N of the best
// square-menu tile -- N = 48 / 96 / 192 and their neighbours, where a 128- or
// 64-column tile idles a quarter of its MFMAs -- not wherever the staging
// term alone would prefer them (N = 64 stays on 64x64).
//
// The ONE list of generic tiles: the candidates below, in this order, and
// the launcher's dispatch (gemm.hip) are both generated from it.
// X(bm, bn, wave rows, wave cols, narrow-only). The narrow-only tiles come
// last: they are judged against the best tile before them.
#define PS_GEMM_TILE_LIST(X)                                                \
  X(128, 128, 2, 2, false) X(128, 32, 4, 1, false) X(32, 128, 1, 4, false)  \
  X(64, 64, 2, 2, false) X(128, 16, 4, 1, false) X(16, 128, 1, 4, false)    \
  X(128, 96, 2, 2, true) X(128, 48, 4, 1, true)

struct GemmTile {
  int bm, bn, wgm, wgn;
  bool narrow_only;
};

inline const GemmTile* ps_gemm_tiles(int* count) {
#define PS_GEMM_ROW(BM_, BN_, WGM_, WGN_, NARROW_) \
  {BM_, BN_, WGM_, WGN_, NARROW_},
  static const GemmTile tiles[] = {PS_GEMM_TILE_LIST(PS_GEMM_ROW)};
#undef PS_GEMM_ROW
  *count = (int)(sizeof(tiles) / sizeof(tiles[0]));
  return tiles;
}

inline const GemmTile* ps_gemm_tile(int bm, int bn) {
  int n;
  const GemmTile* tiles = ps_gemm_tiles(&n);
  for (int i = 0; i < n; ++i)
    if (tiles[i].bm == bm && tiles[i].bn == bn) return &tiles[i];
  return nullptr;
}

inline void pick_gemm_tile(int M, int N, int* bm_out, int* bn_out,
                           bool narrow) {
  int n;
  const GemmTile* tiles = ps_gemm_tiles(&n);
  const double ALPHA = 400.0;
  double best = -1.0;
  int64_t best_npad = 0;
  for (int i = 0; i < n; ++i) {
    const int bm = tiles[i].bm, bn = tiles[i].bn;
    int64_t tm = (M + bm - 1) / bm, tn = (N + bn - 1) / bn;
    double flops = (double)(tm * bm) * (tn * bn) / ALPHA;  // (x K, common)
    double staging = (double)tm * bm * tn + (double)tn * bn * tm;
    double cost = flops + staging;
    if (tiles[i].narrow_only && (!narrow || tn * bn >= best_npad)) continue;
    if (best < 0 || cost < best) {
      best = cost;
      best_npad = tn * bn;
      *bm_out = bm;
      *bn_out = bn;
    }
  }
}

// Row tile of the tr16 path for an interior of M0 rows (M0 % 16 == 0; no
// ragged M tile, so bm divides M0). Prefers the tallest tile: per 32-deep
// k-step a wave reads (FM + FN) fragments for FM * FN MFMAs, and the LDS
// array delivers a fragment in about the time the SIMD retires one MFMA, so
// 32x32 per wave (4 : 4) leaves the reads exposed where 64x64 (8 : 16) and
// 96x64 (10 : 24) hide them; the staged bytes per flop halve as well.
// 96 rows (1x4 waves, 96x32 each, 8 : 12) serve M0 = 96, 288, ...: one row
// tile instead of three re-reads of B (AlexNet conv1's 595 MB colT).
inline int ps_tr_pick_bm(int M0) {
  if (M0 % 128 == 0) return 128;
  if (M0 % 192 == 0) return 192;
  if (M0 % 64 == 0) return 64;
  if (M0 % 96 == 0) return 96;
  return M0 % 32 ? 16 : 32;
}
// the tile every shape got before the 96/128/192-row tiles existed; still
// the fallback when the tall tile cannot fill the chip (see ps_tn_tr_plan)
inline int ps_tr_small_bm(int M0) {
  return M0 % 64 ? (M0 % 32 ? 16 : 32) : 64;
}

inline int64_t ps_tr_tiles(int M0, int N0, int bm, int bn) {
  return (int64_t)(M0 / bm) * ((N0 + bn - 1) / bn);
}

// Split-K depth of a tall tile (64-80 KB of LDS: exactly 2 blocks per CU).
// The kernel places all nbx column tiles of one (by, bz) group on ONE XCD
// (they share an A slice through its L2) and deals the groups round-robin
// over the 8 XCDs, so the unit of residency is the XCD: 32 CUs x 2 = 64
// blocks. One group more than fits and that XCD runs a second, nearly
// empty wave while the other seven idle -- measured +35..55 % per launch
// (AlexNet conv2: 480 blocks 270 us, 510 blocks 421 us). So: the deepest
// split whose groups still fit their XCD at once, ceil(nby * sk / 8) * nbx
// <= 64. Wider rows of tiles than an XCD holds (nbx > 64) fall back to
// filling the chip once by count.
// The 128- and 192-row tiles also keep K slices of at least PS_TR_TALL_KMIN:
// a block ends in bm x bn f32 atomics (64-96 KB at the chip's ~1.3 TB/s of
// atomic adds, ~5 GB/s per CU), which cost as much as ~800 k-rows of its
// MFMAs. Measured on GoogLeNet's wgrads against the 64-row tile: slices of
// 256-448 lose (192x1152: 55.6 vs 38.7 us, 128x896: 35.8 vs 29.1,
// 256x1152: 30.5 vs 23.1), slices of 1088 and up win (192x576: 63 vs 81 us;
// AlexNet conv4/5 at 1408). The 96-row tile replaces 32-row tiles and wins
// at 384-448 already (96x832: 28.3 vs 29.7 us, 288x1344: 26.2 vs 31.8).
constexpr int PS_TR_TALL_KMIN = 1024;
inline int64_t ps_tr_tall_splitk(int M0, int N0, int K, int bm, int bn) {
  const int nbx = (N0 + bn - 1) / bn, nby = M0 / bm;
  const int slots = PS_NUM_CUS / 8 * ps_tr_blocks_per_cu(bm, bn);
  const int gpx = slots / nbx;  // groups an XCD holds at once
  int64_t sk = gpx >= 1 ? (int64_t)8 * gpx / nby
                        : (int64_t)8 * slots / ((int64_t)nbx * nby);
  if (bm != 96 && sk > K / PS_TR_TALL_KMIN) sk = K / PS_TR_TALL_KMIN;
  return sk < 1 ? 1 : sk;
}

// Shape plan for the tr16 TN path. Returns false if the generic path must
// run; fills the interior [M0 x N0] (edge strips go through the generic
// kernel), tile (bm, bn) and split-K for the interior.
inline bool ps_tn_tr_plan(const GemmShape& g, const TrTune& tune,
                          GemmPlan* p) {
  if (!g.tr_ok || g.K % 64) return false;
  const int M0 = g.M & ~15, N0 = g.N & ~63;
  if (M0 == 0 || N0 == 0) return false;
  if (g.gather_b && (M0 != g.M || N0 != g.N)) return false;
  if ((M0 != g.M || N0 != g.N) && (int64_t)M0 * N0 * g.K < (1LL << 33))
    return false;
  // path choice is made on the small tile's grid, as it always was: the
  // tall tiles change how a tr16 GEMM runs, not which GEMMs are tr16
  const int sbm = ps_tr_small_bm(M0);
  if (ps_tr_tiles(M0, N0, sbm, N0 % 128 == 0 ? 128 : 64) >= 1024)
    return false;
  // The small tiles take 128 columns only where they divide N0. Running
  // them ragged was measured and never won: 64x576x1.6M (VGG conv1_2)
  // 381.5 us against 383.3 at bn = 64, GoogLeNet's 64x192 56.7 against
  // 50.0 us, 320x1472 27.0 against 24.2, 96x192 13.6 against 10.6 -- the
  // dead half of the last tile idles two of four waves.
  const int sbn = N0 % 128 == 0 ? 128 : 64;
  int bn = sbn;
  int bm = ps_tr_pick_bm(M0);
  const bool can_split = g.K >= 512 && g.atomic_ok;
  const int64_t maxsk = (g.K + 255) / 256;
  if (bm > 64) bn = 128;  // tall tiles are 128 wide; N0 = 64 runs ragged
  // Fallback to the small tile: a tall tile whose grid cannot give every CU
  // a block even at its deepest split (tiny K, few tiles) trades
  // parallelism for nothing. Measured down to 288 blocks (AlexNet conv2-5,
  // profiles/wgrad_tr16_tiles.md) the tall tile still beats the small one.
  if (bm > 64) {
    const int64_t sk = can_split ? ps_tr_tall_splitk(M0, N0, g.K, bm, bn) : 1;
    if (ps_tr_tiles(M0, N0, bm, bn) * (sk < maxsk ? sk : maxsk) < PS_NUM_CUS)
      bm = sbm, bn = sbn;
  }
  if (tune.bm > 0 && tune.bn > 0 && ps_tr_tile(tune.bm, tune.bn) &&
      M0 % tune.bm == 0 && N0 >= tune.bn / 2) {
    bm = tune.bm;
    bn = tune.bn;
  }
  if (!ps_tr_tile(bm, bn)) return false;
  const int64_t tiles = ps_tr_tiles(M0, N0, bm, bn);
  int sk = 1, kchunk = g.K;
  if (tiles < 384 && can_split) {
    int64_t want;
    if (tune.target > 0)
      want = tune.target / tiles;
    else if (bm > 64)
      want = ps_tr_tall_splitk(M0, N0, g.K, bm, bn);
    else  // the small tiles keep the historical 512-block round-up
      want = (512 + tiles - 1) / tiles;
    sk = (int)(want < maxsk ? want : maxsk);
    if (sk < 1) sk = 1;
    kchunk = ((g.K / sk + 63) / 64) * 64;
    // A-slice residency: tiles of one (by,bz) group share a bm x kchunk
    // A slice via their XCD's 4 MiB L2 -- keep it under ~2 MiB so the
    // NT-streamed B tiles have room to pass through without evicting it
    const int kcap = ((2 << 20) / (bm * 2) / 64) * 64;
    if (M0 == bm && kchunk > kcap && g.K > kcap) kchunk = kcap;
    sk = (g.K + kchunk - 1) / kchunk;
  }
  // Deterministic mode: the same split, but every slice stores its partial
  // into slab bz of a [sk][M0][N0] workspace and a reduce kernel sums the
  // slabs in order. The depth is the atomic plan's: a block's epilogue moves
  // the same bm x bn floats either way, so the reasoning behind
  // PS_TR_TALL_KMIN carries over, and the reduce reads sk * M0 * N0 floats
  // once. Only the workspace cap can shrink it; sk = ceil(K / kchunk) keeps
  // every slice non-empty.
  int64_t ws_elems = 0;
  if (g.deterministic && sk > 1) {
    const int64_t slab = (int64_t)M0 * N0;
    const int64_t fit = PS_WS_CAP_BYTES / 4 / slab;
    if (sk > fit) {
      const int64_t want = fit < 1 ? 1 : fit;
      kchunk = (int)(((g.K + want - 1) / want + 63) / 64 * 64);
      sk = (g.K + kchunk - 1) / kchunk;
    }
    if (sk > 1) ws_elems = sk * slab;
    else kchunk = g.K;
  }
  *p = {true, sk, ws_elems, bm, bn, kchunk, M0, N0, 0, 0};
  return true;
}

// grid.z of a split tr16 launch: padded until nby * skz % 8 == 0, which
// enables the kernel's (by, bz) -> XCD clustering; padded bz blocks exit
inline int ps_tr_grid_z(const GemmPlan& p) {
  int skz = p.splitk;
  if (skz > 1) {
    const int nby = p.M0 / p.bm;
    while (((int64_t)nby * skz) & 7) ++skz;
  }
  return skz;
}

// 2D XCD super-tiling for re-read-bound grids (small K, many tiles -- the
// fc-wgrad class: fc6 dW is 4096x9216x256, each A panel re-read by 72 tile
// columns and each B panel by 32 rows from HBM/L3). Each XCD owns an ry x cx
// RECTANGLE of tiles whose A+B panels fit its 4 MiB L2 (3 MiB budget), so
// panel re-reads inside the rectangle are L2 hits. Unsplit grids of at least
// 512 full tiles with K <= 1024 only. Picks (ry, cx) with ry | nby,
// cx | nbx and (nby/ry)*(nbx/cx) == 8, minimizing the L2 working set
// ry*bm + cx*bn (K common factor); leaves (0, 0) when nothing fits.
inline void ps_pick_xcd_rect(const GemmShape& g, GemmPlan* p) {
  p->ry = p->cx = 0;
  if (p->splitk > 1 || g.K > 1024 || g.M % p->bm || g.N % p->bn) return;
  const int nby = g.M / p->bm, nbx = g.N / p->bn;
  if ((int64_t)nby * nbx < 512) return;
  int64_t best = -1;
  for (int gy = 1; gy <= 8; gy <<= 1) {
    const int gx = 8 / gy;
    if (nby % gy || nbx % gx) continue;
    const int ry = nby / gy, cx = nbx / gx;
    const int64_t ws_bytes =
        ((int64_t)ry * p->bm + (int64_t)cx * p->bn) * g.K * g.esize;
    if (ws_bytes > (3LL << 20)) continue;  // must fit the 4 MiB L2
    if (best < 0 || ws_bytes < best) {
      best = ws_bytes;
      p->ry = ry;
      p->cx = cx;
    }
  }
}

// Generic path, every launch decision: tile, split-K, K slice, rectangle.
// Splits K when the output tile grid cannot fill 256 CUs but K is deep (conv
// wgrad: M=Cout, N=Kcol, K=N*OH*OW up to ~800k). 2 blocks/CU resident ->
// ~512 workgroups fill the chip; split K until the grid gets there (wgrad
// at 512x4608 is 144 tiles = 28% occupancy without). may_split = false
// plans an unsplit sub-problem (the tr16 edge strips).
// kchunk rounds the slice up to whole staged tiles, so the last slices of a
// deep split can be EMPTY (K < splitk * (splitk - 1) * bk, e.g. bf16
// 128x128x200000 on 512 slices); the kernel adds zeros for those.
inline void ps_generic_plan(const GemmShape& g, GemmPlan* p,
                            bool may_split = true) {
  *p = {false, 1, 0, 0, 0, 0, 0, 0, 0, 0};
  pick_gemm_tile(g.M, g.N, &p->bm, &p->bn, g.nt);
  const int64_t tiles =
      (int64_t)((g.M + p->bm - 1) / p->bm) * ((g.N + p->bn - 1) / p->bn);
  const bool thin = may_split && tiles < 384;
  // deterministic mode: as if C could not take atomics -- deep-K shapes take
  // the workspace branch below, the rest run unsplit
  if (thin && g.atomic_ok && !g.deterministic && g.K >= 512) {
    // atomic split-K: no workspace, so split much deeper (chunk >= 256)
    // -- the un-split grid leaves most of the 256 CUs idle
    const int64_t a = (512 + tiles - 1) / tiles, b = (g.K + 255) / 256;
    int sk = (int)(a < b ? a : b);
    if (sk > 1) p->splitk = sk;
  } else if (thin && g.K >= 4096) {
    // workspace split-K + reduce; cap the f32 workspace at 256 MB
    const int64_t a = (512 + tiles - 1) / tiles, b = (g.K + 2047) / 2048;
    int sk = (int)(a < b ? a : b);
    int64_t ws_elems = (int64_t)sk * g.M * g.N;
    if (sk > 1 && ws_elems * 4 <= PS_WS_CAP_BYTES) {
      p->splitk = sk;
      p->ws_elems = ws_elems;
    }
  }
  // built for 128x128 alone; its split is sized on the menu's tile above,
  // as it always was
  if (g.only128) p->bm = p->bn = 128;
  const int slice = (g.K + p->splitk - 1) / p->splitk;
  p->kchunk = (slice + g.bk - 1) / g.bk * g.bk;
  ps_pick_xcd_rect(g, p);
}

// ---------------------------------------------------------------------------
// Block-index remaps. The hardware dispatcher places linear block l on XCD
// l % 8, each with a private 4 MiB L2. Every remap is a PERMUTATION of its
// launch grid (tests/gemm_plan_host.cpp enumerates them); the kernels call
// the same functions with gridDim / blockIdx.
// ---------------------------------------------------------------------------
struct GemmBlock {
  int bx, by, bz;
};

// T1 XCD-aware swizzle: consecutive tiles share A/B panels, so give each XCD
// a CONTIGUOUS run of tiles instead of a round-robin comb. Bijective only
// when the flattened grid is a multiple of 8 -- identity otherwise. z (the
// split-K slice) folds into the flatten so the remap stays a permutation of
// the whole grid.
PS_HD inline GemmBlock ps_remap_linear(int nbx, int nby, int nbz, int bx,
                                       int by, int bz) {
  const int64_t nwg = (int64_t)nbx * nby * nbz;
  if ((nwg & 7) == 0 && nwg > 8) {
    int64_t id = ((int64_t)bz * nby + by) * nbx + bx;
    const int64_t cpx = nwg >> 3;
    id = (id & 7) * cpx + (id >> 3);
    bx = (int)(id % nbx);
    by = (int)((id / nbx) % nby);
    bz = (int)(id / ((int64_t)nbx * nby));
  }
  return {bx, by, bz};
}

// The planned rectangle (ps_pick_xcd_rect): XCD k owns rectangle k, and its
// j-th block takes the rectangle's j-th tile, row-major. Needs nby % ry == 0,
// nbx % cx == 0, (nby/ry)*(nbx/cx) == 8 and grid.z == 1.
PS_HD inline GemmBlock ps_remap_rect(int nbx, int ry, int cx, int bx,
                                     int by) {
  const int regs_x = nbx / cx;
  const int64_t l = (int64_t)by * nbx + bx;
  const int k = (int)(l & 7);
  const int64_t j = l >> 3;
  return {(k % regs_x) * cx + (int)(j % cx), (k / regs_x) * ry + (int)(j / cx),
          0};
}

// tr16 L2-reuse placement: all nbx tiles of one (by, bz) group -- they
// stage the SAME A k-slice (bm x kchunk, a few MB) -- land on ONE XCD so
// the re-reads hit that XCD's 4 MiB L2 (34.5 TB/s aggregate) instead of
// HBM: group g goes to XCD g % 8 and its tiles get consecutive slots there.
// Split launches whose nby * nbz is a multiple of 8 only (ps_tr_grid_z pads
// grid.z until it is; padded bz blocks have no K slice and exit); every
// other grid takes the linear swizzle.
PS_HD inline GemmBlock ps_remap_tr(bool splitk, int nbx, int nby, int nbz,
                                   int bx, int by, int bz) {
  const int64_t G = (int64_t)nby * nbz;  // (by, bz) groups
  if (!(splitk && (G & 7) == 0 && G >= 8))
    return ps_remap_linear(nbx, nby, nbz, bx, by, bz);
  const int64_t l = ((int64_t)bz * nby + by) * nbx + bx;
  const int xcd = (int)(l & 7);
  const int64_t j = l >> 3;
  const int g2 = (int)((j / nbx) * 8 + xcd);
  return {(int)(j % nbx), g2 % nby, g2 / nby};
}

