// Host check of the GEMM planner (ps_gemm_plan.h, the header gemm.hip plans
// and launches from): sweeps shapes through ps_tn_tr_plan and checks every
// invariant the tr16 TN kernel relies on, including the ragged last N
// tile's column ownership, emulated with the same ps_tr_wave_live /
// ps_tr_sub_live the kernel calls. Then the generic planner: a sweep of
// ps_generic_plan over layouts, element sizes and shapes, every invariant of
// a generic launch, and pinned decisions of model GEMMs. And the block-index
// remaps both kernels call (ps_remap_linear / _rect / _tr): each enumerated
// over planned and hand-picked grids and checked to be a permutation that
// places blocks on XCDs as documented. Stand-alone: no HIP, no torch.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "ps_gemm_plan.h"

static int g_fail = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (++g_fail <= 20) {                       \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                 \
        std::printf("\n");                        \
      }                                           \
    }                                             \
  } while (0)

static const TrTune kAuto = {0, 0, 0};

// a bf16 K-major x K-major GEMM that may take tr16
static GemmShape shape(int M, int N, int K, bool gather) {
  return {M, N, K, /*esize=*/2, /*bk=*/64, /*atomic_ok=*/true,
          /*tr_ok=*/true, gather, /*nt=*/false, /*only128=*/false};
}

// a GEMM for the generic path. layout: 0 both K-last (nt), 1 A K-last x B
// K-major, 2 A K-major x B K-last (128x128 only), 3 both K-major
static GemmShape gshape(int M, int N, int K, int layout, int esize,
                        bool atomic_ok) {
  return {M, N, K, esize, /*bk=*/esize == 2 ? 64 : 16, atomic_ok,
          /*tr_ok=*/false, /*gather_b=*/false, layout == 0, layout == 2};
}

// ---------------------------------------------------------------------------
// block-index remaps: each is a permutation of its launch grid
// ---------------------------------------------------------------------------
static std::vector<int> g_hits;

static int tile_id(const GemmBlock& t, int nbx, int nby, int nbz) {
  if (t.bx < 0 || t.bx >= nbx || t.by < 0 || t.by >= nby || t.bz < 0 ||
      t.bz >= nbz)
    return -1;
  return (t.bz * nby + t.by) * nbx + t.bx;
}

static void check_hit_once(const char* what, int nbx, int nby, int nbz) {
  for (size_t i = 0; i < g_hits.size(); ++i)
    if (g_hits[i] != 1) {
      CHECK(false, "%s %dx%dx%d: tile %zu hit %d times", what, nbx, nby, nbz,
            i, g_hits[i]);
      return;
    }
}

// linear swizzle: identity unless the grid is a multiple of 8 above 8; then
// the blocks of XCD k (l % 8 == k) take the k-th contiguous eighth, in order
static void check_linear(int nbx, int nby, int nbz) {
  const int n = nbx * nby * nbz;
  g_hits.assign(n, 0);
  for (int bz = 0; bz < nbz; ++bz)
    for (int by = 0; by < nby; ++by)
      for (int bx = 0; bx < nbx; ++bx) {
        const int l = (bz * nby + by) * nbx + bx;
        const int id =
            tile_id(ps_remap_linear(nbx, nby, nbz, bx, by, bz), nbx, nby, nbz);
        CHECK(id >= 0, "linear %dx%dx%d: block %d out of range", nbx, nby,
              nbz, l);
        if (id < 0) return;
        ++g_hits[id];
        if (n % 8 != 0 || n <= 8)
          CHECK(id == l, "linear %dx%dx%d: not the identity", nbx, nby, nbz);
        else
          CHECK(id == (l & 7) * (n / 8) + (l >> 3),
                "linear %dx%dx%d: block %d -> tile %d", nbx, nby, nbz, l, id);
      }
  check_hit_once("linear", nbx, nby, nbz);
}

// 2D rectangle: the blocks of XCD k all land in rectangle k (ry x cx tiles)
static void check_rect(int nbx, int nby, int ry, int cx) {
  g_hits.assign(nbx * nby, 0);
  for (int by = 0; by < nby; ++by)
    for (int bx = 0; bx < nbx; ++bx) {
      const int l = by * nbx + bx;
      const GemmBlock t = ps_remap_rect(nbx, ry, cx, bx, by);
      const int id = tile_id(t, nbx, nby, 1);
      CHECK(id >= 0, "rect %dx%d (%dx%d): block %d out of range", nbx, nby,
            ry, cx, l);
      if (id < 0) return;
      ++g_hits[id];
      CHECK((t.by / ry) * (nbx / cx) + t.bx / cx == (l & 7),
            "rect %dx%d (%dx%d): block %d of XCD %d in rectangle %d", nbx,
            nby, ry, cx, l, l & 7, (t.by / ry) * (nbx / cx) + t.bx / cx);
    }
  check_hit_once("rect", nbx, nby, 1);
}

// tr16 clustering over the PADDED grid: all nbx tiles of a (by, bz) group
// come from blocks of one XCD
static void check_tr_remap(bool split, int nbx, int nby, int nbz) {
  const bool clustered = split && (nby * nbz) % 8 == 0 && nby * nbz >= 8;
  g_hits.assign(nbx * nby * nbz, 0);
  std::vector<int> xcd(nby * nbz, -1);
  for (int bz = 0; bz < nbz; ++bz)
    for (int by = 0; by < nby; ++by)
      for (int bx = 0; bx < nbx; ++bx) {
        const int l = (bz * nby + by) * nbx + bx;
        const GemmBlock t = ps_remap_tr(split, nbx, nby, nbz, bx, by, bz);
        const int id = tile_id(t, nbx, nby, nbz);
        CHECK(id >= 0, "tr %dx%dx%d: block %d out of range", nbx, nby, nbz, l);
        if (id < 0) return;
        ++g_hits[id];
        if (!clustered) continue;
        int& x = xcd[t.bz * nby + t.by];
        if (x < 0) x = l & 7;
        CHECK(x == (l & 7), "tr %dx%dx%d: group (%d, %d) on XCDs %d and %d",
              nbx, nby, nbz, t.by, t.bz, x, l & 7);
      }
  check_hit_once("tr", nbx, nby, nbz);
}

// each distinct grid once: sweeps plan the same grid many times over
static std::set<std::vector<int>> g_seen;
static bool first_time(std::vector<int> key) {
  return g_seen.insert(std::move(key)).second;
}
constexpr int64_t kMaxEnum = 1 << 16;  // blocks enumerated per grid

static long g_empty_slices = 0, g_rects = 0, g_remaps = 0;

// every invariant of one generic plan, and the remap of its launch grid
static void check_generic_plan(const GemmShape& g, const GemmPlan& p) {
  const int M = g.M, N = g.N, K = g.K;
  CHECK(!p.tr16, "generic plan marked tr16");
  const GemmTile* t = ps_gemm_tile(p.bm, p.bn);
  CHECK(t != nullptr, "%dx%dx%d: tile %dx%d is not in the list", M, N, K,
        p.bm, p.bn);
  if (!t) return;
  CHECK(t->wgm * t->wgn == 4, "tile %dx%d: not 4 waves", p.bm, p.bn);
  CHECK(!t->narrow_only || g.nt, "%dx%dx%d: N-fitting tile %dx%d off nt", M,
        N, K, p.bm, p.bn);
  CHECK(!g.only128 || (p.bm == 128 && p.bn == 128), "%dx%dx%d: tile %dx%d",
        M, N, K, p.bm, p.bn);
  CHECK(p.splitk >= 1 && p.kchunk > 0 && p.kchunk % g.bk == 0 &&
            (int64_t)p.splitk * p.kchunk >= K,
        "%dx%dx%d: splitk %d, kchunk %d, bk %d", M, N, K, p.splitk, p.kchunk,
        g.bk);
  CHECK(p.ws_elems == 0 || p.ws_elems == (int64_t)p.splitk * M * N,
        "%dx%dx%d: workspace %lld", M, N, K, (long long)p.ws_elems);
  CHECK(p.ws_elems * 4 <= (256LL << 20), "%dx%dx%d: workspace %lld", M, N, K,
        (long long)p.ws_elems);
  // a split is atomic (no workspace) exactly when C may take atomics
  if (p.splitk > 1)
    CHECK((p.ws_elems == 0) == g.atomic_ok, "%dx%dx%d: split %d, ws %lld", M,
          N, K, p.splitk, (long long)p.ws_elems);
  else
    CHECK(p.ws_elems == 0, "%dx%dx%d: unsplit with a workspace", M, N, K);
  // Planned splits CAN leave empty last slices (kchunk rounds up to whole
  // staged tiles), but only deep splits of a short K; the kernel's
  // tolerance of them stays.
  if ((int64_t)(p.splitk - 1) * p.kchunk >= K) {
    ++g_empty_slices;
    CHECK(K < (int64_t)p.splitk * (p.splitk - 1) * g.bk,
          "%dx%dx%d: empty slice at splitk %d, kchunk %d", M, N, K, p.splitk,
          p.kchunk);
  }
  const int nbx = (N + p.bn - 1) / p.bn, nby = (M + p.bm - 1) / p.bm;
  if (p.ry || p.cx) {
    ++g_rects;
    CHECK(p.ry > 0 && p.cx > 0 && p.splitk == 1 && M % p.bm == 0 &&
              N % p.bn == 0 && K <= 1024 && (int64_t)nbx * nby >= 512,
          "%dx%dx%d: rectangle %dx%d on tile %dx%d split %d", M, N, K, p.ry,
          p.cx, p.bm, p.bn, p.splitk);
    if (p.ry <= 0 || p.cx <= 0) return;
    CHECK(nby % p.ry == 0 && nbx % p.cx == 0 &&
              (nby / p.ry) * (nbx / p.cx) == 8,
          "%dx%dx%d: rectangle %dx%d in grid %dx%d", M, N, K, p.ry, p.cx, nby,
          nbx);
    CHECK(((int64_t)p.ry * p.bm + (int64_t)p.cx * p.bn) * K * g.esize <=
              (3LL << 20),
          "%dx%dx%d: rectangle %dx%d over the L2 budget", M, N, K, p.ry, p.cx);
    if ((int64_t)nbx * nby <= kMaxEnum && first_time({1, nbx, nby, p.ry, p.cx}))
      check_rect(nbx, nby, p.ry, p.cx), ++g_remaps;
  } else if ((int64_t)nbx * nby * p.splitk <= kMaxEnum &&
             first_time({0, nbx, nby, p.splitk})) {
    check_linear(nbx, nby, p.splitk), ++g_remaps;
  }
}

// every invariant of one tr16 plan
static void check_plan(const GemmShape& g, const GemmPlan& p,
                       std::vector<int>& owner) {
  const int M = g.M, N = g.N, K = g.K;
  const TrTile* t = ps_tr_tile(p.bm, p.bn);
  CHECK(t != nullptr, "%dx%dx%d: tile %dx%d is not instantiated", M, N, K,
        p.bm, p.bn);
  if (!t) return;
  CHECK(t->wgm * t->wgn == 4, "tile %dx%d: not 4 waves", p.bm, p.bn);
  CHECK(p.M0 > 0 && p.N0 > 0 && p.M0 <= M && p.N0 <= N && p.M0 % 16 == 0 &&
            p.N0 % 64 == 0,
        "%dx%dx%d: interior %dx%d", M, N, K, p.M0, p.N0);
  CHECK(p.M0 % p.bm == 0, "%dx%dx%d: bm %d does not divide M0 %d", M, N, K,
        p.bm, p.M0);
  CHECK(p.splitk >= 1 && (int64_t)p.splitk * p.kchunk >= K,
        "%dx%dx%d: splitk %d * kchunk %d < K", M, N, K, p.splitk, p.kchunk);
  CHECK((int64_t)(p.splitk - 1) * p.kchunk < K,
        "%dx%dx%d: empty last slice (splitk %d, kchunk %d)", M, N, K,
        p.splitk, p.kchunk);
  CHECK(p.kchunk % 64 == 0, "%dx%dx%d: kchunk %d", M, N, K, p.kchunk);
  CHECK(p.ws_elems == 0, "%dx%dx%d: tr16 plan with a workspace", M, N, K);
  const int bpc = ps_tr_blocks_per_cu(p.bm, p.bn);
  CHECK(bpc >= 1 && (int64_t)ps_tr_lds_bytes(p.bm, p.bn) * bpc <= 160 * 1024,
        "tile %dx%d: %d B LDS x %d blocks/CU", p.bm, p.bn,
        ps_tr_lds_bytes(p.bm, p.bn), bpc);
  if (g.gather_b)
    CHECK(p.M0 == M && p.N0 == N, "%dx%dx%d: gathered plan with edge strips",
          M, N, K);
  const int skz = ps_tr_grid_z(p);
  CHECK(skz >= p.splitk, "grid z %d < splitk %d", skz, p.splitk);
  if (p.splitk > 1)
    CHECK(((int64_t)(p.M0 / p.bm) * skz) % 8 == 0,
          "%dx%dx%d: nby*skz not a multiple of 8", M, N, K);
  // the padded bz values are exactly those without a K slice (they exit)
  for (int bz = 0; bz < skz; ++bz)
    CHECK((bz >= p.splitk) == ((int64_t)bz * p.kchunk >= K),
          "%dx%dx%d: bz %d of %d (splitk %d, kchunk %d)", M, N, K, bz, skz,
          p.splitk, p.kchunk);
  // column ownership over the launch grid: grid.x = ceil(N0 / bn)
  const int nbx = (p.N0 + p.bn - 1) / p.bn, wcols = p.bn / t->wgn;
  if ((int64_t)nbx * (p.M0 / p.bm) * skz <= kMaxEnum &&
      first_time({2, p.splitk > 1, nbx, p.M0 / p.bm, skz}))
    check_tr_remap(p.splitk > 1, nbx, p.M0 / p.bm, skz), ++g_remaps;
  owner.assign(p.N0, 0);
  for (int bx = 0; bx < nbx; ++bx) {
    const int n0 = bx * p.bn;
    for (int w = 0; w < t->wgn; ++w) {
      const int wn = w * wcols;
      if (!ps_tr_wave_live(n0, wn, p.N0)) continue;
      CHECK(n0 + wn + wcols <= p.N0,
            "%dx%dx%d tile %dx%d: live wave stores columns [%d, %d) past %d",
            M, N, K, p.bm, p.bn, n0 + wn, n0 + wn + wcols, p.N0);
      for (int c = n0 + wn; c < std::min(n0 + wn + wcols, p.N0); ++c)
        ++owner[c];
    }
    // staging: 64-column sub-images; a staged one lies inside the operand
    // and every live wave reads only staged ones
    for (int i = 0; i < p.bn / 64; ++i) {
      const bool staged = p.bn <= 64 || ps_tr_sub_live(n0, i, p.N0);
      if (staged)
        CHECK(n0 + 64 * i + 64 <= p.N0,
              "%dx%dx%d: stages columns [%d, %d) of %d", M, N, K, n0 + 64 * i,
              n0 + 64 * i + 64, p.N0);
      for (int w = 0; w < t->wgn; ++w) {
        const int wn = w * wcols;
        if (wn / 64 == i && ps_tr_wave_live(n0, wn, p.N0))
          CHECK(staged, "%dx%dx%d: live wave %d reads an unstaged sub-image",
                M, N, K, w);
      }
    }
  }
  for (int c = 0; c < p.N0; ++c)
    if (owner[c] != 1) {
      CHECK(false, "%dx%dx%d tile %dx%d: column %d owned %d times", M, N, K,
            p.bm, p.bn, c, owner[c]);
      break;
    }
}

struct Named {
  const char* name;
  int M, N, K;
  bool gather;
};

int main() {
  std::vector<int> owner;
  const int Ks[] = {64,    448,   512,    1568,   6272,
                    25088, 43264, 186624, 774400, 1605632};
  long planned = 0, tall = 0;
  for (int gather = 0; gather < 2; ++gather)
    for (int M = 16; M <= 512; M += 16)
      for (int N = 64; N <= 4608; N += 64)
        for (int K : Ks) {
          const GemmShape g = shape(M, N, K, gather != 0);
          GemmPlan p;
          if (!ps_tn_tr_plan(g, kAuto, &p)) {
            ps_generic_plan(g, &p);
            check_generic_plan(g, p);
            continue;
          }
          CHECK(p.tr16, "tr16 plan not marked");
          CHECK(p.M0 == M && p.N0 == N, "%dx%d: clean shape with strips", M,
                N);
          check_plan(g, p, owner);
          ++planned;
          tall += p.bm > 64;
        }
  CHECK(planned > 10000 && tall > 1000, "sweep reached %ld plans, %ld tall",
        planned, tall);

  // shapes off the 16 / 64 grid: strips only without a gather, and only
  // when the interior is worth a second launch
  {
    GemmPlan p;
    CHECK(!ps_tn_tr_plan(shape(100, 200, 1 << 20, true), kAuto, &p),
          "gathered plan off the 64-column grid");
    CHECK(!ps_tn_tr_plan(shape(100, 200, 4096, false), kAuto, &p),
          "small ragged shape took tr16");
    const GemmShape g = shape(100, 200, 1 << 20, false);
    CHECK(ps_tn_tr_plan(g, kAuto, &p) && p.M0 == 96 && p.N0 == 192,
          "100x200 interior");
    check_plan(g, p, owner);
    GemmShape bad = shape(128, 128, 4096, false);
    bad.tr_ok = false;
    CHECK(!ps_tn_tr_plan(bad, kAuto, &p), "ineligible operands took tr16");
    bad = shape(128, 128, 4096, false);
    bad.atomic_ok = false;
    CHECK(ps_tn_tr_plan(bad, kAuto, &p) && p.splitk == 1,
          "split-K without atomics");
  }

  // The conv weight gradients the tall tiles were built for: AlexNet at
  // batch 256 and VGG-16 at batch 32. Each gets a per-wave sub-tile of at
  // least 32x64 MFMA outputs in either orientation (conv1's 96-row tile is
  // 1x4 waves of 96x32: one row tile, so its column matrix streams once).
  // Measured exception: VGG's 64x576 (conv1_2) keeps 64x64. A ragged 64x128
  // tile measured 381.5 us against 383.3 us there, within noise, and lost
  // on every GoogLeNet shape of that kind (64x192: 56.7 against 50.0 us),
  // so the small tiles never run ragged (profiles/wgrad_tr16_tiles.md).
  const Named named[] = {
      {"alexnet conv1", 96, 384, 774400, false},
      {"alexnet conv2", 128, 1216, 186624, true},
      {"alexnet conv3", 384, 2304, 43264, true},
      {"alexnet conv4", 192, 1728, 43264, true},
      {"alexnet conv5", 128, 1728, 43264, true},
      {"vgg 64x576", 64, 576, 32 * 224 * 224, true},
      {"vgg 128x1152", 128, 1152, 32 * 112 * 112, true},
      {"vgg 256x2304", 256, 2304, 32 * 56 * 56, true},
      {"vgg 512x4608", 512, 4608, 32 * 28 * 28, true},
  };
  const int want_bm[] = {96, 128, 128, 192, 128, 64, 128, 128, 128};
  const int want_bn[] = {128, 128, 128, 128, 128, 64, 128, 128, 128};
  int i = 0;
  for (const Named& q : named) {
    const GemmShape g = shape(q.M, q.N, q.K, q.gather);
    GemmPlan p;
    const bool ok = ps_tn_tr_plan(g, kAuto, &p);
    CHECK(ok, "%s: not tr16", q.name);
    if (!ok) continue;
    check_plan(g, p, owner);
    const TrTile* t = ps_tr_tile(p.bm, p.bn);
    const int sm = p.bm / t->wgm, sn = p.bn / t->wgn;
    if (want_bn[i] == 128)
      CHECK(std::min(sm, sn) >= 32 && std::max(sm, sn) >= 64,
            "%s: per-wave sub-tile %dx%d (tile %dx%d)", q.name, sm, sn, p.bm,
            p.bn);
    CHECK(p.bm == want_bm[i] && p.bn == want_bn[i], "%s: tile %dx%d", q.name,
          p.bm, p.bn);
    // every XCD's share of the (by, bz) groups is resident at once: no
    // second, nearly empty wave on one XCD while the others idle
    if (p.bm > 64) {
      const int nbx = (p.N0 + p.bn - 1) / p.bn, nby = p.M0 / p.bm;
      const int per_xcd = (nby * p.splitk + 7) / 8 * nbx;
      CHECK(per_xcd <= PS_NUM_CUS / 8 * ps_tr_blocks_per_cu(p.bm, p.bn),
            "%s: %d blocks on one XCD", q.name, per_xcd);
      CHECK(ps_tr_tiles(p.M0, p.N0, p.bm, p.bn) * p.splitk >= PS_NUM_CUS,
            "%s: tall tile on %d slices leaves CUs idle", q.name, p.splitk);
    }
    std::printf("%-14s tile %3dx%3d splitk %3d kchunk %6d grid z %3d\n",
                q.name, p.bm, p.bn, p.splitk, p.kchunk, ps_tr_grid_z(p));
    ++i;
  }

  // tall tiles step down when even the deepest split leaves CUs idle
  {
    GemmPlan p;
    // GoogLeNet (batch 32) wgrads whose K slices would fall under
    // PS_TR_TALL_KMIN keep the 64-row plan they always had ...
    CHECK(ps_tn_tr_plan(shape(192, 1152, 25088, false), kAuto, &p) &&
              p.bm == 64 && p.bn == 128 && ps_tr_grid_z(p) == 24,
          "192x1152x25088");
    CHECK(ps_tn_tr_plan(shape(256, 1152, 6272, false), kAuto, &p) &&
              p.bm == 64 && p.bn == 128, "256x1152x6272");
    // ... deep ones and 96-row ones take the tall tile
    CHECK(ps_tn_tr_plan(shape(192, 576, 100352, false), kAuto, &p) &&
              p.bm == 192 && p.kchunk >= PS_TR_TALL_KMIN, "192x576x100352");
    CHECK(ps_tn_tr_plan(shape(96, 832, 25088, false), kAuto, &p) &&
              p.bm == 96, "96x832x25088");
    CHECK(ps_tn_tr_plan(shape(128, 128, 128, false), kAuto, &p) &&
              p.bm == 64, "128x128x128 kept the tall tile");
    // ... and the override reaches them at the GPU tests' small shapes
    const int forced[][5] = {{128, 128, 128, 128, 128}, {128, 192, 1024, 128, 128},
                             {192, 320, 1024, 192, 128}, {96, 384, 2048, 96, 128},
                             {384, 256, 4096, 128, 128}, {128, 64, 512, 128, 128}};
    for (const auto& f : forced) {
      const GemmShape g = shape(f[0], f[1], f[2], false);
      const TrTune tune = {f[3], f[4], 0};
      const bool ok = ps_tn_tr_plan(g, tune, &p);
      CHECK(ok && p.bm == f[3] && p.bn == f[4], "override %dx%d at %dx%dx%d",
            f[3], f[4], f[0], f[1], f[2]);
      if (ok) check_plan(g, p, owner);
    }
    // an override that does not fit the shape is ignored, not obeyed
    const TrTune odd = {192, 128, 0};
    CHECK(ps_tn_tr_plan(shape(128, 256, 4096, false), odd, &p) &&
              p.bm != 192, "192-row override on M = 128");
  }

  // ---- generic plans: every layout, both element sizes, with and without
  // atomics; sizes on and off every tile, thin and huge
  {
    const int Ms[] = {1,   16,  33,   64,   96,   100,  128,   192,   256, 300,
                      384, 512, 676,  1000, 2048, 4096, 8192,  25088, 802816};
    const int Ns[] = {1,   16,  32,   48,   64,   96,   100,  128,
                      192, 256, 384,  1000, 1152, 4096, 9216, 32768};
    const int Kg[] = {1,    16,   63,   64,   96,    200,    256,
                      333,  512,  576,  1024, 1040,  1200,   4096,
                      4608, 9216, 25088, 100352, 200000, 774400};
    long plans = 0, splits = 0, ws_splits = 0;
    for (int M : Ms)
      for (int N : Ns)
        for (int K : Kg)
          for (int layout = 0; layout < 4; ++layout)
            for (int esize = 2; esize <= 4; esize += 2)
              for (int atomic = 0; atomic < 2; ++atomic) {
                if ((int64_t)M * N > (1LL << 31)) continue;
                const GemmShape g = gshape(M, N, K, layout, esize, atomic);
                GemmPlan p;
                ps_generic_plan(g, &p);
                check_generic_plan(g, p);
                ++plans;
                splits += p.splitk > 1;
                ws_splits += p.ws_elems > 0;
                // an unsplit sub-problem (tr16 edge strip): same tile
                GemmPlan q;
                ps_generic_plan(g, &q, /*may_split=*/false);
                check_generic_plan(g, q);
                CHECK(q.splitk == 1 && q.bm == p.bm && q.bn == p.bn,
                      "%dx%dx%d: unsplit plan %dx%d split %d", M, N, K, q.bm,
                      q.bn, q.splitk);
              }
    CHECK(plans > 50000 && splits > 5000 && ws_splits > 1000 && g_rects > 10,
          "generic sweep: %ld plans, %ld split, %ld with a workspace, %ld "
          "rectangles", plans, splits, ws_splits, g_rects);
    // empty last slices do occur among planned splits
    GemmPlan p;
    ps_generic_plan(gshape(128, 128, 200000, 3, 2, true), &p);
    CHECK(p.splitk == 512 && p.kchunk == 448 && g_empty_slices > 0,
          "128x128x200000: splitk %d kchunk %d", p.splitk, p.kchunk);
  }

  // ---- remaps on grids no plan above gives: gridDim.z > 1, totals that are
  // not multiples of 8 (identity), 8 itself, and one block
  {
    const int grids[][3] = {{1, 1, 1}, {2, 2, 2},  {4, 2, 1}, {3, 5, 7},
                            {4, 4, 3}, {16, 1, 1}, {5, 8, 3}, {7, 9, 16},
                            {1, 1, 24}, {13, 1, 8}, {6, 10, 4}};
    for (const auto& d : grids) {
      check_linear(d[0], d[1], d[2]);
      check_tr_remap(true, d[0], d[1], d[2]);
      check_tr_remap(false, d[0], d[1], d[2]);
    }
    const int rects[][4] = {{72, 32, 16, 18}, {32, 16, 8, 8}, {512, 1, 1, 64},
                            {8, 64, 8, 8},    {1, 512, 64, 1}, {24, 40, 10, 12}};
    for (const auto& d : rects) check_rect(d[0], d[1], d[2], d[3]);
    CHECK(g_remaps > 300, "only %ld planned grids enumerated", g_remaps);
  }

  // ---- pinned decisions: what the launcher computed for these GEMMs before
  // the plan carried them (tile, split, workspace, kchunk of a split,
  // rectangle). layout as in gshape.
  {
    struct Pin {
      const char* name;
      int M, N, K, layout, esize;
      bool atomic;
      int bm, bn, splitk;
      long long ws;
      int kchunk, ry, cx;
    };
    const Pin pins[] = {
        {"alexnet conv1 fwd", 774400, 96, 384, 0, 2, false, 128, 96, 1, 0, 0, 0, 0},
        {"alexnet conv2 fwd", 186624, 128, 1200, 0, 2, false, 128, 128, 1, 0, 0, 0, 0},
        {"alexnet conv3 fwd", 43264, 384, 2304, 0, 2, false, 128, 128, 1, 0, 0, 0, 0},
        {"vgg conv1_2 fwd", 1605632, 64, 576, 0, 2, false, 64, 64, 1, 0, 0, 0, 0},
        {"vgg conv5 fwd", 6272, 512, 4608, 0, 2, false, 128, 128, 3, 9633792, 1536, 0, 0},
        {"alexnet fc6 fwd", 256, 4096, 9216, 0, 2, false, 128, 128, 5, 5242880, 1856, 0, 0},
        {"alexnet fc7 fwd", 256, 4096, 4096, 0, 2, false, 128, 128, 2, 2097152, 2048, 0, 0},
        {"alexnet fc8 fwd", 256, 1000, 4096, 0, 2, false, 128, 128, 2, 512000, 2048, 0, 0},
        {"alexnet fc6 dx", 256, 9216, 4096, 1, 2, false, 128, 128, 2, 4718592, 2048, 0, 0},
        {"alexnet fc7 dx", 256, 4096, 4096, 1, 2, false, 128, 128, 2, 2097152, 2048, 0, 0},
        {"alexnet fc8 dx", 256, 4096, 1000, 1, 2, false, 128, 128, 1, 0, 0, 0, 0},
        {"alexnet fc6 dW f32", 4096, 9216, 256, 3, 4, true, 128, 128, 1, 0, 0, 0, 0},
        // K = 32 * 7 * 7 is no multiple of 64: these miss tr16
        {"googlenet 5b 1x1 wgrad", 128, 832, 1568, 3, 2, true, 128, 128, 7, 0, 256, 0, 0},
        {"googlenet 5b 3x3 wgrad", 384, 1728, 1568, 3, 2, true, 128, 128, 7, 0, 256, 0, 0},
        {"fc6 dW class, nt bf16", 4096, 9216, 256, 0, 2, true, 128, 128, 1, 0, 0, 16, 18},
        {"2048x4096x64", 2048, 4096, 64, 0, 2, true, 128, 128, 1, 0, 0, 8, 8},
        {"64x32768x64", 64, 32768, 64, 0, 2, true, 64, 64, 1, 0, 0, 1, 64},
        // 16 blocks: linear swizzle
        {"512x512x96", 512, 512, 96, 0, 2, true, 128, 128, 1, 0, 0, 0, 0},
        {"2048x4096x64 f32", 2048, 4096, 64, 0, 4, true, 128, 128, 1, 0, 0, 8, 8},
    };
    for (const Pin& q : pins) {
      GemmPlan p;
      ps_generic_plan(gshape(q.M, q.N, q.K, q.layout, q.esize, q.atomic), &p);
      CHECK(p.bm == q.bm && p.bn == q.bn && p.splitk == q.splitk &&
                p.ws_elems == q.ws && p.ry == q.ry && p.cx == q.cx &&
                (q.splitk == 1 || p.kchunk == q.kchunk),
            "%s: tile %dx%d split %d ws %lld kchunk %d rectangle %dx%d",
            q.name, p.bm, p.bn, p.splitk, (long long)p.ws_elems, p.kchunk,
            p.ry, p.cx);
    }
  }

  if (g_fail) {
    std::printf("%d gemm-plan host checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("all gemm-plan host checks passed\n");
  return 0;
}
