// Host check of the GEMM planner (ps_gemm_plan.h, the header gemm.hip plans
// and launches from): sweeps shapes through ps_tn_tr_plan and checks every
// invariant the tr16 TN kernel relies on, including the ragged last N
// tile's column ownership, emulated with the same ps_tr_wave_live /
// ps_tr_sub_live the kernel calls. Stand-alone: no HIP, no torch.
#include <algorithm>
#include <cstdio>
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

static GemmShape shape(int M, int N, int K, bool gather) {
  return {M, N, K, 1, /*atomic_ok=*/true, /*tr_ok=*/true, gather};
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
  // column ownership over the launch grid: grid.x = ceil(N0 / bn)
  const int nbx = (p.N0 + p.bn - 1) / p.bn, wcols = p.bn / t->wgn;
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
            CHECK(!p.tr16, "generic plan marked tr16");
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

  if (g_fail) {
    std::printf("%d gemm-plan host checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("all gemm-plan host checks passed\n");
  return 0;
}
