// Host check of the skinny split-K plans (ps_gemm_plan.h, ps_skinny_plan):
// thin tile grids at batch-sized M whose C cannot take atomics. Every such
// plan covers K exactly once with whole staged tiles and no empty slice,
// keeps its slices at the floor, its grid within the block slots and its
// workspace under the cap; every other plan -- not thin, M above the skinny
// bound, atomic-capable C, deterministic mode, the 128x128-only layout, the
// switch off -- is what the header gave before the skinny plans existed (a
// dozen of those pinned as data). No GPU needed.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

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

// layout: 0 both K-last (nt), 1 A K-last x B K-major, 2 A K-major x B K-last
// (128x128 only), 3 both K-major. kmin: the skinny switch as gemm.hip sets it
// (0 where A is K-major).
static GemmShape gshape(int M, int N, int K, int layout, int esize,
                        bool atomic_ok, int kmin) {
  GemmShape g = {M, N, K, esize, /*bk=*/esize == 2 ? 64 : 16, atomic_ok,
                 /*tr_ok=*/false, /*gather_b=*/false, layout == 0,
                 layout == 2};
  g.skinny_kmin = layout <= 1 ? kmin : 0;
  return g;
}

static bool same_plan(const GemmPlan& a, const GemmPlan& b) {
  return a.tr16 == b.tr16 && a.splitk == b.splitk &&
         a.ws_elems == b.ws_elems && a.bm == b.bm && a.bn == b.bn &&
         a.kchunk == b.kchunk && a.M0 == b.M0 && a.N0 == b.N0 &&
         a.ry == b.ry && a.cx == b.cx && a.skinny == b.skinny;
}

static long g_skinny = 0, g_split = 0, g_small_tile = 0, g_short_k = 0;

// does the skinny plan own this shape?
static bool skinny_applies(const GemmShape& g) {
  int bm = 128, bn = 128;
  pick_gemm_tile(g.M, g.N, &bm, &bn, g.nt);
  const int64_t tiles =
      (int64_t)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn);
  return tiles < 384 && g.skinny_kmin > 0 && !g.atomic_ok &&
         !g.deterministic && !g.only128 && g.M <= PS_SKINNY_MAX_M;
}

static void check_skinny(const GemmShape& g, const GemmPlan& p) {
  const int M = g.M, N = g.N, K = g.K;
  ++g_skinny;
  const GemmTile* t = ps_gemm_tile(p.bm, p.bn);
  CHECK(t && (!t->narrow_only || g.nt), "%dx%dx%d: tile %dx%d", M, N, K, p.bm,
        p.bn);
  // an unsplit 64x64 grid of 512 tiles may take the 2D-XCD rectangle
  CHECK(!p.tr16 && p.splitk >= 1 &&
            ((p.ry == 0 && p.cx == 0) || (p.splitk == 1 && K <= 1024)),
        "%dx%dx%d: tr16 %d rectangle %dx%d split %d", M, N, K, p.tr16, p.ry,
        p.cx, p.splitk);
  // slices cover K exactly once: whole staged tiles, the last one not empty
  CHECK(p.kchunk > 0 && p.kchunk % g.bk == 0, "%dx%dx%d: kchunk %d", M, N, K,
        p.kchunk);
  CHECK((int64_t)p.splitk * p.kchunk >= K &&
            (int64_t)(p.splitk - 1) * p.kchunk < K,
        "%dx%dx%d: %d slices of %d", M, N, K, p.splitk, p.kchunk);
  const int64_t tiles =
      (int64_t)((M + p.bm - 1) / p.bm) * ((N + p.bn - 1) / p.bn);
  CHECK(p.skinny, "%dx%dx%d: not marked skinny", M, N, K);
  if (p.splitk > 1) {
    ++g_split;
    g_small_tile += p.bm == 64 && p.bn == 64;
    g_short_k += K < 4096;
    CHECK(p.ws_elems == (int64_t)p.splitk * M * N &&
              p.ws_elems * 4 <= PS_WS_CAP_BYTES,
          "%dx%dx%d: workspace %lld at split %d", M, N, K,
          (long long)p.ws_elems, p.splitk);
    // the slice floor and the block slots, unless a tune forced the depth
    CHECK(g.skinny_tune.splitk > 0 ||
              (p.kchunk >= g.skinny_kmin &&
               tiles * p.splitk <= PS_SKINNY_SLOTS),
          "%dx%dx%d: split %d: slice %d under the floor %d, or %lld blocks",
          M, N, K, p.splitk, p.kchunk, g.skinny_kmin,
          (long long)(tiles * p.splitk));
  } else {
    CHECK(p.ws_elems == 0 && p.kchunk >= K,
          "%dx%dx%d: unsplit with ws %lld, kchunk %d", M, N, K,
          (long long)p.ws_elems, p.kchunk);
  }
}

int main() {
  const int Ms[] = {1, 2, 8, 16, 31, 32, 33, 64, 100, 128, 200, 256, 300, 511,
                    512};
  const int Ns[] = {8,   16,  48,   72,   96,   128,  136,  256, 384,
                    1000, 1024, 2048, 4096, 4104, 9216};
  const int Ks[] = {64,   100,  256,  511,  512,  1000, 1024, 1536, 2112,
                    3000, 4096, 4608, 9216, 12544, 25088};
  const int kmins[] = {256, 512, 1024, 2048};
  for (int M : Ms)
    for (int N : Ns)
      for (int K : Ks)
        for (int layout = 0; layout < 4; ++layout)
          for (int esize = 2; esize <= 4; esize += 2)
            for (int atomic = 0; atomic < 2; ++atomic)
              for (int det = 0; det < 2; ++det)
                for (int kmin : kmins) {
                  GemmShape g = gshape(M, N, K, layout, esize, atomic, kmin);
                  g.deterministic = det;
                  GemmShape off = g;
                  off.skinny_kmin = 0;
                  GemmPlan p, q;
                  ps_generic_plan(g, &p);
                  ps_generic_plan(off, &q);
                  if (skinny_applies(g)) {
                    check_skinny(g, p);
                  } else {
                    CHECK(same_plan(p, q) && !p.skinny,
                          "%dx%dx%d layout %d: plan moved with the switch", M,
                          N, K, layout);
                  }
                  // an unsplit sub-problem never takes the skinny plan
                  GemmPlan u;
                  ps_generic_plan(g, &u, /*may_split=*/false);
                  CHECK(u.splitk == 1 && !u.skinny && u.ws_elems == 0,
                        "%dx%dx%d: unsplit plan split %d", M, N, K, u.splitk);
                }
  // M above the bound, and grids that are not thin, keep their plans
  for (int M : {513, 1024, 6272, 43264})
    for (int N : {128, 512, 4096})
      for (int K : {1024, 4608, 9216}) {
        GemmShape g = gshape(M, N, K, 0, 2, false, PS_SKINNY_KMIN);
        GemmPlan p, q;
        ps_generic_plan(g, &p);
        g.skinny_kmin = 0;
        ps_generic_plan(g, &q);
        CHECK(same_plan(p, q) && !p.skinny, "%dx%dx%d: plan moved", M, N, K);
      }
  CHECK(g_skinny > 10000 && g_split > 3000 && g_small_tile > 100 &&
            g_short_k > 500,
        "sweep: %ld skinny plans, %ld split, %ld on 64x64, %ld with K < 4096",
        g_skinny, g_split, g_small_tile, g_short_k);

  // ---- the plans of the fc GEMMs this was built for (default floor)
  {
    struct Fc {
      const char* name;
      int M, N, K, layout, bm, bn, splitk, kchunk;
    };
    const Fc fcs[] = {
        {"alexnet fc6 fwd", 256, 4096, 9216, 0, 128, 128, 8, 1152},
        {"alexnet fc7 fwd", 256, 4096, 4096, 0, 128, 128, 8, 512},
        {"alexnet fc8 fwd", 256, 1000, 4096, 0, 64, 64, 8, 512},
        {"alexnet fc6 dx", 256, 9216, 4096, 1, 128, 128, 3, 1408},
        {"alexnet fc7 dx", 256, 4096, 4096, 1, 128, 128, 8, 512},
        {"alexnet fc8 dx", 256, 4096, 1000, 1, 64, 64, 2, 512},
        {"vgg16 fc7 fwd", 32, 4096, 4096, 0, 32, 128, 8, 512},
    };
    for (const Fc& q : fcs) {
      const GemmShape g =
          gshape(q.M, q.N, q.K, q.layout, 2, false, PS_SKINNY_KMIN);
      GemmPlan p;
      ps_generic_plan(g, &p);
      check_skinny(g, p);
      CHECK(p.bm == q.bm && p.bn == q.bn && p.splitk == q.splitk &&
                p.kchunk == q.kchunk,
            "%s: tile %dx%d split %d kchunk %d", q.name, p.bm, p.bn, p.splitk,
            p.kchunk);
    }
  }

  // ---- a forced depth is rounded to one without an empty slice: 2112 = 33
  // staged bf16 tiles on 8 slices is 5 tiles each, so 7 slices (the last of
  // 3 tiles), not 8 with an empty one
  {
    GemmShape g = gshape(32, 256, 2112, 0, 2, false, PS_SKINNY_KMIN);
    g.skinny_tune = {0, 0, 8};
    GemmPlan p;
    ps_generic_plan(g, &p);
    check_skinny(g, p);
    CHECK(p.splitk == 7 && p.kchunk == 320, "32x256x2112 at 8: %d x %d",
          p.splitk, p.kchunk);
    // K = 1000 on 6: ceil(1000 / 6) = 167 -> 192 per slice, the last 40
    g = gshape(8, 72, 1000, 1, 2, false, PS_SKINNY_KMIN);
    g.skinny_tune = {64, 64, 6};
    ps_generic_plan(g, &p);
    check_skinny(g, p);
    CHECK(p.splitk == 6 && p.kchunk == 192 && p.bm == 64 && p.bn == 64,
          "8x72x1000 at 6: %dx%d, %d x %d", p.bm, p.bn, p.splitk, p.kchunk);
    // unforced, K = 1000 makes two slices of 512 as staged (the floor)
    g.skinny_tune = {0, 0, 0};
    ps_generic_plan(g, &p);
    check_skinny(g, p);
    CHECK(p.splitk == 2 && p.kchunk == 512, "8x72x1000: %d x %d", p.splitk,
          p.kchunk);
    // a depth whose workspace would pass the cap is not taken
    g = gshape(512, 9216, 25088, 0, 2, false, PS_SKINNY_KMIN);
    g.skinny_tune = {0, 0, 32};
    ps_generic_plan(g, &p);
    CHECK(p.ws_elems * 4 <= PS_WS_CAP_BYTES, "cap: %lld",
          (long long)p.ws_elems);
  }

  // ---- pinned: plans the skinny planner must NOT touch, as the header gave
  // them before it existed (switch on, default floor). layout as in gshape.
  {
    struct Pin {
      const char* name;
      int M, N, K, layout, esize;
      bool atomic, det;
      int bm, bn, splitk;
      long long ws;
      int kchunk, ry, cx;
    };
    const Pin pins[] = {
        {"vgg conv5 fwd", 6272, 512, 4608, 0, 2, false, false, 128, 128, 3, 9633792, 1536, 0, 0},
        {"alexnet conv2 fwd", 186624, 128, 1200, 0, 2, false, false, 128, 128, 1, 0, 1216, 0, 0},
        {"1024x4096x4096 fwd, M over the bound", 1024, 4096, 4096, 0, 2, false, false, 128, 128, 2, 8388608, 2048, 0, 0},
        {"alexnet fc6 fwd, deterministic", 256, 4096, 9216, 0, 2, false, true, 128, 128, 5, 5242880, 1856, 0, 0},
        {"alexnet fc8 fwd, deterministic", 256, 1000, 4096, 0, 2, false, true, 128, 128, 2, 512000, 2048, 0, 0},
        {"alexnet fc7 dx, deterministic", 256, 4096, 4096, 1, 2, false, true, 128, 128, 2, 2097152, 2048, 0, 0},
        {"fc7 dx f32, atomic C", 256, 4096, 4096, 1, 4, true, false, 128, 128, 8, 0, 512, 0, 0},
        {"fc8 dx f32, atomic C", 256, 4096, 1000, 1, 4, true, false, 128, 128, 4, 0, 256, 0, 0},
        {"alexnet fc6 dW f32", 4096, 9216, 256, 3, 4, true, false, 128, 128, 1, 0, 256, 0, 0},
        {"googlenet 5b 1x1 wgrad", 128, 832, 1568, 3, 2, true, false, 128, 128, 7, 0, 256, 0, 0},
        {"256x4096x9216, A K-major x B K-last", 256, 4096, 9216, 2, 2, false, false, 128, 128, 5, 5242880, 1856, 0, 0},
        {"256x4096x9216, both K-major", 256, 4096, 9216, 3, 2, false, false, 128, 128, 5, 5242880, 1856, 0, 0},
        {"64x32768x64", 64, 32768, 64, 0, 2, true, false, 64, 64, 1, 0, 64, 1, 64},
    };
    for (const Pin& q : pins) {
      GemmShape g =
          gshape(q.M, q.N, q.K, q.layout, q.esize, q.atomic, PS_SKINNY_KMIN);
      g.deterministic = q.det;
      GemmPlan p;
      ps_generic_plan(g, &p);
      CHECK(p.bm == q.bm && p.bn == q.bn && p.splitk == q.splitk &&
                p.ws_elems == q.ws && p.kchunk == q.kchunk && p.ry == q.ry &&
                p.cx == q.cx && !p.skinny,
            "%s: tile %dx%d split %d ws %lld kchunk %d rectangle %dx%d",
            q.name, p.bm, p.bn, p.splitk, (long long)p.ws_elems, p.kchunk,
            p.ry, p.cx);
    }
  }

  if (g_fail) {
    std::printf("%d skinny-plan host checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("all skinny-plan host checks passed\n");
  return 0;
}
