// Host-side check of the GEMM planner in deterministic mode (ps_gemm_plan.h
// with GemmShape::deterministic set): over the shape sweeps of
// gemm_plan_host.cpp, no plan asks for atomics, every workspace is sized for
// exactly the slabs its kernel writes and stays under the cap, the K slices
// cover K, and with the flag off the planner gives what it gave before the
// flag existed. Driven by tests/test_gemm_det_plan_host.py.
#include <cstdint>
#include <cstdio>

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

// the two shape builders of gemm_plan_host.cpp: positional, so the new
// field takes its default
static GemmShape shape(int M, int N, int K, bool gather) {
  return {M, N, K, /*esize=*/2, /*bk=*/64, /*atomic_ok=*/true,
          /*tr_ok=*/true, gather, /*nt=*/false, /*only128=*/false};
}
static GemmShape gshape(int M, int N, int K, int layout, int esize,
                        bool atomic_ok) {
  return {M, N, K, esize, /*bk=*/esize == 2 ? 64 : 16, atomic_ok,
          /*tr_ok=*/false, /*gather_b=*/false, layout == 0, layout == 2};
}

static bool same_plan(const GemmPlan& a, const GemmPlan& b) {
  return a.tr16 == b.tr16 && a.splitk == b.splitk &&
         a.ws_elems == b.ws_elems && a.bm == b.bm && a.bn == b.bn &&
         a.kchunk == b.kchunk && a.M0 == b.M0 && a.N0 == b.N0 &&
         a.ry == b.ry && a.cx == b.cx;
}

// what ps_gemm_plan does: tr16 first, else generic
static bool plan_any(const GemmShape& g, const TrTune& tune, GemmPlan* p) {
  if (ps_tn_tr_plan(g, tune, p)) return true;
  ps_generic_plan(g, p);
  return false;
}

static long g_tr_ws = 0, g_gen_ws = 0, g_capped = 0;

// every invariant a deterministic plan must hold; off is the plan of the
// same shape with the flag off
static void check_det(const GemmShape& g, const TrTune& tune) {
  GemmShape d = g;
  d.deterministic = true;
  GemmShape e = g;
  e.deterministic = false;
  GemmPlan off, off2, p;
  const bool tr_off = plan_any(g, tune, &off);
  const bool tr_off2 = plan_any(e, tune, &off2);
  const bool tr = plan_any(d, tune, &p);
  // flag off: field by field what the defaulted shape plans
  CHECK(tr_off == tr_off2 && same_plan(off, off2),
        "%dx%dx%d: deterministic = false changed the plan", g.M, g.N, g.K);
  CHECK(off.splitk > 1 || off.ws_elems == 0, "%dx%dx%d: unsplit workspace",
        g.M, g.N, g.K);
  // the mode changes how a GEMM splits, not which path or tile runs it
  CHECK(tr == tr_off && p.tr16 == tr && p.bm == off.bm && p.bn == off.bn &&
            p.M0 == off.M0 && p.N0 == off.N0,
        "%dx%dx%d: deterministic plan took another path or tile", g.M, g.N,
        g.K);
  // no atomics: a split has a workspace
  CHECK(p.splitk >= 1 && (p.splitk == 1) == (p.ws_elems == 0),
        "%dx%dx%d: split %d with ws %lld", g.M, g.N, g.K, p.splitk,
        (long long)p.ws_elems);
  CHECK(p.ws_elems * 4 <= PS_WS_CAP_BYTES, "%dx%dx%d: ws %lld over the cap",
        g.M, g.N, g.K, (long long)p.ws_elems);
  CHECK((int64_t)p.splitk * p.kchunk >= g.K, "%dx%dx%d: slices miss K", g.M,
        g.N, g.K);
  if (tr) {
    CHECK(p.ws_elems == (p.splitk > 1 ? (int64_t)p.splitk * p.M0 * p.N0 : 0),
          "%dx%dx%d: tr16 ws %lld for %d slabs of %dx%d", g.M, g.N, g.K,
          (long long)p.ws_elems, p.splitk, p.M0, p.N0);
    CHECK(p.kchunk % 64 == 0 && (int64_t)(p.splitk - 1) * p.kchunk < g.K,
          "%dx%dx%d: empty tr16 slice (%d x %d)", g.M, g.N, g.K, p.splitk,
          p.kchunk);
    CHECK(p.splitk <= off.splitk, "%dx%dx%d: deterministic split deeper",
          g.M, g.N, g.K);
    // grid.z pads past splitk; those blocks have no slice, hence no slab
    CHECK(ps_tr_grid_z(p) >= p.splitk &&
              (int64_t)p.splitk * p.kchunk >= g.K,
          "%dx%dx%d: grid z", g.M, g.N, g.K);
    g_tr_ws += p.ws_elems > 0;
    g_capped += p.splitk < off.splitk;
  } else {
    CHECK(p.ws_elems == (p.splitk > 1 ? (int64_t)p.splitk * g.M * g.N : 0),
          "%dx%dx%d: generic ws", g.M, g.N, g.K);
    CHECK(p.kchunk % g.bk == 0, "%dx%dx%d: kchunk", g.M, g.N, g.K);
    g_gen_ws += p.ws_elems > 0;
  }
}

int main() {
  // the tr16 sweep of gemm_plan_host.cpp
  const int Ks[] = {64,    448,   512,    1568,   6272,
                    25088, 43264, 186624, 774400, 1605632};
  for (int gather = 0; gather < 2; ++gather)
    for (int M = 16; M <= 512; M += 16)
      for (int N = 64; N <= 4608; N += 64)
        for (int K : Ks) check_det(shape(M, N, K, gather != 0), kAuto);
  // off-grid shapes (edge strips) and forced tiles / targets
  check_det(shape(100, 200, 1 << 20, false), kAuto);
  check_det(shape(100, 200, 4096, false), kAuto);
  {
    const int forced[][5] = {
        {16, 64, 1344, 16, 64},     {32, 128, 1344, 16, 128},
        {64, 64, 1344, 64, 64},     {128, 192, 1344, 64, 128},
        {96, 128, 1344, 96, 128},   {128, 128, 1344, 128, 128},
        {384, 192, 1344, 192, 128}, {256, 192, 1344, 128, 128}};
    for (const auto& f : forced) {
      const int tiles = (f[0] / f[3]) * ((f[1] + f[4] - 1) / f[4]);
      const TrTune tune = {f[3], f[4], 4 * tiles};
      GemmShape g = shape(f[0], f[1], f[2], false);
      check_det(g, tune);
      g.deterministic = true;
      GemmPlan p;
      CHECK(ps_tn_tr_plan(g, tune, &p) && p.bm == f[3] && p.bn == f[4] &&
                p.splitk == 4 && p.kchunk == 384 &&
                p.ws_elems == (int64_t)4 * f[0] * f[1],
            "forced %dx%d tile at %dx%dx%d: split %d kchunk %d", f[3], f[4],
            f[0], f[1], f[2], p.splitk, p.kchunk);
    }
  }
  // a slab so large that the cap must shrink the split, not refuse it
  {
    GemmShape g = shape(512, 4608, 1605632, false);
    g.deterministic = true;
    GemmPlan p;
    if (ps_tn_tr_plan(g, kAuto, &p))
      CHECK(p.ws_elems * 4 <= PS_WS_CAP_BYTES, "cap");
    const TrTune deep = {64, 128, 1 << 20};
    check_det(shape(512, 4608, 1605632, false), deep);
    check_det(shape(512, 2304, 1605632, true), deep);
  }
  // the generic sweep of gemm_plan_host.cpp
  {
    const int Ms[] = {1,   16,  33,   64,   96,   100,  128,   192,   256, 300,
                      384, 512, 676,  1000, 2048, 4096, 8192,  25088, 802816};
    const int Ns[] = {1,   16,  32,   48,   64,   96,   100,  128,
                      192, 256, 384,  1000, 1152, 4096, 9216, 32768};
    const int Kg[] = {1,    16,   63,   64,   96,    200,    256,
                      333,  512,  576,  1024, 1040,  1200,   4096,
                      4608, 9216, 25088, 100352, 200000, 774400};
    for (int M : Ms)
      for (int N : Ns)
        for (int K : Kg)
          for (int layout = 0; layout < 4; ++layout)
            for (int esize = 2; esize <= 4; esize += 2)
              for (int atomic = 0; atomic < 2; ++atomic) {
                if ((int64_t)M * N > (1LL << 31)) continue;
                const GemmShape g = gshape(M, N, K, layout, esize, atomic);
                check_det(g, kAuto);
                // with the mode on, atomic_ok makes no difference
                GemmShape a = g, b = g;
                a.deterministic = b.deterministic = true;
                a.atomic_ok = true;
                b.atomic_ok = false;
                GemmPlan pa, pb;
                ps_generic_plan(a, &pa);
                ps_generic_plan(b, &pb);
                CHECK(same_plan(pa, pb), "%dx%dx%d: atomic_ok still matters",
                      M, N, K);
              }
  }
  CHECK(g_tr_ws > 5000 && g_gen_ws > 1000 && g_capped > 0,
        "sweep reached %ld tr16 / %ld generic workspace plans, %ld capped",
        g_tr_ws, g_gen_ws, g_capped);
  if (g_fail) {
    std::printf("%d gemm-det-plan host checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("all gemm-det-plan host checks passed (%ld tr16, %ld generic "
              "workspace plans, %ld capped)\n",
              g_tr_ws, g_gen_ws, g_capped);
  return 0;
}
