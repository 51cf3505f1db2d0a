// Host check of the tr16 K-tail plans (ps_gemm_plan.h): with GemmShape::ktail
// set, ps_tn_tr_plan accepts K % 64 != 0 and keeps the slice invariants the
// kernel relies on; without it the same shapes are refused, as they always
// were. Stand-alone: no HIP, no torch.
#include <cstdio>

#include "ps_gemm_plan.h"

static int g_fail = 0;
#define CHECK(cond, ...)                               \
  do {                                                 \
    if (!(cond) && ++g_fail <= 20) {                   \
      std::printf("FAIL line %d: ", __LINE__);         \
      std::printf(__VA_ARGS__);                        \
      std::printf("\n");                               \
    }                                                  \
  } while (0)

static GemmShape shape(int M, int N, int K, bool gather, bool det,
                       bool ktail) {
  GemmShape g = {M, N, K, /*esize=*/2, /*bk=*/64, /*atomic_ok=*/true,
                 /*tr_ok=*/true, gather, /*nt=*/false, /*only128=*/false};
  g.deterministic = det;
  g.ktail = ktail;
  return g;
}

int main() {
  const TrTune kAuto = {0, 0, 0};
  const int Ks[] = {65, 96, 776, 1568, 5408, 8450};
  long planned = 0, split = 0;
  for (int mode = 0; mode < 4; ++mode)
    for (int M = 16; M <= 512; M += 16)
      for (int N = 64; N <= 4608; N += 64)
        for (int K : Ks) {
          const bool gather = mode & 1, det = mode & 2;
          GemmPlan p;
          CHECK(!ps_tn_tr_plan(shape(M, N, K, gather, det, false), kAuto, &p),
                "%dx%dx%d took tr16 without the K-tail", M, N, K);
          if (!ps_tn_tr_plan(shape(M, N, K, gather, det, true), kAuto, &p))
            continue;
          ++planned;
          split += p.splitk > 1;
          CHECK(p.tr16 && ps_tr_tile(p.bm, p.bn) && p.kchunk % 64 == 0 &&
                    (int64_t)p.splitk * p.kchunk >= K &&
                    (int64_t)(p.splitk - 1) * p.kchunk < K,
                "%dx%dx%d: tile %dx%d, %d slices of %d", M, N, K, p.bm, p.bn,
                p.splitk, p.kchunk);
          // padded bz <=> no slice
          for (int bz = 0; bz < ps_tr_grid_z(p); ++bz)
            CHECK((bz >= p.splitk) == ((int64_t)bz * p.kchunk >= K),
                  "%dx%dx%d: bz %d (splitk %d, kchunk %d)", M, N, K, bz,
                  p.splitk, p.kchunk);
          CHECK(p.ws_elems == (det && p.splitk > 1
                                   ? (int64_t)p.splitk * p.M0 * p.N0 : 0),
                "%dx%dx%d: workspace %lld", M, N, K, (long long)p.ws_elems);
        }
  CHECK(planned > 50000 && split > 10000, "sweep: %ld plans, %ld split",
        planned, split);
  GemmPlan p;
  CHECK(!ps_tn_tr_plan(shape(64, 64, 40, false, false, true), kAuto, &p),
        "K = 40 took tr16");
  // the GPU test's prologue-staged tail: four slices, the last of 8 rows
  const TrTune t64 = {64, 64, 0};
  CHECK(ps_tn_tr_plan(shape(64, 64, 776, false, false, true), t64, &p) &&
            p.splitk == 4 && p.kchunk == 256, "64x64x776");
  if (g_fail) return std::printf("%d K-tail plan checks FAILED\n", g_fail), 1;
  std::printf("all tr16 K-tail plan checks passed\n");
  return 0;
}
