// Host check of the NN tr16 plans (ps_gemm_plan.h, ps_nn_tr_plan) against
// what gemm_nn_tr_kernel relies on: an NN tile, K slices of whole 64-row
// tiles with none empty, a grid within the block slots when skinny, a
// workspace under the cap, a block remap that is a permutation of the grid.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ps_gemm_plan.h"

static int g_fail = 0;
#define CHECK(cond, what, g)                                               \
  if (!(cond) && ++g_fail <= 20)                                           \
  std::printf("FAIL line %d: %dx%dx%d: %s\n", __LINE__, (g).M, (g).N, (g).K, what)

// an eligible bf16 K-last x K-major GEMM as gemm_shape() describes it
static GemmShape nn_shape(int M, int N, int K, bool atomic_ok = false) {
  GemmShape g = {M, N, K, 2, 64, atomic_ok, false, false, false, false};
  g.skinny_kmin = PS_SKINNY_KMIN;
  g.nn_ok = true;
  return g;
}

static void check_plan(const GemmShape& g, const GemmPlan& p) {
  CHECK(p.tr16_nn && !p.tr16 && !p.split3, "flags", g);
  CHECK(ps_nn_tile(p.bm, p.bn) && ps_nn_lds_bytes(p.bm, p.bn) <= 64 * 1024,
        "tile", g);
  CHECK(p.kchunk > 0 && p.kchunk % 64 == 0 &&
            (int64_t)p.splitk * p.kchunk >= g.K &&
            (int64_t)(p.splitk - 1) * p.kchunk < g.K, "slices", g);
  const int nby = (g.M + p.bm - 1) / p.bm, nbx = (g.N + p.bn - 1) / p.bn;
  CHECK(!p.skinny || g.skinny_tune.splitk > 0 ||
            (int64_t)nby * nbx * p.splitk <= PS_SKINNY_SLOTS, "slots", g);
  // a split is a workspace split, whatever C could take
  CHECK(p.ws_elems == (p.splitk > 1 ? (int64_t)p.splitk * g.M * g.N : 0) &&
            p.ws_elems * 4 <= PS_WS_CAP_BYTES, "workspace", g);
  // the remap, called as the kernel calls it, hits every block once
  std::vector<int> seen((size_t)nby * nbx * p.splitk, 0);
  size_t once = 0;
  for (int z = 0; z < p.splitk; ++z)
    for (int y = 0; y < nbx; ++y)
      for (int x = 0; x < nby; ++x) {
        const GemmBlock b = ps_remap_nn(nby, nbx, p.splitk, x, y, z);
        if (b.bx >= 0 && b.bx < nbx && b.by >= 0 && b.by < nby && b.bz >= 0 &&
            b.bz < p.splitk)
          once += ++seen[((size_t)b.bz * nbx + b.bx) * nby + b.by] == 1;
      }
  CHECK(once == seen.size(), "remap is no permutation", g);
}

int main() {
  struct Case {
    int M, N, K;  // dx[M, N = Kin] over K = Nout
    SkinnyTune tune;
    int bm, bn, splitk, kchunk;  // expected; bm = 0: only the invariants
  };
  const Case cases[] = {
      // AlexNet fc6 / fc7 / fc8 dx, VGG-16's at batch 32, a conv dgrad
      {256, 9216, 4096, {0, 0, 0}, 128, 128, 3, 1408},
      {256, 4096, 4096, {0, 0, 0}, 128, 128, 8, 512},
      {256, 4096, 1000, {0, 0, 0}, 64, 64, 2, 512},
      {32, 25088, 4096, {0, 0, 0}, 64, 64, 1, 4096},
      {32, 4096, 4096, {0, 0, 0}, 64, 64, 8, 512},
      {32, 4096, 1000, {0, 0, 0}, 64, 64, 2, 512},
      {6272, 4608, 512, {0, 0, 0}, 128, 128, 1, 512},
      // the shapes of tests/test_gpu_tr16_nn.py
      {64, 64, 64, {64, 64, 0}, 64, 64, 1, 64},
      {128, 128, 128, {128, 128, 0}, 128, 128, 1, 128},
      {50, 64, 128, {0, 0, 0}, 64, 64, 1, 128},
      {1, 64, 64, {0, 0, 0}, 64, 64, 1, 64},
      {64, 64, 96, {0, 0, 0}, 64, 64, 1, 128},
      {64, 64, 72, {0, 0, 0}, 64, 64, 1, 128},
      {64, 192, 64, {128, 128, 0}, 128, 128, 1, 64},
      {64, 64, 1096, {64, 64, 4}, 64, 64, 4, 320},
      {50, 192, 136, {0, 0, 0}, 64, 64, 1, 192},
      {256, 128, 1000, {0, 0, 0}, 0, 0, 0, 0},
  };
  GemmPlan p;
  for (const Case& c : cases)
    for (int variant = 0; variant < 4; ++variant) {
      GemmShape g = nn_shape(c.M, c.N, c.K, variant & 1);
      g.deterministic = variant >> 1;
      g.skinny_tune = c.tune;
      if (c.tune.splitk) g.skinny_kmin = 64;
      CHECK(ps_nn_tr_plan(g, &p), "not taken", g);
      check_plan(g, p);
      CHECK(c.bm == 0 || (p.bm == c.bm && p.bn == c.bn &&
                          p.splitk == c.splitk && p.kchunk == c.kchunk),
            "not the expected plan", g);
      // the switch off: a GemmShape that says nothing of nn_ok
      g.nn_ok = GemmShape{}.nn_ok;
      CHECK(!ps_nn_tr_plan(g, &p), "taken with the switch off", g);
    }
  // what the kernel cannot run stays where it was
  for (const GemmShape& g : {nn_shape(64, 100, 64), nn_shape(64, 64, 68),
                             nn_shape(64, 64, 56)})
    CHECK(!ps_nn_tr_plan(g, &p), "taken", g);
  // 11 slabs of 512 x 11904 floats fit the 256 MiB cap, the 16 asked for
  // do not
  GemmShape g = nn_shape(512, 11904, 8192);
  g.skinny_tune = {0, 0, 16};
  CHECK(ps_nn_tr_plan(g, &p) && p.splitk == 11, "cap", g);
  check_plan(g, p);

  if (g_fail) std::printf("%d nn-tr-plan host checks FAILED\n", g_fail);
  else std::printf("all nn-tr-plan host checks passed\n");
  return g_fail ? 1 : 0;
}
