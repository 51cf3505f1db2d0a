// sd_plan_streams() of ps_softmax_dense_plan.h on the host: one stream is
// sd_plan, two tiles and their labels fit the block's LDS budget under the
// same unit rule. Built by tests/test_softmax_heads_cpu.py.
#include <cstdio>
#include <initializer_list>

#include "ps_softmax_dense_plan.h"

using namespace ps;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      printf("FAILED %s (rows=%lld C=%d itemsize=%d)\n", #cond,            \
             (long long)rows, C, itemsize);                                \
      return 1;                                                            \
    }                                                                      \
  } while (0)

int main() {
  const int64_t row_counts[] = {1, 30, 63, 264, 100000, 1 << 21, 1LL << 31};
  for (int64_t rows : row_counts)
    for (int itemsize : {2, 4})
      for (int C = 1; C <= SD_MAX_C + 1; ++C) {
        const SoftmaxDensePlan p = sd_plan(rows, C, itemsize, 0);
        const SoftmaxDensePlan one = sd_plan_streams(rows, C, itemsize, 1);
        const SoftmaxDensePlan two = sd_plan_streams(rows, C, itemsize, 2);
        CHECK(one.G == p.G && one.TR == p.TR && one.tiles == p.tiles &&
              one.blocks == p.blocks && one.lds == p.lds);
        CHECK(two.G == p.G && two.flip == p.flip);
        if (C > SD_MAX_C) {
          CHECK(p.G == 0);
          continue;
        }
        const int rb = SD_THREADS / p.G, vn = 16 / itemsize;
        CHECK(two.TR >= 1 && two.TR <= p.TR);
        CHECK(two.TR % rb == 0 && two.TR % vn == 0);
        CHECK(two.tiles == (rows + two.TR - 1) / two.TR);
        const size_t tile = (size_t)sd_tile_bytes(two.TR, C, itemsize);
        CHECK(tile == (size_t)two.TR * C * itemsize);  // the second starts aligned
        CHECK(two.lds == 2 * tile + 4 * (size_t)two.TR);
        CHECK(two.lds <= (size_t)SD_TILE_BYTES);
      }
  printf("all softmax-heads plan host checks passed\n");
  return 0;
}
