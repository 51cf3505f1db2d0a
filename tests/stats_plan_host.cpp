// Host sweep of the blob-statistics planner (ps_stats_plan.h). For many
// (count, itemsize, pointer misalignment) it walks the index pattern of
// stats.hip's stats_block on the host -- scalar head to the first 16-byte
// boundary, grid-stride vector loop with STATS_UNROLL accumulators, one
// leftover load per accumulator, scalar tail -- and checks that every element
// is read exactly once and inside the tensor, that no accumulator's add chain
// is longer than the plan says, and the plan's block rule: one block below the
// floor, proportional to bytes above it, capped.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ps_stats_plan.h"

using namespace ps;

static int g_fail = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      if (++g_fail < 20) {                       \
        printf("FAIL %s: ", #cond);              \
        printf(__VA_ARGS__);                     \
        printf("\n");                            \
      }                                          \
    }                                            \
  } while (0)

// misalign: bytes of the data pointer past a 16-byte boundary (a multiple of
// the element size). full: also count every element's reads.
static void walk(int64_t n, int es, int misalign, bool full) {
  const StatsPlan plan = stats_plan(n, es);
  const int ve = STATS_VEC_BYTES / es;
  int64_t head = ((16 - misalign) & 15) / es;
  if (head > n) head = n;
  const int64_t nvec = (n - head) / ve;
  const int64_t tail0 = head + nvec * ve;
  std::vector<uint8_t> seen(full ? n : 0, 0);
  const int nb = plan.blocks;
  const int64_t stride = (int64_t)nb * STATS_THREADS;
  int64_t longest = 0;
  // without the element count only the busiest threads matter: the first
  // ones of block 0 (they also take the head and the tail)
  const int blocks = full ? nb : 1;
  const int threads = full ? STATS_THREADS : 16;
  for (int b = 0; b < blocks; ++b)
    for (int tid = 0; tid < threads; ++tid) {
      int64_t chain[STATS_UNROLL] = {};
      auto vec = [&](int u, int64_t i) {
        CHECK(i >= 0 && i < nvec, "n=%lld es=%d vec %lld of %lld",
              (long long)n, es, (long long)i, (long long)nvec);
        ++chain[u];
        if (full)
          for (int k = 0; k < ve; ++k) ++seen[head + i * ve + k];
      };
      int64_t i = (int64_t)b * STATS_THREADS + tid;
      for (; i + (STATS_UNROLL - 1) * stride < nvec; i += STATS_UNROLL * stride)
        for (int u = 0; u < STATS_UNROLL; ++u) vec(u, i + u * stride);
      for (int u = 0; u < STATS_UNROLL - 1; ++u)
        if (i < nvec) {
          vec(u, i);
          i += stride;
        }
      CHECK(i >= nvec, "n=%lld es=%d: loads left over", (long long)n, es);
      if (b == 0) {
        if (tid < head) {
          ++chain[STATS_UNROLL - 1];
          if (full) ++seen[tid];
        } else if (tid - head < n - tail0) {
          ++chain[STATS_UNROLL - 1];
          CHECK(tail0 + tid - head < n, "tail out of range");
          if (full) ++seen[tail0 + tid - head];
        }
      }
      for (int u = 0; u < STATS_UNROLL; ++u)
        if (chain[u] > longest) longest = chain[u];
    }
  CHECK(longest <= plan.chain, "n=%lld es=%d mis=%d: chain %lld > plan %lld",
        (long long)n, es, misalign, (long long)longest, (long long)plan.chain);
  CHECK(n - tail0 < ve && head < ve, "head / tail longer than a vector");
  if (full)
    for (int64_t e = 0; e < n; ++e)
      CHECK(seen[e] == 1, "n=%lld es=%d mis=%d: element %lld read %d times",
            (long long)n, es, misalign, (long long)e, seen[e]);
}

int main() {
  for (int es : {2, 4}) {
    // block rule
    int prev = 0;
    for (int64_t n = 1; n < ((int64_t)1 << 31); n += n / 3 + 1) {
      const StatsPlan p = stats_plan(n, es);
      const int64_t bytes = n * es;
      CHECK(p.blocks >= 1 && p.blocks <= STATS_MAX_BLOCKS, "blocks %d", p.blocks);
      CHECK(p.blocks >= prev, "blocks not monotone at n=%lld", (long long)n);
      CHECK(bytes >= STATS_FLOOR_BYTES || p.blocks == 1, "floor");
      if (bytes >= STATS_FLOOR_BYTES && p.blocks < STATS_MAX_BLOCKS)
        CHECK((int64_t)p.blocks * STATS_TRIP_BYTES >= bytes &&
                  (int64_t)(p.blocks - 1) * STATS_TRIP_BYTES < bytes,
              "not proportional at n=%lld", (long long)n);
      CHECK(p.chain >= 1, "chain");
      CHECK(stats_reduce_depth(p.blocks, es) <= 3 + 2 + 6 + 3 + 16 + 6, "depth");
      prev = p.blocks;
      walk(n, es, 0, false);
      walk(n, es, 16 - es, false);
    }
    // every element exactly once: small counts at every misalignment, and
    // counts around the floor and a few trips
    for (int mis = 0; mis < 16; mis += es) {
      for (int64_t n = 1; n <= 600; ++n) walk(n, es, mis, true);
      for (int64_t n : {2049, 65537, 16384, 16385, 32768, 300001, 1 << 20})
        walk(n, es, mis, true);
    }
    // past the cap: several trips per thread
    walk(((int64_t)12 << 20) + 77, es, es, true);
  }
  if (g_fail) {
    printf("%d stats-plan host checks FAILED\n", g_fail);
    return 1;
  }
  printf("all stats-plan host checks passed\n");
  return 0;
}
