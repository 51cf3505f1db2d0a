// Launch plan of the blob-statistics pass (stats.hip): how many blocks read
// one tensor, and how long the longest chain of dependent float adds into
// one accumulator gets. Host-only arithmetic on (count, itemsize), shared by
// the launcher, the bindings (ops.blob_stats_plan) and the tests, which
// derive their error bound from it.
#pragma once
#include <cstdint>

namespace ps {

constexpr int STATS_THREADS = 256;  // four waves
// independent accumulators per thread = 16-byte loads in flight per thread
constexpr int STATS_UNROLL = 4;
constexpr int STATS_VEC_BYTES = 16;
// one block's loads of one grid-stride trip: 256 x 4 x 16 B. Four resident
// blocks keep 64 KiB per CU in flight, what a streaming read needs to hide
// an HBM miss.
constexpr int64_t STATS_TRIP_BYTES =
    (int64_t)STATS_THREADS * STATS_UNROLL * STATS_VEC_BYTES;
// below this one block reads the tensor: the partial of a second block
// would cost more than the read it saves
constexpr int64_t STATS_FLOOR_BYTES = 64 << 10;
// 256 CUs x 4 blocks; larger tensors take further grid-stride trips
constexpr int STATS_MAX_BLOCKS = 1024;
// finalize: one wave per slot, lane l adds partials l, l + 64, ... in order
constexpr int STATS_FINAL_LANES = 64;

// A block's partial and a slot's final record share one 16-byte layout.
struct StatsRec {
  float asum;          // sum of |x|; NaN / Inf propagate
  float maxabs;        // largest finite |x|
  uint32_t nonfinite;  // NaN or Inf elements
  uint32_t pad;
};

struct StatsPlan {
  int blocks;
  // Longest serial add chain per accumulator: every trip adds one
  // tree-summed vector to each of the STATS_UNROLL accumulators; the
  // scalar head or tail adds at most one more element.
  int64_t chain;
};

inline StatsPlan stats_plan(int64_t count, int itemsize) {
  const int64_t bytes = count * itemsize;
  int64_t blocks = 1;
  if (bytes >= STATS_FLOOR_BYTES) {
    blocks = (bytes + STATS_TRIP_BYTES - 1) / STATS_TRIP_BYTES;
    if (blocks > STATS_MAX_BLOCKS) blocks = STATS_MAX_BLOCKS;
  }
  const int64_t nvec = bytes / STATS_VEC_BYTES;  // most 16-byte loads
  const int64_t per_trip = blocks * STATS_THREADS;
  const int64_t loads = (nvec + per_trip - 1) / per_trip;  // per thread
  return {(int)blocks, (loads + STATS_UNROLL - 1) / STATS_UNROLL + 1};
}

// Adds on the path from one accumulator to the record, after the chain: the
// tree over a vector's elements, over the accumulators, over the 64 lanes,
// the serial sum over the block's waves, then finalize's serial and lane
// sums over the partials.
inline int stats_reduce_depth(int blocks, int itemsize) {
  const int vec = STATS_VEC_BYTES / itemsize;
  int d = 0;
  for (int v = vec; v > 1; v >>= 1) ++d;
  for (int u = STATS_UNROLL; u > 1; u >>= 1) ++d;
  d += 6;                       // lanes
  d += STATS_THREADS / 64 - 1;  // waves
  d += (blocks + STATS_FINAL_LANES - 1) / STATS_FINAL_LANES;  // partials
  d += 6;                       // finalize lanes
  return d;
}

}  // namespace ps
