// Launch plan of the MVN kernels (mvn.hip): which of the two reduction
// geometries and three regimes a problem runs in, how a group's lanes are
// laid out as (item slot, channel vector), and the grid. Host-only
// arithmetic on the problem shape, derived once per launch.
//
// Both geometries are one picture. A slab is what one group reduces; it has
// `items` items, and a lane owns every slots-th item from its own slot on:
//   per channel: a slab is one image x cvb channel vectors, an item is a
//                pixel, the cvb lanes of a slot read one contiguous run of
//                cvb * 16 bytes, and every channel keeps its own statistic
//   across:      a slab is one image's C*H*W contiguous elements, an item
//                is one vector of it, cvb = 1, and all of it is one set
#pragma once
#include <cstddef>
#include <cstdint>

namespace ps {

constexpr int MVN_THREADS = 256;
// wave-resident: items one lane keeps in registers (raw 16-byte vectors)
constexpr int MVN_WAVE_ITEMS = 8;
// LDS a block may stage. The CU has 160 KiB; a block takes at most 64 KiB so
// that two blocks always share a CU and one streams while the other reduces.
constexpr int MVN_LDS_BYTES = 64 << 10;
// channel vectors of one pixel a group takes: 8 x 16 B = one 128-byte line;
// single elements (V = 1): up to a wave's worth
constexpr int MVN_MAX_CVB = 8;
constexpr int MVN_MAX_CVB_SCALAR = 64;
// fewer blocks than this leave CUs idle: slabs are split to reach it ...
constexpr int64_t MVN_FILL_BLOCKS = 512;
// ... while a lane of a split block still keeps this many items
constexpr int MVN_SPLIT_MIN_ITEMS = 2;

enum MvnRegime { MVN_WAVE = 0, MVN_LDS = 1, MVN_SPLIT = 2 };

struct MvnPlan {
  int rows;       // 1: across channels (one set per image), 0: per channel
  int V;          // elements per lane access: 8 (bf16), 4 (fp32) or 1
  int C;          // elements between two items of a slot column's start
  int cv;         // channel vectors per item
  int cvb;        // ... of which one group takes this many (a power of two)
  int cgroups;    // groups across the channel vectors
  int items;      // items of a slab
  int split;      // chunks per slab (1 unless MVN_SPLIT)
  int chunk;      // items per chunk; the last one may be shorter
  int per_lane;   // most items any lane owns
  int regime;
  int64_t sets;   // statistics: N (across) or N * C
  int64_t groups; // slabs * split
  int64_t blocks;
  size_t lds;     // dynamic LDS bytes of a block
};

inline int64_t mvn_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// fp32 or bf16, and a grid and item count that fit an int
inline bool mvn_ok(int64_t N, int64_t C, int64_t P, int itemsize) {
  return N >= 0 && C >= 1 && P >= 1 && (itemsize == 2 || itemsize == 4) &&
         C * P < ((int64_t)1 << 31) && N * C < ((int64_t)1 << 31);
}

// N images of P pixels x C channels, channels innermost. vec: every tensor
// is 16-byte aligned. force_split: tests only, chunks per slab (0 = planned).
inline MvnPlan mvn_plan(int64_t N, int C, int64_t P, int itemsize, bool across,
                        bool backward, bool vec, int force_split) {
  MvnPlan p{};
  const int vn = 16 / itemsize;
  const int64_t L = (int64_t)C * P;
  p.rows = across ? 1 : 0;
  if (across) {
    // a row starts at n * L elements: aligned for every n only if vn | L
    p.V = (vec && L % vn == 0) ? vn : 1;
    p.C = p.V;
    p.cv = p.cvb = p.cgroups = 1;
    p.items = (int)(L / p.V);
    p.sets = N;
  } else {
    p.V = (vec && C % vn == 0) ? vn : 1;
    p.C = C;
    p.cv = C / p.V;
    const int cap = p.V == 1 ? MVN_MAX_CVB_SCALAR : MVN_MAX_CVB;
    p.cvb = 1;
    while (p.cvb < cap && p.cvb < p.cv) p.cvb *= 2;
    p.cgroups = (int)mvn_cdiv(p.cv, p.cvb);
    p.items = (int)P;
    p.sets = N * C;
  }
  const int64_t slabs = N * p.cgroups;
  const int raw = p.V == 1 ? itemsize : 16;
  const int layers = backward ? 2 : 1;  // the backward stages x and dy
  const int lds_items = MVN_LDS_BYTES / (MVN_THREADS * raw * layers);
  const int wave_per = (int)mvn_cdiv(p.items, 64 / p.cvb);
  const int blk_slots = MVN_THREADS / p.cvb;
  const int blk_per = (int)mvn_cdiv(p.items, blk_slots);
  // a wave per slab when the slab fits its registers and either there are
  // slabs enough for every CU or a whole block would have idle lanes
  if (force_split <= 0 && wave_per <= MVN_WAVE_ITEMS &&
      (slabs >= 4 * MVN_FILL_BLOCKS || blk_per <= 1)) {
    p.regime = MVN_WAVE;
    p.split = 1;
    p.chunk = p.items;
    p.per_lane = wave_per;
    p.groups = slabs;
    p.blocks = mvn_cdiv(slabs, MVN_THREADS / 64);
    p.lds = 0;
    return p;
  }
  int64_t S = mvn_cdiv(blk_per, lds_items);  // what LDS demands
  if (force_split > 0) {
    if (S < force_split) S = force_split;
  } else if (slabs * S < MVN_FILL_BLOCKS) {  // what the chip wants
    int64_t want = mvn_cdiv(MVN_FILL_BLOCKS, slabs);
    const int64_t most = blk_per / MVN_SPLIT_MIN_ITEMS;
    if (want > most) want = most;
    if (S < want) S = want;
  }
  if (S > p.items) S = p.items;
  p.chunk = (int)mvn_cdiv(p.items, S);
  p.split = (int)mvn_cdiv(p.items, p.chunk);  // no empty chunk
  p.per_lane = (int)mvn_cdiv(p.chunk, blk_slots);
  p.regime = p.split > 1 ? MVN_SPLIT : MVN_LDS;
  p.groups = slabs * p.split;
  p.blocks = p.groups;
  p.lds = (size_t)p.per_lane * MVN_THREADS * raw * layers;
  return p;
}

// floats of (mean, M2) or (sum dy, sum dy*y) partials a split plan needs
inline int64_t mvn_ws_floats(const MvnPlan& p) {
  return p.split > 1 ? 2 * p.sets * p.split : 0;
}

}  // namespace ps
