// Launch geometry of the WITHIN_CHANNEL LRN kernels (lrn_within.hip): how a
// block's 256 lanes are laid out as (segment, pixel, channel vector), how
// many rows a block walks, and the flattened grid. Host-only arithmetic on
// the problem shape, derived once per launch.
#pragma once
#include <cstdint>

namespace ps {

constexpr int LRNW_THREADS = 256;
// channel vectors of one pixel that one block takes: 8 x 16 B = one 128-byte
// line per pixel. More channels go to further blocks (channels are
// independent), so a segment always has 32 pixel slots or more to spend.
constexpr int LRNW_MAX_CVB = 8;
// rows a block emits. The walk also loads the halo rows above and below
// (2R forward, 4R + 1 backward), so shorter strips repeat more of x ...
constexpr int LRNW_STRIP = 8;
// ... and are taken only while the grid would leave most CUs without a block
constexpr int LRNW_MIN_STRIP = 4;
constexpr int64_t LRNW_MIN_BLOCKS = 256;

struct LrnWithinPlan {
  int V;          // channels per lane: 8 (bf16), 4 (fp32) or 1
  int cv;         // channel vectors per pixel, C / V
  int cvb;        // ... of which one block takes this many
  int cgroups;    // blocks across the channel vectors
  int halo;       // halo columns each side of a segment: R fwd, 2R bwd
  int pw;         // pixels a segment emits
  int sp;         // pixel slots of a segment, pw + 2 * halo
  int colgroups;  // segments across one image row
  int segs;       // segments (one per image) in a block
  int imgroups;   // blocks across the images
  int strip;      // rows a block emits
  int strips;     // blocks down an image
  int64_t blocks;
};

inline int lrnw_cdiv(int a, int b) { return (a + b - 1) / b; }

// sizes 3, 5, 7 on 2- or 4-byte elements; any channel count
inline bool lrn_within_ok(int C, int size, int itemsize) {
  return C >= 1 && (size == 3 || size == 5 || size == 7) &&
         (itemsize == 2 || itemsize == 4);
}

// vec: the tensors are 16-byte aligned. strip: rows per block, 0 = default.
inline LrnWithinPlan lrn_within_plan(int N, int C, int H, int W, int itemsize,
                                     int R, bool backward, bool vec,
                                     int strip) {
  LrnWithinPlan p{};
  const int vn = 16 / itemsize;
  p.V = (vec && C % vn == 0) ? vn : 1;
  p.cv = C / p.V;
  p.cgroups = lrnw_cdiv(p.cv, LRNW_MAX_CVB);
  p.cvb = lrnw_cdiv(p.cv, p.cgroups);
  p.halo = backward ? 2 * R : R;
  const int slots = LRNW_THREADS / p.cvb;  // >= 32 > 2 * halo
  if (W + 2 * p.halo <= slots) {
    // whole rows: images share a block when a row leaves lanes over
    p.colgroups = 1;
    p.pw = W;
    p.sp = W + 2 * p.halo;
    p.segs = slots / p.sp;
    if (p.segs > N) p.segs = N;
  } else {
    // a row spans blocks; equal shares, so the last one is not mostly idle
    p.colgroups = lrnw_cdiv(W, slots - 2 * p.halo);
    p.pw = lrnw_cdiv(W, p.colgroups);
    p.sp = p.pw + 2 * p.halo;
    p.segs = 1;
  }
  p.imgroups = lrnw_cdiv(N, p.segs);
  const int64_t per_strip =
      (int64_t)p.cgroups * p.colgroups * p.imgroups;
  if (strip > 0) {
    p.strip = strip;
  } else {
    p.strip = LRNW_STRIP;
    while (p.strip > LRNW_MIN_STRIP &&
           per_strip * lrnw_cdiv(H, p.strip) < LRNW_MIN_BLOCKS)
      p.strip /= 2;
  }
  if (p.strip > H) p.strip = H;
  p.strips = lrnw_cdiv(H, p.strip);
  p.blocks = per_strip * p.strips;
  return p;
}

}  // namespace ps
