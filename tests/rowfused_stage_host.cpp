// Host check of how the row-fused conv kernels stage a tile's input window
// (ps_rowfused.h: ps_rf_vec, ps_rf_narrow_off, ps_rf_elem_mask -- the
// functions conv_rowfused.hip's rf_load_x / rf_store_x fetch and mask with).
// x is a buffer filled with its own indices + 1, walked through a layout's
// strides; for every tile and every 16 B vector of its staged image
//   - the kind returned is the one the rules name (ZERO / WIDE / NARROW),
//   - a WIDE or NARROW vector reads only elements in [0, span), where span is
//     1 + sum (size_i - 1) * stride_i, and the emulated loads trap anything
//     outside it (the buffer is exactly span elements, so the sanitizer build
//     traps it too),
//   - load + mask reproduces the window of the header comment element for
//     element: pixel iw of channel c of row ih where it lies inside the
//     image, zero elsewhere.
// Layouts: NCHW contiguous, NCHW with padded rows, channels-last, and -- by
// construction of the buffer -- an x that starts at element 0 and ends at
// the last element of its buffer. Driven by tests/test_rowfused_stage_host.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ps_rowfused.h"

namespace {

int g_fail = 0;
long g_checks = 0;
long g_kinds[3] = {0, 0, 0};
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++g_checks;                                           \
    if (!(cond)) {                                        \
      if (g_fail < 50) {                                  \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__);  \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                                \
      }                                                   \
      ++g_fail;                                           \
    }                                                     \
  } while (0)

struct Geo {
  int N, C, H, W, Co, k, s, p;
};

enum Layout { NCHW, NCHW_PADDED_ROWS, CHANNELS_LAST };

RowFusedX strides_of(const Geo& g, Layout l) {
  RowFusedX X{};
  if (l == CHANNELS_LAST) {
    X.sw = g.C; X.sh = g.W * g.C; X.sc = 1;
    X.sn = (int64_t)g.H * g.W * g.C;
  } else {
    const int row = l == NCHW_PADDED_ROWS ? g.W + 4 : g.W;
    X.sw = 1; X.sh = row; X.sc = g.H * row;
    X.sn = (int64_t)g.C * g.H * row;
  }
  X.span = 1 + (g.N - 1) * X.sn + (int64_t)(g.C - 1) * X.sc +
           (int64_t)(g.H - 1) * X.sh + (int64_t)(g.W - 1) * X.sw;
  return X;
}

// x[i] = i + 1: a staged value names the element it came from, 0 is a zero
struct Mem {
  std::vector<int64_t> v;
  explicit Mem(int64_t span) : v((size_t)span) {
    for (int64_t i = 0; i < span; ++i) v[(size_t)i] = i + 1;
  }
  int64_t at(int64_t off, const char* what) {
    const bool in = off >= 0 && off < (int64_t)v.size();
    CHECK(in, "%s load at element %ld outside [0, %ld)", what, (long)off,
          (long)v.size());
    return in ? v[(size_t)off] : -1;
  }
};

void check_layout(const Geo& g, Layout lay, int tile_step) {
  const int Kpad = (g.k * g.k * g.C + 63) & ~63;
  const RowFusedTiling t = ps_rowfused_tiling(g.N, g.C, g.H, g.W, g.Co, g.k,
                                              g.k, g.s, g.s, g.p, g.p, Kpad);
  CHECK(t.ok, "shape refused (W %d k %d)", g.W, g.k);
  if (!t.ok) return;
  const RowFusedX X = strides_of(g, lay);
  Mem mem(X.span);
  const int vpr = t.rsw_ld / 8;
  const int total = t.srows * t.C * vpr;
  // the kernels walk idx up to a multiple of their thread count past total
  const int walked = (total + PS_RF_THREADS - 1) / PS_RF_THREADS * PS_RF_THREADS;
  for (int64_t ti = 0; ti < t.tiles; ++ti) {
    if (ti % tile_step && ti != t.tiles - 1 && ti >= t.tiles_per_img) continue;
    const RowFusedTile tl = ps_rf_tile(t, ti);
    for (int idx = 0; idx < walked; ++idx) {
      const RowFusedVec d = ps_rf_vec(t, tl, X, idx);
      // the window, from the header comment
      const int rc = idx / vpr, sr = rc / t.C, c = rc % t.C;
      const int ih = tl.oh0 * t.sh - t.ph + sr;
      const int iw0 = tl.ow0 * t.sw - t.pw + (idx % vpr) * 8;
      int64_t want[8];
      int nlive = 0;
      int64_t row = 0;
      for (int j = 0; j < 8; ++j) {
        const int iw = iw0 + j;
        const bool in = idx < total && ih >= 0 && ih < t.H && iw >= 0 &&
                        iw < t.W;
        row = tl.n * X.sn + (int64_t)ih * X.sh + (int64_t)c * X.sc;
        want[j] = in ? row + (int64_t)iw * X.sw + 1 : 0;
        nlive += in;
      }
      // the kind the rules name. This repeats ps_rf_vec_at's own condition,
      // so it only pins the rule down; the checks that are independent of
      // the code under test are the bounds trap in Mem::at and the
      // element-for-element window comparison below
      int kind = PS_RF_ZERO;
      if (nlive) {
        const int64_t first = row + iw0;
        kind = X.sw == 1 && first >= 0 && first + 8 <= X.span ? PS_RF_WIDE
                                                              : PS_RF_NARROW;
      }
      CHECK(d.kind == kind, "tile %ld idx %d: kind %d, want %d", (long)ti, idx,
            d.kind, kind);
      CHECK(d.lo >= 0 && d.lo <= d.hi && d.hi <= 8, "range [%d, %d)", d.lo,
            d.hi);
      CHECK(d.hi - d.lo == nlive, "tile %ld idx %d: %d live, want %d",
            (long)ti, idx, d.hi - d.lo, nlive);
      if (d.kind < 0 || d.kind > 2) continue;
      ++g_kinds[d.kind];
      // emulate rf_load_x ...
      int64_t got[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (d.kind == PS_RF_WIDE) {
        CHECK(X.sw == 1, "wide load on a strided row");
        for (int j = 0; j < 8; ++j) got[j] = mem.at(d.off + j, "wide");
      } else if (d.kind == PS_RF_NARROW) {
        for (int j = 0; j < 8; ++j)
          got[j] = mem.at(ps_rf_narrow_off(t, d, X.sw, j), "narrow");
      }
      // ... and rf_store_x's mask
      const unsigned em = ps_rf_elem_mask(d.lo, d.hi);
      CHECK(em < 256u, "mask %x", em);
      for (int j = 0; j < 8; ++j) {
        if (!(em >> j & 1u)) got[j] = 0;
        CHECK(got[j] == want[j],
              "tile %ld idx %d elem %d: staged %ld, window %ld (kind %d)",
              (long)ti, idx, j, (long)got[j], (long)want[j], d.kind);
      }
    }
  }
}

void check_geo(const Geo& g, int tile_step) {
  check_layout(g, NCHW, tile_step);
  check_layout(g, NCHW_PADDED_ROWS, tile_step);
  check_layout(g, CHANNELS_LAST, tile_step);
}

}  // namespace

int main() {
  // the shapes of tests/test_gpu_rowfused_stage.py, every tile
  const Geo small[] = {
      {2, 3, 35, 35, 16, 11, 4, 0},   // right edge, as conv1
      {2, 3, 14, 14, 16, 7, 2, 3},    // both edges, odd pad
      {1, 3, 12, 13, 16, 3, 1, 1},    // one image: both ends of the span
      {2, 3, 9, 6, 16, 3, 1, 1},      // a row shorter than a vector
      {2, 3, 9, 8, 16, 3, 1, 1},      // a row equal to a vector
      {2, 3, 6, 130, 16, 3, 1, 1},    // segment mode, iw0 = 127
      {2, 3, 12, 20, 16, 3, 1, 1},
      {2, 3, 15, 19, 16, 11, 4, 0},
      {8, 3, 80, 16, 16, 3, 1, 1},    // many tiles
      {2, 1, 9, 9, 16, 5, 2, 2},      // one channel
      {2, 4, 21, 21, 16, 7, 2, 3},    // four channels
      {1, 3, 3, 3, 16, 3, 1, 1},      // the whole tensor inside one vector
      {1, 1, 1, 5, 16, 1, 1, 0},      // span shorter than a vector
  };
  for (const Geo& g : small) check_geo(g, 1);
  // the four zoo first layers -- three geometries, AlexNet and CaffeNet
  // share theirs: the first image's tiles, a sample of the rest, and the
  // last tile
  const Geo zoo[] = {
      {3, 3, 227, 227, 96, 11, 4, 0},   // AlexNet / CaffeNet conv1
      {3, 3, 224, 224, 64, 3, 1, 1},    // VGG-16 conv1_1
      {3, 3, 224, 224, 64, 7, 2, 3},    // GoogLeNet conv1
  };
  for (const Geo& g : zoo) check_geo(g, 41);
  // AlexNet's window: 45 edge vectors per tile, all of them one wide load
  // except the very last of the tensor
  {
    const Geo& g = zoo[0];
    const RowFusedTiling t = ps_rowfused_tiling(g.N, g.C, g.H, g.W, g.Co, g.k,
                                                g.k, g.s, g.s, g.p, g.p, 384);
    const RowFusedX X = strides_of(g, NCHW);
    long narrow = 0, wide_edge = 0;
    for (int64_t ti = 0; ti < t.tiles; ++ti)
      for (int idx = 0; idx < t.srows * t.C * (t.rsw_ld / 8); ++idx) {
        const RowFusedVec d = ps_rf_vec(t, ps_rf_tile(t, ti), X, idx);
        narrow += d.kind == PS_RF_NARROW;
        wide_edge += d.kind == PS_RF_WIDE && d.hi < 8;
      }
    CHECK(narrow == 1, "AlexNet NCHW: %ld narrow vectors", narrow);
    CHECK(wide_edge > 40 * t.tiles, "AlexNet NCHW: %ld wide edge vectors",
          wide_edge);
  }
  std::printf("%ld checks, %d failures; vectors: %ld zero, %ld wide, %ld "
              "narrow\n", g_checks, g_fail, g_kinds[0], g_kinds[1],
              g_kinds[2]);
  CHECK(g_kinds[0] > 0 && g_kinds[1] > 0 && g_kinds[2] > 0, "a kind unseen");
  if (g_fail) return 1;
  std::printf("all row-fused staging host checks passed\n");
  return 0;
}
