// Host check of the row-fused first-layer conv's plan (ps_rowfused.h, the
// header conv_rowfused.hip's kernels walk tiles and address staged rows
// with): over a sweep of first-layer geometries
//   - the tile walk covers every output position exactly once,
//   - every staged byte an operand read would use lies inside the staged
//     image and is the element a plain /-and-% im2col decode names, or is the
//     zero header for pad columns and dead positions,
//   - the k -> staged-offset table of each 8-element fragment group equals
//     the direct (ky, kx, c) decode,
//   - the LDS need is what the kernels lay out, and the plan (ps_conv_plan.h)
//     refuses what does not fit, small layers, and deterministic mode.
// Driven by tests/test_rowfused_plan_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ps_conv_plan.h"
#include "ps_rowfused.h"

namespace {

int g_fail = 0;
long g_checks = 0;
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

int kpad_of(const Geo& g) { return (g.k * g.k * g.C + 63) & ~63; }

RowFusedTiling tiling_of(const Geo& g) {
  return ps_rowfused_tiling(g.N, g.C, g.H, g.W, g.Co, g.k, g.k, g.s, g.s, g.p,
                            g.p, kpad_of(g));
}

// ---- LDS need, recomputed from the layout the kernels use -----------------
void check_lds(const Geo& g, const RowFusedTiling& t) {
  const int Kpad = kpad_of(g);
  const int Ho = (g.H + 2 * g.p - g.k) / g.s + 1;
  const int Wo = (g.W + 2 * g.p - g.k) / g.s + 1;
  if (Ho <= 0 || Wo <= 0) {
    CHECK(!t.ok, "empty output accepted");
    return;
  }
  const int R = Wo <= PS_RF_TM ? (PS_RF_TM / Wo < Ho ? PS_RF_TM / Wo : Ho) : 1;
  const int WS = Wo <= PS_RF_TM ? Wo : PS_RF_TM;
  const int64_t srows = (int64_t)(R - 1) * g.s + g.k;
  // channel-planar image: srows * C lines of rsw_ld pixels
  const int64_t rsw_ld = (((int64_t)WS - 1) * g.s + g.k + 7) / 8 * 8;
  const int64_t xs = 16 + srows * g.C * rsw_ld * 2;
  const int Cop = g.Co <= 16 ? 16 : g.Co <= 32 ? 32 : g.Co <= 64 ? 64
                : g.Co <= 96 ? 96 : 128;
  const int64_t fwd = (int64_t)Cop * (Kpad + 8) * 2 + Kpad * 4 + 2 * xs;
  const int64_t wg = 2 * 128 * 4 + 2 * (int64_t)128 * (Cop + 8) * 2 + 2 * xs;
  const bool fits = fwd <= 160 * 1024 && wg <= 160 * 1024 &&
                    srows * g.C * (rsw_ld / 8) <= PS_RF_THREADS * PS_RF_XV &&
                    g.Co % 8 == 0 && g.Co <= 128;
  CHECK(t.ok == fits, "ok=%d fits=%d (C%d k%d s%d p%d W%d Co%d)", t.ok, fits,
        g.C, g.k, g.s, g.p, g.W, g.Co);
  if (!t.ok) return;
  CHECK(t.fwd_lds == fwd && t.wg_lds == wg, "lds %d/%d want %ld/%ld",
        t.fwd_lds, t.wg_lds, (long)fwd, (long)wg);
  CHECK(t.xs_bytes == xs, "xs_bytes");
  // regions in order, 16 B aligned, inside the need
  CHECK(t.fwd_koff_off == Cop * t.w_ld * 2 && t.fwd_koff_off % 16 == 0, "koff");
  CHECK(t.fwd_xs_off == t.fwd_koff_off + Kpad * 4 && t.fwd_xs_off % 16 == 0,
        "fwd xs");
  CHECK(t.fwd_xs_off + 2 * t.xs_bytes == t.fwd_lds, "fwd end");
  CHECK(t.wg_dy_off == 2 * PS_RF_TM * 4, "wg dy");
  CHECK(t.wg_xs_off == t.wg_dy_off + 2 * PS_RF_TM * t.dy_ld * 2 &&
        t.wg_xs_off % 16 == 0, "wg xs");
  CHECK(t.wg_xs_off + 2 * t.xs_bytes == t.wg_lds, "wg end");
  CHECK(t.xs_bytes % 16 == 0 && t.rsw_ld % 8 == 0 && t.rsw_ld >= t.rsw, "xs");
  // the last fragment of a dy row and of a weight row stay inside the row
  CHECK(t.dy_ld >= t.Cop && t.w_ld >= Kpad && t.dy_ld % 8 == 0, "row strides");
}

// ---- tile walk + addressing ----------------------------------------------
void check_walk(const Geo& g, const RowFusedTiling& t, int tile_step) {
  const int Kpad = kpad_of(g);
  const int64_t NP = (int64_t)g.N * t.Ho * t.Wo;
  std::vector<int> seen((size_t)NP, 0);
  // the k table as the forward builds it, and its 8-element groups against
  // the direct decode: element e of group (ks, q) is k = ks + q*8 + e
  std::vector<int> koff((size_t)Kpad);
  for (int k = 0; k < Kpad; ++k) koff[k] = ps_rf_koff(t, k);
  for (int ks = 0; ks < Kpad; ks += 32)
    for (int q = 0; q < 4; ++q)
      for (int e = 0; e < 8; ++e) {
        const int k = ks + q * 8 + e;
        if (k >= t.Kcol) {
          CHECK(koff[k] == PS_RF_NEG, "pad k %d not flagged", k);
          continue;
        }
        const int c = k % g.C, kx = (k / g.C) % g.k, ky = k / (g.C * g.k);
        CHECK(koff[k] == ((ky * g.C + c) * t.rsw_ld + kx) * 2,
              "koff[%d] = %d, direct decode (%d,%d,%d)", k, koff[k], ky, kx, c);
      }
  for (int64_t ti = 0; ti < t.tiles; ++ti) {
    const RowFusedTile tl = ps_rf_tile(t, ti);
    CHECK(tl.nlive > 0 && tl.nlive <= PS_RF_TM, "nlive %d", tl.nlive);
    CHECK(tl.n >= 0 && tl.n < g.N && tl.oh0 < t.Ho && tl.ow0 < t.Wo, "tile");
    const bool addr = ti % tile_step == 0 || ti == t.tiles - 1;
    for (int p = 0; p < PS_RF_TM; ++p) {
      const bool live = p < tl.nlive;
      const int oh = tl.oh0 + p / t.WS, ow = tl.ow0 + p % t.WS;
      if (live) {
        const int64_t idx = tl.pos0 + p;
        CHECK(oh < t.Ho && ow < t.Wo, "live position outside the image");
        CHECK(idx == ((int64_t)tl.n * t.Ho + oh) * t.Wo + ow,
              "position %d of tile %ld is not NHWC row pos0 + p", p, (long)ti);
        if (idx >= 0 && idx < NP) ++seen[(size_t)idx];
      }
      if (!addr) continue;
      const int pb = live ? ps_rf_pbase(t, p) : PS_RF_NEG;
      for (int k = 0; k < Kpad; ++k) {
        const int a = ps_rf_addr(pb, koff[k]);
        if (!live || k >= t.Kcol) {
          CHECK(a == 0, "dead read at byte %d", a);  // the zero header
          continue;
        }
        CHECK(a >= PS_RF_HDR && a + 2 <= t.xs_bytes && a % 2 == 0,
              "byte %d outside the staged image of %d", a, t.xs_bytes);
        const int el = (a - PS_RF_HDR) / 2;
        const int line = el / t.rsw_ld, e = el % t.rsw_ld;
        const int sr = line / g.C, sc = line % g.C;
        CHECK(sr < t.srows && e < t.rsw, "staged (%d,%d) of (%d,%d)", sr, e,
              t.srows, t.rsw);
        // what the staging puts there against the im2col entry's pixel
        const int ih = tl.oh0 * g.s - g.p + sr;
        const int iw = tl.ow0 * g.s - g.p + e;
        const int c = k % g.C, kx = (k / g.C) % g.k, ky = k / (g.C * g.k);
        CHECK(ih == oh * g.s - g.p + ky && iw == ow * g.s - g.p + kx &&
                  sc == c,
              "p %d k %d reads (%d,%d,%d)", p, k, ih, iw, sc);
      }
    }
  }
  for (int64_t i = 0; i < NP; ++i)
    CHECK(seen[(size_t)i] == 1, "position %ld covered %d times", (long)i,
          seen[(size_t)i]);
}

void sweep() {
  const int ks[] = {1, 2, 3, 4, 5, 7, 11};
  const int Cos[] = {16, 24, 64, 80, 96, 128};
  for (int C = 1; C <= 4; ++C)
    for (int k : ks)
      for (int s = 1; s <= 4; ++s)
        for (int p = 0; p <= 5 && p < (k > 1 ? k : 2); ++p)
          for (int W = 18; W <= 19; ++W) {
            Geo g = {2, C, 14, W, 16, k, s, p};
            for (int Co : Cos) {
              g.Co = Co;
              check_lds(g, tiling_of(g));
            }
            g.Co = 16;
            const RowFusedTiling t = tiling_of(g);
            if (t.ok) check_walk(g, t, 1);
          }
}

void named_shapes() {
  // the layers the path is for, the Wo-segment shape and the many-tiles
  // shape of tests/test_gpu_rowfused_conv.py; addresses on a sample of tiles
  const Geo shapes[] = {
      {4, 3, 227, 227, 96, 11, 4, 0},   // AlexNet / CaffeNet conv1
      {2, 3, 224, 224, 64, 3, 1, 1},    // VGG-16 conv1_1 (Wo-segment mode)
      {2, 3, 224, 224, 64, 7, 2, 3},    // GoogLeNet conv1
      {2, 3, 9, 130, 16, 3, 1, 1},      // Wo = 130 > tile
      {8, 3, 80, 16, 16, 3, 1, 1},      // many tiles
      {2, 4, 39, 39, 96, 11, 4, 0},     // Kpad = 512
  };
  for (const Geo& g : shapes) {
    const RowFusedTiling t = tiling_of(g);
    check_lds(g, t);
    CHECK(t.ok, "named shape refused (W %d k %d)", g.W, g.k);
    if (t.ok) check_walk(g, t, 37);
  }
  const RowFusedTiling v = tiling_of(shapes[1]);
  CHECK(v.segs == 2 && v.R == 1 && v.WS == PS_RF_TM, "VGG segments");
  const RowFusedTiling a = tiling_of(shapes[0]);
  CHECK(a.R == 2 && a.segs == 1 && a.srows == 15, "AlexNet rows per tile");
}

void plan_policy() {
  // {force_implicit, implicit_bytes, dgrad_fwd_bytes, packed, rowfused,
  //  rowfused_bytes, deterministic}
  const ConvPolicy on = {false, 192LL << 20, 128LL << 20, false,
                         true,  256LL << 20, false};
  auto plan = [](const ConvPolicy& pol, int N, int C, int HW, int Co, int k,
                 int s, int p, int G, int eb) {
    return ps_conv_plan(N, C, HW, HW, Co, k, k, s, s, p, p, G, eb, pol);
  };
  const ConvPlan a = plan(on, 256, 3, 227, 96, 11, 4, 0, 1, 2);
  CHECK(a.rowfused && !a.packed && !a.implicit && a.ld_col == 384 &&
            a.wk_ld == 384, "AlexNet conv1 is row-fused on the plain layout");
  // 205 MB and 154 MB of colT: under the default threshold (they measured
  // slower row-fused), taken once it is lowered
  CHECK(!plan(on, 32, 3, 224, 64, 3, 1, 1, 1, 2).rowfused, "VGG conv1_1");
  CHECK(!plan(on, 32, 3, 224, 64, 7, 2, 3, 1, 2).rowfused, "GoogLeNet conv1");
  ConvPolicy low = on;
  low.rowfused_bytes = 128LL << 20;
  CHECK(plan(low, 32, 3, 224, 64, 3, 1, 1, 1, 2).rowfused, "VGG at 128 MiB");
  CHECK(plan(low, 32, 3, 224, 64, 7, 2, 3, 1, 2).rowfused,
        "GoogLeNet at 128 MiB");
  CHECK(!plan(on, 100, 3, 32, 32, 5, 1, 2, 1, 2).rowfused,
        "CIFAR conv1 is under the threshold");
  CHECK(!plan(on, 256, 3, 227, 96, 11, 4, 0, 1, 4).rowfused, "fp32 stays");
  CHECK(!plan(on, 256, 96, 27, 256, 5, 1, 2, 2, 2).rowfused, "grouped stays");
  CHECK(!plan(on, 256, 8, 227, 96, 11, 4, 0, 1, 2).rowfused, "whole 16 B channel runs stay");
  ConvPolicy pol = on;
  pol.deterministic = true;
  CHECK(!plan(pol, 256, 3, 227, 96, 11, 4, 0, 1, 2).rowfused, "deterministic");
  pol = on;
  pol.rowfused = false;
  CHECK(!plan(pol, 256, 3, 227, 96, 11, 4, 0, 1, 2).rowfused, "switch off");
  pol = on;
  pol.packed = true;
  CHECK(!plan(pol, 256, 3, 227, 96, 11, 4, 0, 1, 2).rowfused, "packed wins");
  pol = on;
  pol.rowfused_bytes = 0;
  CHECK(plan(pol, 2, 3, 35, 96, 11, 4, 0, 1, 2).rowfused, "threshold 0");
  // a window that cannot be staged: the plan keeps the column matrix
  // (Wo = 128 at stride 4: 11 rows x 4 channels of 519 pixels)
  CHECK(!ps_conv_plan(64, 4, 64, 519, 64, 11, 11, 4, 4, 0, 0, 1, 2, pol)
             .rowfused, "oversized window accepted");
  CHECK(ps_conv_plan(64, 4, 64, 4000, 64, 11, 11, 1, 1, 0, 0, 1, 2, pol)
            .rowfused, "a wide image runs as Wo segments");
  CHECK(!plan(pol, 64, 3, 64, 136, 3, 1, 1, 1, 2).rowfused, "Co > 128");
}

}  // namespace

int main() {
  sweep();
  named_shapes();
  plan_policy();
  std::printf("%ld checks, %d failures\n", g_checks, g_fail);
  if (g_fail) return 1;
  std::printf("all row-fused plan host checks passed\n");
  return 0;
}
