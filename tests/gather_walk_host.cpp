// Host check of the gather GEMM's address walk (ps_gather.h): the tap state
// a lane advances by adds must equal the direct decode at every k-tile, and
// (row context + tap) must give the offset and the zero-page decision of a
// plain /-and-% im2col decode for every row and column of the conv shapes
// tests/test_gpu_gather_gemm.py runs on the GPU. Also checks where the
// planner hands out the N-fitting 128x96 / 128x48 tiles (ps_gemm_plan.h).
// Driven by tests/test_gather_walk_host.py.
#include <cstdio>
#include <cstdlib>

#include "ps_conv_plan.h"
#include "ps_gather.h"
#include "ps_gemm_plan.h"

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

// ground truth with integer division, no helper involved
struct Ref {
  int kkh, kkw, cg;
  bool zero;
  int64_t off;
};
Ref ref_decode(const GatherDesc& d, int64_t row, int k) {
  Ref r;
  r.cg = k % d.Cg;
  const int khw = k / d.Cg;
  r.kkw = khw % d.kw;
  r.kkh = khw / d.kw;
  const int ow = (int)(row % d.Wo);
  const int64_t t = row / d.Wo;
  const int oh = (int)(t % d.Ho);
  const int64_t n = t / d.Ho;
  const int ih = oh * d.sh - d.ph + r.kkh, iw = ow * d.sw - d.pw + r.kkw;
  r.zero = k >= d.kg_max || ih < 0 || ih >= d.H || iw < 0 || iw >= d.W;
  r.off = ((n * d.H + ih) * d.W + iw) * d.C + d.c0 + r.cg;
  return r;
}

// the staging's lane -> column map: 16 B slots of a k-tile, XOR-swizzled by
// the row-parity bit
int lane_kc(int slot, int parity, int epb) { return (slot ^ (parity << 1)) * epb; }

// ---- 1. incremental tap == direct decode ---------------------------------
void sweep_taps() {
  const int Cgs[] = {8, 16, 24, 48, 64, 96, 192, 256, 512};
  const int kws[] = {1, 3, 5, 7, 11};
  const int khs[] = {1, 3, 5};
  const int kbegins[] = {0, 64, 1536, 2048};
  // bf16: 64-deep tiles of 8-element chunks; f32: 16-deep tiles of 4
  const int steps[2] = {64, 16}, epbs[2] = {8, 4};
  for (int Cg : Cgs)
    for (int kw : kws)
      for (int kh : khs)
        for (int fmt = 0; fmt < 2; ++fmt) {
          const int step = steps[fmt], epb = epbs[fmt];
          GatherDesc d{};
          d.C = 2 * Cg; d.c0 = Cg; d.Cg = Cg;
          d.kh = kh; d.kw = kw;
          d.H = 13; d.W = 17; d.Ho = 13; d.Wo = 17;
          d.sh = d.sw = 1; d.ph = kh / 2; d.pw = kw / 2;
          d.kg_max = kh * kw * Cg;
          ps_fill_gather_inv(&d);
          const int Kpad = (d.kg_max + step - 1) / step * step;
          for (int kb : kbegins)
            for (int slot = 0; slot < step / epb; ++slot)
              for (int par = 0; par < 2; ++par) {
                int k = kb + lane_kc(slot, par, epb);
                if (k >= Kpad) continue;
                GatherTap t = ps_gather_tap(d, k);
                for (; k < Kpad; k += step) {
                  const Ref r = ref_decode(d, 0, k);
                  CHECK(t.kkh == r.kkh && t.kkw == r.kkw && t.cg == r.cg,
                        "Cg %d kw %d kh %d step %d k %d: tap (%d,%d,%d) want "
                        "(%d,%d,%d)", Cg, kw, kh, step, k, t.kkh, t.kkw, t.cg,
                        r.kkh, r.kkw, r.cg);
                  CHECK(t.off == (r.kkh * d.W + r.kkw) * d.C + d.c0 + r.cg,
                        "Cg %d kw %d kh %d step %d k %d: tap offset %d", Cg,
                        kw, kh, step, k, t.off);
                  const GatherTap dir = ps_gather_tap(d, k);
                  CHECK(dir.kkh == t.kkh && dir.kkw == t.kkw &&
                            dir.cg == t.cg && dir.off == t.off,
                        "Cg %d kw %d kh %d k %d: walk != ps_gather_tap", Cg,
                        kw, kh, k);
                  ps_gather_tap_advance(d, t, k, step);
                }
              }
        }
}

// ---- 2. (row context + walked tap) == plain decode, GPU test shapes ------
struct Case {
  const char* name;
  int N, C, H, W, Co, k, s, p, G, elem_bytes;
};
const Case kCases[] = {
    {"conv2-like", 4, 96, 13, 13, 256, 5, 1, 2, 2, 2},
    {"conv4-like", 4, 384, 13, 13, 384, 3, 1, 1, 2, 2},
    {"small-Cg", 4, 8, 16, 16, 96, 3, 1, 1, 1, 2},
    {"strided", 8, 64, 17, 17, 128, 3, 2, 1, 1, 2},
    {"wide-kernel", 4, 16, 12, 12, 48, 7, 1, 3, 1, 2},
    {"split-K", 2, 512, 8, 8, 128, 3, 1, 1, 1, 2},
    {"small-Cg f32", 4, 8, 16, 16, 96, 3, 1, 1, 1, 4},
};

void check_desc(const char* name, const char* role, const GatherDesc& d,
                int64_t rows, int step, int epb) {
  const int Kpad = (d.kg_max + step - 1) / step * step;
  for (int kc = 0; kc < step; kc += epb) {
    GatherTap t = ps_gather_tap(d, kc);
    for (int k = kc; k < Kpad; k += step) {
      for (int64_t row = 0; row < rows; ++row) {
        const GatherRow rc = ps_gather_row(d, (int)row);
        const Ref r = ref_decode(d, row, k);
        const bool oob = ps_gather_oob(d, rc, t, k);
        CHECK(oob == r.zero, "%s %s row %ld k %d: zero page %d want %d", name,
              role, (long)row, k, (int)oob, (int)r.zero);
        if (k >= d.kg_max) CHECK(oob, "%s %s k %d: pad column read", name, role, k);
        if (!r.zero)
          CHECK(ps_gather_offset(rc, t) == r.off,
                "%s %s row %ld k %d: offset %ld want %ld", name, role,
                (long)row, k, (long)ps_gather_offset(rc, t), (long)r.off);
      }
      ps_gather_tap_advance(d, t, k, step);
    }
  }
}

void sweep_cases() {
  // implicit forward forced; dgrad-as-forward forced (threshold 0)
  const ConvPolicy pol = {true, 192LL << 20, 0, false};
  for (const Case& c : kCases) {
    const ConvPlan p = ps_conv_plan(c.N, c.C, c.H, c.W, c.Co, c.k, c.k, c.s,
                                    c.s, c.p, c.p, c.G, c.elem_bytes, pol);
    const int epb = 16 / c.elem_bytes, step = c.elem_bytes == 2 ? 64 : 16;
    CHECK(p.implicit, "%s: plan is not implicit", c.name);
    for (int grp = 0; grp < c.G; ++grp) {
      const GatherDesc df =
          ps_gather_desc(p, PS_GATHER_FWD, nullptr, nullptr, grp);
      check_desc(c.name, "fwd", df, p.NP, step, epb);
      if (p.dgrad_as_fwd) {
        const GatherDesc dd =
            ps_gather_desc(p, PS_GATHER_DGRAD_AS_FWD, nullptr, nullptr, grp);
        check_desc(c.name, "dgrad", dd, (int64_t)c.N * c.H * c.W, step, epb);
      }
    }
    // every stride-1 case must reach the dgrad-as-forward gather
    if (c.s == 1) CHECK(p.dgrad_as_fwd, "%s: no dgrad-as-forward", c.name);
  }
}

// ---- 3. the N-fitting tiles go where they cut padded MFMA work -----------
void check_tiles() {
  struct Q { int M, N, bm, bn; };
  const Q want[] = {
      {300, 96, 128, 96},      // tests/test_gpu_gather_gemm.py tile shapes
      {300, 192, 128, 96},
      {260, 48, 128, 48},
      {43264, 192, 128, 96},   // AlexNet conv4 forward, conv4/5 dgrad
      {774400, 96, 128, 96},   // AlexNet conv1 forward
      {186624, 48, 128, 48},   // AlexNet conv2 dgrad
      {43264, 128, 128, 128},  // nothing to cut: the square menu stays
      {43264, 384, 128, 128},
      {43264, 256, 128, 128},
      {1605632, 64, 64, 64},
      {256, 4096, 128, 128},
      {256, 1000, 128, 128},
  };
  for (const Q& q : want) {
    int bm = 0, bn = 0;
    pick_gemm_tile(q.M, q.N, &bm, &bn, true);
    CHECK(bm == q.bm && bn == q.bn, "tile of %dx%d: %dx%d, want %dx%d", q.M,
          q.N, bm, bn, q.bm, q.bn);
    // other layouts never see the narrow tiles
    int bm0 = 0, bn0 = 0;
    pick_gemm_tile(q.M, q.N, &bm0, &bn0, false);
    CHECK(bn0 != 96 && bn0 != 48, "narrow tile without the flag");
  }
  // a narrow tile never pads N more than the tile it replaces, and its
  // double-buffered padded LDS images leave two blocks per CU
  for (int N = 1; N <= 1024; ++N) {
    int bm = 0, bn = 0, bm0 = 0, bn0 = 0;
    pick_gemm_tile(4096, N, &bm, &bn, true);
    pick_gemm_tile(4096, N, &bm0, &bn0, false);
    if (bn == 96 || bn == 48) {
      CHECK((N + bn - 1) / bn * bn < (N + bn0 - 1) / bn0 * bn0,
            "N %d: %dx%d pads more than %dx%d", N, bm, bn, bm0, bn0);
      CHECK(2 * (bm + bn) * (64 + 8) * 2 <= 80 * 1024, "N %d: LDS", N);
    } else {
      CHECK(bm == bm0 && bn == bn0, "N %d: square pick changed", N);
    }
  }
}

}  // namespace

int main() {
  sweep_taps();
  sweep_cases();
  check_tiles();
  std::printf("%ld checks, %d failures\n", g_checks, g_fail);
  if (g_fail) return 1;
  std::printf("all gather-walk host checks passed\n");
  return 0;
}
