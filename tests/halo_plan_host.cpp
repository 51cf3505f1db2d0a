// Host check of the halo-tile conv plan (ps_halo.h, the header conv_halo.hip
// walks tiles, stages patches and addresses LDS with): every output pixel is
// owned by exactly one fragment lane of one tile, every fragment read at
// every tap hits the patch chunk that staging wrote for that input pixel,
// staging fills each 16 B of the patch exactly once, the LDS total is within
// the limit, and ineligible shapes are refused.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ps_halo.h"

#define CHECK(c) \
  if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); std::exit(1); }

struct Shape {
  int N, Ci, H, W, Co, kh, kw, ph, pw, blocks;
};

static void check(const Shape& s) {
  const HaloTiling t = ps_halo_tiling(s.N, s.Ci, s.H, s.W, s.Co, s.kh, s.kw, 1,
                                      1, s.ph, s.pw, 1, 2, s.blocks);
  CHECK(t.ok);
  CHECK(t.TH * t.TW == PS_HALO_TILE && t.TH % 4 == 0 && t.TW % 16 == 0);
  CHECK(t.lds == t.x_off + 2 * t.patch_bytes && t.lds <= PS_HALO_LDS_MAX);
  CHECK(t.x_off == s.Co * t.w_ld * 2 && t.x_off % 16 == 0);
  CHECK(t.nvec <= PS_HALO_NV * PS_HALO_THREADS && t.blocks <= s.blocks);
  CHECK((int64_t)t.blocks * t.tpb >= t.tiles &&
        (int64_t)(t.blocks - 1) * t.tpb < t.tiles);
  // staging: a bijection onto the patch's 16 B slots, chunks stay in a pixel
  std::vector<int> slot(t.nvec, 0);
  for (int idx = 0; idx < t.nvec; ++idx) {
    int pr, pc, c;
    ps_halo_vec(t, idx, &pr, &pc, &c);
    CHECK(pr >= 0 && pr < t.PH && pc >= 0 && pc < t.PW && c >= 0 && c < t.CH);
    const int off = ps_halo_lds_off(t, pr, pc, c);
    CHECK(off % 16 == 0 && off >= 0 && off + 16 <= t.patch_bytes);
    CHECK(off / 16 / t.CH == pr * t.PW + pc);
    ++slot[off / 16];
  }
  for (int v : slot) CHECK(v == 1);
  // coverage, and every read inside the patch at the pixel the tap wants
  std::vector<int> owned((size_t)s.N * t.Ho * t.Wo, 0);
  for (int64_t ti = 0; ti < t.tiles; ++ti) {
    const HaloTile tl = ps_halo_tile(t, ti);
    CHECK(tl.n >= 0 && tl.n < s.N && tl.oh0 < t.Ho && tl.ow0 < t.Wo);
    for (int w = 0; w < 4; ++w)
      for (int f = 0; f < 4; ++f)
        for (int l = 0; l < 16; ++l) {
          int row, col0;
          ps_halo_frag(t, w, f, &row, &col0);
          CHECK(row < t.TH && col0 + 15 < t.TW && col0 % 16 == 0);
          for (int ky = 0; ky < s.kh; ++ky)
            for (int kx = 0; kx < s.kw; ++kx) {
              const int pr = row + ky, pc = col0 + l + kx;
              CHECK(pr < t.PH && pc < t.PW);
              // the kernel's key ignores col0 (0 or 16)
              CHECK(((pc >> t.ksh) & t.kmask) ==
                    (((l + kx) >> t.ksh) & t.kmask));
            }
          const int oh = tl.oh0 + row, ow = tl.ow0 + col0 + l;
          if (oh < t.Ho && ow < t.Wo)
            ++owned[((size_t)tl.n * t.Ho + oh) * t.Wo + ow];
        }
  }
  for (int v : owned) CHECK(v == 1);
}

int main() {
  const Shape shapes[] = {
      {2, 64, 5, 5, 64, 3, 3, 1, 1, 256},   {2, 64, 19, 37, 64, 3, 3, 1, 1, 2},
      {2, 64, 19, 37, 64, 3, 3, 0, 0, 2},   {2, 64, 19, 37, 64, 3, 3, 2, 2, 2},
      {2, 32, 16, 16, 32, 5, 5, 2, 2, 256}, {2, 32, 9, 33, 64, 5, 5, 2, 2, 256},
      {2, 64, 9, 20, 48, 3, 1, 1, 0, 256},  {2, 96, 9, 20, 16, 3, 3, 1, 1, 3},
      {32, 64, 224, 224, 64, 3, 3, 1, 1, 256}};
  for (const Shape& s : shapes) check(s);
  // VGG conv1_2: the header comment's budget
  const HaloTiling v =
      ps_halo_tiling(32, 64, 224, 224, 64, 3, 3, 1, 1, 1, 1, 1, 2, 256);
  CHECK(v.TH == 8 && v.TW == 32 && v.x_off == 74752 &&
        v.patch_bytes == 43520 && v.lds == 161792 && v.tiles == 6272);
  // refused: fp32, groups, stride, 7x7, pad > k - 1, Ci % 32, Co % 16,
  // Co > 64, a filter bank that does not fit
  auto ok = [](int Ci, int Co, int k, int s, int p, int G, int eb) {
    return ps_halo_tiling(2, Ci, 20, 20, Co, k, k, s, s, p, p, G, eb, 256).ok;
  };
  CHECK(ok(64, 64, 3, 1, 1, 1, 2));
  CHECK(!ok(64, 64, 3, 1, 1, 1, 4) && !ok(64, 64, 3, 1, 1, 2, 2));
  CHECK(!ok(64, 64, 3, 2, 1, 1, 2) && !ok(32, 16, 7, 1, 3, 1, 2));
  CHECK(!ok(64, 64, 3, 1, 3, 1, 2) && !ok(48, 64, 3, 1, 1, 1, 2));
  CHECK(!ok(64, 24, 3, 1, 1, 1, 2) && !ok(64, 128, 3, 1, 1, 1, 2));
  CHECK(!ok(64, 64, 5, 1, 2, 1, 2));
  std::printf("all halo plan host checks passed\n");
  return 0;
}
