// Halo-tile direct convolution (conv_halo.hip): tile walk, staged-patch
// addressing and LDS sizing, shared by the planner (ps_conv_plan.h), the
// kernel and a stand-alone host program (tests/halo_plan_host.cpp). Plain
// C++, no torch / HIP includes.
//
// A TILE is a TH x TW rectangle of output pixels of one image, 256 pixels
// (8 x 32, or 16 x 16 when the image is at most 16 wide or two 8 x 32 patches
// do not fit). Tile indices run image by image, inside an image column strip
// by column strip, top to bottom: a block's consecutive tiles walk down a
// strip, so the vertical halo it re-reads is what it has just read.
//
// The tile's input PATCH is PH x PW pixels (PH = TH + kh - 1, PW = TW + kw -
// 1) of Ci channels, patch pixel (pr, pc) being input pixel (oh0 - ph + pr,
// ow0 - pw + pc), zeros outside the image. In LDS a pixel is CH = Ci / 8
// chunks of 16 B with NO padding between pixels; chunk c of pixel (pr, pc)
// sits at
//   ((pr * PW + pc) * CH + (c ^ key(pc))) * 16,  key(pc) = (pc >> ksh) & kmask
// The XOR keeps a chunk inside its pixel and inside its aligned group of
// kmask + 1 chunks (CH is a multiple of 4, kmask is 3, 7 or 15 and never
// exceeds CH - 1 rounded down to such a group).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PS_HALO_HD __host__ __device__
#else
#define PS_HALO_HD
#endif

constexpr int PS_HALO_THREADS = 256;      // 4 waves, 64 pixels x all Co each
constexpr int PS_HALO_TILE = 256;         // output pixels per tile
constexpr int PS_HALO_NV = 16;            // staged 16 B vectors per thread
constexpr int PS_HALO_MAX_CO = 64;        // 4 weight fragments of 16
constexpr int PS_HALO_MAX_K = 5;          // kh, kw
constexpr int PS_HALO_LDS_MAX = 160 << 10;
constexpr int PS_HALO_WPAD = 8;           // LDS weight rows: K + 8 elements

struct HaloTiling {
  int Ci, H, W, Co, Ho, Wo, kh, kw, ph, pw;
  int K;               // kh * kw * Ci, a multiple of 32
  int TH, TW;          // tile
  int PH, PW, CH;      // patch rows, patch pixels per row, chunks per pixel
  int ksh, kmask;      // swizzle key of a patch column
  int tiles_y, tiles_x, tiles_per_img;
  int64_t tiles;       // N * tiles_per_img
  int nvec;            // 16 B vectors of one patch: PH * PW * CH
  // LDS: [weights Co x w_ld][patch 0][patch 1]
  int w_ld;            // elements per LDS weight row
  int x_off;           // byte offset of patch 0
  int patch_bytes;
  int lds;             // total bytes
  int blocks, tpb;     // persistent grid: blocks x tpb consecutive tiles
  bool ok;
};

struct HaloTile {
  int n, oh0, ow0;
};

// max_blocks: cap on the persistent grid (the CU count); it does not bear on
// ok, so a planner may pass 1
inline HaloTiling ps_halo_tiling(int N, int Ci, int H, int W, int Co, int kh,
                                 int kw, int sh, int sw, int ph, int pw,
                                 int G, int elem_bytes, int max_blocks) {
  HaloTiling t{};
  t.Ci = Ci; t.H = H; t.W = W; t.Co = Co; t.kh = kh; t.kw = kw;
  t.ph = ph; t.pw = pw;
  if (elem_bytes != 2 || G != 1 || sh != 1 || sw != 1 || kh < 1 || kw < 1 ||
      kh > PS_HALO_MAX_K || kw > PS_HALO_MAX_K || ph < 0 || pw < 0 ||
      ph > kh - 1 || pw > kw - 1 || Ci <= 0 || Ci % 32 || Co <= 0 ||
      Co % 16 || Co > PS_HALO_MAX_CO || N <= 0 || max_blocks <= 0)
    return t;
  t.Ho = H + 2 * ph - kh + 1;
  t.Wo = W + 2 * pw - kw + 1;
  // one image of either tensor is indexed with an int
  if (t.Ho <= 0 || t.Wo <= 0 || (int64_t)H * W * Ci >= (1LL << 31) ||
      (int64_t)t.Ho * t.Wo * Co >= (1LL << 31))
    return t;
  t.K = kh * kw * Ci;
  t.CH = Ci / 8;
  // 16 lanes of an A fragment read 16 consecutive patch columns: the key
  // spreads them over all 64 banks (conv_halo.hip counts them)
  t.ksh = t.CH == 8 ? 1 : t.CH >= 16 && t.CH % 16 == 0 ? 0 : 2;
  t.kmask = t.CH == 8 ? 7 : t.CH >= 16 && t.CH % 16 == 0 ? 15 : 3;
  t.w_ld = t.K + PS_HALO_WPAD;
  const int64_t wbytes = (int64_t)Co * t.w_ld * 2;
  const int cand[2][2] = {{8, 32}, {16, 16}};
  for (int c = t.Wo <= 16 ? 1 : 0; c < 2 && !t.ok; ++c) {
    t.TH = cand[c][0];
    t.TW = cand[c][1];
    t.PH = t.TH + kh - 1;
    t.PW = t.TW + kw - 1;
    t.nvec = t.PH * t.PW * t.CH;
    const int64_t patch = (int64_t)t.nvec * 16;
    t.ok = wbytes + 2 * patch <= PS_HALO_LDS_MAX &&
           t.nvec <= PS_HALO_NV * PS_HALO_THREADS;
    t.patch_bytes = (int)patch;
  }
  if (!t.ok) return t;
  t.x_off = (int)wbytes;
  t.lds = t.x_off + 2 * t.patch_bytes;
  t.tiles_y = (t.Ho + t.TH - 1) / t.TH;
  t.tiles_x = (t.Wo + t.TW - 1) / t.TW;
  t.tiles_per_img = t.tiles_y * t.tiles_x;
  t.tiles = (int64_t)N * t.tiles_per_img;
  int64_t b = max_blocks < t.tiles ? max_blocks : t.tiles;
  t.tpb = (int)((t.tiles + b - 1) / b);
  t.blocks = (int)((t.tiles + t.tpb - 1) / t.tpb);
  return t;
}

PS_HALO_HD inline HaloTile ps_halo_tile(const HaloTiling& t, int64_t ti) {
  HaloTile r;
  r.n = (int)(ti / t.tiles_per_img);
  const int rem = (int)(ti - (int64_t)r.n * t.tiles_per_img);
  const int strip = rem / t.tiles_y;
  r.oh0 = (rem - strip * t.tiles_y) * t.TH;
  r.ow0 = strip * t.TW;
  return r;
}

// LDS byte offset, inside a patch, of chunk c of patch pixel (pr, pc)
PS_HALO_HD inline int ps_halo_lds_off(const HaloTiling& t, int pr, int pc,
                                      int c) {
  return ((pr * t.PW + pc) * t.CH + (c ^ ((pc >> t.ksh) & t.kmask))) * 16;
}

// staged vector idx (0 <= idx < nvec) -> patch pixel and chunk; consecutive
// idx are consecutive 16 B of the input while a patch row lasts
PS_HALO_HD inline void ps_halo_vec(const HaloTiling& t, int idx, int* pr,
                                   int* pc, int* c) {
  const int pix = idx / t.CH;
  *c = idx - pix * t.CH;
  *pr = pix / t.PW;
  *pc = pix - *pr * t.PW;
}

// A wave owns 4 A fragments of 16 horizontally consecutive pixels: fragment
// f of wave w covers tile row w * (TH / 4) + f / (TW / 16), tile columns
// (f % (TW / 16)) * 16 .. + 15
PS_HALO_HD inline void ps_halo_frag(const HaloTiling& t, int wave, int f,
                                    int* row, int* col0) {
  const int xf = t.TW / 16;
  *row = wave * (t.TH / 4) + f / xf;
  *col0 = (f % xf) * 16;
}

// Weight rows are staged so that a lane's accumulators are consecutive output
// channels: fragment fn's row i holds output channel ps_halo_co(FN, fn, i).
// Fragments pair up (2j, 2j + 1) over 32 channels -- rows 4q .. 4q + 3 of the
// pair hold channels 32j + 8q .. + 3 and + 4 .. + 7, one 16 B store per lane;
// an unpaired last fragment keeps its 16 channels in order (8 B stores).
PS_HALO_HD inline int ps_halo_co(int FN, int fn, int i) {
  if ((fn | 1) < FN)
    return (fn >> 1) * 32 + (i >> 2) * 8 + (fn & 1) * 4 + (i & 3);
  return fn * 16 + i;
}
