// Row-fused first-layer convolution: tile walk, staged-row addressing and LDS
// sizing, shared by the planner (ps_conv_plan.h), the kernels
// (conv_rowfused.hip) and two stand-alone host programs
// (tests/rowfused_plan_host.cpp, tests/rowfused_stage_host.cpp). Plain C++,
// no torch / HIP includes.
//
// A TILE is PS_RF_TM consecutive output positions of one image:
//   full-row mode (Wo <= TM): R = min(TM / Wo, Ho) whole output rows,
//     WS = Wo; position p of the tile is output (oh0 + p / WS, p % WS)
//   segment mode (Wo > TM):   R = 1, WS = TM columns of one output row,
//     the last segment of a row ragged; position p is output (oh0, ow0 + p)
// Either way position p is element (n*Ho + oh0)*Wo + ow0 + p of the NHWC
// rows of y / dy, live while p < nlive.
//
// The tile's input window is STAGED in LDS channel-planar, as srows * C
// lines of rsw_ld bf16: line sr*C + c holds channel c of input row
// ih = oh0*sh - ph + sr, its element w is pixel iw = ow0*sw - pw + w; pixels
// outside the image are zeros. Planar, because the data blob is NCHW: a line
// is then one contiguous run of x and stages with 16 B loads (ps_rf_vec
// below). An interleaved image, whose operand reads would be contiguous, has
// not been measured with such loads; the one form tried staged it with a
// 2-byte load per element. The
// im2col entry (position p, k = (ky, kx, c)) is the staged element
// pbase(p) + koff(k)  with
//   pbase(p) = (p / WS)*sh*C*rsw_ld + (p % WS)*sw
//   koff(k)  = ((k / RUN)*C + k % C)*rsw_ld + (k % RUN) / C,   RUN = kw*C
// and k >= Kcol (the pad columns of the khwc rows) is a zero.
#pragma once
#include <cstdint>

constexpr int PS_RF_TM = 128;             // output positions per tile
constexpr int PS_RF_THREADS = 512;        // block size of both kernels
// the wgrad stages through registers: 16 B vectors per thread of the x
// window and of the dy tile (PS_RF_TM * 128 / 8 / PS_RF_THREADS at most)
constexpr int PS_RF_XV = 3;
constexpr int PS_RF_DV = 4;
constexpr int PS_RF_MAX_CO = 128;         // weights stay in LDS / registers
constexpr int PS_RF_LDS_MAX = 160 << 10;  // one workgroup may take it all
constexpr int PS_RF_HDR = 16;             // zero bytes ahead of a staged image
constexpr int PS_RF_WPAD = 8;             // LDS weight rows: Kpad + 8 elems
constexpr int PS_RF_DYPAD = 8;            // LDS dy rows: Cop + 8 elems
// byte offset that sends a staged read to the zero header (see rf_addr)
constexpr int PS_RF_NEG = -(1 << 24);

struct RowFusedTiling {
  int C, H, W, Ho, Wo, kh, kw, sh, sw, ph, pw;
  int Co, Cop;        // Cop: Co rounded up to a built fragment count x 16
  int Kcol, Kpad;     // im2col row length and the khwc row width (wk_ld)
  int RUN;            // kw * C: elements of one kernel row
  int R, WS, segs;    // rows per tile, columns per tile, tiles per row strip
  int row_tiles;      // ceil(Ho / R)
  int tiles_per_img;  // row_tiles * segs
  int64_t tiles;      // N * tiles_per_img
  int srows;          // staged input rows: (R - 1)*sh + kh
  int rsw;            // staged pixels a line needs: (WS - 1)*sw + kw
  int rsw_ld;         // line stride: rsw rounded up to 8 (16 B stores)
  int xs_bytes;       // one staged image, zero header included
  int w_ld, dy_ld;    // LDS row strides of the weights / the dy tile
  // forward: [weights][koff table][2 staged images]
  int fwd_koff_off, fwd_xs_off, fwd_lds;
  // wgrad: [2 position tables][2 dy tiles][2 staged images]
  int wg_dy_off, wg_xs_off, wg_lds;
  bool ok;            // shape supported and both kernels fit the LDS
};

struct RowFusedTile {
  int n, oh0, ow0;
  int nlive;          // live positions: p < nlive
  int64_t pos0;       // NHWC row index of position 0
};

inline int ps_rf_round_up(int v, int m) { return (v + m - 1) / m * m; }
// the kernels are built for 1, 2, 4, 6 and 8 column fragments of 16
inline int ps_rf_co_pad(int Co) {
  return Co <= 16 ? 16 : Co <= 32 ? 32 : Co <= 64 ? 64 : Co <= 96 ? 96 : 128;
}

inline RowFusedTiling ps_rowfused_tiling(int N, int C, int H, int W, int Co,
                                         int kh, int kw, int sh, int sw,
                                         int ph, int pw, int Kpad) {
  RowFusedTiling t{};
  t.C = C; t.H = H; t.W = W; t.kh = kh; t.kw = kw; t.sh = sh; t.sw = sw;
  t.ph = ph; t.pw = pw;
  t.Ho = (H + 2 * ph - kh) / sh + 1;
  t.Wo = (W + 2 * pw - kw) / sw + 1;
  t.Co = Co;
  t.Cop = ps_rf_co_pad(Co);
  t.RUN = kw * C;
  t.Kcol = kh * t.RUN;
  t.Kpad = Kpad;
  if (t.Ho <= 0 || t.Wo <= 0 || Co <= 0 || Co > PS_RF_MAX_CO || Co % 8 ||
      Kpad % 64 || Kpad < t.Kcol || N <= 0)
    return t;
  if (t.Wo <= PS_RF_TM) {
    t.R = PS_RF_TM / t.Wo < t.Ho ? PS_RF_TM / t.Wo : t.Ho;
    t.WS = t.Wo;
    t.segs = 1;
  } else {
    t.R = 1;
    t.WS = PS_RF_TM;
    t.segs = (t.Wo + PS_RF_TM - 1) / PS_RF_TM;
  }
  t.row_tiles = (t.Ho + t.R - 1) / t.R;
  t.tiles_per_img = t.row_tiles * t.segs;
  t.tiles = (int64_t)N * t.tiles_per_img;
  t.srows = (t.R - 1) * sh + kh;
  t.rsw = (t.WS - 1) * sw + kw;
  t.rsw_ld = ps_rf_round_up(t.rsw, 8);
  const int64_t xs = PS_RF_HDR + (int64_t)t.srows * C * t.rsw_ld * 2;
  t.w_ld = Kpad + PS_RF_WPAD;
  t.dy_ld = t.Cop + PS_RF_DYPAD;
  const int64_t wbytes = (int64_t)t.Cop * t.w_ld * 2;
  const int64_t fwd = wbytes + (int64_t)Kpad * 4 + 2 * xs;
  const int64_t dyb = (int64_t)PS_RF_TM * t.dy_ld * 2;
  const int64_t wg = 2 * (int64_t)PS_RF_TM * 4 + 2 * dyb + 2 * xs;
  if (fwd > PS_RF_LDS_MAX || wg > PS_RF_LDS_MAX) return t;
  if ((int64_t)t.srows * C * (t.rsw_ld / 8) > PS_RF_THREADS * PS_RF_XV)
    return t;
  t.xs_bytes = (int)xs;
  t.fwd_koff_off = (int)wbytes;
  t.fwd_xs_off = (int)(wbytes + Kpad * 4);
  t.fwd_lds = (int)fwd;
  t.wg_dy_off = 2 * PS_RF_TM * 4;
  t.wg_xs_off = (int)(t.wg_dy_off + 2 * dyb);
  t.wg_lds = (int)wg;
  t.ok = true;
  return t;
}

#if defined(__HIPCC__)
#define PS_RF_HD __host__ __device__
#else
#define PS_RF_HD
#endif

// tile index -> where it sits. A block's tiles are consecutive indices:
// consecutive row strips of one image, whose input windows overlap.
PS_RF_HD inline RowFusedTile ps_rf_tile(const RowFusedTiling& t, int64_t ti) {
  RowFusedTile r;
  r.n = (int)(ti / t.tiles_per_img);
  const int rem = (int)(ti - (int64_t)r.n * t.tiles_per_img);
  const int strip = rem / t.segs;
  r.oh0 = strip * t.R;
  r.ow0 = (rem - strip * t.segs) * t.WS;
  const int rows = t.Ho - r.oh0 < t.R ? t.Ho - r.oh0 : t.R;
  const int cols = t.Wo - r.ow0 < t.WS ? t.Wo - r.ow0 : t.WS;
  r.nlive = t.segs == 1 ? rows * t.WS : cols;
  r.pos0 = ((int64_t)r.n * t.Ho + r.oh0) * t.Wo + r.ow0;
  return r;
}

// staged BYTE offsets, relative to a staged image's zero header
PS_RF_HD inline int ps_rf_pbase(const RowFusedTiling& t, int p) {
  return PS_RF_HDR +
         ((p / t.WS) * t.sh * t.C * t.rsw_ld + (p % t.WS) * t.sw) * 2;
}
PS_RF_HD inline int ps_rf_koff(const RowFusedTiling& t, int k) {
  if (k >= t.Kcol) return PS_RF_NEG;
  return (((k / t.RUN) * t.C + k % t.C) * t.rsw_ld + (k % t.RUN) / t.C) * 2;
}
// the byte a read uses: a dead position (pbase = PS_RF_NEG) or a pad column
// lands on the zero header, everything else inside the staged rows
PS_RF_HD inline int ps_rf_addr(int pbase, int koff) {
  const int a = pbase + koff;
  return a < 0 ? 0 : a;
}

// ---- staging one 16 B vector of a window ----------------------------------
// x as the kernels see it: element strides, and the element span of the
// tensor from its first element, 1 + sum (size_i - 1) * stride_i. Elements
// [0, span) are mapped memory of x's storage whatever the layout; nothing
// else may be touched.
struct RowFusedX {
  int64_t sn;      // image stride
  int sc, sh, sw;  // strides inside one image (one image spans < 2^31)
  int64_t span;
};

// Vector idx of a tile's staged image is pixels iw .. iw + 7 of channel c of
// input row ih (idx -> line rc = idx / (rsw_ld / 8), rc -> (sr, c)). How it
// is fetched:
//   ZERO:   the row is outside the image, idx is past the window, or none of
//           the 8 pixels is inside the row. No load.
//   WIDE:   sw == 1 and the 8 elements at off lie inside [0, span), whether
//           or not they lie inside the row: ONE 16 B load (2-byte aligned).
//           Pixels past a row end are the next row's first, pixels before a
//           row start the previous row's last: memory of the same tensor.
//   NARROW: the rest -- the few vectors at the two ends of the span, and any
//           layout with sw != 1. 8 two-byte loads, element j from pixel
//           clamp(iw + j, 0, W - 1) of the row (ps_rf_narrow_off).
// Either way elements outside [lo, hi) are zeroed in registers afterwards
// (ps_rf_elem_mask), so the staged bytes are the window of the header
// comment: pixels outside the image are zeros.
enum { PS_RF_ZERO = 0, PS_RF_WIDE = 1, PS_RF_NARROW = 2 };

struct RowFusedVec {
  int kind;
  int lo, hi;   // live elements of the 8: lo <= j < hi
  int iw;       // pixel of element 0 (may be negative)
  int64_t off;  // WIDE: element 0; NARROW: pixel 0 of the row
};

// the part of the decision that does not depend on the tile: which staged
// row and column vector idx is, and its row's offset from the window's
// first row. A kernel keeps these across its tiles (two divisions saved per
// vector and tile).
struct RowFusedVecPos {
  int sr;     // staged row
  int col;    // column of element 0 inside the staged line
  int rel;    // sr * sh + c * sc, in elements of x
  bool live;  // idx is inside the window
};

PS_RF_HD inline RowFusedVecPos ps_rf_vec_pos(const RowFusedTiling& t,
                                             const RowFusedX& X, int idx) {
  RowFusedVecPos p;
  const int vpr = t.rsw_ld / 8;
  const int rc = idx / vpr;
  p.sr = rc / t.C;
  p.col = (idx - rc * vpr) * 8;
  p.rel = p.sr * X.sh + (rc - p.sr * t.C) * X.sc;
  p.live = idx < t.srows * t.C * vpr;
  return p;
}

PS_RF_HD inline RowFusedVec ps_rf_vec_at(const RowFusedTiling& t,
                                         const RowFusedTile& tl,
                                         const RowFusedX& X,
                                         const RowFusedVecPos& p) {
  RowFusedVec d;
  const int ih0 = tl.oh0 * t.sh - t.ph;
  const int ih = ih0 + p.sr;
  d.iw = tl.ow0 * t.sw - t.pw + p.col;
  d.lo = d.iw < 0 ? (d.iw < -8 ? 8 : -d.iw) : 0;
  d.hi = t.W - d.iw < 8 ? (t.W - d.iw < 0 ? 0 : t.W - d.iw) : 8;
  d.kind = PS_RF_ZERO;
  d.off = 0;
  if (!p.live || ih < 0 || ih >= t.H || d.lo >= d.hi) {
    d.lo = d.hi = 0;
    return d;
  }
  const int64_t row = tl.n * X.sn + (ih0 * X.sh + p.rel);
  const int64_t first = row + d.iw;
  if (X.sw == 1 && first >= 0 && first + 8 <= X.span) {
    d.kind = PS_RF_WIDE;
    d.off = first;
  } else {
    d.kind = PS_RF_NARROW;
    d.off = row;
  }
  return d;
}

PS_RF_HD inline RowFusedVec ps_rf_vec(const RowFusedTiling& t,
                                      const RowFusedTile& tl,
                                      const RowFusedX& X, int idx) {
  return ps_rf_vec_at(t, tl, X, ps_rf_vec_pos(t, X, idx));
}

// NARROW: the element that stands in for element j (a live j is its own
// pixel; a dead one repeats the row's nearest pixel and is masked away)
PS_RF_HD inline int64_t ps_rf_narrow_off(const RowFusedTiling& t,
                                         const RowFusedVec& d, int sw, int j) {
  int px = d.iw + j;
  px = px < 0 ? 0 : px > t.W - 1 ? t.W - 1 : px;
  return d.off + (int64_t)px * sw;
}

// bit j set: element j of the vector is kept
PS_RF_HD inline unsigned ps_rf_elem_mask(int lo, int hi) {
  return ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}
