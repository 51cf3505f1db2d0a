// Implicit-GEMM gather arithmetic: im2col row -> pixel, im2col column -> tap,
// and the walk that moves a tap along k by adds instead of divisions. Plain
// integer C++ (no torch / HIP includes): the gather GEMM's staging,
// gather_addr and the host test (tests/gather_walk_host.cpp) all call the
// same functions.
//
// An im2col element (row, k) of group slice k = (kkh * kw + kkw) * Cg + cg
// lives at element offset
//     ((n * H + ih0 + kkh) * W + iw0 + kkw) * C + c0 + cg
//   =  row part                          + tap part
//     ((n * H + ih0) * W + iw0) * C      + (kkh * W + kkw) * C + c0 + cg
// of the gathered NHWC tensor, with (n, oh, ow) = decode(row),
// ih0 = oh * sh - ph, iw0 = ow * sw - pw. The row part never changes over k
// and the tap part is the same for every row, so a lane that stages the same
// rows for every k-tile keeps the row parts and moves ONE tap.
#pragma once
#include <cstdint>

#include "ps_conv_plan.h"  // PS_HD, GatherDesc

// exact unsigned divide by a small runtime constant via f32 reciprocal +
// fixup (x < 2^24; integer division is ~40 cycles each on the device)
PS_HD inline int ps_fdiv_fix(int x, int d, float inv, int& rem) {
  int q = (int)((float)x * inv);
  rem = x - q * d;
  if (rem < 0) { --q; rem += d; }
  else if (rem >= d) { ++q; rem -= d; }
  return q;
}

// Row part. `base` is the element offset of pixel (n, ih0, iw0), channel 0;
// it is negative or past a row's end for rows whose window starts in the
// padding -- only in-bounds (row, tap) sums are ever dereferenced.
struct GatherRow {
  int64_t base;
  int ih0, iw0;
};

PS_HD inline GatherRow ps_gather_row(const GatherDesc& g, int row) {
  int ow, oh;
  const int t = ps_fdiv_fix(row, g.Wo, g.inv_Wo, ow);
  const int n = ps_fdiv_fix(t, g.Ho, g.inv_Ho, oh);
  GatherRow r;
  r.ih0 = oh * g.sh - g.ph;
  r.iw0 = ow * g.sw - g.pw;
  r.base = (((int64_t)n * g.H + r.ih0) * g.W + r.iw0) * g.C;
  return r;
}

// Tap part: the decoded column and its element offset (never negative).
struct GatherTap {
  int kkh, kkw, cg;
  int off;  // (kkh * W + kkw) * C + c0 + cg
};

PS_HD inline GatherTap ps_gather_tap(const GatherDesc& g, int k) {
  GatherTap t;
  const int khw = ps_fdiv_fix(k, g.Cg, g.inv_Cg, t.cg);
  t.kkh = ps_fdiv_fix(khw, g.kw, g.inv_kw, t.kkw);
  t.off = (t.kkh * g.W + t.kkw) * g.C + g.c0 + t.cg;
  return t;
}

// Most cg wraps one step of `step` columns can take.
PS_HD inline int ps_gather_max_wraps(int Cg, int step) {
  return (Cg - 1 + step) / Cg;
}

// Move the tap of column k to column k + step. Up to two cg wraps (Cg >=
// step / 2: every AlexNet / VGG layer at the 64-deep bf16 tile) go by
// compare-and-carry, every lane running the same two straight-line steps;
// narrower groups would need a lane-divergent carry chain up to step / Cg
// long and re-decode instead. Walks past kh on the zero-padded columns
// (k >= kg_max) like the decode does.
PS_HD inline void ps_gather_tap_advance(const GatherDesc& g, GatherTap& t,
                                        int k, int step) {
  if (ps_gather_max_wraps(g.Cg, step) > 2) {
    t = ps_gather_tap(g, k + step);
    return;
  }
  t.cg += step;
  t.off += step;
  for (int i = 0; i < 2; ++i) {
    const bool wc = t.cg >= g.Cg;  // into the next pixel of the tap row
    t.cg -= wc ? g.Cg : 0;
    t.kkw += wc ? 1 : 0;
    t.off += wc ? g.C - g.Cg : 0;
    const bool ww = t.kkw >= g.kw;  // into the next tap row
    t.kkw -= ww ? g.kw : 0;
    t.kkh += ww ? 1 : 0;
    t.off += ww ? (g.W - g.kw) * g.C : 0;
  }
}

// Padding test of (row, tap) at column k. The column test is part of it:
// padded columns decode to taps past kh and must read the zero page whether
// or not that pixel exists.
// The pixel test alone is ps_gather_pad (bitwise |: no branches), for a
// caller that hoists the column test out of its row loop.
PS_HD inline bool ps_gather_pad(const GatherDesc& g, int ih0, int iw0,
                                const GatherTap& t) {
  return ((unsigned)(ih0 + t.kkh) >= (unsigned)g.H) |
         ((unsigned)(iw0 + t.kkw) >= (unsigned)g.W);
}
PS_HD inline bool ps_gather_oob(const GatherDesc& g, const GatherRow& r,
                                const GatherTap& t, int k) {
  return (k >= g.kg_max) | ps_gather_pad(g, r.ih0, r.iw0, t);
}

// element offset into the gathered tensor (valid iff !ps_gather_oob)
PS_HD inline int64_t ps_gather_offset(const GatherRow& r, const GatherTap& t) {
  return r.base + t.off;
}
