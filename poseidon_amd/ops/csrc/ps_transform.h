// DataTransformer on the device: index walk and per-element arithmetic of
//     out[n,c,h,w] = (float(raw[n,c,h+h_off,ws]) - mean[c,h+h_off,ws]) * scale
//     ws = w_off + w, or w_off + Wo-1-w when the image is mirrored
// (the mean is indexed at the SOURCE position). Plain C++ (no torch / HIP
// includes): transform.hip's kernel and the host test
// (tests/transform_walk_host.cpp) both run ps_transform_group.
//
// A thread owns 8 consecutive elements of the FLAT [N,C,Ho,Wo] output, so its
// 16-byte store is aligned whatever Wo is. It decodes (n,c,h,w) of its first
// element once (the only divisions) and then walks: w++, wrapping into h++,
// c++, n++. One fp32 subtract, one fp32 multiply per element, in that order,
// so the result equals numpy's (arr - mean)[crop][mirror] * scale bit for bit.
#pragma once
#include <cstdint>

#include "ps_conv_plan.h"  // PS_HD

#if defined(__FAST_MATH__)
#error "ps_transform.h promises numpy's fp32 results: no fast-math"
#endif

enum : int {
  PS_MEAN_NONE = 0,     // mean unused
  PS_MEAN_SCALAR = 1,   // mean[0]
  PS_MEAN_CHANNEL = 2,  // mean[c]
  PS_MEAN_IMAGE = 3,    // mean[C][H][W]
};

constexpr int PS_TRANSFORM_VEC = 8;  // outputs per thread

struct TransformGeom {
  int N, C, H, W;  // raw [N,C,H,W] uint8
  int Ho, Wo;      // out [N,C,Ho,Wo]; Ho <= H, Wo <= W
  int mean_mode;
  float scale;
};

struct TransformCursor {
  int n, c, h, w;           // output position
  int h_off, w_off, flip;   // image n's draw
  int64_t row;              // raw offset of source row (n, c, h + h_off)
  int mrow;                 // mean-image offset of source row (c, h + h_off)
};

// image n's (h_off, w_off, flip) from params[N][3]. Offsets are clamped into
// the source so that no params content can make the kernel read outside raw.
PS_HD inline void ps_transform_image(const TransformGeom& g, const int* params,
                                     TransformCursor& p) {
  int ho = params[3 * (int64_t)p.n], wo = params[3 * (int64_t)p.n + 1];
  const int hmax = g.H - g.Ho, wmax = g.W - g.Wo;
  p.h_off = ho < 0 ? 0 : (ho > hmax ? hmax : ho);
  p.w_off = wo < 0 ? 0 : (wo > wmax ? wmax : wo);
  p.flip = params[3 * (int64_t)p.n + 2] != 0;
}

PS_HD inline void ps_transform_row(const TransformGeom& g, TransformCursor& p) {
  const int hs = p.h + p.h_off;
  p.mrow = (p.c * g.H + hs) * g.W;
  p.row = (((int64_t)p.n * g.C + p.c) * g.H + hs) * g.W;
}

PS_HD inline TransformCursor ps_transform_decode(const TransformGeom& g,
                                                 const int* params,
                                                 int64_t flat) {
  TransformCursor p;
  p.w = (int)(flat % g.Wo);
  int64_t t = flat / g.Wo;
  p.h = (int)(t % g.Ho);
  t /= g.Ho;
  p.c = (int)(t % g.C);
  p.n = (int)(t / g.C);
  ps_transform_image(g, params, p);
  ps_transform_row(g, p);
  return p;
}

// step to the next flat element; only called while one remains, so p.n < N
// whenever params are read
PS_HD inline void ps_transform_next(const TransformGeom& g, const int* params,
                                    TransformCursor& p) {
  if (++p.w < g.Wo) return;
  p.w = 0;
  if (++p.h == g.Ho) {
    p.h = 0;
    if (++p.c == g.C) {
      p.c = 0;
      ++p.n;
      ps_transform_image(g, params, p);
    }
  }
  ps_transform_row(g, p);
}

PS_HD inline float ps_transform_value(const TransformGeom& g,
                                      const TransformCursor& p,
                                      const uint8_t* raw, const float* mean) {
  const int ws = p.w_off + (p.flip ? g.Wo - 1 - p.w : p.w);
  const float v = (float)raw[p.row + ws];
  float m = 0.f;
  if (g.mean_mode == PS_MEAN_SCALAR) m = mean[0];
  else if (g.mean_mode == PS_MEAN_CHANNEL) m = mean[p.c];
  else if (g.mean_mode == PS_MEAN_IMAGE) m = mean[p.mrow + ws];
  const float d = v - m;
  return d * g.scale;
}

// A whole group inside one output row (p.w + 8 <= Wo) reads 8 CONSECUTIVE
// source bytes and mean values, backwards when mirrored: fetched as two
// blocks (wide loads on the device) and reversed in registers.
PS_HD inline void ps_transform_row8(const TransformGeom& g,
                                    const TransformCursor& p,
                                    const uint8_t* raw, const float* mean,
                                    float* v) {
  constexpr int V = PS_TRANSFORM_VEC;
  // lowest source column of the group: Wo-1-(w+7) when mirrored
  const int ws0 = p.w_off + (p.flip ? g.Wo - V - p.w : p.w);
  uint8_t b[V];
  float m[V];
  __builtin_memcpy(b, raw + p.row + ws0, sizeof b);
  if (g.mean_mode == PS_MEAN_IMAGE) {
    __builtin_memcpy(m, mean + p.mrow + ws0, sizeof m);
  } else {
    const float c = g.mean_mode == PS_MEAN_SCALAR    ? mean[0]
                    : g.mean_mode == PS_MEAN_CHANNEL ? mean[p.c] : 0.f;
    for (int j = 0; j < V; ++j) m[j] = c;
  }
  for (int j = 0; j < V; ++j) {  // constant indices only: stays in registers
    const float x = p.flip ? (float)b[V - 1 - j] : (float)b[j];
    const float y = p.flip ? m[V - 1 - j] : m[j];
    const float d = x - y;
    v[j] = d * g.scale;
  }
}

// the `count` (1..8) outputs from flat index flat0 on, as fp32
PS_HD inline void ps_transform_group(const TransformGeom& g,
                                     const uint8_t* raw, const int* params,
                                     const float* mean, int64_t flat0,
                                     int count, float* v) {
  TransformCursor p = ps_transform_decode(g, params, flat0);
  if (count == PS_TRANSFORM_VEC && p.w + PS_TRANSFORM_VEC <= g.Wo) {
    ps_transform_row8(g, p, raw, mean, v);
    return;
  }
  for (int j = 0; j < count; ++j) {
    if (j) ps_transform_next(g, params, p);
    v[j] = ps_transform_value(g, p, raw, mean);
  }
}
