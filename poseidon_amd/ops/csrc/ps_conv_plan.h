// Convolution plan: every layout decision of the conv pipeline (column
// stride, padded weight width, implicit-GEMM choice, dgrad-as-forward
// choice) derived ONCE from the problem shape. Plain C++ (no torch / HIP
// includes) so it also compiles into a stand-alone host program.
#pragma once
#include <cstdint>

#include "ps_rowfused.h"

#if defined(__HIPCC__)
#define PS_HD __host__ __device__
#else
#define PS_HD
#endif

struct ConvGeom {
  int N, C, H, W;
  int Ho, Wo;
  int kh, kw, sh, sw, ph, pw;
  int G;
};

// Implicit-GEMM gather descriptor: the GEMM's A operand (conv fwd) or
// K-major B operand (conv wgrad) is the im2col matrix, gathered on the fly
// from NHWC x instead of materialized. Out-of-bounds (padding) lanes load
// from a 16-byte zero page.
struct GatherDesc {
  const void* x;      // NHWC activations
  const void* zero;   // >=16B of zeros
  int C, H, W, Ho, Wo;
  int kh, kw, sh, sw, ph, pw;
  int Cg, c0;         // group channel count and channel offset
  int kg_max;         // k >= kg_max reads the zero page (padded N/K)
  // f32 reciprocals for division-free index decode (exact with the +-1
  // fixup in the kernel; operands < 2^24)
  float inv_Cg, inv_kw, inv_Wo, inv_Ho;
};

inline void ps_fill_gather_inv(GatherDesc* g) {
  g->inv_Cg = 1.0f / g->Cg;
  g->inv_kw = 1.0f / g->kw;
  g->inv_Wo = 1.0f / g->Wo;
  g->inv_Ho = 1.0f / g->Ho;
}

struct ConvPolicy {
  bool force_implicit;      // global implicit-GEMM switch
  int64_t implicit_bytes;   // colT above this goes implicit per layer
  int64_t dgrad_fwd_bytes;  // dcolT above this runs dgrad as a forward conv
  bool packed;              // packed small-channel first-layer switch
  // row-fused small-channel first layers (ps_rowfused.h): switch, the colT
  // size above which a layer takes the path, and deterministic mode, which
  // keeps it off (its wgrad adds floats atomically)
  bool rowfused;
  int64_t rowfused_bytes;
  bool deterministic;
};

// Packed first-layer layout (G==1, C <= 4, even sw): x is copied once into
// xp[N][H][Wp][8], each 16 B chunk holding two horizontally adjacent pixels
// of PS_PK_SLOTS channel slots, the left padding pw baked in as zero pixels.
// The kh x kw / stride (sh, sw) conv over x is then EXACTLY a
// kh x ceil(kw/2) / stride (sh, sw/2) / pad (ph, 0) conv with 8 channels
// over xp, which the gather GEMMs run with 16 B-aligned chunks and no
// column matrix. Unused slots and the phantom tap kx == kw of an odd kw
// carry zero weights.
constexpr int PS_PK_SLOTS = 4;               // channel slots per pixel
constexpr int PS_PK_C = 2 * PS_PK_SLOTS;     // channels of xp (one chunk)

// pixel iw of x -> chunk and half-chunk of an xp row
PS_HD inline int ps_pk_chunk(int iw, int pw) { return (iw + pw) >> 1; }
PS_HD inline int ps_pk_half(int iw, int pw) { return (iw + pw) & 1; }
// element index of x[n][c][ih][iw] in xp
PS_HD inline int64_t ps_pk_x_index(int n, int ih, int iw, int c, int H,
                                   int Wp, int pw) {
  return (((int64_t)n * H + ih) * Wp + ps_pk_chunk(iw, pw)) * PS_PK_C +
         ps_pk_half(iw, pw) * PS_PK_SLOTS + c;
}
// khwc weight rows: column of tap (ky, kx, c) for a tap-row width kw_ld and
// c_ld channel slots. Plain khwc is (kw, Cg); the packed layout is
// (2 * pk_kw, PS_PK_SLOTS), which makes it the (ky, kx/2, 8-channel) order
// the gather decodes.
PS_HD inline int ps_khwc_col(int ky, int kx, int c, int kw_ld, int c_ld) {
  return (ky * kw_ld + kx) * c_ld + c;
}
inline void ps_khwc_layout(int kw, int Cg, bool packed, int* kw_ld,
                           int* c_ld) {
  *kw_ld = packed ? 2 * ((kw + 1) / 2) : kw;
  *c_ld = packed ? PS_PK_SLOTS : Cg;
}

struct ConvPlan {
  ConvGeom g;
  int Co, Cg, Cog;
  int Kg, Kcol;     // per-group and total im2col row length
  int64_t NP;       // im2col rows: N*Ho*Wo
  int vec;          // elements per 16 B
  bool is_1x1;      // 1x1/s1/p0: x rows ARE the col rows (aliased, never padded)
  // Materialized colT column stride. G==1 rows round up to a BK (64)
  // multiple with ZERO columns: the fwd GEMM's K becomes glds-clean (no
  // k-tail; VGG conv1_1 K=27 otherwise takes the guarded staging path for
  // every tile) and the wgrad's N tr16-clean (no edge strips).
  int ld_col;
  int wk_ld;        // khwc weight row width: ld_col / G
  bool kpad;        // ld_col != Kcol: colT / wk pad columns must be zero
  // forward gathers im2col rows inside the GEMM staging (no column matrix;
  // the wgrad GEMM gathers too) -- needs 16 B runs contiguous per group
  bool implicit;
  int Kgw_implicit; // implicit wgrad N: Kg rounded up to 64 via kg_max
  // stride-1 dgrad as a FORWARD conv of dy with rotated weights
  // (dx = conv(dy, rot180 W, pad = k-1-p)) through the gather GEMM
  bool dgrad_as_fwd;
  // packed first layer (see PS_PK_SLOTS): forward and wgrad gather from xp.
  // wk_ld then is the packed row width, pk_Kg rounded up to 64
  bool packed;
  int pk_W;         // Wp: 16 B chunks per xp row
  int pk_kw;        // kw': taps per row in chunks, ceil(kw / 2)
  int pk_Kg;        // kh * pk_kw * 8
  int kw_ld, c_ld;  // khwc tap-row width and channel slots (ps_khwc_col)
  // row-fused first layer: forward and wgrad build their operands from
  // staged input rows (conv_rowfused.hip); no column matrix. The layouts
  // (ld_col, wk_ld, khwc order) are the materialized path's.
  bool rowfused;
};

inline ConvPlan ps_conv_plan(int N, int C, int H, int W, int Co, int kh,
                             int kw, int sh, int sw, int ph, int pw, int G,
                             int elem_bytes, const ConvPolicy& policy) {
  ConvPlan p;
  p.g = {N, C, H, W, (H + 2 * ph - kh) / sh + 1, (W + 2 * pw - kw) / sw + 1,
         kh, kw, sh, sw, ph, pw, G};
  p.Co = Co;
  p.Cg = C / G;
  p.Cog = Co / G;
  p.Kg = kh * kw * p.Cg;
  p.Kcol = G * p.Kg;
  p.NP = (int64_t)N * p.g.Ho * p.g.Wo;
  p.vec = 16 / elem_bytes;
  p.is_1x1 = kh == 1 && kw == 1 && sh == 1 && sw == 1 && ph == 0 && pw == 0;
  p.ld_col = (p.is_1x1 || G != 1) ? p.Kcol : (p.Kcol + 63) & ~63;
  p.wk_ld = p.ld_col / G;
  p.kpad = p.ld_col != p.Kcol;
  const int64_t colT_bytes = p.NP * p.Kcol * elem_bytes;
  p.implicit = (policy.force_implicit || colT_bytes > policy.implicit_bytes) &&
               !p.is_1x1 && p.Cg % p.vec == 0;
  p.Kgw_implicit = (p.Kg + 63) & ~63;
  // packing needs whole pixel pairs per stride step (even sw). The dgrad
  // of such a conv, if anyone asks for it, takes the unpacked path.
  p.packed = policy.packed && G == 1 &&
             C <= PS_PK_SLOTS && elem_bytes == 2 && sw % 2 == 0 && !p.is_1x1 &&
             p.g.Ho > 0 && p.g.Wo > 0;
  p.pk_kw = (kw + 1) / 2;
  p.pk_W = (p.g.Wo - 1) * (sw / 2) + p.pk_kw;
  p.pk_Kg = kh * p.pk_kw * PS_PK_C;
  ps_khwc_layout(kw, p.Cg, p.packed, &p.kw_ld, &p.c_ld);
  if (p.packed) {
    p.implicit = false;
    p.wk_ld = (p.pk_Kg + 63) & ~63;
    p.kpad = true;  // unused slots / phantom taps / pad columns stay zero
  }
  // the shapes im2col_rowstage_k takes, once the colT they would write is
  // big enough to matter and both kernels' LDS images fit
  p.rowfused = policy.rowfused && !policy.deterministic && elem_bytes == 2 &&
               G == 1 && C % p.vec != 0 && !p.is_1x1 && !p.packed &&
               !p.implicit && p.g.Ho > 0 && p.g.Wo > 0 &&
               p.NP * p.ld_col * elem_bytes >= policy.rowfused_bytes &&
               ps_rowfused_tiling(N, C, H, W, Co, kh, kw, sh, sw, ph, pw,
                                  p.wk_ld).ok;
  // worth it only when the dcolT it eliminates is substantial (small
  // inception dgrads measured faster on the materialized NT + col2im)
  p.dgrad_as_fwd = sh == 1 && sw == 1 && !p.is_1x1 && p.Cog % p.vec == 0 &&
                   ph <= kh - 1 && pw <= kw - 1 &&
                   colT_bytes > policy.dgrad_fwd_bytes;
  return p;
}

enum ConvGatherRole {
  PS_GATHER_FWD,           // A rows gathered from x (xp for a packed plan)
  PS_GATHER_WGRAD,         // K-major B gathered from x (same window as fwd)
  PS_GATHER_DGRAD_AS_FWD,  // A rows gathered from dy, roles of x/y swapped
};

// `x` is the gathered tensor: x for fwd/wgrad, dy for dgrad-as-forward.
inline GatherDesc ps_gather_desc(const ConvPlan& p, ConvGatherRole role,
                                 const void* x, const void* zero, int grp) {
  const ConvGeom& g = p.g;
  GatherDesc d;
  d.x = x;
  d.zero = zero;
  d.kh = g.kh; d.kw = g.kw;
  if (role == PS_GATHER_DGRAD_AS_FWD) {
    d.C = p.Co; d.H = g.Ho; d.W = g.Wo; d.Ho = g.H; d.Wo = g.W;
    d.sh = 1; d.sw = 1; d.ph = g.kh - 1 - g.ph; d.pw = g.kw - 1 - g.pw;
    d.Cg = p.Cog; d.c0 = grp * p.Cog;
    d.kg_max = g.kh * g.kw * p.Cog;
  } else if (p.packed) {
    // x is xp: the equivalent 8-channel conv over chunk columns
    d.kw = p.pk_kw;
    d.C = PS_PK_C; d.H = g.H; d.W = p.pk_W; d.Ho = g.Ho; d.Wo = g.Wo;
    d.sh = g.sh; d.sw = g.sw / 2; d.ph = g.ph; d.pw = 0;
    d.Cg = PS_PK_C; d.c0 = 0;
    d.kg_max = p.pk_Kg;
  } else {
    d.C = g.C; d.H = g.H; d.W = g.W; d.Ho = g.Ho; d.Wo = g.Wo;
    d.sh = g.sh; d.sw = g.sw; d.ph = g.ph; d.pw = g.pw;
    d.Cg = p.Cg; d.c0 = grp * p.Cg;
    d.kg_max = p.Kg;
  }
  ps_fill_gather_inv(&d);
  return d;
}
