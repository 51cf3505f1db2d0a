// Halo-tile direct convolution for gfx950: stride-1 bf16 convs with few
// output channels (Co <= 64, Ci % 32 == 0, kernels up to 5 x 5), where the
// gather GEMM is left with a 32 x 32 wave tile, stages every input element
// once per tap and re-stages the filter bank for every tile.
//
//   out[n][oh][ow][co] = act(bias[co] + sum_{ky,kx,c}
//       in[n][oh + ky - ph][ow + kx - pw][c] * w[co][(ky*kw + kx)*Ci + c])
//
// in / out are NHWC bf16, w is K-last khwc rows with a row stride: the
// forward's wk [Co][wk_ld] or the dgrad-as-forward's wr [Cg][kh*kw*Cog] (in
// = dy, pad = k - 1 - p, no bias, no ReLU). Accumulation is f32, one bf16
// rounding at the end. No atomics: the result is a function of the shape.
//
// Tile walk, patch addressing and LDS layout: ps_halo.h (checked on the host
// by tests/halo_plan_host.cpp).
//
// Weights stationary. The grid is persistent, one 256-thread block per CU
//   (capped by the tile count), each block walking tpb consecutive tiles. It
//   stages the whole filter bank into LDS once, rows padded by 8 elements
//   ((K + 8) * 2 B is an odd number of 16 B units, so the 16 rows of a B
//   fragment start in 16 different 16 B columns), and keeps it.
// Input staged once. A tile is 256 output pixels of one image (8 x 32 or
//   16 x 16). Its haloed patch PH x PW x Ci goes global -> registers -> LDS
//   once; all kh * kw taps read it at shifted addresses. The k-loop has one
//   trip per 32-deep k-step, (ky, kx, channel group) advancing as three
//   wave-uniform counters; Ci % 32 == 0, so a step never straddles a tap.
// Fragments. v_mfma_f32_16x16x32_bf16 with the WEIGHTS as the A operand and
//   16 horizontally consecutive pixels as the B operand: D[co][pixel]. A
//   lane then holds 4 consecutive channels of ONE pixel per accumulator, and
//   with the channel order of ps_halo_co two accumulators make one 16 B
//   store. Each lane reads one 16 B run of 8 channels (ds_read_b128) per
//   fragment and k-step.
// Wave tile. A wave owns 64 pixels (4 pixel fragments) x all Co (FN = Co / 16
//   weight fragments): 4 * FN accumulators, 16 for Co = 64. Per k-step it
//   reads 4 + FN fragments of 1 KiB for 4 * FN MFMAs: 8 KiB per 16 MFMAs at
//   Co = 64. Four waves read 32 KiB per step; 16 MFMAs of 16 cycles are 256
//   cycles per SIMD, in which the LDS delivers 32 KiB at 128 B / clk: the LDS
//   reads and the MFMAs of a step take the same time, so half the MFMA peak
//   is the ceiling if the two do not overlap at all. The 32 x 32 wave tile of
//   the gather GEMM reads 4 KiB per 4 MFMAs, twice as much per MFMA.
// Bank conflicts, on paper (64 banks of 4 B; a ds_read_b128 is served 16
//   lanes at a time). A Ci = 64 pixel is 128 B: unswizzled, the 16 lanes of a
//   pixel fragment -- 16 consecutive pixels, same chunk -- would sit on 2 x 4
//   banks, 8 lanes on each. The patch is therefore stored unpadded with
//   chunk c of patch column pc at chunk slot c ^ ((pc >> 1) & 7): pixel
//   parity picks the bank half, pc >> 1 takes 8 consecutive values over the
//   16 lanes, so the slots differ and the 16 lanes cover 64 banks once: no
//   conflict. Ci = 32 (64 B pixels): key (pc >> 2) & 3, pc & 3 picks the
//   bank quarter, 4 slots: 64 banks once. Ci = 128: key pc & 15. Other Ci:
//   key (pc >> 2) & 3, correct but not counted. Padding the pixel to 144 B
//   is conflict-free too but costs 12.5 % of the patch, and then two 8 x 32
//   patches no longer fit beside VGG conv1_2's weights (below). The weight
//   fragments (16 rows, (K + 8) * 2 B apart): row r starts at 16 B column
//   r * (4m + 1) mod 16, all different: no conflict.
// Overlap. Two patch buffers. The loads of tile i + 1's patch are issued
//   into registers before the k-loop of tile i and written to the other
//   buffer after it; one barrier per tile.
//   Budget for VGG conv1_2 (Ci = Co = 64, 3 x 3, 8 x 32 tile):
//     weights 64 x 584 x 2           =  74,752 B
//     patch   10 x 34 x 128 B        =  43,520 B, two of them 87,040 B
//     total                          = 161,792 B of 163,840
//   (with 144 B pixels two patches are 97,920 B: 172,672 B, over.) A ring of
//   input rows walking down the strip would stage 8 rows instead of 10 per
//   tile, but needs 2 TH + kh - 1 = 19 row slots where 20 already fit, and a
//   second code path where a block starts a new strip. The re-read halo
//   rows were read by the same CU one tile earlier, so they come from L2;
//   the walk order of ps_halo.h is chosen for that.
//   Registers per lane, Co = 64: 64 accumulators, 2 x (4 + 4) fragments of 4
//   for the k-loop's register double buffer, 11 staged vectors of 4 in
//   flight (the array holds PS_HALO_NV), 2 x 11 staging positions, 16 bias
//   values. One wave per SIMD, so up to 512 are there; the compiler's count
//   is in profiles/halo_conv.md.
// Edges. Patch pixels outside the image are staged as zeros; pixels of a
//   ragged tile past Ho / Wo are computed from whatever the patch holds and
//   not stored. The k-loop knows nothing of either.

#include "ps_common.h"
#include "ps_api.h"
#include "ps_halo.h"

#include <atomic>
#include <mutex>

// This file's device code is built without packed f32 arithmetic (the
// epilogue's adds are the only f32 VALU work here): a per-file switch, since
// the extension's sources share one set of compiler flags.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace ps {
namespace {

constexpr int HL_THREADS = PS_HALO_THREADS;
constexpr int HL_NV = PS_HALO_NV;

typedef unsigned hl_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((ext_vector_type(4))) __bf16 hl_bf16x4;

// where staged vector v of this thread comes from and goes to, the same for
// every tile: rel = element offset from the patch's first pixel in the input
// image (may point outside the image; guarded by pr, pc), pos = LDS offset
// / 16 | pr << 16 | pc << 24, negative past the patch
struct HlPos {
  int rel, pos;
};

template <int FN>
__global__ __launch_bounds__(HL_THREADS)
void conv_halo_k(HaloTiling t, const __bf16* __restrict__ in,
                 const __bf16* __restrict__ w, int64_t w_ldg,
                 const float* __restrict__ bias, __bf16* __restrict__ out,
                 int relu) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* wl = reinterpret_cast<__bf16*>(smem);
  char* xs0 = smem + t.x_off;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = lane & 15, q = lane >> 4;
  const int64_t t0 = (int64_t)blockIdx.x * t.tpb;
  const int64_t t1 = t0 + t.tpb < t.tiles ? t0 + t.tpb : t.tiles;
  if (t0 >= t1) return;

  // the filter bank, once per block: LDS row fn * 16 + i is channel
  // ps_halo_co(FN, fn, i)
  {
    const int vpr = t.K / 8;
    for (int i = tid; i < FN * 16 * vpr; i += HL_THREADS) {
      const int row = i / vpr;
      const int kv = (i - row * vpr) * 8;
      const int co = ps_halo_co(FN, row >> 4, row & 15);
      *reinterpret_cast<bf16x8*>(&wl[row * t.w_ld + kv]) =
          *reinterpret_cast<const bf16x8*>(&w[(int64_t)co * w_ldg + kv]);
    }
  }

  // staging positions, tile-invariant
  HlPos sp[HL_NV];
#pragma unroll
  for (int v = 0; v < HL_NV; ++v) {
    const int idx = v * HL_THREADS + tid;
    sp[v].rel = 0;
    sp[v].pos = -1;
    if (idx < t.nvec) {
      int pr, pc, c;
      ps_halo_vec(t, idx, &pr, &pc, &c);
      sp[v].rel = (pr * t.W + pc) * t.Ci + c * 8;
      sp[v].pos = ps_halo_lds_off(t, pr, pc, c) >> 4 | pr << 16 | pc << 24;
    }
  }
  hl_u32x4 sv[HL_NV];
  // issue the loads of a tile's patch (zeros where the image ends)
  auto load = [&](int64_t ti) {
    const HaloTile tl = ps_halo_tile(t, ti);
    const int ih0 = tl.oh0 - t.ph, iw0 = tl.ow0 - t.pw;
    // first patch pixel; it may lie before the image, rel brings a guarded
    // vector back inside
    const __bf16* base =
        in + ((int64_t)tl.n * t.H * t.W + (int64_t)ih0 * t.W + iw0) * t.Ci;
#pragma unroll
    for (int v = 0; v < HL_NV; ++v) {
      if (v * HL_THREADS >= t.nvec) break;
      const int ih = ih0 + ((sp[v].pos >> 16) & 0xff);
      const int iw = iw0 + ((sp[v].pos >> 24) & 0x7f);
      sv[v] = hl_u32x4{0u, 0u, 0u, 0u};
      if (sp[v].pos >= 0 && ih >= 0 && ih < t.H && iw >= 0 && iw < t.W)
        sv[v] = *reinterpret_cast<const hl_u32x4*>(base + sp[v].rel);
    }
  };
  auto store = [&](char* xs) {
#pragma unroll
    for (int v = 0; v < HL_NV; ++v) {
      if (v * HL_THREADS >= t.nvec) break;
      if (sp[v].pos >= 0)
        *reinterpret_cast<hl_u32x4*>(xs + (sp[v].pos & 0xffff) * 16) = sv[v];
    }
  };
  load(t0);
  store(xs0);

  // the lane's fragment bases inside a patch: pixel (row, col0 + l) at tap
  // (0, 0), chunk q, before the swizzle
  int ab[4], prow[4], pcol[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    ps_halo_frag(t, wid, f, &prow[f], &pcol[f]);
    ab[f] = (prow[f] * t.PW + pcol[f] + l) * t.CH * 16;
  }
  // bias of the lane's channels, loaded and waited for once (a load pending
  // at the epilogue would put a vmcnt(0) in front of its stores)
  float bv[FN][4];
#pragma unroll
  for (int fn = 0; fn < FN; ++fn)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bv[fn][r] = bias ? bias[ps_halo_co(FN, fn, q * 4 + r)] : 0.0f;
      asm volatile("" : "+v"(bv[fn][r]));
    }
  const int wrow = (l * t.w_ld + q * 8) * 2;  // lane's byte offset in a w frag
  const int wfrag = 16 * t.w_ld * 2;
  const int ccn = t.Ci / 32;
  const int steps = t.kh * t.kw * ccn;
  __syncthreads();

  for (int64_t ti = t0; ti < t1; ++ti) {
    const int cur = (int)(ti - t0) & 1;
    if (ti + 1 < t1) load(ti + 1);
    {
      const char* xs = xs0 + cur * t.patch_bytes;
      const char* wb = smem + wrow;
      f32x4 acc[FN][4] = {};
      // step counters: channel group cc, tap (ky, kx); all wave-uniform
      int cc = 0, kx = 0, ky = 0;
      // fragments of one k-step; the pixel column of lane l at tap kx is
      // col0 + l + kx, and col0 is 0 or 16, which no key sees
      auto frags = [&](int s, bf16x8 (&wf)[FN], bf16x8 (&pf)[4]) {
        const int key = ((l + kx) >> t.ksh) & t.kmask;
        const int off =
            ((ky * t.PW + kx) * t.CH + ((cc * 4 + q) ^ key)) * 16;
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          wf[fn] = *reinterpret_cast<const bf16x8*>(wb + fn * wfrag + s * 64);
#pragma unroll
        for (int f = 0; f < 4; ++f)
          pf[f] = *reinterpret_cast<const bf16x8*>(xs + ab[f] + off);
        if (++cc == ccn) {
          cc = 0;
          if (++kx == t.kw) { kx = 0; ++ky; }
        }
      };
      auto mma = [&](const bf16x8 (&wf)[FN], const bf16x8 (&pf)[4]) {
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
#pragma unroll
          for (int f = 0; f < 4; ++f)
            acc[fn][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wf[fn], pf[f], acc[fn][f], 0, 0, 0);
      };
      // register double buffer: the reads of step s + 1 are issued ahead of
      // the MFMAs of step s
      bf16x8 wf0[FN], pf0[4], wf1[FN], pf1[4];
      frags(0, wf0, pf0);
      for (int s = 0; s < steps; s += 2) {
        if (s + 1 < steps) frags(s + 1, wf1, pf1);
        mma(wf0, pf0);
        if (s + 2 < steps) frags(s + 2, wf0, pf0);
        if (s + 1 < steps) mma(wf1, pf1);
      }

      // D map: column (lane & 15) is the pixel, row (lane >> 4) * 4 + r the
      // weight row. + bias, ReLU, one rounding, 16 B (8 B) per pixel and pair
      const HaloTile tl = ps_halo_tile(t, ti);
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int oh = tl.oh0 + prow[f], ow = tl.ow0 + pcol[f] + l;
        if (oh >= t.Ho || ow >= t.Wo) continue;
        __bf16* o = out + (((int64_t)tl.n * t.Ho + oh) * t.Wo + ow) * t.Co;
#pragma unroll
        for (int fn = 0; fn < FN; fn += 2) {
          const int fp = fn + 1 < FN ? fn + 1 : fn;  // the pair's second
          bf16x8 h;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = acc[fn][f][r] + bv[fn][r];
            float u = acc[fp][f][r] + bv[fp][r];
            if (relu && v < 0.0f) v = 0.0f;
            if (relu && u < 0.0f) u = 0.0f;
            h[r] = (__bf16)v;
            h[4 + r] = (__bf16)u;
          }
          __bf16* oc = o + ps_halo_co(FN, fn, q * 4);
          if (fn + 1 < FN)
            *reinterpret_cast<bf16x8*>(oc) = h;
          else
            *reinterpret_cast<hl_bf16x4*>(oc) = hl_bf16x4{h[0], h[1], h[2], h[3]};
        }
      }
    }
    if (ti + 1 < t1) store(xs0 + (cur ^ 1) * t.patch_bytes);
    __syncthreads();
  }
}

// tests / tuning: cap on the persistent grid (0 = one block per CU)
std::atomic<int> g_hl_blocks{0};
// CU count, set once by ps_halo_prepare together with the LDS attribute
std::atomic<int> g_hl_cus{0};
std::once_flag g_hl_once;
std::atomic<int64_t> g_hl_launches{0};

template <typename K>
bool hl_allow_lds(K kernel) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             PS_HALO_LDS_MAX) == hipSuccess;
}

template <int FN>
void hl_launch(const HaloTiling& t, const void* in, const void* w,
               int64_t w_ld, const float* bias, void* out, int relu,
               hipStream_t s) {
  conv_halo_k<FN><<<dim3((unsigned)t.blocks), HL_THREADS, t.lds, s>>>(
      t, (const __bf16*)in, (const __bf16*)w, w_ld, bias, (__bf16*)out, relu);
}

}  // namespace
}  // namespace ps

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

extern "C" {

void ps_halo_set_blocks(int n) { ps::g_hl_blocks.store(n < 0 ? 0 : n); }

int ps_halo_max_blocks() {
  const int cap = ps::g_hl_blocks.load();
  const int cus = ps::g_hl_cus.load();
  return cap > 0 ? cap : cus > 0 ? cus : 256;
}

int64_t ps_halo_launches(int reset) {
  return reset ? ps::g_hl_launches.exchange(0) : ps::g_hl_launches.load();
}

// Once per process, at plan time: the device's CU count and the LDS
// attribute of every instantiation. Returns 0 without a usable device; the
// launcher must not be called then.
int ps_halo_prepare() {
  using namespace ps;
  std::call_once(g_hl_once, [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess || n <= 0)
      return;
    const bool ok =
        hl_allow_lds(conv_halo_k<1>) && hl_allow_lds(conv_halo_k<2>) &&
        hl_allow_lds(conv_halo_k<3>) && hl_allow_lds(conv_halo_k<4>);
    if (ok) g_hl_cus.store(n);
  });
  return g_hl_cus.load() > 0 ? 1 : 0;
}

// out = act(conv(in, w) + bias), t from ps_halo_tiling with t->ok. in / out
// NHWC bf16, 16 B aligned; w bf16 rows of t->K elements, w_ld apart (a
// multiple of 8), 16 B aligned; bias f32 [Co] or null.
void ps_conv_halo(const HaloTiling* t, const void* in, const void* w,
                  int64_t w_ld, const float* bias, void* out, int relu,
                  hipStream_t s) {
  using namespace ps;
  g_hl_launches.fetch_add(1);
  switch (t->Co / 16) {
    case 1: hl_launch<1>(*t, in, w, w_ld, bias, out, relu, s); break;
    case 2: hl_launch<2>(*t, in, w, w_ld, bias, out, relu, s); break;
    case 3: hl_launch<3>(*t, in, w, w_ld, bias, out, relu, s); break;
    default: hl_launch<4>(*t, in, w, w_ld, bias, out, relu, s); break;
  }
}

}  // extern "C"
