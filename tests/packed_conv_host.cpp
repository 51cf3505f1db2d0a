// Host check of the packed first-layer conv layout (ps_conv_plan.h): packs
// x and W with the header's mapping functions, evaluates the conv over the
// packed tensors exactly as the gather GEMMs decode it (ps_gather_desc +
// the zero-page rules of gemm.hip's gather_addr), and compares forward y
// and dW with a direct 7-loop convolution. Integer-valued inputs make float
// arithmetic exact, so the comparison is ==. Also checks which shapes the
// plan sends down the packed path. Driven by tests/test_packed_conv_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ps_conv_plan.h"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);    \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      ++g_fail;                                           \
    }                                                     \
  } while (0)

unsigned g_seed = 12345u;
float rnd_int() {  // small integers: every product and sum stays exact
  g_seed = g_seed * 1664525u + 1013904223u;
  return (float)((int)((g_seed >> 16) % 7) - 3);
}

// the bindings' thresholds, with the packed switch on
const ConvPolicy kOn = {false, 192LL << 20, 128LL << 20, true};

// The gathered operand element (row, k) as gemm.hip reads it. check_kg_max
// = false is the tr16 wgrad staging, which has no k >= kg_max test: its pad
// columns may read real memory (the result is never unpacked) but must stay
// inside the tensor. Returns 0 for the zero page.
float gathered(const GatherDesc& d, const std::vector<float>& xp, int64_t row,
               int k, bool check_kg_max, bool* in_bounds) {
  *in_bounds = true;
  if (check_kg_max && k >= d.kg_max) return 0.0f;
  const int cg = k % d.Cg, khw = k / d.Cg;
  const int kkw = khw % d.kw, kkh = khw / d.kw;
  const int ow = (int)(row % d.Wo);
  const int64_t t = row / d.Wo;
  const int oh = (int)(t % d.Ho);
  const int64_t n = t / d.Ho;
  const int ih = oh * d.sh - d.ph + kkh, iw = ow * d.sw - d.pw + kkw;
  if (ih < 0 || ih >= d.H || iw < 0 || iw >= d.W) return 0.0f;
  const int64_t idx = ((n * d.H + ih) * d.W + iw) * d.C + d.c0 + cg;
  // element cg of a 16 B load: the whole aligned chunk must be inside xp
  const int64_t chunk = idx - cg;
  if (chunk < 0 || chunk % 8 != 0 || chunk + 8 > (int64_t)xp.size()) {
    *in_bounds = false;
    return 0.0f;
  }
  return xp[idx];
}

struct Geo {
  const char* name;
  int N, C, H, W, Co, kh, kw, sh, sw, ph, pw;
};

void run_geometry(const Geo& q) {
  const ConvPlan p = ps_conv_plan(q.N, q.C, q.H, q.W, q.Co, q.kh, q.kw, q.sh,
                                  q.sw, q.ph, q.pw, 1, 2, kOn);
  CHECK(p.packed, "%s: plan is not packed", q.name);
  if (!p.packed) return;
  const ConvGeom& g = p.g;
  CHECK(p.wk_ld % 64 == 0 && p.wk_ld >= p.pk_Kg, "%s: wk_ld", q.name);
  CHECK(p.pk_Kg == q.kh * p.pk_kw * PS_PK_C, "%s: pk_Kg", q.name);

  std::vector<float> x((size_t)q.N * q.C * q.H * q.W);
  std::vector<float> w((size_t)q.Co * q.C * q.kh * q.kw);
  std::vector<float> dy((size_t)p.NP * q.Co);
  for (float& v : x) v = rnd_int();
  for (float& v : w) v = rnd_int();
  for (float& v : dy) v = rnd_int();
  auto X = [&](int n, int c, int ih, int iw) -> float {
    if (ih < 0 || ih >= q.H || iw < 0 || iw >= q.W) return 0.0f;
    return x[(((size_t)n * q.C + c) * q.H + ih) * q.W + iw];
  };
  auto Wt = [&](int co, int c, int ky, int kx) -> float& {
    return w[(((size_t)co * q.C + c) * q.kh + ky) * q.kw + kx];
  };

  // pack with the header's mapping
  std::vector<float> xp((size_t)q.N * q.H * p.pk_W * PS_PK_C, 0.0f);
  for (int n = 0; n < q.N; ++n)
    for (int c = 0; c < q.C; ++c)
      for (int ih = 0; ih < q.H; ++ih)
        for (int iw = 0; iw < q.W; ++iw) {
          if (ps_pk_chunk(iw, q.pw) >= p.pk_W) continue;  // never read
          const int64_t i = ps_pk_x_index(n, ih, iw, c, q.H, p.pk_W, q.pw);
          CHECK(i >= 0 && i < (int64_t)xp.size(), "%s: xp index", q.name);
          xp[i] = X(n, c, ih, iw);
        }
  std::vector<float> wk((size_t)q.Co * p.wk_ld, 0.0f);
  for (int co = 0; co < q.Co; ++co)
    for (int c = 0; c < q.C; ++c)
      for (int ky = 0; ky < q.kh; ++ky)
        for (int kx = 0; kx < q.kw; ++kx) {
          const int col = ps_khwc_col(ky, kx, c, p.kw_ld, p.c_ld);
          CHECK(col >= 0 && col < p.pk_Kg, "%s: wk column", q.name);
          wk[(size_t)co * p.wk_ld + col] = Wt(co, c, ky, kx);
        }

  const GatherDesc df = ps_gather_desc(p, PS_GATHER_FWD, nullptr, nullptr, 0);
  const GatherDesc dw = ps_gather_desc(p, PS_GATHER_WGRAD, nullptr, nullptr, 0);
  CHECK(df.Cg % 8 == 0 && df.C % 8 == 0 && df.c0 % 8 == 0,
        "%s: gather not 16 B aligned", q.name);

  // forward over the padded K, as conv2d_forward_ex runs it
  int bad_y = 0, oob = 0;
  for (int64_t np = 0; np < p.NP; ++np) {
    const int ow = (int)(np % g.Wo), oh = (int)((np / g.Wo) % g.Ho);
    const int n = (int)(np / ((int64_t)g.Wo * g.Ho));
    for (int co = 0; co < q.Co; ++co) {
      float acc = 0.0f;
      for (int k = 0; k < p.wk_ld; ++k) {
        bool in;
        acc += gathered(df, xp, np, k, true, &in) * wk[(size_t)co * p.wk_ld + k];
        oob += !in;
      }
      float ref = 0.0f;
      for (int c = 0; c < q.C; ++c)
        for (int ky = 0; ky < q.kh; ++ky)
          for (int kx = 0; kx < q.kw; ++kx)
            ref += X(n, c, oh * q.sh - q.ph + ky, ow * q.sw - q.pw + kx) *
                   Wt(co, c, ky, kx);
      bad_y += acc != ref;
    }
  }
  CHECK(bad_y == 0, "%s: %d forward outputs differ", q.name, bad_y);

  // wgrad: dwk[co][k] over k < wk_ld (= Kgw), then the unpack's read
  std::vector<float> dwk((size_t)q.Co * p.wk_ld, 0.0f);
  for (int co = 0; co < q.Co; ++co)
    for (int k = 0; k < p.wk_ld; ++k) {
      float acc = 0.0f;
      for (int64_t np = 0; np < p.NP; ++np) {
        bool in;
        acc += dy[(size_t)np * q.Co + co] *
               gathered(dw, xp, np, k, false, &in);
        oob += !in;
      }
      dwk[(size_t)co * p.wk_ld + k] = acc;
    }
  CHECK(oob == 0, "%s: %d gathered chunks leave xp", q.name, oob);
  int bad_dw = 0;
  for (int co = 0; co < q.Co; ++co)
    for (int c = 0; c < q.C; ++c)
      for (int ky = 0; ky < q.kh; ++ky)
        for (int kx = 0; kx < q.kw; ++kx) {
          float ref = 0.0f;
          for (int64_t np = 0; np < p.NP; ++np) {
            const int ow = (int)(np % g.Wo), oh = (int)((np / g.Wo) % g.Ho);
            const int n = (int)(np / ((int64_t)g.Wo * g.Ho));
            ref += dy[(size_t)np * q.Co + co] *
                   X(n, c, oh * q.sh - q.ph + ky, ow * q.sw - q.pw + kx);
          }
          const float got = dwk[(size_t)co * p.wk_ld +
                                ps_khwc_col(ky, kx, c, p.kw_ld, p.c_ld)];
          bad_dw += got != ref;
        }
  CHECK(bad_dw == 0, "%s: %d weight gradients differ", q.name, bad_dw);
  std::printf("ok %-28s Wp=%d kw'=%d Kg'=%d wk_ld=%d NP=%lld\n", q.name,
              p.pk_W, p.pk_kw, p.pk_Kg, p.wk_ld, (long long)p.NP);
}

bool packed_for(int N, int C, int HW, int Co, int k, int s, int pad, int G,
                int elem_bytes, const ConvPolicy& pol) {
  return ps_conv_plan(N, C, HW, HW, Co, k, k, s, s, pad, pad, G, elem_bytes,
                      pol).packed;
}

void check_selection() {
  // real shapes
  CHECK(packed_for(256, 3, 227, 96, 11, 4, 0, 1, 2, kOn),
        "AlexNet conv1 bf16 must be packed");
  const ConvPlan a = ps_conv_plan(256, 3, 227, 227, 96, 11, 11, 4, 4, 0, 0, 1,
                                  2, kOn);
  CHECK(a.pk_Kg == 528 && a.wk_ld == 576 && a.pk_kw == 6 && a.pk_W == 114 &&
        a.kw_ld == 12 && a.c_ld == 4 && !a.implicit && a.NP == 774400,
        "AlexNet conv1 packed plan values");
  CHECK(!packed_for(256, 3, 227, 96, 11, 4, 0, 1, 4, kOn),
        "fp32 stays unpacked");
  CHECK(!packed_for(32, 3, 224, 64, 3, 1, 1, 1, 2, kOn),
        "VGG conv1_1 (stride 1) stays unpacked");
  CHECK(packed_for(32, 3, 224, 64, 7, 2, 3, 1, 2, kOn),
        "GoogLeNet conv1 qualifies with the switch on");
  ConvPolicy off = kOn;
  off.packed = false;
  CHECK(!packed_for(256, 3, 227, 96, 11, 4, 0, 1, 2, off), "switch off");
  CHECK(!packed_for(2, 3, 16, 8, 3, 1, 1, 1, 2, kOn), "stride 1");
  CHECK(!packed_for(2, 3, 16, 8, 3, 3, 1, 1, 2, kOn), "odd stride");
  CHECK(!packed_for(2, 4, 16, 8, 3, 2, 1, 2, 2, kOn), "G == 2");
  CHECK(!packed_for(2, 8, 16, 8, 3, 2, 1, 1, 2, kOn), "C == 8");
  CHECK(!packed_for(2, 3, 16, 8, 1, 1, 0, 1, 2, kOn), "1x1");
  CHECK(packed_for(2, 3, 16, 8, 1, 2, 0, 1, 2, kOn), "1x1 stride 2");
  // an unpacked plan keeps the plain khwc layout
  const ConvPlan v = ps_conv_plan(32, 3, 224, 224, 64, 3, 3, 1, 1, 1, 1, 1, 2,
                                  kOn);
  CHECK(v.kw_ld == 3 && v.c_ld == 3 && v.wk_ld == 64, "VGG conv1_1 layout");
}

}  // namespace

int main() {
  const Geo geos[] = {
      // odd width + odd kw: phantom tap; window reaches the last pixel
      {"alexnet-conv1 W=19 H=15", 2, 3, 15, 19, 5, 11, 11, 4, 4, 0, 0},
      {"7x7 s2 p3 W=14 (odd pw)", 2, 3, 9, 14, 4, 7, 7, 2, 2, 3, 3},
      {"4x4 s2 p1 (even kw)", 2, 3, 10, 10, 3, 4, 4, 2, 2, 1, 1},
      {"C=1 5x5 s2 p2", 3, 1, 11, 11, 4, 5, 5, 2, 2, 2, 2},
      {"C=4 3x3 s2 exact reach W=9", 2, 4, 9, 9, 6, 3, 3, 2, 2, 0, 0},
      {"C=2 3x5 sh1 sw2 ph1 pw2", 2, 2, 7, 12, 3, 3, 5, 1, 2, 1, 2},
      {"W not reached: 3x3 s4 W=12", 1, 3, 8, 12, 2, 3, 3, 4, 4, 0, 0},
      {"1x1 s2", 2, 3, 6, 7, 4, 1, 1, 2, 2, 0, 0},
      {"one output column", 1, 3, 5, 5, 2, 5, 5, 2, 2, 0, 0},
  };
  for (const Geo& q : geos) run_geometry(q);
  check_selection();
  if (g_fail) {
    std::printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("all packed-conv host checks passed\n");
  return 0;
}
