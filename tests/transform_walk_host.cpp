// Host check of the data-transform index walk (ps_transform.h): the whole
// transform, run group by group exactly as transform.hip's threads run it
// (8 flat outputs per group, decode once, walk by increment, ragged tail),
// must equal a naive four-loop decode for every shape
// tests/test_gpu_data_transform.py runs on the GPU, in every mean mode. All
// buffers are exact-size heap blocks, so under AddressSanitizer a read past
// the last source row, the last mean row or the last params triple, or a
// write past the output, stops the program. Driven by
// tests/test_transform_walk_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ps_transform.h"

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

struct Shape {
  int N, C, H, W, crop;
};

// exact-size heap block (no vector capacity slack)
template <typename T>
struct Heap {
  T* p;
  size_t n;
  explicit Heap(size_t n_) : p((T*)std::malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) {}
  ~Heap() { std::free(p); }
  Heap(const Heap&) = delete;
  Heap& operator=(const Heap&) = delete;
};

uint32_t g_lcg = 12345u;
uint32_t lcg() { return g_lcg = g_lcg * 1664525u + 1013904223u; }

void run_shape(const Shape& s, int mean_mode, float scale, int param_kind) {
  TransformGeom g;
  g.N = s.N; g.C = s.C; g.H = s.H; g.W = s.W;
  g.Ho = s.crop ? s.crop : s.H;
  g.Wo = s.crop ? s.crop : s.W;
  g.mean_mode = mean_mode;
  g.scale = scale;
  const int64_t nraw = (int64_t)s.N * s.C * s.H * s.W;
  const int64_t total = (int64_t)s.N * s.C * g.Ho * g.Wo;
  Heap<uint8_t> raw(nraw);
  for (int64_t i = 0; i < nraw; ++i) raw.p[i] = (uint8_t)(i * 7 + (i >> 8));
  const size_t nmean = mean_mode == PS_MEAN_SCALAR    ? 1
                       : mean_mode == PS_MEAN_CHANNEL ? (size_t)s.C
                       : mean_mode == PS_MEAN_IMAGE
                           ? (size_t)s.C * s.H * s.W : 0;
  Heap<float> mean(nmean);
  for (size_t i = 0; i < nmean; ++i)
    mean.p[i] = 100.f + (float)(lcg() % 4000) * 0.01f;
  Heap<int> params(3 * (size_t)s.N);
  const int hmax = s.H - g.Ho, wmax = s.W - g.Wo;
  for (int n = 0; n < s.N; ++n) {
    int ho, wo;
    switch ((n + param_kind) % 3) {
      case 0: ho = 0; wo = 0; break;                // top-left corner
      case 1: ho = hmax; wo = wmax; break;          // bottom-right corner
      default: ho = hmax / 2; wo = wmax / 3; break; // interior
    }
    params.p[3 * n] = ho;
    params.p[3 * n + 1] = wo;
    params.p[3 * n + 2] = (n + param_kind) & 1;
  }
  Heap<float> out(total);
  std::memset(out.p, 0xff, total * sizeof(float));

  // every group of 8 a kernel thread would take, tail group included
  const int64_t ngroups = (total + PS_TRANSFORM_VEC - 1) / PS_TRANSFORM_VEC;
  for (int64_t grp = 0; grp < ngroups; ++grp) {
    const int64_t flat0 = grp * PS_TRANSFORM_VEC;
    const int count = total - flat0 >= PS_TRANSFORM_VEC
                          ? PS_TRANSFORM_VEC : (int)(total - flat0);
    Heap<float> v(count);  // exact size: the group writes count values
    ps_transform_group(g, raw.p, params.p, nmean ? mean.p : nullptr, flat0,
                       count, v.p);
    for (int j = 0; j < count; ++j) out.p[flat0 + j] = v.p[j];
  }

  // naive decode
  int64_t flat = 0;
  for (int n = 0; n < s.N; ++n) {
    const int ho = params.p[3 * n], wo = params.p[3 * n + 1];
    const int flip = params.p[3 * n + 2];
    for (int c = 0; c < s.C; ++c)
      for (int h = 0; h < g.Ho; ++h)
        for (int w = 0; w < g.Wo; ++w, ++flat) {
          const int hs = h + ho, ws = wo + (flip ? g.Wo - 1 - w : w);
          const int64_t src = (((int64_t)n * s.C + c) * s.H + hs) * s.W + ws;
          float m = 0.f;
          if (mean_mode == PS_MEAN_SCALAR) m = mean.p[0];
          if (mean_mode == PS_MEAN_CHANNEL) m = mean.p[c];
          if (mean_mode == PS_MEAN_IMAGE) m = mean.p[(c * s.H + hs) * s.W + ws];
          volatile float d = (float)raw.p[src] - m;
          const float want = d * scale;
          CHECK(std::memcmp(&want, &out.p[flat], sizeof(float)) == 0,
                "N%d C%d H%d W%d crop %d mode %d: (%d,%d,%d,%d) got %g want %g",
                s.N, s.C, s.H, s.W, s.crop, mean_mode, n, c, h, w,
                (double)out.p[flat], (double)want);
        }
  }
  CHECK(flat == total, "walked %lld of %lld", (long long)flat, (long long)total);
}

// params outside the source are clamped into it: the run must stay inside
// the exact-size buffers (the sanitizer build checks that) and equal the run
// with the clamped values
void run_clamp() {
  TransformGeom g;
  g.N = 2; g.C = 3; g.H = 9; g.W = 11; g.Ho = 5; g.Wo = 5;
  g.mean_mode = PS_MEAN_NONE; g.scale = 1.f;
  Heap<uint8_t> raw((size_t)g.N * g.C * g.H * g.W);
  for (size_t i = 0; i < raw.n; ++i) raw.p[i] = (uint8_t)i;
  Heap<int> bad(6), good(6);
  const int b[6] = {-3, 1000, 1, 99, -1, 0}, k[6] = {0, 6, 1, 4, 0, 0};
  std::memcpy(bad.p, b, sizeof b);
  std::memcpy(good.p, k, sizeof k);
  const int64_t total = (int64_t)g.N * g.C * g.Ho * g.Wo;
  for (int64_t f0 = 0; f0 < total; f0 += PS_TRANSFORM_VEC) {
    const int count = total - f0 >= 8 ? 8 : (int)(total - f0);
    float x[8], y[8];
    ps_transform_group(g, raw.p, bad.p, nullptr, f0, count, x);
    ps_transform_group(g, raw.p, good.p, nullptr, f0, count, y);
    for (int j = 0; j < count; ++j)
      CHECK(x[j] == y[j], "clamp: flat %lld", (long long)(f0 + j));
  }
}

}  // namespace

int main() {
  // tests/test_gpu_data_transform.py's shapes
  const Shape shapes[] = {{3, 3, 9, 11, 5},
                          {2, 1, 7, 13, 0},
                          {1, 3, 8, 8, 8},
                          {2, 3, 37, 41, 32},
                          {16, 3, 300, 300, 0}};
  const float scales[] = {1.0f, 0.00390625f, 0.017f};
  for (int mode = PS_MEAN_NONE; mode <= PS_MEAN_IMAGE; ++mode)
    for (float sc : scales)
      for (int kind = 0; kind < 3; ++kind)
        run_shape(shapes[0], mode, sc, kind);
  for (size_t i = 1; i < sizeof shapes / sizeof shapes[0]; ++i)
    for (int mode = PS_MEAN_NONE; mode <= PS_MEAN_IMAGE; ++mode)
      run_shape(shapes[i], mode, 0.017f, (int)i);
  run_clamp();
  std::printf("%ld checks, %d failures\n", g_checks, g_fail);
  if (g_fail) return 1;
  std::printf("all transform-walk host checks passed\n");
  return 0;
}
