// Torch bindings for the poseidon_amd CDNA4 kernels. All GPU activations
// are channels-last (NHWC physical); bindings normalize layouts and compose
// the conv pipeline (im2col -> MFMA GEMM -> bias / col2im / weight repack).
//
// Dtypes: activations are fp32 or bf16 (the MFMA fast path); parameter
// master copies are always fp32 -- conv/linear cast weights to bf16 shadows
// per call when the activations are bf16, and weight/bias GRADIENTS are
// produced in fp32 (bf16 GEMM with fp32 accumulate and fp32 output).
//
// These entry points are the ONLY GPU compute path -- ops/functional.py has
// no eager-torch fallback on CUDA tensors, so a passing GPU test means these
// kernels ran.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <utility>

#include "ps_api.h"
#include "ps_mt.h"

namespace {

using at::Tensor;

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

bool is_bf16(const Tensor& t) { return t.scalar_type() == at::kBFloat16; }

// Every dtype-generic kernel has a ps_<op>_f32 (float pointers) and a
// ps_<op>_bf16 (void pointers) entry: P converts a tensor's data pointer to
// whichever the chosen one takes, PS_CALL picks by dtype.
struct P {
  void* p;
  explicit P(const Tensor& t) : p(t.data_ptr()) {}
  operator float*() const { return (float*)p; }
  operator void*() const { return p; }
};
#define PS_CALL(op, bf16, ...) \
  ((bf16) ? ps_##op##_bf16(__VA_ARGS__) : ps_##op##_f32(__VA_ARGS__))
// same for the weight repacks, which read fp32 masters in both flavours
#define PS_CALL_W(op, bf16, ...) \
  ((bf16) ? ps_##op##_f32_bf16(__VA_ARGS__) : ps_##op##_f32(__VA_ARGS__))

void check_float_like(const Tensor& t, const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16,
              name, ": expected float32 or bfloat16");
  TORCH_CHECK(t.is_cuda(), name, ": expected device tensor");
}

Tensor cl4(const Tensor& t) {  // channels-last contiguous view of a 4D tensor
  TORCH_CHECK(t.dim() == 4, "expected 4D tensor");
  return t.contiguous(at::MemoryFormat::ChannelsLast);
}

Tensor empty_cl(at::IntArrayRef shape, const at::TensorOptions& opts) {
  return at::empty(shape, opts.memory_format(at::MemoryFormat::ChannelsLast));
}

// persistent output (layer cache) when its shape and dtype fit, else a fresh
// channels-last tensor: reuse keeps the consumer's dy identity stable across
// iterations so net-level multi-tensor batching can key on it
Tensor reuse_or_empty_cl(const c10::optional<Tensor>& cached,
                         at::IntArrayRef shape, const Tensor& like) {
  if (cached.has_value() && cached->sizes() == shape &&
      cached->scalar_type() == like.scalar_type())
    return *cached;
  return empty_cl(shape, like.options());
}

// 2D [N*H*W, C] view of a channels-last 4D tensor (physical NHWC rows).
Tensor rows2d(const Tensor& t_cl) {
  int64_t NP = t_cl.size(0) * t_cl.size(2) * t_cl.size(3);
  return t_cl.permute({0, 2, 3, 1}).reshape({NP, t_cl.size(1)});
}

// rows x C view of a per-channel operand: channels-last 4D (C = channels)
// or anything else contiguous (C = last dim)
Tensor as_rows(const Tensor& t, int64_t* rows, int* C) {
  Tensor tc = t.dim() == 4 ? cl4(t) : t.contiguous();
  *C = (int)(t.dim() == 4 ? tc.size(1) : tc.size(-1));
  *rows = tc.numel() / *C;
  return tc;
}

// fp32 master weight -> compute-dtype shadow (bf16 cast via our kernel)
Tensor weight_shadow(const Tensor& w_f32, bool bf16) {
  if (!bf16) return w_f32.contiguous();
  auto wc = w_f32.contiguous();
  Tensor out = at::empty(wc.sizes(), wc.options().dtype(at::kBFloat16));
  ps_f32_to_bf16(wc.data_ptr<float>(), out.data_ptr(), wc.numel(), stream());
  return out;
}

// ---------------------------------------------------------------------------
// GEMM plumbing
// ---------------------------------------------------------------------------

// Implicit-GEMM mode: gather im2col inside the GEMM staging instead of
// materializing the column matrix. Correct for every Cg%VEC==0 conv and
// covered by tests in both modes; measured slightly behind the
// materialized+vectorized-im2col pipeline on VGG/GoogLeNet shapes (gather
// address ALU in the staging inner loop), so default off -- toggle with
// set_implicit_gemm for experiments.
std::atomic<bool> g_implicit_gemm{false};
// Per-layer auto-policy: a conv whose materialized colT would exceed this
// goes implicit regardless of the global flag (VGG's 224/112-resolution
// 3x3 convs build 1-2 GB column matrices; gathering from x reads KHW x
// less HBM). Measured: global implicit loses ~4-8% on AlexNet/GoogLeNet
// (gather decode overhead on small colT), wins on the giant-colT layers:
// with the gather-staged tr16 wgrad (gemm.hip stage_kmaj_tr<GATHER>) the
// implicit path beats materialization wherever the column matrix is large.
std::atomic<int64_t> g_implicit_thresh{192LL << 20};
// stride-1 dgrad runs as a forward conv with rotated weights once the
// dcolT it eliminates exceeds this (no dcolT round-trip -- up to 2 GB for
// VGG conv1_2 -- and no col2im)
std::atomic<int64_t> g_dgrad_fwd_thresh{128LL << 20};
// Packed small-channel first layers (ps_conv_plan.h, PS_PK_SLOTS): G==1,
// C<=4, even-sw bf16 convs run forward and wgrad through the gather GEMMs
// from a pair-packed copy of x -- no colT, no im2col. Default OFF: measured
// on AlexNet conv1 (docs/performance.md item 20) the im2col and layout
// copies it removes (0.34 ms) cost less than the gather GEMMs lose to the
// 1.5x longer packed K (wgrad 316 -> 634 us, forward 303 -> 382 us);
// GoogLeNet's 7x7 conv1 gains 1.3% with it on. PS_PACKED_CONV=1 turns it on
// at import.
std::atomic<bool> g_packed_conv{false};
// Row-fused small-channel first layers (ps_rowfused.h, conv_rowfused.hip):
// bf16 G==1 convs with C % 8 != 0 whose column matrix would reach the
// threshold run forward and wgrad from staged input rows -- no colT, no
// im2col. Never in deterministic mode (the wgrad adds floats atomically).
// Default ON with a 256 MiB threshold, i.e. AlexNet / CaffeNet conv1 (595
// MB): five of five same-call pairs win on each, by 0.081 / 0.087 ms a step,
// 5.4x / 3.1x the parent's spread (docs/performance.md item 27). Under the
// threshold (VGG conv1_1 205 MB, GoogLeNet conv1 154 MB) it measured slower.
// PS_ROWFUSED_CONV=0/1 sets the switch at import.
std::atomic<bool> g_rowfused_conv{true};
std::atomic<int64_t> g_rowfused_thresh{256LL << 20};

void set_rowfused_conv(bool on) { g_rowfused_conv.store(on); }
bool rowfused_conv() { return g_rowfused_conv.load(); }
int64_t rowfused_threshold() { return g_rowfused_thresh.load(); }
void set_rowfused_threshold(int64_t bytes) { g_rowfused_thresh.store(bytes); }
void set_implicit_gemm(bool on) { g_implicit_gemm.store(on); }
void set_packed_conv(bool on) { g_packed_conv.store(on); }
void set_implicit_threshold(int64_t bytes) { g_implicit_thresh.store(bytes); }
void set_dgrad_fwd_threshold(int64_t bytes) { g_dgrad_fwd_thresh.store(bytes); }

// Deterministic mode (ps_api.h): bit-reproducible float reductions. The
// launchers choose the ordered kernels by the flag; the bindings allocate the
// scratch those need (torch allocations, so they are graph-capture safe) and
// raise where no ordered form exists.
bool deterministic() { return ps_deterministic() != 0; }
void set_deterministic(bool on) { ps_set_deterministic(on ? 1 : 0); }
int64_t float_atomic_launches(bool reset) {
  return ps_float_atomic_launches(reset ? 1 : 0);
}

// out[c] += column sums of d[R][C] (out: f32 [C] on d's device)
void colsum_into(const Tensor& d, float* out, int64_t R, int C) {
  Tensor scratch;  // deterministic mode: [blocks][C] partials
  const int64_t n = ps_colsum_scratch_elems(R, C, is_bf16(d) ? 1 : 0);
  if (n > 0) scratch = at::empty({n}, d.options().dtype(at::kFloat));
  PS_CALL(colsum, is_bf16(d), P(d), out, R, C,
          n > 0 ? scratch.data_ptr<float>() : nullptr, stream());
}

// 64B zero page for implicit-GEMM padding loads (per device, persistent)
const void* zero_page(const Tensor& like) {
  static Tensor z;
  if (!z.defined())
    z = at::zeros({64}, like.options().dtype(at::kByte));
  return z.data_ptr();
}

// C[M,N] = alpha * op(A) @ op(B) (+ bias, relu) + beta * C at element
// offsets into A/B/C. A/B share a dtype; C is fp32 or matches them.
void run_gemm(const Tensor& A, const Tensor& B, Tensor& C,
              const float* bias, int M, int N, int K,
              int64_t lda, int64_t ldb, int64_t ldc,
              int64_t a_off, int64_t b_off, int64_t c_off,
              bool a_klast, bool b_klast, float alpha, float beta,
              const GatherDesc* gather_a = nullptr,
              const GatherDesc* gather_b = nullptr, bool relu = false,
              bool c_prezeroed = false) {
  GemmArgs g;
  g.in_bf16 = is_bf16(A);
  g.out_f32 = !is_bf16(C);
  TORCH_CHECK(is_bf16(B) == g.in_bf16, "gemm: A/B dtype mismatch");
  TORCH_CHECK(g.in_bf16 || g.out_f32, "f32 gemm must have f32 out");
  g.A = (const char*)A.data_ptr() + a_off * A.element_size();
  g.B = (const char*)B.data_ptr() + b_off * B.element_size();
  g.C = (char*)C.data_ptr() + c_off * C.element_size();
  g.bias = bias;
  g.M = M; g.N = N; g.K = K;
  g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.alpha = alpha; g.beta = beta;
  g.a_klast = a_klast; g.b_klast = b_klast;
  g.gather_a = gather_a;
  g.gather_b = gather_b;
  g.relu = relu;
  g.c_prezeroed = c_prezeroed;
  GemmPlan plan;
  ps_gemm_plan(&g, &plan);
  TORCH_CHECK(!deterministic() || plan.splitk == 1 || plan.ws_elems > 0,
              "gemm: deterministic mode has no ordered form of this split-K "
              "plan (", M, "x", N, "x", K, ")");
  Tensor ws;  // keep alive until launch returns
  if (plan.ws_elems > 0)
    ws = at::empty({plan.ws_elems}, C.options().dtype(at::kFloat));
  ps_gemm_run(&g, &plan, ws.defined() ? ws.data_ptr<float>() : nullptr,
              stream());
}

// Generic exposed GEMM (tests): C[M,N] = op(A)@op(B); op via *_klast flags.
Tensor gemm(const Tensor& A, const Tensor& B, int M, int N, int K,
            bool a_klast, bool b_klast) {
  check_float_like(A, "A");
  auto Ac = A.contiguous();
  auto Bc = B.contiguous();
  Tensor C = at::empty({M, N}, A.options().dtype(at::kFloat));
  int64_t lda = a_klast ? K : M;
  int64_t ldb = b_klast ? K : N;
  run_gemm(Ac, Bc, C, nullptr, M, N, K, lda, ldb, N, 0, 0, 0,
           a_klast, b_klast, 1.0f, 0.0f);
  return C;
}

// The plan gemm() above would run for this shape right now (tests, tuning):
// path, tile, split-K depth, K slice and workspace size.
py::dict gemm_plan(int M, int N, int K, bool a_klast, bool b_klast,
                   bool bf16) {
  GemmArgs g{};
  // planning reads the operands' alignment only; gemm() passes fresh
  // allocations, which are 256 B aligned
  g.A = g.B = reinterpret_cast<const void*>(uintptr_t{256});
  g.C = reinterpret_cast<void*>(uintptr_t{256});
  g.M = M; g.N = N; g.K = K;
  g.lda = a_klast ? K : M;
  g.ldb = b_klast ? K : N;
  g.ldc = N;
  g.alpha = 1.0f;
  g.a_klast = a_klast; g.b_klast = b_klast;
  g.in_bf16 = bf16;
  g.out_f32 = true;
  GemmPlan p;
  ps_gemm_plan(&g, &p);
  py::dict d;
  d["tr16"] = p.tr16;
  d["splitk"] = p.splitk;
  d["ws_elems"] = p.ws_elems;
  d["bm"] = p.bm;
  d["bn"] = p.bn;
  d["kchunk"] = p.kchunk;
  d["grid_z"] = p.tr16 ? ps_tr_grid_z(p) : p.splitk;
  return d;
}

// ---------------------------------------------------------------------------
// InnerProduct
// ---------------------------------------------------------------------------

// per-step bf16 shadow from the net-level repack table when it fits (skips
// the per-call f32->bf16 cast of the fc masters: VGG casts 138M params
// twice per step otherwise)
Tensor linear_weight(const Tensor& w, const c10::optional<Tensor>& w_shadow,
                     bool bf16) {
  if (w_shadow.has_value() && bf16 && w_shadow->numel() == w.numel())
    return w_shadow->view(w.sizes());
  return weight_shadow(w, bf16);
}

Tensor linear_forward(const Tensor& x, const Tensor& w,
                      const c10::optional<Tensor>& bias, bool fuse_relu,
                      const c10::optional<Tensor>& w_shadow) {
  check_float_like(x, "x");
  auto xc = x.contiguous();
  auto wc = linear_weight(w, w_shadow, is_bf16(x));
  int M = xc.size(0), K = xc.size(1), N = wc.size(0);
  TORCH_CHECK(wc.size(1) == K, "linear: K mismatch");
  Tensor y = at::empty({M, N}, x.options());
  const float* bp = nullptr;
  Tensor bc;
  if (bias.has_value()) {
    bc = bias->contiguous();
    bp = bc.data_ptr<float>();
  }
  run_gemm(xc, wc, y, bp, M, N, K, K, K, N, 0, 0, 0, true, true, 1.0f, 0.0f,
           nullptr, nullptr, fuse_relu);
  return y;
}

std::vector<c10::optional<Tensor>> linear_backward(
    const Tensor& x, const Tensor& w, const Tensor& dy,
    bool need_dx, bool need_dw, bool has_bias,
    const c10::optional<Tensor>& w_shadow,
    const c10::optional<Tensor>& dw_acc,
    const c10::optional<Tensor>& dw_out) {
  check_float_like(dy, "dy");
  TORCH_CHECK(!(dw_acc.has_value() && dw_out.has_value()),
              "linear_backward: dw_acc and dw_out exclude each other");
  auto xc = x.contiguous();
  auto wc = linear_weight(w, w_shadow, is_bf16(dy));
  auto dyc = dy.contiguous();
  int M = xc.size(0), K = xc.size(1), N = wc.size(0);
  c10::optional<Tensor> dx, dw, db;
  if (need_dx) {
    Tensor t = at::empty({M, K}, x.options());
    // dx[M,K] = dy[M,N] @ W[N,K]: contraction N; A=dy K-last, B=W K-major
    run_gemm(dyc, wc, t, nullptr, M, K, N, N, K, K, 0, 0, 0, true, false,
             1.0f, 0.0f);
    dx = t;
  }
  if (need_dw) {
    // dW[N,K] = dy^T[N,M] @ x[M,K]: contraction M; both K-major; fp32 out.
    // With dw_acc, accumulate straight into the param diff (beta=1): saves
    // the separate diff.add_(dw) pass over the fc weights (VGG: a 138M
    // element read-modify-write per step). With dw_out, WRITE the param
    // diff (beta=0): for a weight with one writer per backward that is the
    // same bits as adding into a zeroed diff, without the zero pass, the
    // temporary and the add. The target's old contents are never read: a
    // split-K plan clears or workspaces its own target.
    const bool own = !dw_acc.has_value() && !dw_out.has_value();
    Tensor t = dw_acc.has_value() ? *dw_acc
               : dw_out.has_value()
                   ? *dw_out
                   : at::empty({N, K}, x.options().dtype(at::kFloat));
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                t.is_contiguous() && t.dim() == 2 && t.size(0) == N &&
                t.size(1) == K,
                "linear_backward: dW target must be contiguous f32 [N,K]");
    run_gemm(dyc, xc, t, nullptr, N, K, M, N, K, K, 0, 0, 0, false, false,
             1.0f, dw_acc.has_value() ? 1.0f : 0.0f);
    if (own) dw = t;
  }
  if (has_bias) {
    Tensor t = at::zeros({N}, x.options().dtype(at::kFloat));
    colsum_into(dyc, t.data_ptr<float>(), M, N);
    db = t;
  }
  return {dx, dw, db};
}

// SFB reconstruction: dW[N,K] = a[M,N]^T @ b[M,K] -> fp32
Tensor gemm_at_b(const Tensor& a, const Tensor& b) {
  check_float_like(a, "a");
  auto ac = a.contiguous();
  auto bc = b.contiguous();
  int M = ac.size(0), N = ac.size(1), K = bc.size(1);
  Tensor t = at::empty({N, K}, a.options().dtype(at::kFloat));
  run_gemm(ac, bc, t, nullptr, N, K, M, N, K, K, 0, 0, 0, false, false,
           1.0f, 0.0f);
  return t;
}

// ---------------------------------------------------------------------------
// Convolution (im2col + grouped MFMA GEMM, NHWC). Every layout decision
// comes from the ConvPlan (ps_conv_plan.h).
// ---------------------------------------------------------------------------

// packed: PS_PACKED_AUTO asks the global policy; the wgrad passes what its
// forward actually did (read off the cache slot) instead
enum { PS_PACKED_OFF = 0, PS_PACKED_ON = 1, PS_PACKED_AUTO = -1 };
// rowfused likewise: AUTO asks the switch, the threshold and the mode; ON
// (the forward left the row-fused sentinel) asks only whether the shape can
// run it; OFF keeps the plan off the path
enum { PS_ROWFUSED_OFF = 0, PS_ROWFUSED_ON = 1, PS_ROWFUSED_AUTO = -1 };

// elements from x's first to its last, inclusive: what the row-fused staging
// may read (ps_rowfused.h, RowFusedX::span)
int64_t rowfused_span(const Tensor& x) {
  int64_t span = 1;
  for (int64_t d = 0; d < x.dim(); ++d) {
    TORCH_CHECK(x.size(d) > 0 && x.stride(d) >= 0,
                "row-fused conv: empty or negatively strided x");
    span += (x.size(d) - 1) * x.stride(d);
  }
  return span;
}

ConvPlan conv_plan_for(at::IntArrayRef x_shape, int Co, int kh, int kw,
                       int sh, int sw, int ph, int pw, int G, bool bf16,
                       int packed = PS_PACKED_AUTO,
                       int rowfused = PS_ROWFUSED_AUTO) {
  TORCH_CHECK(x_shape.size() == 4 && G > 0 && x_shape[1] % G == 0 &&
              Co % G == 0, "conv channel/group mismatch");
  const bool rf_auto = rowfused == PS_ROWFUSED_AUTO;
  const ConvPolicy policy = {
      g_implicit_gemm.load(), g_implicit_thresh.load(),
      g_dgrad_fwd_thresh.load(),
      packed == PS_PACKED_AUTO ? g_packed_conv.load() : packed == PS_PACKED_ON,
      rf_auto ? g_rowfused_conv.load() : rowfused == PS_ROWFUSED_ON,
      rf_auto ? g_rowfused_thresh.load() : 0,
      rf_auto && ps_deterministic() != 0};
  ConvPlan p = ps_conv_plan((int)x_shape[0], (int)x_shape[1], (int)x_shape[2],
                            (int)x_shape[3], Co, kh, kw, sh, sw, ph, pw, G,
                            bf16 ? 2 : 4, policy);
  // plan time is where the row-fused kernels read the CU count and get their
  // LDS attribute (once per process), never a launch or a captured region;
  // without a usable device the plan keeps the column matrix
  if (p.rowfused && !ps_rowfused_prepare()) p.rowfused = false;
  return p;
}

// the plan as Python sees it (Net sizes its persistent wk buffers from it)
py::dict conv_plan(std::vector<int64_t> x_shape, std::vector<int64_t> w_shape,
                   std::vector<int64_t> stride, std::vector<int64_t> pad,
                   int G, bool bf16) {
  TORCH_CHECK(w_shape.size() == 4 && stride.size() == 2 && pad.size() == 2);
  TORCH_CHECK(x_shape.size() == 4 && w_shape[1] * G == x_shape[1],
              "conv channel/group mismatch");
  const ConvPlan p = conv_plan_for(x_shape, (int)w_shape[0], (int)w_shape[2],
                                   (int)w_shape[3], (int)stride[0],
                                   (int)stride[1], (int)pad[0], (int)pad[1],
                                   G, bf16);
  py::dict d;
  d["N"] = p.g.N; d["C"] = p.g.C; d["H"] = p.g.H; d["W"] = p.g.W;
  d["Ho"] = p.g.Ho; d["Wo"] = p.g.Wo; d["G"] = p.g.G;
  d["Co"] = p.Co; d["Cg"] = p.Cg; d["Cog"] = p.Cog;
  d["Kg"] = p.Kg; d["Kcol"] = p.Kcol; d["NP"] = p.NP; d["vec"] = p.vec;
  d["is_1x1"] = p.is_1x1; d["ld_col"] = p.ld_col; d["wk_ld"] = p.wk_ld;
  d["kpad"] = p.kpad; d["implicit"] = p.implicit;
  d["Kgw_implicit"] = p.Kgw_implicit; d["dgrad_as_fwd"] = p.dgrad_as_fwd;
  d["packed"] = p.packed; d["pk_W"] = p.pk_W; d["pk_kw"] = p.pk_kw;
  d["pk_Kg"] = p.pk_Kg; d["kw_ld"] = p.kw_ld; d["c_ld"] = p.c_ld;
  d["rowfused"] = p.rowfused;
  // width of the khwc wgrad scratch
  d["Kgw"] = p.implicit ? p.Kgw_implicit : p.wk_ld;
  return d;
}

// (kw_ld, c_ld) of a conv's khwc rows, packed or plain
std::vector<int64_t> khwc_layout(int64_t Cg, int64_t kw, bool packed) {
  int kw_ld, c_ld;
  ps_khwc_layout((int)kw, (int)Cg, packed, &kw_ld, &c_ld);
  return {kw_ld, c_ld};
}

// weights [Co,Cig,kh,kw] fp32 -> khwc [Co, kh*kw*Cig] in compute dtype
Tensor weight_khwc_tr(const Tensor& w, int G, bool bf16) {
  auto wc = w.contiguous();
  int Co = wc.size(0), Cig = wc.size(1), kh = wc.size(2), kw = wc.size(3);
  int Kg = kh * kw * Cig;
  Tensor wkT = at::empty({(int64_t)G * Kg, (int64_t)(Co / G)},
                         w.options().dtype(bf16 ? at::kBFloat16 : at::kFloat));
  PS_CALL_W(weight_to_khwc_tr, bf16, wc.data_ptr<float>(), P(wkT), Co, Cig,
          kh, kw, G, stream());
  return wkT;
}

std::vector<Tensor> conv2d_forward_ex(const Tensor& x, const Tensor& w,
                                      const c10::optional<Tensor>& bias,
                                      int sh, int sw, int ph, int pw, int G,
                                      bool fuse_relu,
                                      const c10::optional<Tensor>& wk_cached,
                                      const c10::optional<Tensor>& wkT_cached) {
  check_float_like(x, "x");
  const bool bf16 = is_bf16(x);
  TORCH_CHECK(x.dim() == 4 && w.size(1) * G == x.size(1),
              "conv channel/group mismatch");
  const ConvPlan p = conv_plan_for(x.sizes(), (int)w.size(0),
                                   (int)w.size(2), (int)w.size(3), sh, sw, ph,
                                   pw, G, bf16);
  const ConvGeom& g = p.g;
  const int Co = p.Co, Cog = p.Cog;
  // only the 1x1 alias and the implicit gather want x channels-last as a
  // whole; the other paths read it through its own strides (below)
  Tensor x_cl = (p.is_1x1 || p.implicit) ? cl4(x) : Tensor();

  // fused repack: one kernel writes both the khwc fwd operand and the
  // per-group transpose the dgrad GEMM wants (cached by the layer). When
  // the layer provides PRE-REPACKED buffers (the net-level multi-tensor
  // repack, repack_mt_run), skip the per-layer kernel entirely. Shadows of
  // another dtype (fp32 compute with bf16 shadows) are not usable; shadows
  // of another WIDTH mean the caller sized them off a different plan.
  const auto cdt = bf16 ? at::kBFloat16 : at::kFloat;
  Tensor wk, wkT;
  if (wk_cached.has_value() && wkT_cached.has_value() &&
      wk_cached->scalar_type() == cdt) {
    TORCH_CHECK(wk_cached->size(1) == p.wk_ld, "conv2d_forward: cached wk is ",
                wk_cached->size(1), " wide, the plan's wk_ld is ", p.wk_ld);
    wk = *wk_cached;
    wkT = *wkT_cached;
  } else {
    auto wc = w.contiguous();
    auto wkopts = w.options().dtype(cdt);
    wk = p.kpad ? at::zeros({Co, (int64_t)p.wk_ld}, wkopts)
                : at::empty({Co, (int64_t)p.wk_ld}, wkopts);
    wkT = at::empty({(int64_t)p.Kcol, (int64_t)Cog}, wkopts);
    PS_CALL_W(weight_to_khwc_both, bf16, wc.data_ptr<float>(), P(wk), P(wkT),
            Co, p.Cg, g.kh, g.kw, G, p.wk_ld, p.kw_ld, p.c_ld, stream());
  }

  // the cache slot: colT, the empty 1-D implicit sentinel, or -- 4-D -- the
  // packed xp, which the wgrad gathers from (it never touches x again)
  Tensor colT;
  if (p.rowfused) {
    // no column matrix at all: the kernel stages x rows through x's own
    // strides and keeps wk in LDS. The cache slot is an empty 2-D sentinel
    // (the implicit one is 1-D, the packed input 4-D).
    TORCH_CHECK(x.numel() / g.N < (1LL << 31) &&
                (g.H - 1) * x.stride(2) + (g.W - 1) * x.stride(3) +
                (g.C - 1) * x.stride(1) < (1LL << 31),
                "row-fused conv: one image must span < 2^31 elements");
    TORCH_CHECK(wk.is_contiguous() && ((uintptr_t)wk.data_ptr() & 15) == 0,
                "row-fused conv: wk must be contiguous and 16 B aligned");
    const RowFusedTiling t = ps_rowfused_tiling(
        g.N, g.C, g.H, g.W, Co, g.kh, g.kw, g.sh, g.sw, g.ph, g.pw, p.wk_ld);
    Tensor y = empty_cl({g.N, Co, g.Ho, g.Wo}, x.options());
    Tensor bc;
    const float* bp = nullptr;
    if (bias.has_value()) {
      bc = bias->contiguous();
      bp = bc.data_ptr<float>();
    }
    ps_conv_rowfused_fwd(&t, x.data_ptr(), x.stride(0), x.stride(1),
                         x.stride(2), x.stride(3), rowfused_span(x),
                         wk.data_ptr(), bp, y.data_ptr(), fuse_relu ? 1 : 0,
                         stream());
    return {y, at::empty({0, (int64_t)p.ld_col}, x.options()), wkT};
  }
  if (p.packed) {
    colT = at::empty({g.N, g.H, (int64_t)p.pk_W, PS_PK_C}, x.options());
    ps_pack_pairs_bf16(x.data_ptr(), colT.data_ptr(), g.N, g.C, g.H, g.W,
                       p.pk_W, g.pw, x.stride(0), x.stride(1), x.stride(2),
                       x.stride(3), stream());
  } else if (p.is_1x1) {
    colT = rows2d(x_cl);  // alias: x rows ARE the col rows
  } else if (!p.implicit) {
    colT = at::empty({p.NP, (int64_t)p.ld_col}, x.options());
    // the rowstage im2col of a small-channel first layer reads the (NCHW)
    // data blob as it is; every other shape wants NHWC, which activations
    // already are
    const bool staged = PS_CALL(im2col_rowstage, bf16, P(x), P(colT), &g,
                                p.ld_col, x.stride(0), x.stride(1),
                                x.stride(2), x.stride(3), stream());
    if (!staged) {
      const Tensor xc = cl4(x);
      PS_CALL(im2col_nhwc, bf16, P(xc), P(colT), &g, p.ld_col, stream());
      // pad columns (ld_col > Kcol) must be zero for the GEMMs; only the
      // rowstage kernel writes them itself
      if (p.kpad)
        PS_CALL(zero_cols, bf16, P(colT), p.NP, p.ld_col, p.Kcol, stream());
    }
  }

  Tensor y = empty_cl({g.N, Co, g.Ho, g.Wo}, x.options());
  const float* bp = nullptr;
  Tensor bc;
  if (bias.has_value()) {
    bc = bias->contiguous();
    bp = bc.data_ptr<float>();
  }
  // per-group K incl. pad: wk rows are PADDED to wk_ld, so the implicit
  // GEMM runs over the padded K too (gather k >= kg_max reads the zero
  // page, wk pad cols are zero)
  const int Kgl = p.wk_ld;
  const bool gather = p.implicit || p.packed;
  const Tensor& xg = p.packed ? colT : x_cl;  // what the gather reads
  for (int grp = 0; grp < G; ++grp) {
    GatherDesc ga{};
    if (gather)
      ga = ps_gather_desc(p, PS_GATHER_FWD, xg.data_ptr(), zero_page(xg), grp);
    run_gemm(gather ? xg : colT, wk, y, bp ? bp + grp * Cog : nullptr,
             (int)p.NP, Cog, Kgl,
             /*lda=*/gather ? Kgl : p.ld_col, /*ldb=*/Kgl, /*ldc=*/Co,
             /*a_off=*/gather ? 0 : (int64_t)grp * Kgl,
             /*b_off=*/(int64_t)grp * Cog * Kgl,
             /*c_off=*/(int64_t)grp * Cog,
             true, true, 1.0f, 0.0f, gather ? &ga : nullptr, nullptr,
             fuse_relu);
  }
  if (!colT.defined())
    colT = at::empty({0}, x.options());  // implicit mode: wgrad gathers too
  return {y, colT, wkT};
}

Tensor conv2d_backward_input(const Tensor& w, const Tensor& dy,
                             std::vector<int64_t> x_shape, int sh, int sw,
                             int ph, int pw, int G,
                             const c10::optional<Tensor>& wkT_cache,
                             const c10::optional<Tensor>& dx_out) {
  check_float_like(dy, "dy");
  const bool bf16 = is_bf16(dy);
  auto dy_cl = cl4(dy);
  const ConvPlan p = conv_plan_for(x_shape, (int)w.size(0), (int)w.size(2),
                                   (int)w.size(3), sh, sw, ph, pw, G, bf16);
  const ConvGeom& g = p.g;
  TORCH_CHECK(dy_cl.size(1) == p.Co && dy_cl.size(2) == g.Ho &&
              dy_cl.size(3) == g.Wo, "conv dgrad: dy does not match x_shape");
  const int Co = p.Co, Cg = p.Cg, Cog = p.Cog, Kg = p.Kg;
  Tensor dx = reuse_or_empty_cl(dx_out, x_shape, dy);

  if (p.dgrad_as_fwd) {
    const int K2 = g.kh * g.kw * Cog;
    auto wc = w.contiguous();
    Tensor wr = at::empty({(int64_t)G * Cg, (int64_t)K2}, dy.options());
    PS_CALL_W(weight_to_dgrad, bf16, wc.data_ptr<float>(), P(wr), Co, Cg,
            g.kh, g.kw, G, stream());
    int64_t NP2 = (int64_t)g.N * g.H * g.W;
    for (int grp = 0; grp < G; ++grp) {
      GatherDesc ga = ps_gather_desc(p, PS_GATHER_DGRAD_AS_FWD,
                                     dy_cl.data_ptr(), zero_page(dy_cl), grp);
      run_gemm(dy_cl, wr, dx, nullptr,
               (int)NP2, Cg, K2,
               /*lda=*/K2, /*ldb=*/K2, /*ldc=*/g.C,
               /*a_off=*/0, /*b_off=*/(int64_t)grp * Cg * K2,
               /*c_off=*/(int64_t)grp * Cg,
               true, true, 1.0f, 0.0f, &ga);
    }
    return dx;
  }

  // transposed khwc repack [G][Kg][Cog]: the dgrad GEMM becomes pure NT
  // (both operands K-last) instead of a K-major-staged NN
  Tensor wkT = wkT_cache.has_value() && wkT_cache->scalar_type() ==
                       (bf16 ? at::kBFloat16 : at::kFloat)
                   ? *wkT_cache
                   : weight_khwc_tr(w, G, bf16);

  Tensor dcolT = p.is_1x1 ? rows2d(dx)
                          : at::empty({p.NP, (int64_t)p.Kcol}, dy.options());
  Tensor dy2 = rows2d(dy_cl);
  for (int grp = 0; grp < G; ++grp) {
    // dcolT_g[NP, Kg] = dy_g[NP, Cog] @ wkT_g[Kg, Cog]^T: NT, contraction Cog
    run_gemm(dy2, wkT, dcolT, nullptr,
             (int)p.NP, Kg, Cog,
             /*lda=*/Co, /*ldb=*/Cog, /*ldc=*/p.Kcol,
             /*a_off=*/(int64_t)grp * Cog, /*b_off=*/(int64_t)grp * Kg * Cog,
             /*c_off=*/(int64_t)grp * Kg,
             true, true, 1.0f, 0.0f);
  }
  if (!p.is_1x1)
    PS_CALL(col2im_nhwc, bf16, P(dcolT), P(dx), &g, stream());
  return dx;
}

// dW accumulated into dw_out (fp32 NCHW [Co,Cg,kh,kw]); db into db_out.
// Returns the khwc scratch dwk it used: callers that keep it alive, hand it
// back as dwk_buf AND guarantee it is zeroed each iteration (net-level
// zero_mt) save both the allocation and the atomic-split-K memset.
Tensor conv2d_backward_weight_acc(const Tensor& x, const Tensor& colT,
                                  const Tensor& dy, Tensor dw_out,
                                  c10::optional<Tensor> db_out,
                                  int sh, int sw, int ph, int pw, int G,
                                  const c10::optional<Tensor>& dwk_buf,
                                  bool skip_unpack, bool skip_db) {
  check_float_like(dy, "dy");
  auto dy_cl = cl4(dy);
  // "forward was implicit" / "forward was packed" come from the cache slot
  // (empty 1-D sentinel / 4-D xp), not from the global switches: toggling
  // one between forward and backward must stay harmless
  const bool implicit = colT.numel() == 0 && colT.dim() == 1;
  const bool packed = colT.dim() == 4;
  // the row-fused forward leaves an empty 2-D slot (a colT has NP rows)
  const bool rowfused = colT.dim() == 2 && colT.size(0) == 0;
  const ConvPlan p = conv_plan_for(x.sizes(), (int)dw_out.size(0),
                                   (int)dw_out.size(2), (int)dw_out.size(3),
                                   sh, sw, ph, pw, G, is_bf16(dy),
                                   packed ? PS_PACKED_ON : PS_PACKED_OFF,
                                   rowfused ? PS_ROWFUSED_ON : PS_ROWFUSED_OFF);
  TORCH_CHECK(dw_out.size(1) == p.Cg && dy_cl.size(2) == p.g.Ho &&
              dy_cl.size(3) == p.g.Wo, "conv wgrad: shape mismatch");
  const int Co = p.Co, Cog = p.Cog;
  if (rowfused) {
    // dwk[Co][wk_ld] += dy^T @ col from x through its strides: no colT, no
    // layout copy of x. The kernel adds atomically, which deterministic mode
    // does not allow -- and there the forward never leaves this sentinel.
    TORCH_CHECK(p.rowfused && is_bf16(x) && is_bf16(dy),
                "conv wgrad: row-fused cache slot does not match the plan");
    TORCH_CHECK(!ps_deterministic(),
                "conv wgrad: the row-fused wgrad has no deterministic form");
    const ConvGeom& g = p.g;
    TORCH_CHECK(x.numel() / g.N < (1LL << 31) &&
                (g.H - 1) * x.stride(2) + (g.W - 1) * x.stride(3) +
                (g.C - 1) * x.stride(1) < (1LL << 31),
                "row-fused conv: one image must span < 2^31 elements");
    const int Kgw = p.wk_ld;
    const bool prez =
        dwk_buf.has_value() && dwk_buf->numel() == (int64_t)Co * Kgw;
    Tensor dwk = prez ? *dwk_buf
               : at::empty({Co, (int64_t)Kgw}, dy.options().dtype(at::kFloat));
    const RowFusedTiling t = ps_rowfused_tiling(
        g.N, g.C, g.H, g.W, Co, g.kh, g.kw, g.sh, g.sw, g.ph, g.pw, p.wk_ld);
    ps_conv_rowfused_wgrad(&t, x.data_ptr(), x.stride(0), x.stride(1),
                           x.stride(2), x.stride(3), rowfused_span(x),
                           dy_cl.data_ptr(), dwk.data_ptr<float>(),
                           prez ? 1 : 0, stream());
    if (!skip_unpack)
      ps_weight_from_khwc_f32(dwk.data_ptr<float>(), dw_out.data_ptr<float>(),
                              Co, p.Cg, g.kh, g.kw, /*ld=*/Kgw,
                              /*beta=*/1.0f, p.kw_ld, p.c_ld, stream());
    if (db_out.has_value() && !skip_db)
      colsum_into(dy_cl, db_out->data_ptr<float>(), p.NP, Co);
    return dwk;
  }
  if (packed) {
    TORCH_CHECK(p.packed && colT.is_contiguous() && is_bf16(colT) &&
                colT.size(0) == p.g.N && colT.size(1) == p.g.H &&
                colT.size(2) == p.pk_W && colT.size(3) == PS_PK_C,
                "conv wgrad: packed input does not match the plan");
  } else {
    TORCH_CHECK(implicit || colT.size(1) == p.ld_col,
                "conv wgrad: colT width does not match the plan");
  }
  // only the implicit gather reads x here: the materialized and the packed
  // wgrad work from the cache slot alone (no layout copy of the data blob)
  const Tensor xg = packed ? colT : implicit ? cl4(x) : Tensor();
  const bool gather = implicit || packed;
  // colT may carry zero pad columns (ld_col): run the GEMM over the padded
  // width too (zero B columns -> zero dwk columns, skipped below).
  // Implicit wgrads pad the same way via the gather's kg_max bound, which
  // makes them tr16-eligible (N % 64 == 0, no edge strips) -- grouped
  // convs included (per-group dwk slices stay contiguous at c_off =
  // grp*Cog*Kgw; AlexNet conv2 Kg=1200 was stuck on the register-staged
  // gather TN path at 403 us/group without this).
  const int Kgw = implicit ? p.Kgw_implicit : p.wk_ld;

  // fp32 gradient accumulation regardless of activation dtype
  const bool prez = dwk_buf.has_value() && dwk_buf->numel() == (int64_t)Co * Kgw;
  Tensor dwk = prez ? *dwk_buf
             : at::empty({Co, (int64_t)Kgw}, dy.options().dtype(at::kFloat));
  Tensor dy2 = rows2d(dy_cl);
  for (int grp = 0; grp < G; ++grp) {
    // dwk_g[Cog, Kg] = dy_g^T[Cog, NP] @ colT_g[NP, Kg]: contraction NP
    GatherDesc gb{};
    if (gather)
      gb = ps_gather_desc(p, PS_GATHER_WGRAD, xg.data_ptr(), zero_page(xg),
                          grp);
    run_gemm(dy2, gather ? xg : colT, dwk, nullptr,
             Cog, Kgw, (int)p.NP,
             /*lda=*/Co, /*ldb=*/gather ? Kgw : p.ld_col, /*ldc=*/Kgw,
             /*a_off=*/(int64_t)grp * Cog,
             /*b_off=*/gather ? 0 : (int64_t)grp * Kgw,
             /*c_off=*/(int64_t)grp * Cog * Kgw,
             false, false, 1.0f, 0.0f, nullptr, gather ? &gb : nullptr,
             false, prez);
  }
  if (!skip_unpack)
    ps_weight_from_khwc_f32(dwk.data_ptr<float>(), dw_out.data_ptr<float>(),
                            Co, p.Cg, p.g.kh, p.g.kw, /*ld=*/Kgw,
                            /*beta=*/1.0f, p.kw_ld, p.c_ld, stream());
  if (db_out.has_value() && !skip_db)
    colsum_into(dy_cl, db_out->data_ptr<float>(), p.NP, Co);
  return dwk;
}

// ---------------------------------------------------------------------------
// NHWC channel concat / slice (CONCAT + SLICE layers, GoogLeNet inception)
// ---------------------------------------------------------------------------

Tensor concat_channels(std::vector<Tensor> inputs) {
  TORCH_CHECK(!inputs.empty());
  auto x0 = cl4(inputs[0]);
  int64_t N = x0.size(0), H = x0.size(2), W = x0.size(3);
  int64_t rows = N * H * W;
  int C_out = 0;
  for (auto& t : inputs) C_out += t.size(1);
  Tensor y = empty_cl({N, (int64_t)C_out, H, W}, x0.options());
  const bool bf16 = is_bf16(x0);
  const int V = bf16 ? 8 : 4;
  bool aligned = true;
  for (auto& t : inputs) aligned = aligned && (t.size(1) % V == 0);
  std::vector<Tensor> cls;
  cls.reserve(inputs.size());
  for (auto& t : inputs) cls.push_back(cl4(t));
  if (aligned) {
    // up to 4 branches per launch (GoogLeNet inception: one launch/join)
    int off = 0;
    for (size_t i0 = 0; i0 < cls.size(); i0 += 4) {
      void* ptrs[4];
      int c_end[4];
      int n = (int)std::min<size_t>(4, cls.size() - i0);
      int c_begin = off;
      for (int j = 0; j < n; ++j) {
        ptrs[j] = cls[i0 + j].data_ptr();
        off += (int)cls[i0 + j].size(1);
        c_end[j] = off;
      }
      PS_CALL(chan_concat4, bf16, P(y), ptrs, c_end, n, c_begin, rows, C_out,
              0, nullptr, stream());
    }
    return y;
  }
  int off = 0;
  for (auto& tc : cls) {
    int Ci = tc.size(1);
    PS_CALL(chan_copy, is_bf16(tc), P(tc), P(y), rows, Ci, C_out, off,
            stream());
    off += Ci;
  }
  return y;
}

// split the wide NHWC tensor into per-range narrow tensors (concat backward
// / slice forward), up to 4 ranges per launch
std::vector<Tensor> split_channels(const Tensor& x,
                                   std::vector<int64_t> sizes,
                                   const c10::optional<std::vector<Tensor>>&
                                       outs_cache,
                                   const c10::optional<std::vector<Tensor>>&
                                       relu_masks) {
  auto xc = cl4(x);
  int64_t N = xc.size(0), H = xc.size(2), W = xc.size(3);
  int64_t rows = N * H * W;
  int C_in = xc.size(1);
  const bool bf16 = is_bf16(xc);
  const int V = bf16 ? 8 : 4;
  std::vector<Tensor> outs;
  outs.reserve(sizes.size());
  const bool reuse = outs_cache.has_value() &&
      outs_cache->size() == sizes.size() &&
      std::all_of(outs_cache->begin(), outs_cache->end(),
                  [&](const Tensor& t) {
                    return t.scalar_type() == x.scalar_type();
                  });
  for (size_t j = 0; j < sizes.size(); ++j)
    outs.push_back(reuse_or_empty_cl(
        reuse ? c10::optional<Tensor>((*outs_cache)[j]) : c10::nullopt,
        {N, sizes[j], H, W}, x));
  bool aligned = true;
  for (int64_t c : sizes) aligned = aligned && (c % V == 0);
  if (aligned) {
    int off = 0;
    for (size_t i0 = 0; i0 < outs.size(); i0 += 4) {
      void* ptrs[4];
      const void* masks[4];
      bool any_mask = false;
      int c_end[4];
      int n = (int)std::min<size_t>(4, outs.size() - i0);
      int c_begin = off;
      for (int j = 0; j < n; ++j) {
        ptrs[j] = outs[i0 + j].data_ptr();
        masks[j] = nullptr;
        if (relu_masks.has_value() && i0 + j < relu_masks->size() &&
            (*relu_masks)[i0 + j].defined()) {
          const Tensor& mk = (*relu_masks)[i0 + j];
          TORCH_CHECK(mk.scalar_type() == x.scalar_type() &&
                      mk.numel() == outs[i0 + j].numel(),
                      "split mask dtype/shape mismatch");
          masks[j] = mk.data_ptr();
          any_mask = true;
        }
        off += (int)sizes[i0 + j];
        c_end[j] = off;
      }
      PS_CALL(chan_concat4, bf16, P(xc), ptrs, c_end, n, c_begin, rows, C_in,
              1, any_mask ? masks : nullptr, stream());
    }
  } else {
    int off = 0;
    for (size_t j = 0; j < outs.size(); ++j) {
      int Ci = (int)sizes[j];
      PS_CALL(chan_slice, bf16, P(xc), P(outs[j]), rows, C_in, Ci, off,
              stream());
      off += Ci;
    }
  }
  return outs;
}

Tensor slice_channels(const Tensor& x, int64_t c_off, int64_t c_len) {
  auto xc = cl4(x);
  int64_t N = xc.size(0), H = xc.size(2), W = xc.size(3);
  int64_t rows = N * H * W;
  Tensor y = empty_cl({N, c_len, H, W}, x.options());
  PS_CALL(chan_slice, is_bf16(xc), P(xc), P(y), rows, (int)xc.size(1),
          (int)c_len, (int)c_off, stream());
  return y;
}

// ---------------------------------------------------------------------------
// Pooling
// ---------------------------------------------------------------------------

int pool_out(int h, int k, int p, int s) {
  int out = (int)std::ceil((double)(h + 2 * p - k) / s) + 1;
  if (p > 0 && (out - 1) * s >= h + p) --out;
  return out;
}

PoolGeom pool_geom(const Tensor& x_cl, int kh, int kw, int sh, int sw,
                   int ph, int pw) {
  PoolGeom g;
  g.N = x_cl.size(0); g.C = x_cl.size(1); g.H = x_cl.size(2); g.W = x_cl.size(3);
  g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw; g.ph = ph; g.pw = pw;
  g.Ho = pool_out(g.H, kh, ph, sh);
  g.Wo = pool_out(g.W, kw, pw, sw);
  return g;
}

// backward: input extent from the recorded x shape, output extent from dy
PoolGeom pool_geom_bwd(const std::vector<int64_t>& x_shape,
                       const Tensor& dy_cl, int kh, int kw, int sh, int sw,
                       int ph, int pw) {
  PoolGeom g;
  g.N = x_shape[0]; g.C = x_shape[1]; g.H = x_shape[2]; g.W = x_shape[3];
  g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw; g.ph = ph; g.pw = pw;
  g.Ho = dy_cl.size(2); g.Wo = dy_cl.size(3);
  return g;
}

std::vector<Tensor> pool_max_forward(const Tensor& x, int kh, int kw, int sh,
                                     int sw, int ph, int pw) {
  check_float_like(x, "x");
  auto x_cl = cl4(x);
  PoolGeom g = pool_geom(x_cl, kh, kw, sh, sw, ph, pw);
  Tensor y = empty_cl({g.N, g.C, g.Ho, g.Wo}, x.options());
  Tensor mask = empty_cl({g.N, g.C, g.Ho, g.Wo}, x.options().dtype(at::kByte));
  PS_CALL(maxpool_fwd, is_bf16(x), P(x_cl), P(y), mask.data_ptr<uint8_t>(), &g,
          stream());
  return {y, mask};
}

Tensor pool_max_backward(const Tensor& dy, const Tensor& mask,
                         std::vector<int64_t> x_shape, int kh, int kw, int sh,
                         int sw, int ph, int pw,
                         const c10::optional<Tensor>& dx_out) {
  auto dy_cl = cl4(dy);
  auto mask_cl = cl4(mask);
  PoolGeom g = pool_geom_bwd(x_shape, dy_cl, kh, kw, sh, sw, ph, pw);
  Tensor dx = reuse_or_empty_cl(dx_out, x_shape, dy);
  PS_CALL(maxpool_bwd, is_bf16(dy), P(dy_cl), mask_cl.data_ptr<uint8_t>(),
          P(dx), &g, stream());
  return dx;
}

Tensor pool_ave_forward(const Tensor& x, int kh, int kw, int sh, int sw,
                        int ph, int pw) {
  check_float_like(x, "x");
  auto x_cl = cl4(x);
  PoolGeom g = pool_geom(x_cl, kh, kw, sh, sw, ph, pw);
  Tensor y = empty_cl({g.N, g.C, g.Ho, g.Wo}, x.options());
  PS_CALL(avepool_fwd, is_bf16(x), P(x_cl), P(y), &g, stream());
  return y;
}

Tensor pool_ave_backward(const Tensor& dy, std::vector<int64_t> x_shape,
                         int kh, int kw, int sh, int sw, int ph, int pw) {
  auto dy_cl = cl4(dy);
  PoolGeom g = pool_geom_bwd(x_shape, dy_cl, kh, kw, sh, sw, ph, pw);
  Tensor dx = empty_cl(x_shape, dy.options());
  PS_CALL(avepool_bwd, is_bf16(dy), P(dy_cl), P(dx), &g, stream());
  return dx;
}

std::vector<Tensor> pool_stoch_forward_train(const Tensor& x, int kh, int kw,
                                             int sh, int sw, int ph, int pw,
                                             int64_t seed) {
  check_float_like(x, "x");
  auto x_cl = cl4(x).to(at::kFloat);  // stochastic pooling runs fp32
  PoolGeom g = pool_geom(x_cl, kh, kw, sh, sw, ph, pw);
  Tensor y = empty_cl({g.N, g.C, g.Ho, g.Wo}, x_cl.options());
  Tensor mask = empty_cl({g.N, g.C, g.Ho, g.Wo},
                         x_cl.options().dtype(at::kByte));
  ps_stochpool_fwd_train_f32(x_cl.data_ptr<float>(), y.data_ptr<float>(),
                             mask.data_ptr<uint8_t>(), &g, (uint64_t)seed,
                             stream());
  return {y.to(x.scalar_type()), mask};
}

Tensor pool_stoch_forward_test(const Tensor& x, int kh, int kw, int sh,
                               int sw, int ph, int pw) {
  check_float_like(x, "x");
  auto x_cl = cl4(x).to(at::kFloat);
  PoolGeom g = pool_geom(x_cl, kh, kw, sh, sw, ph, pw);
  Tensor y = empty_cl({g.N, g.C, g.Ho, g.Wo}, x_cl.options());
  ps_stochpool_fwd_test_f32(x_cl.data_ptr<float>(), y.data_ptr<float>(), &g,
                            stream());
  return y.to(x.scalar_type());
}

// ---------------------------------------------------------------------------
// LRN (scale is fp32 in both paths)
// ---------------------------------------------------------------------------

std::vector<Tensor> lrn_forward(const Tensor& x, int size, double alpha,
                                double beta) {
  check_float_like(x, "x");
  auto x_cl = cl4(x);
  int64_t rows = (int64_t)x_cl.size(0) * x_cl.size(2) * x_cl.size(3);
  int C = x_cl.size(1);
  auto opts_cl = x.options().memory_format(at::MemoryFormat::ChannelsLast);
  Tensor y = at::empty_like(x_cl, opts_cl);
  if (ps_lrn_v8_ok(C, size)) {
    // halo-register path: no scale tensor at all (backward recomputes it)
    PS_CALL(lrn_fwd_v8, is_bf16(x), P(x_cl), P(y), rows, C, size, (float)alpha,
            (float)beta, stream());
    return {y, at::empty({0}, x.options().dtype(at::kFloat))};
  }
  Tensor scale = at::empty_like(x_cl, opts_cl.dtype(at::kFloat));
  PS_CALL(lrn_fwd, is_bf16(x), P(x_cl), P(y), scale.data_ptr<float>(), rows, C,
          size, (float)alpha, (float)beta, stream());
  return {y, scale};
}

Tensor lrn_backward(const Tensor& x, const Tensor& y, const Tensor& scale,
                    const Tensor& dy, int size, double alpha, double beta) {
  auto x_cl = cl4(x);
  auto y_cl = cl4(y);
  auto dy_cl = cl4(dy);
  int64_t rows = (int64_t)x_cl.size(0) * x_cl.size(2) * x_cl.size(3);
  int C = x_cl.size(1);
  Tensor dx = at::empty_like(x_cl, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (scale.numel() == 0) {  // forward used the halo-register path
    TORCH_CHECK(ps_lrn_v8_ok(C, size), "lrn: empty scale but v8 ineligible");
    PS_CALL(lrn_bwd_v8, is_bf16(x), P(x_cl), P(y_cl), P(dy_cl), P(dx), rows, C,
            size, (float)alpha, (float)beta, stream());
    return dx;
  }
  auto sc_cl = cl4(scale);
  // ratio workspace only feeds the C>256 fallback path; the row-block
  // kernels keep the ratio in LDS
  Tensor ratio = at::empty({C > 256 ? rows * C : 0},
                           x.options().dtype(at::kFloat));
  PS_CALL(lrn_bwd, is_bf16(x), P(x_cl), P(y_cl), sc_cl.data_ptr<float>(),
          P(dy_cl), P(dx), ratio.data_ptr<float>(), rows, C, size,
          (float)alpha, (float)beta, stream());
  return dx;
}

// ---------------------------------------------------------------------------
// Fused backward tails of a conv block (conv -> relu -> [lrn] -> [max pool]):
// one pass over the conv output writes dx, already masked by the in-place
// ReLU, and adds its column sum into the conv's fp32 bias gradient.
// ---------------------------------------------------------------------------

// Block caps of the launches that end in a bias flush. Every block issues C
// global atomics when it retires, so past the point where the chip is busy
// more blocks only add atomic traffic: the cap is an atomics budget over C,
// clamped to a per-kernel range (measured sweeps:
// profiles/bwd_tail_fusion.md). The LRN tail is latency-bound and wants
// two rounds of its 4 resident blocks per CU; the flat pool and ReLU tails
// stream and do with 1-2 blocks per CU once C is large.
int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
int lrn_tail_blocks(int C) { return clampi((512 << 10) / C, 1024, 2048); }
int pool_tail_blocks(int C) { return clampi((128 << 10) / C, 256, 2048); }
int relu_tail_blocks(int C) { return clampi((64 << 10) / C, 256, 1024); }
// 0 = the rules above; tests lower it to force grid striding
std::atomic<int> g_tail_blocks{0};
void set_bwd_tail_blocks(int64_t n) { g_tail_blocks = n > 0 ? (int)n : 0; }
int tail_blocks(int dflt) {
  const int n = g_tail_blocks.load();
  return n > 0 ? n : dflt;
}

float* tail_db(const c10::optional<Tensor>& db, int C) {
  if (!db.has_value()) return nullptr;
  TORCH_CHECK(db->is_cuda() && db->scalar_type() == at::kFloat &&
              db->is_contiguous() && db->numel() == C,
              "bias gradient: contiguous f32 device tensor of C elements");
  return db->data_ptr<float>();
}
// Deterministic mode: the tail kernels run WITHOUT their bias flush (LDS and
// global float atomics) -- dx keeps the mask fusion -- and the bias gradient
// is the ordered column sum of the stored dx, which is the very set of
// values the flush would have added.
float* tail_kernel_db(float* db) { return deterministic() ? nullptr : db; }
void tail_db_ordered(const Tensor& dx, float* db, int C) {
  if (db && deterministic()) colsum_into(dx, db, dx.numel() / C, C);
}

// LRN backward on the vec8 path. pool_mask given: dy is the top diff of the
// max pool that consumes this LRN's output (mask and geometry are that
// pool's) and the pool's own backward is skipped. relu: x is a post-ReLU
// conv output, dx is masked by x > 0. db: += column sum of dx.
Tensor lrn_backward_tail(const Tensor& x, const Tensor& y, const Tensor& dy,
                         int size, double alpha, double beta, bool relu,
                         const c10::optional<Tensor>& db,
                         const c10::optional<Tensor>& pool_mask, int kh,
                         int kw, int sh, int sw, int ph, int pw,
                         const c10::optional<Tensor>& dx_out) {
  auto x_cl = cl4(x);
  auto y_cl = cl4(y);
  auto dy_cl = cl4(dy);
  int64_t rows = (int64_t)x_cl.size(0) * x_cl.size(2) * x_cl.size(3);
  int C = x_cl.size(1);
  TORCH_CHECK(ps_lrn_v8_ok(C, size), "lrn tail: needs the vec8 LRN path");
  TORCH_CHECK(y.sizes() == x.sizes() && y.scalar_type() == x.scalar_type() &&
              dy.scalar_type() == x.scalar_type());
  TORCH_CHECK(rows < (int64_t)1 << 31, "lrn tail: rows exceed 32 bits");
  Tensor dx = reuse_or_empty_cl(dx_out, x.sizes(), x);
  PoolGeom g{};
  Tensor mask_cl;
  const uint8_t* mask = nullptr;
  if (pool_mask.has_value()) {
    mask_cl = cl4(*pool_mask);
    TORCH_CHECK(mask_cl.scalar_type() == at::kByte &&
                mask_cl.sizes() == dy.sizes(), "lrn tail: u8 mask like dy");
    g = pool_geom_bwd(x.sizes().vec(), dy_cl, kh, kw, sh, sw, ph, pw);
    TORCH_CHECK(dy_cl.size(0) == g.N && dy_cl.size(1) == g.C &&
                g.Ho == pool_out(g.H, kh, ph, sh) &&
                g.Wo == pool_out(g.W, kw, pw, sw),
                "lrn tail: pool top diff does not match the geometry");
    mask = mask_cl.data_ptr<uint8_t>();
  } else {
    TORCH_CHECK(dy.sizes() == x.sizes());
  }
  float* dbp = tail_db(db, C);
  PS_CALL(lrn_bwd_v8_tail, is_bf16(x), P(x_cl), P(y_cl), P(dy_cl), mask, &g,
          P(dx), tail_kernel_db(dbp), relu ? 1 : 0, rows, C, size,
          (float)alpha, (float)beta, tail_blocks(lrn_tail_blocks(C)),
          stream());
  tail_db_ordered(dx, dbp, C);
  return dx;
}

// max-pool backward whose bottom is a post-ReLU conv output x: dx masked by
// x > 0, db += column sum of dx
Tensor pool_max_backward_tail(const Tensor& dy, const Tensor& mask,
                              const Tensor& x, int kh, int kw, int sh, int sw,
                              int ph, int pw, const c10::optional<Tensor>& db,
                              const c10::optional<Tensor>& dx_out) {
  auto dy_cl = cl4(dy);
  auto mask_cl = cl4(mask);
  auto x_cl = cl4(x);
  PoolGeom g = pool_geom_bwd(x.sizes().vec(), dy_cl, kh, kw, sh, sw, ph, pw);
  TORCH_CHECK(g.C % (is_bf16(dy) ? 8 : 4) == 0,
              "pool tail: channels must fill whole vectors");
  TORCH_CHECK(x.scalar_type() == dy.scalar_type() &&
              mask_cl.scalar_type() == at::kByte &&
              mask_cl.sizes() == dy.sizes() && dy_cl.size(0) == g.N &&
              dy_cl.size(1) == g.C && g.Ho == pool_out(g.H, kh, ph, sh) &&
              g.Wo == pool_out(g.W, kw, pw, sw) && g.C * 4 <= 64 * 1024,
              "pool tail: operands do not match the geometry");
  Tensor dx = reuse_or_empty_cl(dx_out, x.sizes(), dy);
  float* dbp = tail_db(db, g.C);
  PS_CALL(maxpool_bwd_tail, is_bf16(dy), P(dy_cl), mask_cl.data_ptr<uint8_t>(),
          P(x_cl), P(dx), tail_kernel_db(dbp), &g,
          tail_blocks(pool_tail_blocks(g.C)), stream());
  tail_db_ordered(dx, dbp, g.C);
  return dx;
}

// in-place slope-0 ReLU backward of a channels-last 4D (or [rows, C]) dy
// + db += column sum of dx
Tensor relu_backward_bias(const Tensor& x, Tensor dy, Tensor db) {
  int64_t rows;
  int C;
  Tensor xc = as_rows(x, &rows, &C);
  Tensor dyc = as_rows(dy, &rows, &C);
  TORCH_CHECK(dyc.data_ptr() == dy.data_ptr(),
              "relu_backward_bias: dy must be dense in its row layout");
  TORCH_CHECK(x.sizes() == dy.sizes() && x.scalar_type() == dy.scalar_type() &&
              C % (is_bf16(x) ? 8 : 4) == 0 && C * 4 <= 64 * 1024,
              "relu_backward_bias: mismatched operands or unaligned channels");
  float* dbp = tail_db(db, C);
  if (deterministic()) {
    // the plain slope-0 ReLU backward stores the same dx (g * 0 keeps its
    // sign bit there too), then the ordered column sum of it
    PS_CALL(relu_bwd, is_bf16(x), P(xc), P(dyc), P(dyc), rows * C, 0.0f,
            stream());
    tail_db_ordered(dyc, dbp, C);
    return dy;
  }
  PS_CALL(relu_bwd_bias, is_bf16(x), P(xc), P(dyc), P(dyc), dbp, rows, C,
          tail_blocks(relu_tail_blocks(C)), stream());
  return dy;
}

// ---------------------------------------------------------------------------
// Softmax family
// ---------------------------------------------------------------------------

// output shaped and laid out like an as_rows() operand
Tensor empty_like_rows(const Tensor& tc) {
  return at::empty_like(tc, tc.options(),
                        tc.dim() == 4 ? at::MemoryFormat::ChannelsLast
                                      : at::MemoryFormat::Preserve);
}

Tensor softmax_forward(const Tensor& x) {
  check_float_like(x, "x");
  int64_t rows;
  int C;
  Tensor xc = as_rows(x, &rows, &C);
  Tensor y = empty_like_rows(xc);
  PS_CALL(softmax_rows, is_bf16(x), P(xc), P(y), rows, C, stream());
  return y;
}

Tensor softmax_backward(const Tensor& y, const Tensor& dy) {
  int64_t rows;
  int C;
  Tensor yc = as_rows(y, &rows, &C);
  Tensor dyc = as_rows(dy, &rows, &C);
  Tensor dx = empty_like_rows(yc);
  PS_CALL(softmax_bwd_rows, is_bf16(y), P(yc), P(dyc), P(dx), rows, C,
          stream());
  return dx;
}

std::vector<Tensor> softmax_loss_forward(const Tensor& logits,
                                         const Tensor& labels) {
  check_float_like(logits, "logits");
  auto xc = logits.contiguous();
  auto lc = labels.contiguous().to(at::kFloat);
  int64_t rows = xc.size(0);
  int C = xc.size(1);
  Tensor prob = at::empty_like(xc);
  Tensor loss = at::zeros({}, xc.options().dtype(at::kFloat));
  Tensor row_loss;  // deterministic mode: per-row terms, summed in order
  if (deterministic())
    row_loss = at::empty({rows}, loss.options());
  PS_CALL(softmax_loss_fwd, is_bf16(xc), P(xc), lc.data_ptr<float>(), P(prob),
          loss.data_ptr<float>(),
          row_loss.defined() ? row_loss.data_ptr<float>() : nullptr, rows, C,
          stream());
  loss.div_((double)rows);
  return {loss, prob};
}

Tensor softmax_loss_backward(const Tensor& prob, const Tensor& labels,
                             double loss_weight) {
  auto pc = prob.contiguous();
  auto lc = labels.contiguous().to(at::kFloat);
  int64_t rows = pc.size(0);
  int C = pc.size(1);
  Tensor dx = at::empty_like(pc);
  PS_CALL(softmax_loss_bwd, is_bf16(pc), P(pc), lc.data_ptr<float>(), P(dx),
          rows, C, (float)(loss_weight / rows), stream());
  return dx;
}

// ---------------------------------------------------------------------------
// neuron ops
// ---------------------------------------------------------------------------

Tensor any_contig(const Tensor& t) {
  return (t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast))
             ? t : t.contiguous();
}

Tensor relu_forward(const Tensor& x, double slope) {
  check_float_like(x, "x");
  auto xc = any_contig(x);
  Tensor y = at::empty_like(xc);
  PS_CALL(relu_fwd, is_bf16(x), P(xc), P(y), xc.numel(), (float)slope,
          stream());
  return y;
}

Tensor relu_backward(const Tensor& x, const Tensor& dy, double slope,
                     bool in_place) {
  auto xc = any_contig(x);
  auto dyc = xc.dim() == 4 && xc.is_contiguous(at::MemoryFormat::ChannelsLast)
                 ? cl4(dy) : dy.contiguous();
  // in-place (dx == dy): elementwise same-index, safe; keeps the grad
  // buffer identity stable for the net-level colsum batch (a fresh dx
  // every iteration churned every fused-relu conv's dy pointer)
  Tensor dx = (in_place && dyc.is_alias_of(dy) &&
               dyc.data_ptr() == dy.data_ptr())
                  ? dyc : at::empty_like(xc);
  PS_CALL(relu_bwd, is_bf16(x), P(xc), P(dyc), P(dx), xc.numel(), (float)slope,
          stream());
  return dx;
}

#define PS_BIND_UNARY(pyname, op)                                           \
  Tensor pyname(const Tensor& x) {                                          \
    check_float_like(x, #pyname);                                           \
    auto xc = any_contig(x);                                                \
    Tensor y = at::empty_like(xc);                                          \
    PS_CALL(op, is_bf16(x), P(xc), P(y), xc.numel(), stream());             \
    return y;                                                               \
  }

#define PS_BIND_BINARY(pyname, op)                                          \
  Tensor pyname(const Tensor& a, const Tensor& b) {                         \
    auto ac = any_contig(a);                                                \
    auto bc = any_contig(b);                                                \
    Tensor y = at::empty_like(ac);                                          \
    PS_CALL(op, is_bf16(a), P(ac), P(bc), P(y), ac.numel(), stream());      \
    return y;                                                               \
  }

PS_BIND_UNARY(sigmoid_forward, sigmoid_fwd)
PS_BIND_BINARY(sigmoid_backward, sigmoid_bwd)
PS_BIND_UNARY(tanh_forward, tanh_fwd)
PS_BIND_BINARY(tanh_backward, tanh_bwd)
PS_BIND_UNARY(bnll_forward, bnll_fwd)
PS_BIND_BINARY(bnll_backward, bnll_bwd)

std::vector<Tensor> dropout_forward(const Tensor& x, double ratio,
                                    int64_t seed, int64_t offset) {
  check_float_like(x, "x");
  auto xc = any_contig(x);
  Tensor y = at::empty_like(xc);
  Tensor mask = at::empty(xc.sizes(), xc.options().dtype(at::kByte));
  PS_CALL(dropout_fwd, is_bf16(x), P(xc), P(y), mask.data_ptr<uint8_t>(),
          xc.numel(), (float)ratio, (uint64_t)seed, (uint64_t)offset,
          stream());
  return {y, mask};
}

// graph-replayable dropout: philox offset lives in device memory and is
// incremented in-stream, so each replay draws a fresh mask
std::vector<Tensor> dropout_forward_offdev(const Tensor& x, double ratio,
                                           int64_t seed, Tensor offset_dev) {
  check_float_like(x, "x");
  auto xc = any_contig(x);
  Tensor y = at::empty_like(xc);
  Tensor mask = at::empty(xc.sizes(), xc.options().dtype(at::kByte));
  if (is_bf16(x))
    ps_dropout_fwd_bf16_offdev(xc.data_ptr(), y.data_ptr(),
                               mask.data_ptr<uint8_t>(), xc.numel(),
                               (float)ratio, (uint64_t)seed,
                               offset_dev.data_ptr(), stream());
  else
    ps_dropout_fwd_f32_offdev(xc.data_ptr<float>(), y.data_ptr<float>(),
                              mask.data_ptr<uint8_t>(), xc.numel(),
                              (float)ratio, (uint64_t)seed,
                              offset_dev.data_ptr(), stream());
  ps_u64_inc(offset_dev.data_ptr(), stream());
  return {y, mask};
}

Tensor dropout_backward(const Tensor& dy, const Tensor& mask, double ratio) {
  auto dyc = any_contig(dy);
  Tensor dx = at::empty_like(dyc);
  PS_CALL(dropout_bwd, is_bf16(dy), P(dyc), mask.data_ptr<uint8_t>(), P(dx),
          dyc.numel(), (float)ratio, stream());
  return dx;
}

Tensor threshold_forward(const Tensor& x, double thr) {
  auto xc = any_contig(x);
  Tensor y = at::empty_like(xc);
  PS_CALL(threshold_fwd, is_bf16(x), P(xc), P(y), xc.numel(), (float)thr,
          stream());
  return y;
}

// pairwise running max: y/mask updated in place; mask[i] = blob index of
// the current max (start by calling with mask filled 0 and y = blob 0)
void eltwise_max_step(Tensor y, const Tensor& b, Tensor mask, int64_t idx_b) {
  auto bc = any_contig(b);
  PS_CALL(eltwise_max_fwd, is_bf16(y), P(y), P(bc), P(y),
          mask.data_ptr<uint8_t>(), y.numel(), (int)idx_b, stream());
}

Tensor eltwise_max_backward(const Tensor& dy, const Tensor& mask,
                            int64_t idx) {
  auto dyc = any_contig(dy);
  Tensor dx = at::empty_like(dyc);
  PS_CALL(eltwise_max_bwd, is_bf16(dy), P(dyc), mask.data_ptr<uint8_t>(),
          P(dx), dyc.numel(), (int)idx, stream());
  return dx;
}

Tensor contrastive_forward(const Tensor& dist_sq, const Tensor& sim,
                           double margin, bool legacy) {
  auto d = dist_sq.contiguous().to(at::kFloat);
  auto sm = sim.contiguous().to(at::kFloat);
  Tensor loss = at::empty_like(d);
  ps_contrastive_fwd_f32(d.data_ptr<float>(), sm.data_ptr<float>(),
                         loss.data_ptr<float>(), d.numel(), (float)margin,
                         legacy ? 1 : 0, stream());
  return loss;
}

// ---------------------------------------------------------------------------
// optimizer updates (in-place on fp32 master params)
// ---------------------------------------------------------------------------

void sgd_update(Tensor w, const Tensor& g, Tensor h, double lr, double mom,
                double wd) {
  ps_sgd_update(w.data_ptr<float>(), g.data_ptr<float>(), h.data_ptr<float>(),
                w.numel(), (float)lr, (float)mom, (float)wd, stream());
}
// graph-replayable: lr read from lr_dev[0] * lr_mult at kernel time
void sgd_update_lrdev(Tensor w, const Tensor& g, Tensor h, double lr_mult,
                      double mom, double wd, const Tensor& lr_dev) {
  ps_sgd_update_lrdev(w.data_ptr<float>(), g.data_ptr<float>(),
                      h.data_ptr<float>(), w.numel(), (float)lr_mult,
                      (float)mom, (float)wd, lr_dev.data_ptr<float>(),
                      stream());
}
void nesterov_update(Tensor w, const Tensor& g, Tensor h, double lr,
                     double mom, double wd) {
  ps_nesterov_update(w.data_ptr<float>(), g.data_ptr<float>(),
                     h.data_ptr<float>(), w.numel(), (float)lr, (float)mom,
                     (float)wd, stream());
}
void adagrad_update(Tensor w, const Tensor& g, Tensor h, double lr,
                    double delta, double wd) {
  ps_adagrad_update(w.data_ptr<float>(), g.data_ptr<float>(),
                    h.data_ptr<float>(), w.numel(), (float)lr, (float)delta,
                    (float)wd, stream());
}

// ---------------------------------------------------------------------------
// Multi-tensor apply tables (layouts: ps_mt.h). Each *_prepare checks its
// tensors and fills one descriptor per tensor; mt_tables cuts every tensor
// into chunks and uploads both tables -- build once, reuse forever.
// ---------------------------------------------------------------------------

template <typename T>
Tensor vec_to_dev(const std::vector<T>& v, const Tensor& like) {
  Tensor host = at::from_blob(const_cast<T*>(v.data()),
                              {(int64_t)(v.size() * sizeof(T))},
                              at::TensorOptions().dtype(at::kByte));
  return host.to(like.device());
}

// extent(desc) -> {length, chunk step} of that tensor in the units its
// kernel's Chunk.off counts. Returns {desc_dev(u8), chunk_dev(u8), nchunks}.
template <typename Chunk = ps::MTChunk, typename Desc, typename Extent>
std::vector<Tensor> mt_tables(const std::vector<Desc>& descs,
                              const Tensor& like, Extent extent) {
  std::vector<Chunk> chunks;
  for (size_t t = 0; t < descs.size(); ++t) {
    const std::pair<int64_t, int64_t> e = extent(descs[t]);
    for (int64_t off = 0; off < e.first; off += e.second)
      chunks.push_back({(int)t, off});
  }
  return {vec_to_dev(descs, like), vec_to_dev(chunks, like),
          at::scalar_tensor((int64_t)chunks.size())};
}

// the elementwise tables: d.n elements in MT_CHUNK steps
const auto mt_by_elts = [](const auto& d) {
  return std::pair<int64_t, int64_t>(d.n, ps::MT_CHUNK);
};

std::vector<Tensor> sgd_mt_prepare(std::vector<Tensor> ws,
                                   std::vector<Tensor> gs,
                                   std::vector<Tensor> hs,
                                   std::vector<double> lr_mults,
                                   std::vector<double> wds,
                                   std::vector<c10::optional<Tensor>> shadows) {
  const size_t nt = ws.size();
  TORCH_CHECK(gs.size() == nt && hs.size() == nt && lr_mults.size() == nt &&
              wds.size() == nt, "sgd_mt_prepare: length mismatch");
  // bf16 shadows the update keeps current, one entry (or None) per tensor;
  // empty = none
  TORCH_CHECK(shadows.empty() || shadows.size() == nt,
              "sgd_mt_prepare: shadows length mismatch");
  std::vector<ps::MTDesc> descs(nt);
  for (size_t t = 0; t < nt; ++t) {
    TORCH_CHECK(ws[t].is_cuda() && ws[t].is_contiguous() &&
                ws[t].scalar_type() == at::kFloat &&
                gs[t].is_contiguous() && hs[t].is_contiguous(),
                "sgd_mt_prepare: params must be contiguous f32 CUDA");
    int64_t n = ws[t].numel();
    TORCH_CHECK(gs[t].numel() == n && hs[t].numel() == n);
    void* shadow = nullptr;
    if (!shadows.empty() && shadows[t].has_value()) {
      const Tensor& sh = *shadows[t];
      // the vec4 body stores four bf16 at once: 8-byte alignment
      TORCH_CHECK(sh.is_cuda() && sh.is_contiguous() &&
                  sh.scalar_type() == at::kBFloat16 && sh.numel() == n &&
                  (uintptr_t)sh.data_ptr() % 8 == 0,
                  "sgd_mt_prepare: a shadow must be contiguous bf16 CUDA "
                  "with its tensor's element count");
      shadow = sh.data_ptr();
    }
    descs[t] = {ws[t].data_ptr<float>(), gs[t].data_ptr<float>(),
                hs[t].data_ptr<float>(), n, (float)lr_mults[t],
                (float)wds[t], shadow};
  }
  return mt_tables(descs, ws[0], mt_by_elts);
}

void sgd_mt_run(const Tensor& desc_dev, const Tensor& chunk_dev,
                int64_t nchunks, double lr, double mom,
                const c10::optional<Tensor>& lr_dev) {
  ps_sgd_mt(desc_dev.data_ptr(), chunk_dev.data_ptr(), (int)nchunks,
            (float)lr, (float)mom,
            lr_dev.has_value() ? lr_dev->data_ptr<float>() : nullptr,
            stream());
}

std::vector<Tensor> zero_mt_prepare(std::vector<Tensor> ts) {
  std::vector<ps::MTZeroDesc> descs(ts.size());
  for (size_t t = 0; t < ts.size(); ++t) {
    TORCH_CHECK(ts[t].is_cuda() && ts[t].is_contiguous() &&
                ts[t].scalar_type() == at::kFloat,
                "zero_mt_prepare: tensors must be contiguous f32 CUDA");
    descs[t] = {ts[t].data_ptr<float>(), ts[t].numel()};
  }
  return mt_tables(descs, ts[0], mt_by_elts);
}

void zero_mt_run(const Tensor& desc_dev, const Tensor& chunk_dev,
                 int64_t nchunks) {
  ps_zero_mt(desc_dev.data_ptr(), chunk_dev.data_ptr(), (int)nchunks,
             stream());
}

// Blob statistics (stats.hip). The three buffers a caller keeps: stats
// [slots][4] f32 (StatsRec), scratch [slots][STATS_MAX_BLOCKS][4] f32, nblk
// [slots] i32. A tensor is read as its flat storage, which any
// non-overlapping dense layout allows; anything else raises (no copy).
std::vector<int64_t> blob_stats_plan(int64_t count, int64_t itemsize) {
  TORCH_CHECK(count >= 0 && (itemsize == 2 || itemsize == 4),
              "blob_stats_plan: bf16 or fp32 elements");
  const ps::StatsPlan p = ps::stats_plan(count, (int)itemsize);
  return {p.blocks, p.chain};
}
int64_t blob_stats_reduce_depth(int64_t blocks, int64_t itemsize) {
  return ps::stats_reduce_depth((int)blocks, (int)itemsize);
}
int64_t blob_stats_max_blocks() { return ps::STATS_MAX_BLOCKS; }

void check_stats_input(const Tensor& t) {
  check_float_like(t, "blob_stats");
  TORCH_CHECK(t.is_non_overlapping_and_dense(),
              "blob_stats: tensor must be non-overlapping and dense");
  TORCH_CHECK(t.numel() < (int64_t)1 << 32, "blob_stats: tensor too large");
}
void check_stats_buffers(const Tensor& scratch, const Tensor& nblk,
                         int64_t slot_end) {
  TORCH_CHECK(scratch.is_cuda() && scratch.is_contiguous() &&
              scratch.scalar_type() == at::kFloat &&
              nblk.is_cuda() && nblk.is_contiguous() &&
              nblk.scalar_type() == at::kInt,
              "blob_stats: scratch must be f32 and nblk i32, on the device");
  TORCH_CHECK(slot_end <= nblk.numel() &&
              scratch.numel() >= nblk.numel() * ps::STATS_MAX_BLOCKS * 4,
              "blob_stats: slot out of range");
}

void blob_stats(const Tensor& t, Tensor scratch, Tensor nblk, int64_t slot) {
  check_stats_input(t);
  TORCH_CHECK(slot >= 0, "blob_stats: negative slot");
  check_stats_buffers(scratch, nblk, slot + 1);
  ps_blob_stats(t.data_ptr(), t.numel(), is_bf16(t) ? 1 : 0, (int)slot,
                scratch.data_ptr(), nblk.data_ptr<int>(), stream());
}

std::vector<Tensor> blob_stats_mt_prepare(std::vector<Tensor> ts,
                                          std::vector<int64_t> slots) {
  TORCH_CHECK(!ts.empty() && ts.size() == slots.size(),
              "blob_stats_mt_prepare: one slot per tensor");
  std::vector<ps::StatsDesc> descs(ts.size());
  int64_t max_slot = 0;
  for (size_t t = 0; t < ts.size(); ++t) {
    check_stats_input(ts[t]);
    TORCH_CHECK(slots[t] >= 0 && ts[t].numel() > 0,
                "blob_stats_mt_prepare: empty tensor or negative slot");
    const int bf = is_bf16(ts[t]) ? 1 : 0;
    descs[t] = {ts[t].data_ptr(), ts[t].numel(), (int)slots[t],
                ps::stats_plan(ts[t].numel(), bf ? 2 : 4).blocks, bf, 0};
    max_slot = std::max(max_slot, slots[t]);
  }
  auto mt = mt_tables(descs, ts[0], [](const ps::StatsDesc& d) {
    return std::pair<int64_t, int64_t>(d.blocks, 1);
  });
  mt.push_back(at::scalar_tensor(max_slot));
  return mt;
}

void blob_stats_mt_run(const Tensor& desc_dev, const Tensor& chunk_dev,
                       int64_t nchunks, int64_t max_slot, Tensor scratch,
                       Tensor nblk) {
  check_stats_buffers(scratch, nblk, max_slot + 1);
  ps_blob_stats_mt(desc_dev.data_ptr(), chunk_dev.data_ptr(), (int)nchunks,
                   scratch.data_ptr(), nblk.data_ptr<int>(), stream());
}

void blob_stats_finalize(Tensor stats, const Tensor& scratch,
                         const Tensor& nblk, int64_t slot0, int64_t nslots) {
  TORCH_CHECK(slot0 >= 0 && nslots >= 0, "blob_stats_finalize: bad range");
  check_stats_buffers(scratch, nblk, slot0 + nslots);
  TORCH_CHECK(stats.is_cuda() && stats.is_contiguous() &&
              stats.scalar_type() == at::kFloat &&
              stats.numel() >= nblk.numel() * 4,
              "blob_stats_finalize: stats must be f32 [slots][4]");
  ps_blob_stats_finalize(scratch.data_ptr(), nblk.data_ptr<int>(),
                         stats.data_ptr(), (int)slot0, (int)nslots, stream());
}

int64_t blob_stats_launches(bool reset) {
  return ps_blob_stats_launches(reset ? 1 : 0);
}

// one launch sums every deferred conv bias gradient: descs keyed on the
// (now identity-stable) activation-grad buffers. Chunk.off = start row.
std::vector<Tensor> colsum_mt_prepare(std::vector<Tensor> dys,
                                      std::vector<Tensor> dbs) {
  std::vector<ps::ColsumDesc> descs(dys.size());
  int max_c = 0;
  for (size_t t = 0; t < dys.size(); ++t) {
    const Tensor& d = dys[t];
    // NO cl4() here: a layout copy would leave the desc pointing at a
    // temporary. The conv top diffs are channels-last by construction.
    const int vec = 16 / (int)d.element_size();
    TORCH_CHECK(d.is_cuda() && d.dim() == 4 &&
                d.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                d.size(1) % vec == 0 &&
                dbs[t].scalar_type() == at::kFloat,
                "colsum_mt: channels-last CUDA dy with C % 16B required");
    // one kernel instantiation reads every dy of the table
    TORCH_CHECK(d.scalar_type() == dys[0].scalar_type(),
                "colsum_mt: all dys must share one dtype");
    int C = (int)d.size(1);
    int64_t R = d.numel() / C;
    // ~256K elements per block: coarse enough that terminal atomics on
    // the C-wide bias vectors stay rare
    int64_t rows_per = std::max<int64_t>(4, (262144 / C + 3) & ~3LL);
    descs[t] = {d.data_ptr(), dbs[t].data_ptr<float>(), R, rows_per, C};
    max_c = std::max(max_c, C);
  }
  TORCH_CHECK(max_c <= 8192, "colsum_mt: C exceeds the LDS budget");
  auto mt = mt_tables<ps::ColsumChunk>(descs, dys[0], [](const ps::ColsumDesc& d) {
    return std::pair<int64_t, int64_t>(d.R, d.rows_per);
  });
  mt.push_back(at::scalar_tensor((int64_t)max_c));
  // [4] tensors in the table, [5] deterministic mode's [nchunks][max_c]
  // partials: sized here, once, so a captured graph keeps a stable pointer
  // (empty when the table is prepared with the mode off)
  const int64_t nchunks = mt[1].numel() * mt[1].element_size() /
                          (int64_t)sizeof(ps::ColsumChunk);
  mt.push_back(at::scalar_tensor((int64_t)dys.size()));
  mt.push_back(at::empty({deterministic() ? nchunks * max_c : 0},
                         dys[0].options().dtype(at::kFloat)));
  return mt;
}

void colsum_mt_run(const Tensor& desc_dev, const Tensor& chunk_dev,
                   int64_t nchunks, bool bf16, int64_t max_c,
                   int64_t ntensors, const Tensor& scratch) {
  TORCH_CHECK(!deterministic() || scratch.numel() >= nchunks * max_c,
              "colsum_mt: table was prepared with deterministic mode off; "
              "prepare it again");
  ps_colsum_mt(desc_dev.data_ptr(), chunk_dev.data_ptr(), (int)nchunks,
               bf16 ? 1 : 0, (int)max_c, (int)ntensors,
               deterministic() ? scratch.data_ptr<float>() : nullptr,
               stream());
}

// one table for every deferred conv-wgrad unpack (dwk khwc -> dw NCHW,
// accumulate); identities are the persistent dwk buffers + param diffs
std::vector<Tensor> unpack_mt_prepare(std::vector<Tensor> dwks,
                                      std::vector<Tensor> dws,
                                      std::vector<int64_t> Cigs,
                                      std::vector<int64_t> khs,
                                      std::vector<int64_t> kws,
                                      std::vector<int64_t> kw_lds,
                                      std::vector<int64_t> c_lds,
                                      std::vector<bool> overwrites) {
  const size_t nt = dwks.size();
  // khwc_layout() per tensor; empty = every conv plain (kw, Cig)
  TORCH_CHECK((kw_lds.empty() && c_lds.empty()) ||
              (kw_lds.size() == nt && c_lds.size() == nt),
              "unpack_mt_prepare: layout length mismatch");
  // per tensor: write dw instead of adding to it; empty = all accumulate
  TORCH_CHECK(overwrites.empty() || overwrites.size() == nt,
              "unpack_mt_prepare: overwrites length mismatch");
  std::vector<ps::MTUnpackDesc> descs(nt);
  for (size_t t = 0; t < nt; ++t) {
    TORCH_CHECK(dwks[t].is_cuda() && dwks[t].scalar_type() == at::kFloat &&
                dws[t].is_cuda() && dws[t].is_contiguous() &&
                dws[t].scalar_type() == at::kFloat,
                "unpack_mt_prepare: f32 CUDA tensors required");
    int Co = (int)dwks[t].size(0);
    int ldk = (int)dwks[t].size(1);
    int64_t n = dws[t].numel();
    TORCH_CHECK(n == (int64_t)Co * Cigs[t] * khs[t] * kws[t]);
    const int kw_ld = kw_lds.empty() ? (int)kws[t] : (int)kw_lds[t];
    const int c_ld = c_lds.empty() ? (int)Cigs[t] : (int)c_lds[t];
    TORCH_CHECK(kw_ld >= kws[t] && c_ld >= Cigs[t] &&
                (int64_t)khs[t] * kw_ld * c_ld <= ldk,
                "unpack_mt_prepare: khwc layout exceeds the dwk row");
    descs[t] = {dwks[t].data_ptr<float>(), dws[t].data_ptr<float>(), n,
                Co, (int)Cigs[t], (int)khs[t], (int)kws[t], ldk, kw_ld, c_ld,
                !overwrites.empty() && overwrites[t] ? 1 : 0};
  }
  return mt_tables(descs, dwks[0], mt_by_elts);
}

void unpack_mt_run(const Tensor& desc_dev, const Tensor& chunk_dev,
                   int64_t nchunks) {
  ps_unpack_mt(desc_dev.data_ptr(), chunk_dev.data_ptr(), (int)nchunks,
               stream());
}

std::vector<Tensor> repack_mt_prepare(std::vector<Tensor> masters,
                                      std::vector<Tensor> wks,
                                      std::vector<Tensor> wkTs,
                                      std::vector<int64_t> Gs,
                                      std::vector<int64_t> kw_lds,
                                      std::vector<int64_t> c_lds) {
  const size_t nt = masters.size();
  // the plan's (kw_ld, c_ld) per tensor; empty = every shadow plain khwc
  TORCH_CHECK((kw_lds.empty() && c_lds.empty()) ||
              (kw_lds.size() == nt && c_lds.size() == nt),
              "repack_mt_prepare: layout length mismatch");
  std::vector<ps::MTRepackDesc> descs(nt);
  for (size_t t = 0; t < nt; ++t) {
    const Tensor& m = masters[t];
    TORCH_CHECK(m.is_cuda() && m.is_contiguous() &&
                m.scalar_type() == at::kFloat && m.dim() == 4 &&
                wks[t].scalar_type() == at::kBFloat16,
                "repack_mt_prepare: f32 NCHW masters + bf16 outputs");
    const bool has_t = wkTs[t].numel() > 0;
    TORCH_CHECK(!has_t || wkTs[t].scalar_type() == at::kBFloat16);
    const int kw_ld = kw_lds.empty() ? (int)m.size(3) : (int)kw_lds[t];
    const int c_ld = c_lds.empty() ? (int)m.size(1) : (int)c_lds[t];
    TORCH_CHECK(kw_ld >= m.size(3) && c_ld >= m.size(1) &&
                m.size(2) * kw_ld * c_ld <= wks[t].size(1),
                "repack_mt_prepare: khwc layout exceeds the wk row");
    descs[t] = {m.data_ptr<float>(), wks[t].data_ptr(),
                has_t ? wkTs[t].data_ptr() : nullptr,
                m.numel(), (int)m.size(0), (int)m.size(1), (int)m.size(2),
                (int)m.size(3), (int)Gs[t], (int)wks[t].size(1), kw_ld, c_ld};
  }
  return mt_tables(descs, masters[0], mt_by_elts);
}

void repack_mt_run(const Tensor& desc_dev, const Tensor& chunk_dev,
                   int64_t nchunks) {
  ps_repack_mt(desc_dev.data_ptr(), chunk_dev.data_ptr(), (int)nchunks,
               stream());
}

// standalone bias colsum (eager fallback for the net-level batch)
void colsum_acc(const Tensor& dy, Tensor db) {
  int64_t R;
  int C;
  Tensor d = as_rows(dy, &R, &C);
  colsum_into(d, db.data_ptr<float>(), R, C);
}

// ---------------------------------------------------------------------------
// data-layer transform: raw uint8 records -> the layer's NCHW top, in place
// ---------------------------------------------------------------------------

void data_transform(const Tensor& raw, const Tensor& params,
                    const c10::optional<Tensor>& mean, int64_t mean_mode,
                    double scale, Tensor out) {
  TORCH_CHECK(raw.is_cuda() && params.is_cuda() && out.is_cuda(),
              "data_transform: expected device tensors");
  TORCH_CHECK(raw.scalar_type() == at::kByte && raw.dim() == 4 &&
                  raw.is_contiguous(),
              "data_transform: raw must be contiguous uint8 [N,C,H,W]");
  const int64_t N = raw.size(0), C = raw.size(1), H = raw.size(2),
                W = raw.size(3);
  TORCH_CHECK(params.scalar_type() == at::kInt && params.is_contiguous() &&
                  params.dim() == 2 && params.size(0) == N &&
                  params.size(1) == 3,
              "data_transform: params must be contiguous int32 [N,3]");
  check_float_like(out, "data_transform out");
  TORCH_CHECK(out.dim() == 4 && out.is_contiguous() && out.size(0) == N &&
                  out.size(1) == C && out.size(2) >= 1 && out.size(2) <= H &&
                  out.size(3) >= 1 && out.size(3) <= W,
              "data_transform: out must be contiguous [N,C,Ho,Wo] with "
              "Ho <= H, Wo <= W");
  TORCH_CHECK(C * H * W < (int64_t(1) << 31) && N < (int64_t(1) << 29),
              "data_transform: record too large");
  TORCH_CHECK((uintptr_t)out.data_ptr() %
                      (PS_TRANSFORM_VEC * out.element_size()) == 0,
              "data_transform: out must be aligned to 8 elements");
  int64_t want = 0;
  switch (mean_mode) {
    case PS_MEAN_NONE: break;
    case PS_MEAN_SCALAR: want = 1; break;
    case PS_MEAN_CHANNEL: want = C; break;
    case PS_MEAN_IMAGE: want = C * H * W; break;
    default: TORCH_CHECK(false, "data_transform: bad mean_mode ", mean_mode);
  }
  const float* mp = nullptr;
  if (want) {
    TORCH_CHECK(mean.has_value() && mean->is_cuda() &&
                    mean->scalar_type() == at::kFloat &&
                    mean->is_contiguous() && mean->numel() == want,
                "data_transform: mean must be contiguous fp32 with ", want,
                " elements");
    mp = mean->data_ptr<float>();
  }
  TransformGeom g;
  g.N = (int)N; g.C = (int)C; g.H = (int)H; g.W = (int)W;
  g.Ho = (int)out.size(2); g.Wo = (int)out.size(3);
  g.mean_mode = (int)mean_mode;
  g.scale = (float)scale;
  PS_CALL(data_transform, is_bf16(out), raw.data_ptr<uint8_t>(),
          params.data_ptr<int>(), mp, P(out), &g, stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("data_transform", &data_transform);
  m.def("gemm", &gemm);
  m.def("gemm_plan", &gemm_plan);
  m.def("linear_forward", &linear_forward);
  m.def("linear_backward", &linear_backward);
  m.def("gemm_at_b", &gemm_at_b);
  m.def("conv_plan", &conv_plan);
  m.def("conv2d_forward_ex", &conv2d_forward_ex);
  m.def("conv2d_backward_input", &conv2d_backward_input);
  m.def("conv2d_backward_weight_acc", &conv2d_backward_weight_acc);
  m.def("set_implicit_gemm", &set_implicit_gemm);
  m.def("set_deterministic", &set_deterministic);
  m.def("deterministic", &deterministic);
  m.def("float_atomic_launches", &float_atomic_launches);
  // tests / tuning: force the tr16 TN tile and its split-K block target
  // (all 0 = the planner's choice)
  m.def("set_tr16_tune", &ps_gemm_set_tr_tune);
  m.def("set_implicit_threshold", &set_implicit_threshold);
  m.def("set_packed_conv", &set_packed_conv);
  m.def("khwc_layout", &khwc_layout);
  // one process can run either conv1 path: env overrides, read once here
  if (const char* e = std::getenv("PS_PACKED_CONV"))
    set_packed_conv(std::atoi(e) != 0);
  m.def("set_rowfused_conv", &set_rowfused_conv);
  m.def("set_rowfused_threshold", &set_rowfused_threshold);
  m.def("rowfused_conv", &rowfused_conv);
  m.def("rowfused_threshold", &rowfused_threshold);
  // tests only: cap on the row-fused kernels' persistent grid (0 = auto)
  m.def("set_rowfused_blocks", &ps_rowfused_set_blocks);
  if (const char* e = std::getenv("PS_ROWFUSED_CONV"))
    set_rowfused_conv(std::atoi(e) != 0);
  m.def("set_dgrad_fwd_threshold", &set_dgrad_fwd_threshold);
  m.def("concat_channels", &concat_channels);
  m.def("slice_channels", &slice_channels);
  m.def("split_channels", &split_channels);
  m.def("pool_max_forward", &pool_max_forward);
  m.def("pool_max_backward", &pool_max_backward);
  m.def("pool_ave_forward", &pool_ave_forward);
  m.def("pool_ave_backward", &pool_ave_backward);
  m.def("pool_stoch_forward_train", &pool_stoch_forward_train);
  m.def("pool_stoch_forward_test", &pool_stoch_forward_test);
  m.def("lrn_forward", &lrn_forward);
  m.def("lrn_backward", &lrn_backward);
  m.def("lrn_backward_tail", &lrn_backward_tail);
  m.def("pool_max_backward_tail", &pool_max_backward_tail);
  m.def("relu_backward_bias", &relu_backward_bias);
  m.def("set_bwd_tail_blocks", &set_bwd_tail_blocks);
  m.def("lrn_v8_ok", &ps_lrn_v8_ok);
  m.def("softmax_forward", &softmax_forward);
  m.def("softmax_backward", &softmax_backward);
  m.def("softmax_loss_forward", &softmax_loss_forward);
  m.def("softmax_loss_backward", &softmax_loss_backward);
  m.def("relu_forward", &relu_forward);
  m.def("relu_backward", &relu_backward);
  m.def("sigmoid_forward", &sigmoid_forward);
  m.def("sigmoid_backward", &sigmoid_backward);
  m.def("tanh_forward", &tanh_forward);
  m.def("tanh_backward", &tanh_backward);
  m.def("bnll_forward", &bnll_forward);
  m.def("bnll_backward", &bnll_backward);
  m.def("dropout_forward", &dropout_forward);
  m.def("dropout_backward", &dropout_backward);
  m.def("sgd_update", &sgd_update);
  m.def("sgd_update_lrdev", &sgd_update_lrdev);
  m.def("threshold_forward", &threshold_forward);
  m.def("eltwise_max_step", &eltwise_max_step);
  m.def("eltwise_max_backward", &eltwise_max_backward);
  m.def("contrastive_forward", &contrastive_forward);
  m.def("sgd_mt_prepare", &sgd_mt_prepare);
  m.def("sgd_mt_run", &sgd_mt_run);
  m.def("zero_mt_prepare", &zero_mt_prepare);
  m.def("zero_mt_run", &zero_mt_run);
  m.def("repack_mt_prepare", &repack_mt_prepare);
  m.def("blob_stats_plan", &blob_stats_plan);
  m.def("blob_stats_reduce_depth", &blob_stats_reduce_depth);
  m.def("blob_stats_max_blocks", &blob_stats_max_blocks);
  m.def("blob_stats", &blob_stats);
  m.def("blob_stats_mt_prepare", &blob_stats_mt_prepare);
  m.def("blob_stats_mt_run", &blob_stats_mt_run);
  m.def("blob_stats_finalize", &blob_stats_finalize);
  m.def("blob_stats_launches", &blob_stats_launches);
  m.def("colsum_mt_prepare", &colsum_mt_prepare);
  m.def("colsum_mt_run", &colsum_mt_run);
  m.def("colsum_acc", &colsum_acc);
  m.def("unpack_mt_prepare", &unpack_mt_prepare);
  m.def("unpack_mt_run", &unpack_mt_run);
  m.def("repack_mt_run", &repack_mt_run);
  m.def("dropout_forward_offdev", &dropout_forward_offdev);
  m.def("nesterov_update", &nesterov_update);
  m.def("adagrad_update", &adagrad_update);
  m.attr("compute_dtypes") = std::vector<std::string>{"float32", "bfloat16"};
}
