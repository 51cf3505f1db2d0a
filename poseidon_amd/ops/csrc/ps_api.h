// C API between the HIP kernel translation units and the torch bindings.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "ps_conv_plan.h"  // ConvGeom, GatherDesc, ConvPlan
#include "ps_gemm_plan.h"  // GemmPlan, TrTune
#include "ps_stats_plan.h"  // StatsPlan, StatsRec
#include "ps_transform.h"  // TransformGeom, PS_MEAN_*

struct GemmArgs {
  const void* A;
  const void* B;
  void* C;
  const float* bias;  // may be null
  int M, N, K;
  int64_t lda, ldb, ldc;
  float alpha, beta;
  bool a_klast, b_klast;
  bool in_bf16;   // A/B are bf16 (else fp32)
  bool out_f32;   // C is fp32 (else bf16; fp32 inputs require fp32 out)
  // implicit-GEMM: gather A (K-last rows = im2col rows) / gather B (K-major)
  const GatherDesc* gather_a;
  const GatherDesc* gather_b;
  // fused epilogue: y = max(y, 0) (conv/IP + in-place ReLU pairs)
  bool relu;
  // caller guarantees C is already zero (net-level zero_mt): atomic
  // split-K skips its per-launch memset
  bool c_prezeroed;
  // >= 16 B of zeros on the operands' device, or null: what the tr16 K-tails
  // (TN and NN) read for the dead k of materialized operands (K % 64 != 0)
  const void* zero = nullptr;
};

// the tr16 K-tail switch's value without PS_TR16_KTAIL (ps_set_tr16_ktail)
constexpr int PS_TR16_KTAIL_DEFAULT = 1;

// fp32 K elements per staged tile of the split-precision kernel
constexpr int PS_SPLIT3_BK = 32;

struct PoolGeom {
  int N, C, H, W, Ho, Wo;
  int kh, kw, sh, sw, ph, pw;
};

extern "C" {
// gemm.hip
void ps_gemm_plan(const GemmArgs* g, GemmPlan* plan);
void ps_gemm_run(const GemmArgs* g, const GemmPlan* plan, float* ws,
                 hipStream_t s);
// tests / tuning: force the tr16 tile and split-K block target (0 = planner)
void ps_gemm_set_tr_tune(int bm, int bn, int target);
// tr16 K-tail, process-wide (initially PS_TR16_KTAIL=0/1, else the default
// below): ps_gemm_plan lets K % 64 != 0 contractions with K > 64 take the
// tr16 kernel, whose last K tile then reads its dead rows from a zero page.
void ps_set_tr16_ktail(int on);
int ps_tr16_ktail();
// NN tr16, process-wide (initially PS_TR16_NN=0/1, default off): ps_gemm_plan
// sends bf16 GEMMs with a K-last A and a K-major B (the InnerProduct data
// gradients) to gemm_nn_tr_kernel where ps_nn_tr_plan takes them. Its K-tail
// (K % 64 != 0) needs GemmArgs::zero and does not depend on the TN switch.
void ps_set_tr16_nn(int on);
int ps_tr16_nn();
// host-side count of gemm_nn_tr_kernel launches
int64_t ps_tr16_nn_launches(int reset);
// The skinny plan (ps_gemm_plan.h): kmin > 0 switches it on with that K-slice
// floor, 0 switches it off; bm, bn, splitk force its tile and depth for
// tests and tuning runs (0 = planner).
void ps_gemm_set_skinny(int kmin, int bm, int bn, int splitk);
int ps_gemm_skinny_kmin();

// Deterministic mode, process-wide (initially PS_DETERMINISTIC=1): every
// float reduction runs in an order fixed by the shape and the plan. No
// launcher takes an atomic-float path while it is on.
void ps_set_deterministic(int on);
int ps_deterministic();
// Host-side count of launched kernel instantiations that add floats
// atomically (LDS or global): each launcher calls ps_count_float_atomic.
void ps_count_float_atomic();
int64_t ps_float_atomic_launches(int reset);

// gemm_split.hip: split-precision fp32 GEMMs. Each fp32 operand is staged as
// two bf16 images hi + lo and a product is three bf16 MFMAs (lo*hi + hi*lo +
// hi*hi) into the fp32 accumulator. The switch is process-wide (initially
// PS_FP32_SPLIT=1, default off); ps_gemm_plan reads it and marks the plans
// that ps_gemm_run then sends to ps_gemm_split_run.
void ps_set_fp32_split(int on);
int ps_fp32_split();
// host-side count of ps_gemm_split_run launches
int64_t ps_fp32_split_launches(int reset);
// a generic plan with split3 set; split-K zeroing / workspace as ps_gemm_run
void ps_gemm_split_run(const GemmArgs* g, const GemmPlan* plan, float* ws,
                       hipStream_t s);

// elementwise.hip
void ps_relu_fwd_f32(const float*, float*, int64_t, float, hipStream_t);
void ps_relu_bwd_f32(const float*, const float*, float*, int64_t, float, hipStream_t);
void ps_sigmoid_fwd_f32(const float*, float*, int64_t, hipStream_t);
void ps_sigmoid_bwd_f32(const float*, const float*, float*, int64_t, hipStream_t);
void ps_tanh_fwd_f32(const float*, float*, int64_t, hipStream_t);
void ps_tanh_bwd_f32(const float*, const float*, float*, int64_t, hipStream_t);
void ps_bnll_fwd_f32(const float*, float*, int64_t, hipStream_t);
void ps_bnll_bwd_f32(const float*, const float*, float*, int64_t, hipStream_t);
void ps_dropout_fwd_f32(const float*, float*, uint8_t*, int64_t, float,
                        uint64_t, uint64_t, hipStream_t);
void ps_dropout_bwd_f32(const float*, const uint8_t*, float*, int64_t, float,
                        hipStream_t);
// out[c] += column sums of in[R][C]. scratch: ps_colsum_scratch_elems(R, C)
// floats (deterministic mode's [blocks][C] partials; null when that is 0)
int64_t ps_colsum_scratch_elems(int64_t R, int C, int bf16);
void ps_colsum_f32(const float*, float*, int64_t, int, float* scratch,
                   hipStream_t);
void ps_relu_fwd_bf16(const void*, void*, int64_t, float, hipStream_t);
void ps_relu_bwd_bf16(const void*, const void*, void*, int64_t, float, hipStream_t);
// slope-0 relu backward + bias colsum: (x, dy, dx, db, rows, C, max blocks)
void ps_relu_bwd_bias_f32(const float*, const float*, float*, float*, int64_t,
                          int, int, hipStream_t);
void ps_relu_bwd_bias_bf16(const void*, const void*, void*, float*, int64_t,
                           int, int, hipStream_t);
void ps_sigmoid_fwd_bf16(const void*, void*, int64_t, hipStream_t);
void ps_sigmoid_bwd_bf16(const void*, const void*, void*, int64_t, hipStream_t);
void ps_tanh_fwd_bf16(const void*, void*, int64_t, hipStream_t);
void ps_tanh_bwd_bf16(const void*, const void*, void*, int64_t, hipStream_t);
void ps_bnll_fwd_bf16(const void*, void*, int64_t, hipStream_t);
void ps_bnll_bwd_bf16(const void*, const void*, void*, int64_t, hipStream_t);
void ps_dropout_fwd_bf16(const void*, void*, uint8_t*, int64_t, float,
                         uint64_t, uint64_t, hipStream_t);
void ps_dropout_bwd_bf16(const void*, const uint8_t*, void*, int64_t, float,
                         hipStream_t);
void ps_colsum_bf16(const void*, float*, int64_t, int, float* scratch,
                    hipStream_t);
// (descs, chunks, nchunks, bf16, max C, tensors, scratch [nchunks][max C] in
// deterministic mode | null)
void ps_colsum_mt(const void*, const void*, int, int, int, int, float*,
                  hipStream_t);
void ps_threshold_fwd_f32(const float*, float*, int64_t, float, hipStream_t);
void ps_threshold_fwd_bf16(const void*, void*, int64_t, float, hipStream_t);
void ps_eltwise_max_fwd_f32(const float*, const float*, float*, uint8_t*,
                            int64_t, int, hipStream_t);
void ps_eltwise_max_fwd_bf16(const void*, const void*, void*, uint8_t*,
                             int64_t, int, hipStream_t);
void ps_eltwise_max_bwd_f32(const float*, const uint8_t*, float*, int64_t,
                            int, hipStream_t);
void ps_eltwise_max_bwd_bf16(const void*, const uint8_t*, void*, int64_t,
                             int, hipStream_t);
void ps_contrastive_fwd_f32(const float*, const float*, float*, int64_t,
                            float, int, hipStream_t);
void ps_dropout_fwd_f32_offdev(const float*, float*, uint8_t*, int64_t, float,
                               uint64_t, const void*, hipStream_t);
void ps_dropout_fwd_bf16_offdev(const void*, void*, uint8_t*, int64_t, float,
                                uint64_t, const void*, hipStream_t);

// pool.hip
void ps_maxpool_fwd_f32(const float*, float*, uint8_t*, const PoolGeom*, hipStream_t);
void ps_maxpool_bwd_f32(const float*, const uint8_t*, float*, const PoolGeom*, hipStream_t);
void ps_avepool_fwd_f32(const float*, float*, const PoolGeom*, hipStream_t);
void ps_avepool_bwd_f32(const float*, float*, const PoolGeom*, hipStream_t);
void ps_stochpool_fwd_train_f32(const float*, float*, uint8_t*, const PoolGeom*,
                                uint64_t, hipStream_t);
void ps_stochpool_fwd_test_f32(const float*, float*, const PoolGeom*, hipStream_t);
void ps_maxpool_fwd_bf16(const void*, void*, uint8_t*, const PoolGeom*, hipStream_t);
void ps_maxpool_bwd_bf16(const void*, const uint8_t*, void*, const PoolGeom*, hipStream_t);
// fused conv -> relu -> max pool tail: (dy, mask, x | null, dx, db | null,
// geom, max blocks)
void ps_maxpool_bwd_tail_f32(const float*, const uint8_t*, const float*,
                             float*, float*, const PoolGeom*, int, hipStream_t);
void ps_maxpool_bwd_tail_bf16(const void*, const uint8_t*, const void*, void*,
                              float*, const PoolGeom*, int, hipStream_t);
void ps_avepool_fwd_bf16(const void*, void*, const PoolGeom*, hipStream_t);
void ps_avepool_bwd_bf16(const void*, void*, const PoolGeom*, hipStream_t);

// lrn.hip
void ps_lrn_fwd_f32(const float*, float*, float*, int64_t, int, int, float,
                    float, hipStream_t);
void ps_lrn_bwd_f32(const float*, const float*, const float*, const float*,
                    float*, float*, int64_t, int, int, float, float, hipStream_t);
void ps_lrn_fwd_bf16(const void*, void*, float*, int64_t, int, int, float,
                     float, hipStream_t);
void ps_lrn_bwd_bf16(const void*, const void*, const float*, const void*,
                     void*, float*, int64_t, int, int, float, float, hipStream_t);
// halo-register path (no scale tensor), C % 8 == 0
int ps_lrn_v8_ok(int C, int size);
void ps_lrn_fwd_v8_f32(const float*, float*, int64_t, int, int, float, float,
                       hipStream_t);
void ps_lrn_fwd_v8_bf16(const void*, void*, int64_t, int, int, float, float,
                        hipStream_t);
void ps_lrn_bwd_v8_f32(const float*, const float*, const float*, float*,
                       int64_t, int, int, float, float, hipStream_t);
void ps_lrn_bwd_v8_bf16(const void*, const void*, const void*, void*, int64_t,
                        int, int, float, float, hipStream_t);
// fused conv -> relu -> lrn [-> max pool] tail: (x, y, dy, pool mask | null,
// pool geom | null, dx, db | null, relu, rows, C, size, alpha, beta, max
// blocks of a launch that sums db). With a mask, dy is the POOL's top diff.
void ps_lrn_bwd_v8_tail_f32(const float*, const float*, const float*,
                            const uint8_t*, const PoolGeom*, float*, float*,
                            int, int64_t, int, int, float, float, int,
                            hipStream_t);
void ps_lrn_bwd_v8_tail_bf16(const void*, const void*, const void*,
                             const uint8_t*, const PoolGeom*, void*, float*,
                             int, int64_t, int, int, float, float, int,
                             hipStream_t);

// lrn_within.hip: WITHIN_CHANNEL LRN on NHWC tensors, sizes 3 / 5 / 7.
// fwd (x, y, N, C, H, W, size, alpha, beta); bwd (x, dy, dx, ...) recomputes
// the scale. Not in place: x, dy and the output are distinct.
int ps_lrn_within_ok(int C, int size, int itemsize);
void ps_lrn_within_fwd_f32(const float*, float*, int, int, int, int, int,
                           float, float, hipStream_t);
void ps_lrn_within_fwd_bf16(const void*, void*, int, int, int, int, int,
                            float, float, hipStream_t);
void ps_lrn_within_bwd_f32(const float*, const float*, float*, int, int, int,
                           int, int, float, float, hipStream_t);
void ps_lrn_within_bwd_bf16(const void*, const void*, void*, int, int, int,
                            int, int, float, float, hipStream_t);
// tests only: rows a block emits (0 = the plan's own)
void ps_lrn_within_set_strip(int n);
// host-side count of the launches above
int64_t ps_lrn_within_launches(int reset);

// mvn.hip: mean-variance normalisation of N images of P pixels x C channels,
// channels innermost; across: one set per image, else one per (image,
// channel). fwd (x, y, stats, ws, N, C, P, across, norm_var, vec) writes
// (mean, rstd) fp32 pairs, [N] or [N * C] of them; bwd (x, dy, dx, stats, ws,
// ...) reads them. vec: x, dy and the output are 16-byte aligned. ws:
// ps_mvn_ws_floats() floats (0: none needed). Not in place.
int64_t ps_mvn_ws_floats(int64_t N, int64_t C, int64_t P, int itemsize,
                         int across, int backward, int vec);
void ps_mvn_fwd_f32(const float*, float*, float*, float*, int64_t, int64_t,
                    int64_t, int, int, int, hipStream_t);
void ps_mvn_fwd_bf16(const void*, void*, float*, float*, int64_t, int64_t,
                     int64_t, int, int, int, hipStream_t);
void ps_mvn_bwd_f32(const float*, const float*, float*, float*, float*,
                    int64_t, int64_t, int64_t, int, int, int, hipStream_t);
void ps_mvn_bwd_bf16(const void*, const void*, void*, float*, float*, int64_t,
                     int64_t, int64_t, int, int, int, hipStream_t);
// tests only: chunks per slab of the split regime (0 = the plan's own)
void ps_mvn_set_split(int n);
// host-side count of the launches above
int64_t ps_mvn_launches(int reset);

// softmax.hip
void ps_softmax_rows_f32(const float*, float*, int64_t, int, hipStream_t);
void ps_softmax_bwd_rows_f32(const float*, const float*, float*, int64_t, int,
                             hipStream_t);
// (x, labels, prob, loss, row_loss, rows, C): loss += sum of -log p. With
// row_loss (rows floats; required in deterministic mode) each row's term is
// stored there and one block sums them in a fixed order into loss.
void ps_softmax_loss_fwd_f32(const float*, const float*, float*, float*,
                             float*, int64_t, int, hipStream_t);
void ps_softmax_loss_bwd_f32(const float*, const float*, float*, int64_t, int,
                             float, hipStream_t);
void ps_softmax_rows_bf16(const void*, void*, int64_t, int, hipStream_t);
void ps_softmax_bwd_rows_bf16(const void*, const void*, void*, int64_t, int,
                              hipStream_t);
void ps_softmax_loss_fwd_bf16(const void*, const float*, void*, float*,
                              float*, int64_t, int, hipStream_t);
void ps_softmax_loss_bwd_bf16(const void*, const float*, void*, int64_t, int,
                              float, hipStream_t);
// loss[0] += partial[0 .. n), one block, in a fixed order (loss_sum_k)
void ps_loss_sum(const float* partial, float* loss, int64_t n, hipStream_t);

// softmax_dense.hip: per-position softmax loss over rows of C contiguous
// logits (rows = N*H*W of a channels-last blob), labels[rows] fp32. Lane-group
// kernels, plan in ps_softmax_dense_plan.h; they take what
// ps_softmax_dense_ok() accepts and 16-byte aligned tensors, anything else
// belongs on the wave-per-row kernels above.
// fwd (x, labels, prob, loss, partial, rows, C, max_blocks): loss += mean of
// -log p over the rows, by one atomicAdd per block, or with partial
// (ps_softmax_dense_blocks() floats; required in deterministic mode) by one
// ordered sum of the blocks' terms. max_blocks: cap of the grid, 0 = the
// plan's own; the same value sizes partial.
// bwd (prob, labels, dx, rows, C, w): dx = (prob - onehot) * w.
int ps_softmax_dense_ok(int64_t rows, int64_t C, int itemsize);
int ps_softmax_dense_max_c();
int64_t ps_softmax_dense_blocks(int64_t rows, int C, int itemsize,
                                int max_blocks);
void ps_softmax_dense_fwd_f32(const float*, const float*, float*, float*,
                              float*, int64_t, int, int, hipStream_t);
void ps_softmax_dense_fwd_bf16(const void*, const float*, void*, float*,
                               float*, int64_t, int, int, hipStream_t);
void ps_softmax_dense_bwd_f32(const float*, const float*, float*, int64_t, int,
                              float, hipStream_t);
void ps_softmax_dense_bwd_bf16(const void*, const float*, void*, int64_t, int,
                               float, hipStream_t);
// host-side count of the launches above and of softmax_heads.hip's
// lane-group kernels, which add theirs with ps_softmax_dense_count_launch()
int64_t ps_softmax_dense_launches(int reset);
void ps_softmax_dense_count_launch();

// softmax_heads.hip: the plain softmax over rows of C contiguous elements
// (rows = N*H*W of a channels-last blob) on lane-group kernels, for what
// ps_softmax_dense_ok() accepts and 16-byte aligned tensors.
// fwd (x, y, rows, C): y = softmax(x) per row.
// bwd (y, dy, dx, rows, C): dx = (dy - sum_c dy * y) * y per row.
void ps_softmax_heads_fwd_f32(const float*, float*, int64_t, int, hipStream_t);
void ps_softmax_heads_fwd_bf16(const void*, void*, int64_t, int, hipStream_t);
void ps_softmax_heads_bwd_f32(const float*, const float*, float*, int64_t, int,
                              hipStream_t);
void ps_softmax_heads_bwd_bf16(const void*, const void*, void*, int64_t, int,
                               hipStream_t);
// (x, labels, count, acc, rows, C, top_k, lane_groups): top-k accuracy over
// the rows by rank counting, labels[rows] fp32. count (pre-zeroed int32) +=
// the rows whose label has fewer than top_k elements ahead of it (greater, or
// equal with a higher index); a label outside [0, C) or a NaN at the label
// is a miss. acc[0] = count / rows, on the device. lane_groups: the
// lane-group kernel where ps_softmax_dense_ok() holds (x then 16-byte
// aligned), else and above SD_MAX_C one wave per row. 1 <= top_k <= C.
void ps_accuracy_rows_f32(const float*, const float*, int*, float*, int64_t,
                          int, int, int, hipStream_t);
void ps_accuracy_rows_bf16(const void*, const float*, int*, float*, int64_t,
                           int, int, int, hipStream_t);

// sgd.hip
void ps_sgd_update(float*, const float*, float*, int64_t, float, float, float,
                   hipStream_t);
void ps_nesterov_update(float*, const float*, float*, int64_t, float, float,
                        float, hipStream_t);
void ps_adagrad_update(float*, const float*, float*, int64_t, float, float,
                       float, hipStream_t);
void ps_f32_to_bf16(const float*, void*, int64_t, hipStream_t);
void ps_sgd_update_lrdev(float*, const float*, float*, int64_t, float, float,
                         float, const float*, hipStream_t);
void ps_u64_inc(void*, hipStream_t);
// multi-tensor apply (descriptor/chunk tables built by bindings; layouts in
// ps_mt.h)
void ps_sgd_mt(const void* descs, const void* chunks, int nchunks, float lr,
               float mom, const float* lr_dev, hipStream_t);
void ps_zero_mt(const void* descs, const void* chunks, int nchunks,
                hipStream_t);
void ps_repack_mt(const void* descs, const void* chunks, int nchunks,
                  hipStream_t);
void ps_unpack_mt(const void* descs, const void* chunks, int nchunks,
                  hipStream_t);

// stats.hip: blob statistics for debug_info (ps_stats_plan.h). scratch is
// [slots][STATS_MAX_BLOCKS] StatsRec partials, nblk [slots] the block count
// each slot was last launched with, stats [slots] StatsRec.
void ps_blob_stats(const void* p, int64_t n, int bf16, int slot,
                   void* scratch, int* nblk, hipStream_t);
// (StatsDesc table, MTChunk table with off = block index, chunks)
void ps_blob_stats_mt(const void* descs, const void* chunks, int nchunks,
                      void* scratch, int* nblk, hipStream_t);
void ps_blob_stats_finalize(const void* scratch, const int* nblk, void* stats,
                            int slot0, int nslots, hipStream_t);
// host-side count of the three launches above
int64_t ps_blob_stats_launches(int reset);

// transform.hip: (raw uint8 [N,C,H,W], params int32 [N,3], mean | null, out
// [N,C,Ho,Wo], geom). out must be aligned to 8 of its elements.
void ps_data_transform_f32(const uint8_t*, const int*, const float*, float*,
                           const TransformGeom*, hipStream_t);
void ps_data_transform_bf16(const uint8_t*, const int*, const float*, void*,
                            const TransformGeom*, hipStream_t);

// conv_rowfused.hip: row-fused first layer (ps_rowfused.h), bf16 only. x is
// read through its element strides (sn, sc, sh, sw) and never outside its
// element span [0, span) (RowFusedX); wk is the khwc shadow [Co][Kpad];
// y / dy are NHWC rows; dwk is f32 [Co][Kpad], added to atomically (cleared
// first unless prezeroed).
void ps_conv_rowfused_fwd(const RowFusedTiling*, const void* x, int64_t sn,
                          int64_t sc, int64_t sh, int64_t sw, int64_t span,
                          const void* wk, const float* bias, void* y,
                          int relu, hipStream_t);
void ps_conv_rowfused_wgrad(const RowFusedTiling*, const void* x, int64_t sn,
                            int64_t sc, int64_t sh, int64_t sw, int64_t span,
                            const void* dy, float* dwk, int prezeroed,
                            hipStream_t);
// once per process, when a plan comes out row-fused: reads the CU count and
// sets the kernels' LDS attribute; 0 = no usable device
int ps_rowfused_prepare();
// tests only: cap on the persistent grid (0 = one block per CU)
void ps_rowfused_set_blocks(int n);

// conv_halo.hip: halo-tile direct conv (ps_halo.h), bf16 NHWC in and out,
// stride 1. w is K-last khwc rows w_ld elements apart: the forward's wk or
// the dgrad-as-forward's wr (in = dy, pads k - 1 - p, no bias, no relu).
void ps_conv_halo(const HaloTiling*, const void* in, const void* w,
                  int64_t w_ld, const float* bias, void* out, int relu,
                  hipStream_t);
// once per process, when a plan comes out halo: reads the CU count and sets
// the kernels' LDS attribute; 0 = no usable device
int ps_halo_prepare();
// persistent grid size for ps_halo_tiling: the tests' cap, else the CU count
int ps_halo_max_blocks();
// tests only: cap on the persistent grid (0 = one block per CU)
void ps_halo_set_blocks(int n);
// host-side count of ps_conv_halo launches
int64_t ps_halo_launches(int reset);

// im2col.hip
void ps_chan_concat4_f32(float*, void* const*, const int*, int, int, int64_t,
                         int, int, const void* const*, hipStream_t);
void ps_chan_concat4_bf16(void*, void* const*, const int*, int, int, int64_t,
                          int, int, const void* const*, hipStream_t);
void ps_chan_copy_f32(const float*, float*, int64_t, int, int, int, hipStream_t);
void ps_chan_copy_bf16(const void*, void*, int64_t, int, int, int, hipStream_t);
void ps_chan_slice_f32(const float*, float*, int64_t, int, int, int, hipStream_t);
void ps_chan_slice_bf16(const void*, void*, int64_t, int, int, int, hipStream_t);
void ps_im2col_nhwc_f32(const float*, float*, const ConvGeom*, int ldcol,
                        hipStream_t);
// rowstage im2col through x's element strides; false = not its shape
bool ps_im2col_rowstage_f32(const float*, float*, const ConvGeom*, int ldcol,
                            int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                            hipStream_t);
bool ps_im2col_rowstage_bf16(const void*, void*, const ConvGeom*, int ldcol,
                             int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                             hipStream_t);
void ps_col2im_nhwc_f32(const float*, float*, const ConvGeom*, hipStream_t);
void ps_im2col_nhwc_bf16(const void*, void*, const ConvGeom*, int ldcol,
                         hipStream_t);
void ps_col2im_nhwc_bf16(const void*, void*, const ConvGeom*, hipStream_t);
void ps_weight_to_khwc_f32(const float*, float*, int, int, int, int, hipStream_t);
void ps_weight_to_khwc_f32_bf16(const float*, void*, int, int, int, int, hipStream_t);
void ps_zero_cols_f32(float*, int64_t rows, int ld, int c_lo, hipStream_t);
void ps_zero_cols_bf16(void*, int64_t rows, int ld, int c_lo, hipStream_t);
void ps_weight_to_dgrad_f32(const float*, float*, int, int, int, int, int,
                            hipStream_t);
void ps_weight_to_dgrad_f32_bf16(const float*, void*, int, int, int, int,
                                 int, hipStream_t);
void ps_weight_from_khwc_f32(const float*, float*, int, int, int, int,
                             int ld, float beta, int kw_ld, int c_ld,
                             hipStream_t);
void ps_weight_to_khwc_tr_f32(const float*, float*, int, int, int, int, int,
                              hipStream_t);
void ps_weight_to_khwc_tr_f32_bf16(const float*, void*, int, int, int, int,
                                   int, hipStream_t);
void ps_weight_to_khwc_both_f32(const float*, float*, float*, int, int, int,
                                int, int, int ldk, int kw_ld, int c_ld,
                                hipStream_t);
void ps_weight_to_khwc_both_f32_bf16(const float*, void*, void*, int, int,
                                     int, int, int, int ldk, int kw_ld,
                                     int c_ld, hipStream_t);
// x (bf16, element strides sn/sc/sh/sw) -> xp[N][H][Wp][8]
void ps_pack_pairs_bf16(const void* x, void* xp, int N, int C, int H, int W,
                        int Wp, int pw, int64_t sn, int64_t sc, int64_t sh,
                        int64_t sw, hipStream_t);
}
