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
};

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

// Deterministic mode, process-wide (initially PS_DETERMINISTIC=1): every
// float reduction runs in an order fixed by the shape and the plan. No
// launcher takes an atomic-float path while it is on.
void ps_set_deterministic(int on);
int ps_deterministic();
// Host-side count of launched kernel instantiations that add floats
// atomically (LDS or global): each launcher calls ps_count_float_atomic.
void ps_count_float_atomic();
int64_t ps_float_atomic_launches(int reset);

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
