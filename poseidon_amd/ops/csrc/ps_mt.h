// Multi-tensor apply tables: one launch covers every tensor of a kind via a
// device-resident (descriptor, chunk) table the bindings build once --
// shapes are static so a table never changes. Shared by the kernels
// (sgd.hip, elementwise.hip) and the host code that fills the tables.
#pragma once
#include <cstdint>

#include "ps_conv_plan.h"  // ps_khwc_col

namespace ps {

// elements per workgroup: 256 threads x vec4 x 8 iters
constexpr int MT_CHUNK = 8192;

// workgroup -> (tensor index, start element)
struct MTChunk {
  int t;
  int64_t off;
};

struct MTDesc {  // SGD update
  float* w;
  const float* g;
  float* h;
  int64_t n;
  float lr_mult;
  float wd;
  void* shadow;  // bf16 copy of w in w's own flat layout, or null: written
                 // from the registers that hold the new weight
};

struct MTZeroDesc {
  float* p;
  int64_t n;
};

// conv weight repack: fp32 masters -> bf16 khwc shadow + per-group dgrad
// transpose
struct MTRepackDesc {
  const float* src;  // fp32 master, NCHW [Co][Cig][kh][kw]
  void* wk;          // bf16 [Co][ldk] khwc (pad cols pre-zeroed)
  void* wkT;         // bf16 [G*Kg][Cog]
  int64_t n;         // Co*Cig*kh*kw
  int Co, Cig, kh, kw, G, ldk;
  int kw_ld, c_ld;   // wk tap-row width / channel slots (ps_khwc_col)
};

// inverse of the repack for GRADIENTS: khwc fp32 wgrad scratch -> NCHW
struct MTUnpackDesc {
  const float* dwk;  // fp32 [Co][ldk] khwc
  float* dw;         // fp32 NCHW [Co][Cig][kh][kw], accumulated into
  int64_t n;         // Co*Cig*kh*kw
  int Co, Cig, kh, kw, ldk;
  int kw_ld, c_ld;   // dwk tap-row width / channel slots (ps_khwc_col)
  int overwrite;     // dw = ... instead of dw += ... (single-writer diffs
                     // that nobody zeroed)
};

// blob statistics (stats.hip); its chunks count BLOCKS of the tensor's plan
// (MTChunk.off = block index within the tensor)
struct StatsDesc {
  const void* p;  // dense storage, bf16 or fp32, element-aligned only
  int64_t n;
  int slot;
  int blocks;     // ps_stats_plan.h
  int bf16;
  int pad;
};

// bias colsum; its chunks count ROWS (ColsumChunk.off = start row)
struct ColsumDesc {
  const void* dy;
  float* db;
  int64_t R;
  int64_t rows_per;  // rows per chunk (block)
  int C;
};
struct ColsumChunk {
  int t;
  int64_t off;
};

}  // namespace ps
