// Launch plan of the dense softmax-loss kernels (softmax_dense.hip): rows of
// C contiguous logits, one row per (n, h, w) of a channels-last blob, C small
// and rows in the millions. Host-only arithmetic on the problem shape,
// derived once per launch.
//
// A row belongs to a group of G lanes (a power of two, 1 .. 64) and lane j of
// the group owns the elements j, j + G, j + 2G of it, at most
// SD_MAX_PER_LANE, in registers. A wave serves 64 / G rows at a time and a
// block of SD_THREADS lanes 256 / G. A block's tile is TR consecutive rows:
// one contiguous span of TR * C elements that moves global <-> LDS in 16-byte
// vectors, with the rows' TR labels staged behind it. TR is a multiple of
// both 256 / G (every pass of the block is full but the last tile's) and
// 16 / itemsize (so TR * C * itemsize is a multiple of 16 and every tile
// starts 16-byte aligned when the tensor does).
//
// LDS layout: the tile is a plain image of global memory, row pitch C, no
// padding -- padding a row would turn the 16-byte staging stores into
// per-element scatters. Reasoned from 64 banks x 4 bytes (what the other
// kernels of this project assume for gfx950), a lane group's read of its
// k-th element touches G consecutive elements and the groups of a wave sit C
// apart. Odd C / G, or a ragged last element (C not a multiple of G), spreads
// the groups over the banks by itself, partly overlapping at worst. What
// serialises is C == 2 G, every power-of-two C: all groups read even
// G-blocks, then all read odd ones, half the banks each time. For exactly
// that case lanes visit their two elements in opposite orders
// (sd_flip(lane)), quarter-wave by quarter-wave, so that one read covers
// even blocks from half the lanes and odd blocks from the other half: all 64
// banks once under a 64-lane x 64-bank model and all 32 once under a
// 32-lane x 32-bank one. 2-byte elements halve the dwords a read spans and
// had no two-way case to begin with. None of this has been measured with the
// bank-conflict counter.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ps {

constexpr int SD_THREADS = 256;
// elements of a row one lane keeps in registers
constexpr int SD_MAX_PER_LANE = 3;
// largest C the lane-group kernels take (G = 64); above it the dense path
// runs the wave-per-row kernels of softmax.hip
constexpr int SD_MAX_C = 64 * SD_MAX_PER_LANE;
// LDS of a block, tile and labels: 16 KiB lets eight blocks (all 32 wave
// slots of a CU) share the 160 KiB, so some stream while others reduce;
// about 4 vectors a lane
constexpr int SD_TILE_BYTES = 16 << 10;
constexpr int SD_LDS_BANKS = 64;  // x 4 bytes; see the layout note above
// fewer blocks than this leave CUs idle: tiles shrink to reach it
constexpr int64_t SD_FILL_BLOCKS = 1024;
// blocks of the forward, 4 a CU: each ends in one atomicAdd on the loss (or
// one partial), and adds to one address do not overlap
constexpr int SD_MAX_BLOCKS = 1024;

struct SoftmaxDensePlan {
  int G;         // lanes of a row's group; 0: beyond the lane-group range
  int per_lane;  // ceil(C / G) <= SD_MAX_PER_LANE
  int flip;      // C == 2 G: lanes alternate the order of their two elements
  int TR;        // rows of a tile
  int64_t tiles;   // the backward's grid: a tile a block
  int64_t blocks;  // the forward's: a block walks every blocks-th tile
  size_t lds;    // dynamic LDS bytes of a block: the tile, then its labels
};

// bytes of the tile proper; the TR fp32 labels follow it
__host__ __device__ inline int sd_tile_bytes(int TR, int C, int itemsize) {
  return (TR * C * itemsize + 15) & ~15;
}

__host__ __device__ inline int sd_flip(int lane) {
  return ((lane >> 4) ^ (lane >> 5)) & 1;
}

inline bool sd_lane_group_ok(int64_t rows, int64_t C, int itemsize) {
  return rows >= 1 && C >= 1 && C <= SD_MAX_C &&
         (itemsize == 2 || itemsize == 4);
}

// max_blocks: cap of the forward's grid (0 = SD_MAX_BLOCKS; tests lower it
// so that the blocks of a small tensor walk several tiles)
inline SoftmaxDensePlan sd_plan(int64_t rows, int C, int itemsize,
                                int max_blocks) {
  SoftmaxDensePlan p{};
  if (!sd_lane_group_ok(rows, C, itemsize)) return p;
  p.G = 1;
  while (p.G * SD_MAX_PER_LANE < C) p.G *= 2;
  p.per_lane = (C + p.G - 1) / p.G;
  p.flip = C == 2 * p.G;
  const int vn = 16 / itemsize;
  const int rb = SD_THREADS / p.G;
  const int unit = rb > vn ? rb : vn;  // both powers of two
  int64_t k = SD_TILE_BYTES / ((int64_t)unit * (C * itemsize + 4));
  const int64_t fill = rows / (unit * SD_FILL_BLOCKS);
  if (k > fill) k = fill;
  if (k < 1) k = 1;
  p.TR = (int)(k * unit);
  p.tiles = (rows + p.TR - 1) / p.TR;
  const int64_t cap = max_blocks > 0 ? max_blocks : SD_MAX_BLOCKS;
  p.blocks = p.tiles < cap ? p.tiles : cap;
  p.lds = (size_t)sd_tile_bytes(p.TR, C, itemsize) + 4 * (size_t)p.TR;
  return p;
}

// The plan of a kernel that keeps `streams` tiles of the same TR rows in LDS
// at once (softmax_heads.hip: the softmax backward stages y and dy, 2; the
// softmax forward and the accuracy kernel stage one). The tiles lie one
// behind the other, each sd_tile_bytes() long, the room of TR labels behind
// the last; TR follows sd_plan's unit rule and is sized so that all of it
// fits SD_TILE_BYTES. streams == 1 is sd_plan.
//
// Two tiles of pitch C, reasoned as above and as little measured: a lane
// reads y[r][c] and dy[r][c] with two instructions, so the tiles never meet
// in one access, and the second tile is the first one moved by
// sd_tile_bytes(), the same number of banks for every lane -- a rotation of
// the bank pattern, which conflicts exactly where the single tile does. The
// C == 2 G flip therefore serves both reads, and the dx store, which goes to
// the address its lane read dy from, repeats the dy read's pattern. What two
// tiles change is TR (about half), not the access.
inline SoftmaxDensePlan sd_plan_streams(int64_t rows, int C, int itemsize,
                                        int streams) {
  SoftmaxDensePlan p = sd_plan(rows, C, itemsize, 0);
  if (p.G == 0 || streams <= 1) return p;
  const int vn = 16 / itemsize;
  const int rb = SD_THREADS / p.G;
  const int unit = rb > vn ? rb : vn;
  int64_t k = SD_TILE_BYTES /
              ((int64_t)unit * ((int64_t)streams * C * itemsize + 4));
  const int64_t fill = rows / (unit * SD_FILL_BLOCKS);
  if (k > fill) k = fill;
  if (k < 1) k = 1;
  p.TR = (int)(k * unit);
  p.tiles = (rows + p.TR - 1) / p.TR;
  p.blocks = p.tiles < SD_MAX_BLOCKS ? p.tiles : SD_MAX_BLOCKS;
  p.lds = (size_t)streams * sd_tile_bytes(p.TR, C, itemsize) +
          4 * (size_t)p.TR;
  // one unit of rows always fits for streams <= 2; more may not
  if (p.lds > (size_t)SD_TILE_BYTES) p = SoftmaxDensePlan{};
  return p;
}

}  // namespace ps
