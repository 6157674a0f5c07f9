// The decomposition of the cell scans (scene statistics, the joint histogram, derived fields): one
// tile = 4 k-planes x 4 j-rows x 128 cells along x of one box, the tiles of a box numbered chunk
// fastest, then the brick of rows along y, then along z.  The host's count and the device's decode
// of a tile number live here together (tests/cxx/field_boxes_test.cpp holds one against the other),
// with the device's shared steps: the search that finds a tile's box in the prefix sums of the
// boxes' tiles and the workgroup's prefix sum.
#ifndef AVR_CELL_TILES_H
#define AVR_CELL_TILES_H

#include <cstdint>

#include "avr_internal.h"

namespace avr {

// tiles of one box; UINT32_MAX if they do not fit 31 bits
inline uint32_t cell_tiles(int nx, int ny, int nz) {
  const uint64_t bricks_y = static_cast<uint64_t>((ny + kBrickY - 1) / kBrickY);
  const uint64_t bricks_z = static_cast<uint64_t>((nz + kBrickZ - 1) / kBrickZ);
  const uint64_t chunks = static_cast<uint64_t>((nx + kClassifyChunk - 1) / kClassifyChunk);
  const uint64_t tiles = bricks_y * bricks_z * chunks;
  return tiles < (uint64_t{1} << 31) ? static_cast<uint32_t>(tiles) : UINT32_MAX;
}

struct CellTile {
  int chunk, bj, bk;  // the tile's cells: i in [128 chunk, +128), j in [4 bj, +4), k in [4 bk, +4)
};

// What numbers a box's tiles: its chunks along x and its bricks of rows along y.  Apart from the
// decode, so that a kernel can work it out before it has loaded the tile's number (the order of
// its instructions follows the order here).
struct CellTileShape {
  int chunks, bricks_y;
};
AVR_HD inline __attribute__((always_inline)) CellTileShape cell_tile_shape(int nx, int ny) {
  CellTileShape s;
  s.bricks_y = (ny + kBrickY - 1) >> 2;
  s.chunks = (nx + kClassifyChunk - 1) / kClassifyChunk;
  return s;
}
// Tile number `local` (< cell_tiles) of a box -> its chunk and its brick of rows.
AVR_HD inline __attribute__((always_inline)) CellTile cell_tile_of(const CellTileShape& s,
                                                                   uint32_t local) {
  CellTile t;
  t.chunk = static_cast<int>(local % static_cast<uint32_t>(s.chunks));
  local /= static_cast<uint32_t>(s.chunks);
  t.bj = static_cast<int>(local % static_cast<uint32_t>(s.bricks_y));
  t.bk = static_cast<int>(local / static_cast<uint32_t>(s.bricks_y));
  return t;
}
AVR_HD inline __attribute__((always_inline)) CellTile cell_tile_of(int nx, int ny, uint32_t local) {
  return cell_tile_of(cell_tile_shape(nx, ny), local);
}

#if defined(__HIP__)
// The box that entry number `at` of a prefix sum belongs to: the largest b with begin[b] <= at
// (binary search).  P: a pointer to T, the sums' type, in whichever address space the kernel reads
// them through.
template <typename P, typename T>
__device__ __forceinline__ int locate_box(P begin, int n_boxes, T at) {
  int lo = 0, hi = n_boxes;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (begin[mid] <= at) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// The sum of v over the workgroup's THREADS lanes before this one, and over all of them.  `slot` <
// SLOTS: the caller's call number, each call of a kernel has its own LDS.
template <int THREADS, int SLOTS>
__device__ __forceinline__ uint32_t block_exclusive_sum(uint32_t v, int slot, uint32_t* total) {
  __shared__ uint32_t wave_sums[SLOTS][THREADS / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inclusive = v;
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) {
    const uint32_t below = __shfl_up(inclusive, step, 64);
    if (lane >= static_cast<uint32_t>(step)) inclusive += below;
  }
  if (lane == 63u) wave_sums[slot][wave] = inclusive;
  __syncthreads();
  uint32_t before = inclusive - v, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < THREADS / 64; ++w) {
    const uint32_t s = wave_sums[slot][w];
    if (w < wave) before += s;
    all += s;
  }
  *total = all;
  return before;
}
#endif

}  // namespace avr

#endif
