// Grid fields ("Grid fields"): a uniform grid of level L over a region of that
// level's index space written onto every cell of a scene's boxes -- the inverse of the covering
// grid (avr_covering_grid.hip).
//
//   grid_field_kernel     16 consecutive tiles per workgroup, one or two cells per lane and pass
//
// The output is streamed as derive_kernel streams it (avr_cell_tiles.h): one tile = 4 k-planes x 4
// j-rows x 128 cells of one box, rows written coalesced and as f64 pairs where the box allows it
// (box.paired), 16 consecutive tiles per workgroup, the workgroup's box found once and walked on
// from there.  The box table, the tile prefix sums and the level table are read through the
// constant address space: scalar loads, once per tile.
//
// A cell with index I of a box of level l, per axis, with R the product of the ratios between l
// and L.  Which of the four cases a tile takes is decided from its box's level, a scalar branch:
//   same      G = I; grid[G - lo] with its bits kept if G lies in the region, else fill;
//   finer, constant   G = floor_div(I, R), then as above;
//   finer, linear     p = I - G R, c = 2 p + 1 - R, t = f64(|c|) / f64(2 R), the neighbour N = G - 1
//             for c < 0 and G + 1 otherwise, wrapped into the region (periodic) or replaced by G
//             (clamped) where it leaves it; fill if G is outside the region on any axis, else the
//             eight values combined along x, then y, then z, each step a + t * (b - a);
//   coarser   s = +0.0 and, for kk, then jj, then ii ascending over the part of [I R, (I + 1) R)
//             inside the region, s = s + grid[...]; s / f64(n) with n > 0 cells, else fill.
// The totals count the cells that got fill (outside) and the coarser cells with 0 < n < R^3
// (partial): summed per workgroup, then one 64-bit atomic add per non-zero counter.
//
// Every load lies inside the region (indices are clipped, wrapped or clamped into it before they
// address the grid; nx * ny * nz < 2^31 keeps the 32-bit element offset exact), every store inside
// a box's dims (the host's span rule keeps its 32-bit element offset in bounds).  Every cell is
// written once by one lane, from values only that lane read.  Arithmetic is IEEE binary64, round to
// nearest, nothing fused (-ffp-contract=off), denormals kept; / is the correctly rounded
// __ddiv_rn.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "avr_cell_tiles.h"
#include "avr_internal.h"
#include "avr_level_cells.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTilesPerGroup = 16;  // tiles (2048 cells each) per workgroup

typedef double __attribute__((address_space(1))) global_double;
typedef const double __attribute__((address_space(1))) const_global_double;
typedef const GridBoxDev __attribute__((address_space(4))) constant_box;
typedef const GridLevelsDev __attribute__((address_space(4))) constant_levels;
typedef const uint32_t __attribute__((address_space(4))) constant_u32;
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef double2_t __attribute__((address_space(1))) global_double2;

enum GridCase : int { kSame = 0, kFinerConstant = 1, kFinerLinear = 2, kCoarser = 3 };

// What one axis of a cell needs of the grid.  Offsets are relative to the region's first index and
// lie in [0, dim); which members a case uses is its own, the others are never formed.
struct AxisCell {
  bool inside;      // same, finer: G lies in the region
  uint32_t g, n;    // same, finer: G - lo; linear: the neighbour's offset too
  double t;         // linear: the weight of the neighbour
  uint32_t first, count;  // coarser: the clipped footprint [first, first + count)
  bool full;        // coarser: the whole footprint lies in the region
};

// index: the cell's index at its box's level; r: R; lo, dim: the region along this axis.
template <int CASE>
__device__ __forceinline__ AxisCell axis_cell(long long index, long long r, double two_r,
                                              long long lo, long long dim, bool periodic) {
  AxisCell c = {};
  if (CASE == kCoarser) {
    // |index| <= 2^30 and r <= 2^32: inside 64 bits
    const long long begin = index * r, end = begin + r;
    const long long first = begin > lo ? begin : lo;
    const long long last = end < lo + dim ? end : lo + dim;
    c.count = last > first ? static_cast<uint32_t>(last - first) : 0u;
    c.first = last > first ? static_cast<uint32_t>(first - lo) : 0u;
    c.full = static_cast<long long>(c.count) == r;
    return c;
  }
  const long long g = CASE == kSame ? index : floor_div(index, r);
  c.inside = g >= lo && g < lo + dim;
  c.g = c.inside ? static_cast<uint32_t>(g - lo) : 0u;
  if (CASE == kFinerLinear) {
    const long long p = index - g * r;
    const long long centre = 2 * p + 1 - r;  // |centre| < 2^31
    const long long size = centre < 0 ? -centre : centre;
    c.t = __ddiv_rn(static_cast<double>(size), two_r);
    long long n = centre < 0 ? g - 1 : g + 1;
    if (n < lo) n = periodic ? lo + dim - 1 : g;
    if (n >= lo + dim) n = periodic ? lo : g;
    c.n = c.inside ? static_cast<uint32_t>(n - lo) : 0u;
  }
  return c;
}

// The value of one cell.  nx, ny: the region's dims along x and y.
template <int CASE>
__device__ __forceinline__ double cell_value(const_global_double* grid, uint32_t nx, uint32_t ny,
                                             double fill, const AxisCell& x, const AxisCell& y,
                                             const AxisCell& z, uint32_t* outside,
                                             uint32_t* partial) {
  if (CASE == kCoarser) {
    if (x.count == 0u || y.count == 0u || z.count == 0u) {
      *outside += 1u;
      return fill;
    }
    double s = 0.0;
    for (uint32_t kk = z.first; kk < z.first + z.count; ++kk) {
      for (uint32_t jj = y.first; jj < y.first + y.count; ++jj) {
        const_global_double* row = grid + (kk * ny + jj) * nx;
        for (uint32_t ii = x.first; ii < x.first + x.count; ++ii) s = s + row[ii];
      }
    }
    if (!(x.full && y.full && z.full)) *partial += 1u;
    // the clipped footprint lies inside the region: fewer than 2^31 cells
    return __ddiv_rn(s, static_cast<double>(x.count * y.count * z.count));
  }
  if (!(x.inside && y.inside && z.inside)) {
    *outside += 1u;
    return fill;
  }
  if (CASE != kFinerLinear) return grid[(z.g * ny + y.g) * nx + x.g];
  const uint32_t row00 = (z.g * ny + y.g) * nx, row01 = (z.g * ny + y.n) * nx;
  const uint32_t row10 = (z.n * ny + y.g) * nx, row11 = (z.n * ny + y.n) * nx;
  const double a00 = grid[row00 + x.g], b00 = grid[row00 + x.n];
  const double a01 = grid[row01 + x.g], b01 = grid[row01 + x.n];
  const double a10 = grid[row10 + x.g], b10 = grid[row10 + x.n];
  const double a11 = grid[row11 + x.g], b11 = grid[row11 + x.n];
  const double x00 = a00 + x.t * (b00 - a00);
  const double x01 = a01 + x.t * (b01 - a01);
  const double x10 = a10 + x.t * (b10 - a10);
  const double x11 = a11 + x.t * (b11 - a11);
  const double y0 = x00 + y.t * (x01 - x00);
  const double y1 = x10 + y.t * (x11 - x10);
  return y0 + z.t * (y1 - y0);
}

// One tile with N cells per lane and pass: N == 2 needs the output 16-byte aligned with even
// strides (box.paired).
template <int CASE, int N>
__device__ __forceinline__ void grid_tile(const GridFieldArgs& a, constant_box* box,
                                          const CellTile& at, long long r, double two_r,
                                          uint32_t* outside, uint32_t* partial) {
  // the box's descriptor, once per tile and through the constant address space: scalar loads
  const int nx = box->nx, ny = box->ny, nz = box->nz;
  const long long box_x = box->lo[0], box_y = box->lo[1], box_z = box->lo[2];
  global_double* out = (global_double*)box->out;
  const uint32_t jo = static_cast<uint32_t>(box->jstride), ko = static_cast<uint32_t>(box->kstride);
  const_global_double* grid = (const_global_double*)a.grid;
  const uint32_t gnx = static_cast<uint32_t>(a.nx), gny = static_cast<uint32_t>(a.ny);
  const bool periodic = a.periodic != 0;
  constexpr int kLanesPerRow = kClassifyChunk / N;      // 64 or 128
  constexpr int kRowsPerPass = kThreads / kLanesPerRow;  // 4 or 2
  constexpr int kPasses = 16 / kRowsPerPass;             // 4 or 8
  const int t = static_cast<int>(threadIdx.x);
  const int i = at.chunk * kClassifyChunk + (t % kLanesPerRow) * N;
  if (i >= nx) return;  // no cell of this tile is the lane's; it goes on to the next tile
  const bool whole = i + N - 1 < nx;
  const AxisCell x0 = axis_cell<CASE>(box_x + i, r, two_r, a.lo[0], a.nx, periodic);
  const AxisCell x1 = axis_cell<CASE>(box_x + i + 1, r, two_r, a.lo[0], a.nx, periodic);
  for (int pass = 0; pass < kPasses; ++pass) {
    const int row = pass * kRowsPerPass + t / kLanesPerRow;
    const int j = at.bj * kBrickY + (row & 3), k = at.bk * kBrickZ + (row >> 2);
    if (j >= ny || k >= nz) continue;
    const AxisCell y = axis_cell<CASE>(box_y + j, r, two_r, a.lo[1], a.ny, periodic);
    const AxisCell z = axis_cell<CASE>(box_z + k, r, two_r, a.lo[2], a.nz, periodic);
    const uint32_t to = static_cast<uint32_t>(i) + static_cast<uint32_t>(j) * jo +
                        static_cast<uint32_t>(k) * ko;
    const double v0 = cell_value<CASE>(grid, gnx, gny, a.fill, x0, y, z, outside, partial);
    if (N == 2 && whole) {
      const double v1 = cell_value<CASE>(grid, gnx, gny, a.fill, x1, y, z, outside, partial);
      const double2_t pair = {v0, v1};
      *(global_double2*)(out + to) = pair;
    } else {
      out[to] = v0;
    }
  }
}

template <int CASE>
__device__ __forceinline__ void grid_tile_of(const GridFieldArgs& a, constant_box* box,
                                             const CellTile& at, long long r, double two_r,
                                             uint32_t* outside, uint32_t* partial) {
  if (box->paired) {
    grid_tile<CASE, 2>(a, box, at, r, two_r, outside, partial);
  } else {
    grid_tile<CASE, 1>(a, box, at, r, two_r, outside, partial);
  }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int mask = 32; mask > 0; mask >>= 1) v += __shfl_xor(v, mask, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void grid_field_kernel(const GridFieldArgs a) {
  __shared__ uint32_t wave_totals[kThreads / 64][2];
  constant_box* boxes = (constant_box*)a.boxes;
  constant_u32* tile_begin = (constant_u32*)a.tile_begin;
  constant_levels* levels = (constant_levels*)a.levels;
  const uint32_t first = blockIdx.x * kTilesPerGroup;
  const uint32_t last = (first + kTilesPerGroup < a.n_tiles) ? first + kTilesPerGroup : a.n_tiles;
  uint32_t outside = 0, partial = 0;  // a workgroup holds at most 32768 cells
  // the workgroup's tiles are consecutive: one search (scalar loads) for the first, then a walk
  // along the boxes
  int b = locate_box(tile_begin, a.n_boxes, first);
  uint32_t begin = tile_begin[b], end = tile_begin[b + 1];
  for (uint32_t t = first; t < last; ++t) {
    while (t >= end) {  // t < n_tiles = tile_begin[n_boxes]; boxes without tiles are passed over
      ++b;
      begin = end;
      end = tile_begin[b + 1];
    }
    constant_box* box = boxes + b;
    const CellTile at = cell_tile_of(box->nx, box->ny, t - begin);
    // the case is the box's level's: uniform, read with scalar loads
    const int level = box->level;
    const int direction = levels->direction[level];
    const long long r = levels->refine[level];
    const double two_r = levels->two_r[level];
    if (direction == kGridSame) {
      grid_tile_of<kSame>(a, box, at, r, two_r, &outside, &partial);
    } else if (direction == kGridCoarser) {
      grid_tile_of<kCoarser>(a, box, at, r, two_r, &outside, &partial);
    } else if (a.interpolation != 0) {
      grid_tile_of<kFinerLinear>(a, box, at, r, two_r, &outside, &partial);
    } else {
      grid_tile_of<kFinerConstant>(a, box, at, r, two_r, &outside, &partial);
    }
  }
  const int tid = static_cast<int>(threadIdx.x);
  outside = wave_sum(outside);
  partial = wave_sum(partial);
  if ((tid & 63) == 0) {
    wave_totals[tid >> 6][0] = outside;
    wave_totals[tid >> 6][1] = partial;
  }
  __syncthreads();
  if (tid < 2) {
    uint32_t total = 0;
    for (int w = 0; w < kThreads / 64; ++w) total += wave_totals[w][tid];
    if (total != 0u) atomicAdd(&a.totals[tid], static_cast<unsigned long long>(total));
  }
}

}  // namespace

int launch_grid_field(const GridFieldArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_tiles == 0) return AVR_OK;
  const uint32_t groups = (args.n_tiles + kTilesPerGroup - 1) / kTilesPerGroup;
  hipLaunchKernelGGL(grid_field_kernel, dim3(groups), dim3(kThreads), 0, stream, args);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string("grid_field_kernel: ") + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

}  // namespace avr
