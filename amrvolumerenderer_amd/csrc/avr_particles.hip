// Particle fields ("Particle fields"): particles given as points and values deposited
// onto the cells of a scene's boxes, nearest grid point or cloud in cell, as a sum or a density.
//
//   particle_cells_kernel<M>   one lane per particle: its leaf, its one (ngp) or eight (cic)
//                              contributions (cell ordinal, share), its level
//   particle_clear_kernel      +0.0 to every cell of the output's boxes, in avr_cell_tiles.h tiles
//   particle_sum_kernel<Q>     one lane per sorted contribution: the head of a run of equal cells
//                              adds the run in list order and stores the cell once
//
// Between the first kernel and the other two the caller sorts the contributions by cell, stably
// (plumbing: torch.sort in runtime.py), so that a cell's shares stand in list order.  There is no
// floating-point atomic anywhere: equal arguments give equal bits.
//
// The leaf of a particle is found as streamlines_kernel finds the leaf of a point: levels from the
// finest, q = (P - prob_lo) / dx_l, the finiteness and [-2^30, 2^30) rule, the host's locator (a
// uniform grid of blocks over the level-0 index bounding box, per block the boxes that meet it,
// finest level first).  The eight corners of a cloud follow the same-or-coarser rule through the
// same lists; a corner inside the leaf's own box needs no list.  The box table, the cell prefix, the
// level table and the block lists are read through the constant address space.  Every loop is
// bounded by a count known at launch: the levels, a block's list, the eight corners, the boxes
// (binary search), the contributions.  The totals are counted per lane, summed per wave and
// workgroup and added with one 64-bit integer atomic per non-zero counter.
//
// Stores: cells and shares at p C + c with p < n and c < C; a level at p; +0.0 and a sum at i + j
// jstride + k kstride of a box with (i, j, k) inside its dims -- an ordinal that names no cell is
// skipped.  Arithmetic is IEEE binary64, round to nearest, nothing fused (-ffp-contract=off),
// denormals kept; / is the correctly rounded __ddiv_rn.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "avr_cell_tiles.h"
#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTilesPerGroup = 16;       // tiles (2048 cells each) per workgroup of the clear
constexpr double kIndexLimit = 1073741824.0;  // 2^30

typedef double __attribute__((address_space(1))) global_double;
typedef const double __attribute__((address_space(1))) const_global_double;
typedef long long __attribute__((address_space(1))) global_i64;
typedef const long long __attribute__((address_space(1))) const_global_i64;
typedef const ParticleBoxDev __attribute__((address_space(4))) constant_particle_box;
typedef const GridBoxDev __attribute__((address_space(4))) constant_box;
typedef const IsoLevelsDev __attribute__((address_space(4))) constant_levels;
typedef const ParticleLevelsDev __attribute__((address_space(4))) constant_volumes;
typedef const uint32_t __attribute__((address_space(4))) constant_u32;
typedef const int32_t __attribute__((address_space(4))) constant_i32;
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef long long long2_t __attribute__((ext_vector_type(2)));
typedef double2_t __attribute__((address_space(1))) global_double2;
typedef long2_t __attribute__((address_space(1))) global_long2;

__device__ __forceinline__ int floor_div(int a, int r) {
  const int q = a / r;
  return (a % r != 0 && a < 0) ? q - 1 : q;
}

// A cell of a box: the box's number (< 0: none) and the cell's place in it.
struct Cell {
  int box;
  uint32_t i, j, k;
};

// What the lookups read, each through the constant address space.
struct Tables {
  constant_particle_box* boxes;
  constant_u32* cell_begin;
  constant_u32* block_begin;
  constant_i32* block_boxes;
  constant_levels* levels;
};

// Whether the box holds the index (gx, gy, gz) of its own level; the unsigned difference also
// refuses an index below the box's first (|index| <= 2^30 + 1 and n < 2^28).
__device__ __forceinline__ bool box_holds(constant_particle_box* box, int gx, int gy, int gz,
                                          Cell* cell) {
  const uint32_t i = static_cast<uint32_t>(gx) - static_cast<uint32_t>(box->lo[0]);
  const uint32_t j = static_cast<uint32_t>(gy) - static_cast<uint32_t>(box->lo[1]);
  const uint32_t k = static_cast<uint32_t>(gz) - static_cast<uint32_t>(box->lo[2]);
  cell->i = i;
  cell->j = j;
  cell->k = k;
  return i < static_cast<uint32_t>(box->nx) && j < static_cast<uint32_t>(box->ny) &&
         k < static_cast<uint32_t>(box->nz);
}

// The cell that holds the level-`level` index (gx, gy, gz): of the boxes of level `level` (only
// that level if exact), then level - 1, ..., 0, the first that contains the index mapped to its
// level by floor division -- streamlines_kernel's find_cell over this kernel's tables.
__device__ __forceinline__ Cell find_cell(const Tables& t, const StreamLocatorDev& locator,
                                          int level, int gx, int gy, int gz, bool exact) {
  Cell cell;
  cell.box = -1;
  cell.i = cell.j = cell.k = 0;
  int zx = gx, zy = gy, zz = gz;
  for (int m = level; m > 0; --m) {
    const int r = t.levels->ratio[m - 1];
    zx = floor_div(zx, r);
    zy = floor_div(zy, r);
    zz = floor_div(zz, r);
  }
  if (zx < locator.origin[0] || zy < locator.origin[1] || zz < locator.origin[2]) return cell;
  const uint32_t bx = (static_cast<uint32_t>(zx) - static_cast<uint32_t>(locator.origin[0])) >> locator.shift;
  const uint32_t by = (static_cast<uint32_t>(zy) - static_cast<uint32_t>(locator.origin[1])) >> locator.shift;
  const uint32_t bz = (static_cast<uint32_t>(zz) - static_cast<uint32_t>(locator.origin[2])) >> locator.shift;
  const uint32_t n0 = static_cast<uint32_t>(locator.n[0]), n1 = static_cast<uint32_t>(locator.n[1]);
  if (bx >= n0 || by >= n1 || bz >= static_cast<uint32_t>(locator.n[2])) return cell;
  const uint32_t block = (bz * n1 + by) * n0 + bx;
  const uint32_t first = t.block_begin[block], last = t.block_begin[block + 1];
  int at = level;  // the level (gx, gy, gz) is mapped to so far
  for (uint32_t e = first; e < last; ++e) {
    const int b = t.block_boxes[e];
    constant_particle_box* box = t.boxes + b;
    const int m = box->level;
    if (m > level) continue;
    if (exact && m < level) break;
    while (at > m) {
      const int r = t.levels->ratio[at - 1];
      gx = floor_div(gx, r);
      gy = floor_div(gy, r);
      gz = floor_div(gz, r);
      --at;
    }
    if (box_holds(box, gx, gy, gz, &cell)) {
      cell.box = b;
      return cell;
    }
  }
  return cell;
}

// cell_begin of the cell's box + (k ny + j) nx + i: below 2^31.
__device__ __forceinline__ long long ordinal_of(const Tables& t, const Cell& cell) {
  constant_particle_box* box = t.boxes + cell.box;
  const uint32_t nx = static_cast<uint32_t>(box->nx), ny = static_cast<uint32_t>(box->ny);
  return static_cast<long long>(t.cell_begin[cell.box] + (cell.k * ny + cell.j) * nx + cell.i);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int mask = 32; mask > 0; mask >>= 1) v += __shfl_xor(v, mask, 64);
  return v;
}

// v[0] and v[1] of every wave's lanes summed over the workgroup and added to totals[0], totals[1].
__device__ __forceinline__ void add_totals(uint32_t v0, uint32_t v1, unsigned long long* totals) {
  __shared__ uint32_t wave_totals[kThreads / 64][2];
  const int tid = static_cast<int>(threadIdx.x);
  v0 = wave_sum(v0);
  v1 = wave_sum(v1);
  if ((tid & 63) == 0) {
    wave_totals[tid >> 6][0] = v0;
    wave_totals[tid >> 6][1] = v1;
  }
  __syncthreads();
  if (tid < 2) {
    uint32_t total = 0;
    for (int w = 0; w < kThreads / 64; ++w) total += wave_totals[w][tid];
    if (total != 0u) atomicAdd(&totals[tid], static_cast<unsigned long long>(total));
  }
}

template <int METHOD>
__global__ __launch_bounds__(kThreads) void particle_cells_kernel(const ParticleCellsArgs a) {
  constexpr int kEntries = METHOD == kParticleCic ? 8 : 1;
  Tables t;
  t.boxes = (constant_particle_box*)a.boxes;
  t.cell_begin = (constant_u32*)a.cell_begin;
  t.block_begin = (constant_u32*)a.block_begin;
  t.block_boxes = (constant_i32*)a.block_boxes;
  t.levels = (constant_levels*)a.levels;
  const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
  uint32_t outside = 0, rerouted = 0;  // a workgroup holds 256 particles, 2048 corners
  if (p < a.n) {
    const_global_double* points = (const_global_double*)a.points;
    const double point[3] = {points[p * 3ull + 0], points[p * 3ull + 1], points[p * 3ull + 2]};
    const double v = a.values != nullptr ? ((const_global_double*)a.values)[p] : 1.0;
    // the leaf: the finest level first
    double q[3] = {0.0, 0.0, 0.0};
    Cell leaf;
    leaf.box = -1;
    leaf.i = leaf.j = leaf.k = 0;
    bool inside = true;
    int level = a.n_levels - 1;
    for (; level >= 0 && inside; --level) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        q[d] = __ddiv_rn(point[d] - t.levels->prob_lo[d], t.levels->cell_size[level][d]);
        inside = inside && q[d] >= -kIndexLimit && q[d] < kIndexLimit;  // false for a NaN
      }
      if (!inside) break;
      leaf = find_cell(t, a.locator, level, static_cast<int>(floor(q[0])),
                       static_cast<int>(floor(q[1])), static_cast<int>(floor(q[2])), true);
      if (leaf.box >= 0) break;
    }
    const bool found = leaf.box >= 0;
    long long cells[kEntries];
    double shares[kEntries];
    if (!found) {
      outside = 1u;
#pragma unroll
      for (int c = 0; c < kEntries; ++c) {
        cells[c] = kParticleOutside;
        shares[c] = 0.0;
      }
    } else {
      const long long own = ordinal_of(t, leaf);
      if (METHOD == kParticleNgp) {
        cells[0] = own;
        shares[0] = v;
      } else {
        constant_particle_box* home = t.boxes + leaf.box;
        int base[3];
        double w[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const double u = q[d] - 0.5;
          const double low = floor(u);
          base[d] = static_cast<int>(low);
          w[d] = u - low;
        }
#pragma unroll
        for (int c = 0; c < kEntries; ++c) {
          const int di = c & 1, dj = (c >> 1) & 1, dk = c >> 2;
          const double wx = di ? w[0] : 1.0 - w[0];
          const double wy = dj ? w[1] : 1.0 - w[1];
          const double wz = dk ? w[2] : 1.0 - w[2];
          shares[c] = ((wx * wy) * wz) * v;
          const int gx = base[0] + di, gy = base[1] + dj, gz = base[2] + dk;
          Cell corner;
          if (box_holds(home, gx, gy, gz, &corner)) {
            corner.box = leaf.box;
          } else {
            corner = find_cell(t, a.locator, level, gx, gy, gz, false);
          }
          if (corner.box >= 0) {
            cells[c] = ordinal_of(t, corner);
          } else {  // absent: the share stays with the particle's own cell
            cells[c] = own;
            rerouted += 1u;
          }
        }
      }
    }
    global_i64* cells_out = (global_i64*)a.cells + static_cast<unsigned long long>(p) * kEntries;
    global_double* shares_out =
        (global_double*)a.shares + static_cast<unsigned long long>(p) * kEntries;
    if (METHOD == kParticleCic && a.paired != 0) {
#pragma unroll
      for (int c = 0; c < kEntries; c += 2) {
        const long2_t cell_pair = {cells[c], cells[c + 1 < kEntries ? c + 1 : c]};
        const double2_t share_pair = {shares[c], shares[c + 1 < kEntries ? c + 1 : c]};
        *(global_long2*)(cells_out + c) = cell_pair;
        *(global_double2*)(shares_out + c) = share_pair;
      }
    } else {
#pragma unroll
      for (int c = 0; c < kEntries; ++c) {
        cells_out[c] = cells[c];
        shares_out[c] = shares[c];
      }
    }
    if (a.levels_out != nullptr) a.levels_out[p] = found ? static_cast<uint8_t>(level) : 255;
  }
  add_totals(outside, rerouted, a.totals);
}

// One tile of +0.0 with N cells per lane and pass: N == 2 needs the output 16-byte aligned with
// even strides (box.paired).  The rows and passes are grid_field_kernel's.
template <int N>
__device__ __forceinline__ void clear_tile(constant_box* box, const CellTile& at) {
  const int nx = box->nx, ny = box->ny, nz = box->nz;
  global_double* out = (global_double*)box->out;
  const uint32_t jo = static_cast<uint32_t>(box->jstride), ko = static_cast<uint32_t>(box->kstride);
  constexpr int kLanesPerRow = kClassifyChunk / N;      // 64 or 128
  constexpr int kRowsPerPass = kThreads / kLanesPerRow;  // 4 or 2
  constexpr int kPasses = 16 / kRowsPerPass;             // 4 or 8
  const int t = static_cast<int>(threadIdx.x);
  const int i = at.chunk * kClassifyChunk + (t % kLanesPerRow) * N;
  if (i >= nx) return;
  const bool whole = i + N - 1 < nx;
  for (int pass = 0; pass < kPasses; ++pass) {
    const int row = pass * kRowsPerPass + t / kLanesPerRow;
    const int j = at.bj * kBrickY + (row & 3), k = at.bk * kBrickZ + (row >> 2);
    if (j >= ny || k >= nz) continue;
    const uint32_t to = static_cast<uint32_t>(i) + static_cast<uint32_t>(j) * jo +
                        static_cast<uint32_t>(k) * ko;
    if (N == 2 && whole) {
      const double2_t pair = {0.0, 0.0};
      *(global_double2*)(out + to) = pair;
    } else {
      out[to] = 0.0;
    }
  }
}

__global__ __launch_bounds__(kThreads) void particle_clear_kernel(const ParticleDepositArgs a) {
  constant_box* boxes = (constant_box*)a.boxes;
  constant_u32* tile_begin = (constant_u32*)a.tile_begin;
  const uint32_t first = blockIdx.x * kTilesPerGroup;
  const uint32_t last = (first + kTilesPerGroup < a.n_tiles) ? first + kTilesPerGroup : a.n_tiles;
  // the workgroup's tiles are consecutive: one search for the first, then a walk along the boxes
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
    if (box->paired) {
      clear_tile<2>(box, at);
    } else {
      clear_tile<1>(box, at);
    }
  }
}

template <int QUANTITY>
__global__ __launch_bounds__(kThreads) void particle_sum_kernel(const ParticleDepositArgs a) {
  const uint32_t at = blockIdx.x * kThreads + threadIdx.x;
  if (at >= a.n) return;
  const_global_i64* cells = (const_global_i64*)a.cells;
  const_global_double* shares = (const_global_double*)a.shares;
  const long long cell = cells[at];
  if (at != 0u && cells[at - 1u] == cell) return;  // not the head of its run
  // 0xFFFFFFFF, and whatever else names no cell, is skipped
  if (cell < 0 || cell >= static_cast<long long>(a.n_cells)) return;
  double s = 0.0;
  for (uint32_t e = at; e < a.n && cells[e] == cell; ++e) s = s + shares[e];
  constant_u32* cell_begin = (constant_u32*)a.cell_begin;
  const uint32_t ordinal = static_cast<uint32_t>(cell);
  const int b = locate_box(cell_begin, a.n_boxes, ordinal);
  constant_box* box = (constant_box*)a.boxes + b;
  const uint32_t local = ordinal - cell_begin[b];
  const uint32_t nx = static_cast<uint32_t>(box->nx), ny = static_cast<uint32_t>(box->ny);
  const uint32_t i = local % nx, row = local / nx;
  const uint32_t j = row % ny, k = row / ny;
  if (k >= static_cast<uint32_t>(box->nz)) return;  // cannot happen below n_cells; no store if so
  const unsigned long long to = static_cast<unsigned long long>(i) +
                                static_cast<unsigned long long>(j) * static_cast<uint32_t>(box->jstride) +
                                static_cast<unsigned long long>(k) * static_cast<uint32_t>(box->kstride);
  if (QUANTITY == kParticleDensity) {
    s = __ddiv_rn(s, ((constant_volumes*)a.levels)->volume[box->level]);
  }
  ((global_double*)box->out)[to] = s;
}

int launched(const char* kernel) {
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string(kernel) + ": " + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

}  // namespace

int launch_particle_cells(const ParticleCellsArgs& args, int method, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n == 0) return AVR_OK;
  const dim3 grid((args.n + kThreads - 1) / kThreads);
  if (method == kParticleCic) {
    hipLaunchKernelGGL(particle_cells_kernel<kParticleCic>, grid, dim3(kThreads), 0, stream, args);
  } else {
    hipLaunchKernelGGL(particle_cells_kernel<kParticleNgp>, grid, dim3(kThreads), 0, stream, args);
  }
  return launched("particle_cells_kernel");
}

int launch_particle_deposit(const ParticleDepositArgs& args, int quantity, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_tiles == 0) return AVR_OK;  // no cells: nothing to clear, nothing to store to
  const uint32_t groups = (args.n_tiles + kTilesPerGroup - 1) / kTilesPerGroup;
  hipLaunchKernelGGL(particle_clear_kernel, dim3(groups), dim3(kThreads), 0, stream, args);
  const int cleared = launched("particle_clear_kernel");
  if (cleared != AVR_OK || args.n == 0) return cleared;
  const dim3 grid((args.n + kThreads - 1) / kThreads);
  if (quantity == kParticleDensity) {
    hipLaunchKernelGGL(particle_sum_kernel<kParticleDensity>, grid, dim3(kThreads), 0, stream, args);
  } else {
    hipLaunchKernelGGL(particle_sum_kernel<kParticleSum>, grid, dim3(kThreads), 0, stream, args);
  }
  return launched("particle_sum_kernel");
}

}  // namespace avr
