// Streamlines ("Streamlines"): RK4 field lines of a vector field given as three
// congruent scenes, followed through the leaf cells of every level, with the velocity interpolated
// trilinearly between cell centres.
//
//   streamlines_kernel<S>    one lane per seed; S: a sample scene is interpolated at every point
//
// A lane keeps its point, takes up to max_steps steps of four stages each and writes every point
// as it is reached.  A stage finds the leaf of its point through the host's locator (a uniform grid
// of blocks over the scene's level-0 index bounding box, per block the boxes of any level that
// meet it, finest level first), finds the eight cell centres around the point by the isosurfaces'
// same-or-coarser corner rule through the same lists, and gathers three (four with a sample)
// values per corner.  A corner inside the leaf's own box needs no list: boxes of one level do not
// overlap and the corner rule tries the leaf's level first, so that box is the rule's first hit.
// Only cells of the scene's boxes are ever read.
//
// The step loop is one loop of max_steps + 1 trips with the four stages as an inner loop around a
// single copy of the evaluation, so all lanes of a wave are in the same stage; a lane whose line
// has ended idles until its wave's last line ends.  Every loop is bounded by a count known at
// launch: max_steps, the four stages, the levels, a block's list, the eight corners.  No atomics:
// equal arguments give equal bits.  Arithmetic is IEEE binary64, round to nearest, nothing fused
// (-ffp-contract=off); / and sqrt are the correctly rounded __ddiv_rn and __dsqrt_rn.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 64;  // one wave: its slot is free again when its own last line has ended
constexpr double kIndexLimit = 1073741824.0;  // 2^30

__device__ __forceinline__ int floor_div(int a, int r) {
  const int q = a / r;
  return (a % r != 0 && a < 0) ? q - 1 : q;
}

// A cell of a box: the box's number (< 0: none) and the cell's place in it.
struct Cell {
  int box;
  uint32_t i, j, k;
};

// Whether `box` holds the index (gx, gy, gz) of its own level; the unsigned difference also
// refuses an index below the box's first (|index| <= 2^30 + 1 and n < 2^28).
__device__ __forceinline__ bool box_holds(const StreamBoxDev& box, int gx, int gy, int gz,
                                          Cell* cell) {
  const uint32_t i = static_cast<uint32_t>(gx) - static_cast<uint32_t>(box.lo[0]);
  const uint32_t j = static_cast<uint32_t>(gy) - static_cast<uint32_t>(box.lo[1]);
  const uint32_t k = static_cast<uint32_t>(gz) - static_cast<uint32_t>(box.lo[2]);
  cell->i = i;
  cell->j = j;
  cell->k = k;
  return i < static_cast<uint32_t>(box.nx) && j < static_cast<uint32_t>(box.ny) &&
         k < static_cast<uint32_t>(box.nz);
}

// The cell that holds the level-`level` index (gx, gy, gz): of the boxes of level `level` (only
// that level if exact), then level - 1, ..., 0, the first that contains the index mapped to its
// level by floor division.  Every such box is in the list of the block that holds the index mapped
// to level 0, and the list has the finest level first.
__device__ __forceinline__ Cell find_cell(const StreamArgs& a, int level, int gx, int gy, int gz,
                                          bool exact) {
  Cell cell;
  cell.box = -1;
  cell.i = cell.j = cell.k = 0;
  int zx = gx, zy = gy, zz = gz;
  for (int m = level; m > 0; --m) {
    const int r = a.levels->ratio[m - 1];
    zx = floor_div(zx, r);
    zy = floor_div(zy, r);
    zz = floor_div(zz, r);
  }
  const StreamLocatorDev& locator = a.locator;
  if (zx < locator.origin[0] || zy < locator.origin[1] || zz < locator.origin[2]) return cell;
  const uint32_t bx = (static_cast<uint32_t>(zx) - static_cast<uint32_t>(locator.origin[0])) >> locator.shift;
  const uint32_t by = (static_cast<uint32_t>(zy) - static_cast<uint32_t>(locator.origin[1])) >> locator.shift;
  const uint32_t bz = (static_cast<uint32_t>(zz) - static_cast<uint32_t>(locator.origin[2])) >> locator.shift;
  const uint32_t n0 = static_cast<uint32_t>(locator.n[0]), n1 = static_cast<uint32_t>(locator.n[1]);
  if (bx >= n0 || by >= n1 || bz >= static_cast<uint32_t>(locator.n[2])) return cell;
  const uint32_t block = (bz * n1 + by) * n0 + bx;
  const uint32_t first = a.block_begin[block], last = a.block_begin[block + 1];
  int at = level;  // the level (gx, gy, gz) is mapped to so far
  for (uint32_t e = first; e < last; ++e) {
    const int b = a.block_boxes[e];
    const StreamBoxDev& box = a.boxes[b];
    const int m = box.level;
    if (m > level) continue;
    if (exact && m < level) break;
    while (at > m) {
      const int r = a.levels->ratio[at - 1];
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

// Fields 0..2 (and 3 with sample) of one cell.
__device__ __forceinline__ void load_cell(const StreamBoxDev& box, const Cell& cell, bool sample,
                                          double out[4]) {
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    if (f < 3 || sample) {
      out[f] = box.cells[f][cell.i + cell.j * static_cast<uint32_t>(box.jstride[f]) +
                            cell.k * static_cast<uint32_t>(box.kstride[f])];
    }
  }
}

__device__ __forceinline__ double trilinear(const double v[8], const double w[3]) {
  const double a00 = v[0] + w[0] * (v[1] - v[0]);
  const double a10 = v[2] + w[0] * (v[3] - v[2]);
  const double a01 = v[4] + w[0] * (v[5] - v[4]);
  const double a11 = v[6] + w[0] * (v[7] - v[6]);
  const double b0 = a00 + w[1] * (a10 - a00);
  const double b1 = a01 + w[1] * (a11 - a01);
  return b0 + w[2] * (b1 - b0);
}

// What one point evaluates to.
struct Evaluation {
  bool leaf;        // the point has a leaf; nothing else is set without one
  bool finite;      // the velocity is trilinear, or the leaf's own with every component finite
  int level;        // of the leaf
  double v[3];
  double sample;    // when asked for
};

// sample (the same in every lane): the sample field, field 3 of the boxes, is evaluated as well.
__device__ __forceinline__ Evaluation evaluate(const StreamArgs& a, const double p[3], bool sample) {
  Evaluation out;
  out.leaf = false;
  out.finite = false;
  out.level = 0;
  out.v[0] = out.v[1] = out.v[2] = 0.0;
  out.sample = 0.0;
  // the leaf: the finest level first
  double q[3] = {0.0, 0.0, 0.0};
  Cell leaf;
  leaf.box = -1;
  leaf.i = leaf.j = leaf.k = 0;
  int level = a.n_levels - 1;
  for (; level >= 0; --level) {
    bool inside = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      q[d] = __ddiv_rn(p[d] - a.levels->prob_lo[d], a.levels->cell_size[level][d]);
      inside = inside && q[d] >= -kIndexLimit && q[d] < kIndexLimit;  // false for a NaN
    }
    if (!inside) return out;
    leaf = find_cell(a, level, static_cast<int>(floor(q[0])), static_cast<int>(floor(q[1])),
                     static_cast<int>(floor(q[2])), true);
    if (leaf.box >= 0) break;
  }
  if (leaf.box < 0) return out;
  out.leaf = true;
  out.level = level;
  const StreamBoxDev& home = a.boxes[leaf.box];
  // the eight cell centres around the point
  int base[3];
  double w[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double u = q[d] - 0.5;
    const double low = floor(u);
    base[d] = static_cast<int>(low);
    w[d] = u - low;
  }
  double v[4][8];
  bool present = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int gx = base[0] + (c & 1), gy = base[1] + ((c >> 1) & 1), gz = base[2] + (c >> 2);
    Cell corner;
    double values[4] = {0.0, 0.0, 0.0, 0.0};
    if (box_holds(home, gx, gy, gz, &corner)) {
      load_cell(home, corner, sample, values);
    } else {
      corner = find_cell(a, level, gx, gy, gz, false);
      if (corner.box >= 0) {
        load_cell(a.boxes[corner.box], corner, sample, values);
      } else {
        present = false;
      }
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) v[f][c] = values[f];
  }
  bool smooth = present;  // the three components share one decision
#pragma unroll
  for (int f = 0; f < 3; ++f) {
#pragma unroll
    for (int c = 0; c < 8; ++c) smooth = smooth && __builtin_isfinite(v[f][c]);
  }
  bool smooth_sample = present;
#pragma unroll
  for (int c = 0; c < 8; ++c) smooth_sample = smooth_sample && __builtin_isfinite(v[3][c]);
  // the piecewise-constant fallback: the leaf cell's own values
  double own[4] = {0.0, 0.0, 0.0, 0.0};
  if (!smooth || (sample && !smooth_sample)) load_cell(home, leaf, sample, own);
  out.finite = smooth || (__builtin_isfinite(own[0]) && __builtin_isfinite(own[1]) &&
                          __builtin_isfinite(own[2]));
#pragma unroll
  for (int f = 0; f < 3; ++f) out.v[f] = smooth ? trilinear(v[f], w) : own[f];
  if (sample) out.sample = smooth_sample ? trilinear(v[3], w) : own[3];
  return out;
}

template <bool HAS_S>
__global__ __launch_bounds__(kThreads) void streamlines_kernel(const StreamArgs a) {
  const uint32_t seed = blockIdx.x * kThreads + threadIdx.x;
  if (seed >= a.n_seeds) return;
  double p[3] = {a.seeds[seed * 3ull + 0], a.seeds[seed * 3ull + 1], a.seeds[seed * 3ull + 2]};
  const unsigned long long first_slot = static_cast<unsigned long long>(seed) * (a.max_steps + 1ull);
  uint32_t count = 0, status = kStreamMaxStepsReached;
  bool ended = false;
  for (uint32_t n = 0; n <= a.max_steps && !ended; ++n) {
    double k[3] = {0.0, 0.0, 0.0}, sum[3] = {0.0, 0.0, 0.0}, h = 0.0;
#pragma unroll 1
    for (int stage = 0; stage < 4 && !ended; ++stage) {
      const double reach = stage == 3 ? h : 0.5 * h;
      double at[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) at[d] = stage == 0 ? p[d] : p[d] + reach * k[d];
      const Evaluation e = evaluate(a, at, HAS_S && stage == 0);
      if (stage == 0) {
        if (n == 0 && !e.leaf) {  // the seed is outside: no point
          status = kStreamOutside;
          ended = true;
          break;
        }
        const unsigned long long slot = first_slot + n;
        a.points[slot * 3ull + 0] = p[0];
        a.points[slot * 3ull + 1] = p[1];
        a.points[slot * 3ull + 2] = p[2];
        if (HAS_S) a.samples[slot] = e.leaf ? e.sample : __builtin_nan("");
        count = n + 1u;
        if (n == a.max_steps) {
          ended = true;
          break;
        }
      }
      if (!e.leaf || !e.finite) {
        status = !e.leaf ? kStreamOutside : kStreamNonFinite;
        ended = true;
        break;
      }
      const double norm = __dsqrt_rn((e.v[0] * e.v[0] + e.v[1] * e.v[1]) + e.v[2] * e.v[2]);
      if (norm == 0.0) {
        status = kStreamStagnant;
        ended = true;
        break;
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) k[d] = __ddiv_rn(a.direction * e.v[d], norm);
      if (stage == 0) {
        const double* dx = a.levels->cell_size[e.level];
        const double least = fmin(fmin(dx[0], dx[1]), dx[2]);
        h = a.step * least;
#pragma unroll
        for (int d = 0; d < 3; ++d) sum[d] = k[d];
      } else {
#pragma unroll
        for (int d = 0; d < 3; ++d) sum[d] = sum[d] + (stage == 3 ? k[d] : 2.0 * k[d]);
      }
    }
    if (ended) break;
    const double sixth = __ddiv_rn(h, 6.0);
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] = p[d] + sixth * sum[d];
  }
  a.counts[seed] = count;
  a.status[seed] = static_cast<uint8_t>(status);
}

}  // namespace

int launch_streamlines(const StreamArgs& args, bool has_sample, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_seeds == 0) return AVR_OK;
  const dim3 grid((args.n_seeds + kThreads - 1) / kThreads);
  if (has_sample) {
    hipLaunchKernelGGL(streamlines_kernel<true>, grid, dim3(kThreads), 0, stream, args);
  } else {
    hipLaunchKernelGGL(streamlines_kernel<false>, grid, dim3(kThreads), 0, stream, args);
  }
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string("streamlines kernel: ") + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

}  // namespace avr
