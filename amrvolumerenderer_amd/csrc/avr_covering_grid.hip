// Covering grids ("Covering grid"): a field resampled to the cells of one level L
// over a region of that level's index space -- the value of the leaf where the data is of the same
// or a coarser level, the volume-weighted mean of the leaves where it is finer.
//
//   covering_grid_kernel     one workgroup per output tile, one lane per output cell
//
// The output is cut into the tiles of avr_cell_tiles.h: 128 cells along x by 4 rows by 4 planes.
// A workgroup of 256 lanes takes one tile in 8 passes of two rows, so that every store of a wave
// is 64 consecutive cells along x.  The tile's candidate list (the boxes whose cells hold a cell of
// the tile, an ancestor or a descendant of one; made by the host) is the same for every lane of
// the workgroup: its bounds come from the tile's number alone.
//
// A cell G of level L:
//   1. find_same_or_coarser (avr_level_cells.h) over the tile's candidates: a hit gives the cell's
//      stored double, bits kept, coverage 1.0 and the hit's level;
//   2. else, for every loaded level m > L in ascending order, the leaves of level m inside the
//      cell's footprint [G R_m, (G + 1) R_m) are added in ascending k, then j, then i; the level
//      contributes w_m * sum to the numerator and w_m * count to the denominator, and the value is
//      their quotient, the coverage the denominator;
//   3. else the cell is absent: the fill value (bits kept), coverage 0.0, level -1.
// In rule 2 the footprint is first held against the candidates of level m.  If one box alone meets
// it -- the common case: the footprint lies inside a box -- the cells of the overlap are read with
// plain strided loads in k, j, i order.  Only when several boxes meet it is every fine cell of
// their common hull looked up among them.  Boxes of one level lie apart, so both ways add the same
// cells in the same order: the bits agree.
//
// Every load lies inside a box's dims (the overlap is clipped to the box; the host's span rule
// keeps the 32-bit element offset in bounds), every store inside nx * ny * nz < 2^31 cells.  Every
// cell is written once by one lane, from values only that lane read: no atomics, equal arguments
// give equal bits.  Arithmetic is IEEE binary64, round to nearest, nothing fused
// (-ffp-contract=off), denormals kept; / is the correctly rounded __ddiv_rn.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "avr_cell_tiles.h"
#include "avr_internal.h"
#include "avr_level_cells.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerPass = kThreads / kClassifyChunk;           // 2
constexpr int kPasses = kBrickY * kBrickZ / kRowsPerPass;         // 8
static_assert(kThreads % kClassifyChunk == 0 && kBrickY == 4 && kBrickZ == 4,
              "a pass is whole rows of a 4 x 4 brick");

// [lo, hi) per axis, in some level's index space
struct Span3 {
  long long lo[3], hi[3];
};

// the part of `footprint` that box holds; false if it holds none of it
__device__ __forceinline__ bool overlap(const CoverBoxDev& box, const Span3& footprint, Span3* out) {
  const int n[3] = {box.nx, box.ny, box.nz};
  bool meets = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const long long lo = box.lo[d], hi = lo + n[d];
    out->lo[d] = footprint.lo[d] > lo ? footprint.lo[d] : lo;
    out->hi[d] = footprint.hi[d] < hi ? footprint.hi[d] : hi;
    meets = meets && out->lo[d] < out->hi[d];
  }
  return meets;
}

__device__ __forceinline__ bool box_holds(const CoverBoxDev& box, long long x, long long y,
                                          long long z) {
  return x >= box.lo[0] && x < static_cast<long long>(box.lo[0]) + box.nx &&
         y >= box.lo[1] && y < static_cast<long long>(box.lo[1]) + box.ny &&
         z >= box.lo[2] && z < static_cast<long long>(box.lo[2]) + box.nz;
}

// the cell at index (x, y, z) of a box that holds it
__device__ __forceinline__ double box_cell(const CoverBoxDev& box, long long x, long long y,
                                           long long z) {
  const uint32_t i = static_cast<uint32_t>(x - box.lo[0]);
  const uint32_t j = static_cast<uint32_t>(y - box.lo[1]);
  const uint32_t k = static_cast<uint32_t>(z - box.lo[2]);
  return box.cells[i + j * static_cast<uint32_t>(box.jstride) +
                   k * static_cast<uint32_t>(box.kstride)];
}

// The leaves of level m inside `footprint`, added in ascending k, then j, then i: their sum from
// +0.0 and their number.
__device__ __forceinline__ void add_level(const CoverArgs& a, uint32_t first, uint32_t last, int m,
                                          const Span3& footprint, double* sum, long long* count) {
  // the candidates of level m that meet the footprint: how many, the last one, their hull
  int meeting = 0;
  uint32_t only = first;
  Span3 hull = {};
  for (uint32_t q = first; q < last; ++q) {
    const CoverBoxDev& box = a.boxes[a.candidates[q]];
    if (box.level != m) continue;
    Span3 part;
    if (!overlap(box, footprint, &part)) continue;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      hull.lo[d] = (meeting == 0 || part.lo[d] < hull.lo[d]) ? part.lo[d] : hull.lo[d];
      hull.hi[d] = (meeting == 0 || part.hi[d] > hull.hi[d]) ? part.hi[d] : hull.hi[d];
    }
    ++meeting;
    only = q;
  }
  double s = 0.0;
  long long n = 0;
  if (meeting == 1) {
    // one box: the hull is the overlap, every cell of it a leaf
    const CoverBoxDev& box = a.boxes[a.candidates[only]];
    const uint32_t js = static_cast<uint32_t>(box.jstride), ks = static_cast<uint32_t>(box.kstride);
    const uint32_t i0 = static_cast<uint32_t>(hull.lo[0] - box.lo[0]);
    const uint32_t i1 = static_cast<uint32_t>(hull.hi[0] - box.lo[0]);
    const uint32_t j0 = static_cast<uint32_t>(hull.lo[1] - box.lo[1]);
    const uint32_t j1 = static_cast<uint32_t>(hull.hi[1] - box.lo[1]);
    const uint32_t k0 = static_cast<uint32_t>(hull.lo[2] - box.lo[2]);
    const uint32_t k1 = static_cast<uint32_t>(hull.hi[2] - box.lo[2]);
    for (uint32_t k = k0; k < k1; ++k) {
      for (uint32_t j = j0; j < j1; ++j) {
        const double* row = box.cells + (j * js + k * ks);
        for (uint32_t i = i0; i < i1; ++i) s = s + row[i];
      }
    }
    n = static_cast<long long>(i1 - i0) * (j1 - j0) * (k1 - k0);  // at most the box's cells
  } else if (meeting > 1) {
    uint32_t hit = only;  // the candidate that held the cell before
    for (long long z = hull.lo[2]; z < hull.hi[2]; ++z) {
      for (long long y = hull.lo[1]; y < hull.hi[1]; ++y) {
        for (long long x = hull.lo[0]; x < hull.hi[0]; ++x) {
          const CoverBoxDev* holder = &a.boxes[a.candidates[hit]];
          if (holder->level != m || !box_holds(*holder, x, y, z)) {
            holder = nullptr;
            for (uint32_t q = first; q < last; ++q) {
              const CoverBoxDev& other = a.boxes[a.candidates[q]];
              if (other.level == m && box_holds(other, x, y, z)) {
                holder = &other;
                hit = q;
                break;
              }
            }
          }
          if (holder == nullptr) continue;
          s = s + box_cell(*holder, x, y, z);
          ++n;
        }
      }
    }
  }
  *sum = s;
  *count = n;
}

__global__ __launch_bounds__(kThreads) void covering_grid_kernel(const CoverArgs a) {
  const uint32_t tile = blockIdx.x;
  const CellTile at = cell_tile_of(a.nx, a.ny, tile);
  const uint32_t first = a.candidate_begin[tile], last = a.candidate_begin[tile + 1];
  const int t = static_cast<int>(threadIdx.x);
  const int i = at.chunk * kClassifyChunk + t % kClassifyChunk;
  if (i >= a.nx) return;
  const long long gx = static_cast<long long>(a.lo[0]) + i;
  for (int pass = 0; pass < kPasses; ++pass) {
    const int row = pass * kRowsPerPass + t / kClassifyChunk;
    const int j = at.bj * kBrickY + (row & 3), k = at.bk * kBrickZ + (row >> 2);
    if (j >= a.ny || k >= a.nz) continue;
    const long long gy = static_cast<long long>(a.lo[1]) + j;
    const long long gz = static_cast<long long>(a.lo[2]) + k;
    double value = a.fill, coverage = 0.0;
    int level = -1;
    const LevelCell found = find_same_or_coarser(a.boxes, a.candidates, first, last,
                                                 a.levels->ratio, a.level, gx, gy, gz);
    if (found.box >= 0) {
      const CoverBoxDev& box = a.boxes[found.box];
      value = box.cells[found.i + found.j * static_cast<uint32_t>(box.jstride) +
                        found.k * static_cast<uint32_t>(box.kstride)];
      coverage = 1.0;
      level = found.level;
    } else if (first < last) {
      double num = 0.0, den = 0.0;
      for (int m = a.level + 1; m <= a.finest; ++m) {
        const long long r = a.levels->refine[m];  // <= 2^30 and |G| <= 2^30: inside 64 bits
        Span3 footprint;
        footprint.lo[0] = gx * r;
        footprint.lo[1] = gy * r;
        footprint.lo[2] = gz * r;
#pragma unroll
        for (int d = 0; d < 3; ++d) footprint.hi[d] = footprint.lo[d] + r;
        double s;
        long long n;
        add_level(a, first, last, m, footprint, &s, &n);
        if (n > 0) {
          const double w = a.levels->weight[m];
          num = num + w * s;
          den = den + w * static_cast<double>(n);
          level = m;
        }
      }
      if (den > 0.0) {
        value = __ddiv_rn(num, den);
        coverage = den;
      }
    }
    const size_t cell = (static_cast<size_t>(k) * static_cast<size_t>(a.ny) +
                         static_cast<size_t>(j)) * static_cast<size_t>(a.nx) +
                        static_cast<size_t>(i);
    a.values[cell] = value;
    if (a.coverage != nullptr) a.coverage[cell] = coverage;
    if (a.cell_level != nullptr) a.cell_level[cell] = static_cast<int8_t>(level);
  }
}

}  // namespace

int launch_covering_grid(const CoverArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_tiles == 0) return AVR_OK;
  hipLaunchKernelGGL(covering_grid_kernel, dim3(args.n_tiles), dim3(kThreads), 0, stream, args);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string("covering_grid_kernel: ") + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

}  // namespace avr
