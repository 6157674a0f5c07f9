// Which cell of an AMR hierarchy holds an index ("The same-or-coarser rule"): the
// index of some level is mapped down by floor division through the ratios, and of the boxes of the
// same or a coarser level that hold it there, the one of the highest level wins.  Plain integer
// code without HIP, one definition for the host and the device: the gradient's halo and the
// isosurfaces' shell call it in their kernels, and tests/cxx/level_cells_test.cpp holds it against
// a scan of all boxes on the CPU.  (The clumps' unite_ghost keeps the loop written out, with the
// use of the hit inside it: clump_merge_kernel is bound by dependent loads, and its device code is
// kept byte for byte.)
#ifndef AVR_LEVEL_CELLS_H
#define AVR_LEVEL_CELLS_H

#include <cstdint>

#ifndef AVR_HD  // avr_internal.h's, for a file that includes this header alone
#if defined(__HIP__)
#define AVR_HD __host__ __device__
#else
#define AVR_HD
#endif
#endif

namespace avr {

// The levels a field product takes: n_levels lies in [1, 16].
constexpr int kFieldMaxLevels = 16;

// floor(a / r) for r > 0
AVR_HD inline __attribute__((always_inline)) int64_t floor_div(int64_t a, int64_t r) {
  const int64_t q = a / r;
  return (a % r != 0 && a < 0) ? q - 1 : q;
}

// A cell of a box: the box's number (< 0: none), the box's level and the cell's place in the box.
struct LevelCell {
  int box, level;
  uint32_t i, j, k;
};

// The cell that holds the level-`level` index (gx, gy, gz).  Only the boxes candidates[first, last)
// are tested, whatever their order: one of a finer level, or of a level no higher than that of a
// hit before it, is passed over; for any other the index is mapped to its level by floor division
// (ratio[l]: level l -> l + 1).  Boxes of one level do not overlap, so the hit is the only one of
// its level.  Box: any record with nx, ny, nz (0 for a box without cells), level and lo[3].
template <class Box>
AVR_HD inline __attribute__((always_inline)) LevelCell find_same_or_coarser(
    const Box* boxes, const int32_t* candidates, uint32_t first, uint32_t last,
    const int32_t* ratio, int level, long long gx, long long gy, long long gz) {
  LevelCell cell;
  cell.box = -1;
  cell.level = -1;
  cell.i = cell.j = cell.k = 0;
  for (uint32_t q = first; q < last; ++q) {
    const int c = candidates[q];
    const Box& other = boxes[c];
    if (other.level > level || other.level <= cell.level) continue;
    long long ox = gx, oy = gy, oz = gz;
    for (int m = level; m > other.level; --m) {
      const long long r = ratio[m - 1];
      ox = floor_div(ox, r);
      oy = floor_div(oy, r);
      oz = floor_div(oz, r);
    }
    ox -= other.lo[0];
    oy -= other.lo[1];
    oz -= other.lo[2];
    if (ox >= 0 && ox < other.nx && oy >= 0 && oy < other.ny && oz >= 0 && oz < other.nz) {
      cell.box = c;
      cell.level = other.level;
      cell.i = static_cast<uint32_t>(ox);
      cell.j = static_cast<uint32_t>(oy);
      cell.k = static_cast<uint32_t>(oz);
    }
  }
  return cell;
}

}  // namespace avr

#endif
