// The box rules of the products that stream every cell of a scene's boxes once (slice images, the
// joint histogram, on-axis projections, derived fields): what a box must satisfy before a kernel
// addresses its cells with 32 bits, once.  Host only and free of HIP and of the C ABI's handles: it
// works on avr_box, throws std::invalid_argument with the message the C ABI reports, and is tested
// as a plain C++ program (tests/cxx/field_boxes_test.cpp).
#ifndef AVR_FIELD_BOXES_H
#define AVR_FIELD_BOXES_H

#include <cstdint>
#include <stdexcept>
#include <vector>

#include "../../include/avr_hip.h"

namespace avr {

// One field's cells of one box as a kernel addresses them.
struct FieldView {
  const double* cells = nullptr;
  int32_t jstride = 0, kstride = 0;  // element strides (Array4)
  int32_t last = 0;                  // element offset of the box's last cell, < 2^28
  // cells 16-byte aligned and both strides even: f64 pairs load.  The rule of every kernel that
  // forms element offsets; classify_tile (avr_kernels.hip), which forms byte offsets, also caps
  // jstride below 2^27 and says why.
  bool paired = false;
};

inline void require_box(bool condition, const char* message) {
  if (!condition) throw std::invalid_argument(message);
}

// A box without cells: it takes no tile and its cells may be null.
inline bool box_is_empty(const avr_box& box) {
  return box.dims[0] <= 0 || box.dims[1] <= 0 || box.dims[2] <= 0;
}

// The view of a box that is not empty.  The span rule is what keeps the kernels' 32-bit element
// offsets (i + j * jstride + k * kstride, unsigned) in bounds.
inline FieldView field_view(const avr_box& box) {
  require_box(box.cells != nullptr, "box has no cell data");
  const int64_t span = static_cast<int64_t>(box.dims[0] - 1) +
                       static_cast<int64_t>(box.dims[1] - 1) * box.jstride +
                       static_cast<int64_t>(box.dims[2] - 1) * box.kstride;
  require_box(box.jstride >= 0 && box.kstride >= 0 && span < (int64_t{1} << 28),
              "box spans more than 2^28 cells (or has negative strides)");
  FieldView view;
  view.cells = box.cells;
  view.jstride = static_cast<int32_t>(box.jstride);
  view.kstride = static_cast<int32_t>(box.kstride);
  view.last = static_cast<int32_t>(span);
  view.paired = (reinterpret_cast<uintptr_t>(box.cells) & 15u) == 0 && (box.jstride & 1) == 0 &&
                (box.kstride & 1) == 0;
  return view;
}

// One box of n_fields fields that share a box list: the reference's level lies below n_levels and,
// field by field in order, the field's box has the reference's dims and level and (unless the box
// is empty) a view.  Fills views[0 .. n_fields) -- left zeroed for an empty box -- and *paired, the
// AND over the fields (1 for an empty box).  Returns whether the box holds cells.
inline bool field_box_views(const avr_box& reference, const avr_box* const* fields, int n_fields,
                            int n_levels, FieldView* views, int32_t* paired) {
  require_box(reference.level >= 0 && reference.level < n_levels,
              "a box's level is not below n_levels");
  const bool empty = box_is_empty(reference);
  *paired = 1;
  for (int f = 0; f < n_fields; ++f) {
    const avr_box& in = *fields[f];
    views[f] = FieldView{};
    require_box(in.dims[0] == reference.dims[0] && in.dims[1] == reference.dims[1] &&
                    in.dims[2] == reference.dims[2] && in.level == reference.level,
                "the scenes' boxes differ in dims or level");
    if (empty) continue;
    views[f] = field_view(in);
    if (!views[f].paired) *paired = 0;
  }
  return !empty;
}

// tile_begin is the prefix sum of the boxes' tiles ({0} before the first box): appends the next
// box's.  The kernels number tiles with 31 bits; a count of UINT32_MAX (one box's tiles already
// past them) is refused like any other.
inline void append_tiles(std::vector<uint32_t>* tile_begin, uint32_t tiles) {
  const uint64_t total = static_cast<uint64_t>(tile_begin->back()) + tiles;
  require_box(total < (uint64_t{1} << 31), "scene has too many cells");
  tile_begin->push_back(static_cast<uint32_t>(total));
}

}  // namespace avr

#endif
