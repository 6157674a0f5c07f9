// The host plans of the field products (slice images, the joint histogram, on-axis projections,
// derived fields, gradient fields, clumps with their members and pair energies, isosurfaces,
// streamlines, covering grids, grid fields, rays, per-ray sums, power spectra, isolated potentials,
// structure functions, velocity cubes, particle fields, particle groups):
// everything a call works out from its arguments before
// the first HIP call -- the argument rules, the box table, the tile prefix and the product's own
// tables.  Host only and free of HIP and of the C ABI's handles, like avr_field_boxes.h whose box
// rules it applies: a plan works on arrays of avr_box and the ABI's plain arguments, throws
// std::invalid_argument with the message the C ABI reports, and fills vectors and PODs that the
// entry point stages (tests/cxx/field_plans_test.cpp).  Pointers the ABI refuses as "null
// argument" whatever the other arguments are have been checked by the entry point.
//
// What a plan hands to its entry point (csrc/avr_field_products.cpp), one rule for every product:
//  - `args`, the struct the kernel is launched with.  The plan fills every field that is not a
//    device address -- counts, sizes, bounds, the locator, the image window -- and leaves every
//    address null; the entry point copies it and fills only addresses: the staged tables, the
//    context's scratch block and the caller's device arrays.
//  - visit_tables(args..., visit): the tables the call stages, named once, as visit(where in args
//    the table's device address goes, the host table, its count) in the order they are staged.  The
//    stager runs it twice, to size the batch (StagingSize, avr_internal.h) and to fill it; a table of count 0 is
//    staged as one value-initialised element that nothing reads, so a plan is never padded.
//  - `scratch` (where a product has a scratch block): the block's total bytes and each part's
//    byte offset, in part order.
#ifndef AVR_FIELD_PLANS_H
#define AVR_FIELD_PLANS_H

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "avr_cell_tiles.h"
#include "avr_field_boxes.h"
#include "avr_internal.h"
#include "avr_level_cells.h"

namespace avr {

// One part of a context scratch block: `bytes` from byte `offset` of the block on.  An optional
// part that the call does without is not present: it has no bytes and its address stays null.
struct ScratchPart {
  size_t offset = 0, bytes = 0;
  bool present = false;
};
// The next part of a block of `*total` bytes so far, behind the parts before it.
inline ScratchPart next_scratch_part(size_t* total, size_t bytes, bool present = true) {
  ScratchPart part;
  part.offset = *total;
  part.bytes = present ? bytes : 0;
  part.present = present;
  *total += part.bytes;
  return part;
}

inline void require_image_size(int width, int height) {
  require_box(width > 0 && height > 0, "image width and height must be positive");
  require_box(static_cast<int64_t>(width) * height <= (int64_t{1} << 31) - 1,
              "image has more than 2^31-1 pixels");
}

// ---- slice images -------------------------------------------------------------------------
// What launch_slice takes besides the plane: the slice kernel has no argument struct of its own.
struct SliceArgs {
  const SliceBoxDev* boxes;
  int32_t n_boxes;
  int32_t width, height;
};
struct SlicePlan {
  SlicePlaneDev plane;
  std::vector<SliceBoxDev> boxes;  // a box without cells stays zeroed but for index and level
  SliceArgs args{};
  template <class Visit>
  void visit_tables(SliceArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
  }
};
// global_index (may be null): what the box image holds for box b; by default b.
inline SlicePlan plan_slice(const avr_box* boxes, size_t n_boxes, const int32_t* global_index,
                            const double origin[3], const double du[3], const double dv[3],
                            int width, int height) {
  require_image_size(width, height);
  SlicePlan plan;
  for (int a = 0; a < 3; ++a) {
    require_box(std::isfinite(origin[a]) && std::isfinite(du[a]) && std::isfinite(dv[a]),
                "slice plane must be finite");
    plan.plane.origin[a] = origin[a];
    plan.plane.du[a] = du[a];
    plan.plane.dv[a] = dv[a];
  }
  plan.boxes.resize(n_boxes);
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& in = boxes[b];
    SliceBoxDev& dev = plan.boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    dev.global_index = global_index != nullptr ? global_index[b] : static_cast<int32_t>(b);
    require_box(in.level >= 0 && in.level <= 127, "box level must lie in [0, 127]");
    dev.level = in.level;
    if (box_is_empty(in)) continue;  // holds no point
    const FieldView view = field_view(in);
    for (int a = 0; a < 3; ++a) {
      dev.minc[a] = in.min_corner[a];
      dev.maxc[a] = in.max_corner[a];
      dev.n[a] = in.dims[a];
    }
    dev.cells = view.cells;
    dev.jstride = view.jstride;
    dev.kstride = view.kstride;
  }
  plan.args.n_boxes = static_cast<int32_t>(n_boxes);
  plan.args.width = width;
  plan.args.height = height;
  return plan;
}

// ---- joint histogram ----------------------------------------------------------------------
// n + 1 finite, strictly increasing edges; returns n / (e[n] - e[0]), or 0 if that is not finite
inline double joint_histogram_axis(const double* edges, int n, const char* axis) {
  const std::string name(axis);
  require_box(edges != nullptr, (name + "_edges is null").c_str());
  require_box(n >= 1 && n <= kJointHistogramMaxBins,
              (name + " bin count must lie in [1, 1024]").c_str());
  for (int i = 0; i <= n; ++i) {
    require_box(std::isfinite(edges[i]), (name + "_edges must be finite").c_str());
    require_box(i == 0 || edges[i - 1] < edges[i],
                (name + "_edges must be strictly increasing").c_str());
  }
  const double scale = static_cast<double>(n) / (edges[n] - edges[0]);
  return std::isfinite(scale) ? scale : 0.0;
}

struct JointHistogramPlan {
  std::vector<JointBoxDev> boxes;
  std::vector<uint32_t> tile_begin;
  std::vector<double> x_edges, y_edges;  // nx + 1 and ny + 1 (empty without scene_y)
  JointHistogramArgs args{};
  template <class Visit>
  void visit_tables(JointHistogramArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->tile_begin, tile_begin.data(), tile_begin.size());
    visit(&to->x_edges, x_edges.data(), x_edges.size());
    if (!y_edges.empty()) visit(&to->y_edges, y_edges.data(), y_edges.size());
  }
};
// y and s (may be null): the boxes of the second axis' field and of the summed field; an absent
// field repeats x.
inline JointHistogramPlan plan_joint_histogram(const avr_box* x, const avr_box* y, const avr_box* s,
                                               size_t n_boxes, const double* x_edges, int nx,
                                               const double* y_edges, int ny, int n_levels) {
  JointHistogramPlan plan;
  plan.args.x_scale = joint_histogram_axis(x_edges, nx, "x");
  if (y != nullptr) {
    plan.args.y_scale = joint_histogram_axis(y_edges, ny, "y");
  } else {
    require_box(ny == 1, "without scene_y there is one y bin");
  }
  require_box(static_cast<int64_t>(nx) * ny <= kJointHistogramMaxCells,
              "the histogram has more than 2^20 bins");
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  const avr_box* fields[3] = {x, y != nullptr ? y : x, s != nullptr ? s : x};
  plan.boxes.resize(n_boxes);
  plan.tile_begin.assign(1, 0u);
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = x[b];
    const avr_box* in[3] = {&first, &fields[1][b], &fields[2][b]};
    FieldView views[3];
    JointBoxDev& dev = plan.boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    const bool cells = field_box_views(first, in, 3, n_levels, views, &dev.paired);
    dev.level = first.level;
    for (int f = 0; f < 3; ++f) {
      dev.cells[f] = views[f].cells;
      dev.jstride[f] = views[f].jstride;
      dev.kstride[f] = views[f].kstride;
    }
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
    }
    append_tiles(&plan.tile_begin, cells ? cell_tiles(dev.nx, dev.ny, dev.nz) : 0u);
  }
  plan.args.n_boxes = static_cast<int32_t>(n_boxes);
  plan.args.n_tiles = plan.tile_begin.back();
  plan.args.nx = nx;
  plan.args.ny = ny;
  plan.args.x_lo = x_edges[0];
  plan.args.x_hi = x_edges[nx];
  plan.x_edges.assign(x_edges, x_edges + nx + 1);
  if (y != nullptr) {
    plan.args.y_lo = y_edges[0];
    plan.args.y_hi = y_edges[ny];
    plan.y_edges.assign(y_edges, y_edges + ny + 1);
  }
  return plan;
}

// ---- on-axis projection -------------------------------------------------------------------
// The partial planes: S [entries] f64, Wt [entries] f64 (with a weight), n [entries] u32.
struct AxisScratch {
  ScratchPart s, w, n;
  size_t total = 0;
};
inline AxisScratch axis_scratch(size_t entries, bool weighted) {
  AxisScratch scratch;
  scratch.s = next_scratch_part(&scratch.total, entries * sizeof(double));
  scratch.w = next_scratch_part(&scratch.total, entries * sizeof(double), weighted);
  scratch.n = next_scratch_part(&scratch.total, entries * sizeof(uint32_t));
  return scratch;
}
struct AxisProjectionPlan {
  std::vector<AxisBoxDev> boxes;     // as the reduction reads them
  std::vector<AxisPlaneDev> planes;  // as the gather reads them
  std::vector<uint32_t> tile_begin;
  uint32_t entries = 0;  // of the partial planes, all boxes: columns x segments, below 2^31
  AxisReduceArgs reduce{};
  AxisGatherArgs gather{};
  AxisScratch scratch;
  template <class Visit>
  void visit_tables(AxisReduceArgs* to_reduce, AxisGatherArgs* to_gather, Visit&& visit) const {
    visit(&to_reduce->boxes, boxes.data(), boxes.size());
    visit(&to_gather->boxes, planes.data(), planes.size());
    visit(&to_reduce->tile_begin, tile_begin.data(), tile_begin.size());
  }
};
// w (may be null): the boxes of the weight field; without one it repeats f.
inline AxisProjectionPlan plan_axis_projection(const avr_box* f, const avr_box* w, size_t n_boxes,
                                               int axis, const double origin_uv[2], double du,
                                               double dv, int width, int height,
                                               const double* level_dl, int n_levels) {
  require_box(axis >= 0 && axis <= 2, "axis must be 0 (x), 1 (y) or 2 (z)");
  require_image_size(width, height);
  require_box(std::isfinite(origin_uv[0]) && std::isfinite(origin_uv[1]) && std::isfinite(du) &&
                  std::isfinite(dv), "the window must be finite");
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  for (int l = 0; l < n_levels; ++l) {
    require_box(std::isfinite(level_dl[l]), "level_dl must be finite");
  }
  const int axis_u = (axis + 1) % 3, axis_v = (axis + 2) % 3;
  AxisProjectionPlan plan;
  plan.boxes.resize(n_boxes);
  plan.planes.resize(n_boxes);
  plan.tile_begin.assign(1, 0u);
  uint64_t entries = 0;
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = f[b];
    const avr_box* in[2] = {&first, w != nullptr ? &w[b] : &first};
    FieldView views[2];
    AxisBoxDev& dev = plan.boxes[b];
    AxisPlaneDev& plane = plan.planes[b];
    std::memset(&dev, 0, sizeof(dev));
    std::memset(&plane, 0, sizeof(plane));
    const bool cells = field_box_views(first, in, 2, n_levels, views, &dev.paired);
    dev.cells_f = views[0].cells;
    dev.jstride_f = views[0].jstride;
    dev.kstride_f = views[0].kstride;
    dev.cells_w = views[1].cells;
    dev.jstride_w = views[1].jstride;
    dev.kstride_w = views[1].kstride;
    uint32_t tiles = 0;
    dev.plane_begin = plane.plane_begin = static_cast<uint32_t>(entries);
    if (cells) {
      require_box(std::isfinite(first.min_corner[axis_u]) && std::isfinite(first.max_corner[axis_u]) &&
                      std::isfinite(first.min_corner[axis_v]) &&
                      std::isfinite(first.max_corner[axis_v]),
                  "box corners must be finite");
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
      tiles = axis_projection_tiles(axis, dev.nx, dev.ny, dev.nz);
      plane.min_u = first.min_corner[axis_u];
      plane.max_u = first.max_corner[axis_u];
      plane.min_v = first.min_corner[axis_v];
      plane.max_v = first.max_corner[axis_v];
      plane.dl = level_dl[first.level];
      plane.n_u = first.dims[axis_u];
      plane.n_v = first.dims[axis_v];
      plane.segments = (first.dims[axis] + kAxisSegment - 1) / kAxisSegment;
      entries += static_cast<uint64_t>(plane.n_u) * static_cast<uint64_t>(plane.n_v) *
                 static_cast<uint64_t>(plane.segments);
    }
    append_tiles(&plan.tile_begin, tiles);
    require_box(entries < (uint64_t{1} << 31), "scene has too many cells");
  }
  plan.entries = static_cast<uint32_t>(entries);
  plan.scratch = axis_scratch(plan.entries, w != nullptr);
  plan.reduce.n_boxes = plan.gather.n_boxes = static_cast<int32_t>(n_boxes);
  plan.reduce.n_tiles = plan.tile_begin.back();
  plan.gather.width = width;
  plan.gather.height = height;
  plan.gather.origin_u = origin_uv[0];
  plan.gather.origin_v = origin_uv[1];
  plan.gather.du = du;
  plan.gather.dv = dv;
  return plan;
}

// ---- shared by the products that write a scene: no written cell is also read --------------
// The cell ranges [first byte, last byte] of the boxes a product reads and of those it writes: no
// written box may share a byte with a read one.  Sorted by first byte, the read ranges that begin
// at or before a written one's last byte overlap it iff the largest of their last bytes reaches it.
typedef std::vector<std::pair<uintptr_t, uintptr_t>> ByteRanges;
inline void append_byte_range(ByteRanges* ranges, const FieldView& view) {
  const uintptr_t begin = reinterpret_cast<uintptr_t>(view.cells);
  ranges->emplace_back(begin, begin + static_cast<uintptr_t>(view.last) * 8 + 7);
}
// `bytes` > 0 bytes from `at` on: an array a call writes
inline void append_byte_range(ByteRanges* ranges, const void* at, uint64_t bytes) {
  const uintptr_t begin = reinterpret_cast<uintptr_t>(at);
  ranges->emplace_back(begin, begin + static_cast<uintptr_t>(bytes) - 1);
}
inline void require_no_shared_byte(
    ByteRanges* read_ranges, const ByteRanges& write_ranges,
    const char* message = "an output box's cells overlap an input box's cells") {
  std::sort(read_ranges->begin(), read_ranges->end());
  std::vector<uintptr_t> reach(read_ranges->size());
  for (size_t r = 0; r < read_ranges->size(); ++r) {
    reach[r] = r == 0 ? (*read_ranges)[r].second : std::max(reach[r - 1], (*read_ranges)[r].second);
  }
  for (const auto& w : write_ranges) {
    const size_t before =
        std::upper_bound(read_ranges->begin(), read_ranges->end(),
                         std::make_pair(w.second, UINTPTR_MAX)) - read_ranges->begin();
    require_box(before == 0 || reach[before - 1] < w.first, message);
  }
}

// ---- derived fields -----------------------------------------------------------------------
// The entry point applies it before it reads the array of input scenes, the plan first of all.
inline void require_derive_input_count(int n_inputs) {
  require_box(n_inputs >= 0 && n_inputs <= kDeriveMaxFields, "n_inputs must lie in [0, 6]");
}

// The program: known opcodes, operands in range, a stack that neither underflows nor holds more
// than 8 values, exactly one value at the end.
inline void verify_derive_program(const uint32_t* instructions, int n_instructions, int n_constants,
                                  int n_inputs) {
  int depth = 0;
  for (int pc = 0; pc < n_instructions; ++pc) {
    const uint32_t op = instructions[pc] & 0xffu, operand = instructions[pc] >> 8;
    require_box(op < kDeriveOpCount, "unknown opcode");
    int pops = 2;
    if (op <= kDeriveBuiltin) {
      pops = 0;
      const uint32_t limit = op == kDeriveConst   ? static_cast<uint32_t>(n_constants)
                             : op == kDeriveField ? static_cast<uint32_t>(n_inputs)
                                                  : kDeriveBuiltinCount;
      require_box(operand < limit, "an operand index is out of range");
    } else {
      require_box(operand == 0, "an operator takes no operand");
      if (op == kDeriveNeg || op == kDeriveSquare || op == kDeriveSqrt || op == kDeriveAbs) {
        pops = 1;
      } else if (op == kDeriveWhere) {
        pops = 3;
      }
    }
    require_box(depth >= pops, "the program underflows its stack");
    depth += 1 - pops;
    require_box(depth <= kDeriveMaxDepth, "the program's stack is deeper than 8");
  }
  require_box(depth == 1, "the program must end with exactly one value");
}

struct DerivePlan {
  std::vector<DeriveBoxDev> boxes;
  std::vector<uint32_t> tile_begin;
  DeriveProgramDev program;
  DeriveArgs args{};
  template <class Visit>
  void visit_tables(DeriveArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->tile_begin, tile_begin.data(), tile_begin.size());
    visit(&to->program, &program, 1);
  }
};
// inputs: n_inputs box lists of n_boxes boxes each; out: the boxes written, the reference of the
// box rules.
inline DerivePlan plan_derive(const avr_box* const* inputs, int n_inputs, const avr_box* out,
                              size_t n_boxes, const uint32_t* instructions, int n_instructions,
                              const double* constants, int n_constants, const double* box_origin,
                              const double* level_cell_size, int n_levels) {
  require_derive_input_count(n_inputs);
  require_box(n_instructions >= 1 && n_instructions <= kDeriveMaxInstructions,
              "n_instructions must lie in [1, 64]");
  require_box(n_constants >= 0 && n_constants <= kDeriveMaxConstants,
              "n_constants must lie in [0, 16]");
  require_box(n_constants == 0 || constants != nullptr, "null argument");
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  verify_derive_program(instructions, n_instructions, n_constants, n_inputs);
  for (int l = 0; l < n_levels * 3; ++l) {
    require_box(std::isfinite(level_cell_size[l]), "level_cell_size must be finite");
  }
  require_box(n_boxes == 0 || box_origin != nullptr, "null argument");
  DerivePlan plan;
  plan.boxes.resize(n_boxes);
  plan.tile_begin.assign(1, 0u);
  ByteRanges read_ranges, write_ranges;  // of the inputs' boxes and of the output's
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = out[b];
    const avr_box* in[kDeriveMaxFields + 1];  // the inputs, then the output
    for (int f = 0; f < n_inputs; ++f) in[f] = &inputs[f][b];
    in[n_inputs] = &first;
    FieldView views[kDeriveMaxFields + 1];
    DeriveBoxDev& dev = plan.boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    const bool cells = field_box_views(first, in, n_inputs + 1, n_levels, views, &dev.paired);
    dev.level = first.level;
    for (int f = 0; f <= n_inputs; ++f) {
      const bool is_out = f == n_inputs;
      const int slot = is_out ? kDeriveMaxFields : f;
      if (is_out) {
        dev.out = const_cast<double*>(views[f].cells);
      } else {
        dev.cells[f] = views[f].cells;
      }
      dev.jstride[slot] = views[f].jstride;
      dev.kstride[slot] = views[f].kstride;
      if (cells) append_byte_range(is_out ? &write_ranges : &read_ranges, views[f]);
    }
    for (int a = 0; a < 3; ++a) {
      require_box(std::isfinite(box_origin[b * 3 + a]), "box_origin must be finite");
      dev.origin[a] = box_origin[b * 3 + a];
    }
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
    }
    append_tiles(&plan.tile_begin, cells ? cell_tiles(dev.nx, dev.ny, dev.nz) : 0u);
  }
  require_no_shared_byte(&read_ranges, write_ranges);
  std::memset(&plan.program, 0, sizeof(plan.program));
  std::memcpy(plan.program.code, instructions, static_cast<size_t>(n_instructions) * sizeof(uint32_t));
  if (n_constants != 0) {
    std::memcpy(plan.program.constants, constants, static_cast<size_t>(n_constants) * sizeof(double));
  }
  std::memcpy(plan.program.cell_size, level_cell_size,
              static_cast<size_t>(n_levels) * 3 * sizeof(double));
  plan.args.n_boxes = static_cast<int32_t>(n_boxes);
  plan.args.n_tiles = plan.tile_begin.back();
  plan.args.n_fields = n_inputs;
  plan.args.n_instructions = n_instructions;
  return plan;
}

// ---- shared by the products that cross levels (gradient fields, clumps, isosurfaces,
// ---- streamlines): the level setup, the boxes in index space, the candidate lists ----------
// The cells [lo, hi] of a box, or of a face's ghost slab, in some level's index space.
struct IndexRegion {
  int64_t lo[3], hi[3];
};
inline bool regions_meet(const IndexRegion& a, const IndexRegion& b) {
  for (int d = 0; d < 3; ++d) {
    if (a.lo[d] > b.hi[d] || b.lo[d] > a.hi[d]) return false;
  }
  return true;
}

// ratio[l]: level l -> l + 1, at least 2 between two of the call's levels and 1 from n_levels - 1
// on.
inline void fill_level_ratios(const int32_t* level_ratio, int n_levels,
                              int32_t (&ratio)[kFieldMaxLevels]) {
  for (int l = 0; l < kFieldMaxLevels; ++l) ratio[l] = 1;
  for (int l = 0; l + 1 < n_levels; ++l) {
    require_box(level_ratio[l] >= 2, "a level ratio is below 2");
    ratio[l] = level_ratio[l];
  }
}
// level_cell_size: (dx, dy, dz) per level; prob_lo: three values.  Everything else of `levels` is
// left zero.
inline void fill_level_geometry(const double* level_cell_size, const double* prob_lo, int n_levels,
                                IsoLevelsDev* levels) {
  std::memset(levels, 0, sizeof(*levels));
  for (int l = 0; l < n_levels; ++l) {
    for (int d = 0; d < 3; ++d) {
      const double size = level_cell_size[l * 3 + d];
      require_box(std::isfinite(size) && size > 0.0, "level_cell_size must be finite and positive");
      levels->cell_size[l][d] = size;
    }
  }
  for (int d = 0; d < 3; ++d) {
    require_box(std::isfinite(prob_lo[d]), "prob_lo must be finite");
    levels->prob_lo[d] = prob_lo[d];
  }
}
// The cells of box b (which has some) in its level's index space, from box_index_lo (per box the
// index of its first cell, 3 per box), also as the device box's lo.  Inside [-2^30, 2^30) the
// ghost indices next to a box, and their children, stay far inside 64 bits.
inline IndexRegion box_index_region(const int32_t* box_index_lo, size_t b, const int32_t dims[3],
                                    int32_t (&dev_lo)[3]) {
  IndexRegion region;
  for (int d = 0; d < 3; ++d) {
    const int64_t lo = box_index_lo[b * 3 + d];
    dev_lo[d] = box_index_lo[b * 3 + d];
    region.lo[d] = lo;
    region.hi[d] = lo + dims[d] - 1;
    require_box(lo >= -(int64_t{1} << 30) && region.hi[d] < (int64_t{1} << 30),
                "a box's index range leaves [-2^30, 2^30)");
  }
  return region;
}
// ... of every box; a box without cells (nx == 0) keeps a zeroed entry that nothing reads.  Box: a
// device box with nx and lo; first: the scene whose dims the boxes took.
template <class Box>
inline std::vector<IndexRegion> box_index_regions(const int32_t* box_index_lo, const avr_box* first,
                                                  std::vector<Box>* boxes) {
  std::vector<IndexRegion> regions(boxes->size());
  for (size_t b = 0; b < boxes->size(); ++b) {
    if ((*boxes)[b].nx <= 0) continue;
    regions[b] = box_index_region(box_index_lo, b, first[b].dims, (*boxes)[b].lo);
  }
  return regions;
}
// No later box of box b's level shares an index with it ...
template <class Box>
inline void require_level_disjoint(const std::vector<Box>& boxes,
                                   const std::vector<IndexRegion>& regions, size_t b) {
  for (size_t c = b + 1; boxes[b].nx > 0 && c < boxes.size(); ++c) {
    require_box(boxes[c].nx <= 0 || boxes[c].level != boxes[b].level ||
                    !regions_meet(regions[b], regions[c]),
                "two boxes of one level overlap in index space");
  }
}
// ... and so for every box: the boxes of one level lie apart in index space.
template <class Box>
inline void require_levels_disjoint(const std::vector<Box>& boxes,
                                    const std::vector<IndexRegion>& regions) {
  for (size_t b = 0; b < boxes.size(); ++b) require_level_disjoint(boxes, regions, b);
}

// The boxes that can hold a cell of `region`, a range of indices of box b's level: the region at
// the box's own level, at every coarser one and, where finest is one above the box's level, one
// level finer; a box other than b of a level up to finest whose cells meet the region there is
// appended, in scene order.  Box: a device box with nx (0 without cells) and level; ratio[l]:
// level l -> l + 1.
template <class Box>
inline void append_region_candidates(const std::vector<Box>& boxes,
                                     const std::vector<IndexRegion>& regions, size_t b,
                                     const IndexRegion& region, const int32_t* ratio, int finest,
                                     std::vector<int32_t>* candidates) {
  const int level = boxes[b].level;
  IndexRegion slab[kFieldMaxLevels + 1];  // [m] at level m
  slab[level] = region;
  for (int m = level; m > 0; --m) {
    for (int d = 0; d < 3; ++d) {
      slab[m - 1].lo[d] = floor_div(slab[m].lo[d], ratio[m - 1]);
      slab[m - 1].hi[d] = floor_div(slab[m].hi[d], ratio[m - 1]);
    }
  }
  if (finest > level) {
    const int64_t r = ratio[level];
    for (int d = 0; d < 3; ++d) {
      slab[finest].lo[d] = slab[level].lo[d] * r;
      slab[finest].hi[d] = slab[level].hi[d] * r + (r - 1);
    }
  }
  for (size_t c = 0; c < boxes.size(); ++c) {
    if (c == b || boxes[c].nx <= 0 || boxes[c].level > finest) continue;
    if (regions_meet(slab[boxes[c].level], regions[c])) {
      candidates->push_back(static_cast<int32_t>(c));
    }
  }
  require_box(candidates->size() < (size_t{1} << 31), "scene has too many neighbouring boxes");
}

// The boxes that can hold a ghost of one face of box b: append_region_candidates for the ghost
// slab next to the face (axis, side: 0 low, 1 high).
template <class Box>
inline void append_face_candidates(const std::vector<Box>& boxes,
                                   const std::vector<IndexRegion>& regions, size_t b, int axis,
                                   int side, const int32_t* ratio, int finest,
                                   std::vector<int32_t>* candidates) {
  IndexRegion slab = regions[b];
  slab.lo[axis] = slab.hi[axis] = side == 0 ? regions[b].lo[axis] - 1 : regions[b].hi[axis] + 1;
  append_region_candidates(boxes, regions, b, slab, ratio, finest, candidates);
}

// ---- gradient fields ----------------------------------------------------------------------
// The face planes: [2][faces] f64, then [2][faces] presence bytes.
struct GradientScratch {
  ScratchPart face_value, face_present;
  size_t total = 0;
};
inline GradientScratch gradient_scratch(size_t faces) {
  GradientScratch scratch;
  scratch.face_value = next_scratch_part(&scratch.total, faces * 2 * sizeof(double));
  scratch.face_present = next_scratch_part(&scratch.total, faces * 2);
  return scratch;
}
struct GradientPlan {
  std::vector<GradientBoxDev> boxes;
  std::vector<uint32_t> tile_begin;
  std::vector<uint32_t> face_begin;  // n_boxes + 1: prefix sum of the boxes' face cells
  // CSR over (box, side), entry 2 b + side: the boxes that can hold a ghost of that face
  std::vector<uint32_t> candidate_begin;
  std::vector<int32_t> candidates;   // empty when no face has a neighbour
  LevelRatiosDev levels;
  GradientArgs args{};
  GradientScratch scratch;
  template <class Visit>
  void visit_tables(GradientArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->tile_begin, tile_begin.data(), tile_begin.size());
    visit(&to->face_begin, face_begin.data(), face_begin.size());
    visit(&to->candidate_begin, candidate_begin.data(), candidate_begin.size());
    visit(&to->candidates, candidates.data(), candidates.size());
    visit(&to->levels, &levels, 1);
  }
};
// box_index_lo: per box the index of its first cell in its level's index space (3 per box);
// level_ratio[l]: level l -> l + 1.
inline GradientPlan plan_gradient(const avr_box* in, const avr_box* out, size_t n_boxes, int axis,
                                  const int32_t* box_index_lo, const int32_t* level_ratio,
                                  const double* level_cell_size, int n_levels) {
  require_box(axis >= 0 && axis <= 2, "axis must be 0 (x), 1 (y) or 2 (z)");
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  require_box(n_levels == 1 || level_ratio != nullptr, "null argument");
  GradientPlan plan;
  LevelRatiosDev& levels = plan.levels;
  fill_level_ratios(level_ratio, n_levels, levels.ratio);
  for (int l = 0; l < n_levels; ++l) {
    require_box(std::isfinite(level_cell_size[l]) && level_cell_size[l] > 0.0,
                "level_cell_size must be finite and positive");
  }
  require_box(n_boxes == 0 || box_index_lo != nullptr, "null argument");
  std::vector<GradientBoxDev>& boxes = plan.boxes;
  boxes.resize(n_boxes);
  std::vector<IndexRegion> regions(n_boxes);
  plan.tile_begin.assign(1, 0u);
  plan.face_begin.assign(1, 0u);
  ByteRanges read_ranges, write_ranges;
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = in[b];
    const avr_box* fields[2] = {&first, &out[b]};
    FieldView views[2];
    GradientBoxDev& dev = boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    const bool cells = field_box_views(first, fields, 2, n_levels, views, &dev.paired);
    dev.in = views[0].cells;
    dev.out = const_cast<double*>(views[1].cells);
    dev.jstride_in = views[0].jstride;
    dev.kstride_in = views[0].kstride;
    dev.jstride_out = views[1].jstride;
    dev.kstride_out = views[1].kstride;
    dev.level = first.level;
    dev.dx = level_cell_size[first.level];
    dev.face_begin = plan.face_begin.back();
    uint64_t faces = 0;
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
      append_byte_range(&read_ranges, views[0]);
      append_byte_range(&write_ranges, views[1]);
      regions[b] = box_index_region(box_index_lo, b, first.dims, dev.lo);
      faces = static_cast<uint64_t>(first.dims[(axis + 1) % 3]) *
              static_cast<uint64_t>(first.dims[(axis + 2) % 3]);
    }
    append_tiles(&plan.tile_begin, cells ? cell_tiles(dev.nx, dev.ny, dev.nz) : 0u);
    const uint64_t total = plan.face_begin.back() + faces;
    require_box(total < (uint64_t{1} << 30), "scene has too many cells");
    plan.face_begin.push_back(static_cast<uint32_t>(total));
  }
  require_no_shared_byte(&read_ranges, write_ranges);
  // Per box and side the ghost slab at the box's own level, at every coarser one and one level
  // finer; a box of one of those levels whose cells meet the slab there is a candidate.
  std::vector<int32_t>& candidates = plan.candidates;
  plan.candidate_begin.assign(1, 0u);
  for (size_t b = 0; b < n_boxes; ++b) {
    const int level = boxes[b].level;
    const bool cells = boxes[b].nx > 0;
    require_level_disjoint(boxes, regions, b);
    for (int side = 0; side < 2; ++side) {
      if (cells) {
        const int finest = level + 1 < n_levels ? level + 1 : level;
        append_face_candidates(boxes, regions, b, axis, side, levels.ratio, finest, &candidates);
      }
      plan.candidate_begin.push_back(static_cast<uint32_t>(candidates.size()));
    }
  }
  plan.scratch = gradient_scratch(plan.face_begin.back());
  plan.args.n_boxes = static_cast<int32_t>(n_boxes);
  plan.args.n_levels = n_levels;
  plan.args.n_tiles = plan.tile_begin.back();
  plan.args.n_faces = plan.face_begin.back();
  return plan;
}

// ---- clumps -------------------------------------------------------------------------------
// The parent entries, padded to whole chunks, then one count per chunk.
struct ClumpScratch {
  ScratchPart parent, chunk_roots;
  size_t total = 0;
};
inline ClumpScratch clump_scratch(size_t chunks) {
  ClumpScratch scratch;
  scratch.parent = next_scratch_part(&scratch.total, chunks * kClumpChunk * sizeof(uint32_t));
  scratch.chunk_roots = next_scratch_part(&scratch.total, chunks * sizeof(uint32_t));
  return scratch;
}
struct ClumpPlan {
  std::vector<ClumpBoxDev> boxes;
  std::vector<uint32_t> tile_begin;
  std::vector<uint32_t> cell_begin;  // n_boxes + 1: prefix sum of the boxes' cells, in scene order
  // CSR over (box, axis, side), entry 6 b + 2 axis + side: the boxes of the same or a coarser
  // level that can hold a ghost of that face
  std::vector<uint32_t> candidate_begin;
  std::vector<int32_t> candidates;   // empty when no face has a neighbour
  LevelRatiosDev levels;
  ClumpArgs args{};
  ClumpScratch scratch;
  template <class Visit>
  void visit_tables(ClumpArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->tile_begin, tile_begin.data(), tile_begin.size());
    visit(&to->candidate_begin, candidate_begin.data(), candidate_begin.size());
    visit(&to->candidates, candidates.data(), candidates.size());
    visit(&to->levels, &levels, 1);
  }
};
// box_index_lo and level_ratio as plan_gradient takes them.  The rules, in this order: the bounds,
// n_levels, the box rules (the input is the reference), the ratios, the index ranges, boxes of one
// level apart in index space, no output byte shared with an input, fewer than 2^31 cells.
inline ClumpPlan plan_clumps(const avr_box* in, const avr_box* out, size_t n_boxes, double lower,
                             double upper, const int32_t* box_index_lo, const int32_t* level_ratio,
                             int n_levels) {
  require_box(!std::isnan(lower) && !std::isnan(upper), "a bound is NaN");
  require_box(lower <= upper, "lower must not exceed upper");
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  require_box(n_levels == 1 || level_ratio != nullptr, "null argument");
  require_box(n_boxes == 0 || box_index_lo != nullptr, "null argument");
  ClumpPlan plan;
  std::vector<ClumpBoxDev>& boxes = plan.boxes;
  boxes.resize(n_boxes);
  plan.tile_begin.assign(1, 0u);
  ByteRanges read_ranges, write_ranges;
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = in[b];
    const avr_box* fields[2] = {&first, &out[b]};
    FieldView views[2];
    ClumpBoxDev& dev = boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    const bool cells = field_box_views(first, fields, 2, n_levels, views, &dev.paired);
    dev.in = views[0].cells;
    dev.out = const_cast<double*>(views[1].cells);
    dev.jstride_in = views[0].jstride;
    dev.kstride_in = views[0].kstride;
    dev.jstride_out = views[1].jstride;
    dev.kstride_out = views[1].kstride;
    dev.level = first.level;
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
      append_byte_range(&read_ranges, views[0]);
      append_byte_range(&write_ranges, views[1]);
    }
    append_tiles(&plan.tile_begin, cells ? cell_tiles(dev.nx, dev.ny, dev.nz) : 0u);
  }
  LevelRatiosDev& levels = plan.levels;
  fill_level_ratios(level_ratio, n_levels, levels.ratio);
  const std::vector<IndexRegion> regions = box_index_regions(box_index_lo, in, &boxes);
  require_levels_disjoint(boxes, regions);
  require_no_shared_byte(&read_ranges, write_ranges);
  plan.cell_begin.assign(1, 0u);
  uint64_t total = 0;
  for (size_t b = 0; b < n_boxes; ++b) {
    // a box's cells are at most 2^28 (its span), so the sum stays far inside 64 bits
    total += static_cast<uint64_t>(boxes[b].nx) * static_cast<uint64_t>(boxes[b].ny) *
             static_cast<uint64_t>(boxes[b].nz);
    require_box(total < (uint64_t{1} << 31), "scene has too many cells for 32-bit labels");
    boxes[b].cell_begin = plan.cell_begin.back();
    plan.cell_begin.push_back(static_cast<uint32_t>(total));
  }
  plan.candidate_begin.assign(1, 0u);
  for (size_t b = 0; b < n_boxes; ++b) {
    for (int face = 0; face < 6; ++face) {
      if (boxes[b].nx > 0) {
        append_face_candidates(boxes, regions, b, face >> 1, face & 1, levels.ratio, boxes[b].level,
                               &plan.candidates);
      }
      plan.candidate_begin.push_back(static_cast<uint32_t>(plan.candidates.size()));
    }
  }
  plan.args.n_boxes = static_cast<int32_t>(n_boxes);
  plan.args.n_levels = n_levels;
  plan.args.n_tiles = plan.tile_begin.back();
  plan.args.n_cells = plan.cell_begin.back();
  plan.args.n_chunks = (plan.args.n_cells + kClumpChunk - 1) / kClumpChunk;
  plan.args.lower = lower;
  plan.args.upper = upper;
  plan.scratch = clump_scratch(plan.args.n_chunks);
  return plan;
}

struct ClumpTablePlan {
  std::vector<JointBoxDev> boxes;  // field 0: the labels; field 1: the summed field, or the labels
  std::vector<uint32_t> tile_begin;
  ClumpTableArgs args{};
  template <class Visit>
  void visit_tables(ClumpTableArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->tile_begin, tile_begin.data(), tile_begin.size());
  }
};
// field (may be null): the boxes of the summed field.
inline ClumpTablePlan plan_clump_table(const avr_box* labels, const avr_box* field, size_t n_boxes,
                                       uint64_t n_clumps, int n_levels) {
  require_box(n_clumps >= 1, "n_clumps must be at least 1");
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  require_box(n_clumps < static_cast<uint64_t>(kClumpTableMaxEntries) &&
                  n_clumps * static_cast<uint64_t>(n_levels) <
                      static_cast<uint64_t>(kClumpTableMaxEntries),
              "n_clumps * n_levels must stay below 2^28");
  ClumpTablePlan plan;
  plan.boxes.resize(n_boxes);
  plan.tile_begin.assign(1, 0u);
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = labels[b];
    const avr_box* in[2] = {&first, field != nullptr ? &field[b] : &first};
    FieldView views[2];
    JointBoxDev& dev = plan.boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    const bool cells = field_box_views(first, in, 2, n_levels, views, &dev.paired);
    dev.level = first.level;
    for (int f = 0; f < 2; ++f) {
      dev.cells[f] = views[f].cells;
      dev.jstride[f] = views[f].jstride;
      dev.kstride[f] = views[f].kstride;
    }
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
    }
    append_tiles(&plan.tile_begin, cells ? cell_tiles(dev.nx, dev.ny, dev.nz) : 0u);
  }
  plan.args.n_boxes = static_cast<int32_t>(n_boxes);
  plan.args.n_tiles = plan.tile_begin.back();
  plan.args.n_clumps = static_cast<uint32_t>(n_clumps);
  return plan;
}

// The links and extents of a label field ("Clump tree").  refined[b]: box b in the
// index space of level n_levels - 1, a cell of level l covering R_l = ratio[l] * ... *
// ratio[n_levels - 2] cells of it per axis.
struct ClumpLinksPlan {
  std::vector<JointBoxDev> boxes;  // field 0: the labels; field 1: the parent labels, or the labels
  std::vector<ClumpLinkBoxDev> refined;  // a box without cells keeps a zeroed entry
  std::vector<uint32_t> tile_begin;
  ClumpLinkArgs args{};
  template <class Visit>
  void visit_tables(ClumpLinkArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->refined, refined.data(), refined.size());
    visit(&to->tile_begin, tile_begin.data(), tile_begin.size());
  }
};
// parents (may be null): the boxes of the label scene of the ladder's step below.  box_index_lo
// and level_ratio as plan_gradient takes them.  The rules, in this order: n_clumps, n_parents,
// n_levels, null arrays, the box rules on the labels, the ratios, the index ranges, the refined
// index ranges, the parents' boxes against the labels'.
inline ClumpLinksPlan plan_clump_links(const avr_box* labels, const avr_box* parents,
                                       size_t n_boxes, uint64_t n_clumps, uint64_t n_parents,
                                       const int32_t* box_index_lo, const int32_t* level_ratio,
                                       int n_levels) {
  const uint64_t limit = static_cast<uint64_t>(kClumpTableMaxEntries);
  require_box(n_clumps >= 1 && n_clumps < limit, "n_clumps must lie in [1, 2^28)");
  if (parents != nullptr) {
    require_box(n_parents >= 1 && n_parents < limit, "n_parents must lie in [1, 2^28)");
  } else {
    require_box(n_parents == 0, "without a parent scene n_parents must be 0");
  }
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  require_box(n_levels == 1 || level_ratio != nullptr, "null argument");
  require_box(n_boxes == 0 || box_index_lo != nullptr, "null argument");
  ClumpLinksPlan plan;
  plan.boxes.resize(n_boxes);
  plan.refined.resize(n_boxes);
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = labels[b];
    const avr_box* in[1] = {&first};
    FieldView view;
    JointBoxDev& dev = plan.boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    std::memset(&plan.refined[b], 0, sizeof(plan.refined[b]));
    const bool cells = field_box_views(first, in, 1, n_levels, &view, &dev.paired);
    dev.level = first.level;
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
    }
  }
  LevelRatiosDev levels;
  fill_level_ratios(level_ratio, n_levels, levels.ratio);
  // R_l, held at 2^32 from there on: a cell that wide cannot lie inside [-2^30, 2^30)
  int64_t scale[kFieldMaxLevels];
  scale[n_levels - 1] = 1;
  for (int l = n_levels - 2; l >= 0; --l) {
    scale[l] = std::min(scale[l + 1] * levels.ratio[l], int64_t{1} << 32);
  }
  std::vector<IndexRegion> regions(n_boxes);
  for (size_t b = 0; b < n_boxes; ++b) {
    if (plan.boxes[b].nx <= 0) continue;
    int32_t lo[3];
    regions[b] = box_index_region(box_index_lo, b, labels[b].dims, lo);
  }
  for (size_t b = 0; b < n_boxes; ++b) {
    if (plan.boxes[b].nx <= 0) continue;
    const int64_t r = scale[plan.boxes[b].level];
    for (int d = 0; d < 3; ++d) {
      const int64_t lo = regions[b].lo[d] * r, hi = (regions[b].hi[d] + 1) * r - 1;
      require_box(lo >= -(int64_t{1} << 30) && hi < (int64_t{1} << 30),
                  "a box's refined index range leaves [-2^30, 2^30)");
      plan.refined[b].lo[d] = static_cast<int32_t>(lo);
    }
    plan.refined[b].scale = static_cast<int32_t>(r);
  }
  plan.tile_begin.assign(1, 0u);
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = labels[b];
    const avr_box* in[2] = {&first, parents != nullptr ? &parents[b] : &first};
    FieldView views[2];
    JointBoxDev& dev = plan.boxes[b];
    const bool cells = field_box_views(first, in, 2, n_levels, views, &dev.paired);
    for (int f = 0; f < 2; ++f) {
      dev.cells[f] = views[f].cells;
      dev.jstride[f] = views[f].jstride;
      dev.kstride[f] = views[f].kstride;
    }
    append_tiles(&plan.tile_begin, cells ? cell_tiles(dev.nx, dev.ny, dev.nz) : 0u);
  }
  plan.args.n_boxes = static_cast<int32_t>(n_boxes);
  plan.args.n_tiles = plan.tile_begin.back();
  plan.args.n_clumps = static_cast<uint32_t>(n_clumps);
  plan.args.n_parents = static_cast<uint32_t>(n_parents);
  return plan;
}

// The member cells of a label field's wanted clumps ("Clump binding").  The cell
// ordinals are those of "Clumps": cell_begin[b] + (k ny + j) nx + i.
struct ClumpMembersPlan {
  std::vector<JointBoxDev> boxes;    // every field: the labels
  std::vector<uint32_t> tile_begin;
  std::vector<uint32_t> cell_begin;  // n_boxes + 1: prefix sum of the boxes' cells, in scene order
  ClumpMembersArgs args{};
  template <class Visit>
  void visit_tables(ClumpMembersArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->tile_begin, tile_begin.data(), tile_begin.size());
    visit(&to->cell_begin, cell_begin.data(), cell_begin.size());
  }
};
// The prefix sum of the boxes' cells: fewer than 2^31 in all.  Box: a device box with nx, ny, nz.
template <class Box>
inline std::vector<uint32_t> cell_ordinals(const std::vector<Box>& boxes) {
  std::vector<uint32_t> cell_begin(1, 0u);
  uint64_t total = 0;
  for (const Box& box : boxes) {
    // a box's cells are at most 2^28 (its span), so the sum stays far inside 64 bits
    total += static_cast<uint64_t>(box.nx) * static_cast<uint64_t>(box.ny) *
             static_cast<uint64_t>(box.nz);
    require_box(total < (uint64_t{1} << 31), "scene has too many cells for 32-bit labels");
    cell_begin.push_back(static_cast<uint32_t>(total));
  }
  return cell_begin;
}
// The rules, in this order: n_clumps, capacity, the box rules (a level below 16), fewer than 2^31
// cells.
inline ClumpMembersPlan plan_clump_members(const avr_box* labels, size_t n_boxes, uint64_t n_clumps,
                                           uint64_t capacity) {
  require_box(n_clumps >= 1 && n_clumps < static_cast<uint64_t>(kClumpTableMaxEntries),
              "n_clumps must lie in [1, 2^28)");
  require_box(capacity >= 1 && capacity < (uint64_t{1} << 31), "capacity must lie in [1, 2^31)");
  ClumpMembersPlan plan;
  plan.boxes.resize(n_boxes);
  plan.tile_begin.assign(1, 0u);
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = labels[b];
    const avr_box* in[1] = {&first};
    FieldView view;
    JointBoxDev& dev = plan.boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    const bool cells = field_box_views(first, in, 1, kFieldMaxLevels, &view, &dev.paired);
    dev.level = first.level;
    for (int f = 0; f < 3; ++f) {
      dev.cells[f] = view.cells;
      dev.jstride[f] = view.jstride;
      dev.kstride[f] = view.kstride;
    }
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
    }
    append_tiles(&plan.tile_begin, cells ? cell_tiles(dev.nx, dev.ny, dev.nz) : 0u);
  }
  plan.cell_begin = cell_ordinals(plan.boxes);
  plan.args.n_boxes = static_cast<int32_t>(n_boxes);
  plan.args.n_tiles = plan.tile_begin.back();
  plan.args.n_clumps = static_cast<uint32_t>(n_clumps);
  plan.args.capacity = capacity;
  return plan;
}

// What is looked up per member key: the level and centre of the key's cell, and a field's value.
struct ClumpMemberDataPlan {
  std::vector<ClumpMemberBoxDev> boxes;
  std::vector<uint32_t> cell_begin;
  IsoLevelsDev levels;
  ClumpMemberDataArgs args{};
  template <class Visit>
  void visit_tables(ClumpMemberDataArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->cell_begin, cell_begin.data(), cell_begin.size());
    visit(&to->levels, &levels, 1);
  }
};
// scene: the boxes the keys' ordinals count; field (may be null): a field's boxes, congruent to
// them.  The rules, in this order: n_members, n_levels, null arrays, the box rules, fewer than 2^31
// cells, the ratios, the index ranges, finite sizes and origin.
inline ClumpMemberDataPlan plan_clump_member_data(const avr_box* scene, const avr_box* field,
                                                  size_t n_boxes, uint64_t n_members,
                                                  const int32_t* box_index_lo,
                                                  const int32_t* level_ratio,
                                                  const double* level_cell_size,
                                                  const double* prob_lo, int n_levels) {
  require_box(n_members < (uint64_t{1} << 31), "n_members must stay below 2^31");
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  require_box(n_levels == 1 || level_ratio != nullptr, "null argument");
  require_box(n_boxes == 0 || box_index_lo != nullptr, "null argument");
  require_box(level_cell_size != nullptr && prob_lo != nullptr, "null argument");
  ClumpMemberDataPlan plan;
  plan.boxes.resize(n_boxes);
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = scene[b];
    const avr_box* in[2] = {&first, field != nullptr ? &field[b] : &first};
    FieldView views[2];
    ClumpMemberBoxDev& dev = plan.boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    int32_t paired;
    const bool cells = field_box_views(first, in, 2, n_levels, views, &paired);
    dev.level = first.level;
    if (field != nullptr) {
      dev.field = views[1].cells;
      dev.jstride = views[1].jstride;
      dev.kstride = views[1].kstride;
    }
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
    }
  }
  plan.cell_begin = cell_ordinals(plan.boxes);
  int32_t ratio[kFieldMaxLevels];
  fill_level_ratios(level_ratio, n_levels, ratio);
  box_index_regions(box_index_lo, scene, &plan.boxes);
  fill_level_geometry(level_cell_size, prob_lo, n_levels, &plan.levels);
  plan.args.n_boxes = static_cast<int32_t>(n_boxes);
  plan.args.n_cells = plan.cell_begin.back();
  plan.args.n_members = static_cast<uint32_t>(n_members);
  return plan;
}

// The pairwise self-energy of member segments ("Clump binding").  Segment s holds the
// members offsets[s] .. offsets[s + 1] - 1, cut into tiles of kClumpPairTile; every tile pair
// (i_tile, j_tile) with j_tile >= i_tile belongs to exactly one item.  A row of T tiles is cut
// into j chunks of clump_pair_chunk(T) tiles, so that a segment of a few tiles still fills more
// than a few workgroups, and no lane ever adds more than 64 * 256 terms in a row.
inline uint32_t clump_pair_chunk(uint32_t tiles) {
  return std::min(kClumpPairMaxChunk, std::max(1u, (tiles + 7u) / 8u));
}
struct ClumpPairsPlan {
  std::vector<ClumpPairItem> items;     // segment by segment, row by row, chunk by chunk
  std::vector<uint32_t> partial_begin;  // n_segments + 1: a segment's items and partials
  // depth[s]: the longest chain of rounded additions a term of segment s passes through -- the
  // terms one lane adds in a row (at most the segment's members, and the chunk's), 8 for the
  // workgroup's shuffle steps (6 are taken), the 3 additions of its four waves' sums through LDS,
  // the partials one lane of the reduction adds, and that wave's 6 shuffle steps.  0 for a
  // segment of fewer than two members, which has no term.
  std::vector<int64_t> depth;
  ClumpPairArgs args{};
  size_t scratch_bytes = 0;             // the partials
  template <class Visit>
  void visit_tables(ClumpPairArgs* to, Visit&& visit) const {
    visit(&to->items, items.data(), items.size());
    visit(&to->partial_begin, partial_begin.data(), partial_begin.size());
  }
};
// The items of a segment of `count` members: one per row and j chunk.
inline uint64_t clump_pair_items(uint32_t count) {
  if (count < 2) return 0;
  const uint32_t tiles = (count + kClumpPairTile - 1) / kClumpPairTile;
  const uint32_t chunk = clump_pair_chunk(tiles);
  uint64_t items = 0;
  for (uint32_t i = 0; i < tiles; ++i) items += (tiles - i + chunk - 1) / chunk;
  return items;
}
// The rules, in this order: the offsets ascend from 0; no segment holds more than 2^22 members;
// fewer than 2^31 members in all; fewer than 2^28 segments; fewer than 2^26 items, counted before
// any table is made.
inline ClumpPairsPlan plan_clump_pairs(const int64_t* offsets, uint64_t n_segments) {
  require_box(offsets != nullptr, "null argument");
  require_box(offsets[0] == 0, "offsets must ascend from 0");
  for (uint64_t s = 0; s < n_segments; ++s) {
    require_box(offsets[s] <= offsets[s + 1], "offsets must ascend from 0");
  }
  for (uint64_t s = 0; s < n_segments; ++s) {
    require_box(static_cast<uint64_t>(offsets[s + 1] - offsets[s]) <= kClumpPairMaxSegment,
                "a segment holds more than 2^22 members");
  }
  require_box(offsets[n_segments] < (int64_t{1} << 31), "the segments hold 2^31 or more members");
  require_box(n_segments < static_cast<uint64_t>(kClumpTableMaxEntries),
              "n_segments must stay below 2^28");
  uint64_t n_items = 0;
  for (uint64_t s = 0; s < n_segments; ++s) {
    n_items += clump_pair_items(static_cast<uint32_t>(offsets[s + 1] - offsets[s]));
    require_box(n_items < kClumpPairMaxItems, "the segments make 2^26 or more work items");
  }
  ClumpPairsPlan plan;
  plan.items.reserve(n_items);
  plan.partial_begin.assign(1, 0u);
  plan.partial_begin.reserve(n_segments + 1);
  plan.depth.assign(n_segments, 0);
  n_items = 0;
  for (uint64_t s = 0; s < n_segments; ++s) {
    const uint32_t begin = static_cast<uint32_t>(offsets[s]);
    const uint32_t count = static_cast<uint32_t>(offsets[s + 1] - offsets[s]);
    if (count >= 2) {
      const uint32_t tiles = (count + kClumpPairTile - 1) / kClumpPairTile;
      const uint32_t chunk = clump_pair_chunk(tiles);
      const uint64_t segment_items = clump_pair_items(count);
      n_items += segment_items;
      for (uint32_t i = 0; i < tiles; ++i) {
        for (uint32_t j = i; j < tiles; j += chunk) {
          plan.items.push_back({begin, count, i, j | (std::min(chunk, tiles - j) << 16)});
        }
      }
      const int64_t lane_terms = std::min<int64_t>(count, int64_t{chunk} * kClumpPairTile);
      const int64_t strided = static_cast<int64_t>((segment_items + 63) / 64);
      plan.depth[s] = lane_terms + 8 + 3 + strided + 6;
    }
    plan.partial_begin.push_back(static_cast<uint32_t>(n_items));
  }
  plan.args.n_items = static_cast<uint32_t>(n_items);
  plan.args.n_segments = static_cast<uint32_t>(n_segments);
  plan.scratch_bytes = static_cast<size_t>(n_items) * sizeof(double);
  return plan;
}

// ---- isosurfaces --------------------------------------------------------------------------
// The shells' values (and sample values), the chunks' offsets, triangles and skipped cubes, then
// the shells' code bytes.
struct IsoScratch {
  ScratchPart shell_value, shell_sample, chunk_offset, chunk_triangles, chunk_skipped, shell_code;
  size_t total = 0;
};
inline IsoScratch iso_scratch(size_t shell, size_t chunks, bool has_sample) {
  IsoScratch scratch;
  scratch.shell_value = next_scratch_part(&scratch.total, shell * sizeof(double));
  scratch.shell_sample = next_scratch_part(&scratch.total, shell * sizeof(double), has_sample);
  scratch.chunk_offset = next_scratch_part(&scratch.total, chunks * sizeof(unsigned long long));
  scratch.chunk_triangles = next_scratch_part(&scratch.total, chunks * sizeof(uint32_t));
  scratch.chunk_skipped = next_scratch_part(&scratch.total, chunks * sizeof(uint32_t));
  scratch.shell_code = next_scratch_part(&scratch.total, shell);
  return scratch;
}
struct IsoPlan {
  std::vector<IsoBoxDev> boxes;
  std::vector<uint32_t> base_begin;   // n_boxes + 1: prefix sum of the boxes' cube bases
  std::vector<uint64_t> shell_begin;  // n_boxes + 1: prefix sum of the boxes' shell cells
  // CSR over boxes: the boxes of the same or a coarser level that can hold a cell of the box's
  // one-cell ghost shell
  std::vector<uint32_t> candidate_begin;
  std::vector<int32_t> candidates;    // empty when no box has a neighbour
  IsoLevelsDev levels;
  IsoArgs args{};
  IsoScratch scratch;
  template <class Visit>
  void visit_tables(IsoArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->shell_begin, shell_begin.data(), shell_begin.size());
    visit(&to->levels, &levels, 1);
    visit(&to->base_begin, base_begin.data(), base_begin.size());
    visit(&to->candidate_begin, candidate_begin.data(), candidate_begin.size());
    visit(&to->candidates, candidates.data(), candidates.size());
  }
};
// sample (may be null): the boxes of the sample field.  box_index_lo and level_ratio as
// plan_gradient takes them; level_cell_size: (dx, dy, dz) per level; prob_lo: three values.  The
// outputs are device arrays of `capacity` triangles (unused, and free to be null, with capacity
// 0); counts is never null.  The rules, in this order: the value, n_levels, null arrays, the cell
// sizes, prob_lo, the capacity and its arrays, the box rules (the field is the reference, so an
// incongruent sample scene is refused here), the ratios, the index ranges, boxes of one level
// apart in index space, no output byte shared with an input, fewer than 2^31 cube bases.
inline IsoPlan plan_isosurface(const avr_box* field, const avr_box* sample, size_t n_boxes,
                               double value, const int32_t* box_index_lo,
                               const int32_t* level_ratio, const double* level_cell_size,
                               const double* prob_lo, int n_levels, uint64_t capacity,
                               const void* vertices, const void* levels_out, const void* samples,
                               const void* counts) {
  require_box(std::isfinite(value), "value must be finite");
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  require_box(n_levels == 1 || level_ratio != nullptr, "null argument");
  require_box(n_boxes == 0 || box_index_lo != nullptr, "null argument");
  IsoPlan plan;
  IsoLevelsDev& levels = plan.levels;
  fill_level_geometry(level_cell_size, prob_lo, n_levels, &levels);
  require_box(capacity < kIsoMaxCapacity, "capacity must stay below 2^36");
  if (capacity > 0) {
    require_box(vertices != nullptr && levels_out != nullptr, "null argument");
    require_box((samples != nullptr) == (sample != nullptr),
                "samples_dev is given exactly when sample is");
  }
  std::vector<IsoBoxDev>& boxes = plan.boxes;
  boxes.resize(n_boxes);
  ByteRanges read_ranges, write_ranges;
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = field[b];
    const avr_box* fields[2] = {&first, sample != nullptr ? &sample[b] : &first};
    FieldView views[2];
    IsoBoxDev& dev = boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    int32_t paired;
    const bool cells = field_box_views(first, fields, 2, n_levels, views, &paired);
    dev.in = views[0].cells;
    dev.sample = views[1].cells;
    dev.jstride_in = views[0].jstride;
    dev.kstride_in = views[0].kstride;
    dev.jstride_sample = views[1].jstride;
    dev.kstride_sample = views[1].kstride;
    dev.level = first.level;
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
      append_byte_range(&read_ranges, views[0]);
      if (sample != nullptr) append_byte_range(&read_ranges, views[1]);
    }
  }
  fill_level_ratios(level_ratio, n_levels, levels.ratio);
  const std::vector<IndexRegion> regions = box_index_regions(box_index_lo, field, &boxes);
  require_levels_disjoint(boxes, regions);
  // what the call writes: the two counts always, the triangles' arrays with a capacity
  append_byte_range(&write_ranges, counts, 2 * sizeof(uint64_t));
  if (capacity > 0) {
    append_byte_range(&write_ranges, vertices, capacity * 9 * sizeof(double));
    append_byte_range(&write_ranges, levels_out, capacity);
    if (samples != nullptr) append_byte_range(&write_ranges, samples, capacity * 3 * sizeof(double));
  }
  require_no_shared_byte(&read_ranges, write_ranges,
                         "an output array overlaps an input box's cells");
  plan.base_begin.assign(1, 0u);
  plan.shell_begin.assign(1, uint64_t{0});
  uint64_t bases = 0;
  for (size_t b = 0; b < n_boxes; ++b) {
    // a box's cells are at most 2^28 (its span), its bases at most eight times as many
    if (boxes[b].nx > 0) {
      bases += (static_cast<uint64_t>(boxes[b].nx) + 1) * (static_cast<uint64_t>(boxes[b].ny) + 1) *
               (static_cast<uint64_t>(boxes[b].nz) + 1);
    }
    require_box(bases < (uint64_t{1} << 31), "scene has too many cube bases");
    boxes[b].base_begin = plan.base_begin.back();
    boxes[b].shell_begin = plan.shell_begin.back();
    plan.base_begin.push_back(static_cast<uint32_t>(bases));
    plan.shell_begin.push_back(plan.shell_begin.back() +
                               (boxes[b].nx > 0
                                    ? iso_shell_cells(boxes[b].nx, boxes[b].ny, boxes[b].nz)
                                    : uint64_t{0}));
  }
  plan.candidate_begin.assign(1, 0u);
  for (size_t b = 0; b < n_boxes; ++b) {
    if (boxes[b].nx > 0) {
      IndexRegion grown = regions[b];
      for (int d = 0; d < 3; ++d) {
        grown.lo[d] -= 1;
        grown.hi[d] += 1;
      }
      append_region_candidates(boxes, regions, b, grown, levels.ratio, boxes[b].level,
                               &plan.candidates);
    }
    plan.candidate_begin.push_back(static_cast<uint32_t>(plan.candidates.size()));
  }
  plan.args.n_boxes = static_cast<int32_t>(n_boxes);
  plan.args.n_levels = n_levels;
  plan.args.n_bases = plan.base_begin.back();
  plan.args.n_chunks = (plan.args.n_bases + kIsoChunk - 1) / kIsoChunk;
  plan.args.n_shell = plan.shell_begin.back();
  plan.args.value = value;
  plan.args.capacity = capacity;
  plan.scratch = iso_scratch(plan.args.n_shell, plan.args.n_chunks, sample != nullptr);
  return plan;
}

// ---- streamlines --------------------------------------------------------------------------
struct StreamPlan {
  std::vector<StreamBoxDev> boxes;
  IsoLevelsDev levels;
  // the locator (StreamLocatorDev): CSR over its blocks, per block the boxes of any level whose
  // cells, mapped to level 0, meet it, finest level first, then in scene order
  StreamLocatorDev locator;
  std::vector<uint32_t> block_begin;  // blocks + 1 ({0} for a scene without cells)
  std::vector<int32_t> block_boxes;
  StreamArgs args{};
  template <class Visit>
  void visit_tables(StreamArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->levels, &levels, 1);
    visit(&to->block_begin, block_begin.data(), block_begin.size());
    visit(&to->block_boxes, block_boxes.data(), block_boxes.size());
  }
};
// The blocks of the locator: the smallest power-of-two side that leaves at most `limit` blocks over
// the level-0 index range [lo, hi].
inline void size_stream_locator(const int64_t lo[3], const int64_t hi[3], int64_t limit,
                                StreamLocatorDev* locator) {
  for (int shift = 0; shift <= 31; ++shift) {
    int64_t n[3], blocks = 1;
    for (int d = 0; d < 3; ++d) {
      n[d] = ((hi[d] - lo[d]) >> shift) + 1;
      blocks *= n[d];  // n[d] <= 2^31 and limit <= 2^24: compared before the next factor
      if (blocks > limit) break;
    }
    if (blocks > limit) continue;
    for (int d = 0; d < 3; ++d) {
      locator->origin[d] = static_cast<int32_t>(lo[d]);
      locator->n[d] = static_cast<int32_t>(n[d]);
    }
    locator->shift = shift;
    return;
  }
}
// The locator of the streamlines and the rays (StreamLocatorDev): every box mapped to level 0, the
// blocks over their bounding box, the lists -- CSR over the blocks ({0} for a scene without cells),
// per block the boxes of any level whose cells, mapped to level 0, meet it, finest level first,
// then in scene order.  Returns whether the scene has cells, and with them *bound (may be null),
// the level-0 index bounding box the blocks cover.  Box: a device box with nx (0 without cells) and
// level; ratio[l]: level l -> l + 1; max_entries: the bound on the lists.
template <class Box>
inline bool build_level_locator(const std::vector<Box>& boxes,
                                const std::vector<IndexRegion>& regions, const int32_t* ratio,
                                int64_t max_entries, StreamLocatorDev* locator_out,
                                std::vector<uint32_t>* block_begin,
                                std::vector<int32_t>* block_boxes, IndexRegion* bound = nullptr) {
  std::memset(locator_out, 0, sizeof(*locator_out));
  block_begin->assign(1, 0u);
  block_boxes->clear();
  const size_t n_boxes = boxes.size();
  std::vector<IndexRegion> coarse(n_boxes);  // [b]: box b at level 0
  std::vector<size_t> order;                 // the boxes with cells, finest level first
  int64_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (size_t b = 0; b < n_boxes; ++b) {
    if (boxes[b].nx <= 0) continue;
    coarse[b] = regions[b];
    for (int m = boxes[b].level; m > 0; --m) {
      for (int d = 0; d < 3; ++d) {
        coarse[b].lo[d] = floor_div(coarse[b].lo[d], ratio[m - 1]);
        coarse[b].hi[d] = floor_div(coarse[b].hi[d], ratio[m - 1]);
      }
    }
    for (int d = 0; d < 3; ++d) {
      lo[d] = order.empty() ? coarse[b].lo[d] : std::min(lo[d], coarse[b].lo[d]);
      hi[d] = order.empty() ? coarse[b].hi[d] : std::max(hi[d], coarse[b].hi[d]);
    }
    order.push_back(b);
  }
  if (order.empty()) return false;
  std::stable_sort(order.begin(), order.end(),
                   [&](size_t x, size_t y) { return boxes[x].level > boxes[y].level; });
  // a few blocks per box keep the lists short; 2^24 blocks at the most
  const int64_t limit = std::min(kStreamMaxBlocks, 64 + 8 * static_cast<int64_t>(order.size()));
  size_stream_locator(lo, hi, limit, locator_out);
  const StreamLocatorDev& locator = *locator_out;
  const size_t blocks = static_cast<size_t>(locator.n[0]) * locator.n[1] * locator.n[2];
  auto block_range = [&](size_t b, int64_t first[3], int64_t last[3]) {
    for (int d = 0; d < 3; ++d) {
      first[d] = (coarse[b].lo[d] - lo[d]) >> locator.shift;
      last[d] = (coarse[b].hi[d] - lo[d]) >> locator.shift;
    }
  };
  // the lists' size from the boxes' extents, before anything of that size is made
  uint64_t entries = 0;
  for (size_t b : order) {
    int64_t first[3], last[3];
    block_range(b, first, last);
    entries += static_cast<uint64_t>(last[0] - first[0] + 1) *
               static_cast<uint64_t>(last[1] - first[1] + 1) *
               static_cast<uint64_t>(last[2] - first[2] + 1);  // at most 2^24 each
    require_box(entries < static_cast<uint64_t>(max_entries),
                "the locator's lists hold 2^28 entries or more");
  }
  auto for_blocks = [&](size_t b, auto&& visit) {
    int64_t first[3], last[3];
    block_range(b, first, last);
    for (int64_t z = first[2]; z <= last[2]; ++z) {
      for (int64_t y = first[1]; y <= last[1]; ++y) {
        for (int64_t x = first[0]; x <= last[0]; ++x) {
          visit(static_cast<size_t>((z * locator.n[1] + y) * locator.n[0] + x));
        }
      }
    }
  };
  std::vector<uint32_t> fill(blocks + 1, 0u);
  for (size_t b : order) for_blocks(b, [&](size_t block) { ++fill[block + 1]; });
  for (size_t block = 0; block < blocks; ++block) fill[block + 1] += fill[block];
  block_begin->assign(fill.begin(), fill.end());
  block_boxes->resize(static_cast<size_t>(fill[blocks]));
  for (size_t b : order) {
    for_blocks(b, [&](size_t block) { (*block_boxes)[fill[block]++] = static_cast<int32_t>(b); });
  }
  if (bound != nullptr) {
    for (int d = 0; d < 3; ++d) {
      bound->lo[d] = lo[d];
      bound->hi[d] = hi[d];
    }
  }
  return true;
}

// vx, vy, vz: the boxes of the three components; sample (may be null): those of the sample field.
// box_index_lo, level_ratio, level_cell_size and prob_lo as plan_isosurface takes them.  seeds,
// points, samples, counts and status are device arrays of n_seeds lines of max_steps + 1 points
// (free to be null with n_seeds == 0, samples null exactly without a sample scene).  The rules, in
// this order: step, direction, max_steps, the number of points, n_levels, null arrays, the cell
// sizes, prob_lo, samples_dev, the box rules (vx is the reference, so an incongruent vy, vz or
// sample scene is refused here), the ratios, the index ranges, boxes of one level apart in index
// space, no output byte and no seed shared with an input, the locator's size (max_entries: the
// bound on its lists, lowered by the plan's test only).
inline StreamPlan plan_streamlines(const avr_box* vx, const avr_box* vy, const avr_box* vz,
                                   const avr_box* sample, size_t n_boxes, uint64_t n_seeds,
                                   double step, int direction, uint64_t max_steps,
                                   const int32_t* box_index_lo, const int32_t* level_ratio,
                                   const double* level_cell_size, const double* prob_lo,
                                   int n_levels, const void* seeds, const void* points,
                                   const void* samples, const void* counts, const void* status,
                                   int64_t max_entries = kStreamMaxEntries) {
  require_box(std::isfinite(step) && step > 0.0 && step <= 1.0,
              "step must be finite and lie in (0, 1]");
  require_box(direction == 1 || direction == -1, "direction must be +1 or -1");
  require_box(max_steps <= kStreamMaxSteps, "max_steps must not exceed 2^20");
  // n_seeds < 2^32 first: the product then stays inside 64 bits
  require_box(n_seeds < (uint64_t{1} << 32) && n_seeds * (max_steps + 1) < (uint64_t{1} << 32),
              "n_seeds * (max_steps + 1) must stay below 2^32");
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  require_box(n_levels == 1 || level_ratio != nullptr, "null argument");
  require_box(n_boxes == 0 || box_index_lo != nullptr, "null argument");
  require_box(n_seeds == 0 || (seeds != nullptr && points != nullptr && counts != nullptr &&
                               status != nullptr), "null argument");
  StreamPlan plan;
  IsoLevelsDev& levels = plan.levels;
  fill_level_geometry(level_cell_size, prob_lo, n_levels, &levels);
  require_box((samples != nullptr) == (sample != nullptr),
              "samples_dev is given exactly when sample is");
  std::vector<StreamBoxDev>& boxes = plan.boxes;
  boxes.resize(n_boxes);
  ByteRanges read_ranges, write_ranges;
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = vx[b];
    const avr_box* fields[4] = {&first, &vy[b], &vz[b], sample != nullptr ? &sample[b] : &first};
    FieldView views[4];
    StreamBoxDev& dev = boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    int32_t paired;
    const bool cells = field_box_views(first, fields, 4, n_levels, views, &paired);
    for (int f = 0; f < 4; ++f) {
      dev.cells[f] = views[f].cells;
      dev.jstride[f] = views[f].jstride;
      dev.kstride[f] = views[f].kstride;
      if (cells && (f < 3 || sample != nullptr)) append_byte_range(&read_ranges, views[f]);
    }
    dev.level = first.level;
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
    }
  }
  fill_level_ratios(level_ratio, n_levels, levels.ratio);
  const std::vector<IndexRegion> regions = box_index_regions(box_index_lo, vx, &boxes);
  require_levels_disjoint(boxes, regions);
  if (n_seeds > 0) {
    const uint64_t slots = n_seeds * (max_steps + 1);
    append_byte_range(&write_ranges, seeds, n_seeds * 3 * sizeof(double));
    append_byte_range(&write_ranges, points, slots * 3 * sizeof(double));
    if (samples != nullptr) append_byte_range(&write_ranges, samples, slots * sizeof(double));
    append_byte_range(&write_ranges, counts, n_seeds * sizeof(uint32_t));
    append_byte_range(&write_ranges, status, n_seeds);
    require_no_shared_byte(&read_ranges, write_ranges,
                           "an output array or the seeds overlap an input box's cells");
  }
  build_level_locator(boxes, regions, levels.ratio, max_entries, &plan.locator, &plan.block_begin,
                      &plan.block_boxes);
  plan.args.locator = plan.locator;
  plan.args.n_levels = n_levels;
  plan.args.n_seeds = static_cast<uint32_t>(n_seeds);
  plan.args.max_steps = static_cast<uint32_t>(max_steps);
  plan.args.step = step;
  plan.args.direction = static_cast<double>(direction);
  return plan;
}

// ---- covering grids -----------------------------------------------------------------------
// ratio[from] * ... * ratio[to - 1] (from <= to), or 2^32 if it is more: from 2^31 on, every index
// but 0 and -1 times the factor lies outside [-2^30, 2^30) whatever the factor is, and every index
// of that range divided by it gives 0 or -1.
inline int64_t level_factor(const int32_t* ratio, int from, int to) {
  int64_t factor = 1;
  for (int l = from; l < to; ++l) {
    factor = std::min(factor * ratio[l], int64_t{1} << 32);  // below 2^63: a ratio is below 2^31
  }
  return factor;
}
// A region of level `from` (inside [-2^30, 2^30)) at level `to`: its descendants at a finer level,
// the cells that hold it at a coarser one.  Past a factor of 2^32 the finer region is not exact,
// but meets [-2^30, 2^30) in the same cells.
inline IndexRegion region_at_level(const IndexRegion& region, int from, int to,
                                   const int32_t* ratio) {
  IndexRegion out;
  const int64_t r = from <= to ? level_factor(ratio, from, to) : level_factor(ratio, to, from);
  for (int d = 0; d < 3; ++d) {
    out.lo[d] = from <= to ? region.lo[d] * r : floor_div(region.lo[d], r);
    out.hi[d] = from <= to ? region.hi[d] * r + (r - 1) : floor_div(region.hi[d], r);
  }
  return out;
}

// The candidate lists of the tiles of `output`, a region of level `level` cut into the tiles of
// avr_cell_tiles.h (numbered as cell_tile_of numbers a box's): CSR over the tiles, per tile every
// box, in scene order, whose cells meet the tile's index slab at the box's own level -- the slab
// mapped down by floor division for a coarser box and multiplied up for a finer one, which is to
// say that the box, mapped to `level` the other way, meets the tile.  A sibling of
// append_region_candidates, which serves "the surroundings of box b" and looks one level finer at
// the most; this one serves a region that belongs to no box and looks at every level.  Box: a
// device box with nx (0 without cells) and level; ratio[l]: level l -> l + 1.
template <class Box>
inline void tile_candidate_lists(const std::vector<Box>& boxes,
                                 const std::vector<IndexRegion>& regions, const int32_t* ratio,
                                 int level, const IndexRegion& output,
                                 std::vector<uint32_t>* candidate_begin,
                                 std::vector<int32_t>* candidates) {
  const int nx = static_cast<int>(output.hi[0] - output.lo[0] + 1);
  const int ny = static_cast<int>(output.hi[1] - output.lo[1] + 1);
  const int nz = static_cast<int>(output.hi[2] - output.lo[2] + 1);
  const size_t tiles = cell_tiles(nx, ny, nz);
  const CellTileShape shape = cell_tile_shape(nx, ny);
  const int64_t edge[3] = {kClassifyChunk, kBrickY, kBrickZ};
  // the tiles box c meets: [first, last] per axis; false if it meets none
  auto tile_range = [&](size_t c, int64_t first[3], int64_t last[3]) {
    if (boxes[c].nx <= 0) return false;
    const IndexRegion at = region_at_level(regions[c], boxes[c].level, level, ratio);
    if (!regions_meet(at, output)) return false;
    for (int d = 0; d < 3; ++d) {
      first[d] = (std::max(at.lo[d], output.lo[d]) - output.lo[d]) / edge[d];
      last[d] = (std::min(at.hi[d], output.hi[d]) - output.lo[d]) / edge[d];
    }
    return true;
  };
  // the lists' size from the boxes' extents, before anything of that size is made
  uint64_t entries = 0;
  for (size_t c = 0; c < boxes.size(); ++c) {
    int64_t first[3], last[3];
    if (!tile_range(c, first, last)) continue;
    entries += static_cast<uint64_t>(last[0] - first[0] + 1) *
               static_cast<uint64_t>(last[1] - first[1] + 1) *
               static_cast<uint64_t>(last[2] - first[2] + 1);  // at most 2^31 tiles each
    require_box(entries < (uint64_t{1} << 31), "the tiles' candidate lists hold 2^31 entries or more");
  }
  auto for_tiles = [&](size_t c, auto&& visit) {
    int64_t first[3], last[3];
    if (!tile_range(c, first, last)) return;
    for (int64_t bk = first[2]; bk <= last[2]; ++bk) {
      for (int64_t bj = first[1]; bj <= last[1]; ++bj) {
        for (int64_t chunk = first[0]; chunk <= last[0]; ++chunk) {
          visit(static_cast<size_t>((bk * shape.bricks_y + bj) * shape.chunks + chunk));
        }
      }
    }
  };
  std::vector<uint32_t> fill(tiles + 1, 0u);
  for (size_t c = 0; c < boxes.size(); ++c) for_tiles(c, [&](size_t tile) { ++fill[tile + 1]; });
  for (size_t tile = 0; tile < tiles; ++tile) fill[tile + 1] += fill[tile];
  candidate_begin->assign(fill.begin(), fill.end());
  candidates->resize(static_cast<size_t>(fill[tiles]));
  for (size_t c = 0; c < boxes.size(); ++c) {
    for_tiles(c, [&](size_t tile) { (*candidates)[fill[tile]++] = static_cast<int32_t>(c); });
  }
}

struct CoveringGridPlan {
  std::vector<CoverBoxDev> boxes;
  CoverLevelsDev levels;   // the ratios, and R_m and w_m of the loaded levels finer than `level`
  int32_t finest = -1;     // the finest level that has a box with cells (-1: none has)
  // CSR over the output's tiles (tile_candidate_lists): candidate_begin has tiles + 1 entries
  std::vector<uint32_t> candidate_begin;
  std::vector<int32_t> candidates;  // empty when no box meets the region
  CoverArgs args{};
  template <class Visit>
  void visit_tables(CoverArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->levels, &levels, 1);
    visit(&to->candidate_begin, candidate_begin.data(), candidate_begin.size());
    visit(&to->candidates, candidates.data(), candidates.size());
  }
};
// The field resampled to the cells [lo, lo + dims) of level `level` ("Covering
// grid").  box_index_lo and level_ratio as plan_gradient takes them; n_levels counts the levels up
// to the finer of `level` and the finest loaded one; `fill` is what a cell no box covers gets (any
// value, NaN included).  values, coverage and cell_level are device
// arrays of dims[0] * dims[1] * dims[2] entries (f64, f64, i8); coverage and cell_level may be
// null, values has been checked by the entry point.  The rules, in this order: n_levels, level,
// null arrays, the box rules, the ratios, the index ranges, boxes of one level apart in index
// space, dims, the region inside [-2^30, 2^30) at `level` and at the finest loaded level, fewer
// than 2^31 cells, no output byte shared with an input, the candidate lists' size.
inline CoveringGridPlan plan_covering_grid(const avr_box* field, size_t n_boxes, int level,
                                           const int32_t lo[3], const int32_t dims[3],
                                           const int32_t* box_index_lo,
                                           const int32_t* level_ratio, int n_levels, double fill,
                                           const void* values, const void* coverage,
                                           const void* cell_level) {
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  require_box(level >= 0 && level < n_levels, "level must lie in [0, n_levels)");
  require_box(n_levels == 1 || level_ratio != nullptr, "null argument");
  require_box(n_boxes == 0 || box_index_lo != nullptr, "null argument");
  CoveringGridPlan plan;
  std::vector<CoverBoxDev>& boxes = plan.boxes;
  boxes.resize(n_boxes);
  ByteRanges read_ranges, write_ranges;
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = field[b];
    const avr_box* fields[1] = {&first};
    FieldView view;
    CoverBoxDev& dev = boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    int32_t paired;
    const bool cells = field_box_views(first, fields, 1, n_levels, &view, &paired);
    dev.cells = view.cells;
    dev.jstride = view.jstride;
    dev.kstride = view.kstride;
    dev.level = first.level;
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
      append_byte_range(&read_ranges, view);
      plan.finest = std::max(plan.finest, dev.level);
    }
  }
  CoverLevelsDev& levels = plan.levels;
  std::memset(&levels, 0, sizeof(levels));
  fill_level_ratios(level_ratio, n_levels, levels.ratio);
  const std::vector<IndexRegion> regions = box_index_regions(box_index_lo, field, &boxes);
  require_levels_disjoint(boxes, regions);
  require_box(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, "dims must be at least 1");
  const int finest = std::max(plan.finest, level);
  const int64_t limit = int64_t{1} << 30, up = level_factor(levels.ratio, level, finest);
  IndexRegion output;
  for (int d = 0; d < 3; ++d) {
    output.lo[d] = lo[d];
    output.hi[d] = static_cast<int64_t>(lo[d]) + dims[d] - 1;
    require_box(output.lo[d] >= -limit && output.hi[d] < limit &&
                    output.lo[d] * up >= -limit && (output.hi[d] + 1) * up <= limit,
                "the region leaves [-2^30, 2^30) at its level or at the finest loaded one");
  }
  // dims are at most 2^31 each here: two factors first
  const uint64_t plane = static_cast<uint64_t>(dims[0]) * static_cast<uint64_t>(dims[1]);
  require_box(plane < (uint64_t{1} << 31) &&
                  plane * static_cast<uint64_t>(dims[2]) < (uint64_t{1} << 31),
              "the region has 2^31 cells or more");
  const uint64_t n_cells = plane * static_cast<uint64_t>(dims[2]);
  append_byte_range(&write_ranges, values, n_cells * sizeof(double));
  if (coverage != nullptr) append_byte_range(&write_ranges, coverage, n_cells * sizeof(double));
  if (cell_level != nullptr) append_byte_range(&write_ranges, cell_level, n_cells);
  require_no_shared_byte(&read_ranges, write_ranges,
                         "an output array overlaps an input box's cells");
  // R_m and w_m: the region rule keeps R_m of a loaded level at 2^30 or less, R_m^3 inside 2^90
  for (int m = 0; m < kFieldMaxLevels; ++m) levels.refine[m] = 1;
  for (int m = level + 1; m <= plan.finest; ++m) {
    const int64_t r = level_factor(levels.ratio, level, m);
    levels.refine[m] = static_cast<int32_t>(r);
    const unsigned __int128 cube = static_cast<unsigned __int128>(r) * static_cast<uint64_t>(r) *
                                   static_cast<uint64_t>(r);
    levels.weight[m] = 1.0 / static_cast<double>(cube);
  }
  tile_candidate_lists(boxes, regions, levels.ratio, level, output, &plan.candidate_begin,
                       &plan.candidates);
  plan.args.level = level;
  plan.args.finest = plan.finest;
  for (int d = 0; d < 3; ++d) plan.args.lo[d] = lo[d];
  plan.args.nx = dims[0];
  plan.args.ny = dims[1];
  plan.args.nz = dims[2];
  plan.args.n_tiles = static_cast<uint32_t>(plan.candidate_begin.size() - 1);
  plan.args.fill = fill;
  return plan;
}

// ---- grid fields --------------------------------------------------------------------------
struct GridFieldPlan {
  std::vector<GridBoxDev> boxes;
  std::vector<uint32_t> tile_begin;
  GridLevelsDev levels;    // per level R, f64(2 R) and whether it is finer or coarser than `level`
  int32_t finest = -1;     // the finest level that has a box with cells (-1: none has)
  GridFieldArgs args{};
  template <class Visit>
  void visit_tables(GridFieldArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->tile_begin, tile_begin.data(), tile_begin.size());
    visit(&to->levels, &levels, 1);
  }
};
// The grid of the cells [lo, lo + dims) of level `level` written onto the cells of the boxes `out`
// ("Grid fields").  box_index_lo, level_ratio and n_levels as plan_covering_grid takes
// them; `fill` is what a cell outside the region gets (any bits).  grid: a device array of dims[0]
// * dims[1] * dims[2] f64; totals: a device array of two 64-bit counts; both have been checked by
// the entry point.  The rules, in this order: n_levels, level, null arrays, the box rules (the
// output is the reference), the ratios, the index ranges, dims, the region inside [-2^30, 2^30) at
// `level` and at the finest box level, fewer than 2^31 cells, interpolation and periodic, no byte
// of the grid or the totals shared with an output box's cells.
inline GridFieldPlan plan_grid_field(const avr_box* out, size_t n_boxes, int level,
                                     const int32_t lo[3], const int32_t dims[3],
                                     const int32_t* box_index_lo, const int32_t* level_ratio,
                                     int n_levels, int interpolation, int periodic, double fill,
                                     const void* grid, const void* totals) {
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  require_box(level >= 0 && level < n_levels, "level must lie in [0, n_levels)");
  require_box(n_levels == 1 || level_ratio != nullptr, "null argument");
  require_box(n_boxes == 0 || box_index_lo != nullptr, "null argument");
  GridFieldPlan plan;
  std::vector<GridBoxDev>& boxes = plan.boxes;
  boxes.resize(n_boxes);
  plan.tile_begin.assign(1, 0u);
  ByteRanges read_ranges, write_ranges;  // of the grid and the totals, and of the output's boxes
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = out[b];
    const avr_box* fields[1] = {&first};
    FieldView view;
    GridBoxDev& dev = boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    const bool cells = field_box_views(first, fields, 1, n_levels, &view, &dev.paired);
    dev.out = const_cast<double*>(view.cells);
    dev.jstride = view.jstride;
    dev.kstride = view.kstride;
    dev.level = first.level;
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
      append_byte_range(&write_ranges, view);
      plan.finest = std::max(plan.finest, dev.level);
    }
    append_tiles(&plan.tile_begin, cells ? cell_tiles(dev.nx, dev.ny, dev.nz) : 0u);
  }
  int32_t ratio[kFieldMaxLevels];
  fill_level_ratios(level_ratio, n_levels, ratio);
  box_index_regions(box_index_lo, out, &boxes);
  require_box(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, "dims must be at least 1");
  const int finest = std::max(plan.finest, level);
  const int64_t limit = int64_t{1} << 30, up = level_factor(ratio, level, finest);
  for (int d = 0; d < 3; ++d) {
    const int64_t first = lo[d], last = first + dims[d] - 1;
    require_box(first >= -limit && last < limit && first * up >= -limit && (last + 1) * up <= limit,
                "the region leaves [-2^30, 2^30) at its level or at the finest box level");
  }
  // dims are at most 2^31 each here: two factors first
  const uint64_t plane = static_cast<uint64_t>(dims[0]) * static_cast<uint64_t>(dims[1]);
  require_box(plane < (uint64_t{1} << 31) &&
                  plane * static_cast<uint64_t>(dims[2]) < (uint64_t{1} << 31),
              "the region has 2^31 cells or more");
  require_box(interpolation == 0 || interpolation == 1,
              "interpolation must be 0 (constant) or 1 (linear)");
  require_box(periodic == 0 || periodic == 1, "periodic must be 0 or 1");
  const uint64_t n_cells = plane * static_cast<uint64_t>(dims[2]);
  append_byte_range(&read_ranges, grid, n_cells * sizeof(double));
  append_byte_range(&read_ranges, totals, 2 * sizeof(uint64_t));
  require_no_shared_byte(&read_ranges, write_ranges,
                         "the grid or the totals overlap an output box's cells");
  // R of a finer level with cells is at most 2^30 by the region rule; of a coarser one it is held
  // at 2^32, where a cell's footprint meets [-2^30, 2^30) as it does at the true factor
  GridLevelsDev& levels = plan.levels;
  std::memset(&levels, 0, sizeof(levels));
  for (int l = 0; l < kFieldMaxLevels; ++l) {
    const int64_t r = l < n_levels ? (l < level ? level_factor(ratio, l, level)
                                                : level_factor(ratio, level, l))
                                   : 1;
    levels.refine[l] = r;
    levels.two_r[l] = 2.0 * static_cast<double>(r);
    levels.direction[l] = l >= n_levels || l == level ? kGridSame
                                                      : (l > level ? kGridFiner : kGridCoarser);
  }
  plan.args.n_boxes = static_cast<int32_t>(n_boxes);
  plan.args.n_tiles = plan.tile_begin.back();
  plan.args.level = level;
  for (int d = 0; d < 3; ++d) plan.args.lo[d] = lo[d];
  plan.args.nx = dims[0];
  plan.args.ny = dims[1];
  plan.args.nz = dims[2];
  plan.args.interpolation = interpolation;
  plan.args.periodic = periodic;
  plan.args.fill = fill;
  return plan;
}

// ---- rays -----------------------------------------------------------------------------------
struct RayPlan {
  std::vector<CoverBoxDev> boxes;
  IsoLevelsDev levels;
  // the streamlines' locator (build_level_locator) and the level-0 box [Blo, Bhi] it covers
  StreamLocatorDev locator;
  std::vector<uint32_t> block_begin;  // blocks + 1 ({0} for a scene without cells)
  std::vector<int32_t> block_boxes;
  int32_t bound_lo[3] = {0, 0, 0}, bound_hi[3] = {-1, -1, -1};
  RayArgs args{};
  template <class Visit>
  void visit_tables(RayArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit_walk_tables(to, visit);
  }
  // ... but for the boxes: what the per-ray sums stage behind their own
  template <class Visit>
  void visit_walk_tables(RayArgs* to, Visit&& visit) const {
    visit(&to->levels, &levels, 1);
    visit(&to->block_begin, block_begin.data(), block_begin.size());
    visit(&to->block_boxes, block_boxes.data(), block_boxes.size());
  }
};
// The leaf cells that n_rays segments start[s] -> end[s] cross ("Rays").  box_index_lo,
// level_ratio, level_cell_size and prob_lo as plan_isosurface takes them.  start, end: device
// arrays f64 [n_rays][3].  The count pass (offsets == nullptr) writes counts u32 [n_rays], status
// u8 [n_rays] and span f64 [n_rays][2]; the emit pass reads offsets i64 [n_rays + 1] and writes
// t0, t1, value f64 [n_segments], level i8 [n_segments] (free to be null with n_segments == 0),
// integral and covered f64 [n_rays]; the arrays of the other pass are not looked at.  All of them
// are free to be null with n_rays == 0.  The rules, in this order: max_trips, n_rays, n_segments,
// n_levels, null arrays (the hierarchy's, level_cell_size and prob_lo among them, then the rays'
// and the outputs'), the cell sizes, prob_lo, the box rules, the ratios, the index ranges,
// boxes of one level apart in index space, no output byte and no byte of start, end or offsets
// shared with an input, the locator's size (max_entries: the bound on its lists, lowered by the
// plan's test only), the bounding box refined to the finest level inside [-2^30, 2^30].
// What plan_rays and plan_ray_sums share: the rules above in their order, the tables and the
// locator.  arrays_present: whether the call's own arrays pass the null rule; arrays: the byte
// ranges of start, end and what the call writes (looked at only once n_rays > 0 and every size
// rule has passed).  weight (may be null): the boxes of a second scene read at the same cells,
// n_weight_boxes of them; its rules come after the field's box rules -- as many boxes as the
// field has and, box by box, the field's level, dims and corner (from which the caller recovered
// the one index both share), then the view rule -- and its cells count as inputs in the
// shared-byte rule.  Such a scene is a companion: its boxes, the message of its congruence rule
// and where its table goes; several are taken in their order.
struct RayCompanion {
  const avr_box* boxes;
  size_t n_boxes;
  const char* differ;
  std::vector<CoverBoxDev>* table;
};
inline RayPlan plan_ray_walk(const avr_box* field, size_t n_boxes, const RayCompanion* companions,
                             size_t n_companions, uint64_t n_rays, uint64_t max_trips,
                             uint64_t n_segments, const int32_t* box_index_lo,
                             const int32_t* level_ratio, const double* level_cell_size,
                             const double* prob_lo, int n_levels, bool arrays_present,
                             const ByteRanges& arrays, int64_t max_entries) {
  require_box(max_trips >= 1 && max_trips <= kRayMaxTrips, "max_trips must lie in [1, 2^30]");
  require_box(n_rays < (uint64_t{1} << 32), "n_rays must stay below 2^32");
  require_box(n_segments <= kRayMaxSegments, "n_segments must not exceed 2^40");
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  require_box(level_cell_size != nullptr && prob_lo != nullptr, "null argument");
  require_box(n_levels == 1 || level_ratio != nullptr, "null argument");
  require_box(n_boxes == 0 || box_index_lo != nullptr, "null argument");
  require_box(n_rays == 0 || arrays_present, "null argument");
  RayPlan plan;
  IsoLevelsDev& levels = plan.levels;
  fill_level_geometry(level_cell_size, prob_lo, n_levels, &levels);
  std::vector<CoverBoxDev>& boxes = plan.boxes;
  boxes.resize(n_boxes);
  ByteRanges read_ranges;
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = field[b];
    const avr_box* fields[1] = {&first};
    FieldView view;
    CoverBoxDev& dev = boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    int32_t paired;
    const bool cells = field_box_views(first, fields, 1, n_levels, &view, &paired);
    dev.cells = view.cells;
    dev.jstride = view.jstride;
    dev.kstride = view.kstride;
    dev.level = first.level;
    if (cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
      append_byte_range(&read_ranges, view);
    }
  }
  for (size_t c = 0; c < n_companions; ++c) {
    const RayCompanion& companion = companions[c];
    const char* differ = companion.differ;
    require_box(companion.n_boxes == n_boxes, differ);
    companion.table->resize(n_boxes);
    for (size_t b = 0; b < n_boxes; ++b) {
      const avr_box& first = field[b];
      const avr_box& other = companion.boxes[b];
      CoverBoxDev& dev = (*companion.table)[b];
      std::memset(&dev, 0, sizeof(dev));
      require_box(other.level == first.level && other.dims[0] == first.dims[0] &&
                      other.dims[1] == first.dims[1] && other.dims[2] == first.dims[2] &&
                      other.min_corner[0] == first.min_corner[0] &&
                      other.min_corner[1] == first.min_corner[1] &&
                      other.min_corner[2] == first.min_corner[2], differ);
      dev.level = other.level;
      if (box_is_empty(other)) continue;
      const FieldView view = field_view(other);
      dev.cells = view.cells;
      dev.jstride = view.jstride;
      dev.kstride = view.kstride;
      dev.nx = other.dims[0];
      dev.ny = other.dims[1];
      dev.nz = other.dims[2];
      append_byte_range(&read_ranges, view);
    }
  }
  fill_level_ratios(level_ratio, n_levels, levels.ratio);
  const std::vector<IndexRegion> regions = box_index_regions(box_index_lo, field, &boxes);
  require_levels_disjoint(boxes, regions);
  for (size_t c = 0; c < n_companions; ++c) {
    for (size_t b = 0; b < n_boxes; ++b) {
      for (int d = 0; d < 3; ++d) (*companions[c].table)[b].lo[d] = boxes[b].lo[d];
    }
  }
  if (n_rays > 0) {
    require_no_shared_byte(&read_ranges, arrays,
                           "an output array or the rays overlap an input box's cells");
  }
  IndexRegion bound;
  if (build_level_locator(boxes, regions, levels.ratio, max_entries, &plan.locator,
                          &plan.block_begin, &plan.block_boxes, &bound)) {
    // an absent cell has the finest level's geometry wherever it lies in [Blo, Bhi]: the kernel's
    // 32-bit indices, one step past a cell included, and f64(index) stay exact
    const int64_t limit = int64_t{1} << 30, up = level_factor(levels.ratio, 0, n_levels - 1);
    for (int d = 0; d < 3; ++d) {
      require_box(bound.lo[d] * up >= -limit && (bound.hi[d] + 1) * up <= limit,
                  "the scene's bounding box leaves [-2^30, 2^30] at the finest level");
      plan.bound_lo[d] = static_cast<int32_t>(bound.lo[d]);
      plan.bound_hi[d] = static_cast<int32_t>(bound.hi[d]);
    }
  }
  plan.args.locator = plan.locator;
  for (int d = 0; d < 3; ++d) {
    plan.args.bound_lo[d] = plan.bound_lo[d];
    plan.args.bound_hi[d] = plan.bound_hi[d];
  }
  plan.args.n_levels = n_levels;
  plan.args.n_rays = static_cast<uint32_t>(n_rays);
  plan.args.max_trips = static_cast<uint32_t>(max_trips);
  plan.args.n_segments = n_segments;
  return plan;
}

inline RayPlan plan_rays(const avr_box* field, size_t n_boxes, uint64_t n_rays, uint64_t max_trips,
                         const int32_t* box_index_lo, const int32_t* level_ratio,
                         const double* level_cell_size, const double* prob_lo, int n_levels,
                         const void* start, const void* end, const void* offsets,
                         uint64_t n_segments, const void* counts, const void* status,
                         const void* span, const void* t0, const void* t1, const void* level,
                         const void* value, const void* integral, const void* covered,
                         int64_t max_entries = kStreamMaxEntries) {
  const bool emit = offsets != nullptr;
  bool present = start != nullptr && end != nullptr;
  ByteRanges arrays;
  if (n_rays > 0) {
    append_byte_range(&arrays, start, n_rays * 3 * sizeof(double));
    append_byte_range(&arrays, end, n_rays * 3 * sizeof(double));
    if (emit) {
      present = present && integral != nullptr && covered != nullptr &&
                (n_segments == 0 ||
                 (t0 != nullptr && t1 != nullptr && level != nullptr && value != nullptr));
      append_byte_range(&arrays, offsets, (n_rays + 1) * sizeof(int64_t));
      if (n_segments > 0) {
        append_byte_range(&arrays, t0, n_segments * sizeof(double));
        append_byte_range(&arrays, t1, n_segments * sizeof(double));
        append_byte_range(&arrays, level, n_segments);
        append_byte_range(&arrays, value, n_segments * sizeof(double));
      }
      append_byte_range(&arrays, integral, n_rays * sizeof(double));
      append_byte_range(&arrays, covered, n_rays * sizeof(double));
    } else {
      present = present && counts != nullptr && status != nullptr && span != nullptr;
      append_byte_range(&arrays, counts, n_rays * sizeof(uint32_t));
      append_byte_range(&arrays, status, n_rays);
      append_byte_range(&arrays, span, n_rays * 2 * sizeof(double));
    }
  }
  RayPlan plan = plan_ray_walk(field, n_boxes, nullptr, 0, n_rays, max_trips, n_segments,
                               box_index_lo, level_ratio, level_cell_size, prob_lo, n_levels,
                               present, arrays, max_entries);
  if (!emit) plan.args.n_segments = 0;  // the count pass has no packed arrays
  return plan;
}

// ---- per-ray sums ("Off-axis projection") --------------------------------------
struct RaySumsPlan {
  RayPlan walk;                            // plan_rays' tables, entry for entry; its args launch
  std::vector<CoverBoxDev> weight_boxes;   // empty without a weight scene
  bool weighted = false;
  template <class Visit>
  void visit_tables(RayArgs* to, Visit&& visit) const {
    visit(&to->boxes, walk.boxes.data(), walk.boxes.size());
    if (weighted) visit(&to->weight_boxes, weight_boxes.data(), weight_boxes.size());
    walk.visit_walk_tables(to, visit);
  }
};
// The sums of the one walk, per ray: plan_rays' rules in plan_rays' order with the same messages
// (there is no n_segments), the same locator, and the weight rules (plan_ray_walk) after the
// field's box rules.  weight (may be null): the weight scene's n_weight_boxes boxes; weight_out is
// null exactly without it ("null argument" otherwise).  counts u32 [n_rays], status u8 [n_rays],
// span f64 [n_rays][2], integral, weight_out, counted and covered f64 [n_rays]: device arrays,
// free to be null with n_rays == 0; none of them, nor start or end, may share a byte with a cell
// of either scene.
inline RaySumsPlan plan_ray_sums(const avr_box* field, size_t n_boxes, const avr_box* weight,
                                 size_t n_weight_boxes, uint64_t n_rays, uint64_t max_trips,
                                 const int32_t* box_index_lo, const int32_t* level_ratio,
                                 const double* level_cell_size, const double* prob_lo, int n_levels,
                                 const void* start, const void* end, const void* counts,
                                 const void* status, const void* span, const void* integral,
                                 const void* weight_out, const void* counted, const void* covered,
                                 int64_t max_entries = kStreamMaxEntries) {
  const bool present = start != nullptr && end != nullptr && counts != nullptr &&
                       status != nullptr && span != nullptr && integral != nullptr &&
                       counted != nullptr && covered != nullptr &&
                       (weight != nullptr) == (weight_out != nullptr);
  ByteRanges arrays;
  if (n_rays > 0) {
    append_byte_range(&arrays, start, n_rays * 3 * sizeof(double));
    append_byte_range(&arrays, end, n_rays * 3 * sizeof(double));
    append_byte_range(&arrays, counts, n_rays * sizeof(uint32_t));
    append_byte_range(&arrays, status, n_rays);
    append_byte_range(&arrays, span, n_rays * 2 * sizeof(double));
    append_byte_range(&arrays, integral, n_rays * sizeof(double));
    if (weight_out != nullptr) append_byte_range(&arrays, weight_out, n_rays * sizeof(double));
    append_byte_range(&arrays, counted, n_rays * sizeof(double));
    append_byte_range(&arrays, covered, n_rays * sizeof(double));
  }
  RaySumsPlan plan;
  plan.weighted = weight != nullptr;
  const RayCompanion companion = {weight, n_weight_boxes,
                                  "the weight scene's boxes differ from the field's",
                                  &plan.weight_boxes};
  plan.walk = plan_ray_walk(field, n_boxes, &companion, plan.weighted ? 1 : 0, n_rays, max_trips,
                            0, box_index_lo, level_ratio, level_cell_size, prob_lo, n_levels,
                            present, arrays, max_entries);
  return plan;
}

// ---- ray transfer ("Ray transfer") -----------------------------------------------
struct RayTransferPlan {
  RayPlan walk;                            // plan_rays' tables, entry for entry; its args launch
  std::vector<CoverBoxDev> opacity_boxes;
  std::vector<CoverBoxDev> bin_boxes;      // empty for grey
  std::vector<CoverBoxDev> width_boxes;    // empty for grey and sharp
  std::vector<double> edges;               // n_channels + 1 as given; empty for grey
  std::vector<double> rdv;                 // [c]: 1.0 / (edges[c + 1] - edges[c])
  int form = kTransferGrey;
  int32_t n_channels = 1;                  // 1 for grey
  int32_t chunk = 1;                       // channels of a chunk: min(the size asked for, n_channels)
  uint32_t n_chunks = 1;                   // the grid's y extent; the last chunk may be partial
  size_t lds_bytes = 0;                    // of a workgroup: the chunk's tables and accumulators
  template <class Visit>
  void visit_tables(RayArgs* to, Visit&& visit) const {
    visit(&to->boxes, walk.boxes.data(), walk.boxes.size());
    visit(&to->transfer.opacity_boxes, opacity_boxes.data(), opacity_boxes.size());
    if (form != kTransferGrey) {
      visit(&to->transfer.bin_boxes, bin_boxes.data(), bin_boxes.size());
      visit(&to->transfer.edges, edges.data(), edges.size());
      visit(&to->transfer.rdv, rdv.data(), rdv.size());
    }
    if (form == kTransferBroadened) {
      visit(&to->transfer.width_boxes, width_boxes.data(), width_boxes.size());
    }
    walk.visit_walk_tables(to, visit);
  }
};
// Emission and absorption along the one walk.  source, opacity, bin (may be null: grey) and width
// (may be null: sharp): the four scenes' boxes; edges: n_channels + 1 of them, given exactly with
// bin.  chunk: the channels of a chunk as asked for (the context's setting).  counts u32 [n_rays],
// status u8 [n_rays], span f64 [n_rays][2], intensity and tau f64 [n_channels][n_rays], outside f64
// [2][n_rays] (exactly with bin), counted and covered f64 [n_rays]: device arrays, free to be null
// with n_rays == 0.  The rules, in this order.  Its own: no opacity scene, a width without a bin
// scene, a bin scene without edges or edges without one, and -- while there are rays -- an
// `outside` without a bin scene or a bin scene without one ("null argument"); with a bin scene
// n_channels in [1, 1024] and finite, strictly increasing edges, without one n_channels == 1;
// n_channels x n_rays below 2^31; the chunk in [1, 32].  Then plan_rays' in plan_rays' order with
// the same messages (there is no n_segments), the three scenes' congruence -- opacity, bin, width:
// the weight scene's rules of plan_ray_sums, reworded per scene -- after the source's box rules,
// and no byte of an output, of start or of end shared with a cell of any of the four scenes.
inline RayTransferPlan plan_ray_transfer(
    const avr_box* source, size_t n_boxes, const avr_box* opacity, size_t n_opacity_boxes,
    const avr_box* bin, size_t n_bin_boxes, const avr_box* width, size_t n_width_boxes,
    uint64_t n_rays, uint64_t max_trips, const int32_t* box_index_lo, const int32_t* level_ratio,
    const double* level_cell_size, const double* prob_lo, int n_levels, const double* edges,
    int n_channels, int chunk, const void* start, const void* end, const void* counts,
    const void* status, const void* span, const void* intensity, const void* tau,
    const void* outside, const void* counted, const void* covered,
    int64_t max_entries = kStreamMaxEntries) {
  require_box(opacity != nullptr, "null argument");
  require_box(width == nullptr || bin != nullptr, "null argument");
  require_box((bin != nullptr) == (edges != nullptr), "null argument");
  require_box(n_rays == 0 || (bin != nullptr) == (outside != nullptr), "null argument");
  if (bin != nullptr) {
    require_box(n_channels >= 1 && n_channels <= kTransferMaxChannels,
                "n_channels must lie in [1, 1024]");
    for (int i = 0; i <= n_channels; ++i) {
      require_box(std::isfinite(edges[i]), "edges must be finite");
      require_box(i == 0 || edges[i - 1] < edges[i], "edges must be strictly increasing");
    }
  } else {
    require_box(n_channels == 1, "n_channels must be 1 without a bin scene");
  }
  require_box(n_rays < (uint64_t{1} << 31) &&
                  static_cast<uint64_t>(n_channels) * n_rays < (uint64_t{1} << 31),
              "the channels of all rays are 2^31 entries or more");
  require_box(chunk >= 1 && chunk <= kTransferMaxChunk, "the chunk must lie in [1, 32]");
  const bool present = start != nullptr && end != nullptr && counts != nullptr &&
                       status != nullptr && span != nullptr && intensity != nullptr &&
                       tau != nullptr && counted != nullptr && covered != nullptr;
  const uint64_t channels = static_cast<uint64_t>(n_channels);
  ByteRanges arrays;
  if (n_rays > 0) {
    append_byte_range(&arrays, start, n_rays * 3 * sizeof(double));
    append_byte_range(&arrays, end, n_rays * 3 * sizeof(double));
    append_byte_range(&arrays, counts, n_rays * sizeof(uint32_t));
    append_byte_range(&arrays, status, n_rays);
    append_byte_range(&arrays, span, n_rays * 2 * sizeof(double));
    append_byte_range(&arrays, intensity, channels * n_rays * sizeof(double));
    append_byte_range(&arrays, tau, channels * n_rays * sizeof(double));
    if (outside != nullptr) append_byte_range(&arrays, outside, n_rays * 2 * sizeof(double));
    append_byte_range(&arrays, counted, n_rays * sizeof(double));
    append_byte_range(&arrays, covered, n_rays * sizeof(double));
  }
  RayTransferPlan plan;
  plan.form = bin == nullptr ? kTransferGrey
                             : (width == nullptr ? kTransferSharp : kTransferBroadened);
  const RayCompanion companions[3] = {
      {opacity, n_opacity_boxes, "the opacity scene's boxes differ from the source's",
       &plan.opacity_boxes},
      {bin, n_bin_boxes, "the bin scene's boxes differ from the source's", &plan.bin_boxes},
      {width, n_width_boxes, "the width scene's boxes differ from the source's",
       &plan.width_boxes}};
  plan.walk = plan_ray_walk(source, n_boxes, companions, static_cast<size_t>(1 + plan.form), n_rays,
                            max_trips, 0, box_index_lo, level_ratio, level_cell_size, prob_lo,
                            n_levels, present, arrays, max_entries);
  plan.n_channels = n_channels;
  plan.chunk = std::min(chunk, n_channels);
  plan.n_chunks = static_cast<uint32_t>((n_channels + plan.chunk - 1) / plan.chunk);
  plan.lds_bytes = ray_transfer_lds_bytes(plan.form, plan.chunk);
  RayTransferPart& t = plan.walk.args.transfer;
  t.n_channels = n_channels;
  t.chunk = plan.chunk;
  if (plan.form != kTransferGrey) {
    plan.edges.assign(edges, edges + n_channels + 1);
    plan.rdv.resize(static_cast<size_t>(n_channels));
    for (int c = 0; c < n_channels; ++c) {
      const double dv = edges[c + 1] - edges[c];
      plan.rdv[static_cast<size_t>(c)] = 1.0 / dv;
    }
    t.lo = edges[0];
    t.hi = edges[n_channels];
  }
  return plan;
}

// ---- power spectra ------------------------------------------------------------------------
// The twiddle table of a length-n transform ("Power spectrum"): n / 2 pairs W[m] =
// (cos t, sin t) with t = -(2.0 pi m) / n evaluated in that order in f64, by the C library's cos
// and sin.  n: a power of two in [1, 1024]; n == 1 has no entry.
inline std::vector<double> fft_twiddles(int n) {
  const double pi = 3.14159265358979323846;
  std::vector<double> table(static_cast<size_t>(n / 2) * 2);
  for (int m = 0; m < n / 2; ++m) {
    const double theta = -(2.0 * pi * static_cast<double>(m)) / static_cast<double>(n);
    table[2 * m] = std::cos(theta);
    table[2 * m + 1] = std::sin(theta);
  }
  return table;
}
inline bool fft_length_ok(int64_t n) { return n >= 1 && n <= kFftMaxLength && (n & (n - 1)) == 0; }
inline int fft_log2(int n) {
  int p = 0;
  while ((1 << p) < n) ++p;
  return p;
}
// Fewer than 2^31 cells: dims that are in order hold at most 2^30, so the rule guards the kernels'
// 32-bit cell index against a change of kFftMaxLength.
inline void require_cell_count(uint64_t cells) {
  require_box(cells < (uint64_t{1} << 31), "the grid has 2^31 cells or more");
}
// dims = (nx, ny, nz): every one a power of two in [1, 1024], fewer than 2^31 cells in all.
// Returns the cells.
inline uint64_t require_fft_dims(const int32_t dims[3]) {
  for (int d = 0; d < 3; ++d) {
    require_box(fft_length_ok(dims[d]), "dims must be powers of two in [1, 1024]");
  }
  const uint64_t cells = static_cast<uint64_t>(dims[0]) * static_cast<uint64_t>(dims[1]) *
                         static_cast<uint64_t>(dims[2]);  // at most 2^30
  require_cell_count(cells);
  return cells;
}
// The workgroups of a streaming kernel that takes kSpectralGroupElements elements each.
inline uint32_t spectral_groups(uint64_t elements) {
  return static_cast<uint32_t>((elements + kSpectralGroupElements - 1) / kSpectralGroupElements);
}
// How a strided pass over lines of length n cuts a plane of `columns` adjacent lines into
// workgroups: `group` adjacent columns each -- kFftGroupElements / n, at least kFftMinColumns, at
// most the plane's -- so that a workgroup's global accesses are runs of `group` 16-byte elements;
// the last of the `groups` holds `last` columns, fewer when group does not divide columns.
struct FftColumnGroups {
  uint32_t group, groups, last;
};
inline FftColumnGroups fft_column_groups(uint64_t columns, int n) {
  const uint64_t wanted = std::max<uint64_t>(kFftGroupElements / n, kFftMinColumns);
  FftColumnGroups cut;
  cut.group = static_cast<uint32_t>(std::min(columns, wanted));
  cut.groups = static_cast<uint32_t>((columns + cut.group - 1) / cut.group);
  cut.last = static_cast<uint32_t>(columns - static_cast<uint64_t>(cut.groups - 1) * cut.group);
  return cut;
}
// The lines a workgroup of an x pass (forward or inverse) stages: kFftGroupElements / nx, at least
// one, at most all x_lines of them.
inline uint32_t fft_x_group(uint32_t x_lines, int nx) {
  return static_cast<uint32_t>(
      std::min<uint64_t>(x_lines, std::max(kFftGroupElements / nx, 1)));
}
// The strided passes along y (pass[0]) and z (pass[1]) of a grid of dims = (nx, ny, nz).
inline void fft_column_passes(const int32_t dims[3], FftPassDev pass_out[2]) {
  const uint64_t row = static_cast<uint64_t>(dims[0]);
  const uint64_t plane = row * static_cast<uint64_t>(dims[1]);
  for (int axis = 1; axis <= 2; ++axis) {
    FftPassDev& pass = pass_out[axis - 1];
    pass.n = dims[axis];
    pass.log2n = fft_log2(dims[axis]);
    pass.planes = axis == 1 ? static_cast<uint32_t>(dims[2]) : 1u;
    pass.columns = static_cast<uint32_t>(axis == 1 ? row : plane);
    pass.plane_stride = plane;
    pass.line_stride = axis == 1 ? row : plane;
    const FftColumnGroups cut = fft_column_groups(pass.columns, pass.n);
    pass.group = cut.group;
    pass.groups = cut.groups;
    pass.last = cut.last;
  }
}
// The lines and passes of the transform of a grid of dims = (nx, ny, nz), forward or inverse.
inline FftLinesDev fft_lines(const int32_t dims[3]) {
  FftLinesDev lines{};
  lines.nx = dims[0];
  lines.log2nx = fft_log2(dims[0]);
  lines.x_lines = static_cast<uint32_t>(dims[1]) * static_cast<uint32_t>(dims[2]);
  lines.x_group = fft_x_group(lines.x_lines, dims[0]);
  fft_column_passes(dims, lines.pass);
  return lines;
}
// A transform's three tables: fft_twiddles for the forward one, fft_inverse_twiddles for the inverse.
struct FftTables {
  std::vector<double> twiddle[3];  // x, y, z; empty for an axis of length 1
  template <class Visit>
  void visit_tables(FftLinesDev* to, Visit&& visit) const {
    for (int d = 0; d < 3; ++d) visit(&to->twiddle[d], twiddle[d].data(), twiddle[d].size());
  }
};
struct Fft3dPlan : FftTables {
  FftArgs args{};
};
// The transform of the real grid `values` [nz][ny][nx] into `spectrum` [nz][ny][nx][2], both device
// arrays the entry point has checked for null.  The rules, in this order: the dims, fewer than 2^31
// cells, no byte shared between the input and the spectrum.
inline Fft3dPlan plan_fft3d(const int32_t dims[3], const void* values, const void* spectrum) {
  const uint64_t cells = require_fft_dims(dims);
  ByteRanges read_ranges, write_ranges;
  append_byte_range(&read_ranges, values, cells * sizeof(double));
  append_byte_range(&write_ranges, spectrum, cells * 2 * sizeof(double));
  require_no_shared_byte(&read_ranges, write_ranges, "the spectrum overlaps the input");
  Fft3dPlan plan;
  for (int d = 0; d < 3; ++d) plan.twiddle[d] = fft_twiddles(dims[d]);
  plan.args.lines = fft_lines(dims);
  return plan;
}

// ---- inverse transform, Helmholtz split, potential ----------------------------------------
// ("Inverse transform, Helmholtz split, potential")
// The inverse table of a line of n values: V[m] = (W[m].re, -W[m].im) of the forward table, the
// negation exact.
inline std::vector<double> fft_inverse_twiddles(int n) {
  std::vector<double> table = fft_twiddles(n);
  for (size_t m = 0; m < table.size() / 2; ++m) table[2 * m + 1] = -table[2 * m + 1];
  return table;
}
// No byte shared between any two of the arrays: sorted by first byte, a range overlaps an earlier
// one iff it begins at or before the largest last byte so far.
inline void require_disjoint(ByteRanges* ranges, const char* message) {
  std::sort(ranges->begin(), ranges->end());
  uintptr_t reach = 0;
  for (size_t r = 1; r < ranges->size(); ++r) {
    reach = std::max(reach, (*ranges)[r - 1].second);
    require_box(reach < (*ranges)[r].first, message);
  }
}
struct Ifft3dPlan : FftTables {  // the tables V
  IfftArgs args{};
};
// The inverse of `spectrum` [nz][ny][nx][2] into the real grids `values` and, unless null, `imag`
// [nz][ny][nx], device arrays of which the entry point has checked the first two for null.  The
// rules, in this order: the dims, fewer than 2^31 cells, no byte shared among the arrays.
inline Ifft3dPlan plan_ifft3d(const int32_t dims[3], const void* spectrum, const void* values,
                              const void* imag) {
  const uint64_t cells = require_fft_dims(dims);
  ByteRanges arrays;
  append_byte_range(&arrays, spectrum, cells * 2 * sizeof(double));
  append_byte_range(&arrays, values, cells * sizeof(double));
  if (imag != nullptr) append_byte_range(&arrays, imag, cells * sizeof(double));
  require_disjoint(&arrays, "the spectrum, values and imag overlap");
  Ifft3dPlan plan;
  for (int d = 0; d < 3; ++d) plan.twiddle[d] = fft_inverse_twiddles(dims[d]);
  plan.args.lines = fft_lines(dims);
  plan.args.scale = 1.0 / static_cast<double>(cells);  // cells is a power of two: exact
  return plan;
}

struct SpectrumHelmholtzPlan {
  HelmholtzArgs args{};  // no table: nothing is staged
  uint32_t groups = 0;   // workgroups of 256 lanes, kSpectralGroupElements modes each
};
// The Helmholtz split of the spectra of (vx, vy, vz), each [nz][ny][nx][2]: `spectra` are read and
// overwritten with the solenoidal part, `compressive` written.  h[d] = 1 / L_d.  The rules, in
// this order: no null array, the dims, fewer than 2^31 cells, per axis h finite and positive, h^2
// not below DBL_MIN (kappa^2 of every mode but 0 is a normal number) and (512 h)^2 finite (the
// largest |m| is 511: q cannot overflow), no byte shared between any two of the six arrays.
inline SpectrumHelmholtzPlan plan_spectrum_helmholtz(const int32_t dims[3], const double h[3],
                                                     const double* const spectra[3],
                                                     const double* const compressive[3]) {
  for (int d = 0; d < 3; ++d) {
    require_box(spectra[d] != nullptr && compressive[d] != nullptr, "null argument");
  }
  const uint64_t cells = require_fft_dims(dims);
  for (int d = 0; d < 3; ++d) {
    require_box(std::isfinite(h[d]) && h[d] > 0.0, "inverse_length must be finite and positive");
    require_box(h[d] * h[d] >= DBL_MIN, "inverse_length is too small: its square underflows");
    const double widest = 512.0 * h[d];
    require_box(std::isfinite(widest * widest),
                "inverse_length is too large: a squared wave number overflows");
  }
  ByteRanges arrays;
  for (int d = 0; d < 3; ++d) {
    append_byte_range(&arrays, spectra[d], cells * 2 * sizeof(double));
    append_byte_range(&arrays, compressive[d], cells * 2 * sizeof(double));
  }
  require_disjoint(&arrays, "two of the six spectra overlap");
  SpectrumHelmholtzPlan plan;
  for (int d = 0; d < 3; ++d) {
    plan.args.log2n[d] = fft_log2(dims[d]);
    plan.args.h[d] = h[d];
  }
  plan.args.n_modes = static_cast<uint32_t>(cells);
  plan.groups = spectral_groups(cells);
  return plan;
}

struct InverseLaplacianPlan {
  InverseLaplacianArgs args{};  // no table: nothing is staged
  uint32_t groups = 0;          // workgroups of 256 lanes, kSpectralGroupElements modes each
};
// `spectrum` [nz][ny][nx][2] times scale / q in place, q the shell sums' (g[d] = 1 / L_d^2), 0 at
// q == 0.  The rules, in this order: the dims, fewer than 2^31 cells, g finite and positive, scale
// finite.
inline InverseLaplacianPlan plan_spectrum_inverse_laplacian(const int32_t dims[3],
                                                            const double g[3], double scale) {
  const uint64_t cells = require_fft_dims(dims);
  for (int d = 0; d < 3; ++d) {
    require_box(std::isfinite(g[d]) && g[d] > 0.0,
                "inverse_length_sq must be finite and positive");
  }
  require_box(std::isfinite(scale), "scale must be finite");
  InverseLaplacianPlan plan;
  for (int d = 0; d < 3; ++d) {
    plan.args.log2n[d] = fft_log2(dims[d]);
    plan.args.g[d] = g[d];
  }
  plan.args.n_modes = static_cast<uint32_t>(cells);
  plan.args.scale = scale;
  plan.groups = spectral_groups(cells);
  return plan;
}

// ---- isolated potential ("Isolated potential") -------------------------------
struct IsolatedGreenPlan {
  IsolatedGreenArgs args{};  // no table: nothing is staged
  uint32_t groups = 0;       // workgroups of 256 lanes, kSpectralGroupElements cells each
};
// The Green's grid G = scale / r of the padded grid padded_dims = (Px, Py, Pz) with cells of
// cell_size = (dx, dy, dz), r measured to the nearer image of the origin, and self_value at r == 0.
// The rules, in this order: no null array, the dims powers of two in [1, 1024], fewer than 2^31
// cells, per axis a size finite and positive, size^2 not below DBL_MIN (r2 of every cell but the
// origin is a normal number) and (512 size)^2 finite (the largest offset is 512 cells: r2 cannot
// overflow), scale and self_value finite.
inline IsolatedGreenPlan plan_isolated_green(const int32_t* padded_dims, const double* cell_size,
                                             double scale, double self_value, const void* green) {
  require_box(padded_dims != nullptr && cell_size != nullptr && green != nullptr, "null argument");
  const uint64_t cells = require_fft_dims(padded_dims);
  for (int d = 0; d < 3; ++d) {
    require_box(std::isfinite(cell_size[d]) && cell_size[d] > 0.0,
                "cell_size must be finite and positive");
    require_box(cell_size[d] * cell_size[d] >= DBL_MIN,
                "cell_size is too small: its square underflows");
    const double widest = 512.0 * cell_size[d];
    require_box(std::isfinite(widest * widest),
                "cell_size is too large: a squared distance overflows");
  }
  require_box(std::isfinite(scale) && std::isfinite(self_value),
              "scale and self_value must be finite");
  IsolatedGreenPlan plan;
  for (int d = 0; d < 3; ++d) {
    plan.args.log2n[d] = fft_log2(padded_dims[d]);
    plan.args.size[d] = cell_size[d];
  }
  plan.args.n_cells = static_cast<uint32_t>(cells);
  plan.args.scale = scale;
  plan.args.self_value = self_value;
  plan.groups = spectral_groups(cells);
  return plan;
}

struct SpectrumMultiplyPlan {
  SpectrumMultiplyArgs args{};  // no table: nothing is staged
  uint32_t groups = 0;          // workgroups of 256 lanes, kSpectralGroupElements modes each
};
// a <- a b mode by mode, both spectra [nz][ny][nx][2].  The rules, in this order: no null array,
// the dims powers of two in [1, 1024], fewer than 2^31 cells, no byte shared between a and b.
inline SpectrumMultiplyPlan plan_spectrum_multiply(const int32_t* dims, const void* a,
                                                   const void* b) {
  require_box(dims != nullptr && a != nullptr && b != nullptr, "null argument");
  const uint64_t cells = require_fft_dims(dims);
  ByteRanges arrays;
  append_byte_range(&arrays, a, cells * 2 * sizeof(double));
  append_byte_range(&arrays, b, cells * 2 * sizeof(double));
  require_disjoint(&arrays, "the two spectra overlap");
  SpectrumMultiplyPlan plan;
  plan.args.n_modes = static_cast<uint32_t>(cells);
  plan.groups = spectral_groups(cells);
  return plan;
}

struct SpectrumBinsPlan {
  std::vector<double> edges_sq;  // n_bins + 1
  SpectrumBinsArgs args{};
  uint32_t groups = 0;           // workgroups of 256 lanes, kSpectralGroupElements modes each
  template <class Visit>
  void visit_tables(SpectrumBinsArgs* to, Visit&& visit) const {
    visit(&to->edges_sq, edges_sq.data(), edges_sq.size());
  }
};
// The shell sums of `spectrum` [nz][ny][nx][2] ("Power spectrum"): a mode's q =
// sum_d m_d^2 g[d] against the n_bins + 1 squared edges.  modes (u64 [n_bins]), power (f64
// [n_bins]) and totals (u64 [2]) are device arrays the entry point has checked for null, as it has
// inverse_length_sq and edges_sq.  The rules, in this order: the dims, fewer than 2^31 cells, n_bins, the
// edges finite, E[0] >= 0, strictly increasing, g finite and positive, no output byte shared with
// the spectrum.
inline SpectrumBinsPlan plan_spectrum_bins(const int32_t dims[3], const double g[3],
                                           const double* edges_sq, int n_bins,
                                           const void* spectrum, const void* modes,
                                           const void* power, const void* totals) {
  const uint64_t cells = require_fft_dims(dims);
  require_box(n_bins >= 1 && n_bins <= kSpectrumMaxBins, "n_bins must lie in [1, 2048]");
  for (int i = 0; i <= n_bins; ++i) {
    require_box(std::isfinite(edges_sq[i]), "edges_sq must be finite");
  }
  require_box(edges_sq[0] >= 0.0, "edges_sq must not be negative");
  for (int i = 1; i <= n_bins; ++i) {
    require_box(edges_sq[i - 1] < edges_sq[i], "edges_sq must be strictly increasing");
  }
  for (int d = 0; d < 3; ++d) {
    require_box(std::isfinite(g[d]) && g[d] > 0.0,
                "inverse_length_sq must be finite and positive");
  }
  ByteRanges read_ranges, write_ranges;
  append_byte_range(&read_ranges, spectrum, cells * 2 * sizeof(double));
  append_byte_range(&write_ranges, modes, static_cast<uint64_t>(n_bins) * sizeof(uint64_t));
  append_byte_range(&write_ranges, power, static_cast<uint64_t>(n_bins) * sizeof(double));
  append_byte_range(&write_ranges, totals, 2 * sizeof(uint64_t));
  require_no_shared_byte(&read_ranges, write_ranges, "an output array overlaps the spectrum");
  SpectrumBinsPlan plan;
  plan.edges_sq.assign(edges_sq, edges_sq + n_bins + 1);
  for (int d = 0; d < 3; ++d) {
    plan.args.log2n[d] = fft_log2(dims[d]);
    plan.args.g[d] = g[d];
  }
  plan.args.n_bins = n_bins;
  plan.args.n_modes = static_cast<uint32_t>(cells);
  plan.groups = spectral_groups(cells);
  return plan;
}

// ---- structure functions ("Structure functions") ------------------------------
struct StructureFunctionsPlan {
  std::vector<StructureLagDev> lags;  // n_lags: the lag and its direction (zeros with one component)
  StructureArgs args{};
  uint32_t groups[3] = {0, 0, 0};     // the grid of workgroups of 256 lanes, the lag running
                                      // fastest: (n_lags, shares of kStructureGroupCells cells up
                                      // to kStructureShareRows, rows of that many shares)
  template <class Visit>
  void visit_tables(StructureArgs* to, Visit&& visit) const {
    visit(&to->lags, lags.data(), lags.size());
  }
};
// The moments of orders 1 .. max_order of the increments of n_components grids [nz][ny][nx] of
// dims = (nx, ny, nz) over n_lags lags (lx, ly, lz), three int32 each, with three f64 of
// directions per lag when there are three components.  pairs (u64 [n_lags]), sums (f64 [n_lags][K]
// [max_order], K = n_components) and totals (u64 [2]) are device arrays.  The rules, in this
// order: no null argument; n_components 1 or 3 (and then every component grid non-null), with
// directions given exactly when it is 3; every dim at least 1, fewer than 2^31 cells; n_lags in
// [1, 4096]; max_order in [1, 8]; periodic 0 or 1; no lag zero; every |l_d| < N_d; the directions
// finite; no byte shared between an output and a component grid, none among the outputs.  The
// component grids may alias each other: they are only read.
inline StructureFunctionsPlan plan_structure_functions(
    const double* const* components, int n_components, const int32_t* dims, const int32_t* lags,
    const double* directions, int n_lags, int max_order, int periodic, const void* pairs,
    const void* sums, const void* totals) {
  require_box(components != nullptr && components[0] != nullptr && dims != nullptr &&
                  lags != nullptr && pairs != nullptr && sums != nullptr && totals != nullptr,
              "null argument");
  require_box(n_components == 1 || n_components == 3, "n_components must be 1 or 3");
  require_box((directions != nullptr) == (n_components == 3),
              "directions are given exactly when there are three components");
  for (int c = 1; c < n_components; ++c) require_box(components[c] != nullptr, "null argument");
  uint64_t cells = 1;  // at most 2^31 - 1 before every product: no 64-bit overflow
  for (int d = 0; d < 3; ++d) {
    require_box(dims[d] >= 1, "dims must be at least 1");
    cells *= static_cast<uint64_t>(dims[d]);
    require_cell_count(cells);
  }
  require_box(n_lags >= 1 && n_lags <= kStructureMaxLags, "n_lags must lie in [1, 4096]");
  require_box(max_order >= 1 && max_order <= kStructureMaxOrder, "max_order must lie in [1, 8]");
  require_box(periodic == 0 || periodic == 1, "periodic must be 0 or 1");
  for (int m = 0; m < n_lags; ++m) {
    require_box(lags[3 * m] != 0 || lags[3 * m + 1] != 0 || lags[3 * m + 2] != 0,
                "a lag is zero");
  }
  for (int m = 0; m < n_lags; ++m) {
    for (int d = 0; d < 3; ++d) {
      require_box(std::llabs(static_cast<long long>(lags[3 * m + d])) < dims[d],
                  "a lag spans a grid length or more along an axis");
    }
  }
  if (directions != nullptr) {
    for (int e = 0; e < 3 * n_lags; ++e) {
      require_box(std::isfinite(directions[e]), "directions must be finite");
    }
  }
  const uint64_t kinds = static_cast<uint64_t>(n_components);
  ByteRanges read_ranges, write_ranges;
  for (int c = 0; c < n_components; ++c) {
    append_byte_range(&read_ranges, components[c], cells * sizeof(double));
  }
  append_byte_range(&write_ranges, pairs, static_cast<uint64_t>(n_lags) * sizeof(uint64_t));
  append_byte_range(&write_ranges, sums,
                    static_cast<uint64_t>(n_lags) * kinds * static_cast<uint64_t>(max_order) *
                        sizeof(double));
  append_byte_range(&write_ranges, totals, 2 * sizeof(uint64_t));
  require_no_shared_byte(&read_ranges, write_ranges, "an output array overlaps a component grid");
  require_disjoint(&write_ranges, "two output arrays overlap");
  StructureFunctionsPlan plan;
  plan.lags.resize(static_cast<size_t>(n_lags));
  for (int m = 0; m < n_lags; ++m) {
    StructureLagDev& lag = plan.lags[static_cast<size_t>(m)];
    lag = StructureLagDev{};
    for (int d = 0; d < 3; ++d) {
      lag.l[d] = lags[3 * m + d];
      if (directions != nullptr) lag.u[d] = directions[3 * m + d];
    }
  }
  StructureArgs& a = plan.args;
  for (int d = 0; d < 3; ++d) a.dims[d] = dims[d];
  a.n_lags = n_lags;
  a.max_order = max_order;
  a.periodic = periodic;
  a.n_cells = static_cast<uint32_t>(cells);
  a.shares = static_cast<uint32_t>((cells + kStructureGroupCells - 1) / kStructureGroupCells);
  const uint32_t rows = kStructureLaneStride / static_cast<uint32_t>(dims[0]);
  a.stride[0] = kStructureLaneStride % static_cast<uint32_t>(dims[0]);
  a.stride[1] = rows % static_cast<uint32_t>(dims[1]);
  a.stride[2] = rows / static_cast<uint32_t>(dims[1]);
  plan.groups[0] = static_cast<uint32_t>(n_lags);
  plan.groups[1] = std::min(a.shares, kStructureShareRows);
  plan.groups[2] = (a.shares + kStructureShareRows - 1) / kStructureShareRows;
  return plan;
}

// ---- velocity cubes ("Velocity cubes") ----------------------------------------
// The partial planes of one batch of channels [batch][entries] f64, then under [entries] and over
// [entries] f64 and n [entries] u32, which the first batch writes and gathers.
struct CubeScratch {
  ScratchPart planes, under, over, n;
  size_t total = 0;
};
inline CubeScratch cube_scratch(size_t entries, size_t batch) {
  CubeScratch scratch;
  scratch.planes = next_scratch_part(&scratch.total, batch * entries * sizeof(double));
  scratch.under = next_scratch_part(&scratch.total, entries * sizeof(double));
  scratch.over = next_scratch_part(&scratch.total, entries * sizeof(double));
  scratch.n = next_scratch_part(&scratch.total, entries * sizeof(uint32_t));
  return scratch;
}
struct VelocityCubePlan {
  std::vector<CubeBoxDev> boxes;     // as the reduction reads them
  std::vector<AxisPlaneDev> planes;  // as the gather reads them
  std::vector<uint32_t> tile_begin;
  std::vector<double> edges;         // n_channels + 1, as given
  uint32_t entries = 0;  // of one partial plane, all boxes: columns x segments, below 2^31
  int32_t batch = 0;     // channels per host batch: min(n_channels, floor(bound / entries))
  int32_t n_batches = 0; // the host loops reduce, gather over them; the last may be partial
  CubeReduceArgs reduce{};  // of batch 0; set_batch() makes those of the others
  CubeGatherArgs gather{};
  CubeScratch scratch;
  template <class Visit>
  void visit_tables(CubeReduceArgs* to_reduce, CubeGatherArgs* to_gather, Visit&& visit) const {
    visit(&to_reduce->boxes, boxes.data(), boxes.size());
    visit(&to_gather->boxes, planes.data(), planes.size());
    visit(&to_reduce->tile_begin, tile_begin.data(), tile_begin.size());
    visit(&to_reduce->edges, edges.data(), edges.size());
  }
  // The launch arguments of batch i: its channels, and under, over and n with the first batch.
  void set_batch(int32_t i, CubeReduceArgs* to_reduce, CubeGatherArgs* to_gather) const {
    const int32_t first = i * batch;
    const int32_t count = std::min(batch, reduce.n_channels - first);
    to_reduce->channel_first = to_gather->channel_first = first;
    to_reduce->channel_count = to_gather->channel_count = count;
    to_reduce->totals = to_gather->totals = i == 0 ? 1 : 0;
  }
};
// e, g and s (s may be null: no width field): the boxes of the emission, the bin and the width
// field.  cube (f64 [n_channels][height][width]), under, over and length (f64 [height][width]) are
// the device arrays written.  scratch_entries: the bound on batch x entries (kCubeScratchEntries;
// a parameter so that a test forces several batches on a small scene).  The rules, in this order:
// the axis; the image size; a finite window; n_levels and a finite level_dl; n_channels in [1,
// 1024]; finite, strictly increasing edges; n_channels x width x height below 2^31; per box the
// box rules of field_box_views, finite corners on the image axes and fewer than 2^31 entries and
// tiles; entries within the scratch bound; no byte shared between an output and an input box's
// cells, none among the outputs.
inline VelocityCubePlan plan_velocity_cube(const avr_box* e, const avr_box* g, const avr_box* s,
                                           size_t n_boxes, int axis, const double origin_uv[2],
                                           double du, double dv, int width, int height,
                                           const double* level_dl, int n_levels,
                                           const double* edges, int n_channels, const void* cube,
                                           const void* under, const void* over, const void* length,
                                           uint64_t scratch_entries = kCubeScratchEntries) {
  require_box(axis >= 0 && axis <= 2, "axis must be 0 (x), 1 (y) or 2 (z)");
  require_image_size(width, height);
  require_box(std::isfinite(origin_uv[0]) && std::isfinite(origin_uv[1]) && std::isfinite(du) &&
                  std::isfinite(dv), "the window must be finite");
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  for (int l = 0; l < n_levels; ++l) {
    require_box(std::isfinite(level_dl[l]), "level_dl must be finite");
  }
  require_box(n_channels >= 1 && n_channels <= kCubeMaxChannels,
              "n_channels must lie in [1, 1024]");
  for (int i = 0; i <= n_channels; ++i) {
    require_box(std::isfinite(edges[i]), "edges must be finite");
    require_box(i == 0 || edges[i - 1] < edges[i], "edges must be strictly increasing");
  }
  const uint64_t pixels = static_cast<uint64_t>(width) * static_cast<uint64_t>(height);
  require_box(static_cast<uint64_t>(n_channels) * pixels < (uint64_t{1} << 31),
              "the cube has 2^31 entries or more");
  const int axis_u = (axis + 1) % 3, axis_v = (axis + 2) % 3;
  VelocityCubePlan plan;
  plan.boxes.resize(n_boxes);
  plan.planes.resize(n_boxes);
  plan.tile_begin.assign(1, 0u);
  ByteRanges read_ranges, write_ranges;
  uint64_t entries = 0;
  const int n_fields = s != nullptr ? 3 : 2;
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = e[b];
    const avr_box* in[3] = {&first, &g[b], s != nullptr ? &s[b] : &g[b]};
    FieldView views[3];
    CubeBoxDev& dev = plan.boxes[b];
    AxisPlaneDev& plane = plan.planes[b];
    std::memset(&dev, 0, sizeof(dev));
    std::memset(&plane, 0, sizeof(plane));
    const bool cells = field_box_views(first, in, n_fields, n_levels, views, &dev.paired);
    if (n_fields == 2) views[2] = views[1];
    for (int f = 0; f < 3; ++f) {
      dev.cells[f] = views[f].cells;
      dev.jstride[f] = views[f].jstride;
      dev.kstride[f] = views[f].kstride;
    }
    uint32_t tiles = 0;
    dev.plane_begin = plane.plane_begin = static_cast<uint32_t>(entries);
    if (cells) {
      require_box(std::isfinite(first.min_corner[axis_u]) && std::isfinite(first.max_corner[axis_u]) &&
                      std::isfinite(first.min_corner[axis_v]) &&
                      std::isfinite(first.max_corner[axis_v]),
                  "box corners must be finite");
      for (int f = 0; f < n_fields; ++f) append_byte_range(&read_ranges, views[f]);
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
      tiles = axis_projection_tiles(axis, dev.nx, dev.ny, dev.nz);
      plane.min_u = first.min_corner[axis_u];
      plane.max_u = first.max_corner[axis_u];
      plane.min_v = first.min_corner[axis_v];
      plane.max_v = first.max_corner[axis_v];
      plane.dl = level_dl[first.level];
      plane.n_u = first.dims[axis_u];
      plane.n_v = first.dims[axis_v];
      plane.segments = (first.dims[axis] + kAxisSegment - 1) / kAxisSegment;
      entries += static_cast<uint64_t>(plane.n_u) * static_cast<uint64_t>(plane.n_v) *
                 static_cast<uint64_t>(plane.segments);
    }
    append_tiles(&plan.tile_begin, tiles);
    require_box(entries < (uint64_t{1} << 31), "scene has too many cells");
  }
  require_box(entries <= scratch_entries,
              "the partial planes of one channel exceed the scratch bound");
  append_byte_range(&write_ranges, cube, static_cast<uint64_t>(n_channels) * pixels * sizeof(double));
  append_byte_range(&write_ranges, under, pixels * sizeof(double));
  append_byte_range(&write_ranges, over, pixels * sizeof(double));
  append_byte_range(&write_ranges, length, pixels * sizeof(double));
  require_no_shared_byte(&read_ranges, write_ranges, "an output array overlaps an input box's cells");
  require_disjoint(&write_ranges, "two output arrays overlap");

  plan.entries = static_cast<uint32_t>(entries);
  const uint64_t fit = entries == 0 ? static_cast<uint64_t>(n_channels) : scratch_entries / entries;
  plan.batch = static_cast<int32_t>(std::min<uint64_t>(static_cast<uint64_t>(n_channels), fit));
  plan.n_batches = (n_channels + plan.batch - 1) / plan.batch;
  plan.scratch = cube_scratch(plan.entries, static_cast<size_t>(plan.batch));
  plan.edges.assign(edges, edges + n_channels + 1);
  CubeReduceArgs& r = plan.reduce;
  r.n_boxes = static_cast<int32_t>(n_boxes);
  r.n_tiles = plan.tile_begin.back();
  r.n_channels = n_channels;
  r.chunk = std::min(kCubeChunk[axis], plan.batch);
  r.entries = plan.entries;
  r.lo = edges[0];
  r.hi = edges[n_channels];
  const double scale = static_cast<double>(n_channels) / (edges[n_channels] - edges[0]);
  r.scale = std::isfinite(scale) ? scale : 0.0;
  CubeGatherArgs& t = plan.gather;
  t.n_boxes = static_cast<int32_t>(n_boxes);
  t.width = width;
  t.height = height;
  t.entries = plan.entries;
  t.origin_u = origin_uv[0];
  t.origin_v = origin_uv[1];
  t.du = du;
  t.dv = dv;
  plan.set_batch(0, &r, &t);
  return plan;
}

// ---- particle fields ------------------------------------------------------------------------
struct ParticleCellsPlan {
  std::vector<ParticleBoxDev> boxes;
  std::vector<uint32_t> cell_begin;   // n_boxes + 1: prefix sum of the boxes' cells, in scene order
  IsoLevelsDev levels;
  StreamLocatorDev locator;           // build_level_locator's
  std::vector<uint32_t> block_begin;  // blocks + 1 ({0} for a scene without cells)
  std::vector<int32_t> block_boxes;
  ParticleCellsArgs args{};
  template <class Visit>
  void visit_tables(ParticleCellsArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->cell_begin, cell_begin.data(), cell_begin.size());
    visit(&to->levels, &levels, 1);
    visit(&to->block_begin, block_begin.data(), block_begin.size());
    visit(&to->block_boxes, block_boxes.data(), block_boxes.size());
  }
};
// The contributions of n particles to the cells of the boxes `scene` ("Particle
// fields").  box_index_lo, level_ratio, level_cell_size and prob_lo as plan_streamlines takes them.
// points [n][3], values [n] (may be null), cells and shares [n][C] with C = 1 (method 0, nearest
// grid point) or 8 (method 1, cloud in cell), levels [n] (may be null) and totals [2] are device
// arrays; all but totals are free to be null with n == 0.  The rules, in this order: n_levels, null
// arrays, method, n (below 2^31, with eight entries each below 2^28), the cell sizes, prob_lo, the
// box rules, the ratios, the index ranges, boxes of one level apart in index space, fewer than 2^31
// cells, the locator's size (max_entries: the bound on its lists, lowered by the plan's test
// only), no output byte shared with another output, with the points or with the values.
inline ParticleCellsPlan plan_particle_cells(const avr_box* scene, size_t n_boxes, uint64_t n,
                                             int method, const int32_t* box_index_lo,
                                             const int32_t* level_ratio,
                                             const double* level_cell_size, const double* prob_lo,
                                             int n_levels, const void* points, const void* values,
                                             const void* cells, const void* shares,
                                             const void* levels_out, const void* totals,
                                             int64_t max_entries = kStreamMaxEntries) {
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  require_box(n_levels == 1 || level_ratio != nullptr, "null argument");
  require_box(n_boxes == 0 || box_index_lo != nullptr, "null argument");
  require_box(level_cell_size != nullptr && prob_lo != nullptr && totals != nullptr,
              "null argument");
  require_box(n == 0 || (points != nullptr && cells != nullptr && shares != nullptr),
              "null argument");
  require_box(method == kParticleNgp || method == kParticleCic,
              "method must be 0 (nearest grid point) or 1 (cloud in cell)");
  require_box(n < (uint64_t{1} << (method == kParticleCic ? 28 : 31)),
              method == kParticleCic ? "n must stay below 2^28 for cloud in cell"
                                     : "n must stay below 2^31");
  ParticleCellsPlan plan;
  IsoLevelsDev& levels = plan.levels;
  fill_level_geometry(level_cell_size, prob_lo, n_levels, &levels);
  std::vector<ParticleBoxDev>& boxes = plan.boxes;
  boxes.resize(n_boxes);
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = scene[b];
    const avr_box* fields[1] = {&first};
    FieldView view;
    ParticleBoxDev& dev = boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    int32_t paired;
    const bool has_cells = field_box_views(first, fields, 1, n_levels, &view, &paired);
    dev.level = first.level;
    if (has_cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
    }
  }
  fill_level_ratios(level_ratio, n_levels, levels.ratio);
  const std::vector<IndexRegion> regions = box_index_regions(box_index_lo, scene, &boxes);
  require_levels_disjoint(boxes, regions);
  plan.cell_begin = cell_ordinals(boxes);
  build_level_locator(boxes, regions, levels.ratio, max_entries, &plan.locator, &plan.block_begin,
                      &plan.block_boxes);
  const uint64_t entries = n * (method == kParticleCic ? 8u : 1u);
  if (n > 0) {
    ByteRanges read_ranges, write_ranges;
    append_byte_range(&write_ranges, cells, entries * sizeof(int64_t));
    append_byte_range(&write_ranges, shares, entries * sizeof(double));
    if (levels_out != nullptr) append_byte_range(&write_ranges, levels_out, n);
    append_byte_range(&write_ranges, totals, 2 * sizeof(uint64_t));
    append_byte_range(&read_ranges, points, n * 3 * sizeof(double));
    if (values != nullptr) append_byte_range(&read_ranges, values, n * sizeof(double));
    const ByteRanges written = write_ranges;
    require_disjoint(&write_ranges, "two output arrays overlap");
    require_no_shared_byte(&read_ranges, written,
                           "an output array overlaps the points or the values");
  }
  plan.args.locator = plan.locator;
  plan.args.n_levels = n_levels;
  plan.args.n = static_cast<uint32_t>(n);
  plan.args.paired = ((reinterpret_cast<uintptr_t>(cells) | reinterpret_cast<uintptr_t>(shares)) &
                      15u) == 0;
  return plan;
}

struct ParticleDepositPlan {
  std::vector<GridBoxDev> boxes;
  std::vector<uint32_t> tile_begin;
  std::vector<uint32_t> cell_begin;
  ParticleLevelsDev levels;
  ParticleDepositArgs args{};
  template <class Visit>
  void visit_tables(ParticleDepositArgs* to, Visit&& visit) const {
    visit(&to->boxes, boxes.data(), boxes.size());
    visit(&to->tile_begin, tile_begin.data(), tile_begin.size());
    visit(&to->cell_begin, cell_begin.data(), cell_begin.size());
    visit(&to->levels, &levels, 1);
  }
};
// The contributions cells [n], shares [n] (device arrays, sorted by cell, free to be null with n ==
// 0) added onto the cells of the boxes `out`: the sum, or with quantity 1 the sum over the volume
// of a cell of the box's level.  The rules, in this order: n_levels, null arrays, quantity, n, the
// cell sizes, the box rules, fewer than 2^31 cells, no byte of the cells or the shares shared with
// an output box's cells.  That the cells ascend is the caller's to see to: they live on the device.
inline ParticleDepositPlan plan_particle_deposit(const avr_box* out, size_t n_boxes, uint64_t n,
                                                 int quantity, const double* level_cell_size,
                                                 int n_levels, const void* cells,
                                                 const void* shares) {
  require_box(n_levels >= 1 && n_levels <= kFieldMaxLevels, "n_levels must lie in [1, 16]");
  require_box(level_cell_size != nullptr, "null argument");
  require_box(n == 0 || (cells != nullptr && shares != nullptr), "null argument");
  require_box(quantity == kParticleSum || quantity == kParticleDensity,
              "quantity must be 0 (sum) or 1 (density)");
  require_box(n < (uint64_t{1} << 31), "n_contributions must stay below 2^31");
  ParticleDepositPlan plan;
  for (int l = 0; l < kFieldMaxLevels; ++l) plan.levels.volume[l] = 1.0;
  for (int l = 0; l < n_levels; ++l) {
    const double* size = level_cell_size + l * 3;
    for (int d = 0; d < 3; ++d) {
      require_box(std::isfinite(size[d]) && size[d] > 0.0,
                  "level_cell_size must be finite and positive");
    }
    plan.levels.volume[l] = (size[0] * size[1]) * size[2];
  }
  std::vector<GridBoxDev>& boxes = plan.boxes;
  boxes.resize(n_boxes);
  plan.tile_begin.assign(1, 0u);
  ByteRanges read_ranges, write_ranges;
  for (size_t b = 0; b < n_boxes; ++b) {
    const avr_box& first = out[b];
    const avr_box* fields[1] = {&first};
    FieldView view;
    GridBoxDev& dev = boxes[b];
    std::memset(&dev, 0, sizeof(dev));
    const bool has_cells = field_box_views(first, fields, 1, n_levels, &view, &dev.paired);
    dev.out = const_cast<double*>(view.cells);
    dev.jstride = view.jstride;
    dev.kstride = view.kstride;
    dev.level = first.level;
    if (has_cells) {
      dev.nx = first.dims[0];
      dev.ny = first.dims[1];
      dev.nz = first.dims[2];
      append_byte_range(&write_ranges, view);
    }
    append_tiles(&plan.tile_begin, has_cells ? cell_tiles(dev.nx, dev.ny, dev.nz) : 0u);
  }
  plan.cell_begin = cell_ordinals(boxes);
  if (n > 0) {
    append_byte_range(&read_ranges, cells, n * sizeof(int64_t));
    append_byte_range(&read_ranges, shares, n * sizeof(double));
    require_no_shared_byte(&read_ranges, write_ranges,
                           "the cells or the shares overlap an output box's cells");
  }
  plan.args.n_boxes = static_cast<int32_t>(n_boxes);
  plan.args.n_tiles = plan.tile_begin.back();
  plan.args.n_cells = plan.cell_begin.back();
  plan.args.n = static_cast<uint32_t>(n);
  return plan;
}

// ---- particle groups ------------------------------------------------------------------------
// The grid of both calls: lo, hi finite with lo < hi; dims each in [1, 1024], their product below
// 2^27, at least 3 on a periodic axis.  Fills *grid; the caller has checked the four for null.
inline void fill_group_grid(const double* lo, const double* hi, const int32_t* dims,
                            const int32_t* periodic, GroupGridDev* grid) {
  for (int d = 0; d < 3; ++d) {
    require_box(std::isfinite(lo[d]) && std::isfinite(hi[d]) && lo[d] < hi[d] &&
                    std::isfinite(hi[d] - lo[d]),
                "lo and hi must be finite with lo < hi");
  }
  uint64_t cells = 1;
  for (int d = 0; d < 3; ++d) {
    require_box(dims[d] >= 1 && dims[d] <= kGroupMaxDim, "dims must lie in [1, 1024]");
    cells *= static_cast<uint64_t>(dims[d]);
  }
  require_box(cells < (uint64_t{1} << 27), "the grid must hold fewer than 2^27 cells");
  for (int d = 0; d < 3; ++d) {
    require_box(periodic[d] == 0 || dims[d] >= 3, "a periodic axis needs at least 3 cells");
  }
  for (int d = 0; d < 3; ++d) {
    grid->lo[d] = lo[d];
    grid->hi[d] = hi[d];
    grid->length[d] = hi[d] - lo[d];
    grid->h[d] = grid->length[d] / static_cast<double>(dims[d]);
    grid->top[d] = static_cast<double>(dims[d] - 1);
    grid->dims[d] = dims[d];
    grid->periodic[d] = periodic[d] != 0 ? 1 : 0;
  }
}

struct ParticleGroupCellsPlan {
  ParticleGroupCellsArgs args{};
};
// The cells and parent entries of n particles ("Particle groups").  points [n][3],
// cells [n], parent [n] and totals [1] are device arrays, all free to be null with n == 0; lo, hi,
// dims and periodic are host arrays of three.  The rules, in this order: null arrays, n below 2^31,
// lo and hi, the dims, no output byte shared with another output or with the points.
inline ParticleGroupCellsPlan plan_particle_group_cells(uint64_t n, const double* lo,
                                                        const double* hi, const int32_t* dims,
                                                        const int32_t* periodic,
                                                        const void* points, const void* cells,
                                                        const void* parent, const void* totals) {
  require_box(lo != nullptr && hi != nullptr && dims != nullptr && periodic != nullptr,
              "null argument");
  require_box(n == 0 || (points != nullptr && cells != nullptr && parent != nullptr &&
                         totals != nullptr),
              "null argument");
  require_box(n < (uint64_t{1} << 31), "n must stay below 2^31");
  ParticleGroupCellsPlan plan;
  fill_group_grid(lo, hi, dims, periodic, &plan.args.grid);
  if (n > 0) {
    ByteRanges read_ranges, write_ranges;
    append_byte_range(&write_ranges, cells, n * sizeof(uint32_t));
    append_byte_range(&write_ranges, parent, n * sizeof(uint32_t));
    append_byte_range(&write_ranges, totals, sizeof(uint64_t));
    append_byte_range(&read_ranges, points, n * 3 * sizeof(double));
    const ByteRanges written = write_ranges;
    require_disjoint(&write_ranges, "two output arrays overlap");
    require_no_shared_byte(&read_ranges, written, "an output array overlaps the points");
  }
  plan.args.n = static_cast<uint32_t>(n);
  return plan;
}

// One count per chunk of kGroupChunk particles.
struct GroupScratch {
  ScratchPart chunk_counts;
  size_t total = 0;
};
struct ParticleGroupsPlan {
  ParticleGroupsArgs args{};
  GroupScratch scratch;
};
// The groups of n particles of which the first n_inside sorted slots are inside.  points_sorted
// [n][3], order [n] (i64), cell_begin [cells + 1] (i64), parent [n] (u32, read and written), labels
// [n] (i32), sizes [n] (u32) and n_groups [1] (u64) are device arrays; all but n_groups are free to
// be null with n == 0.  The rules, in this order: null arrays, n below 2^31, n_inside at most n, b
// finite and positive, lo and hi, the dims, h >= b (1 + 2^-10) wherever dims > 1, min_members in
// [1, 2^31), no output byte shared with another output or with an input.
inline ParticleGroupsPlan plan_particle_groups(uint64_t n, uint64_t n_inside, double b,
                                               const double* lo, const double* hi,
                                               const int32_t* dims, const int32_t* periodic,
                                               int64_t min_members, const void* points_sorted,
                                               const void* order, const void* cell_begin,
                                               const void* parent, const void* labels,
                                               const void* sizes, const void* n_groups) {
  require_box(lo != nullptr && hi != nullptr && dims != nullptr && periodic != nullptr &&
                  n_groups != nullptr,
              "null argument");
  require_box(n == 0 || (points_sorted != nullptr && order != nullptr && cell_begin != nullptr &&
                         parent != nullptr && labels != nullptr && sizes != nullptr),
              "null argument");
  require_box(n < (uint64_t{1} << 31), "n must stay below 2^31");
  require_box(n_inside <= n, "n_inside must not exceed n");
  require_box(std::isfinite(b) && b > 0.0, "the linking length must be finite and positive");
  ParticleGroupsPlan plan;
  GroupGridDev& grid = plan.args.grid;
  fill_group_grid(lo, hi, dims, periodic, &grid);
  const double least = b * 1.0009765625;  // b (1 + 2^-10), one rounding
  for (int d = 0; d < 3; ++d) {
    require_box(dims[d] == 1 || grid.h[d] >= least,
                "a cell must be at least (1 + 2^-10) linking lengths wide");
  }
  require_box(min_members >= 1 && min_members < (int64_t{1} << 31),
              "min_members must lie in [1, 2^31)");
  const uint64_t cells = static_cast<uint64_t>(dims[0]) * static_cast<uint64_t>(dims[1]) *
                         static_cast<uint64_t>(dims[2]);
  if (n > 0) {
    ByteRanges read_ranges, write_ranges;
    append_byte_range(&write_ranges, parent, n * sizeof(uint32_t));
    append_byte_range(&write_ranges, labels, n * sizeof(int32_t));
    append_byte_range(&write_ranges, sizes, n * sizeof(uint32_t));
    append_byte_range(&write_ranges, n_groups, sizeof(uint64_t));
    append_byte_range(&read_ranges, points_sorted, n * 3 * sizeof(double));
    append_byte_range(&read_ranges, order, n * sizeof(int64_t));
    append_byte_range(&read_ranges, cell_begin, (cells + 1) * sizeof(int64_t));
    const ByteRanges written = write_ranges;
    require_disjoint(&write_ranges, "two output arrays overlap");
    require_no_shared_byte(&read_ranges, written,
                           "an output array overlaps the points, the order or the cell ranges");
  }
  plan.args.b2 = b * b;
  plan.args.n = static_cast<uint32_t>(n);
  plan.args.n_inside = static_cast<uint32_t>(n_inside);
  plan.args.n_chunks = static_cast<uint32_t>((n + kGroupChunk - 1) / kGroupChunk);
  plan.args.n_cells = static_cast<uint32_t>(cells);
  plan.args.min_members = static_cast<uint32_t>(min_members);
  plan.scratch.chunk_counts =
      next_scratch_part(&plan.scratch.total, (plan.args.n_chunks + 1) * sizeof(uint32_t));
  return plan;
}

}  // namespace avr

#endif
