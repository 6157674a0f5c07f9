// What the field products' plans (csrc/avr_field_plans.h) hand to their entry points, as a plain
// C++ program built with AddressSanitizer and UBSan and without HIP: for all twelve products, on a
// two-level scene of a coarse 4x4x4 box, a fine 4x4x4 box touching it and a box without cells,
//  - every launch argument that is not a device address, against the value written out here from
//    the call's arguments, and every address still null;
//  - the tables visit_tables names: which argument each goes to, its element size and its count, in
//    the order they are staged; that visiting changes nothing; and, for a scene without boxes, that
//    the tables which can be empty report count 0 and the stager's sizing pass counts one element;
//  - the scratch layouts: the parts in order, aligned, apart, ending at the total, and the total
//    against the formula the entry points used to spell out inline.
// No cell is ever allocated or read.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../amrvolumerenderer_amd/csrc/avr_field_plans.h"

namespace avr {
// the kernel file's tile count, not linked here: three tiles per box with cells
uint32_t axis_projection_tiles(int, int, int, int) { return 3; }
}  // namespace avr

namespace {

void fail(const std::string& what) {
  std::fprintf(stderr, "FAILED: %s\n", what.c_str());
  std::exit(1);
}
void expect(bool condition, const std::string& what) {
  if (!condition) fail(what);
}

const void* address(int bit) { return reinterpret_cast<const void*>(uintptr_t{1} << bit); }

// ---- the scene ------------------------------------------------------------------------------
// Box 0: level 0, cells [0, 4)^3.  Box 1: level 1 (ratio 2), cells [8, 12) x [0, 4)^2, which is
// level 0's [4, 6) x [0, 2)^2: it touches box 0's high x face.  Box 2: level 0, no cells.
// Field `id` of the scene has its cells at made-up addresses that nothing reads, 2^36 bytes apart
// from the next field's and 2^31 bytes from the next box's.
std::vector<avr_box> field(int id, bool with_cells = true) {
  std::vector<avr_box> boxes;
  if (!with_cells) return boxes;
  const int level[3] = {0, 1, 0}, n[3] = {4, 4, 0};
  const double x0[3] = {0.0, 1.0, 2.0}, size[3] = {0.25, 0.125, 0.25};
  for (int b = 0; b < 3; ++b) {
    avr_box box{};
    for (int d = 0; d < 3; ++d) {
      box.dims[d] = n[b];
      box.min_corner[d] = d == 0 ? x0[b] : 0.0;
      box.max_corner[d] = box.min_corner[d] + n[b] * size[b];
    }
    box.level = level[b];
    box.jstride = n[b];
    box.kstride = n[b] * n[b];
    if (n[b] > 0) {
      box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 40) + (uintptr_t(id) << 36) +
                                                  (uintptr_t(b) << 31));
    }
    boxes.push_back(box);
  }
  return boxes;
}
const int32_t kIndexLo[9] = {0, 0, 0, 8, 0, 0, 0, 0, 0};
const int32_t kRatio[1] = {2};
const double kCellSize[6] = {0.25, 0.25, 0.25, 0.125, 0.125, 0.125};  // (dx, dy, dz) per level
const double kProbLo[3] = {0.0, 0.0, 0.0};
const int kLevels = 2;
const avr_box kNoBox{};  // what a scene without boxes points at

// ---- the tables a plan names ----------------------------------------------------------------
struct Table {
  const void* to;  // where in the launch arguments the device address goes
  size_t element, count;
  const void* from;
  uint64_t hash;   // of the table's bytes
  bool operator==(const Table& o) const {
    return to == o.to && element == o.element && count == o.count && from == o.from &&
           hash == o.hash;
  }
};
struct Recorder {
  std::vector<Table> tables;
  template <class T>
  void operator()(const T** device, const T* host, size_t count) {
    uint64_t hash = 1469598103934665603ull;
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(host);
    for (size_t i = 0; i < count * sizeof(T); ++i) hash = (hash ^ bytes[i]) * 1099511628211ull;
    tables.push_back({device, sizeof(T), count, host, hash});
  }
};
struct Want {
  const void* to;
  size_t element, count;
};
// The plan's tables are `want`, in order; the sizing pass counts every one of them, an empty one as
// one element; and neither pass changes the plan or sets an address.
template <class Plan, class... Args>
void expect_tables(const std::string& name, const Plan& plan, const std::vector<Want>& want,
                   Args*... args) {
  Recorder first, second;
  plan.visit_tables(args..., first);
  expect(first.tables.size() == want.size(),
         name + ": " + std::to_string(first.tables.size()) + " tables");
  size_t bytes = 0;
  for (size_t t = 0; t < want.size(); ++t) {
    const Table& got = first.tables[t];
    const std::string where = name + ": table " + std::to_string(t);
    expect(got.to == want[t].to, where + " goes to another argument");
    expect(got.element == want[t].element,
           where + " has elements of " + std::to_string(got.element) + " bytes");
    expect(got.count == want[t].count, where + " has " + std::to_string(got.count) + " entries");
    const void* address_now;
    std::memcpy(&address_now, got.to, sizeof(address_now));
    expect(address_now == nullptr, where + ": address set by a visit");
    bytes += (want[t].count != 0 ? want[t].count : 1) * want[t].element;
  }
  avr::StagingSize size;
  plan.visit_tables(args..., size);
  expect(size.items == static_cast<int>(want.size()), name + ": the sizing pass's item count");
  expect(size.bytes == bytes, name + ": the sizing pass counts " + std::to_string(size.bytes) +
                                  " bytes, not " + std::to_string(bytes));
  plan.visit_tables(args..., second);
  expect(first.tables == second.tables, name + ": the plan changed under a visit");
}

// ---- scratch layouts ------------------------------------------------------------------------
struct Part {
  avr::ScratchPart part;
  size_t element;
  bool wanted;  // present
};
void expect_layout(const std::string& name, const std::vector<Part>& parts, size_t total,
                   size_t formula) {
  size_t end = 0;
  for (size_t p = 0; p < parts.size(); ++p) {
    const avr::ScratchPart& part = parts[p].part;
    const std::string where = name + ": part " + std::to_string(p);
    expect(part.present == parts[p].wanted, where + " is present or absent wrongly");
    if (!part.present) {
      expect(part.bytes == 0, where + " is absent and has bytes");
      continue;
    }
    expect(part.offset >= end, where + " begins inside the part before it");
    expect(part.offset == end, where + " leaves a gap the formula does not have");
    expect(part.offset % parts[p].element == 0, where + " is misaligned");
    expect(part.bytes % parts[p].element == 0, where + " holds a broken element");
    end = part.offset + part.bytes;
  }
  expect(end == total, name + ": the last part does not end at the total");
  expect(total == formula, name + ": total " + std::to_string(total) + ", formula " +
                               std::to_string(formula));
}
void expect_axis_layout(const avr::AxisScratch& s, size_t entries, bool weighted) {
  expect_layout("axis scratch", {{s.s, 8, true}, {s.w, 8, weighted}, {s.n, 4, true}}, s.total,
                entries * (weighted ? 20 : 12));
  expect(s.s.bytes == entries * 8 && s.n.bytes == entries * 4, "axis scratch: part sizes");
}
void expect_gradient_layout(const avr::GradientScratch& s, size_t faces) {
  expect_layout("gradient scratch", {{s.face_value, 8, true}, {s.face_present, 1, true}}, s.total,
                faces * 2 * (sizeof(double) + 1));
  expect(s.face_value.bytes == faces * 16, "gradient scratch: part sizes");
}
void expect_clump_layout(const avr::ClumpScratch& s, size_t chunks) {
  expect_layout("clump scratch", {{s.parent, 4, true}, {s.chunk_roots, 4, true}}, s.total,
                (chunks * 1024 + chunks) * sizeof(uint32_t));
  expect(s.parent.bytes == chunks * 4096, "clump scratch: part sizes");
}
void expect_iso_layout(const avr::IsoScratch& s, size_t shell, size_t chunks, bool has_sample) {
  expect_layout("isosurface scratch",
                {{s.shell_value, 8, true}, {s.shell_sample, 8, has_sample},
                 {s.chunk_offset, 8, true}, {s.chunk_triangles, 4, true},
                 {s.chunk_skipped, 4, true}, {s.shell_code, 1, true}},
                s.total, shell * (has_sample ? 2 : 1) * sizeof(double) + chunks * 16 + shell);
  expect(s.shell_value.bytes == shell * 8 && s.chunk_offset.bytes == chunks * 8 &&
             s.chunk_triangles.bytes == chunks * 4 && s.shell_code.bytes == shell,
         "isosurface scratch: part sizes");
}

// ---- the products ---------------------------------------------------------------------------
void test_joint_histogram(bool with_y) {
  const std::string name = with_y ? "joint histogram (x, y)" : "joint histogram (x)";
  const std::vector<avr_box> x = field(0), y = field(1), s = field(2);
  const double x_edges[4] = {0.0, 1.0, 2.0, 4.0}, y_edges[3] = {-1.0, 0.0, 3.0};
  const avr::JointHistogramPlan plan = avr::plan_joint_histogram(
      x.data(), with_y ? y.data() : nullptr, s.data(), 3, x_edges, 3, with_y ? y_edges : nullptr,
      with_y ? 2 : 1, kLevels);
  const avr::JointHistogramArgs& a = plan.args;
  expect(a.n_boxes == 3 && a.n_tiles == 2 && a.nx == 3 && a.ny == (with_y ? 2 : 1), name + ": counts");
  expect(a.x_lo == 0.0 && a.x_hi == 4.0 && a.x_scale == 0.75, name + ": the x axis");
  expect(with_y ? a.y_lo == -1.0 && a.y_hi == 3.0 && a.y_scale == 0.5
                : a.y_lo == 0.0 && a.y_hi == 0.0 && a.y_scale == 0.0, name + ": the y axis");
  expect(a.boxes == nullptr && a.tile_begin == nullptr && a.x_edges == nullptr &&
             a.y_edges == nullptr && a.cells == nullptr && a.sums == nullptr &&
             a.totals == nullptr, name + ": an address is set");
  avr::JointHistogramArgs to = plan.args;
  std::vector<Want> want = {{&to.boxes, sizeof(avr::JointBoxDev), 3},
                            {&to.tile_begin, sizeof(uint32_t), 4},
                            {&to.x_edges, sizeof(double), 4}};
  if (with_y) want.push_back({&to.y_edges, sizeof(double), 3});
  expect_tables(name, plan, want, &to);
  expect(std::memcmp(plan.x_edges.data(), x_edges, sizeof(x_edges)) == 0, name + ": the x edges");
  expect(!with_y || std::memcmp(plan.y_edges.data(), y_edges, sizeof(y_edges)) == 0,
         name + ": the y edges");
}

void test_slice() {
  const std::vector<avr_box> f = field(0);
  const double origin[3] = {0.0, 0.5, 0.5}, du[3] = {0.25, 0.0, 0.0}, dv[3] = {0.0, 0.125, 0.0};
  const avr::SlicePlan plan = avr::plan_slice(f.data(), 3, nullptr, origin, du, dv, 5, 7);
  expect(plan.args.n_boxes == 3 && plan.args.width == 5 && plan.args.height == 7, "slice: counts");
  expect(plan.args.boxes == nullptr, "slice: an address is set");
  avr::SliceArgs to = plan.args;
  expect_tables("slice", plan, {{&to.boxes, sizeof(avr::SliceBoxDev), 3}}, &to);
  const avr::SlicePlan none = avr::plan_slice(&kNoBox, 0, nullptr, origin, du, dv, 5, 7);
  to = none.args;
  expect_tables("slice, no boxes", none, {{&to.boxes, sizeof(avr::SliceBoxDev), 0}}, &to);
}

void test_axis_projection(bool weighted) {
  const std::string name = weighted ? "weighted axis projection" : "axis projection";
  const std::vector<avr_box> f = field(0), w = field(1);
  const double origin_uv[2] = {0.5, -0.25}, level_dl[2] = {0.25, 0.125};
  const avr::AxisProjectionPlan plan = avr::plan_axis_projection(
      f.data(), weighted ? w.data() : nullptr, 3, 2, origin_uv, 0.125, 0.25, 6, 3, level_dl,
      kLevels);
  const avr::AxisReduceArgs& r = plan.reduce;
  const avr::AxisGatherArgs& g = plan.gather;
  expect(r.n_boxes == 3 && r.n_tiles == 6, name + ": the reduction's counts");
  expect(g.n_boxes == 3 && g.width == 6 && g.height == 3 && g.origin_u == 0.5 &&
             g.origin_v == -0.25 && g.du == 0.125 && g.dv == 0.25, name + ": the gather's window");
  expect(r.boxes == nullptr && r.tile_begin == nullptr && r.plane_s == nullptr &&
             r.plane_w == nullptr && r.plane_n == nullptr && g.boxes == nullptr &&
             g.plane_s == nullptr && g.plane_w == nullptr && g.plane_n == nullptr &&
             g.integral == nullptr && g.weight == nullptr && g.length == nullptr,
         name + ": an address is set");
  avr::AxisReduceArgs to_r = plan.reduce;
  avr::AxisGatherArgs to_g = plan.gather;
  expect_tables(name, plan,
                {{&to_r.boxes, sizeof(avr::AxisBoxDev), 3},
                 {&to_g.boxes, sizeof(avr::AxisPlaneDev), 3},
                 {&to_r.tile_begin, sizeof(uint32_t), 4}},
                &to_r, &to_g);
  // 4 x 4 columns of one segment, two boxes
  expect_axis_layout(plan.scratch, 32, weighted);
  expect_axis_layout(avr::axis_scratch(1000003, !weighted), 1000003, !weighted);
}

void test_derive() {
  const std::vector<avr_box> a = field(0), b = field(1), out = field(2);
  const avr_box* inputs[2] = {a.data(), b.data()};
  const uint32_t program[3] = {avr::kDeriveField | (0u << 8), avr::kDeriveField | (1u << 8),
                               avr::kDeriveAdd};
  const double origin[9] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 2.0, 0.0, 0.0};
  const avr::DerivePlan plan = avr::plan_derive(inputs, 2, out.data(), 3, program, 3, nullptr, 0,
                                                origin, kCellSize, kLevels);
  const avr::DeriveArgs& args = plan.args;
  expect(args.n_boxes == 3 && args.n_tiles == 2 && args.n_fields == 2 && args.n_instructions == 3,
         "derive: counts");
  expect(args.boxes == nullptr && args.tile_begin == nullptr && args.program == nullptr,
         "derive: an address is set");
  avr::DeriveArgs to = plan.args;
  expect_tables("derive", plan,
                {{&to.boxes, sizeof(avr::DeriveBoxDev), 3},
                 {&to.tile_begin, sizeof(uint32_t), 4},
                 {&to.program, sizeof(avr::DeriveProgramDev), 1}},
                &to);
}

void test_gradient() {
  const std::vector<avr_box> in = field(0), out = field(1);
  const double dx[2] = {0.25, 0.125};
  const avr::GradientPlan plan =
      avr::plan_gradient(in.data(), out.data(), 3, 0, kIndexLo, kRatio, dx, kLevels);
  const avr::GradientArgs& args = plan.args;
  // 4 x 4 face cells per side and box with cells
  expect(args.n_boxes == 3 && args.n_levels == 2 && args.n_tiles == 2 && args.n_faces == 32,
         "gradient: counts");
  expect(args.boxes == nullptr && args.tile_begin == nullptr && args.face_begin == nullptr &&
             args.candidate_begin == nullptr && args.candidates == nullptr &&
             args.levels == nullptr && args.face_value == nullptr && args.face_present == nullptr,
         "gradient: an address is set");
  avr::GradientArgs to = plan.args;
  // box 0's high face sees box 1 one level finer, box 1's low face sees box 0
  expect_tables("gradient", plan,
                {{&to.boxes, sizeof(avr::GradientBoxDev), 3},
                 {&to.tile_begin, sizeof(uint32_t), 4},
                 {&to.face_begin, sizeof(uint32_t), 4},
                 {&to.candidate_begin, sizeof(uint32_t), 7},
                 {&to.candidates, sizeof(int32_t), 2},
                 {&to.levels, sizeof(avr::LevelRatiosDev), 1}},
                &to);
  expect_gradient_layout(plan.scratch, 32);
  expect_gradient_layout(avr::gradient_scratch(12345), 12345);
  // a lone box: no face has a neighbour
  const avr::GradientPlan lone =
      avr::plan_gradient(in.data(), out.data(), 1, 0, kIndexLo, nullptr, dx, 1);
  to = lone.args;
  expect_tables("gradient, a lone box", lone,
                {{&to.boxes, sizeof(avr::GradientBoxDev), 1},
                 {&to.tile_begin, sizeof(uint32_t), 2},
                 {&to.face_begin, sizeof(uint32_t), 2},
                 {&to.candidate_begin, sizeof(uint32_t), 3},
                 {&to.candidates, sizeof(int32_t), 0},
                 {&to.levels, sizeof(avr::LevelRatiosDev), 1}},
                &to);
}

void test_clumps() {
  const std::vector<avr_box> in = field(0), out = field(1);
  const avr::ClumpPlan plan =
      avr::plan_clumps(in.data(), out.data(), 3, -1.0, 2.5, kIndexLo, kRatio, kLevels);
  const avr::ClumpArgs& args = plan.args;
  // 2 x 64 cells: one chunk of 1024
  expect(args.n_boxes == 3 && args.n_levels == 2 && args.n_tiles == 2 && args.n_cells == 128 &&
             args.n_chunks == 1 && args.lower == -1.0 && args.upper == 2.5, "clumps: counts");
  expect(args.boxes == nullptr && args.tile_begin == nullptr && args.candidate_begin == nullptr &&
             args.candidates == nullptr && args.levels == nullptr && args.parent == nullptr &&
             args.chunk_roots == nullptr && args.count == nullptr, "clumps: an address is set");
  avr::ClumpArgs to = plan.args;
  // only box 1's low x face has a neighbour of its own or a coarser level: box 0
  expect_tables("clumps", plan,
                {{&to.boxes, sizeof(avr::ClumpBoxDev), 3},
                 {&to.tile_begin, sizeof(uint32_t), 4},
                 {&to.candidate_begin, sizeof(uint32_t), 19},
                 {&to.candidates, sizeof(int32_t), 1},
                 {&to.levels, sizeof(avr::LevelRatiosDev), 1}},
                &to);
  expect_clump_layout(plan.scratch, 1);
  expect_clump_layout(avr::clump_scratch(77), 77);
  const avr::ClumpPlan lone =
      avr::plan_clumps(in.data(), out.data(), 1, -1.0, 2.5, kIndexLo, nullptr, 1);
  to = lone.args;
  expect_tables("clumps, a lone box", lone,
                {{&to.boxes, sizeof(avr::ClumpBoxDev), 1},
                 {&to.tile_begin, sizeof(uint32_t), 2},
                 {&to.candidate_begin, sizeof(uint32_t), 7},
                 {&to.candidates, sizeof(int32_t), 0},
                 {&to.levels, sizeof(avr::LevelRatiosDev), 1}},
                &to);
}

void test_clump_table() {
  const std::vector<avr_box> labels = field(0), summed = field(1);
  const avr::ClumpTablePlan plan =
      avr::plan_clump_table(labels.data(), summed.data(), 3, 5, kLevels);
  const avr::ClumpTableArgs& args = plan.args;
  expect(args.n_boxes == 3 && args.n_tiles == 2 && args.n_clumps == 5, "clump table: counts");
  expect(args.boxes == nullptr && args.tile_begin == nullptr && args.cells == nullptr &&
             args.sums == nullptr && args.totals == nullptr, "clump table: an address is set");
  avr::ClumpTableArgs to = plan.args;
  expect_tables("clump table", plan,
                {{&to.boxes, sizeof(avr::JointBoxDev), 3}, {&to.tile_begin, sizeof(uint32_t), 4}},
                &to);
}

void test_isosurface(bool with_sample) {
  const std::string name = with_sample ? "isosurface with samples" : "isosurface";
  const std::vector<avr_box> f = field(0), s = field(1);
  const avr::IsoPlan plan = avr::plan_isosurface(
      f.data(), with_sample ? s.data() : nullptr, 3, 0.5, kIndexLo, kRatio, kCellSize, kProbLo,
      kLevels, 10, address(50), address(51), with_sample ? address(52) : nullptr, address(53));
  const avr::IsoArgs& args = plan.args;
  // 5^3 cube bases and 6^3 - 4^3 shell cells per box with cells
  expect(args.n_boxes == 3 && args.n_levels == 2 && args.n_bases == 250 && args.n_chunks == 1 &&
             args.n_shell == 304 && args.value == 0.5 && args.capacity == 10, name + ": counts");
  expect(args.boxes == nullptr && args.base_begin == nullptr && args.shell_begin == nullptr &&
             args.candidate_begin == nullptr && args.candidates == nullptr &&
             args.levels == nullptr && args.shell_value == nullptr &&
             args.shell_sample == nullptr && args.shell_code == nullptr &&
             args.chunk_triangles == nullptr && args.chunk_skipped == nullptr &&
             args.chunk_offset == nullptr && args.counts == nullptr && args.vertices == nullptr &&
             args.levels_out == nullptr && args.samples == nullptr, name + ": an address is set");
  avr::IsoArgs to = plan.args;
  // only box 1's shell has cells of its own or a coarser level: box 0's
  expect_tables(name, plan,
                {{&to.boxes, sizeof(avr::IsoBoxDev), 3},
                 {&to.shell_begin, sizeof(uint64_t), 4},
                 {&to.levels, sizeof(avr::IsoLevelsDev), 1},
                 {&to.base_begin, sizeof(uint32_t), 4},
                 {&to.candidate_begin, sizeof(uint32_t), 4},
                 {&to.candidates, sizeof(int32_t), 1}},
                &to);
  expect_iso_layout(plan.scratch, 304, 1, with_sample);
  expect_iso_layout(avr::iso_scratch(999, 13, !with_sample), 999, 13, !with_sample);
  const avr::IsoPlan lone = avr::plan_isosurface(
      f.data(), with_sample ? s.data() : nullptr, 1, 0.5, kIndexLo, nullptr, kCellSize, kProbLo, 1,
      0, nullptr, nullptr, nullptr, address(53));
  to = lone.args;
  expect(lone.args.capacity == 0 && lone.args.n_bases == 125, name + ": a lone box's counts");
  expect_tables(name + ", a lone box", lone,
                {{&to.boxes, sizeof(avr::IsoBoxDev), 1},
                 {&to.shell_begin, sizeof(uint64_t), 2},
                 {&to.levels, sizeof(avr::IsoLevelsDev), 1},
                 {&to.base_begin, sizeof(uint32_t), 2},
                 {&to.candidate_begin, sizeof(uint32_t), 2},
                 {&to.candidates, sizeof(int32_t), 0}},
                &to);
}

// The locator of the scene: level 0 spans [0, 5] x [0, 3]^2; 64 + 8 * 2 = 80 blocks at the most,
// so blocks of 2^3 cells, 3 x 2 x 2 of them; box 0 meets eight, box 1 one.
void expect_locator(const std::string& name, const avr::StreamLocatorDev& locator, bool cells) {
  const int32_t n[3] = {cells ? 3 : 0, cells ? 2 : 0, cells ? 2 : 0};
  for (int d = 0; d < 3; ++d) {
    expect(locator.origin[d] == 0 && locator.n[d] == n[d], name + ": the locator's blocks");
  }
  expect(locator.shift == (cells ? 1 : 0), name + ": the locator's shift");
}

void test_streamlines(bool cells) {
  const std::string name = cells ? "streamlines" : "streamlines, no boxes";
  const std::vector<avr_box> vx = field(0, cells), vy = field(1, cells), vz = field(2, cells),
                             s = field(3, cells);
  const size_t n = vx.size();
  const avr::StreamPlan plan = avr::plan_streamlines(
      n ? vx.data() : &kNoBox, n ? vy.data() : &kNoBox, n ? vz.data() : &kNoBox,
      n ? s.data() : &kNoBox, n, 7, 0.25, -1, 9, kIndexLo, kRatio, kCellSize, kProbLo, kLevels,
      address(50), address(51), address(52), address(53), address(54));
  const avr::StreamArgs& args = plan.args;
  expect_locator(name, args.locator, cells);
  expect(args.n_levels == 2 && args.n_seeds == 7 && args.max_steps == 9 && args.step == 0.25 &&
             args.direction == -1.0, name + ": counts");
  expect(args.boxes == nullptr && args.block_begin == nullptr && args.block_boxes == nullptr &&
             args.levels == nullptr && args.seeds == nullptr && args.points == nullptr &&
             args.samples == nullptr && args.counts == nullptr && args.status == nullptr,
         name + ": an address is set");
  avr::StreamArgs to = plan.args;
  expect_tables(name, plan,
                {{&to.boxes, sizeof(avr::StreamBoxDev), cells ? 3u : 0u},
                 {&to.levels, sizeof(avr::IsoLevelsDev), 1},
                 {&to.block_begin, sizeof(uint32_t), cells ? 13u : 1u},
                 {&to.block_boxes, sizeof(int32_t), cells ? 9u : 0u}},
                &to);
}

void test_covering_grid(bool cells) {
  const std::string name = cells ? "covering grid" : "covering grid, no boxes";
  const std::vector<avr_box> f = field(0, cells);
  const int32_t lo[3] = {6, 0, 0}, dims[3] = {5, 3, 2};
  const avr::CoveringGridPlan plan = avr::plan_covering_grid(
      cells ? f.data() : &kNoBox, f.size(), 1, lo, dims, kIndexLo, kRatio, kLevels, -7.5,
      address(50), address(51), address(52));
  const avr::CoverArgs& args = plan.args;
  expect(args.level == 1 && args.finest == (cells ? 1 : -1) && args.lo[0] == 6 && args.lo[1] == 0 &&
             args.lo[2] == 0 && args.nx == 5 && args.ny == 3 && args.nz == 2 && args.n_tiles == 1 &&
             args.fill == -7.5, name + ": counts");
  expect(args.boxes == nullptr && args.candidate_begin == nullptr && args.candidates == nullptr &&
             args.levels == nullptr && args.values == nullptr && args.coverage == nullptr &&
             args.cell_level == nullptr, name + ": an address is set");
  avr::CoverArgs to = plan.args;
  // the one tile meets box 0 (level 1's [0, 8)) and box 1
  expect_tables(name, plan,
                {{&to.boxes, sizeof(avr::CoverBoxDev), cells ? 3u : 0u},
                 {&to.levels, sizeof(avr::CoverLevelsDev), 1},
                 {&to.candidate_begin, sizeof(uint32_t), 2},
                 {&to.candidates, sizeof(int32_t), cells ? 2u : 0u}},
                &to);
}

void expect_ray_args(const std::string& name, const avr::RayArgs& args, bool cells,
                     uint64_t n_segments) {
  expect_locator(name, args.locator, cells);
  const int32_t hi[3] = {5, 3, 3};
  for (int d = 0; d < 3; ++d) {
    expect(args.bound_lo[d] == 0 && args.bound_hi[d] == (cells ? hi[d] : -1),
           name + ": the bounding box");
  }
  expect(args.n_levels == 2 && args.n_rays == 11 && args.max_trips == 20 &&
             args.n_segments == n_segments, name + ": counts");
  expect(args.boxes == nullptr && args.block_begin == nullptr && args.block_boxes == nullptr &&
             args.levels == nullptr && args.start == nullptr && args.end == nullptr &&
             args.counts == nullptr && args.status == nullptr && args.span == nullptr &&
             args.offsets == nullptr && args.t0 == nullptr && args.t1 == nullptr &&
             args.level == nullptr && args.value == nullptr && args.integral == nullptr &&
             args.covered == nullptr && args.weight_boxes == nullptr && args.weight == nullptr &&
             args.counted == nullptr, name + ": an address is set");
}

void test_rays(bool cells, bool emit) {
  const std::string name =
      std::string(emit ? "rays, emit pass" : "rays, count pass") + (cells ? "" : ", no boxes");
  const std::vector<avr_box> f = field(0, cells);
  const avr::RayPlan plan = avr::plan_rays(
      cells ? f.data() : &kNoBox, f.size(), 11, 20, kIndexLo, kRatio, kCellSize, kProbLo, kLevels,
      address(50), address(51), emit ? address(52) : nullptr, 33, address(53), address(54),
      address(55), address(56), address(57), address(58), address(59), address(60), address(61));
  expect_ray_args(name, plan.args, cells, emit ? 33 : 0);
  avr::RayArgs to = plan.args;
  expect_tables(name, plan,
                {{&to.boxes, sizeof(avr::CoverBoxDev), cells ? 3u : 0u},
                 {&to.levels, sizeof(avr::IsoLevelsDev), 1},
                 {&to.block_begin, sizeof(uint32_t), cells ? 13u : 1u},
                 {&to.block_boxes, sizeof(int32_t), cells ? 9u : 0u}},
                &to);
}

void test_ray_sums(bool cells, bool weighted) {
  const std::string name = std::string(weighted ? "weighted ray sums" : "ray sums") +
                           (cells ? "" : ", no boxes");
  const std::vector<avr_box> f = field(0, cells), w = field(1, cells);
  const avr::RaySumsPlan plan = avr::plan_ray_sums(
      cells ? f.data() : &kNoBox, f.size(), weighted ? (cells ? w.data() : &kNoBox) : nullptr,
      weighted ? w.size() : 0, 11, 20, kIndexLo, kRatio, kCellSize, kProbLo, kLevels, address(50),
      address(51), address(53), address(54), address(55), address(56),
      weighted ? address(57) : nullptr, address(58), address(59));
  expect_ray_args(name, plan.walk.args, cells, 0);
  avr::RayArgs to = plan.walk.args;
  std::vector<Want> want = {{&to.boxes, sizeof(avr::CoverBoxDev), cells ? 3u : 0u}};
  if (weighted) want.push_back({&to.weight_boxes, sizeof(avr::CoverBoxDev), cells ? 3u : 0u});
  want.push_back({&to.levels, sizeof(avr::IsoLevelsDev), 1});
  want.push_back({&to.block_begin, sizeof(uint32_t), cells ? 13u : 1u});
  want.push_back({&to.block_boxes, sizeof(int32_t), cells ? 9u : 0u});
  expect_tables(name, plan, want, &to);
}

}  // namespace

int main() {
  // the sizing pass on its own: an empty table is one element
  {
    avr::StagingSize size;
    const int32_t* to = nullptr;
    const avr::CoverBoxDev* boxes_to = nullptr;
    size(&to, static_cast<const int32_t*>(nullptr), 0);
    expect(size.bytes == 4 && size.items == 1, "the sizing pass pads an empty table of int32");
    size(&boxes_to, static_cast<const avr::CoverBoxDev*>(nullptr), 0);
    expect(size.bytes == 4 + 48 && size.items == 2, "the sizing pass pads an empty box table");
    size(&to, static_cast<const int32_t*>(nullptr), 5);
    expect(size.bytes == 4 + 48 + 20 && size.items == 3, "the sizing pass counts a table");
  }
  for (const bool flag : {false, true}) {
    test_joint_histogram(flag);
    test_axis_projection(flag);
    test_isosurface(flag);
    test_streamlines(flag);
    test_covering_grid(flag);
    for (const bool other : {false, true}) {
      test_rays(flag, other);
      test_ray_sums(flag, other);
    }
  }
  test_slice();
  test_derive();
  test_gradient();
  test_clumps();
  test_clump_table();
  std::printf("ok\n");
  return 0;
}
