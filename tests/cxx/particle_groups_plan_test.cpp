// The host plans of the particle groups (csrc/avr_field_plans.h: plan_particle_group_cells,
// plan_particle_groups) as a plain C++ program, built with AddressSanitizer and UBSan and without
// HIP: every refusal message and which one wins when several rules are broken, the 2^31, 2^27 and
// 1024 bounds from counts alone (no array is ever allocated or read), the rule h >= b (1 + 2^-10)
// at equality and one ulp below, 2 and 3 cells on a periodic axis, the shared-byte rule to the
// byte, and the launch arguments against values written out by hand.  Prints "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <string>

#include "../../amrvolumerenderer_amd/csrc/avr_field_plans.h"

namespace {

void fail(const std::string& what) {
  std::fprintf(stderr, "FAILED: %s\n", what.c_str());
  std::exit(1);
}
void expect(bool condition, const std::string& what) {
  if (!condition) fail(what);
}
template <class F>
void expect_message(const std::string& message, F&& call) {
  try {
    call();
  } catch (const std::invalid_argument& e) {
    expect(message == e.what(), "expected \"" + message + "\", got \"" + e.what() + "\"");
    return;
  }
  fail("expected \"" + message + "\", but the plan was made");
}
const void* address(uintptr_t a) { return reinterpret_cast<const void*>(a); }
const void* bytes_from(const void* at, long long offset) {
  return reinterpret_cast<const void*>(reinterpret_cast<uintptr_t>(at) +
                                       static_cast<uintptr_t>(offset));
}

// The arguments of both calls; the arrays lie at made-up addresses that nothing reads.
struct Call {
  uint64_t n = 1000, n_inside = 900;
  double b = 0.125;
  double lo[3] = {0.0, -1.0, 2.0}, hi[3] = {4.0, 1.0, 3.0};
  int32_t dims[3] = {16, 8, 4};  // h = 0.25 on every axis
  int32_t periodic[3] = {0, 0, 0};
  int64_t min_members = 20;
  bool has_box = true;
  const void* points = address(uintptr_t{1} << 44);
  const void* order = address(uintptr_t{2} << 44);
  const void* cell_begin = address(uintptr_t{3} << 44);
  const void* cells = address(uintptr_t{4} << 44);
  const void* parent = address(uintptr_t{5} << 44);
  const void* labels = address(uintptr_t{6} << 44);
  const void* sizes = address(uintptr_t{7} << 44);
  const void* totals = address(uintptr_t{8} << 44);
  const void* n_groups = address(uintptr_t{9} << 44);

  avr::ParticleGroupCellsPlan cells_plan() const {
    return avr::plan_particle_group_cells(n, has_box ? lo : nullptr, hi, dims, periodic, points,
                                          cells, parent, totals);
  }
  avr::ParticleGroupsPlan plan() const {
    return avr::plan_particle_groups(n, n_inside, b, has_box ? lo : nullptr, hi, dims, periodic,
                                     min_members, points, order, cell_begin, parent, labels, sizes,
                                     n_groups);
  }
};

const char* kNull = "null argument";
const char* kCount = "n must stay below 2^31";
const char* kInside = "n_inside must not exceed n";
const char* kLength = "the linking length must be finite and positive";
const char* kBox = "lo and hi must be finite with lo < hi";
const char* kDims = "dims must lie in [1, 1024]";
const char* kCells = "the grid must hold fewer than 2^27 cells";
const char* kPeriodic = "a periodic axis needs at least 3 cells";
const char* kWidth = "a cell must be at least (1 + 2^-10) linking lengths wide";
const char* kMembers = "min_members must lie in [1, 2^31)";
const char* kOutputs = "two output arrays overlap";
const char* kCellsInput = "an output array overlaps the points";
const char* kInputs = "an output array overlaps the points, the order or the cell ranges";

const double kInf = std::numeric_limits<double>::infinity();
const double kNan = std::numeric_limits<double>::quiet_NaN();

void each_rule_alone() {
  Call().cells_plan();
  Call().plan();
  // null arrays: the host arrays always, the device arrays with particles
  { Call c; c.has_box = false; expect_message(kNull, [&] { c.cells_plan(); });
    expect_message(kNull, [&] { c.plan(); }); }
  for (int which = 0; which < 4; ++which) {
    Call c;
    (which == 0 ? c.points : which == 1 ? c.cells : which == 2 ? c.parent : c.totals) = nullptr;
    expect_message(kNull, [&] { c.cells_plan(); });
    c.n = 0;
    c.cells_plan();  // all may be null without particles
  }
  for (int which = 0; which < 7; ++which) {
    Call c;
    (which == 0   ? c.points
     : which == 1 ? c.order
     : which == 2 ? c.cell_begin
     : which == 3 ? c.parent
     : which == 4 ? c.labels
     : which == 5 ? c.sizes
                  : c.n_groups) = nullptr;
    expect_message(kNull, [&] { c.plan(); });
    c.n = c.n_inside = 0;
    if (which == 6) {
      expect_message(kNull, [&] { c.plan(); });  // n_groups is set to 0 even then
    } else {
      c.plan();
    }
  }
  { Call c; c.n = c.n_inside = 0; c.points = c.order = c.cell_begin = c.parent = c.labels =
        c.sizes = c.cells = c.totals = nullptr;
    c.cells_plan();
    const avr::ParticleGroupsPlan plan = c.plan();
    expect(plan.args.n == 0 && plan.args.n_chunks == 0, "an empty call has no chunk"); }
  // the count, from the number alone
  { Call c; c.n = uint64_t{1} << 31; expect_message(kCount, [&] { c.cells_plan(); });
    expect_message(kCount, [&] { c.plan(); });
    c.n = (uint64_t{1} << 31) - 1; c.n_inside = c.n; c.cells_plan();
    const avr::ParticleGroupsPlan plan = c.plan();
    expect(plan.args.n == 0x7fffffffu && plan.args.n_chunks == (1u << 23), "2^31 - 1 particles");
    expect(plan.scratch.total == ((size_t{1} << 23) + 1) * 4, "the scratch of 2^23 chunks"); }
  { Call c; c.n_inside = c.n + 1; expect_message(kInside, [&] { c.plan(); });
    c.n_inside = c.n; c.plan(); c.n_inside = 0; c.plan(); }
  for (double b : {0.0, -0.125, kInf, kNan}) {
    Call c; c.b = b; expect_message(kLength, [&] { c.plan(); }); c.cells_plan();
  }
  // the box
  for (int d = 0; d < 3; ++d) {
    for (int which = 0; which < 5; ++which) {
      Call c;
      if (which == 0) c.lo[d] = kNan;
      if (which == 1) c.hi[d] = kInf;
      if (which == 2) c.lo[d] = -kInf;
      if (which == 3) c.hi[d] = c.lo[d];
      if (which == 4) c.hi[d] = std::nextafter(c.lo[d], -kInf);
      expect_message(kBox, [&] { c.cells_plan(); });
      expect_message(kBox, [&] { c.plan(); });
    }
    { Call c; c.lo[d] = -std::numeric_limits<double>::max();
      c.hi[d] = std::numeric_limits<double>::max();  // the extent overflows
      expect_message(kBox, [&] { c.cells_plan(); }); }
  }
  // the dims: 1 .. 1024 each, fewer than 2^27 in all
  for (int d = 0; d < 3; ++d) {
    for (int32_t bad : {0, -1, 1025, INT32_MAX}) {
      Call c; c.dims[d] = bad; c.b = 1e-9;
      expect_message(kDims, [&] { c.cells_plan(); });
      expect_message(kDims, [&] { c.plan(); });
    }
    Call c; c.dims[d] = 1024; c.b = 1e-9; c.cells_plan(); c.plan();
    c.dims[d] = 1; c.cells_plan(); c.plan();
  }
  { Call c; c.b = 1e-9; c.dims[0] = 1024; c.dims[1] = 1024; c.dims[2] = 128;  // 2^27
    expect_message(kCells, [&] { c.cells_plan(); });
    expect_message(kCells, [&] { c.plan(); });
    c.dims[2] = 127; c.cells_plan();
    const avr::ParticleGroupsPlan plan = c.plan();
    expect(plan.args.n_cells == 1024u * 1024u * 127u, "the cells of the largest grid"); }
  // a periodic axis: 2 cells refused, 3 admitted, 1 refused too
  for (int d = 0; d < 3; ++d) {
    Call c; c.periodic[d] = 1; c.b = 1e-9;
    c.dims[d] = 2; expect_message(kPeriodic, [&] { c.cells_plan(); });
    expect_message(kPeriodic, [&] { c.plan(); });
    c.dims[d] = 1; expect_message(kPeriodic, [&] { c.cells_plan(); });
    c.dims[d] = 3; c.cells_plan(); c.plan();
    c.periodic[d] = 0; c.dims[d] = 2; c.cells_plan(); c.plan();
    c.periodic[d] = -7; c.dims[d] = 3;  // any non-zero flag is a flag
    expect(c.plan().args.grid.periodic[d] == 1, "a flag is stored as 1");
  }
  for (int64_t bad : {int64_t{0}, int64_t{-1}, int64_t{1} << 31, INT64_MAX, INT64_MIN}) {
    Call c; c.min_members = bad; expect_message(kMembers, [&] { c.plan(); });
  }
  { Call c; c.min_members = 1; c.plan(); c.min_members = (int64_t{1} << 31) - 1;
    expect(c.plan().args.min_members == 0x7fffffffu, "the largest min_members"); }
}

// h >= b (1 + 2^-10) wherever dims > 1: at equality, one ulp below, and not asked of one cell.
void the_cell_width_rule() {
  for (int d = 0; d < 3; ++d) {
    Call c;
    c.b = 1.0;
    for (int e = 0; e < 3; ++e) { c.lo[e] = 0.0; c.hi[e] = 1024.0; c.dims[e] = 4; }
    c.hi[d] = 4.00390625;  // 4 (1 + 2^-10): h = 1 + 2^-10 exactly
    const avr::ParticleGroupsPlan plan = c.plan();
    expect(plan.args.grid.h[d] == 1.0009765625 && plan.args.b2 == 1.0, "h at equality");
    c.hi[d] = std::nextafter(4.00390625, 0.0);  // h is one ulp below: the division by 4 is exact
    expect(c.hi[d] / 4.0 == std::nextafter(1.0009765625, 0.0), "one ulp below");
    expect_message(kWidth, [&] { c.plan(); });
    c.cells_plan();  // the first call has no linking length and no such rule
    c.dims[d] = 1;   // one cell along the axis: every pair is tested anyway
    c.plan();
    c.hi[d] = 0.001;
    c.plan();
    c.dims[d] = 2;
    expect_message(kWidth, [&] { c.plan(); });
  }
  // b itself, not b (1 + 2^-10), is not enough
  { Call c; c.b = 0.25; expect_message(kWidth, [&] { c.plan(); });
    c.b = 0.25 / 1.0009765625; c.b = std::nextafter(c.b, 0.0); c.plan(); }
}

void which_rule_wins() {
  { Call c; c.points = nullptr; c.n = uint64_t{1} << 31; expect_message(kNull, [&] { c.plan(); });
    expect_message(kNull, [&] { c.cells_plan(); }); }
  { Call c; c.n = uint64_t{1} << 31; c.n_inside = c.n + 1; c.b = -1.0;
    expect_message(kCount, [&] { c.plan(); }); }
  { Call c; c.n_inside = c.n + 1; c.b = -1.0; expect_message(kInside, [&] { c.plan(); }); }
  { Call c; c.b = kNan; c.lo[0] = kNan; expect_message(kLength, [&] { c.plan(); }); }
  { Call c; c.lo[2] = kNan; c.dims[0] = 0; expect_message(kBox, [&] { c.plan(); });
    expect_message(kBox, [&] { c.cells_plan(); }); }
  { Call c; c.dims[2] = 2000; c.dims[0] = 1024; c.dims[1] = 1024; c.periodic[0] = 1;
    expect_message(kDims, [&] { c.plan(); }); }
  { Call c; c.b = 1e-9; c.dims[0] = 1024; c.dims[1] = 1024; c.dims[2] = 128; c.periodic[0] = 1;
    c.dims[0] = 1024; expect_message(kCells, [&] { c.plan(); }); }
  { Call c; c.periodic[1] = 1; c.dims[1] = 2; c.b = 10.0;
    expect_message(kPeriodic, [&] { c.plan(); }); }
  { Call c; c.b = 10.0; c.min_members = 0; expect_message(kWidth, [&] { c.plan(); }); }
  { Call c; c.min_members = 0; c.labels = c.parent; expect_message(kMembers, [&] { c.plan(); }); }
  { Call c; c.labels = c.parent; c.sizes = c.points;
    expect_message(kOutputs, [&] { c.plan(); }); }
}

// An output shares no byte with another output or an input: refused at one shared byte, admitted
// where the arrays touch.
void shared_bytes() {
  const long long n = 1000, cells = 16 * 8 * 4;
  { Call c; c.parent = bytes_from(c.cells, n * 4 - 1); expect_message(kOutputs, [&] { c.cells_plan(); });
    c.parent = bytes_from(c.cells, n * 4); c.cells_plan();
    c.parent = bytes_from(c.cells, -n * 4 + 1); expect_message(kOutputs, [&] { c.cells_plan(); });
    c.parent = bytes_from(c.cells, -n * 4); c.cells_plan(); }
  { Call c; c.totals = bytes_from(c.parent, n * 4 - 1); expect_message(kOutputs, [&] { c.cells_plan(); });
    c.totals = bytes_from(c.parent, n * 4); c.cells_plan();
    c.totals = bytes_from(c.parent, -7); expect_message(kOutputs, [&] { c.cells_plan(); });
    c.totals = bytes_from(c.parent, -8); c.cells_plan(); }
  { Call c; c.cells = bytes_from(c.points, n * 24 - 1); expect_message(kCellsInput, [&] { c.cells_plan(); });
    c.cells = bytes_from(c.points, n * 24); c.cells_plan();
    c.cells = bytes_from(c.points, -n * 4 + 1); expect_message(kCellsInput, [&] { c.cells_plan(); });
    c.cells = bytes_from(c.points, -n * 4); c.cells_plan(); }
  // the groups: outputs parent, labels, sizes (4 n bytes each) and n_groups (8)
  { Call c; c.labels = bytes_from(c.parent, n * 4 - 1); expect_message(kOutputs, [&] { c.plan(); });
    c.labels = bytes_from(c.parent, n * 4); c.plan(); }
  { Call c; c.sizes = bytes_from(c.labels, -n * 4 + 1); expect_message(kOutputs, [&] { c.plan(); });
    c.sizes = bytes_from(c.labels, -n * 4); c.plan(); }
  { Call c; c.n_groups = bytes_from(c.sizes, n * 4 - 1); expect_message(kOutputs, [&] { c.plan(); });
    c.n_groups = bytes_from(c.sizes, n * 4); c.plan(); }
  // inputs: the points (24 n), the order (8 n), the cell ranges (8 (cells + 1))
  { Call c; c.labels = bytes_from(c.points, n * 24 - 1); expect_message(kInputs, [&] { c.plan(); });
    c.labels = bytes_from(c.points, n * 24); c.plan(); }
  { Call c; c.parent = bytes_from(c.order, n * 8 - 1); expect_message(kInputs, [&] { c.plan(); });
    c.parent = bytes_from(c.order, n * 8); c.plan();
    c.parent = bytes_from(c.order, -n * 4 + 1); expect_message(kInputs, [&] { c.plan(); });
    c.parent = bytes_from(c.order, -n * 4); c.plan(); }
  { Call c; c.n_groups = bytes_from(c.cell_begin, (cells + 1) * 8 - 1);
    expect_message(kInputs, [&] { c.plan(); });
    c.n_groups = bytes_from(c.cell_begin, (cells + 1) * 8); c.plan(); }
  // inputs may share bytes with each other
  { Call c; c.order = c.points; c.cell_begin = c.points; c.plan(); }
}

void launch_arguments() {
  Call c;
  c.periodic[1] = 1;
  const avr::ParticleGroupCellsPlan first = c.cells_plan();
  const avr::ParticleGroupsPlan plan = c.plan();
  for (const avr::GroupGridDev* g : {&first.args.grid, &plan.args.grid}) {
    expect(g->lo[0] == 0.0 && g->lo[1] == -1.0 && g->lo[2] == 2.0, "lo");
    expect(g->hi[0] == 4.0 && g->hi[1] == 1.0 && g->hi[2] == 3.0, "hi");
    expect(g->length[0] == 4.0 && g->length[1] == 2.0 && g->length[2] == 1.0, "length");
    expect(g->h[0] == 0.25 && g->h[1] == 0.25 && g->h[2] == 0.25, "h");
    expect(g->top[0] == 15.0 && g->top[1] == 7.0 && g->top[2] == 3.0, "top");
    expect(g->dims[0] == 16 && g->dims[1] == 8 && g->dims[2] == 4, "dims");
    expect(g->periodic[0] == 0 && g->periodic[1] == 1 && g->periodic[2] == 0, "periodic");
  }
  expect(first.args.n == 1000 && first.args.points == nullptr && first.args.cells == nullptr &&
             first.args.parent == nullptr && first.args.totals == nullptr,
         "the first call's arguments: the count, no address");
  expect(plan.args.b2 == 0.015625 && plan.args.n == 1000 && plan.args.n_inside == 900 &&
             plan.args.n_chunks == 4 && plan.args.n_cells == 512 && plan.args.min_members == 20,
         "the second call's counts");
  expect(plan.args.points == nullptr && plan.args.order == nullptr &&
             plan.args.cell_begin == nullptr && plan.args.parent == nullptr &&
             plan.args.labels == nullptr && plan.args.sizes == nullptr &&
             plan.args.chunk_counts == nullptr && plan.args.n_groups == nullptr,
         "the plan leaves every address null");
  expect(plan.scratch.chunk_counts.present && plan.scratch.chunk_counts.offset == 0 &&
             plan.scratch.chunk_counts.bytes == 20 && plan.scratch.total == 20,
         "the scratch: one count per chunk and one to spare");
  { Call d; d.n = 256; d.n_inside = 0; expect(d.plan().args.n_chunks == 1, "256 particles");
    d.n = 257; expect(d.plan().args.n_chunks == 2, "257 particles");
    d.n = 1; expect(d.plan().args.n_chunks == 1, "one particle"); }
  // b2 is b * b rounded once
  { Call d; d.b = 0.1; expect(d.plan().args.b2 == 0.1 * 0.1, "b2"); }
}

}  // namespace

int main() {
  each_rule_alone();
  the_cell_width_rule();
  which_rule_wins();
  shared_bytes();
  launch_arguments();
  std::printf("ok\n");
  return 0;
}
