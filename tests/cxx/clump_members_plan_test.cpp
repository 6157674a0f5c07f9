// The host plans of the clump members (csrc/avr_field_plans.h: plan_clump_members and
// plan_clump_member_data) as a plain C++ program, built with AddressSanitizer and UBSan and
// without HIP: every refusal message and which one wins when several rules are broken, the cell
// ordinals of boxes with and without cells, the 2^31-cell rule from descriptors alone (no cell is
// ever allocated or read), and the launch arguments, the box tables and the order of visit_tables
// against values written out by hand.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../amrvolumerenderer_amd/csrc/avr_field_plans.h"

namespace {

void fail(const std::string& what) {
  std::fprintf(stderr, "FAILED: %s\n", what.c_str());
  std::exit(1);
}
void expect(bool condition, const std::string& what) {
  if (!condition) fail(what);
}

// A scene of descriptors: box b's cells are contiguous at a made-up address that nothing reads.
struct Scene {
  std::vector<avr_box> labels, field;
  std::vector<int32_t> lo;
  std::vector<int32_t> ratio;
  std::vector<double> sizes = {0.5, 0.5, 0.5};
  double prob_lo[3] = {-1.0, 0.0, 2.0};
  uint64_t n_clumps = 5, capacity = 100, n_members = 7;
  int n_levels = 1;
  bool has_field = true;

  void add(int level, int x, int y, int z, int nx, int ny, int nz) {
    const uintptr_t stride = uintptr_t{1} << 31;  // bytes between two boxes: 2^28 cells
    avr_box box{};
    box.dims[0] = nx;
    box.dims[1] = ny;
    box.dims[2] = nz;
    box.level = level;
    box.jstride = nx;
    box.kstride = static_cast<int64_t>(nx) * ny;
    box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 40) + labels.size() * stride);
    labels.push_back(box);
    box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 41) + field.size() * stride);
    field.push_back(box);
    lo.push_back(x);
    lo.push_back(y);
    lo.push_back(z);
  }
  avr::ClumpMembersPlan members() const {
    return avr::plan_clump_members(labels.data(), labels.size(), n_clumps, capacity);
  }
  avr::ClumpMemberDataPlan data() const {
    return avr::plan_clump_member_data(labels.data(), has_field ? field.data() : nullptr,
                                       labels.size(), n_members, lo.data(),
                                       ratio.empty() ? nullptr : ratio.data(), sizes.data(),
                                       prob_lo, n_levels);
  }
};

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

Scene two_levels() {
  Scene s;
  s.n_levels = 2;
  s.ratio = {2};
  s.sizes = {0.5, 0.5, 0.5, 0.25, 0.25, 0.25};
  s.add(0, 0, 0, 0, 4, 4, 4);
  s.add(0, 4, 0, 0, 0, 4, 4);  // no cells
  s.add(1, -16, 0, 8, 6, 8, 2);
  return s;
}

const char* kClumps = "n_clumps must lie in [1, 2^28)";
const char* kCapacity = "capacity must lie in [1, 2^31)";
const char* kMembers = "n_members must stay below 2^31";
const char* kLevels = "n_levels must lie in [1, 16]";
const char* kNull = "null argument";
const char* kDims = "the scenes' boxes differ in dims or level";
const char* kLevel = "a box's level is not below n_levels";
const char* kNoCells = "box has no cell data";
const char* kSpan = "box spans more than 2^28 cells (or has negative strides)";
const char* kTooMany = "scene has too many cells for 32-bit labels";
const char* kRatio = "a level ratio is below 2";
const char* kRange = "a box's index range leaves [-2^30, 2^30)";
const char* kSize = "level_cell_size must be finite and positive";
const char* kOrigin = "prob_lo must be finite";

struct CountTables {
  int tables = 0;
  size_t counts[4] = {0, 0, 0, 0};
  template <class T>
  void operator()(const T** to, const T* host, size_t n) {
    expect(*to == nullptr && host != nullptr, "a table's address starts null");
    counts[tables++] = n;
  }
};

}  // namespace

int main() {
  // ---- plan_clump_members: messages and precedence ----------------------------------------------
  {
    Scene s = two_levels();
    s.n_clumps = 0;
    s.capacity = 0;
    s.labels[0].cells = nullptr;
    expect_message(kClumps, [&] { s.members(); });
    s.n_clumps = uint64_t{1} << 28;
    expect_message(kClumps, [&] { s.members(); });
    s.n_clumps = (uint64_t{1} << 28) - 1;
    expect_message(kCapacity, [&] { s.members(); });
    s.capacity = uint64_t{1} << 31;
    expect_message(kCapacity, [&] { s.members(); });
    s.capacity = (uint64_t{1} << 31) - 1;
    expect_message(kNoCells, [&] { s.members(); });
    s = two_levels();
    s.labels[2].level = 16;
    expect_message(kLevel, [&] { s.members(); });
    s.labels[2].level = 15;  // any level below 16: the members need no level setup
    s.members();
    s = two_levels();
    s.labels[0].jstride = -4;
    expect_message(kSpan, [&] { s.members(); });
  }
  {  // 2^31 cells and one fewer, from descriptors alone: 8 boxes of 2^28, the last one short
    Scene s;
    for (int b = 0; b < 8; ++b) s.add(0, 0, 0, 1024 * b, 1024, 1024, 256);
    expect_message(kTooMany, [&] { s.members(); });
    expect_message(kTooMany, [&] { s.data(); });
    s.labels[7].dims[0] = s.field[7].dims[0] = 1023;
    const avr::ClumpMembersPlan plan = s.members();
    expect(plan.cell_begin.back() == (uint32_t{1} << 31) - 1024u * 256u, "cells below 2^31");
    s.data();
    // the box rules win over the cell count
    s.labels[7].dims[0] = s.field[7].dims[0] = 1024;
    s.labels[3].cells = nullptr;
    expect_message(kNoCells, [&] { s.members(); });
  }
  // ---- plan_clump_members: the tables ------------------------------------------------------------
  {
    const Scene s = two_levels();
    const avr::ClumpMembersPlan plan = s.members();
    expect(plan.args.n_boxes == 3 && plan.args.n_clumps == 5 && plan.args.capacity == 100,
           "members: launch arguments");
    expect(plan.cell_begin == std::vector<uint32_t>({0, 64, 64, 160}), "members: cell_begin");
    expect(plan.tile_begin == std::vector<uint32_t>({0, 1, 1, 3}) && plan.args.n_tiles == 3,
           "members: tile_begin");  // 6 x 8 x 2 cells: two bricks of rows along y
    expect(plan.boxes[0].nx == 4 && plan.boxes[1].nx == 0 && plan.boxes[2].nz == 2 &&
               plan.boxes[2].level == 1 && plan.boxes[2].cells[0] == s.labels[2].cells &&
               plan.boxes[2].jstride[0] == 6 && plan.boxes[2].kstride[0] == 48 &&
               plan.boxes[0].paired == 1,
           "members: boxes");
    expect(plan.args.keys == nullptr && plan.args.cursor == nullptr && plan.args.wanted == nullptr,
           "members: the plan leaves every address null");
    avr::ClumpMembersArgs args = plan.args;
    CountTables count;
    plan.visit_tables(&args, count);
    expect(count.tables == 3 && count.counts[0] == 3 && count.counts[1] == 4 &&
               count.counts[2] == 4, "members: visit_tables");
    Scene odd = two_levels();
    odd.labels[0].cells += 1;  // 8-byte aligned only
    expect(odd.members().boxes[0].paired == 0, "members: an odd address is not paired");
  }
  // ---- plan_clump_member_data: messages and precedence --------------------------------------------
  {
    Scene s = two_levels();
    s.n_members = uint64_t{1} << 31;
    s.n_levels = 17;
    expect_message(kMembers, [&] { s.data(); });
    s.n_members = (uint64_t{1} << 31) - 1;
    expect_message(kLevels, [&] { s.data(); });
    s.n_levels = 0;
    expect_message(kLevels, [&] { s.data(); });
    s.n_levels = 2;
    s.ratio.clear();
    s.field[2].dims[1] = 7;
    expect_message(kNull, [&] { s.data(); });
    s.ratio = {1};
    expect_message(kDims, [&] { s.data(); });
    s.field[2].dims[1] = 8;
    s.field[2].level = 0;
    expect_message(kDims, [&] { s.data(); });
    s.field[2].level = 1;
    s.field[0].cells = nullptr;
    expect_message(kNoCells, [&] { s.data(); });
    s = two_levels();
    s.n_levels = 1;
    s.ratio.clear();
    expect_message(kLevel, [&] { s.data(); });
    s = two_levels();
    s.ratio = {1};
    s.lo[0] = 1 << 30;
    s.sizes[4] = 0.0;
    expect_message(kRatio, [&] { s.data(); });
    s.ratio = {2};
    expect_message(kRange, [&] { s.data(); });
    s.lo[0] = (1 << 30) - 4;
    s.lo[6] = -(1 << 30) - 1;
    expect_message(kRange, [&] { s.data(); });
    s.lo[6] = -(1 << 30);
    expect_message(kSize, [&] { s.data(); });
    s.sizes[4] = 0.25;
    s.prob_lo[1] = std::numeric_limits<double>::infinity();
    expect_message(kOrigin, [&] { s.data(); });
    s.prob_lo[1] = 0.0;
    s.data();
    // a box without cells needs no cells, and its index is not looked at
    s.labels[1].cells = s.field[1].cells = nullptr;
    s.lo[3] = 1 << 30;
    s.data();
  }
  // ---- plan_clump_member_data: the tables ----------------------------------------------------------
  {
    Scene s = two_levels();
    const avr::ClumpMemberDataPlan plan = s.data();
    expect(plan.args.n_boxes == 3 && plan.args.n_cells == 160 && plan.args.n_members == 7,
           "data: launch arguments");
    expect(plan.cell_begin == std::vector<uint32_t>({0, 64, 64, 160}), "data: cell_begin");
    const avr::ClumpMemberBoxDev& fine = plan.boxes[2];
    expect(fine.field == s.field[2].cells && fine.jstride == 6 && fine.kstride == 48 &&
               fine.nx == 6 && fine.ny == 8 && fine.nz == 2 && fine.level == 1 &&
               fine.lo[0] == -16 && fine.lo[1] == 0 && fine.lo[2] == 8,
           "data: the fine box");
    expect(plan.boxes[1].nx == 0 && plan.boxes[1].level == 0, "data: the box without cells");
    expect(plan.levels.cell_size[1][2] == 0.25 && plan.levels.cell_size[0][0] == 0.5 &&
               plan.levels.prob_lo[0] == -1.0 && plan.levels.prob_lo[2] == 2.0,
           "data: the level geometry");
    avr::ClumpMemberDataArgs args = plan.args;
    CountTables count;
    plan.visit_tables(&args, count);
    expect(count.tables == 3 && count.counts[0] == 3 && count.counts[1] == 4 &&
               count.counts[2] == 1, "data: visit_tables");
    s.has_field = false;
    const avr::ClumpMemberDataPlan bare = s.data();
    expect(bare.boxes[0].field == nullptr && bare.boxes[2].field == nullptr &&
               bare.boxes[2].jstride == 0, "data: without a field");
  }
  std::printf("ok\n");
  return 0;
}
