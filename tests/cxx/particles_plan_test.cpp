// The host plans of the particle fields (csrc/avr_field_plans.h: plan_particle_cells,
// plan_particle_deposit) as a plain C++ program, built with AddressSanitizer and UBSan and without
// HIP: every refusal message and which one wins when several rules are broken, the 2^28 and 2^31
// bounds from counts alone (no array is ever allocated or read), the shared-byte rule to the byte,
// and the staged tables -- box table, cell prefix, locator, tile prefix, volumes -- against values
// written out by hand for a three-level scene with a hole and a box without cells.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
const void* bytes_from(const void* at, long offset) {
  return static_cast<const void*>(static_cast<const char*>(at) + offset);
}

// A scene of descriptors: box b's cells are contiguous at a made-up address that nothing reads; so
// are the arrays of a call.
struct Scene {
  std::vector<avr_box> boxes;
  std::vector<int32_t> index;
  std::vector<int32_t> ratio;
  std::vector<double> sizes;
  std::vector<double> origin = {0.0, -1.0, 2.0};
  int n_levels = 1;
  uint64_t n = 10;
  int method = 0, quantity = 0;
  int64_t max_entries = avr::kStreamMaxEntries;
  const void* points = address(uintptr_t{1} << 44);
  const void* values = address(uintptr_t{2} << 44);
  const void* cells = address(uintptr_t{3} << 44);
  const void* shares = address(uintptr_t{4} << 44);
  const void* levels = address(uintptr_t{5} << 44);
  const void* totals = address(uintptr_t{6} << 44);

  void add(int level, int x, int y, int z, int nx, int ny, int nz) {
    const uintptr_t stride = uintptr_t{1} << 31;  // bytes between two boxes: 2^28 cells
    avr_box box{};
    box.dims[0] = nx;
    box.dims[1] = ny;
    box.dims[2] = nz;
    box.level = level;
    box.jstride = nx;
    box.kstride = static_cast<int64_t>(nx) * ny;
    box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 40) + boxes.size() * stride);
    boxes.push_back(box);
    index.push_back(x);
    index.push_back(y);
    index.push_back(z);
  }
  avr::ParticleCellsPlan plan() const {
    return avr::plan_particle_cells(boxes.data(), boxes.size(), n, method,
                                    index.empty() ? nullptr : index.data(),
                                    ratio.empty() ? nullptr : ratio.data(),
                                    sizes.empty() ? nullptr : sizes.data(),
                                    origin.empty() ? nullptr : origin.data(), n_levels, points,
                                    values, cells, shares, levels, totals, max_entries);
  }
  avr::ParticleDepositPlan deposit() const {
    return avr::plan_particle_deposit(boxes.data(), boxes.size(), n, quantity,
                                      sizes.empty() ? nullptr : sizes.data(), n_levels, cells,
                                      shares);
  }
};

// Three levels at ratio 2.  Level 0 leaves the column i = 4 open (a hole); box 2 has no cells; the
// level-1 box lies over the hole and the level-2 box inside it.
Scene three_levels() {
  Scene s;
  s.n_levels = 3;
  s.ratio = {2, 2};
  s.sizes = {0.5, 0.25, 2.0, 0.25, 0.125, 1.0, 0.125, 0.0625, 0.5};
  s.add(0, 0, 0, 0, 4, 4, 4);    // 64 cells
  s.add(0, 5, 0, 0, 3, 4, 4);    // 48
  s.add(1, 0, 0, 0, 0, 3, 3);    // none
  s.add(1, 8, 0, 0, 4, 4, 4);    // 64: level-0 indices 4..5, 0..1, 0..1
  s.add(2, 16, 0, 0, 2, 2, 2);   // 8: level-0 index (4, 0, 0)
  return s;
}

const char* kLevels = "n_levels must lie in [1, 16]";
const char* kNull = "null argument";
const char* kMethod = "method must be 0 (nearest grid point) or 1 (cloud in cell)";
const char* kQuantity = "quantity must be 0 (sum) or 1 (density)";
const char* kCountNgp = "n must stay below 2^31";
const char* kCountCic = "n must stay below 2^28 for cloud in cell";
const char* kCountDeposit = "n_contributions must stay below 2^31";
const char* kSize = "level_cell_size must be finite and positive";
const char* kOrigin = "prob_lo must be finite";
const char* kBoxLevel = "a box's level is not below n_levels";
const char* kNoCells = "box has no cell data";
const char* kSpan = "box spans more than 2^28 cells (or has negative strides)";
const char* kRatio = "a level ratio is below 2";
const char* kRange = "a box's index range leaves [-2^30, 2^30)";
const char* kOverlap = "two boxes of one level overlap in index space";
const char* kCells = "scene has too many cells for 32-bit labels";
const char* kTiles = "scene has too many cells";
const char* kLocator = "the locator's lists hold 2^28 entries or more";
const char* kOutputs = "two output arrays overlap";
const char* kInputs = "an output array overlaps the points or the values";
const char* kDepositShared = "the cells or the shares overlap an output box's cells";

void cells_messages_and_precedence() {
  three_levels().plan();  // in order
  { Scene s = three_levels(); s.method = 1; s.values = nullptr; s.levels = nullptr; s.plan(); }
  // each rule alone
  { Scene s = three_levels(); s.n_levels = 0; expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.n_levels = 17; expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.ratio.clear(); expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.index.clear(); expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.sizes.clear(); expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.origin.clear(); expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.totals = nullptr; expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.points = nullptr; expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.cells = nullptr; expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.shares = nullptr; expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.n = 0; s.points = s.cells = s.shares = nullptr; s.plan();
    s.totals = nullptr; expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.method = 2; expect_message(kMethod, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.method = -1; expect_message(kMethod, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.sizes[4] = 0.0; expect_message(kSize, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.sizes[8] = HUGE_VAL; expect_message(kSize, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.sizes[0] = -0.5; expect_message(kSize, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.origin[1] = std::nan(""); expect_message(kOrigin, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.boxes[4].level = 3; expect_message(kBoxLevel, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.boxes[1].cells = nullptr; expect_message(kNoCells, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.boxes[1].jstride = -4; expect_message(kSpan, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.ratio[1] = 1; expect_message(kRatio, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.index[3] = (1 << 30) - 2; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.index[1] = -(1 << 30) - 1; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.index[3] = 3; expect_message(kOverlap, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.max_entries = 18; expect_message(kLocator, [&] { s.plan(); });
    s.max_entries = 19; s.plan(); }
  // which rule wins: every earlier rule against a later one that can be broken with it
  { Scene s = three_levels(); s.n_levels = 0; s.totals = nullptr; expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.points = nullptr; s.method = 5; expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.method = 5; s.n = uint64_t{1} << 31; expect_message(kMethod, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.n = uint64_t{1} << 31; s.sizes[0] = 0.0; expect_message(kCountNgp, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.sizes[0] = 0.0; s.origin[0] = HUGE_VAL; expect_message(kSize, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.origin[0] = HUGE_VAL; s.boxes[0].level = 7; expect_message(kOrigin, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.boxes[0].level = 7; s.ratio[0] = 1; expect_message(kBoxLevel, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.boxes[0].cells = nullptr; s.ratio[0] = 1; expect_message(kNoCells, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.ratio[0] = 0; s.index[0] = 1 << 30; expect_message(kRatio, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.index[12] = 1 << 30; s.index[3] = 3; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.index[3] = 3; s.max_entries = 1; expect_message(kOverlap, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.max_entries = 1; s.shares = s.cells; expect_message(kLocator, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.shares = s.cells; s.points = s.cells; expect_message(kOutputs, [&] { s.plan(); }); }
}

void deposit_messages_and_precedence() {
  three_levels().deposit();
  { Scene s = three_levels(); s.quantity = 1; s.n = 0; s.cells = s.shares = nullptr; s.deposit(); }
  { Scene s = three_levels(); s.n_levels = 17; expect_message(kLevels, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.sizes.clear(); expect_message(kNull, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.cells = nullptr; expect_message(kNull, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.shares = nullptr; expect_message(kNull, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.quantity = 2; expect_message(kQuantity, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.quantity = -1; expect_message(kQuantity, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.sizes[5] = std::nan(""); expect_message(kSize, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.boxes[3].level = 3; expect_message(kBoxLevel, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.boxes[3].cells = nullptr; expect_message(kNoCells, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.boxes[3].kstride = int64_t{1} << 28; expect_message(kSpan, [&] { s.deposit(); }); }
  // boxes of one level may share indices here: the ordinals alone say where a share goes
  { Scene s = three_levels(); s.index[3] = 3; s.deposit(); }
  { Scene s = three_levels(); s.n_levels = 0; s.sizes.clear(); expect_message(kLevels, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.cells = nullptr; s.quantity = 9; expect_message(kNull, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.quantity = 9; s.n = uint64_t{1} << 31; expect_message(kQuantity, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.n = uint64_t{1} << 31; s.sizes[0] = 0.0; expect_message(kCountDeposit, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.sizes[0] = 0.0; s.boxes[0].level = 4; expect_message(kSize, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.boxes[0].level = 4; s.cells = s.boxes[1].cells; expect_message(kBoxLevel, [&] { s.deposit(); }); }
}

// From counts alone: the arrays are addresses that nothing reads.
void count_and_size_rules() {
  { Scene s = three_levels(); s.n = (uint64_t{1} << 31) - 1; s.plan(); }
  { Scene s = three_levels(); s.n = uint64_t{1} << 31; expect_message(kCountNgp, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.n = UINT64_MAX; expect_message(kCountNgp, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.method = 1; s.n = (uint64_t{1} << 28) - 1; s.plan(); }
  { Scene s = three_levels(); s.method = 1; s.n = uint64_t{1} << 28; expect_message(kCountCic, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.n = (uint64_t{1} << 31) - 1; s.deposit(); }
  { Scene s = three_levels(); s.n = uint64_t{1} << 31; expect_message(kCountDeposit, [&] { s.deposit(); }); }
  // 2^31 cells: eight boxes of 2^28
  { Scene s; s.sizes = {1.0, 1.0, 1.0};
    for (int b = 0; b < 8; ++b) s.add(0, 1024 * b, 0, 0, 1024, 512, 512);
    expect_message(kCells, [&] { s.plan(); });
    expect_message(kCells, [&] { s.deposit(); });
    s.boxes[7].dims[2] = 511; s.boxes[7].kstride = 1024 * 512; s.plan(); s.deposit(); }
  // tiles: a row of one cell takes a tile's row, so a box of 1 x 2^14 x 2^14 cells has 2^24 tiles
  // and 128 of them 2^31 (the tiles are counted box by box, before the cells)
  { Scene s; s.sizes = {1.0, 1.0, 1.0};
    for (int b = 0; b < 128; ++b) s.add(0, b, 0, 0, 1, 1 << 14, 1 << 14);
    expect_message(kTiles, [&] { s.deposit(); }); }
}

void shared_bytes() {
  // ten particles, one entry each: cells and shares 80 bytes, levels 10, totals 16, points 240,
  // values 80
  { Scene s = three_levels(); s.shares = bytes_from(s.cells, 79); expect_message(kOutputs, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.shares = bytes_from(s.cells, 80); s.plan(); }
  { Scene s = three_levels(); s.cells = bytes_from(s.shares, 79); expect_message(kOutputs, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.levels = bytes_from(s.totals, 15); expect_message(kOutputs, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.levels = bytes_from(s.totals, 16); s.plan(); }
  { Scene s = three_levels(); s.totals = bytes_from(s.levels, 9); expect_message(kOutputs, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.totals = bytes_from(s.levels, 10); s.plan(); }
  { Scene s = three_levels(); s.levels = bytes_from(s.cells, -9); expect_message(kOutputs, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.levels = bytes_from(s.cells, -10); s.plan(); }
  { Scene s = three_levels(); s.points = bytes_from(s.cells, -239); expect_message(kInputs, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.points = bytes_from(s.cells, -240); s.plan(); }
  { Scene s = three_levels(); s.points = bytes_from(s.shares, 79); expect_message(kInputs, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.points = bytes_from(s.shares, 80); s.plan(); }
  { Scene s = three_levels(); s.values = bytes_from(s.levels, 9); expect_message(kInputs, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.values = bytes_from(s.levels, 10); s.plan(); }
  { Scene s = three_levels(); s.values = bytes_from(s.totals, -79); expect_message(kInputs, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.values = bytes_from(s.totals, -80); s.plan(); }
  // the points and the values are both read: they may be one array
  { Scene s = three_levels(); s.values = s.points; s.plan(); }
  // levels that are not asked for have no bytes
  { Scene s = three_levels(); s.levels = nullptr; s.values = nullptr; s.plan(); }
  // eight entries each: 640 bytes
  { Scene s = three_levels(); s.method = 1; s.shares = bytes_from(s.cells, 639); expect_message(kOutputs, [&] { s.plan(); }); }
  { Scene s = three_levels(); s.method = 1; s.shares = bytes_from(s.cells, 640); s.plan(); }
  // the deposit: ten contributions against every output box; box 0 holds 64 cells, box 3 holds 64
  { Scene s = three_levels(); s.cells = s.boxes[0].cells + 63; expect_message(kDepositShared, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.cells = s.boxes[0].cells + 64; s.deposit(); }
  { Scene s = three_levels(); s.shares = bytes_from(s.boxes[3].cells, -79); expect_message(kDepositShared, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.shares = bytes_from(s.boxes[3].cells, -80); s.deposit(); }
  { Scene s = three_levels(); s.shares = bytes_from(s.boxes[3].cells, 511); expect_message(kDepositShared, [&] { s.deposit(); }); }
  { Scene s = three_levels(); s.shares = bytes_from(s.boxes[3].cells, 512); s.deposit(); }
  // a strided box: the bytes between its rows count as its own
  { Scene s = three_levels(); s.boxes[0].jstride = 6; s.boxes[0].kstride = 30;  // spans 3 + 18 + 90 + 1 cells
    s.cells = s.boxes[0].cells + 111; expect_message(kDepositShared, [&] { s.deposit(); });
    s.cells = s.boxes[0].cells + 112; s.deposit(); }
  // a box without cells has no bytes; no contributions, no arrays
  { Scene s = three_levels(); s.cells = s.boxes[2].cells; s.deposit(); }
  { Scene s = three_levels(); s.n = 0; s.cells = s.boxes[0].cells; s.deposit(); }
}

struct Seen {
  const void* where;
  const void* table;
  size_t count;
};

void arguments_and_tables() {
  Scene s = three_levels();
  s.method = 1;
  s.n = 77;
  const avr::ParticleCellsPlan p = s.plan();
  const avr::ParticleCellsArgs& a = p.args;
  expect(a.boxes == nullptr && a.cell_begin == nullptr && a.block_begin == nullptr &&
             a.block_boxes == nullptr && a.levels == nullptr && a.points == nullptr &&
             a.values == nullptr && a.cells == nullptr && a.shares == nullptr &&
             a.levels_out == nullptr && a.totals == nullptr, "the plan leaves every address null");
  expect(a.n == 77 && a.n_levels == 3 && a.paired == 1, "the launch arguments");
  { Scene t = s; t.shares = bytes_from(t.shares, 8); expect(t.plan().args.paired == 0, "an odd address"); }
  expect(p.boxes.size() == 5, "one descriptor per box");
  const int want[5][7] = {{4, 4, 4, 0, 0, 0, 0}, {3, 4, 4, 0, 5, 0, 0}, {0, 0, 0, 1, 0, 0, 0},
                          {4, 4, 4, 1, 8, 0, 0}, {2, 2, 2, 2, 16, 0, 0}};
  for (int b = 0; b < 5; ++b) {
    const avr::ParticleBoxDev& box = p.boxes[b];
    expect(box.nx == want[b][0] && box.ny == want[b][1] && box.nz == want[b][2] &&
               box.level == want[b][3] && box.lo[0] == want[b][4] && box.lo[1] == want[b][5] &&
               box.lo[2] == want[b][6], "box " + std::to_string(b));
  }
  expect(p.cell_begin == std::vector<uint32_t>({0, 64, 112, 112, 176, 184}), "the cell prefix");
  // the locator: the level-0 bounding box (0, 0, 0) .. (7, 3, 3), at most 64 + 8 * 4 blocks, so
  // blocks of 2^3 level-0 cells, 4 x 2 x 2 of them; block 2 holds the three boxes around the hole,
  // finest first
  expect(p.locator.origin[0] == 0 && p.locator.origin[1] == 0 && p.locator.origin[2] == 0 &&
             p.locator.n[0] == 4 && p.locator.n[1] == 2 && p.locator.n[2] == 2 &&
             p.locator.shift == 1, "the locator's blocks");
  expect(a.locator.n[0] == 4 && a.locator.shift == 1, "the locator in the launch arguments");
  expect(p.block_begin == std::vector<uint32_t>({0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16,
                                                 17, 18}), "the block prefix");
  expect(p.block_boxes == std::vector<int32_t>({0, 0, 4, 3, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1,
                                                1}), "the block lists");
  expect(p.levels.cell_size[0][0] == 0.5 && p.levels.cell_size[1][1] == 0.125 &&
             p.levels.cell_size[2][2] == 0.5 && p.levels.prob_lo[1] == -1.0 &&
             p.levels.prob_lo[2] == 2.0 && p.levels.ratio[0] == 2 && p.levels.ratio[1] == 2 &&
             p.levels.ratio[2] == 1 && p.levels.ratio[15] == 1, "the level table");
  std::vector<Seen> seen;
  avr::ParticleCellsArgs to = p.args;
  p.visit_tables(&to, [&](auto* where, const auto* table, size_t count) {
    seen.push_back({static_cast<const void*>(where), static_cast<const void*>(table), count});
  });
  expect(seen.size() == 5 && seen[0].where == &to.boxes && seen[0].table == p.boxes.data() &&
             seen[0].count == 5 && seen[1].where == &to.cell_begin &&
             seen[1].table == p.cell_begin.data() && seen[1].count == 6 &&
             seen[2].where == &to.levels && seen[2].table == &p.levels && seen[2].count == 1 &&
             seen[3].where == &to.block_begin && seen[3].table == p.block_begin.data() &&
             seen[3].count == 17 && seen[4].where == &to.block_boxes &&
             seen[4].table == p.block_boxes.data() && seen[4].count == 18,
         "the staged tables of the cells");
  // a scene without cells: a locator of no blocks
  { Scene t; t.sizes = {1.0, 1.0, 1.0}; const avr::ParticleCellsPlan q = t.plan();
    expect(q.locator.n[0] == 0 && q.block_begin == std::vector<uint32_t>({0}) &&
               q.block_boxes.empty() && q.cell_begin == std::vector<uint32_t>({0}),
           "a scene without boxes");
    const avr::ParticleDepositPlan d = t.deposit();
    expect(d.args.n_tiles == 0 && d.args.n_cells == 0, "nothing to clear"); }

  // the deposit
  s.boxes[3].cells += 1;  // an odd address: single cells
  s.quantity = 1;
  const avr::ParticleDepositPlan d = s.deposit();
  const avr::ParticleDepositArgs& e = d.args;
  expect(e.boxes == nullptr && e.tile_begin == nullptr && e.cell_begin == nullptr &&
             e.levels == nullptr && e.cells == nullptr && e.shares == nullptr,
         "the deposit's plan leaves every address null");
  expect(e.n_boxes == 5 && e.n_tiles == 4 && e.n_cells == 184 && e.n == 77,
         "the deposit's launch arguments");
  expect(d.tile_begin == std::vector<uint32_t>({0, 1, 2, 2, 3, 4}), "the tile prefix");
  expect(d.cell_begin == p.cell_begin, "one cell prefix for both calls");
  expect(d.boxes[0].out == s.boxes[0].cells && d.boxes[0].jstride == 4 && d.boxes[0].kstride == 16 &&
             d.boxes[0].nx == 4 && d.boxes[0].level == 0 && d.boxes[0].paired == 1, "box 0: pairs");
  expect(d.boxes[1].jstride == 3 && d.boxes[1].kstride == 12 && d.boxes[1].paired == 0,
         "box 1: odd strides");
  expect(d.boxes[2].out == nullptr && d.boxes[2].nx == 0 && d.boxes[2].level == 1, "box 2: no cells");
  expect(d.boxes[3].out == s.boxes[3].cells && d.boxes[3].paired == 0 && d.boxes[3].level == 1,
         "box 3: an odd address");
  expect(d.boxes[4].nx == 2 && d.boxes[4].nz == 2 && d.boxes[4].level == 2 && d.boxes[4].paired == 1,
         "box 4");
  expect(d.levels.volume[0] == 0.25 && d.levels.volume[1] == 0.03125 &&
             d.levels.volume[2] == 0.00390625 && d.levels.volume[3] == 1.0 &&
             d.levels.volume[15] == 1.0, "(dx * dy) * dz per level");
  seen.clear();
  avr::ParticleDepositArgs into = d.args;
  d.visit_tables(&into, [&](auto* where, const auto* table, size_t count) {
    seen.push_back({static_cast<const void*>(where), static_cast<const void*>(table), count});
  });
  expect(seen.size() == 4 && seen[0].where == &into.boxes && seen[0].count == 5 &&
             seen[1].where == &into.tile_begin && seen[1].count == 6 &&
             seen[2].where == &into.cell_begin && seen[2].table == d.cell_begin.data() &&
             seen[2].count == 6 && seen[3].where == &into.levels && seen[3].table == &d.levels &&
             seen[3].count == 1, "the staged tables of the deposit");
}

}  // namespace

int main() {
  cells_messages_and_precedence();
  deposit_messages_and_precedence();
  count_and_size_rules();
  shared_bytes();
  arguments_and_tables();
  std::puts("ok");
  return 0;
}
