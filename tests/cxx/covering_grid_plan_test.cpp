// The host plan of the covering grids (csrc/avr_field_plans.h: plan_covering_grid) as a plain C++
// program, built with AddressSanitizer and UBSan and without HIP: every refusal message and which
// one wins when several rules are broken, the 2^31 and 2^30 rules (reached with descriptors only:
// no cell is ever allocated or read), the weights w_m, the number of tiles and their decode
// against cell_tile_of for ragged dims, and every tile's candidate list against an enumeration of
// the tile's cells, their ancestors and their descendants.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
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
  std::vector<avr_box> in;
  std::vector<int32_t> index;
  std::vector<int32_t> ratio;
  int n_levels = 1;
  int level = 0;
  int32_t lo[3] = {0, 0, 0};
  int32_t dims[3] = {8, 4, 4};
  // made-up output addresses, far from every box
  const void* values = reinterpret_cast<const void*>(uintptr_t{1} << 44);
  const void* coverage = reinterpret_cast<const void*>(uintptr_t{1} << 45);
  const void* cell_level = reinterpret_cast<const void*>(uintptr_t{1} << 46);

  void add(int box_level, int x, int y, int z, int nx, int ny, int nz) {
    const uintptr_t stride = uintptr_t{1} << 31;  // bytes between two boxes: 2^28 cells
    avr_box box{};
    box.dims[0] = nx;
    box.dims[1] = ny;
    box.dims[2] = nz;
    box.level = box_level;
    box.jstride = nx;
    box.kstride = static_cast<int64_t>(nx) * ny;
    box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 40) + in.size() * stride);
    in.push_back(box);
    index.push_back(x);
    index.push_back(y);
    index.push_back(z);
  }
  void region(int x, int y, int z, int nx, int ny, int nz) {
    lo[0] = x;
    lo[1] = y;
    lo[2] = z;
    dims[0] = nx;
    dims[1] = ny;
    dims[2] = nz;
  }
  avr::CoveringGridPlan plan() const {
    return avr::plan_covering_grid(in.data(), in.size(), level, lo, dims,
                                   index.empty() ? nullptr : index.data(),
                                   ratio.empty() ? nullptr : ratio.data(), n_levels, /*fill=*/0.0,
                                   values, coverage, cell_level);
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
  s.add(0, 0, 0, 0, 4, 4, 4);
  s.add(0, 4, 0, 0, 4, 4, 4);
  s.add(1, 16, 0, 0, 6, 8, 8);
  return s;  // the region: 8 x 4 x 4 cells of level 0, 128 cells
}

const char* kLevels = "n_levels must lie in [1, 16]";
const char* kLevel = "level must lie in [0, n_levels)";
const char* kNull = "null argument";
const char* kBoxLevel = "a box's level is not below n_levels";
const char* kNoCells = "box has no cell data";
const char* kSpan = "box spans more than 2^28 cells (or has negative strides)";
const char* kRatio = "a level ratio is below 2";
const char* kRange = "a box's index range leaves [-2^30, 2^30)";
const char* kOverlap = "two boxes of one level overlap in index space";
const char* kDims = "dims must be at least 1";
const char* kRegion = "the region leaves [-2^30, 2^30) at its level or at the finest loaded one";
const char* kCells = "the region has 2^31 cells or more";
const char* kShared = "an output array overlaps an input box's cells";

void messages_and_precedence() {
  two_levels().plan();  // in order
  // each rule alone
  { Scene s = two_levels(); s.n_levels = 0; expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_levels = 17; s.ratio.assign(16, 2); expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.level = -1; expect_message(kLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.level = 2; expect_message(kLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.level = 1; s.plan(); }
  { Scene s = two_levels(); s.ratio.clear(); expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.index.clear(); expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[2].level = 2; expect_message(kBoxLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[0].level = -1; expect_message(kBoxLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[1].cells = nullptr; expect_message(kNoCells, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[1].kstride = int64_t{1} << 28; expect_message(kSpan, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[1].jstride = -4; expect_message(kSpan, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.ratio[0] = 1; expect_message(kRatio, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.index[0] = (1 << 30) - 3; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.index[1] = -(1 << 30) - 1; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.index[3] = 3; expect_message(kOverlap, [&] { s.plan(); }); }
  for (int d = 0; d < 3; ++d) {
    { Scene s = two_levels(); s.dims[d] = 0; expect_message(kDims, [&] { s.plan(); }); }
    { Scene s = two_levels(); s.dims[d] = -5; expect_message(kDims, [&] { s.plan(); }); }
  }
  // a finer level than any box: n_levels counts it, and a third level needs its ratio
  { Scene s = two_levels(); s.n_levels = 3; s.ratio = {2, 2}; s.level = 2; s.plan(); }
  // every output against the cells: the last byte in, the byte after out
  { Scene s = two_levels(); s.values = s.in[0].cells + 63; expect_message(kShared, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.values = s.in[0].cells + 64; s.plan(); }
  { Scene s = two_levels(); s.values = s.in[2].cells - 128; s.plan(); }  // 128 cells end before
  { Scene s = two_levels(); s.values = s.in[2].cells - 127; expect_message(kShared, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.coverage = s.in[1].cells - 128; s.plan(); }
  { Scene s = two_levels(); s.coverage = s.in[1].cells - 127; expect_message(kShared, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.coverage = s.in[2].cells + 383; expect_message(kShared, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.cell_level = reinterpret_cast<const char*>(s.in[1].cells) - 128; s.plan(); }
  { Scene s = two_levels(); s.cell_level = reinterpret_cast<const char*>(s.in[1].cells) - 127;
    expect_message(kShared, [&] { s.plan(); }); }
  // an output that is not asked for is not looked at
  { Scene s = two_levels(); s.coverage = s.cell_level = nullptr; s.plan(); }
  // a box without cells takes no part: null cells, any index
  { Scene s = two_levels(); s.in[1].dims[1] = 0; s.in[1].cells = nullptr; s.index[3] = 0;
    const avr::CoveringGridPlan p = s.plan();
    expect(p.boxes[1].nx == 0 && p.finest == 1, "the empty box's descriptor");
    expect(p.candidates == std::vector<int32_t>({0}), "an empty box is no candidate"); }
  // no box at all: every cell is absent
  { Scene s; s.region(-3, 2, 5, 130, 5, 1); const avr::CoveringGridPlan p = s.plan();
    expect(p.finest == -1 && p.candidates.empty() &&
               p.candidate_begin == std::vector<uint32_t>(2 * 2 * 1 + 1, 0u), "a scene without boxes"); }

  // which rule wins: every earlier rule against a later one that can be broken with it
  { Scene s = two_levels(); s.n_levels = 0; s.level = -1; expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.level = 2; s.in[2].level = 5; expect_message(kLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[2].level = 5; s.ratio[0] = 1; expect_message(kBoxLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[0].cells = nullptr; s.ratio[0] = 1; expect_message(kNoCells, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.ratio[0] = -2; s.index[0] = 1 << 30; expect_message(kRatio, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.index[6] = 1 << 30; s.index[3] = 0; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.index[3] = 0; s.dims[0] = 0; expect_message(kOverlap, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.dims[2] = 0; s.lo[0] = 1 << 30; expect_message(kDims, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.region(1 << 29, 0, 0, 2048, 1024, 1024); expect_message(kRegion, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.region(0, 0, 0, 2048, 1024, 1024); s.values = s.in[0].cells;
    expect_message(kCells, [&] { s.plan(); }); }
}

// The 2^30 rule at the region's own level and at the finest loaded one, the 2^31 rule: all from
// the numbers alone.
void index_and_size_rules() {
  const int32_t top = 1 << 30;
  // at the region's level (one level, or the region's level is the finest)
  { Scene s; s.region(top - 1, -top, 0, 1, 1, 1); s.plan(); }
  { Scene s; s.region(top - 1, 0, 0, 2, 1, 1); expect_message(kRegion, [&] { s.plan(); }); }
  { Scene s; s.region(0, -top - 1, 0, 1, 1, 1); expect_message(kRegion, [&] { s.plan(); }); }
  { Scene s; s.region(0, 0, INT32_MAX, 1, 1, 1); expect_message(kRegion, [&] { s.plan(); }); }
  { Scene s; s.region(0, 0, INT32_MAX - 1, 1, 1, INT32_MAX); expect_message(kRegion, [&] { s.plan(); }); }
  { Scene s; s.region(INT32_MIN, 0, 0, INT32_MAX, 1, 1); expect_message(kRegion, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.level = 1; s.region(top - 1, 0, 0, 1, 1, 1); s.plan(); }
  // multiplied up to the finest loaded level: a level-1 box under a level-0 region
  { Scene s = two_levels(); s.region(top / 2 - 1, -top / 2, 0, 1, 1, 1); s.plan(); }
  { Scene s = two_levels(); s.region(top / 2, 0, 0, 1, 1, 1); expect_message(kRegion, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.region(0, -top / 2 - 1, 0, 1, 1, 1); expect_message(kRegion, [&] { s.plan(); }); }
  // ... but not to a level that no box with cells has
  { Scene s = two_levels(); s.in[2].dims[0] = 0; s.region(top / 2, 0, 0, 1, 1, 1); s.plan(); }
  // sixteen levels at a ratio of 2^30: the factor is far past 64 bits, and nothing overflows
  { Scene s; s.n_levels = 16; s.ratio.assign(15, top); s.add(0, 0, 0, 0, 2, 2, 2); s.add(15, 0, 0, 0, 4, 4, 4);
    s.region(0, 0, 0, 1, 1, 1); expect_message(kRegion, [&] { s.plan(); });
    s.region(-1, 0, 0, 1, 1, 1); expect_message(kRegion, [&] { s.plan(); });
    s.level = 15; s.region(-top, -top, top - 3, 3, 2, 3); const avr::CoveringGridPlan p = s.plan();
    expect(p.candidates.empty(), "a level-0 box at a factor past 64 bits meets no far tile");
    s.region(-1, -1, -1, 2, 2, 2); const avr::CoveringGridPlan q = s.plan();
    expect(q.candidates == std::vector<int32_t>({0, 1}), "... and holds the cells next to the origin"); }
  { Scene s; s.n_levels = 3; s.ratio = {top, 2}; s.add(1, 0, 0, 0, 4, 4, 4);
    s.region(0, 0, 0, 1, 1, 1); const avr::CoveringGridPlan p = s.plan();  // R_1 = 2^30 exactly
    expect(p.levels.refine[1] == top && p.levels.weight[1] == 0x1p-90, "R = 2^30 and w = 2^-90"); }
  // 2^31 cells
  { Scene s; s.region(0, 0, 0, 2048, 1024, 1024); expect_message(kCells, [&] { s.plan(); }); }
  { Scene s; s.region(0, 0, 0, 1 << 16, 1 << 16, 1); expect_message(kCells, [&] { s.plan(); }); }
  { Scene s; s.region(-5, 0, 0, 1 << 20, 1 << 20, 1 << 20); expect_message(kCells, [&] { s.plan(); }); }
  { Scene s; s.region(0, 0, 0, 1, 1 << 16, 1 << 15); expect_message(kCells, [&] { s.plan(); }); }
  { Scene s; s.region(0, 0, 0, 2047, 1024, 1024); const avr::CoveringGridPlan p = s.plan();
    expect(p.candidate_begin.size() == size_t{16} * 256 * 256 + 1 && p.candidate_begin.back() == 0,
           "the tiles of 2^31 - 2^20 cells"); }
}

void weights() {
  Scene s;
  s.n_levels = 3;
  s.ratio = {2, 2};
  s.add(0, 0, 0, 0, 4, 4, 4);
  s.add(1, 2, 2, 2, 4, 4, 4);
  s.add(2, 6, 6, 6, 4, 4, 4);
  { const avr::CoveringGridPlan p = s.plan();
    expect(p.finest == 2 && p.levels.weight[0] == 0.0 && p.levels.weight[1] == 0.125 &&
               p.levels.weight[2] == 0.015625 && p.levels.weight[3] == 0.0, "w at ratios 2, 2");
    expect(p.levels.refine[0] == 1 && p.levels.refine[1] == 2 && p.levels.refine[2] == 4 &&
               p.levels.refine[3] == 1, "R at ratios 2, 2");
    expect(p.levels.ratio[0] == 2 && p.levels.ratio[1] == 2 && p.levels.ratio[2] == 1, "the ratios"); }
  { Scene t = s; t.level = 1; const avr::CoveringGridPlan p = t.plan();
    expect(p.levels.weight[1] == 0.0 && p.levels.weight[2] == 0.125 && p.levels.refine[2] == 2,
           "w from level 1 on"); }
  { Scene t = s; t.level = 2; const avr::CoveringGridPlan p = t.plan();
    expect(p.levels.weight[1] == 0.0 && p.levels.weight[2] == 0.0, "no finer level"); }
  { Scene t = s; t.in[2].dims[2] = 0; const avr::CoveringGridPlan p = t.plan();
    expect(p.finest == 1 && p.levels.weight[1] == 0.125 && p.levels.weight[2] == 0.0,
           "a level without cells has no weight"); }
  { Scene t = s; t.ratio = {4, 3}; const avr::CoveringGridPlan p = t.plan();
    expect(p.levels.weight[1] == 0.015625 && p.levels.refine[1] == 4 && p.levels.refine[2] == 12 &&
               p.levels.weight[2] == 1.0 / 1728.0, "w at ratios 4 and 3"); }
}

int64_t floor_div(int64_t a, int64_t r) {
  int64_t q = a / r;
  if (a % r != 0 && a < 0) --q;
  return q;
}

// Three levels at ratios 2 and 4, with boxes at negative indices, boxes that touch, a hole and a
// box without cells (isosurface_plan_test's scene).
Scene hierarchy() {
  Scene s;
  s.n_levels = 3;
  s.ratio = {2, 4};
  s.add(0, -4, -2, -2, 4, 4, 4);
  s.add(0, 0, -2, -2, 3, 4, 4);
  s.add(0, 4, -2, -2, 2, 4, 4);    // a hole at i = 3
  s.add(1, -3, -1, 0, 5, 3, 2);
  s.add(1, 2, -1, 0, 4, 3, 2);
  s.add(1, -8, 4, 0, 6, 2, 2);     // on top of box 0's high-y face
  s.add(2, -12, -4, 0, 8, 8, 4);
  s.add(2, -4, -4, 0, 9, 5, 3);
  s.add(0, 0, 0, 0, 0, 3, 3);      // no cells
  s.add(1, 2, 2, 2, 2, 1, 1);
  return s;
}

// Whether box c holds the level-`level` cell g, an ancestor of it or a descendant of it.
bool related(const Scene& s, size_t c, int level, const int64_t g[3]) {
  const avr_box& box = s.in[c];
  if (box.dims[0] <= 0 || box.dims[1] <= 0 || box.dims[2] <= 0) return false;
  for (int d = 0; d < 3; ++d) {
    int64_t first = g[d], last = g[d];  // the cell at the box's level: one index, or a range
    for (int m = level; m > box.level; --m) first = last = floor_div(first, s.ratio[m - 1]);
    for (int m = level; m < box.level; ++m) {
      first = first * s.ratio[m];
      last = last * s.ratio[m] + (s.ratio[m] - 1);
    }
    const int64_t lo = s.index[c * 3 + d], hi = lo + box.dims[d] - 1;
    if (last < lo || first > hi) return false;
  }
  return true;
}

// Every tile's list against the enumeration; returns how many lists hold a box.
size_t check_lists(const Scene& s) {
  const avr::CoveringGridPlan plan = s.plan();
  const int nx = s.dims[0], ny = s.dims[1], nz = s.dims[2];
  const uint32_t tiles = avr::cell_tiles(nx, ny, nz);
  expect(tiles == static_cast<uint32_t>(((nx + 127) / 128) * ((ny + 3) / 4) * ((nz + 3) / 4)),
         "the number of tiles");
  expect(plan.candidate_begin.size() == size_t{tiles} + 1 && plan.candidate_begin[0] == 0 &&
             plan.candidate_begin.back() == plan.candidates.size(), "the CSR's ends");
  std::vector<std::set<int32_t>> want(tiles);
  size_t cells = 0, filled = 0;
  for (uint32_t t = 0; t < tiles; ++t) {
    const avr::CellTile at = avr::cell_tile_of(nx, ny, t);
    for (int k = at.bk * 4; k < at.bk * 4 + 4 && k < nz; ++k) {
      for (int j = at.bj * 4; j < at.bj * 4 + 4 && j < ny; ++j) {
        for (int i = at.chunk * 128; i < at.chunk * 128 + 128 && i < nx; ++i) {
          ++cells;
          const int64_t g[3] = {int64_t{s.lo[0]} + i, int64_t{s.lo[1]} + j, int64_t{s.lo[2]} + k};
          for (size_t c = 0; c < s.in.size(); ++c) {
            if (related(s, c, s.level, g)) want[t].insert(static_cast<int32_t>(c));
          }
        }
      }
    }
    const uint32_t first = plan.candidate_begin[t], last = plan.candidate_begin[t + 1];
    expect(first <= last && last <= plan.candidates.size(), "a CSR range");
    const std::vector<int32_t> got(plan.candidates.begin() + first, plan.candidates.begin() + last);
    expect(got == std::vector<int32_t>(want[t].begin(), want[t].end()),
           "the candidates of tile " + std::to_string(t) + " at level " + std::to_string(s.level));
    if (!got.empty()) ++filled;
  }
  expect(cells == static_cast<size_t>(nx) * ny * nz, "the tiles hold every cell once");
  for (size_t b = 0; b < s.in.size(); ++b) {
    if (s.in[b].dims[0] <= 0) continue;
    for (int d = 0; d < 3; ++d) expect(plan.boxes[b].lo[d] == s.index[b * 3 + d], "a box's index");
  }
  return filled;
}

void tile_candidates() {
  // the whole hierarchy and a margin on every side, at every level
  { Scene s = hierarchy(); s.level = 0; s.region(-6, -4, -4, 13, 9, 8); expect(check_lists(s) >= 4, "level 0"); }
  { Scene s = hierarchy(); s.level = 1; s.region(-11, -6, -7, 24, 15, 14); expect(check_lists(s) >= 8, "level 1"); }
  { Scene s = hierarchy(); s.level = 2; s.region(-40, -20, -20, 95, 50, 40); expect(check_lists(s) >= 40, "level 2"); }
  // a region apart from every box
  { Scene s = hierarchy(); s.level = 1; s.region(40, 40, 40, 5, 5, 5); expect(check_lists(s) == 0, "apart"); }
  // ragged dims: 1, 127, 128, 129 cells along x, 1, 4, 5 along y and z
  for (int nx : {1, 127, 128, 129}) {
    for (int ny : {1, 4, 5}) {
      for (int nz : {1, 4, 5}) {
        Scene s = hierarchy();
        s.level = 2;
        s.region(-100, -3, -2, nx, ny, nz);
        check_lists(s);
        s.level = 0;
        s.region(-125, -1, -3, nx, ny, nz);
        check_lists(s);
      }
    }
  }
}

}  // namespace

int main() {
  messages_and_precedence();
  index_and_size_rules();
  weights();
  tile_candidates();
  std::puts("ok");
  return 0;
}
