// The host plans of the clumps (csrc/avr_field_plans.h: plan_clumps, plan_clump_table) as a plain
// C++ program, built with AddressSanitizer and UBSan and without HIP: every refusal message and
// which one wins when several rules are broken, cell_begin, the 2^31-cell rule (reached with
// descriptors only: no cell is ever allocated or read), the table's n_clumps * n_levels limit, and
// the candidate lists of all six faces against an enumeration of every ghost cell and its
// ancestors.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../amrvolumerenderer_amd/csrc/avr_field_plans.h"

namespace {

const double kInf = std::numeric_limits<double>::infinity();
const double kNaN = std::numeric_limits<double>::quiet_NaN();

void fail(const std::string& what) {
  std::fprintf(stderr, "FAILED: %s\n", what.c_str());
  std::exit(1);
}
void expect(bool condition, const std::string& what) {
  if (!condition) fail(what);
}

// A scene of descriptors: box b's cells are contiguous at a made-up address that nothing reads.
struct Scene {
  std::vector<avr_box> in, out;
  std::vector<int32_t> lo;
  std::vector<int32_t> ratio;
  double lower = 0.0, upper = 1.0;
  int n_levels = 1;

  void add(int level, int x, int y, int z, int nx, int ny, int nz) {
    const uintptr_t stride = uintptr_t{1} << 31;  // bytes between two boxes: 2^28 cells
    avr_box box{};
    box.dims[0] = nx;
    box.dims[1] = ny;
    box.dims[2] = nz;
    box.level = level;
    box.jstride = nx;
    box.kstride = static_cast<int64_t>(nx) * ny;
    box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 40) + in.size() * stride);
    in.push_back(box);
    box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 41) + out.size() * stride);
    out.push_back(box);
    lo.push_back(x);
    lo.push_back(y);
    lo.push_back(z);
  }
  avr::ClumpPlan plan() const {
    return avr::plan_clumps(in.data(), out.data(), in.size(), lower, upper, lo.data(),
                            ratio.empty() ? nullptr : ratio.data(), n_levels);
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
  return s;
}

const char* kBoundNaN = "a bound is NaN";
const char* kBoundOrder = "lower must not exceed upper";
const char* kLevels = "n_levels must lie in [1, 16]";
const char* kDims = "the scenes' boxes differ in dims or level";
const char* kLevel = "a box's level is not below n_levels";
const char* kNoCells = "box has no cell data";
const char* kSpan = "box spans more than 2^28 cells (or has negative strides)";
const char* kRatio = "a level ratio is below 2";
const char* kRange = "a box's index range leaves [-2^30, 2^30)";
const char* kOverlap = "two boxes of one level overlap in index space";
const char* kShared = "an output box's cells overlap an input box's cells";
const char* kTooMany = "scene has too many cells for 32-bit labels";
const char* kNull = "null argument";

void messages_and_precedence() {
  two_levels().plan();  // in order
  // each rule alone
  { Scene s = two_levels(); s.lower = kNaN; expect_message(kBoundNaN, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.upper = kNaN; expect_message(kBoundNaN, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lower = 2.0; expect_message(kBoundOrder, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lower = kInf; s.upper = -kInf; expect_message(kBoundOrder, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lower = -kInf; s.upper = kInf; s.plan(); }
  { Scene s = two_levels(); s.lower = s.upper = kInf; s.plan(); }
  { Scene s = two_levels(); s.n_levels = 0; expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_levels = 17; s.ratio.assign(16, 2); expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.ratio.clear(); expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.out[1].dims[0] = 3; expect_message(kDims, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.out[2].level = 0; expect_message(kDims, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[2].level = s.out[2].level = 2; expect_message(kLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[0].level = s.out[0].level = -1; expect_message(kLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[1].cells = nullptr; expect_message(kNoCells, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.out[1].kstride = int64_t{1} << 28; expect_message(kSpan, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[1].jstride = -4; expect_message(kSpan, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.ratio[0] = 1; expect_message(kRatio, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[0] = (1 << 30) - 3; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[1] = -(1 << 30) - 1; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[0] = (1 << 30) - 4; s.lo[3] = -(1 << 30); s.plan(); }  // the ends
  { Scene s = two_levels(); s.lo[3] = 3; expect_message(kOverlap, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.out[2].cells = s.in[0].cells + 63; expect_message(kShared, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.out[2].cells = s.in[0].cells + 64; s.plan(); }  // the byte after
  // a box without cells takes no part: null cells, any index
  { Scene s = two_levels(); s.in[1].dims[1] = s.out[1].dims[1] = 0; s.in[1].cells = s.out[1].cells = nullptr;
    s.lo[3] = 0; const avr::ClumpPlan p = s.plan();
    expect(p.cell_begin == std::vector<uint32_t>({0, 64, 64, 448}), "cell_begin with an empty box");
    expect(p.boxes[1].nx == 0 && p.boxes[2].cell_begin == 64, "the empty box's descriptor"); }

  // which rule wins: every earlier rule against every later one that can be broken with it
  { Scene s = two_levels(); s.lower = kNaN; s.n_levels = 0; expect_message(kBoundNaN, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lower = 2.0; s.n_levels = 17; expect_message(kBoundOrder, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_levels = 17; s.out[0].dims[0] = 1; expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.out[2].dims[2] = 1; s.ratio[0] = 0; expect_message(kDims, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[2].level = s.out[2].level = 5; s.ratio[0] = 1; expect_message(kLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.ratio[0] = -2; s.lo[0] = 1 << 30; expect_message(kRatio, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[6] = 1 << 30; s.lo[3] = 0; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[3] = 0; s.out[0].cells = s.in[0].cells; expect_message(kOverlap, [&] { s.plan(); }); }
}

// 1024 x 512 x 512 cells = 2^28 per box, side by side along x
Scene huge(int n_boxes) {
  Scene s;
  for (int b = 0; b < n_boxes; ++b) s.add(0, 1024 * b, 0, 0, 1024, 512, 512);
  return s;
}

void too_many_cells() {
  expect_message(kTooMany, [&] { huge(8).plan(); });
  expect_message(kTooMany, [&] { huge(9).plan(); });
  Scene s = huge(8);  // one row of cells fewer: 2^31 - 2^18 cells
  s.in[7].dims[0] = s.out[7].dims[0] = 1023;
  const avr::ClumpPlan p = s.plan();
  expect(p.cell_begin.size() == 9 && p.cell_begin[7] == 7u << 28 &&
             p.cell_begin[8] == (1u << 31) - (1u << 18), "cell_begin of 2^31 - 2^18 cells");
  expect(p.boxes[7].cell_begin == 7u << 28, "the last box's first ordinal");
  // the shared-byte rule comes first
  Scene t = huge(8);
  t.out[3].cells = t.in[5].cells;
  expect_message(kShared, [&] { t.plan(); });
}

void table_limits() {
  Scene s = two_levels();
  auto table = [&](uint64_t n, int levels, const avr_box* field) {
    return avr::plan_clump_table(s.in.data(), field, s.in.size(), n, levels);
  };
  const avr::ClumpTablePlan p = table(7, 2, s.out.data());
  expect(p.boxes.size() == 3 && p.boxes[2].cells[0] == s.in[2].cells &&
             p.boxes[2].cells[1] == s.out[2].cells && p.boxes[2].level == 1 &&
             p.tile_begin.back() == 1 + 1 + 4, "the table's boxes and tiles");
  expect(table(7, 2, nullptr).boxes[1].cells[1] == s.in[1].cells, "without a field: the labels");
  expect_message("n_clumps must be at least 1", [&] { table(0, 2, nullptr); });
  expect_message(kLevels, [&] { table(1, 0, nullptr); });
  expect_message(kLevels, [&] { table(1, 17, nullptr); });
  const char* limit = "n_clumps * n_levels must stay below 2^28";
  table((uint64_t{1} << 27) - 1, 2, nullptr);
  expect_message(limit, [&] { table(uint64_t{1} << 27, 2, nullptr); });
  table((uint64_t{1} << 24) - 1, 16, nullptr);
  expect_message(limit, [&] { table(uint64_t{1} << 24, 16, nullptr); });
  expect_message(limit, [&] { table(~uint64_t{0}, 2, nullptr); });
  expect_message(limit, [&] { table((uint64_t{1} << 63) + 1, 2, nullptr); });  // the product wraps
  expect_message(kLevel, [&] { table(3, 1, nullptr); });
  std::vector<avr_box> other = s.out;
  other[0].dims[2] = 3;
  expect_message(kDims, [&] { table(3, 2, other.data()); });
  // n_clumps first, then n_levels, then the product, then the boxes
  expect_message("n_clumps must be at least 1", [&] { table(0, 0, other.data()); });
  expect_message(limit, [&] { table(uint64_t{1} << 28, 2, other.data()); });
}

int64_t floor_div(int64_t a, int64_t r) {
  int64_t q = a / r;
  if (a % r != 0 && a < 0) --q;
  return q;
}

// Three levels at ratios 2 and 4, with boxes at negative indices, boxes that touch, a box whose
// face lies on a coarse box's face and a hole.
void candidate_lists() {
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
  const avr::ClumpPlan plan = s.plan();
  const size_t n = s.in.size();
  expect(plan.candidate_begin.size() == 6 * n + 1 && plan.candidate_begin[0] == 0 &&
             plan.candidate_begin.back() == plan.candidates.size(), "the CSR's ends");
  expect(plan.cell_begin.size() == n + 1 && plan.tile_begin.size() == n + 1, "the prefix sums");
  size_t total = 0;
  for (size_t b = 0; b < n; ++b) {
    expect(plan.cell_begin[b] == total && plan.boxes[b].cell_begin == total, "cell_begin");
    total += static_cast<size_t>(plan.boxes[b].nx) * plan.boxes[b].ny * plan.boxes[b].nz;
    for (int d = 0; d < 3 && plan.boxes[b].nx > 0; ++d) {
      expect(plan.boxes[b].lo[d] == s.lo[b * 3 + d], "a box's index");
    }
  }
  expect(plan.cell_begin[n] == total, "the number of cells");
  size_t with_neighbours = 0;
  for (size_t b = 0; b < n; ++b) {
    const avr_box& box = s.in[b];
    for (int face = 0; face < 6; ++face) {
      const int axis = face >> 1, side = face & 1;
      std::set<int32_t> want;
      if (box.dims[0] > 0) {
        int64_t g[3];
        const int u = (axis + 1) % 3, v = (axis + 2) % 3;
        g[axis] = side == 0 ? int64_t{s.lo[b * 3 + axis]} - 1
                            : int64_t{s.lo[b * 3 + axis]} + box.dims[axis];
        for (int a = 0; a < box.dims[u]; ++a) {
          for (int c = 0; c < box.dims[v]; ++c) {
            g[u] = s.lo[b * 3 + u] + a;
            g[v] = s.lo[b * 3 + v] + c;
            int64_t m[3] = {g[0], g[1], g[2]};
            for (int level = box.level; level >= 0; --level) {
              if (level < box.level) {
                for (int d = 0; d < 3; ++d) m[d] = floor_div(m[d], s.ratio[level]);
              }
              for (size_t c2 = 0; c2 < n; ++c2) {
                const avr_box& other = s.in[c2];
                if (c2 == b || other.dims[0] <= 0 || other.level != level) continue;
                bool holds = true;
                for (int d = 0; d < 3; ++d) {
                  holds = holds && m[d] >= s.lo[c2 * 3 + d] &&
                          m[d] < int64_t{s.lo[c2 * 3 + d]} + other.dims[d];
                }
                if (holds) want.insert(static_cast<int32_t>(c2));
              }
            }
          }
        }
      }
      const uint32_t first = plan.candidate_begin[6 * b + face];
      const uint32_t last = plan.candidate_begin[6 * b + face + 1];
      expect(first <= last && last <= plan.candidates.size(), "a CSR range");
      const std::vector<int32_t> got(plan.candidates.begin() + first, plan.candidates.begin() + last);
      expect(got == std::vector<int32_t>(want.begin(), want.end()),
             "the candidates of box " + std::to_string(b) + " face " + std::to_string(face));
      if (!want.empty()) ++with_neighbours;
    }
  }
  expect(with_neighbours >= 20, "the scene has neighbours on many faces");
  // a finer box is never a candidate
  for (size_t b = 0; b < n; ++b) {
    for (uint32_t q = plan.candidate_begin[6 * b]; q < plan.candidate_begin[6 * b + 6]; ++q) {
      expect(s.in[plan.candidates[q]].level <= s.in[b].level, "same or coarser only");
    }
  }
}

}  // namespace

int main() {
  messages_and_precedence();
  too_many_cells();
  table_limits();
  candidate_lists();
  std::puts("ok");
  return 0;
}
