// The host plan of the clump links (csrc/avr_field_plans.h: plan_clump_links) as a plain C++
// program, built with AddressSanitizer and UBSan and without HIP: every refusal message and which
// one wins when several rules are broken, the refined first cell and R_l of every box for ratios
// (2, 2) and (2, 4) with negative indices, the refined-extent rule at its limit and one past it
// (from descriptors alone: no cell is ever allocated or read), n_parents against the presence of a
// parent scene, and the launch arguments and the order of visit_tables against values written out
// by hand.  Prints "ok".
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

// A scene of descriptors: box b's cells are contiguous at a made-up address that nothing reads.
struct Scene {
  std::vector<avr_box> labels, parents;
  std::vector<int32_t> lo;
  std::vector<int32_t> ratio;
  uint64_t n_clumps = 5, n_parents = 3;
  int n_levels = 1;
  bool has_parents = true;

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
    box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 41) + parents.size() * stride);
    parents.push_back(box);
    lo.push_back(x);
    lo.push_back(y);
    lo.push_back(z);
  }
  avr::ClumpLinksPlan plan() const {
    return avr::plan_clump_links(labels.data(), has_parents ? parents.data() : nullptr,
                                 labels.size(), n_clumps, has_parents ? n_parents : 0, lo.data(),
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

const char* kClumps = "n_clumps must lie in [1, 2^28)";
const char* kParents = "n_parents must lie in [1, 2^28)";
const char* kNoParents = "without a parent scene n_parents must be 0";
const char* kLevels = "n_levels must lie in [1, 16]";
const char* kDims = "the scenes' boxes differ in dims or level";
const char* kLevel = "a box's level is not below n_levels";
const char* kNoCells = "box has no cell data";
const char* kSpan = "box spans more than 2^28 cells (or has negative strides)";
const char* kRatio = "a level ratio is below 2";
const char* kRange = "a box's index range leaves [-2^30, 2^30)";
const char* kRefined = "a box's refined index range leaves [-2^30, 2^30)";
const char* kNull = "null argument";

void messages_and_precedence() {
  two_levels().plan();  // in order
  // each rule alone
  { Scene s = two_levels(); s.n_clumps = 0; expect_message(kClumps, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_clumps = uint64_t{1} << 28; expect_message(kClumps, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_clumps = ~uint64_t{0}; expect_message(kClumps, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_clumps = (uint64_t{1} << 28) - 1; s.plan(); }
  { Scene s = two_levels(); s.n_parents = 0; expect_message(kParents, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_parents = uint64_t{1} << 28; expect_message(kParents, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_parents = (uint64_t{1} << 28) - 1; s.plan(); }
  { Scene s = two_levels(); s.n_levels = 0; expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_levels = 17; s.ratio.assign(16, 2); expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.ratio.clear(); expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.labels[2].level = s.parents[2].level = 2; expect_message(kLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.labels[0].level = s.parents[0].level = -1; expect_message(kLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.labels[1].cells = nullptr; expect_message(kNoCells, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.labels[1].kstride = int64_t{1} << 28; expect_message(kSpan, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.labels[1].jstride = -4; expect_message(kSpan, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.ratio[0] = 1; expect_message(kRatio, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[6] = (1 << 30) - 5; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[7] = -(1 << 30) - 1; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[0] = 1 << 29; expect_message(kRefined, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.parents[1].dims[0] = 3; expect_message(kDims, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.parents[2].level = 0; expect_message(kDims, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.parents[1].cells = nullptr; expect_message(kNoCells, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.parents[1].jstride = -4; expect_message(kSpan, [&] { s.plan(); }); }
  // a box without cells takes no part: null cells, any index
  { Scene s = two_levels(); s.labels[1].dims[1] = s.parents[1].dims[1] = 0;
    s.labels[1].cells = s.parents[1].cells = nullptr; s.lo[3] = 1 << 30;
    const avr::ClumpLinksPlan p = s.plan();
    expect(p.boxes[1].nx == 0 && p.refined[1].scale == 0 && p.refined[1].lo[0] == 0 &&
               p.tile_begin == std::vector<uint32_t>({0, 1, 1, 5}), "the empty box's entries"); }

  // which rule wins: every earlier rule against a later one broken with it
  { Scene s = two_levels(); s.n_clumps = 0; s.n_parents = 0; expect_message(kClumps, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_parents = 0; s.n_levels = 0; expect_message(kParents, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_levels = 17; s.labels[0].cells = nullptr; expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.labels[1].cells = nullptr; s.ratio[0] = 0; expect_message(kNoCells, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.labels[2].level = s.parents[2].level = 5; s.ratio[0] = 1; expect_message(kLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.ratio[0] = -2; s.lo[0] = 1 << 30; expect_message(kRatio, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[6] = 1 << 30; s.lo[0] = 1 << 29; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[0] = 1 << 29; s.parents[1].dims[0] = 3; expect_message(kRefined, [&] { s.plan(); }); }
  // the parents' boxes come last: a broken ratio is reported before a parent box that differs
  { Scene s = two_levels(); s.parents[2].dims[2] = 1; s.ratio[0] = 0; expect_message(kRatio, [&] { s.plan(); }); }
}

void parents_and_their_count() {
  Scene s = two_levels();
  s.has_parents = false;
  const avr::ClumpLinksPlan p = s.plan();  // no scene, n_parents 0
  expect(p.args.n_parents == 0 && p.boxes[1].cells[1] == s.labels[1].cells,
         "without a parent scene field 1 is the labels");
  expect_message(kNoParents, [&] {
    avr::plan_clump_links(s.labels.data(), nullptr, s.labels.size(), 5, 3, s.lo.data(),
                          s.ratio.data(), 2);
  });
  expect_message(kParents, [&] {
    avr::plan_clump_links(s.labels.data(), s.parents.data(), s.labels.size(), 5, 0, s.lo.data(),
                          s.ratio.data(), 2);
  });
  // n_clumps still comes first
  expect_message(kClumps, [&] {
    avr::plan_clump_links(s.labels.data(), nullptr, s.labels.size(), 0, 3, s.lo.data(),
                          s.ratio.data(), 2);
  });
}

// Three levels with boxes at negative indices: the finest-level index of every box's first cell and
// R_l, for ratios (2, 2) and (2, 4).
void refined_boxes() {
  for (int last : {2, 4}) {
    Scene s;
    s.n_levels = 3;
    s.ratio = {2, last};
    s.add(0, -4, -2, -3, 4, 4, 4);
    s.add(1, -3, -1, 0, 5, 3, 2);
    s.add(2, -12, -4, 7, 8, 8, 4);
    s.add(1, 5, 0, -7, 1, 1, 1);
    const avr::ClumpLinksPlan p = s.plan();
    const int r0 = 2 * last, r1 = last;
    const int32_t want[4][4] = {{-4 * r0, -2 * r0, -3 * r0, r0},
                                {-3 * r1, -1 * r1, 0, r1},
                                {-12, -4, 7, 1},
                                {5 * r1, 0, -7 * r1, r1}};
    for (int b = 0; b < 4; ++b) {
      expect(p.refined[b].lo[0] == want[b][0] && p.refined[b].lo[1] == want[b][1] &&
                 p.refined[b].lo[2] == want[b][2] && p.refined[b].scale == want[b][3],
             "the refined box " + std::to_string(b) + " at ratios (2, " + std::to_string(last) + ")");
    }
  }
  // one level: R = 1 and the index itself
  Scene s;
  s.add(0, -7, 3, 0, 2, 2, 2);
  const avr::ClumpLinksPlan p = s.plan();
  expect(p.refined[0].scale == 1 && p.refined[0].lo[0] == -7 && p.refined[0].lo[1] == 3, "one level");
}

// The refined extent I R_l .. (I + n) R_l - 1 at the ends of [-2^30, 2^30) and one past them.
void refined_limits() {
  const int32_t half = 1 << 30;
  {  // ratio 4: a level-0 box whose last cell's high end is 2^30 - 1, and one cell further
    Scene s;
    s.n_levels = 2;
    s.ratio = {4};
    s.add(0, half / 4 - 3, 0, 0, 3, 1, 1);
    s.add(0, 0, -half / 4, 0, 1, 2, 1);  // the low end exactly -2^30
    const avr::ClumpLinksPlan p = s.plan();
    expect(p.refined[0].lo[0] == half - 12 && p.refined[1].lo[1] == -half, "the ends are kept");
    s.lo[0] += 1;
    expect_message(kRefined, [&] { s.plan(); });
    s.lo[0] -= 1;
    s.lo[4] -= 1;
    expect_message(kRefined, [&] { s.plan(); });
    s.lo[4] += 1;
    s.labels[0].dims[0] = s.parents[0].dims[0] = 4;  // one cell more
    expect_message(kRefined, [&] { s.plan(); });
  }
  {  // a finest-level box is held by the index rule alone
    Scene s;
    s.n_levels = 2;
    s.ratio = {4};
    s.add(1, half - 4, -half, 0, 4, 1, 1);
    s.plan();
    s.lo[0] += 1;
    expect_message(kRange, [&] { s.plan(); });
  }
  {  // ratios whose product passes 32 bits: a box of level 0 with a cell cannot fit, one without
     // cells is not looked at
    Scene s;
    s.n_levels = 16;
    s.ratio.assign(15, 1 << 20);
    s.add(15, 0, 0, 0, 2, 2, 2);
    s.add(0, 0, 0, 0, 0, 1, 1);
    s.labels[1].cells = s.parents[1].cells = nullptr;
    s.plan();
    s.add(0, 0, 0, 0, 1, 1, 1);
    expect_message(kRefined, [&] { s.plan(); });
    s.labels[2].level = s.parents[2].level = 14;  // R = 2^20: cell 0 fits, cell 1024 does not
    s.plan();
    s.lo[6] = 1023;
    s.plan();
    s.lo[6] = 1024;
    expect_message(kRefined, [&] { s.plan(); });
    s.lo[6] = -1024;
    s.plan();
    s.lo[6] = -1025;
    expect_message(kRefined, [&] { s.plan(); });
  }
}

// What a visit of visit_tables was given, in order.
struct Seen {
  std::vector<const void*> slots, tables;
  std::vector<size_t> counts, widths;
  template <class T>
  void operator()(const T** device, const T* host, size_t count) {
    slots.push_back(device);
    tables.push_back(host);
    counts.push_back(count);
    widths.push_back(sizeof(T));
  }
};

void launch_arguments() {
  Scene s = two_levels();
  s.add(1, -40, 6, 8, 131, 3, 5);  // 2 chunks x 1 x 2 tiles
  s.n_clumps = 77;
  s.n_parents = 12;
  s.labels[2].cells += 1;  // off a 16-byte boundary: this box is not paired
  const avr::ClumpLinksPlan p = s.plan();
  expect(p.args.boxes == nullptr && p.args.refined == nullptr && p.args.tile_begin == nullptr &&
             p.args.extent == nullptr && p.args.parent_lo == nullptr &&
             p.args.parent_hi == nullptr && p.args.totals == nullptr,
         "the plan leaves every address null");
  expect(p.args.n_boxes == 4 && p.args.n_tiles == 1 + 1 + 4 + 4 && p.args.n_clumps == 77 &&
             p.args.n_parents == 12, "the counts");
  expect(p.tile_begin == std::vector<uint32_t>({0, 1, 2, 6, 10}), "the tile prefix");
  expect(p.boxes[0].paired == 1 && p.boxes[2].paired == 0 && p.boxes[3].paired == 0,
         "paired: both fields aligned with even strides");
  expect(p.boxes[3].cells[0] == s.labels[3].cells && p.boxes[3].cells[1] == s.parents[3].cells &&
             p.boxes[3].jstride[0] == 131 && p.boxes[3].kstride[1] == 393 && p.boxes[3].nx == 131 &&
             p.boxes[3].ny == 3 && p.boxes[3].nz == 5 && p.boxes[3].level == 1, "a device box");
  expect(p.refined[3].lo[0] == -40 && p.refined[3].lo[1] == 6 && p.refined[3].lo[2] == 8 &&
             p.refined[3].scale == 1 && p.refined[1].lo[0] == 8 && p.refined[1].scale == 2,
         "the refined boxes");
  avr::ClumpLinkArgs args = p.args;
  Seen seen;
  p.visit_tables(&args, seen);
  expect(seen.slots == std::vector<const void*>({&args.boxes, &args.refined, &args.tile_begin}),
         "visit_tables: boxes, refined, tile_begin");
  expect(seen.tables == std::vector<const void*>({p.boxes.data(), p.refined.data(),
                                                  p.tile_begin.data()}), "the host tables");
  expect(seen.counts == std::vector<size_t>({4, 4, 5}) &&
             seen.widths == std::vector<size_t>({80, 16, 4}), "the tables' counts and widths");
  avr::StagingSize size;
  p.visit_tables(&args, size);
  expect(size.items == 3 && size.bytes == 4 * 80 + 4 * 16 + 5 * 4, "the staging batch");
  // a scene without boxes: nothing to launch
  Scene none;
  none.has_parents = false;  // an empty vector has no array to hand over
  const avr::ClumpLinksPlan q = none.plan();
  expect(q.args.n_tiles == 0 && q.args.n_boxes == 0 && q.tile_begin.size() == 1, "no boxes");
}

}  // namespace

int main() {
  messages_and_precedence();
  parents_and_their_count();
  refined_boxes();
  refined_limits();
  launch_arguments();
  std::puts("ok");
  return 0;
}
