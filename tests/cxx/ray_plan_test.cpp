// The host plan of the rays (csrc/avr_field_plans.h: plan_rays) as a plain C++ program, built with
// AddressSanitizer and UBSan and without HIP: every refusal message and which one wins when
// several rules are broken, the size rules (reached with descriptors only: no cell is ever
// allocated or read), and the locator -- the one build_level_locator makes for plan_rays is the one
// it makes for plan_streamlines over the same boxes, entry for entry, and [Blo, Bhi] is the boxes'
// hull at level 0.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

const void* address(int bit) { return reinterpret_cast<const void*>(uintptr_t{1} << bit); }

// A scene of descriptors: box b's cells are contiguous at a made-up address that nothing reads.
struct Scene {
  std::vector<avr_box> field;
  std::vector<int32_t> lo;
  std::vector<int32_t> ratio;
  std::vector<double> sizes = {0.5, 0.25, 1.0, 0.25, 0.125, 0.5, 0.0625, 0.03125, 0.125};
  double prob_lo[3] = {-1.0, 0.0, 2.0};
  uint64_t n_rays = 100, max_trips = 64, n_segments = 1000;
  int n_levels = 1;
  bool emit = false, no_sizes = false, no_prob_lo = false;
  int64_t max_entries = avr::kStreamMaxEntries;
  // made-up addresses, far from every box
  const void* start = address(46);
  const void* end = address(47);
  const void* offsets = address(48);
  const void* counts = address(49);
  const void* status = address(50);
  const void* span = address(51);
  const void* t0 = address(52);
  const void* t1 = address(53);
  const void* level = address(54);
  const void* value = address(55);
  const void* integral = address(56);
  const void* covered = address(57);

  void add(int box_level, int x, int y, int z, int nx, int ny, int nz) {
    const uintptr_t stride = uintptr_t{1} << 31;  // bytes between two boxes: 2^28 cells
    avr_box box{};
    box.dims[0] = nx;
    box.dims[1] = ny;
    box.dims[2] = nz;
    box.level = box_level;
    box.jstride = nx;
    box.kstride = static_cast<int64_t>(nx) * ny;
    box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 40) + field.size() * stride);
    field.push_back(box);
    lo.push_back(x);
    lo.push_back(y);
    lo.push_back(z);
  }
  avr::RayPlan plan() const {
    return avr::plan_rays(field.data(), field.size(), n_rays, max_trips, lo.data(),
                          ratio.empty() ? nullptr : ratio.data(), no_sizes ? nullptr : sizes.data(),
                          no_prob_lo ? nullptr : prob_lo, n_levels, start, end,
                          emit ? offsets : nullptr, emit ? n_segments : 0, counts, status, span, t0,
                          t1, level, value, integral, covered, max_entries);
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

const char* kMaxTrips = "max_trips must lie in [1, 2^30]";
const char* kRays = "n_rays must stay below 2^32";
const char* kSegments = "n_segments must not exceed 2^40";
const char* kLevels = "n_levels must lie in [1, 16]";
const char* kSizes = "level_cell_size must be finite and positive";
const char* kProbLo = "prob_lo must be finite";
const char* kLevel = "a box's level is not below n_levels";
const char* kNoCells = "box has no cell data";
const char* kSpan = "box spans more than 2^28 cells (or has negative strides)";
const char* kRatio = "a level ratio is below 2";
const char* kRange = "a box's index range leaves [-2^30, 2^30)";
const char* kOverlap = "two boxes of one level overlap in index space";
const char* kShared = "an output array or the rays overlap an input box's cells";
const char* kLocator = "the locator's lists hold 2^28 entries or more";
const char* kBound = "the scene's bounding box leaves [-2^30, 2^30] at the finest level";
const char* kNull = "null argument";

#define REFUSED(message, change)                       \
  {                                                    \
    Scene s = two_levels();                            \
    change;                                            \
    expect_message(message, [&] { s.plan(); });        \
  }
#define ACCEPTED(change)  \
  {                       \
    Scene s = two_levels(); \
    change;               \
    s.plan();             \
  }

void messages_and_precedence() {
  two_levels().plan();  // in order, the count pass
  ACCEPTED(s.emit = true);
  // each rule alone
  REFUSED(kMaxTrips, s.max_trips = 0);
  REFUSED(kMaxTrips, s.max_trips = (uint64_t{1} << 30) + 1);
  REFUSED(kMaxTrips, s.max_trips = ~uint64_t{0});
  ACCEPTED(s.max_trips = 1);
  ACCEPTED(s.max_trips = uint64_t{1} << 30);
  REFUSED(kRays, s.n_rays = uint64_t{1} << 32);
  REFUSED(kRays, s.n_rays = ~uint64_t{0});
  ACCEPTED(s.n_rays = (uint64_t{1} << 32) - 1);
  REFUSED(kSegments, (s.emit = true, s.n_segments = (uint64_t{1} << 40) + 1));
  ACCEPTED((s.emit = true, s.n_segments = uint64_t{1} << 40));
  ACCEPTED(s.n_segments = ~uint64_t{0});  // the count pass does not look at it
  REFUSED(kLevels, s.n_levels = 0);
  REFUSED(kLevels, (s.n_levels = 17, s.ratio.assign(16, 2), s.sizes.assign(51, 1.0)));
  REFUSED(kNull, s.ratio.clear());
  REFUSED(kNull, s.no_sizes = true);
  REFUSED(kNull, s.no_prob_lo = true);
  REFUSED(kLevels, (s.n_levels = 0, s.no_sizes = true));
  REFUSED(kMaxTrips, (s.max_trips = 0, s.no_prob_lo = true));
  REFUSED(kNull, s.start = nullptr);
  REFUSED(kNull, s.end = nullptr);
  REFUSED(kNull, s.counts = nullptr);
  REFUSED(kNull, s.status = nullptr);
  REFUSED(kNull, s.span = nullptr);
  // each pass needs its own arrays only
  ACCEPTED(s.t0 = s.t1 = s.level = s.value = s.integral = s.covered = nullptr);
  ACCEPTED((s.emit = true, s.counts = s.status = s.span = nullptr));
  REFUSED(kNull, (s.emit = true, s.t0 = nullptr));
  REFUSED(kNull, (s.emit = true, s.t1 = nullptr));
  REFUSED(kNull, (s.emit = true, s.level = nullptr));
  REFUSED(kNull, (s.emit = true, s.value = nullptr));
  REFUSED(kNull, (s.emit = true, s.integral = nullptr));
  REFUSED(kNull, (s.emit = true, s.covered = nullptr));
  ACCEPTED((s.emit = true, s.n_segments = 0, s.t0 = s.t1 = s.level = s.value = nullptr));
  // no rays: the arrays may be null, the other rules hold
  ACCEPTED((s.n_rays = 0, s.start = s.end = s.counts = s.status = s.span = nullptr));
  REFUSED(kMaxTrips, (s.n_rays = 0, s.max_trips = 0));
  REFUSED(kSizes, s.sizes[4] = 0.0);
  REFUSED(kSizes, s.sizes[0] = -0.5);
  REFUSED(kSizes, s.sizes[5] = kInf);
  REFUSED(kSizes, s.sizes[2] = kNaN);
  ACCEPTED(s.sizes[6] = kNaN);  // of a level that is not there
  REFUSED(kProbLo, s.prob_lo[1] = kInf);
  REFUSED(kProbLo, s.prob_lo[2] = kNaN);
  REFUSED(kLevel, s.field[2].level = 2);
  REFUSED(kLevel, s.field[0].level = -1);
  REFUSED(kNoCells, s.field[1].cells = nullptr);
  REFUSED(kSpan, s.field[0].kstride = int64_t{1} << 28);
  REFUSED(kSpan, s.field[0].jstride = -4);
  REFUSED(kRatio, s.ratio[0] = 1);
  REFUSED(kRatio, s.ratio[0] = 0);
  REFUSED(kRatio, s.ratio[0] = -2);
  REFUSED(kRange, s.lo[0] = (1 << 30) - 3);
  REFUSED(kRange, s.lo[7] = -(1 << 30) - 1);
  REFUSED(kOverlap, s.lo[3] = 3);
  ACCEPTED(s.lo[6] = 0);  // another level's box over the same indices
  // an output array, the end points or the offsets on an input box's cells: first byte, last
  // byte, one past
  const uintptr_t cells = reinterpret_cast<uintptr_t>(two_levels().field[1].cells);
  REFUSED(kShared, s.start = reinterpret_cast<const void*>(cells));
  REFUSED(kShared, s.end = reinterpret_cast<const void*>(cells + 8));
  REFUSED(kShared, s.status = reinterpret_cast<const void*>(cells + 64 * 8 - 1));
  ACCEPTED(s.status = reinterpret_cast<const void*>(cells + 64 * 8));
  REFUSED(kShared, s.counts = reinterpret_cast<const void*>(cells - 100 * 4 + 1));
  ACCEPTED(s.counts = reinterpret_cast<const void*>(cells - 100 * 4));
  REFUSED(kShared, s.span = reinterpret_cast<const void*>(cells - 100 * 16 + 1));
  ACCEPTED(s.span = reinterpret_cast<const void*>(cells - 100 * 16));
  ACCEPTED(s.t0 = reinterpret_cast<const void*>(cells));  // the count pass does not write it
  REFUSED(kShared, (s.emit = true, s.t0 = reinterpret_cast<const void*>(cells)));
  REFUSED(kShared, (s.emit = true, s.t1 = reinterpret_cast<const void*>(cells + 16)));
  REFUSED(kShared, (s.emit = true, s.value = reinterpret_cast<const void*>(cells - 1000 * 8 + 1)));
  ACCEPTED((s.emit = true, s.value = reinterpret_cast<const void*>(cells - 1000 * 8)));
  REFUSED(kShared, (s.emit = true, s.level = reinterpret_cast<const void*>(cells - 1000 + 1)));
  ACCEPTED((s.emit = true, s.level = reinterpret_cast<const void*>(cells - 1000)));
  REFUSED(kShared, (s.emit = true, s.integral = reinterpret_cast<const void*>(cells)));
  REFUSED(kShared, (s.emit = true, s.covered = reinterpret_cast<const void*>(cells)));
  REFUSED(kShared, (s.emit = true, s.offsets = reinterpret_cast<const void*>(cells - 101 * 8 + 1)));
  ACCEPTED((s.emit = true, s.offsets = reinterpret_cast<const void*>(cells - 101 * 8)));
  ACCEPTED((s.emit = true, s.counts = reinterpret_cast<const void*>(cells)));  // not written
  ACCEPTED((s.n_rays = 0, s.start = reinterpret_cast<const void*>(cells)));  // nothing is read
  REFUSED(kLocator, s.max_entries = 3);
  // the bounding box at the finest level: a level-0 box at 2^29 under a ratio of 4
  REFUSED(kBound, (s.ratio[0] = 4, s.lo[0] = 1 << 29, s.lo[3] = (1 << 29) + 4));
  REFUSED(kBound, (s.ratio[0] = 4, s.lo[1] = -(1 << 29)));
  // which one wins: the rules in the order of the definition
  REFUSED(kMaxTrips, (s.max_trips = 0, s.n_rays = uint64_t{1} << 32));
  REFUSED(kRays, (s.n_rays = uint64_t{1} << 32, s.emit = true, s.n_segments = ~uint64_t{0}));
  REFUSED(kSegments, (s.emit = true, s.n_segments = ~uint64_t{0}, s.n_levels = 0));
  REFUSED(kLevels, (s.n_levels = 0, s.start = nullptr));
  REFUSED(kNull, (s.start = nullptr, s.sizes[0] = 0.0));
  REFUSED(kSizes, (s.sizes[0] = 0.0, s.prob_lo[0] = kNaN));
  REFUSED(kProbLo, (s.prob_lo[0] = kNaN, s.field[2].level = 2));
  REFUSED(kLevel, (s.field[0].level = 2, s.ratio[0] = 1));
  REFUSED(kNoCells, (s.field[0].cells = nullptr, s.ratio[0] = 1));
  REFUSED(kRatio, (s.ratio[0] = 1, s.lo[0] = 1 << 30));
  REFUSED(kRange, (s.lo[0] = 1 << 30, s.lo[3] = 3));
  REFUSED(kOverlap, (s.lo[3] = 3, s.start = reinterpret_cast<const void*>(cells)));
  REFUSED(kShared, (s.start = reinterpret_cast<const void*>(cells), s.max_entries = 3));
  REFUSED(kLocator, (s.max_entries = 3, s.ratio[0] = 4, s.lo[0] = 1 << 29, s.lo[3] = (1 << 29) + 4));
}

// The largest scenes the rules admit, from descriptors alone.
void size_rules() {
  Scene s;
  s.n_levels = 1;
  s.add(0, -(1 << 30), -(1 << 30), -(1 << 30), 1, 1, 1);
  s.add(0, (1 << 30) - 1, (1 << 30) - 1, (1 << 30) - 1, 1, 1, 1);
  s.n_rays = (uint64_t{1} << 32) - 1;
  s.max_trips = uint64_t{1} << 30;
  const avr::RayPlan plan = s.plan();
  expect(plan.locator.origin[0] == -(1 << 30) && plan.locator.shift == 29, "the widest locator's blocks");
  for (int d = 0; d < 3; ++d) {
    expect(plan.bound_lo[d] == -(1 << 30) && plan.bound_hi[d] == (1 << 30) - 1, "the widest bounds");
  }
  // sixteen levels of ratio 2 over one level-0 cell at the origin: 2^15 finest cells a side; the
  // same cell at 2^15 is the last whose children stay inside, at 2^15 + 1 they do not
  Scene deep;
  deep.n_levels = 16;
  deep.ratio.assign(15, 2);
  deep.sizes.assign(48, 0.5);
  deep.add(0, 0, 0, 0, 1, 1, 1);
  deep.plan();
  deep.lo[0] = (1 << 15) - 1;
  deep.plan();
  deep.lo[0] = 1 << 15;
  expect_message(kBound, [&] { deep.plan(); });
  deep.lo[0] = -(1 << 15);
  deep.plan();
  deep.lo[0] = -(1 << 15) - 1;
  expect_message(kBound, [&] { deep.plan(); });
  // a scene without cells: no block at all, and empty bounds
  Scene none;
  none.add(0, 0, 0, 0, 0, 4, 4);
  none.field[0].cells = nullptr;
  const avr::RayPlan empty = none.plan();
  expect(empty.locator.n[0] == 0 && empty.block_begin.size() == 1 && empty.block_boxes.empty(),
         "a scene without cells has no locator");
  expect(empty.bound_hi[0] < empty.bound_lo[0], "a scene without cells has empty bounds");
  // the lists' bound, just met and just missed
  Scene three = two_levels();
  three.max_entries = 100;
  const size_t entries = three.plan().block_boxes.size();
  three.max_entries = static_cast<int64_t>(entries) + 1;
  three.plan();
  three.max_entries = static_cast<int64_t>(entries);
  expect_message(kLocator, [&] { three.plan(); });
}

// plan_streamlines over the same boxes, each as all three components.
avr::StreamPlan stream_plan(const Scene& s) {
  return avr::plan_streamlines(s.field.data(), s.field.data(), s.field.data(), nullptr,
                               s.field.size(), 10, 0.5, 1, 4, s.lo.data(),
                               s.ratio.empty() ? nullptr : s.ratio.data(), s.sizes.data(),
                               s.prob_lo, s.n_levels, address(46), address(47), nullptr,
                               address(49), address(50));
}

void check_same_locator(const Scene& s, const std::string& name) {
  const avr::RayPlan rays = s.plan();
  const avr::StreamPlan lines = stream_plan(s);
  expect(std::memcmp(&rays.locator, &lines.locator, sizeof(rays.locator)) == 0,
         name + ": the locators' shapes differ");
  expect(rays.block_begin == lines.block_begin, name + ": the locators' CSR differs");
  expect(rays.block_boxes == lines.block_boxes, name + ": the locators' lists differ");
  expect(rays.boxes.size() == lines.boxes.size(), name + ": the box tables differ");
  for (size_t b = 0; b < rays.boxes.size(); ++b) {
    const avr::CoverBoxDev& mine = rays.boxes[b];
    const avr::StreamBoxDev& theirs = lines.boxes[b];
    expect(mine.cells == theirs.cells[0] && mine.jstride == theirs.jstride[0] &&
               mine.kstride == theirs.kstride[0] && mine.nx == theirs.nx && mine.ny == theirs.ny &&
               mine.nz == theirs.nz && mine.level == theirs.level && mine.lo[0] == theirs.lo[0] &&
               mine.lo[1] == theirs.lo[1] && mine.lo[2] == theirs.lo[2],
           name + ": a box differs");
  }
  expect(std::memcmp(&rays.levels, &lines.levels, sizeof(rays.levels)) == 0,
         name + ": the level setups differ");
  // [Blo, Bhi]: the hull of the boxes with cells at level 0, and the blocks cover exactly it
  int64_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  bool any = false;
  for (size_t b = 0; b < s.field.size(); ++b) {
    const avr_box& box = s.field[b];
    if (box.dims[0] <= 0 || box.dims[1] <= 0 || box.dims[2] <= 0) continue;
    for (int d = 0; d < 3; ++d) {
      int64_t first = s.lo[b * 3 + d], last = first + box.dims[d] - 1;
      for (int l = box.level; l > 0; --l) {
        first = avr::floor_div(first, s.ratio[l - 1]);
        last = avr::floor_div(last, s.ratio[l - 1]);
      }
      lo[d] = any ? std::min(lo[d], first) : first;
      hi[d] = any ? std::max(hi[d], last) : last;
    }
    any = true;
  }
  expect(any, name + ": no box has cells");
  for (int d = 0; d < 3; ++d) {
    expect(rays.bound_lo[d] == lo[d] && rays.bound_hi[d] == hi[d], name + ": [Blo, Bhi]");
    expect(rays.locator.origin[d] == lo[d], name + ": the locator's origin");
    expect(((hi[d] - lo[d]) >> rays.locator.shift) + 1 == rays.locator.n[d],
           name + ": the blocks do not end with Bhi");
  }
}

void locators() {
  check_same_locator(two_levels(), "two levels");
  {  // three levels, ratios 4 and 2, negative indices, touching and nested boxes, a box without cells
    Scene s;
    s.n_levels = 3;
    s.ratio = {4, 2};
    s.add(0, -3, -2, -1, 5, 4, 3);
    s.add(0, 2, -2, -1, 3, 4, 3);
    s.add(1, -8, -4, 0, 8, 8, 4);
    s.add(2, -16, -8, 0, 0, 4, 4);
    s.field[3].cells = nullptr;
    s.add(1, 0, -4, 0, 4, 8, 4);
    s.add(2, -10, -6, 2, 7, 5, 3);
    s.add(2, -3, -6, 2, 9, 5, 3);
    check_same_locator(s, "three levels");
  }
  {  // a skipped level, and fine boxes that reach past the coarse ones
    Scene s;
    s.n_levels = 3;
    s.ratio = {2, 2};
    s.add(0, 0, 0, 0, 8, 4, 4);
    s.add(2, 30, 8, 8, 8, 8, 8);
    s.add(1, 2, 2, 2, 6, 4, 4);
    check_same_locator(s, "a skipped level");
  }
  {  // eighty boxes of 4^3, a long thin box, a lone cell far away
    Scene s;
    s.n_levels = 1;
    for (int c = 0; c < 5; ++c) {
      for (int b = 0; b < 4; ++b) {
        for (int a = 0; a < 4; ++a) s.add(0, 4 * a, 4 * b, 4 * c, 4, 4, 4);
      }
    }
    s.add(0, 16, 0, 0, 300, 1, 2);
    s.add(0, 500, 40, 40, 1, 1, 1);
    check_same_locator(s, "many boxes");
  }
}

}  // namespace

int main() {
  messages_and_precedence();
  size_rules();
  locators();
  std::printf("ok\n");
  return 0;
}
