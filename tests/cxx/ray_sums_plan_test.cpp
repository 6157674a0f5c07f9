// The host plan of the per-ray sums (csrc/avr_field_plans.h: plan_ray_sums) as a plain C++ program,
// built with AddressSanitizer and UBSan and without HIP: every refusal message and which one wins
// when several rules are broken, the weight scene's rules (count, level, dims, corner, the view
// rule), the shared-byte rule over the new outputs and the weight's cells, and that a plan without
// a weight holds plan_rays' tables entry for entry.  No cell is ever allocated or read.  Prints
// "ok".
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

// Two scenes of descriptors over the same boxes: box b's cells are contiguous at a made-up address
// that nothing reads, the field's from 2^40 on and the weight's from 2^41 on.
struct Scene {
  std::vector<avr_box> field, weight;
  std::vector<int32_t> lo;
  std::vector<int32_t> ratio;
  std::vector<double> sizes = {0.5, 0.25, 1.0, 0.25, 0.125, 0.5, 0.0625, 0.03125, 0.125};
  double prob_lo[3] = {-1.0, 0.0, 2.0};
  uint64_t n_rays = 100, max_trips = 64;
  int n_levels = 1;
  bool weighted = true, no_sizes = false, no_prob_lo = false;
  int64_t max_entries = avr::kStreamMaxEntries;
  // made-up addresses, far from every box
  const void* start = address(46);
  const void* end = address(47);
  const void* counts = address(49);
  const void* status = address(50);
  const void* span = address(51);
  const void* integral = address(52);
  const void* weight_out = address(53);
  const void* counted = address(54);
  const void* covered = address(55);

  void add(int box_level, int x, int y, int z, int nx, int ny, int nz) {
    const uintptr_t stride = uintptr_t{1} << 31;  // bytes between two boxes: 2^28 cells
    avr_box box{};
    box.dims[0] = nx;
    box.dims[1] = ny;
    box.dims[2] = nz;
    box.level = box_level;
    box.jstride = nx;
    box.kstride = static_cast<int64_t>(nx) * ny;
    box.min_corner[0] = 0.25 * x;
    box.min_corner[1] = 0.25 * y;
    box.min_corner[2] = 0.25 * z;
    box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 40) + field.size() * stride);
    field.push_back(box);
    // the weight's rows are padded: its own strides
    box.jstride = nx + 2;
    box.kstride = static_cast<int64_t>(nx + 2) * ny;
    box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 41) + weight.size() * stride);
    weight.push_back(box);
    lo.push_back(x);
    lo.push_back(y);
    lo.push_back(z);
  }
  avr::RaySumsPlan plan() const {
    return avr::plan_ray_sums(field.data(), field.size(), weighted ? weight.data() : nullptr,
                              weighted ? weight.size() : 0, n_rays, max_trips, lo.data(),
                              ratio.empty() ? nullptr : ratio.data(),
                              no_sizes ? nullptr : sizes.data(), no_prob_lo ? nullptr : prob_lo,
                              n_levels, start, end, counts, status, span, integral, weight_out,
                              counted, covered, max_entries);
  }
  avr::RayPlan ray_plan(bool emit) const {
    return avr::plan_rays(field.data(), field.size(), n_rays, max_trips, lo.data(),
                          ratio.empty() ? nullptr : ratio.data(), sizes.data(), prob_lo, n_levels,
                          start, end, emit ? address(48) : nullptr, emit ? 1000 : 0, counts, status,
                          span, address(56), address(57), address(58), address(59), integral,
                          covered, max_entries);
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
const char* kLevels = "n_levels must lie in [1, 16]";
const char* kSizes = "level_cell_size must be finite and positive";
const char* kProbLo = "prob_lo must be finite";
const char* kLevel = "a box's level is not below n_levels";
const char* kNoCells = "box has no cell data";
const char* kSpan = "box spans more than 2^28 cells (or has negative strides)";
const char* kWeight = "the weight scene's boxes differ from the field's";
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
// without a weight scene and its output
#define PLAIN (s.weighted = false, s.weight_out = nullptr)

void messages_and_precedence() {
  two_levels().plan();  // in order, weighted
  ACCEPTED(PLAIN);
  // each of plan_rays' rules alone
  REFUSED(kMaxTrips, s.max_trips = 0);
  REFUSED(kMaxTrips, s.max_trips = (uint64_t{1} << 30) + 1);
  ACCEPTED(s.max_trips = uint64_t{1} << 30);
  REFUSED(kRays, s.n_rays = uint64_t{1} << 32);
  REFUSED(kRays, s.n_rays = ~uint64_t{0});
  ACCEPTED(s.n_rays = (uint64_t{1} << 32) - 1);
  REFUSED(kLevels, s.n_levels = 0);
  REFUSED(kLevels, (s.n_levels = 17, s.ratio.assign(16, 2), s.sizes.assign(51, 1.0)));
  REFUSED(kNull, s.ratio.clear());
  REFUSED(kNull, s.no_sizes = true);
  REFUSED(kNull, s.no_prob_lo = true);
  REFUSED(kNull, s.start = nullptr);
  REFUSED(kNull, s.end = nullptr);
  REFUSED(kNull, s.counts = nullptr);
  REFUSED(kNull, s.status = nullptr);
  REFUSED(kNull, s.span = nullptr);
  REFUSED(kNull, s.integral = nullptr);
  REFUSED(kNull, s.counted = nullptr);
  REFUSED(kNull, s.covered = nullptr);
  REFUSED(kNull, (PLAIN, s.covered = nullptr));
  // the null pairs: a weight scene without its output, an output without the scene
  REFUSED(kNull, s.weight_out = nullptr);
  REFUSED(kNull, s.weighted = false);
  // no rays: the arrays may be null, the other rules hold
  ACCEPTED((s.n_rays = 0, s.start = s.end = s.counts = s.status = s.span = s.integral =
                              s.weight_out = s.counted = s.covered = nullptr));
  REFUSED(kMaxTrips, (s.n_rays = 0, s.max_trips = 0));
  REFUSED(kWeight, (s.n_rays = 0, s.weight.pop_back()));
  REFUSED(kSizes, s.sizes[4] = 0.0);
  REFUSED(kSizes, s.sizes[5] = kInf);
  REFUSED(kSizes, s.sizes[2] = kNaN);
  REFUSED(kProbLo, s.prob_lo[1] = kInf);
  REFUSED(kLevel, (s.field[2].level = 2, s.weight[2].level = 2));
  REFUSED(kLevel, (s.field[0].level = -1, s.weight[0].level = -1));
  REFUSED(kNoCells, s.field[1].cells = nullptr);
  REFUSED(kSpan, s.field[0].kstride = int64_t{1} << 28);
  REFUSED(kSpan, s.field[0].jstride = -4);
  // the weight scene: the count, then box by box level, dims and corner, then the view rule
  REFUSED(kWeight, s.weight.pop_back());
  REFUSED(kWeight, s.weight.push_back(s.weight[0]));
  REFUSED(kWeight, s.weight[2].level = 0);
  REFUSED(kWeight, s.weight[0].level = 1);
  REFUSED(kWeight, s.weight[1].dims[0] = 5);
  REFUSED(kWeight, s.weight[1].dims[1] = 3);
  REFUSED(kWeight, s.weight[2].dims[2] = 9);
  REFUSED(kWeight, s.weight[1].min_corner[0] = 0.0);
  REFUSED(kWeight, s.weight[2].min_corner[2] = 0.125);
  REFUSED(kWeight, std::swap(s.weight[0], s.weight[1]));  // the same boxes in another order
  REFUSED(kNoCells, s.weight[1].cells = nullptr);
  REFUSED(kSpan, s.weight[0].kstride = int64_t{1} << 28);
  REFUSED(kSpan, s.weight[2].jstride = -8);
  ACCEPTED((s.weight[1].jstride = 100, s.weight[1].kstride = 1000));  // its own strides
  ACCEPTED((PLAIN, s.weight[1].dims[0] = 5));                          // not looked at
  {  // a box without cells needs none in either scene
    Scene s = two_levels();
    s.add(1, 40, 0, 0, 0, 4, 4);
    s.field[3].cells = s.weight[3].cells = nullptr;
    const avr::RaySumsPlan plan = s.plan();
    expect(plan.weight_boxes.size() == 4 && plan.weight_boxes[3].nx == 0 &&
               plan.weight_boxes[3].cells == nullptr, "a weight box without cells");
  }
  REFUSED(kRatio, s.ratio[0] = 1);
  REFUSED(kRange, s.lo[0] = (1 << 30) - 3);
  REFUSED(kOverlap, s.lo[3] = 3);
  // an output array or the end points on a cell of either scene: first byte, last byte, one past
  const uintptr_t cells = reinterpret_cast<uintptr_t>(two_levels().field[1].cells);
  const uintptr_t other = reinterpret_cast<uintptr_t>(two_levels().weight[1].cells);
  // the weight's box 1: rows of 6, planes of 24 elements, so its last cell is element 3 + 18 + 72
  const uintptr_t other_bytes = (3 + 3 * 6 + 3 * 24 + 1) * 8;
  REFUSED(kShared, s.start = reinterpret_cast<const void*>(cells));
  REFUSED(kShared, s.end = reinterpret_cast<const void*>(other + 8));
  REFUSED(kShared, s.counts = reinterpret_cast<const void*>(cells - 100 * 4 + 1));
  ACCEPTED(s.counts = reinterpret_cast<const void*>(cells - 100 * 4));
  REFUSED(kShared, s.status = reinterpret_cast<const void*>(cells + 64 * 8 - 1));
  ACCEPTED(s.status = reinterpret_cast<const void*>(cells + 64 * 8));
  REFUSED(kShared, s.status = reinterpret_cast<const void*>(other + other_bytes - 1));
  ACCEPTED(s.status = reinterpret_cast<const void*>(other + other_bytes));
  REFUSED(kShared, s.span = reinterpret_cast<const void*>(other - 100 * 16 + 1));
  ACCEPTED(s.span = reinterpret_cast<const void*>(other - 100 * 16));
  REFUSED(kShared, s.integral = reinterpret_cast<const void*>(other));
  REFUSED(kShared, s.integral = reinterpret_cast<const void*>(cells - 100 * 8 + 1));
  ACCEPTED(s.integral = reinterpret_cast<const void*>(cells - 100 * 8));
  REFUSED(kShared, s.weight_out = reinterpret_cast<const void*>(cells));
  REFUSED(kShared, s.weight_out = reinterpret_cast<const void*>(other - 100 * 8 + 1));
  ACCEPTED(s.weight_out = reinterpret_cast<const void*>(other - 100 * 8));
  REFUSED(kShared, s.counted = reinterpret_cast<const void*>(other + 16));
  REFUSED(kShared, s.counted = reinterpret_cast<const void*>(cells + 16));
  REFUSED(kShared, s.covered = reinterpret_cast<const void*>(other + other_bytes - 1));
  REFUSED(kShared, s.covered = reinterpret_cast<const void*>(cells));
  // without the weight scene its cells are no input
  ACCEPTED((PLAIN, s.covered = reinterpret_cast<const void*>(other)));
  REFUSED(kShared, (PLAIN, s.covered = reinterpret_cast<const void*>(cells)));
  ACCEPTED((s.n_rays = 0, s.start = reinterpret_cast<const void*>(other)));  // nothing is read
  REFUSED(kLocator, s.max_entries = 3);
  REFUSED(kBound, (s.ratio[0] = 4, s.lo[0] = 1 << 29, s.lo[3] = (1 << 29) + 4));
  // which one wins: the rules in the order of the definition
  REFUSED(kMaxTrips, (s.max_trips = 0, s.n_rays = uint64_t{1} << 32));
  REFUSED(kRays, (s.n_rays = uint64_t{1} << 32, s.n_levels = 0));
  REFUSED(kLevels, (s.n_levels = 0, s.start = nullptr));
  REFUSED(kLevels, (s.n_levels = 0, s.no_sizes = true));
  REFUSED(kNull, (s.start = nullptr, s.sizes[0] = 0.0));
  REFUSED(kNull, (s.weight_out = nullptr, s.sizes[0] = 0.0));
  REFUSED(kNull, (s.weight_out = nullptr, s.weight.pop_back()));
  REFUSED(kSizes, (s.sizes[0] = 0.0, s.prob_lo[0] = kNaN));
  REFUSED(kProbLo, (s.prob_lo[0] = kNaN, s.field[2].level = 2));
  REFUSED(kLevel, (s.field[0].level = 2, s.weight.pop_back()));
  REFUSED(kNoCells, (s.field[2].cells = nullptr, s.weight[0].dims[0] = 5));  // the field's box rules first
  REFUSED(kWeight, (s.weight.pop_back(), s.weight[0].cells = nullptr));      // the count before the boxes
  REFUSED(kNoCells, (s.weight[1].dims[0] = 5, s.weight[0].cells = nullptr)); // box by box: the
  REFUSED(kWeight, (s.weight[0].dims[0] = 5, s.weight[1].cells = nullptr));  // earlier box first
  REFUSED(kWeight, (s.weight[1].level = 1, s.weight[1].cells = nullptr));    // in a box: the match first
  REFUSED(kWeight, (s.weight[0].dims[2] = 1, s.ratio[0] = 1));
  REFUSED(kSpan, (s.weight[2].jstride = -1, s.ratio[0] = 1));
  REFUSED(kRatio, (s.ratio[0] = 1, s.lo[0] = 1 << 30));
  REFUSED(kRange, (s.lo[0] = 1 << 30, s.lo[3] = 3));
  REFUSED(kOverlap, (s.lo[3] = 3, s.start = reinterpret_cast<const void*>(other)));
  REFUSED(kShared, (s.counted = reinterpret_cast<const void*>(other), s.max_entries = 3));
  REFUSED(kLocator, (s.max_entries = 3, s.ratio[0] = 4, s.lo[0] = 1 << 29, s.lo[3] = (1 << 29) + 4));
}

bool same_box(const avr::CoverBoxDev& a, const avr::CoverBoxDev& b) {
  return a.cells == b.cells && a.jstride == b.jstride && a.kstride == b.kstride && a.nx == b.nx &&
         a.ny == b.ny && a.nz == b.nz && a.level == b.level && a.lo[0] == b.lo[0] &&
         a.lo[1] == b.lo[1] && a.lo[2] == b.lo[2];
}

// plan_rays over the same boxes, either pass: the same tables entry for entry, with or without a
// weight; and the weight's table: the field's boxes with the weight's cells and strides.
void check_same_tables(const Scene& scene, const std::string& name) {
  for (int weighted = 0; weighted < 2; ++weighted) {
    Scene s = scene;
    s.weighted = weighted != 0;
    if (!s.weighted) s.weight_out = nullptr;
    const avr::RaySumsPlan sums = s.plan();
    expect(sums.weight_boxes.size() == (s.weighted ? s.field.size() : 0),
           name + ": the weight's table");
    for (int emit = 0; emit < 2; ++emit) {
      const avr::RayPlan rays = s.ray_plan(emit != 0);
      const avr::RayPlan& walk = sums.walk;
      expect(std::memcmp(&walk.locator, &rays.locator, sizeof(rays.locator)) == 0,
             name + ": the locators' shapes differ");
      expect(walk.block_begin == rays.block_begin, name + ": the locators' CSR differs");
      expect(walk.block_boxes == rays.block_boxes, name + ": the locators' lists differ");
      expect(std::memcmp(&walk.levels, &rays.levels, sizeof(rays.levels)) == 0,
             name + ": the level setups differ");
      expect(walk.boxes.size() == rays.boxes.size(), name + ": the box tables differ");
      for (size_t b = 0; b < rays.boxes.size(); ++b) {
        expect(same_box(walk.boxes[b], rays.boxes[b]), name + ": a box differs");
      }
      for (int d = 0; d < 3; ++d) {
        expect(walk.bound_lo[d] == rays.bound_lo[d] && walk.bound_hi[d] == rays.bound_hi[d],
               name + ": [Blo, Bhi]");
      }
    }
    for (size_t b = 0; b < sums.weight_boxes.size(); ++b) {
      const avr::CoverBoxDev& mine = sums.weight_boxes[b];
      const avr::CoverBoxDev& theirs = sums.walk.boxes[b];
      const avr_box& in = s.weight[b];
      expect(mine.nx == theirs.nx && mine.ny == theirs.ny && mine.nz == theirs.nz &&
                 mine.level == theirs.level && mine.lo[0] == theirs.lo[0] &&
                 mine.lo[1] == theirs.lo[1] && mine.lo[2] == theirs.lo[2],
             name + ": a weight box is not the field's");
      if (mine.nx > 0) {
        expect(mine.cells == in.cells && mine.jstride == in.jstride && mine.kstride == in.kstride &&
                   mine.cells != theirs.cells && mine.jstride != theirs.jstride,
               name + ": a weight box has not its own cells and strides");
      }
    }
  }
}

void tables() {
  check_same_tables(two_levels(), "two levels");
  {  // three levels, ratios 4 and 2, negative indices, touching and nested boxes, a box without cells
    Scene s;
    s.n_levels = 3;
    s.ratio = {4, 2};
    s.add(0, -3, -2, -1, 5, 4, 3);
    s.add(0, 2, -2, -1, 3, 4, 3);
    s.add(1, -8, -4, 0, 8, 8, 4);
    s.add(2, -16, -8, 0, 0, 4, 4);
    s.field[3].cells = s.weight[3].cells = nullptr;
    s.add(1, 0, -4, 0, 4, 8, 4);
    s.add(2, -10, -6, 2, 7, 5, 3);
    s.add(2, -3, -6, 2, 9, 5, 3);
    check_same_tables(s, "three levels");
  }
  {  // a scene without cells: no locator, empty bounds, with a weight as without
    Scene none;
    none.add(0, 0, 0, 0, 0, 4, 4);
    none.field[0].cells = none.weight[0].cells = nullptr;
    const avr::RaySumsPlan empty = none.plan();
    expect(empty.walk.locator.n[0] == 0 && empty.walk.block_begin.size() == 1 &&
               empty.walk.block_boxes.empty(), "a scene without cells has no locator");
    expect(empty.walk.bound_hi[0] < empty.walk.bound_lo[0], "a scene without cells has empty bounds");
    check_same_tables(none, "no cells");
  }
}

}  // namespace

int main() {
  messages_and_precedence();
  tables();
  std::printf("ok\n");
  return 0;
}
