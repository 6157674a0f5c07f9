// The host plan of the streamlines (csrc/avr_field_plans.h: plan_streamlines) as a plain C++
// program, built with AddressSanitizer and UBSan and without HIP: every refusal message and which
// one wins when several rules are broken, the size rules (reached with descriptors only: no cell
// is ever allocated or read), and the locator against brute force -- for every cell of every box
// and every cell of every box's one-cell ghost shell, the list of the cell's block holds every
// box that a scan of all boxes finds for it at its own and at every coarser level, the lists are
// ordered finest level first and then in scene order, and a walk of the list as the kernel walks
// it ends at the box the scan ends at.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

// A scene of descriptors: box b's cells are contiguous at a made-up address that nothing reads.
struct Scene {
  std::vector<avr_box> vx, vy, vz, sample;
  std::vector<int32_t> lo;
  std::vector<int32_t> ratio;
  std::vector<double> sizes = {0.5, 0.25, 1.0, 0.25, 0.125, 0.5, 0.0625, 0.03125, 0.125};
  double prob_lo[3] = {-1.0, 0.0, 2.0};
  double step = 0.5;
  int direction = 1;
  uint64_t n_seeds = 100, max_steps = 64;
  int n_levels = 1;
  bool with_sample = true;
  int64_t max_entries = avr::kStreamMaxEntries;
  // made-up addresses, far from every box
  const void* seeds = reinterpret_cast<const void*>(uintptr_t{1} << 50);
  const void* points = reinterpret_cast<const void*>(uintptr_t{1} << 51);
  const void* samples = reinterpret_cast<const void*>(uintptr_t{1} << 52);
  const void* counts = reinterpret_cast<const void*>(uintptr_t{1} << 53);
  const void* status = reinterpret_cast<const void*>(uintptr_t{1} << 54);

  void add(int level, int x, int y, int z, int nx, int ny, int nz) {
    const uintptr_t stride = uintptr_t{1} << 31;  // bytes between two boxes: 2^28 cells
    avr_box box{};
    box.dims[0] = nx;
    box.dims[1] = ny;
    box.dims[2] = nz;
    box.level = level;
    box.jstride = nx;
    box.kstride = static_cast<int64_t>(nx) * ny;
    std::vector<avr_box>* fields[4] = {&vx, &vy, &vz, &sample};
    for (int f = 0; f < 4; ++f) {
      box.cells = reinterpret_cast<const double*>((uintptr_t{1} << (40 + f)) + fields[f]->size() * stride);
      fields[f]->push_back(box);
    }
    lo.push_back(x);
    lo.push_back(y);
    lo.push_back(z);
  }
  avr::StreamPlan plan() const {
    return avr::plan_streamlines(vx.data(), vy.data(), vz.data(),
                                 with_sample ? sample.data() : nullptr, vx.size(), n_seeds, step,
                                 direction, max_steps, lo.data(),
                                 ratio.empty() ? nullptr : ratio.data(), sizes.data(), prob_lo,
                                 n_levels, seeds, points, samples, counts, status, max_entries);
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

const char* kStep = "step must be finite and lie in (0, 1]";
const char* kDirection = "direction must be +1 or -1";
const char* kMaxSteps = "max_steps must not exceed 2^20";
const char* kSlots = "n_seeds * (max_steps + 1) must stay below 2^32";
const char* kLevels = "n_levels must lie in [1, 16]";
const char* kSizes = "level_cell_size must be finite and positive";
const char* kProbLo = "prob_lo must be finite";
const char* kSamples = "samples_dev is given exactly when sample is";
const char* kDims = "the scenes' boxes differ in dims or level";
const char* kLevel = "a box's level is not below n_levels";
const char* kNoCells = "box has no cell data";
const char* kSpan = "box spans more than 2^28 cells (or has negative strides)";
const char* kRatio = "a level ratio is below 2";
const char* kRange = "a box's index range leaves [-2^30, 2^30)";
const char* kOverlap = "two boxes of one level overlap in index space";
const char* kShared = "an output array or the seeds overlap an input box's cells";
const char* kLocator = "the locator's lists hold 2^28 entries or more";
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
  two_levels().plan();  // in order
  // each rule alone
  REFUSED(kStep, s.step = 0.0);
  REFUSED(kStep, s.step = -0.5);
  REFUSED(kStep, s.step = kNaN);
  REFUSED(kStep, s.step = kInf);
  REFUSED(kStep, s.step = 2.0);
  REFUSED(kStep, s.step = 1.0000000000000002);
  ACCEPTED(s.step = 1.0);
  ACCEPTED(s.step = 4.9e-324);
  REFUSED(kDirection, s.direction = 0);
  REFUSED(kDirection, s.direction = 2);
  ACCEPTED(s.direction = -1);
  REFUSED(kMaxSteps, (s.max_steps = (uint64_t{1} << 20) + 1, s.n_seeds = 1));
  REFUSED(kMaxSteps, (s.max_steps = ~uint64_t{0}, s.n_seeds = 1));
  ACCEPTED((s.max_steps = uint64_t{1} << 20, s.n_seeds = 4095));
  ACCEPTED(s.max_steps = 0);
  REFUSED(kSlots, (s.max_steps = uint64_t{1} << 20, s.n_seeds = 4096));
  REFUSED(kSlots, (s.max_steps = 0, s.n_seeds = uint64_t{1} << 32));
  REFUSED(kSlots, (s.max_steps = 1, s.n_seeds = uint64_t{1} << 63));  // the product wraps to 0
  REFUSED(kSlots, (s.max_steps = 3, s.n_seeds = uint64_t{1} << 30));
  ACCEPTED((s.max_steps = 0, s.n_seeds = (uint64_t{1} << 32) - 1));
  REFUSED(kLevels, s.n_levels = 0);
  REFUSED(kLevels, (s.n_levels = 17, s.ratio.assign(16, 2), s.sizes.assign(51, 1.0)));
  REFUSED(kNull, s.ratio.clear());
  REFUSED(kNull, s.seeds = nullptr);
  REFUSED(kNull, s.points = nullptr);
  REFUSED(kNull, s.counts = nullptr);
  REFUSED(kNull, s.status = nullptr);
  REFUSED(kSizes, s.sizes[4] = 0.0);
  REFUSED(kSizes, s.sizes[0] = -0.5);
  REFUSED(kSizes, s.sizes[5] = kInf);
  REFUSED(kSizes, s.sizes[2] = kNaN);
  ACCEPTED(s.sizes[6] = kNaN);  // of a level that is not there
  REFUSED(kProbLo, s.prob_lo[1] = kInf);
  REFUSED(kProbLo, s.prob_lo[2] = kNaN);
  REFUSED(kSamples, s.samples = nullptr);
  REFUSED(kSamples, s.with_sample = false);
  ACCEPTED((s.with_sample = false, s.samples = nullptr));
  // no seeds: the arrays may be null, the other rules hold
  ACCEPTED((s.n_seeds = 0, s.seeds = s.points = s.counts = s.status = nullptr));
  REFUSED(kSamples, (s.n_seeds = 0, s.samples = nullptr));
  REFUSED(kStep, (s.n_seeds = 0, s.step = 0.0));
  REFUSED(kDims, s.vy[1].dims[0] = 3);
  REFUSED(kDims, s.vz[2].level = 0);
  REFUSED(kDims, s.sample[0].dims[2] = 5);
  ACCEPTED((s.with_sample = false, s.samples = nullptr, s.sample[0].dims[2] = 5));  // not looked at
  REFUSED(kLevel, s.vx[2].level = s.vy[2].level = s.vz[2].level = s.sample[2].level = 2);
  REFUSED(kLevel, s.vx[0].level = s.vy[0].level = s.vz[0].level = s.sample[0].level = -1);
  REFUSED(kNoCells, s.vz[1].cells = nullptr);
  REFUSED(kNoCells, s.sample[1].cells = nullptr);
  REFUSED(kSpan, s.vy[0].kstride = int64_t{1} << 28);
  REFUSED(kSpan, s.vx[0].jstride = -4);
  REFUSED(kRatio, s.ratio[0] = 1);
  REFUSED(kRatio, s.ratio[0] = 0);
  REFUSED(kRatio, s.ratio[0] = -2);
  REFUSED(kRange, s.lo[0] = (1 << 30) - 3);
  REFUSED(kRange, s.lo[7] = -(1 << 30) - 1);
  ACCEPTED(s.lo[0] = (1 << 30) - 8);
  ACCEPTED(s.lo[8] = -(1 << 30));
  REFUSED(kOverlap, s.lo[3] = 3);
  ACCEPTED(s.lo[6] = 0);  // another level's box over the same indices
  // an output array, or the seeds, on an input box's cells: first byte, last byte, one past
  const uintptr_t cells = reinterpret_cast<uintptr_t>(two_levels().vz[1].cells);
  REFUSED(kShared, s.points = reinterpret_cast<const void*>(cells));
  REFUSED(kShared, s.seeds = reinterpret_cast<const void*>(cells + 8));
  REFUSED(kShared, s.status = reinterpret_cast<const void*>(cells + 64 * 8 - 1));
  ACCEPTED(s.status = reinterpret_cast<const void*>(cells + 64 * 8));
  REFUSED(kShared, s.counts = reinterpret_cast<const void*>(cells - 100 * 4 + 1));
  ACCEPTED(s.counts = reinterpret_cast<const void*>(cells - 100 * 4));
  REFUSED(kShared, s.samples = reinterpret_cast<const void*>(
                       reinterpret_cast<uintptr_t>(two_levels().sample[2].cells) + 16));
  ACCEPTED((s.with_sample = false,
            s.samples = nullptr,  // the sample scene's cells are not read without it
            s.points = reinterpret_cast<const void*>(
                reinterpret_cast<uintptr_t>(two_levels().sample[2].cells))));
  ACCEPTED((s.n_seeds = 0, s.points = reinterpret_cast<const void*>(cells)));  // nothing is written
  REFUSED(kLocator, s.max_entries = 3);
  // which one wins: the rules in the order of the definition
  REFUSED(kStep, (s.step = 0.0, s.direction = 0));
  REFUSED(kDirection, (s.direction = 0, s.max_steps = uint64_t{1} << 21));
  REFUSED(kMaxSteps, (s.max_steps = uint64_t{1} << 21, s.n_seeds = uint64_t{1} << 32));
  REFUSED(kSlots, (s.n_seeds = uint64_t{1} << 32, s.n_levels = 0));
  REFUSED(kLevels, (s.n_levels = 0, s.sizes[0] = 0.0));
  REFUSED(kSizes, (s.sizes[0] = 0.0, s.prob_lo[0] = kNaN));
  REFUSED(kProbLo, (s.prob_lo[0] = kNaN, s.samples = nullptr));
  REFUSED(kSamples, (s.samples = nullptr, s.vy[0].dims[0] = 3));
  REFUSED(kDims, (s.vy[0].dims[0] = 3, s.ratio[0] = 1));
  REFUSED(kNoCells, (s.vz[0].cells = nullptr, s.ratio[0] = 1));
  REFUSED(kRatio, (s.ratio[0] = 1, s.lo[0] = 1 << 30));
  REFUSED(kRange, (s.lo[0] = 1 << 30, s.lo[3] = 3));
  REFUSED(kOverlap, (s.lo[3] = 3, s.points = reinterpret_cast<const void*>(cells)));
  REFUSED(kShared, (s.points = reinterpret_cast<const void*>(cells), s.max_entries = 3));
}

// The largest scenes the rules admit, from descriptors alone.
void size_rules() {
  Scene s;
  s.n_levels = 1;
  s.add(0, -(1 << 30), -(1 << 30), -(1 << 30), 1, 1, 1);
  s.add(0, (1 << 30) - 1, (1 << 30) - 1, (1 << 30) - 1, 1, 1, 1);
  s.n_seeds = 4095;
  s.max_steps = uint64_t{1} << 20;
  const avr::StreamPlan plan = s.plan();
  // two boxes: at most 64 + 16 blocks over 2^31 indices along every axis, so 4 x 4 x 4 of 2^29
  const avr::StreamLocatorDev& locator = plan.locator;
  expect(locator.origin[0] == -(1 << 30) && locator.shift == 29, "the widest locator's blocks");
  expect(locator.n[0] == 4 && locator.n[1] == 4 && locator.n[2] == 4, "the widest locator's shape");
  expect(plan.block_begin.size() == 65 && plan.block_boxes.size() == 2, "the widest locator's lists");
  expect(plan.block_begin[1] == 1 && plan.block_begin[63] == 1 && plan.block_begin[64] == 2 &&
             plan.block_boxes[0] == 0 && plan.block_boxes[1] == 1, "the widest locator's entries");
  // a scene without cells: no block at all
  Scene none;
  none.add(0, 0, 0, 0, 0, 4, 4);
  none.vx[0].cells = none.vy[0].cells = none.vz[0].cells = none.sample[0].cells = nullptr;
  const avr::StreamPlan empty = none.plan();
  expect(empty.locator.n[0] == 0 && empty.block_begin.size() == 1 && empty.block_boxes.empty(),
         "a scene without cells has no locator");
  // the lists' bound, just met and just missed: three boxes, one block each
  Scene three = two_levels();
  three.max_entries = 100;
  const size_t entries = three.plan().block_boxes.size();
  three.max_entries = static_cast<int64_t>(entries) + 1;
  three.plan();
  three.max_entries = static_cast<int64_t>(entries);
  expect_message(kLocator, [&] { three.plan(); });
}

int64_t floor_div(int64_t a, int64_t r) { return avr::floor_div(a, r); }

// The box that holds the level-`level` index g at level m (mapped down by floor division), by a
// scan of all boxes; -1: none.
int scan(const Scene& s, int level, const int64_t g[3], int m) {
  int64_t at[3] = {g[0], g[1], g[2]};
  for (int l = level; l > m; --l) {
    for (int d = 0; d < 3; ++d) at[d] = floor_div(at[d], s.ratio[l - 1]);
  }
  for (size_t b = 0; b < s.vx.size(); ++b) {
    const avr_box& box = s.vx[b];
    if (box.level != m || box.dims[0] <= 0 || box.dims[1] <= 0 || box.dims[2] <= 0) continue;
    bool inside = true;
    for (int d = 0; d < 3; ++d) {
      inside = inside && at[d] >= s.lo[b * 3 + d] && at[d] < s.lo[b * 3 + d] + box.dims[d];
    }
    if (inside) return static_cast<int>(b);
  }
  return -1;
}

void check_locator(const Scene& s, const std::string& name) {
  const avr::StreamPlan plan = s.plan();
  const avr::StreamLocatorDev& locator = plan.locator;
  const size_t blocks = static_cast<size_t>(locator.n[0]) * locator.n[1] * locator.n[2];
  expect(plan.block_begin.size() == blocks + 1 && plan.block_begin[0] == 0 &&
             plan.block_begin[blocks] == plan.block_boxes.size(), name + ": the CSR's ends");
  size_t with_cells = 0;
  for (const avr_box& box : s.vx) with_cells += box.dims[0] > 0 && box.dims[1] > 0 && box.dims[2] > 0;
  expect(static_cast<int64_t>(blocks) <= 64 + 8 * static_cast<int64_t>(with_cells),
         name + ": a few blocks per box");
  // the order of every list: finest level first, then scene order; no box twice
  for (size_t block = 0; block < blocks; ++block) {
    expect(plan.block_begin[block] <= plan.block_begin[block + 1], name + ": the CSR ascends");
    for (uint32_t e = plan.block_begin[block] + 1; e < plan.block_begin[block + 1]; ++e) {
      const int32_t before = plan.block_boxes[e - 1], here = plan.block_boxes[e];
      const int lb = plan.boxes[before].level, lh = plan.boxes[here].level;
      expect(lb > lh || (lb == lh && before < here), name + ": a list's order");
    }
  }
  uint64_t checked = 0;
  for (size_t b = 0; b < s.vx.size(); ++b) {
    const avr_box& box = s.vx[b];
    if (box.dims[0] <= 0 || box.dims[1] <= 0 || box.dims[2] <= 0) continue;
    const int level = box.level;
    // the box's cells and its one-cell ghost shell
    for (int64_t k = -1; k <= box.dims[2]; ++k) {
      for (int64_t j = -1; j <= box.dims[1]; ++j) {
        for (int64_t i = -1; i <= box.dims[0]; ++i) {
          const int64_t g[3] = {s.lo[b * 3] + i, s.lo[b * 3 + 1] + j, s.lo[b * 3 + 2] + k};
          int64_t zero[3] = {g[0], g[1], g[2]};
          for (int l = level; l > 0; --l) {
            for (int d = 0; d < 3; ++d) zero[d] = floor_div(zero[d], s.ratio[l - 1]);
          }
          // the block, as the kernel finds it
          bool has_block = true;
          uint32_t at[3];
          for (int d = 0; d < 3; ++d) {
            has_block = has_block && zero[d] >= locator.origin[d];
            at[d] = (static_cast<uint32_t>(static_cast<int32_t>(zero[d])) -
                     static_cast<uint32_t>(locator.origin[d])) >> locator.shift;
            has_block = has_block && at[d] < static_cast<uint32_t>(locator.n[d]);
          }
          uint32_t first = 0, last = 0;
          if (has_block) {
            const size_t block = (static_cast<size_t>(at[2]) * locator.n[1] + at[1]) * locator.n[0] + at[0];
            first = plan.block_begin[block];
            last = plan.block_begin[block + 1];
          }
          // every level's holder is in the list, and the kernel's walk finds the finest of them
          int wanted = -1;
          for (int m = level; m >= 0; --m) {
            const int holder = scan(s, level, g, m);
            if (holder < 0) continue;
            if (wanted < 0) wanted = holder;
            bool listed = false;
            for (uint32_t e = first; e < last; ++e) listed = listed || plan.block_boxes[e] == holder;
            expect(listed, name + ": a box that holds a cell is missing from its block's list");
          }
          int found = -1, mapped_to = level;
          int64_t c[3] = {g[0], g[1], g[2]};
          for (uint32_t e = first; e < last && found < 0; ++e) {
            const int32_t other = plan.block_boxes[e];
            const avr::StreamBoxDev& dev = plan.boxes[other];
            if (dev.level > level) continue;
            for (; mapped_to > dev.level; --mapped_to) {
              for (int d = 0; d < 3; ++d) c[d] = floor_div(c[d], s.ratio[mapped_to - 1]);
            }
            if (c[0] >= dev.lo[0] && c[0] < dev.lo[0] + dev.nx && c[1] >= dev.lo[1] &&
                c[1] < dev.lo[1] + dev.ny && c[2] >= dev.lo[2] && c[2] < dev.lo[2] + dev.nz) {
              found = other;
            }
          }
          expect(found == wanted, name + ": the walk of a list ends at another box than the scan");
          const bool own = i >= 0 && i < box.dims[0] && j >= 0 && j < box.dims[1] && k >= 0 &&
                           k < box.dims[2];
          expect(!own || found == static_cast<int>(b), name + ": a box's own cell");
          ++checked;
        }
      }
    }
  }
  expect(checked > 0, name + ": nothing was checked");
}

void locators() {
  check_locator(two_levels(), "two levels");
  {  // three levels, ratios 4 and 2, negative indices, touching and nested boxes, a box without cells
    Scene s;
    s.n_levels = 3;
    s.ratio = {4, 2};
    s.add(0, -3, -2, -1, 5, 4, 3);
    s.add(0, 2, -2, -1, 3, 4, 3);
    s.add(1, -8, -4, 0, 8, 8, 4);
    s.add(2, -16, -8, 0, 0, 4, 4);
    s.vx[3].cells = s.vy[3].cells = s.vz[3].cells = s.sample[3].cells = nullptr;
    s.add(1, 0, -4, 0, 4, 8, 4);
    s.add(2, -10, -6, 2, 7, 5, 3);
    s.add(2, -3, -6, 2, 9, 5, 3);
    check_locator(s, "three levels");
  }
  {  // a level that overlaps the one below it, and a skipped level
    Scene s;
    s.n_levels = 3;
    s.ratio = {2, 2};
    s.add(0, 0, 0, 0, 8, 4, 4);
    s.add(2, 16, 8, 8, 8, 8, 8);
    s.add(1, 2, 2, 2, 6, 4, 4);
    check_locator(s, "overlapping levels");
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
    check_locator(s, "many boxes");
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
