// The host plan of ray transfer (csrc/avr_field_plans.h: plan_ray_transfer) as a plain C++ program,
// built with AddressSanitizer and UBSan and without HIP: every refusal message and which one wins
// when several rules are broken, the three extra scenes' rules, 1024 and 1025 channels, the limit
// on channels x rays, the chunk arithmetic, the reciprocals' bits, the shared-byte rule over every
// output and all four scenes' cells to the byte, and that a grey plan holds plan_ray_sums' walk
// tables entry for entry.  No cell is ever allocated or read.  Prints "ok".
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
const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }

// Four scenes of descriptors over the same boxes: box b's cells are contiguous at a made-up address
// that nothing reads; scene f's from 2^40 + f 2^38 on, and scene f's rows are padded by f cells.
struct Scene {
  std::vector<avr_box> boxes[4];  // source, opacity, bin, width
  std::vector<int32_t> lo;
  std::vector<int32_t> ratio;
  std::vector<double> sizes = {0.5, 0.25, 1.0, 0.25, 0.125, 0.5, 0.0625, 0.03125, 0.125};
  std::vector<double> edges = {-2.0, -1.0, 0.5, 0.75, 4.0};
  double prob_lo[3] = {-1.0, 0.0, 2.0};
  uint64_t n_rays = 100, max_trips = 64;
  int n_levels = 1, n_channels = 4, chunk = 8;
  bool binned = true, broadened = true, no_opacity = false, no_edges = false;
  int64_t max_entries = avr::kStreamMaxEntries;
  const void* start = address(46);
  const void* end = address(47);
  const void* counts = address(49);
  const void* status = address(50);
  const void* span = address(51);
  const void* intensity = address(52);
  const void* tau = address(53);
  const void* outside = address(54);
  const void* counted = address(55);
  const void* covered = address(56);

  void add(int box_level, int x, int y, int z, int nx, int ny, int nz) {
    const uintptr_t stride = uintptr_t{1} << 31;  // bytes between two boxes: 2^28 cells
    for (int f = 0; f < 4; ++f) {
      avr_box box{};
      box.dims[0] = nx;
      box.dims[1] = ny;
      box.dims[2] = nz;
      box.level = box_level;
      box.jstride = nx + f;
      box.kstride = static_cast<int64_t>(nx + f) * ny;
      box.min_corner[0] = 0.25 * x;
      box.min_corner[1] = 0.25 * y;
      box.min_corner[2] = 0.25 * z;
      box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 40) + (uintptr_t(f) << 38) +
                                                  boxes[f].size() * stride);
      boxes[f].push_back(box);
    }
    lo.push_back(x);
    lo.push_back(y);
    lo.push_back(z);
  }
  avr::RayTransferPlan plan() const {
    const bool wide = broadened;
    return avr::plan_ray_transfer(
        boxes[0].data(), boxes[0].size(), no_opacity ? nullptr : boxes[1].data(), boxes[1].size(),
        binned ? boxes[2].data() : nullptr, binned ? boxes[2].size() : 0,
        wide ? boxes[3].data() : nullptr, wide ? boxes[3].size() : 0, n_rays, max_trips, lo.data(),
        ratio.empty() ? nullptr : ratio.data(), sizes.data(), prob_lo, n_levels,
        no_edges ? nullptr : edges.data(), n_channels, chunk, start, end, counts, status, span,
        intensity, tau, outside, counted, covered, max_entries);
  }
  avr::RaySumsPlan sums_plan() const {
    return avr::plan_ray_sums(boxes[0].data(), boxes[0].size(), nullptr, 0, n_rays, max_trips,
                              lo.data(), ratio.empty() ? nullptr : ratio.data(), sizes.data(),
                              prob_lo, n_levels, start, end, counts, status, span, intensity,
                              nullptr, counted, covered, max_entries);
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
const char* kLevels = "n_levels must lie in [1, 16]";
const char* kSizes = "level_cell_size must be finite and positive";
const char* kLevel = "a box's level is not below n_levels";
const char* kNoCells = "box has no cell data";
const char* kSpan = "box spans more than 2^28 cells (or has negative strides)";
const char* kOpacity = "the opacity scene's boxes differ from the source's";
const char* kBin = "the bin scene's boxes differ from the source's";
const char* kWidth = "the width scene's boxes differ from the source's";
const char* kRatio = "a level ratio is below 2";
const char* kShared = "an output array or the rays overlap an input box's cells";
const char* kNull = "null argument";
const char* kChannels = "n_channels must lie in [1, 1024]";
const char* kGrey = "n_channels must be 1 without a bin scene";
const char* kFinite = "edges must be finite";
const char* kIncreasing = "edges must be strictly increasing";
const char* kEntries = "the channels of all rays are 2^31 entries or more";
const char* kChunk = "the chunk must lie in [1, 32]";

#define REFUSED(message, change)                       \
  {                                                    \
    Scene s = two_levels();                            \
    change;                                            \
    expect_message(message, [&] { s.plan(); });        \
  }
#define ACCEPTED(change)    \
  {                         \
    Scene s = two_levels(); \
    change;                 \
    s.plan();               \
  }
// the sharp form; the grey form
#define SHARP (s.broadened = false)
#define GREY \
  (s.broadened = s.binned = false, s.no_edges = true, s.outside = nullptr, s.n_channels = 1)

void uniform_edges(Scene* s, int n) {
  s->n_channels = n;
  s->edges.resize(static_cast<size_t>(n) + 1);
  for (int i = 0; i <= n; ++i) s->edges[static_cast<size_t>(i)] = 0.1 * i;
}

void messages_and_precedence() {
  two_levels().plan();
  ACCEPTED(SHARP);
  ACCEPTED(GREY);
  // the plan's own rules
  REFUSED(kNull, s.no_opacity = true);
  REFUSED(kNull, (s.binned = false, s.no_edges = true, s.outside = nullptr));  // s without g
  REFUSED(kNull, s.no_edges = true);                                             // g without edges
  REFUSED(kNull, (GREY, s.no_edges = false));                                    // edges without g
  REFUSED(kNull, s.outside = nullptr);
  REFUSED(kNull, (GREY, s.outside = address(54)));
  ACCEPTED((s.n_rays = 0, s.outside = nullptr));  // no rays: no array is looked at
  REFUSED(kChannels, s.n_channels = 0);
  REFUSED(kChannels, s.n_channels = -3);
  ACCEPTED(uniform_edges(&s, 1024));
  REFUSED(kChannels, uniform_edges(&s, 1025));
  REFUSED(kGrey, (GREY, s.n_channels = 2));
  REFUSED(kGrey, (GREY, s.n_channels = 0));
  REFUSED(kFinite, s.edges[0] = -kInf);
  REFUSED(kFinite, s.edges[4] = kNaN);
  REFUSED(kIncreasing, s.edges[2] = s.edges[1]);
  REFUSED(kIncreasing, s.edges[3] = 5.0);
  ACCEPTED(s.n_rays = (uint64_t{1} << 29) - 1);   // 4 channels
  REFUSED(kEntries, s.n_rays = uint64_t{1} << 29);
  REFUSED(kEntries, (GREY, s.n_rays = uint64_t{1} << 31));
  ACCEPTED((GREY, s.n_rays = (uint64_t{1} << 31) - 1));
  REFUSED(kEntries, s.n_rays = ~uint64_t{0});
  REFUSED(kEntries, (uniform_edges(&s, 1024), s.n_rays = uint64_t{1} << 21));
  ACCEPTED((uniform_edges(&s, 1024), s.n_rays = (uint64_t{1} << 21) - 1));
  REFUSED(kChunk, s.chunk = 0);
  REFUSED(kChunk, s.chunk = 33);
  ACCEPTED(s.chunk = 32);
  // the walk's rules, a few of each kind: they are plan_ray_walk's, tested with plan_ray_sums
  REFUSED(kMaxTrips, s.max_trips = 0);
  REFUSED(kLevels, s.n_levels = 0);
  REFUSED(kNull, s.ratio.clear());
  REFUSED(kNull, s.start = nullptr);
  REFUSED(kNull, s.counts = nullptr);
  REFUSED(kNull, s.intensity = nullptr);
  REFUSED(kNull, s.tau = nullptr);
  REFUSED(kNull, s.counted = nullptr);
  REFUSED(kNull, (GREY, s.covered = nullptr));
  ACCEPTED((s.n_rays = 0, s.start = s.end = s.counts = s.status = s.span = s.intensity = s.tau =
                              s.outside = s.counted = s.covered = nullptr));
  REFUSED(kSizes, s.sizes[4] = 0.0);
  REFUSED(kLevel, s.boxes[0][2].level = 2);
  REFUSED(kNoCells, s.boxes[0][1].cells = nullptr);
  REFUSED(kRatio, s.ratio[0] = 1);
  // the three scenes: the count, then box by box level, dims and corner, then the view rule
  const char* differ[4] = {nullptr, kOpacity, kBin, kWidth};
  for (int f = 1; f < 4; ++f) {
    REFUSED(differ[f], s.boxes[f].pop_back());
    REFUSED(differ[f], s.boxes[f].push_back(s.boxes[f][0]));
    REFUSED(differ[f], s.boxes[f][2].level = 0);
    REFUSED(differ[f], s.boxes[f][1].dims[0] = 5);
    REFUSED(differ[f], s.boxes[f][2].dims[2] = 9);
    REFUSED(differ[f], s.boxes[f][1].min_corner[0] = 0.0);
    REFUSED(differ[f], std::swap(s.boxes[f][0], s.boxes[f][1]));
    REFUSED(kNoCells, s.boxes[f][1].cells = nullptr);
    REFUSED(kSpan, s.boxes[f][0].kstride = int64_t{1} << 28);
    REFUSED(kSpan, s.boxes[f][2].jstride = -8);
    ACCEPTED((s.boxes[f][1].jstride = 100, s.boxes[f][1].kstride = 1000));
  }
  ACCEPTED((SHARP, s.boxes[3][1].dims[0] = 5));   // not looked at
  ACCEPTED((GREY, s.boxes[2].pop_back()));
  {  // a box without cells needs none in any scene
    Scene s = two_levels();
    s.add(1, 40, 0, 0, 0, 4, 4);
    for (int f = 0; f < 4; ++f) s.boxes[f][3].cells = nullptr;
    const avr::RayTransferPlan plan = s.plan();
    expect(plan.width_boxes.size() == 4 && plan.width_boxes[3].nx == 0 &&
               plan.width_boxes[3].cells == nullptr, "a box without cells");
  }
  // which one wins
  REFUSED(kNull, (s.no_opacity = true, s.n_channels = 0));
  REFUSED(kNull, (s.outside = nullptr, s.edges[0] = kNaN));
  REFUSED(kChannels, (s.n_channels = 0, s.n_rays = ~uint64_t{0}));
  REFUSED(kFinite, (s.edges[1] = kInf, s.edges[3] = s.edges[2]));
  REFUSED(kIncreasing, (s.edges[1] = s.edges[0], s.edges[3] = kNaN));
  REFUSED(kIncreasing, (s.edges[2] = s.edges[1], s.n_rays = uint64_t{1} << 29));
  REFUSED(kEntries, (s.n_rays = uint64_t{1} << 29, s.chunk = 0));
  REFUSED(kChunk, (s.chunk = 0, s.max_trips = 0));
  REFUSED(kMaxTrips, (s.max_trips = 0, s.start = nullptr));
  REFUSED(kNull, (s.tau = nullptr, s.sizes[0] = 0.0));
  REFUSED(kNoCells, (s.boxes[0][2].cells = nullptr, s.boxes[1][0].dims[0] = 5));  // the source first
  REFUSED(kOpacity, (s.boxes[1].pop_back(), s.boxes[2].pop_back()));              // in their order
  REFUSED(kBin, (s.boxes[2][0].dims[0] = 5, s.boxes[3].pop_back()));
  REFUSED(kNoCells, (s.boxes[1][1].cells = nullptr, s.boxes[2].pop_back()));
  REFUSED(kWidth, (s.boxes[3][0].level = 1, s.ratio[0] = 1));
  REFUSED(kRatio, (s.ratio[0] = 1, s.tau = at(reinterpret_cast<uintptr_t>(s.boxes[2][0].cells))));
}

// Every output, start and end against a cell of each scene: the first byte, the last byte, one past.
void shared_bytes() {
  const Scene base = two_levels();
  for (int f = 0; f < 4; ++f) {
    // box 1: 4 x 4 x 4 cells, rows of 4 + f, planes of 4 (4 + f): the last cell's element
    const uintptr_t cells = reinterpret_cast<uintptr_t>(base.boxes[f][1].cells);
    const uintptr_t bytes = (3 + 3 * (4 + f) + 3 * 4 * (4 + f) + 1) * 8;
    const std::string name = "scene " + std::to_string(f);
    REFUSED(kShared, s.start = at(cells));
    REFUSED(kShared, s.end = at(cells + 8));
    REFUSED(kShared, s.counts = at(cells - 100 * 4 + 1));
    ACCEPTED(s.counts = at(cells - 100 * 4));
    REFUSED(kShared, s.status = at(cells + bytes - 1));
    ACCEPTED(s.status = at(cells + bytes));
    REFUSED(kShared, s.span = at(cells - 100 * 16 + 1));
    ACCEPTED(s.span = at(cells - 100 * 16));
    // intensity and tau: n_channels x n_rays entries
    REFUSED(kShared, s.intensity = at(cells - 4 * 100 * 8 + 1));
    ACCEPTED(s.intensity = at(cells - 4 * 100 * 8));
    REFUSED(kShared, s.tau = at(cells - 4 * 100 * 8 + 1));
    ACCEPTED(s.tau = at(cells - 4 * 100 * 8));
    REFUSED(kShared, s.tau = at(cells + bytes - 1));
    ACCEPTED(s.tau = at(cells + bytes));
    REFUSED(kShared, s.outside = at(cells - 2 * 100 * 8 + 1));
    ACCEPTED(s.outside = at(cells - 2 * 100 * 8));
    REFUSED(kShared, s.counted = at(cells - 100 * 8 + 1));
    ACCEPTED(s.counted = at(cells - 100 * 8));
    REFUSED(kShared, s.covered = at(cells + 16));
    ACCEPTED((s.n_rays = 0, s.start = at(cells)));  // nothing is read
    // a scene that is not part of the call: its cells are no input
    if (f == 3) ACCEPTED((SHARP, s.covered = at(cells)));
    if (f >= 2) ACCEPTED((GREY, s.covered = at(cells)));
    if (f < 2) REFUSED(kShared, (GREY, s.covered = at(cells)));
    // a grey plan has one channel
    if (f < 2) {
      REFUSED(kShared, (GREY, s.tau = at(cells - 100 * 8 + 1)));
      ACCEPTED((GREY, s.tau = at(cells - 100 * 8)));
    }
  }
}

uint64_t bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}

void chunks_and_reciprocals() {
  struct Want {
    int n_channels, chunk, plan_chunk;
    uint32_t n_chunks;
  };
  const Want wants[] = {{4, 8, 4, 1}, {4, 1, 1, 4}, {4, 3, 3, 2}, {4, 4, 4, 1}, {33, 8, 8, 5},
                        {33, 32, 32, 2}, {1024, 8, 8, 128}, {1024, 32, 32, 32}, {1, 8, 1, 1},
                        {7, 3, 3, 3}};
  for (const Want& w : wants) {
    Scene s = two_levels();
    s.n_rays = 1000;
    uniform_edges(&s, w.n_channels);
    s.chunk = w.chunk;
    const avr::RayTransferPlan plan = s.plan();
    const std::string name = std::to_string(w.n_channels) + " channels in chunks of " +
                             std::to_string(w.chunk);
    expect(plan.chunk == w.plan_chunk && plan.n_chunks == w.n_chunks, name + ": the chunks");
    expect(plan.walk.args.transfer.chunk == w.plan_chunk &&
               plan.walk.args.transfer.n_channels == w.n_channels, name + ": the launch arguments");
    // the chunk's edges and reciprocals, then [channel][2][lane] f64
    expect(plan.lds_bytes == (2u * w.plan_chunk + 1u + 128u * w.plan_chunk) * 8u, name + ": LDS");
    expect(plan.lds_bytes <= 64u * 1024u, name + ": LDS fits a workgroup");
    expect(plan.form == avr::kTransferBroadened, name + ": the form");
    expect(plan.edges == s.edges && plan.rdv.size() == static_cast<size_t>(w.n_channels),
           name + ": the tables");
    expect(plan.walk.args.transfer.lo == s.edges.front() &&
               plan.walk.args.transfer.hi == s.edges.back(), name + ": lo, hi");
  }
  {  // rdv[c]: one subtraction, then one correctly rounded division
    Scene s = two_levels();
    s.edges = {-2.0, -1.0, 0.5, 0.8, 4.0};
    const avr::RayTransferPlan plan = s.plan();
    for (size_t c = 0; c < 4; ++c) {
      volatile double dv = s.edges[c + 1] - s.edges[c];
      volatile double want = 1.0 / dv;
      expect(bits(plan.rdv[c]) == bits(want), "rdv's bits");
    }
    expect(plan.rdv[0] == 1.0 && bits(plan.rdv[2]) == bits(1.0 / (0.8 - 0.5)), "rdv's values");
  }
  {  // grey: one channel, one chunk, no LDS, no tables of channels
    Scene s = two_levels();
    GREY;
    const avr::RayTransferPlan plan = s.plan();
    expect(plan.form == avr::kTransferGrey && plan.n_channels == 1 && plan.chunk == 1 &&
               plan.n_chunks == 1 && plan.lds_bytes == 0 && plan.edges.empty() &&
               plan.rdv.empty() && plan.bin_boxes.empty() && plan.width_boxes.empty(), "grey");
  }
  {
    Scene s = two_levels();
    SHARP;
    const avr::RayTransferPlan plan = s.plan();
    expect(plan.form == avr::kTransferSharp && plan.bin_boxes.size() == 3 &&
               plan.width_boxes.empty(), "sharp");
  }
}

bool same_box(const avr::CoverBoxDev& a, const avr::CoverBoxDev& b) {
  return a.cells == b.cells && a.jstride == b.jstride && a.kstride == b.kstride && a.nx == b.nx &&
         a.ny == b.ny && a.nz == b.nz && a.level == b.level && a.lo[0] == b.lo[0] &&
         a.lo[1] == b.lo[1] && a.lo[2] == b.lo[2];
}

// plan_ray_sums over the source's boxes: the same walk tables entry for entry, in every form; and
// the other scenes' tables: the source's boxes with their own cells and strides.
void check_same_tables(const Scene& scene, const std::string& name) {
  for (int form = 0; form < 3; ++form) {
    Scene s = scene;
    if (form == 0) GREY;
    if (form == 1) SHARP;
    const avr::RayTransferPlan plan = s.plan();
    const avr::RayPlan& walk = plan.walk;
    const avr::RayPlan rays = s.sums_plan().walk;
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
    expect(walk.args.n_rays == rays.args.n_rays && walk.args.max_trips == rays.args.max_trips &&
               walk.args.n_levels == rays.args.n_levels, name + ": the launch arguments");
    const std::vector<avr::CoverBoxDev>* tables[4] = {nullptr, &plan.opacity_boxes,
                                                      &plan.bin_boxes, &plan.width_boxes};
    for (int f = 1; f < 4; ++f) {
      expect(tables[f]->size() == (f <= 1 + form ? s.boxes[0].size() : 0), name + ": a table's size");
      for (size_t b = 0; b < tables[f]->size(); ++b) {
        const avr::CoverBoxDev& mine = (*tables[f])[b];
        const avr::CoverBoxDev& theirs = walk.boxes[b];
        const avr_box& in = s.boxes[f][b];
        expect(mine.nx == theirs.nx && mine.ny == theirs.ny && mine.nz == theirs.nz &&
                   mine.level == theirs.level && mine.lo[0] == theirs.lo[0] &&
                   mine.lo[1] == theirs.lo[1] && mine.lo[2] == theirs.lo[2],
               name + ": a box is not the source's");
        if (mine.nx > 0) {
          expect(mine.cells == in.cells && mine.jstride == in.jstride &&
                     mine.kstride == in.kstride && mine.cells != theirs.cells &&
                     mine.jstride != theirs.jstride,
                 name + ": a box has not its own cells and strides");
        }
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
    for (int f = 0; f < 4; ++f) s.boxes[f][3].cells = nullptr;
    s.add(1, 0, -4, 0, 4, 8, 4);
    s.add(2, -10, -6, 2, 7, 5, 3);
    s.add(2, -3, -6, 2, 9, 5, 3);
    check_same_tables(s, "three levels");
  }
  {  // a scene without cells: no locator, empty bounds
    Scene none;
    none.add(0, 0, 0, 0, 0, 4, 4);
    for (int f = 0; f < 4; ++f) none.boxes[f][0].cells = nullptr;
    const avr::RayTransferPlan empty = none.plan();
    expect(empty.walk.locator.n[0] == 0 && empty.walk.block_begin.size() == 1 &&
               empty.walk.block_boxes.empty(), "a scene without cells has no locator");
    check_same_tables(none, "no cells");
  }
}

}  // namespace

int main() {
  messages_and_precedence();
  shared_bytes();
  chunks_and_reciprocals();
  tables();
  std::printf("ok\n");
  return 0;
}
