// The host plan of the isosurfaces (csrc/avr_field_plans.h: plan_isosurface) as a plain C++
// program, built with AddressSanitizer and UBSan and without HIP: every refusal message and which
// one wins when several rules are broken, base_begin and shell_begin, the numbering of a box's
// shell cells, the 2^31 rule (reached with descriptors only: no cell is ever allocated or read),
// the region candidates against an enumeration of every shell cell and its ancestors, and the
// face candidates of plan_clumps, which must be what they were.  Prints "ok".
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
  std::vector<avr_box> in, sample;
  std::vector<int32_t> lo;
  std::vector<int32_t> ratio;
  std::vector<double> sizes = {0.5, 0.25, 1.0, 0.25, 0.125, 0.5, 0.0625, 0.03125, 0.125};
  double prob_lo[3] = {-1.0, 0.0, 2.0};
  double value = 0.5;
  int n_levels = 1;
  bool with_sample = true;
  uint64_t capacity = 100;
  // made-up output addresses, far from every box
  const void* vertices = reinterpret_cast<const void*>(uintptr_t{1} << 44);
  const void* levels = reinterpret_cast<const void*>(uintptr_t{1} << 45);
  const void* samples = reinterpret_cast<const void*>(uintptr_t{1} << 46);
  const void* counts = reinterpret_cast<const void*>(uintptr_t{1} << 47);

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
    box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 41) + sample.size() * stride);
    sample.push_back(box);
    lo.push_back(x);
    lo.push_back(y);
    lo.push_back(z);
  }
  avr::IsoPlan plan() const {
    return avr::plan_isosurface(in.data(), with_sample ? sample.data() : nullptr, in.size(), value,
                                lo.data(), ratio.empty() ? nullptr : ratio.data(), sizes.data(),
                                prob_lo, n_levels, capacity, vertices, levels, samples, counts);
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

const char* kValue = "value must be finite";
const char* kLevels = "n_levels must lie in [1, 16]";
const char* kSizes = "level_cell_size must be finite and positive";
const char* kProbLo = "prob_lo must be finite";
const char* kCapacity = "capacity must stay below 2^36";
const char* kSamples = "samples_dev is given exactly when sample is";
const char* kDims = "the scenes' boxes differ in dims or level";
const char* kLevel = "a box's level is not below n_levels";
const char* kNoCells = "box has no cell data";
const char* kSpan = "box spans more than 2^28 cells (or has negative strides)";
const char* kRatio = "a level ratio is below 2";
const char* kRange = "a box's index range leaves [-2^30, 2^30)";
const char* kOverlap = "two boxes of one level overlap in index space";
const char* kShared = "an output array overlaps an input box's cells";
const char* kTooMany = "scene has too many cube bases";
const char* kNull = "null argument";

void messages_and_precedence() {
  two_levels().plan();  // in order
  // each rule alone
  { Scene s = two_levels(); s.value = kNaN; expect_message(kValue, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.value = kInf; expect_message(kValue, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.value = -kInf; expect_message(kValue, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.value = -1e308; s.plan(); }
  { Scene s = two_levels(); s.n_levels = 0; expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_levels = 17; s.ratio.assign(16, 2); s.sizes.assign(51, 1.0);
    expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.ratio.clear(); expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.sizes[4] = 0.0; expect_message(kSizes, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.sizes[0] = -0.5; expect_message(kSizes, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.sizes[5] = kInf; expect_message(kSizes, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.sizes[2] = kNaN; expect_message(kSizes, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.sizes[6] = kNaN; s.plan(); }  // of a level that is not there
  { Scene s = two_levels(); s.prob_lo[1] = kInf; expect_message(kProbLo, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.prob_lo[2] = kNaN; expect_message(kProbLo, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.capacity = uint64_t{1} << 36; expect_message(kCapacity, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.capacity = ~uint64_t{0}; expect_message(kCapacity, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.vertices = nullptr; expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.levels = nullptr; expect_message(kNull, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.samples = nullptr; expect_message(kSamples, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.with_sample = false; expect_message(kSamples, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.with_sample = false; s.samples = nullptr; s.plan(); }
  // the count-only call looks at none of the three arrays
  { Scene s = two_levels(); s.capacity = 0; s.vertices = s.levels = s.samples = nullptr; s.plan(); }
  { Scene s = two_levels(); s.capacity = 0; s.with_sample = false; s.plan(); }
  { Scene s = two_levels(); s.sample[1].dims[0] = 3; expect_message(kDims, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.sample[2].level = 0; expect_message(kDims, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[2].level = s.sample[2].level = 2; expect_message(kLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[0].level = s.sample[0].level = -1; expect_message(kLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[1].cells = nullptr; expect_message(kNoCells, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.sample[1].kstride = int64_t{1} << 28; expect_message(kSpan, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[1].jstride = -4; expect_message(kSpan, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.ratio[0] = 1; expect_message(kRatio, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[0] = (1 << 30) - 3; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[1] = -(1 << 30) - 1; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[0] = (1 << 30) - 4; s.lo[3] = -(1 << 30); s.plan(); }  // the ends
  { Scene s = two_levels(); s.lo[3] = 3; expect_message(kOverlap, [&] { s.plan(); }); }
  // every output against the field's and the sample's cells: the last byte in, the byte after out
  { Scene s = two_levels(); s.vertices = s.in[0].cells + 63; expect_message(kShared, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.vertices = s.in[0].cells + 64; s.plan(); }
  { Scene s = two_levels(); s.vertices = s.in[2].cells - 900; s.plan(); }  // 100 triangles end before
  { Scene s = two_levels(); s.vertices = s.in[2].cells - 899; expect_message(kShared, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.levels = reinterpret_cast<const char*>(s.sample[1].cells) - 100; s.plan(); }
  { Scene s = two_levels(); s.levels = reinterpret_cast<const char*>(s.sample[1].cells) - 99;
    expect_message(kShared, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.samples = s.sample[2].cells + 383; expect_message(kShared, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.samples = s.in[1].cells - 300; s.plan(); }
  { Scene s = two_levels(); s.samples = s.in[1].cells - 299; expect_message(kShared, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.counts = s.in[1].cells - 1; expect_message(kShared, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.counts = s.in[1].cells - 2; s.plan(); }
  { Scene s = two_levels(); s.capacity = 0; s.counts = s.sample[0].cells + 10;
    expect_message(kShared, [&] { s.plan(); }); }
  // with no capacity the arrays are not written: they may lie anywhere
  { Scene s = two_levels(); s.capacity = 0; s.vertices = s.in[0].cells; s.plan(); }
  // a box without cells takes no part: null cells, any index
  { Scene s = two_levels(); s.in[1].dims[1] = s.sample[1].dims[1] = 0;
    s.in[1].cells = s.sample[1].cells = nullptr; s.lo[3] = 0; const avr::IsoPlan p = s.plan();
    expect(p.base_begin == std::vector<uint32_t>({0, 125, 125, 125 + 7 * 9 * 9}), "base_begin with an empty box");
    expect(p.shell_begin == std::vector<uint64_t>({0, 152, 152, 152 + 8 * 10 * 10 - 6 * 8 * 8}),
           "shell_begin with an empty box");
    expect(p.boxes[1].nx == 0 && p.boxes[2].base_begin == 125 && p.boxes[2].shell_begin == 152,
           "the empty box's descriptor"); }

  // which rule wins: every earlier rule against a later one that can be broken with it
  { Scene s = two_levels(); s.value = kNaN; s.n_levels = 0; expect_message(kValue, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.n_levels = 17; s.sizes[0] = 0.0; expect_message(kLevels, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.sizes[1] = kNaN; s.prob_lo[0] = kNaN; expect_message(kSizes, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.prob_lo[0] = kNaN; s.capacity = uint64_t{1} << 40; expect_message(kProbLo, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.capacity = uint64_t{1} << 40; s.samples = nullptr; expect_message(kCapacity, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.samples = nullptr; s.sample[0].dims[0] = 1; expect_message(kSamples, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.sample[2].dims[2] = 1; s.ratio[0] = 0; expect_message(kDims, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.in[2].level = s.sample[2].level = 5; s.ratio[0] = 1; expect_message(kLevel, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.ratio[0] = -2; s.lo[0] = 1 << 30; expect_message(kRatio, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[6] = 1 << 30; s.lo[3] = 0; expect_message(kRange, [&] { s.plan(); }); }
  { Scene s = two_levels(); s.lo[3] = 0; s.vertices = s.in[0].cells; expect_message(kOverlap, [&] { s.plan(); }); }
}

void shell_numbering() {
  const int shapes[][3] = {{1, 1, 1}, {3, 1, 2}, {5, 4, 3}, {1, 6, 1}, {2, 2, 7}};
  for (const auto& n : shapes) {
    const uint64_t cells = avr::iso_shell_cells(n[0], n[1], n[2]);
    expect(cells == static_cast<uint64_t>(n[0] + 2) * (n[1] + 2) * (n[2] + 2) -
                        static_cast<uint64_t>(n[0]) * n[1] * n[2], "the shell's size");
    std::set<uint64_t> seen;
    for (int k = -1; k <= n[2]; ++k) {
      for (int j = -1; j <= n[1]; ++j) {
        for (int i = -1; i <= n[0]; ++i) {
          if (i >= 0 && i < n[0] && j >= 0 && j < n[1] && k >= 0 && k < n[2]) continue;
          const uint64_t at = avr::iso_shell_index(n[0], n[1], n[2], i, j, k);
          expect(at < cells, "a shell cell's number is below the shell's size");
          expect(seen.insert(at).second, "two shell cells share a number");
        }
      }
    }
    expect(seen.size() == cells, "the shell cells' numbers are a permutation");
  }
}

// 1023 x 511 x 511 cells: 2^28 cube bases per box, side by side along x
Scene huge(int n_boxes) {
  Scene s;
  s.with_sample = false;
  s.samples = nullptr;
  for (int b = 0; b < n_boxes; ++b) s.add(0, 1023 * b, 0, 0, 1023, 511, 511);
  return s;
}

void too_many_bases() {
  expect_message(kTooMany, [&] { huge(8).plan(); });
  expect_message(kTooMany, [&] { huge(9).plan(); });
  Scene s = huge(8);  // one plane of bases fewer: 2^31 - 2^18 bases
  s.in[7].dims[0] = 1022;
  const avr::IsoPlan p = s.plan();
  expect(p.base_begin.size() == 9 && p.base_begin[7] == 7u << 28 &&
             p.base_begin[8] == (1u << 31) - (1u << 18), "base_begin of 2^31 - 2^18 bases");
  expect(p.boxes[7].base_begin == 7u << 28, "the last box's first ordinal");
  expect(p.shell_begin[1] == avr::iso_shell_cells(1023, 511, 511) &&
             p.boxes[7].shell_begin == 7 * p.shell_begin[1], "shell_begin of large boxes");
  // the shared-byte rule comes first
  Scene t = huge(8);
  t.counts = t.in[5].cells;
  expect_message(kShared, [&] { t.plan(); });
}

int64_t floor_div(int64_t a, int64_t r) {
  int64_t q = a / r;
  if (a % r != 0 && a < 0) --q;
  return q;
}

// Three levels at ratios 2 and 4, with boxes at negative indices, boxes that touch at faces, edges
// and corners, a box whose face lies on a coarse box's face and a hole (clump_plan_test's scene
// and a box that touches box 3 at a corner only).
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
  s.add(1, 2, 2, 2, 2, 1, 1);      // meets box 3 at the corner (1, 1, 1) | (2, 2, 2) only
  return s;
}

// The boxes other than b of level <= b's that hold G, a level-(b's) index, or an ancestor of it.
void holders(const Scene& s, size_t b, const int64_t g[3], std::set<int32_t>* want) {
  int64_t m[3] = {g[0], g[1], g[2]};
  for (int level = s.in[b].level; level >= 0; --level) {
    if (level < s.in[b].level) {
      for (int d = 0; d < 3; ++d) m[d] = floor_div(m[d], s.ratio[level]);
    }
    for (size_t c = 0; c < s.in.size(); ++c) {
      const avr_box& other = s.in[c];
      if (c == b || other.dims[0] <= 0 || other.level != level) continue;
      bool holds = true;
      for (int d = 0; d < 3; ++d) {
        holds = holds && m[d] >= s.lo[c * 3 + d] && m[d] < int64_t{s.lo[c * 3 + d]} + other.dims[d];
      }
      if (holds) want->insert(static_cast<int32_t>(c));
    }
  }
}

void region_candidates() {
  const Scene s = hierarchy();
  const avr::IsoPlan plan = s.plan();
  const size_t n = s.in.size();
  expect(plan.candidate_begin.size() == n + 1 && plan.candidate_begin[0] == 0 &&
             plan.candidate_begin.back() == plan.candidates.size(), "the CSR's ends");
  size_t with_neighbours = 0;
  bool corner_only = false;
  for (size_t b = 0; b < n; ++b) {
    const avr_box& box = s.in[b];
    std::set<int32_t> want;
    if (box.dims[0] > 0) {
      for (int k = -1; k <= box.dims[2]; ++k) {
        for (int j = -1; j <= box.dims[1]; ++j) {
          for (int i = -1; i <= box.dims[0]; ++i) {
            if (i >= 0 && i < box.dims[0] && j >= 0 && j < box.dims[1] && k >= 0 && k < box.dims[2]) continue;
            const int64_t g[3] = {int64_t{s.lo[b * 3]} + i, int64_t{s.lo[b * 3 + 1]} + j,
                                  int64_t{s.lo[b * 3 + 2]} + k};
            holders(s, b, g, &want);
          }
        }
      }
      for (int d = 0; d < 3; ++d) expect(plan.boxes[b].lo[d] == s.lo[b * 3 + d], "a box's index");
    }
    const uint32_t first = plan.candidate_begin[b], last = plan.candidate_begin[b + 1];
    expect(first <= last && last <= plan.candidates.size(), "a CSR range");
    const std::vector<int32_t> got(plan.candidates.begin() + first, plan.candidates.begin() + last);
    expect(got == std::vector<int32_t>(want.begin(), want.end()),
           "the candidates of box " + std::to_string(b));
    if (!want.empty()) ++with_neighbours;
    if (b == 9) corner_only = want.count(3) == 1;
    for (int32_t c : got) expect(s.in[c].level <= box.level, "same or coarser only");
  }
  expect(with_neighbours >= 7 && corner_only, "most boxes have neighbours, one at a corner only");
}

// plan_clumps' face candidates on the same scene: what the six faces' ghost cells give, as before
// the search was generalised.
void face_candidates_are_unchanged() {
  const Scene s = hierarchy();
  std::vector<avr_box> out = s.sample;
  const avr::ClumpPlan plan = avr::plan_clumps(s.in.data(), out.data(), s.in.size(), 0.0, 1.0,
                                               s.lo.data(), s.ratio.data(), 3);
  const size_t n = s.in.size();
  expect(plan.candidate_begin.size() == 6 * n + 1, "the clumps' CSR");
  for (size_t b = 0; b < n; ++b) {
    const avr_box& box = s.in[b];
    for (int face = 0; face < 6; ++face) {
      const int axis = face >> 1, side = face & 1, u = (axis + 1) % 3, v = (axis + 2) % 3;
      std::set<int32_t> want;
      if (box.dims[0] > 0) {
        int64_t g[3];
        g[axis] = side == 0 ? int64_t{s.lo[b * 3 + axis]} - 1 : int64_t{s.lo[b * 3 + axis]} + box.dims[axis];
        for (int a = 0; a < box.dims[u]; ++a) {
          for (int c = 0; c < box.dims[v]; ++c) {
            g[u] = s.lo[b * 3 + u] + a;
            g[v] = s.lo[b * 3 + v] + c;
            holders(s, b, g, &want);
          }
        }
      }
      const std::vector<int32_t> got(plan.candidates.begin() + plan.candidate_begin[6 * b + face],
                                     plan.candidates.begin() + plan.candidate_begin[6 * b + face + 1]);
      expect(got == std::vector<int32_t>(want.begin(), want.end()),
             "the face candidates of box " + std::to_string(b) + " face " + std::to_string(face));
    }
  }
  // the gradient's lists, which look one level finer as well
  const avr::GradientPlan gradient = avr::plan_gradient(s.in.data(), out.data(), n, 0, s.lo.data(),
                                                        s.ratio.data(), s.sizes.data(), 3);
  expect(gradient.candidate_begin.size() == 2 * n + 1, "the gradient's CSR");
  for (size_t b = 0; b < n; ++b) {
    for (int side = 0; side < 2; ++side) {
      // without the finer boxes they are the clumps' lists of the x faces
      std::vector<int32_t> coarse;
      for (uint32_t q = gradient.candidate_begin[2 * b + side]; q < gradient.candidate_begin[2 * b + side + 1]; ++q) {
        if (s.in[gradient.candidates[q]].level <= s.in[b].level) coarse.push_back(gradient.candidates[q]);
      }
      const std::vector<int32_t> clump(plan.candidates.begin() + plan.candidate_begin[6 * b + side],
                                       plan.candidates.begin() + plan.candidate_begin[6 * b + side + 1]);
      expect(coarse == clump, "the gradient's same-or-coarser candidates");
    }
  }
}

}  // namespace

int main() {
  messages_and_precedence();
  shell_numbering();
  too_many_bases();
  region_candidates();
  face_candidates_are_unchanged();
  std::puts("ok");
  return 0;
}
