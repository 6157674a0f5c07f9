// The same-or-coarser cell lookup (csrc/avr_level_cells.h: find_same_or_coarser, floor_div) as a
// plain C++ program, built with AddressSanitizer and UBSan and without HIP: the function the
// gradient's halo and the isosurfaces' shell call in their kernels (the clumps' unite_ghost writes
// the same loop out), run here over every cell of every box's one-cell shell through the candidate lists the three host
// plans make (plan_isosurface's per box, plan_clumps' per face, plan_gradient's per side for each
// axis), each result held against a scan of all boxes.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../amrvolumerenderer_amd/csrc/avr_field_plans.h"
#include "../../amrvolumerenderer_amd/csrc/avr_level_cells.h"

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
  std::vector<avr_box> in, out;
  std::vector<int32_t> lo;
  std::vector<int32_t> ratio = {2, 4};
  int n_levels = 3;

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
};

// Three levels at ratios 2 and 4, the levels mixed in scene order.  Level 0 covers x in [-4, 4),
// y in [-2, 4) (less for x >= 0), z in [-2, 2); past it no box holds an index.
Scene scene() {
  Scene s;
  s.add(0, -4, -2, -2, 4, 4, 4);     //  0: level 0, negative indices
  s.add(2, 6, -4, -4, 6, 6, 6);      //  1: level 2 in box 5; its high-x ghost (level-1 x = 3) lies
                                     //     over the hole between boxes 5 and 7, which box 3 covers
  s.add(1, -6, -2, -2, 6, 4, 4);     //  2: level 1, touches box 5 at x = 0
  s.add(0, 0, -2, -2, 4, 4, 4);      //  3: level 0, touches box 0 at x = 0
  s.add(1, 0, 0, 0, 0, 3, 3);        //  4: no cells
  s.add(1, 0, -2, -2, 3, 4, 4);      //  5: level 1
  s.add(2, -16, -8, -8, 6, 5, 4);    //  6: level 2 in box 2; its low-y ghost (level-1 y = -3) lies
                                     //     below box 2, in box 0: floor(-9 / 4) = -3, not -2
  s.add(1, 4, -2, -2, 2, 4, 4);      //  7: level 1, a hole at x = 3
  s.add(2, 0, -4, -4, 6, 6, 6);      //  8: level 2, touches box 1 at x = 6
  s.add(0, -4, 2, -2, 4, 2, 4);      //  9: level 0, on top of box 0
  s.add(1, -6, 2, -2, 4, 3, 4);      // 10: level 1 over boxes 0 and 9
  s.add(2, -24, 8, -8, 5, 6, 3);     // 11: level 2 in box 10
  return s;
}

struct Want {
  int box;
  int64_t at[3];
};

// The rule, by a scan of all boxes: the box's level first, then every coarser one.
Want brute_force(const Scene& s, int level, const int64_t g[3]) {
  int64_t m[3] = {g[0], g[1], g[2]};
  for (int l = level; l >= 0; --l) {
    if (l < level) {
      for (int d = 0; d < 3; ++d) {
        const int64_t r = s.ratio[l];
        int64_t q = m[d] / r;
        if (m[d] % r != 0 && m[d] < 0) --q;
        m[d] = q;
      }
    }
    for (size_t c = 0; c < s.in.size(); ++c) {
      const avr_box& other = s.in[c];
      if (other.dims[0] <= 0 || other.level != l) continue;
      bool holds = true;
      for (int d = 0; d < 3; ++d) {
        holds = holds && m[d] >= s.lo[c * 3 + d] && m[d] < int64_t{s.lo[c * 3 + d]} + other.dims[d];
      }
      if (holds) return {static_cast<int>(c), {m[0] - s.lo[c * 3], m[1] - s.lo[c * 3 + 1],
                                               m[2] - s.lo[c * 3 + 2]}};
    }
  }
  return {-1, {0, 0, 0}};
}

template <class Box>
void check(const std::vector<Box>& boxes, const std::vector<int32_t>& candidates, uint32_t first,
           uint32_t last, const int32_t* ratio, int level, const int64_t g[3], const Want& want,
           const std::string& what) {
  expect(first <= last && last <= candidates.size(), what + ": a CSR range");
  const avr::LevelCell got = avr::find_same_or_coarser(boxes.data(), candidates.data(), first, last,
                                                       ratio, level, g[0], g[1], g[2]);
  const std::string where = what + " at (" + std::to_string(g[0]) + ", " + std::to_string(g[1]) +
                            ", " + std::to_string(g[2]) + ")";
  if (want.box < 0) {
    expect(got.box < 0, where + ": found box " + std::to_string(got.box) + ", none holds it");
    return;
  }
  expect(got.box == want.box, where + ": box " + std::to_string(got.box) + ", not " +
                                  std::to_string(want.box));
  expect(got.level == boxes[want.box].level, where + ": the level");
  expect(got.i == want.at[0] && got.j == want.at[1] && got.k == want.at[2], where + ": (i, j, k)");
}

void floor_division() {
  expect(avr::floor_div(-9, 4) == -3 && avr::floor_div(-8, 4) == -2 && avr::floor_div(-1, 2) == -1 &&
             avr::floor_div(7, 2) == 3 && avr::floor_div(0, 4) == 0 &&
             avr::floor_div(-(int64_t{1} << 30) - 1, 2) == -(int64_t{1} << 29) - 1,
         "floor_div");
}

void shells() {
  const Scene s = scene();
  const size_t n = s.in.size();
  const double sizes[9] = {1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.125, 0.125, 0.125};
  const double prob_lo[3] = {0.0, 0.0, 0.0};
  const double axis_sizes[3] = {1.0, 0.5, 0.125};
  const void* counts = reinterpret_cast<const void*>(uintptr_t{1} << 47);
  const avr::IsoPlan iso =
      avr::plan_isosurface(s.in.data(), nullptr, n, 0.5, s.lo.data(), s.ratio.data(), sizes, prob_lo,
                           s.n_levels, 0, nullptr, nullptr, nullptr, counts);
  const avr::ClumpPlan clumps = avr::plan_clumps(s.in.data(), s.out.data(), n, 0.0, 1.0,
                                                 s.lo.data(), s.ratio.data(), s.n_levels);
  std::vector<avr::GradientPlan> gradient;
  for (int axis = 0; axis < 3; ++axis) {
    gradient.push_back(avr::plan_gradient(s.in.data(), s.out.data(), n, axis, s.lo.data(),
                                          s.ratio.data(), axis_sizes, s.n_levels));
  }
  int absent = 0, same = 0, coarser = 0, skipped = 0, rounded_down = 0, faces = 0, touching = 0;
  bool empty_in_the_middle = false;
  for (size_t b = 0; b < n; ++b) {
    const avr_box& box = s.in[b];
    if (box.dims[0] <= 0) {
      expect(iso.candidate_begin[b] == iso.candidate_begin[b + 1], "a box without cells has no list");
      bool before = false, after = false;
      for (size_t c = 0; c < n; ++c) {
        if (s.in[c].dims[0] > 0) (c < b ? before : after) = true;
      }
      empty_in_the_middle = empty_in_the_middle || (before && after);
      continue;
    }
    for (int k = -1; k <= box.dims[2]; ++k) {
      for (int j = -1; j <= box.dims[1]; ++j) {
        for (int i = -1; i <= box.dims[0]; ++i) {
          const int at[3] = {i, j, k};
          int outside = 0, axis = 0;
          for (int d = 0; d < 3; ++d) {
            if (at[d] < 0 || at[d] >= box.dims[d]) {
              ++outside;
              axis = d;
            }
          }
          if (outside == 0) continue;
          const int64_t g[3] = {int64_t{s.lo[b * 3]} + i, int64_t{s.lo[b * 3 + 1]} + j,
                                int64_t{s.lo[b * 3 + 2]} + k};
          const Want want = brute_force(s, box.level, g);
          const std::string name = "box " + std::to_string(b);
          check(iso.boxes, iso.candidates, iso.candidate_begin[b], iso.candidate_begin[b + 1],
                iso.levels.ratio, box.level, g, want, name + ", the shell's list");
          if (want.box < 0) {
            ++absent;
          } else if (s.in[want.box].level == box.level) {
            ++same;
          } else {
            ++coarser;
            if (s.in[want.box].level < box.level - 1) ++skipped;
            for (int d = 0; d < 3; ++d) {
              if (g[d] < 0 && g[d] % s.ratio[box.level - 1] != 0) {
                ++rounded_down;
                break;
              }
            }
          }
          if (outside != 1) continue;  // an edge or a corner of the shell: no face's ghost
          ++faces;
          // a face cell's ghost in a box of the same level: the two boxes touch
          if (want.box >= 0 && s.in[want.box].level == box.level) ++touching;
          const int side = at[axis] < 0 ? 0 : 1;
          const size_t face = 6 * b + 2 * axis + side;
          check(clumps.boxes, clumps.candidates, clumps.candidate_begin[face],
                clumps.candidate_begin[face + 1], clumps.levels.ratio, box.level, g, want,
                name + ", face " + std::to_string(2 * axis + side));
          const avr::GradientPlan& plan = gradient[axis];
          check(plan.boxes, plan.candidates, plan.candidate_begin[2 * b + side],
                plan.candidate_begin[2 * b + side + 1], plan.levels.ratio, box.level, g, want,
                name + ", axis " + std::to_string(axis) + " side " + std::to_string(side));
        }
      }
    }
  }
  // the scene holds what it is meant to
  expect(absent > 0, "a ghost that no box holds");
  expect(same > 0 && coarser > 0, "ghosts of the same and of a coarser level");
  expect(skipped > 0, "a ghost over a hole in the next coarser level");
  expect(rounded_down > 0, "a negative ghost index that floor division rounds down");
  expect(faces > 0, "face ghosts");
  expect(touching > 0, "two boxes of one level that touch");
  expect(empty_in_the_middle, "a box without cells between boxes that have some");
}

}  // namespace

int main() {
  floor_division();
  shells();
  std::puts("ok");
  return 0;
}
