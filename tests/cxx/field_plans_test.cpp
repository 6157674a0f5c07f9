// CPU check of the host plans of the field products (amrvolumerenderer_amd/csrc/
// avr_field_plans.h): the derive program's verifier, the shared-byte rule, the gradient's
// neighbour search, the on-axis projection's plane tables, the joint histogram's edge rules and
// the slice's box table.  What is expected is worked out here from definitions of its own
// (enumeration, hand-written tables), never by calling the code under test.  Cells are never
// dereferenced by that code, so made-up addresses stand for them.
//   field_plans_test      runs all cases, prints "ok", exit code 0
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../amrvolumerenderer_amd/csrc/avr_field_plans.h"

// The stage-1 tiling of the on-axis projection belongs to its kernel file, which is not linked
// here; the plan only sums what it returns.  One tile per box with cells keeps the tile prefix
// away from its own 2^31 limit, whose message the entry limit shares.
namespace avr {
uint32_t axis_projection_tiles(int, int, int, int) { return 1; }
}  // namespace avr

namespace {

int failures = 0;
void expect(bool ok, const std::string& what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s\n", what.c_str());
    ++failures;
  }
}

// the message a call refuses with; "" if it does not
template <typename F>
std::string refusal(F&& call) {
  try {
    call();
  } catch (const std::invalid_argument& e) {
    return e.what();
  }
  return "";
}

const double kInf = std::numeric_limits<double>::infinity();
const double kNan = std::numeric_limits<double>::quiet_NaN();

const double* address(uintptr_t a) { return reinterpret_cast<const double*>(a); }
const uintptr_t kBase = 0x100000;  // 16-byte aligned

// a dense box of nx x ny x nz cells
avr_box box(int nx, int ny, int nz, int level = 0, const double* cells = address(kBase)) {
  avr_box b{};
  b.dims[0] = nx;
  b.dims[1] = ny;
  b.dims[2] = nz;
  b.level = level;
  b.cells = cells;
  b.jstride = nx;
  b.kstride = static_cast<int64_t>(nx) * ny;
  for (int a = 0; a < 3; ++a) b.max_corner[a] = 1.0;
  return b;
}

uint32_t tiles_of(const avr_box& b) {  // 4 k-planes x 4 j-rows x 128 cells along x
  if (b.dims[0] <= 0 || b.dims[1] <= 0 || b.dims[2] <= 0) return 0;
  return static_cast<uint32_t>(((b.dims[0] + 127) / 128) * ((b.dims[1] + 3) / 4) *
                               ((b.dims[2] + 3) / 4));
}

// ---- derive: the verifier ------------------------------------------------------------------
const char* const kUnknown = "unknown opcode";
const char* const kOperandRange = "an operand index is out of range";
const char* const kOperatorOperand = "an operator takes no operand";
const char* const kUnderflow = "the program underflows its stack";
const char* const kDeep = "the program's stack is deeper than 8";
const char* const kOneValue = "the program must end with exactly one value";

uint32_t ins(uint32_t op, uint32_t operand = 0) { return op | (operand << 8); }
const uint32_t kConst0 = 0;  // push constants[0]

std::string verify(const std::vector<uint32_t>& code, int n_constants = 1, int n_inputs = 1) {
  return refusal([&] {
    avr::verify_derive_program(code.data(), static_cast<int>(code.size()), n_constants, n_inputs);
  });
}

void derive_verifier() {
  const uint32_t unary[] = {7, 8, 9, 10};                        // neg, square, sqrt, abs
  const uint32_t binary[] = {3, 4, 5, 6, 11, 12, 13, 14, 15, 16, 17, 18};
  const uint32_t where = 19;
  expect(verify({kConst0}) == "", "verifier: one constant");
  expect(verify({ins(20)}) == kUnknown && verify({ins(255)}) == kUnknown, "verifier: opcodes 20 and 255");
  for (uint32_t op : unary) {
    expect(verify({kConst0, ins(op)}) == "", "verifier: a unary operator pops one");
    expect(verify({ins(op)}) == kUnderflow, "verifier: a unary operator on an empty stack");
    expect(verify({kConst0, kConst0, ins(op)}) == kOneValue, "verifier: a unary operator leaves the rest");
    expect(verify({kConst0, ins(op, 1)}) == kOperatorOperand, "verifier: an operand on a unary operator");
  }
  for (uint32_t op : binary) {
    expect(verify({kConst0, kConst0, ins(op)}) == "", "verifier: a binary operator pops two");
    expect(verify({kConst0, ins(op)}) == kUnderflow, "verifier: a binary operator on one value");
    expect(verify({kConst0, kConst0, ins(op, 1)}) == kOperatorOperand,
           "verifier: an operand on a binary operator");
  }
  expect(verify({kConst0, kConst0, kConst0, ins(where)}) == "", "verifier: where pops three");
  expect(verify({kConst0, kConst0, ins(where)}) == kUnderflow, "verifier: where on two values");
  expect(verify({kConst0, kConst0, kConst0, kConst0, ins(where)}) == kOneValue,
         "verifier: where leaves the fourth value");
  expect(verify({kConst0, kConst0, kConst0, ins(where, 3)}) == kOperatorOperand,
         "verifier: an operand on where");
  {
    std::vector<uint32_t> code(8, kConst0);  // depth 8, folded by seven adds
    code.insert(code.end(), 7, ins(3));
    expect(verify(code) == "", "verifier: depth 8 passes");
    code.insert(code.begin(), kConst0);
    code.push_back(ins(3));
    expect(verify(code) == kDeep, "verifier: depth 9 is refused");
  }
  // operand limits: constants (op 0), fields (op 1), built-ins (op 2; there are 8)
  expect(verify({ins(0, 4)}, 5, 1) == "" && verify({ins(0, 5)}, 5, 1) == kOperandRange,
         "verifier: constant index at n_constants - 1 and n_constants");
  expect(verify({ins(0, 0)}, 0, 1) == kOperandRange, "verifier: a constant without constants");
  expect(verify({ins(1, 2)}, 1, 3) == "" && verify({ins(1, 3)}, 1, 3) == kOperandRange,
         "verifier: field index at n_inputs - 1 and n_inputs");
  expect(verify({ins(1, 0)}, 1, 0) == kOperandRange, "verifier: a field without inputs");
  expect(verify({ins(2, 7)}, 0, 0) == "" && verify({ins(2, 8)}, 0, 0) == kOperandRange,
         "verifier: built-in index 7 and 8");
  expect(verify({}) == kOneValue, "verifier: no value at the end");
  expect(verify({kConst0, kConst0}) == kOneValue, "verifier: two values at the end");
}

// ---- derive: the plan ----------------------------------------------------------------------
const char* const kShared = "an output box's cells overlap an input box's cells";

struct DeriveCall {
  std::vector<std::vector<avr_box>> inputs;
  std::vector<avr_box> out;
  std::vector<uint32_t> code = {kConst0};
  std::vector<double> constants = {2.5};
  std::vector<double> origin;     // 3 per box; zeros by default
  std::vector<double> cell_size = {1.0, 2.0, 3.0};
  int n_levels = 1;
  int n_inputs = -1;              // by default inputs.size()
  avr::DerivePlan plan;

  std::string run() {
    std::vector<const avr_box*> lists;
    for (const auto& list : inputs) lists.push_back(list.data());
    std::vector<double> o = origin;
    o.resize(out.size() * 3, 0.0);
    return refusal([&] {
      plan = avr::plan_derive(lists.data(), n_inputs < 0 ? static_cast<int>(lists.size()) : n_inputs,
                              out.data(), out.size(), code.data(), static_cast<int>(code.size()),
                              constants.empty() ? nullptr : constants.data(),
                              static_cast<int>(constants.size()), out.empty() ? nullptr : o.data(),
                              cell_size.data(), n_levels);
    });
  }
};

void derive_plan() {
  {
    DeriveCall call;  // 64 instructions: a constant, 31 x (constant, add), one neg
    for (int i = 0; i < 31; ++i) {
      call.code.push_back(kConst0);
      call.code.push_back(ins(3));
    }
    call.code.push_back(ins(7));
    expect(call.code.size() == 64 && call.run() == "", "derive: 64 instructions pass");
    expect(call.plan.tile_begin == std::vector<uint32_t>({0u}) && call.plan.boxes.empty(),
           "derive: a scene without boxes has the empty prefix");
    bool same = true;
    for (size_t i = 0; i < 64; ++i) same = same && call.plan.program.code[i] == call.code[i];
    expect(same && call.plan.program.constants[0] == 2.5 && call.plan.program.constants[1] == 0.0 &&
               call.plan.program.cell_size[0][0] == 1.0 && call.plan.program.cell_size[0][1] == 2.0 &&
               call.plan.program.cell_size[0][2] == 3.0 && call.plan.program.cell_size[1][0] == 0.0,
           "derive: the program holds the code, the constants and the cell sizes, zero beyond");
    call.code.push_back(ins(7));
    expect(call.run() == "n_instructions must lie in [1, 64]", "derive: 65 instructions are refused");
    call.code.clear();
    expect(call.run() == "n_instructions must lie in [1, 64]", "derive: no instruction is refused");
  }
  {
    DeriveCall call;
    call.n_inputs = 7;
    expect(call.run() == "n_inputs must lie in [0, 6]", "derive: seven inputs");
    call.n_inputs = -1;
    call.constants.assign(17, 1.0);
    expect(call.run() == "n_constants must lie in [0, 16]", "derive: seventeen constants");
    call.constants.assign(16, 1.0);
    expect(call.run() == "", "derive: sixteen constants pass");
    call.n_levels = 17;
    expect(call.run() == "n_levels must lie in [1, 16]", "derive: seventeen levels");
    call.n_levels = 0;
    expect(call.run() == "n_levels must lie in [1, 16]", "derive: no level");
    call.n_levels = 1;
    call.code = {kConst0, kConst0};
    expect(call.run() == kOneValue, "derive: the plan runs the verifier");
    call.code = {kConst0};
    call.cell_size[2] = kInf;
    expect(call.run() == "level_cell_size must be finite", "derive: an infinite cell size");
  }
  {
    // one box of 8 x 4 x 4 at level 1 of 2, two inputs with strides of their own
    DeriveCall call;
    call.n_levels = 2;
    call.cell_size = {1, 1, 1, 0.5, 0.5, 0.5};
    avr_box in0 = box(8, 4, 4, 1, address(kBase));
    avr_box in1 = box(8, 4, 4, 1, address(kBase + 0x10000));
    in1.jstride = 10;
    in1.kstride = 44;
    avr_box out = box(8, 4, 4, 1, address(kBase + 0x20008));  // not 16-byte aligned
    call.inputs = {{in0}, {in1}};
    call.out = {out};
    call.origin = {0.25, 0.5, 0.75};
    call.code = {ins(1, 1)};
    expect(call.run() == "", "derive: one box, two inputs");
    const avr::DeriveBoxDev& dev = call.plan.boxes[0];
    expect(dev.cells[0] == in0.cells && dev.cells[1] == in1.cells && dev.cells[2] == nullptr &&
               dev.out == out.cells, "derive: the box's cells");
    expect(dev.jstride[0] == 8 && dev.kstride[0] == 32 && dev.jstride[1] == 10 &&
               dev.kstride[1] == 44 && dev.jstride[6] == 8 && dev.kstride[6] == 32 &&
               dev.jstride[2] == 0, "derive: the strides, the output's in entry 6");
    expect(dev.nx == 8 && dev.ny == 4 && dev.nz == 4 && dev.level == 1 && dev.paired == 0 &&
               dev.origin[0] == 0.25 && dev.origin[1] == 0.5 && dev.origin[2] == 0.75,
           "derive: dims, level, paired and origin");
    expect(call.plan.tile_begin == std::vector<uint32_t>({0u, tiles_of(out)}), "derive: the tile prefix");
    call.origin[1] = kNan;
    expect(call.run() == "box_origin must be finite", "derive: a NaN origin");
  }
  // shared bytes.  A box of n cells along x at address a holds the bytes [a, a + 8 n - 1].
  {
    DeriveCall call;
    call.inputs = {{box(4, 1, 1)}};
    call.out = {box(4, 1, 1)};
    expect(call.run() == kShared, "shared: the output is the input");
    call.out[0].cells = address(kBase + 31);
    expect(call.run() == kShared, "shared: the output begins on the input's last byte");
    call.out[0].cells = address(kBase + 32);
    expect(call.run() == "", "shared: the output begins one byte past the input");
    call.out[0].cells = address(kBase - 31);
    expect(call.run() == kShared, "shared: the output ends on the input's first byte");
    call.out[0].cells = address(kBase - 32);
    expect(call.run() == "", "shared: the output ends one byte before the input");
  }
  {
    // box 0 reads 128 cells at kBase; box 1 reads one cell inside them (it sorts after the long
    // read) and writes one cell further inside: only the long read reaches it
    DeriveCall call;
    call.inputs = {{box(128, 1, 1, 0, address(kBase)), box(1, 1, 1, 0, address(kBase + 512))}};
    call.out = {box(128, 1, 1, 0, address(kBase + 0x10000)), box(1, 1, 1, 0, address(kBase + 800))};
    expect(call.run() == kShared, "shared: a write nested in a long read, behind a shorter read");
    call.out[1].cells = address(kBase + 1024);
    expect(call.run() == "", "shared: the same write past the long read");
  }
  {
    // a box without cells may name any cells, the input's among them
    DeriveCall call;
    call.inputs = {{box(0, 4, 4), box(4, 1, 1)}};
    call.out = {box(0, 4, 4), box(4, 1, 1, 0, address(kBase + 0x1000))};
    expect(call.run() == "", "shared: an empty box contributes no range");
    expect(call.plan.boxes[0].out == nullptr && call.plan.boxes[0].cells[0] == nullptr &&
               call.plan.boxes[0].nx == 0 && call.plan.boxes[0].paired == 1 &&
               call.plan.tile_begin == std::vector<uint32_t>({0u, 0u, 1u}),
           "shared: an empty box stays zeroed and takes no tile");
  }
  {
    // against the definition: some byte lies in a read range and in a write range
    uint32_t state = 12345u;
    auto next = [&](uint32_t n) {
      state = state * 1664525u + 1013904223u;
      return (state >> 8) % n;
    };
    for (int round = 0; round < 2000; ++round) {
      avr::ByteRanges reads, writes;
      for (uint32_t i = next(6); i > 0; --i) {
        const uintptr_t lo = next(64);
        reads.emplace_back(lo, lo + next(24));
      }
      for (uint32_t i = next(3); i > 0; --i) {
        const uintptr_t lo = next(64);
        writes.emplace_back(lo, lo + next(8));
      }
      bool shared = false;
      for (const auto& r : reads) {
        for (const auto& w : writes) {
          for (uintptr_t byte = w.first; byte <= w.second; ++byte) {
            shared = shared || (r.first <= byte && byte <= r.second);
          }
        }
      }
      const std::string got = refusal([&] { avr::require_no_shared_byte(&reads, writes); });
      expect(got == (shared ? kShared : ""), "shared: random ranges, round " + std::to_string(round));
    }
  }
}

// ---- gradient ------------------------------------------------------------------------------
struct AmrBox {
  int level;
  int lo[3];
  int dims[3];
};
struct AmrScene {
  std::vector<AmrBox> boxes;
  std::vector<int32_t> ratio;     // n_levels - 1
  std::vector<double> cell_size;  // n_levels
};

int64_t floor_quotient(int64_t a, int64_t r) {  // the indices are small: the f64 quotient is exact enough
  return static_cast<int64_t>(std::floor(static_cast<double>(a) / static_cast<double>(r)));
}
bool holds(const AmrBox& b, const int64_t cell[3]) {
  for (int d = 0; d < 3; ++d) {
    if (b.dims[d] <= 0 || cell[d] < b.lo[d] || cell[d] >= b.lo[d] + b.dims[d]) return false;
  }
  return true;
}
// The boxes other than b that hold a ghost cell of b's face, the cell's ancestor at a coarser
// level, or one of its children at the next finer level; ascending.
std::vector<int32_t> neighbours(const AmrScene& scene, size_t b, int axis, int side) {
  const AmrBox& self = scene.boxes[b];
  const int n_levels = static_cast<int>(scene.cell_size.size());
  std::vector<bool> hit(scene.boxes.size(), false);
  if (self.dims[0] <= 0 || self.dims[1] <= 0 || self.dims[2] <= 0) return {};
  const int u = (axis + 1) % 3, v = (axis + 2) % 3;
  for (int iu = 0; iu < self.dims[u]; ++iu) {
    for (int iv = 0; iv < self.dims[v]; ++iv) {
      int64_t ghost[3];
      ghost[axis] = side == 0 ? self.lo[axis] - 1 : self.lo[axis] + self.dims[axis];
      ghost[u] = self.lo[u] + iu;
      ghost[v] = self.lo[v] + iv;
      for (size_t c = 0; c < scene.boxes.size(); ++c) {
        const AmrBox& other = scene.boxes[c];
        if (c == b) continue;
        if (other.level <= self.level) {
          int64_t cell[3] = {ghost[0], ghost[1], ghost[2]};
          for (int m = self.level; m > other.level; --m) {
            for (int d = 0; d < 3; ++d) cell[d] = floor_quotient(cell[d], scene.ratio[m - 1]);
          }
          if (holds(other, cell)) hit[c] = true;
        } else if (other.level == self.level + 1 && other.level < n_levels) {
          const int64_t r = scene.ratio[self.level];
          for (int64_t x = 0; x < r; ++x) {
            for (int64_t y = 0; y < r; ++y) {
              for (int64_t z = 0; z < r; ++z) {
                const int64_t child[3] = {ghost[0] * r + x, ghost[1] * r + y, ghost[2] * r + z};
                if (holds(other, child)) hit[c] = true;
              }
            }
          }
        }
      }
    }
  }
  std::vector<int32_t> list;
  for (size_t c = 0; c < hit.size(); ++c) {
    if (hit[c]) list.push_back(static_cast<int32_t>(c));
  }
  return list;
}

struct GradientCall {
  std::vector<avr_box> in, out;
  std::vector<int32_t> lo;
  avr::GradientPlan plan;
  explicit GradientCall(const AmrScene& scene) {
    for (size_t b = 0; b < scene.boxes.size(); ++b) {
      const AmrBox& s = scene.boxes[b];
      const bool cells = s.dims[0] > 0 && s.dims[1] > 0 && s.dims[2] > 0;
      in.push_back(box(s.dims[0], s.dims[1], s.dims[2], s.level,
                       cells ? address(kBase + b * 0x10000) : nullptr));
      out.push_back(box(s.dims[0], s.dims[1], s.dims[2], s.level,
                        cells ? address(kBase + b * 0x10000 + 0x8000) : nullptr));
      lo.insert(lo.end(), s.lo, s.lo + 3);
    }
  }
  std::string run(const AmrScene& scene, int axis) {
    return refusal([&] {
      plan = avr::plan_gradient(in.data(), out.data(), in.size(), axis, lo.data(),
                                scene.ratio.empty() ? nullptr : scene.ratio.data(),
                                scene.cell_size.data(), static_cast<int>(scene.cell_size.size()));
    });
  }
};

void gradient_scene(const AmrScene& scene, const std::string& name) {
  for (int axis = 0; axis < 3; ++axis) {
    const std::string where = name + ", axis " + std::to_string(axis);
    GradientCall call(scene);
    expect(call.run(scene, axis) == "", "gradient: accepted, " + where);
    const avr::GradientPlan& plan = call.plan;
    std::vector<uint32_t> tile_begin(1, 0u), face_begin(1, 0u), candidate_begin(1, 0u);
    std::vector<int32_t> candidates;
    bool boxes_ok = plan.boxes.size() == scene.boxes.size();
    for (size_t b = 0; boxes_ok && b < scene.boxes.size(); ++b) {
      const AmrBox& s = scene.boxes[b];
      const bool cells = s.dims[0] > 0 && s.dims[1] > 0 && s.dims[2] > 0;
      const avr::GradientBoxDev& dev = plan.boxes[b];
      boxes_ok = dev.face_begin == face_begin.back() && dev.level == s.level &&
                 dev.dx == scene.cell_size[static_cast<size_t>(s.level)] &&
                 dev.in == call.in[b].cells && dev.out == call.out[b].cells;
      if (cells) {
        boxes_ok = boxes_ok && dev.nx == s.dims[0] && dev.ny == s.dims[1] && dev.nz == s.dims[2] &&
                   dev.lo[0] == s.lo[0] && dev.lo[1] == s.lo[1] && dev.lo[2] == s.lo[2] &&
                   dev.jstride_in == s.dims[0] && dev.kstride_out == s.dims[0] * s.dims[1];
      } else {
        boxes_ok = boxes_ok && dev.nx == 0 && dev.ny == 0 && dev.nz == 0;
      }
      tile_begin.push_back(tile_begin.back() + tiles_of(call.in[b]));
      face_begin.push_back(face_begin.back() +
                           (cells ? static_cast<uint32_t>(s.dims[(axis + 1) % 3] * s.dims[(axis + 2) % 3])
                                  : 0u));
      for (int side = 0; side < 2; ++side) {
        const std::vector<int32_t> list = neighbours(scene, b, axis, side);
        expect(cells || list.empty(), "gradient: a box without cells has no neighbour, " + where);
        candidates.insert(candidates.end(), list.begin(), list.end());
        candidate_begin.push_back(static_cast<uint32_t>(candidates.size()));
      }
    }
    expect(boxes_ok, "gradient: the box table, " + where);
    expect(plan.tile_begin == tile_begin, "gradient: tile_begin, " + where);
    expect(plan.face_begin == face_begin, "gradient: face_begin, " + where);
    expect(plan.candidate_begin == candidate_begin, "gradient: candidate_begin, " + where);
    expect(plan.candidates == candidates, "gradient: candidates, " + where);
    expect(!candidates.empty(), "gradient: the scene has neighbours at all, " + where);
    bool ratios = true;
    for (size_t l = 0; l < 16; ++l) {
      ratios = ratios && plan.levels.ratio[l] == (l < scene.ratio.size() ? scene.ratio[l] : 1);
    }
    expect(ratios, "gradient: the ratios, 1 from the finest level on, " + where);
  }
}

void gradient() {
  const char* const kRange = "a box's index range leaves [-2^30, 2^30)";
  // two levels, ratio 2: two coarse boxes side by side, a fine box that straddles their common
  // face with a fine neighbour, a box without cells, a coarse box across a gap, and two fine boxes
  // that hold only the last children (y = 7 of 6..7, x = 9 of 8..9) of box 0's high ghost cells
  AmrScene two;
  two.ratio = {2};
  two.cell_size = {1.0, 0.5};
  two.boxes = {{0, {0, 0, 0}, {4, 4, 4}},   {0, {4, 0, 0}, {4, 4, 4}},  {1, {4, 2, 2}, {8, 4, 4}},
               {1, {12, 2, 2}, {4, 4, 4}},  {0, {8, 0, 0}, {0, 4, 4}},  {0, {0, 4, 0}, {8, 2, 4}},
               {0, {0, 0, 6}, {4, 4, 2}},   {1, {8, 7, 0}, {2, 3, 2}},  {1, {9, 0, 0}, {1, 2, 2}}};
  gradient_scene(two, "two levels");
  // three levels, ratios 2 and 4, around the origin: the boxes' first cells are negative and no
  // multiples of the ratios.  Box 2's low ghost cells along y (-7) have the parent -2 = floor(-7 / 4)
  // in box 7, whose neighbour box 1 begins at -1; box 1's along z (-3) have the parent
  // -2 = floor(-3 / 2) in box 6, whose neighbour box 0 begins at -1.
  AmrScene three;
  three.ratio = {2, 4};
  three.cell_size = {1.0, 0.5, 0.125};
  three.boxes = {{0, {-4, -4, -1}, {8, 8, 5}},   {1, {-3, -1, -2}, {5, 3, 5}},
                 {2, {-7, -6, -5}, {6, 7, 9}},   {2, {-1, -6, -5}, {4, 4, 4}},
                 {1, {2, -3, -3}, {3, 5, 5}},    {2, {-7, 1, -5}, {6, 3, 9}},
                 {0, {-4, -4, -7}, {8, 8, 6}},   {1, {-3, -5, -3}, {5, 4, 5}},
                 {2, {-7, -6, -9}, {5, 7, 4}},   {0, {-7, -4, -4}, {3, 8, 8}}};
  gradient_scene(three, "three levels");
  {
    AmrScene alone;
    alone.cell_size = {1.0};
    alone.boxes = {{0, {0, 0, 0}, {4, 4, 4}}, {0, {9, 9, 9}, {0, 0, 0}}};
    GradientCall lone(alone);
    expect(lone.run(alone, 0) == "" && lone.plan.candidates.empty() &&
               lone.plan.candidate_begin == std::vector<uint32_t>(5, 0u),
           "gradient: no neighbour anywhere leaves the list empty and every range empty");
  }
  {
    AmrScene scene = two;
    scene.boxes[1].lo[0] = 3;  // meets box 0 in the cells x = 3
    GradientCall call(scene);
    expect(call.run(scene, 0) == "two boxes of one level overlap in index space",
           "gradient: two boxes of a level overlap");
    scene.boxes[1].level = 1;  // another level: no longer compared
    scene.boxes[2].lo[0] = 14;
    scene.boxes[3].lo[0] = 30;
    GradientCall other(scene);
    expect(other.run(scene, 0) == "", "gradient: boxes of different levels may overlap in index");
  }
  {
    AmrScene scene;
    scene.cell_size = {1.0};
    scene.boxes = {{0, {-(1 << 30), 0, 0}, {4, 4, 4}}};
    GradientCall low(scene);
    expect(low.run(scene, 1) == "", "gradient: a first index of -2^30 passes");
    low.lo[0] -= 1;
    expect(low.run(scene, 1) == kRange, "gradient: a first index of -2^30 - 1");
    scene.boxes = {{0, {0, 0, (1 << 30) - 4}, {4, 4, 4}}};
    GradientCall high(scene);
    expect(high.run(scene, 1) == "", "gradient: a last index of 2^30 - 1 passes");
    high.lo[2] += 1;
    expect(high.run(scene, 1) == kRange, "gradient: a last index of 2^30");
  }
  {
    AmrScene scene = two;
    GradientCall call(scene);
    scene.ratio = {1};
    expect(call.run(scene, 0) == "a level ratio is below 2", "gradient: a ratio of 1");
    scene.ratio = {2};
    for (double bad : {0.0, kInf, -1.0, kNan}) {
      scene.cell_size = {1.0, bad};
      expect(call.run(scene, 0) == "level_cell_size must be finite and positive",
             "gradient: a cell size of " + std::to_string(bad));
    }
    scene.cell_size = {1.0, 0.5};
    expect(call.run(scene, 3) == "axis must be 0 (x), 1 (y) or 2 (z)" &&
               call.run(scene, -1) == "axis must be 0 (x), 1 (y) or 2 (z)", "gradient: the axis");
    scene.cell_size.assign(17, 1.0);
    expect(call.run(scene, 0) == "n_levels must lie in [1, 16]", "gradient: seventeen levels");
    scene.cell_size = {1.0};  // the fine boxes' level is not below n_levels
    expect(call.run(scene, 0) == "a box's level is not below n_levels", "gradient: the box rules apply");
    scene.cell_size = {1.0, 0.5};
    call.out[2].cells = call.in[1].cells;
    expect(call.run(scene, 0) == kShared, "gradient: an output box on another box's input");
  }
}

// ---- on-axis projection --------------------------------------------------------------------
struct AxisCall {
  std::vector<avr_box> f, w;  // w empty: no weight
  double origin_uv[2] = {0.0, 0.0};
  double du = 1.0, dv = 1.0;
  int width = 4, height = 4;
  std::vector<double> level_dl = {1.0};
  avr::AxisProjectionPlan plan;
  std::string run(int axis) {
    return refusal([&] {
      plan = avr::plan_axis_projection(f.data(), w.empty() ? nullptr : w.data(), f.size(), axis,
                                       origin_uv, du, dv, width, height, level_dl.data(),
                                       static_cast<int>(level_dl.size()));
    });
  }
};

void axis_projection() {
  const char* const kTooMany = "scene has too many cells";
  const int image_u[3] = {1, 2, 0}, image_v[3] = {2, 0, 1};  // x: (y, z); y: (z, x); z: (x, y)
  for (int axis = 0; axis < 3; ++axis) {
    const std::string where = ", axis " + std::to_string(axis);
    // columns of 1, 128 and 129 cells, a box without cells between them
    AxisCall call;
    call.level_dl = {0.5, 0.25};
    const int lengths[4] = {1, 128, 0, 129};
    const uint32_t segments[4] = {1, 1, 0, 2};
    for (int b = 0; b < 4; ++b) {
      int dims[3];
      dims[axis] = lengths[b];
      dims[image_u[axis]] = 3 + b;
      dims[image_v[axis]] = 5 + b;
      avr_box one = box(dims[0], dims[1], dims[2], b % 2, lengths[b] > 0 ? address(kBase) : nullptr);
      for (int a = 0; a < 3; ++a) {
        one.min_corner[a] = 1.0 + a + 10.0 * b;
        one.max_corner[a] = 4.5 + 2.0 * a + 10.0 * b;
      }
      call.f.push_back(one);
    }
    call.w = call.f;
    for (avr_box& weight : call.w) {
      if (weight.cells != nullptr) weight.cells = address(kBase + 0x100000);
    }
    call.w[0].jstride += 2;
    expect(call.run(axis) == "", "axis: accepted" + where);
    uint32_t entries = 0;
    std::vector<uint32_t> tile_begin(1, 0u);
    for (size_t b = 0; b < 4 && call.plan.boxes.size() == 4 && call.plan.planes.size() == 4; ++b) {
      const avr_box& in = call.f[b];
      const avr::AxisBoxDev& dev = call.plan.boxes[b];
      const avr::AxisPlaneDev& plane = call.plan.planes[b];
      const std::string which = where + ", box " + std::to_string(b);
      expect(dev.plane_begin == entries && plane.plane_begin == entries,
             "axis: plane_begin is the running entry count in both tables" + which);
      if (lengths[b] > 0) {
        expect(plane.segments == static_cast<int32_t>(segments[b]), "axis: the segments" + which);
        expect(plane.n_u == in.dims[image_u[axis]] && plane.n_v == in.dims[image_v[axis]] &&
                   plane.min_u == in.min_corner[image_u[axis]] && plane.max_u == in.max_corner[image_u[axis]] &&
                   plane.min_v == in.min_corner[image_v[axis]] && plane.max_v == in.max_corner[image_v[axis]],
               "axis: u and v pick the dims and the corners" + which);
        expect(plane.dl == call.level_dl[b % 2], "axis: the level's path length" + which);
        expect(dev.nx == in.dims[0] && dev.ny == in.dims[1] && dev.nz == in.dims[2] &&
                   dev.cells_f == in.cells && dev.cells_w == call.w[b].cells &&
                   dev.jstride_f == in.jstride && dev.jstride_w == call.w[b].jstride &&
                   dev.kstride_f == in.kstride && dev.kstride_w == call.w[b].kstride,
               "axis: the fields' cells and strides" + which);
        entries += static_cast<uint32_t>(in.dims[image_u[axis]] * in.dims[image_v[axis]]) * segments[b];
        tile_begin.push_back(tile_begin.back() + 1);
      } else {
        expect(dev.nx == 0 && dev.cells_f == nullptr && plane.n_u == 0 && plane.segments == 0 &&
                   plane.min_u == 0.0 && plane.max_u == 0.0, "axis: a box without cells stays zeroed" + which);
        tile_begin.push_back(tile_begin.back());
      }
    }
    expect(call.plan.entries == entries, "axis: the entry total" + where);
    expect(call.plan.tile_begin == tile_begin, "axis: the tile prefix" + where);
    // without a weight the weight's entries repeat the field's
    call.w.clear();
    expect(call.run(axis) == "" && call.plan.boxes[0].cells_w == call.f[0].cells &&
               call.plan.boxes[0].jstride_w == call.plan.boxes[0].jstride_f,
           "axis: no weight repeats the field" + where);
    // corners: only the image axes of a box with cells
    for (int which = 0; which < 2; ++which) {
      for (double bad : {kNan, kInf}) {
        AxisCall broken = call;
        const int a = which == 0 ? image_u[axis] : image_v[axis];
        broken.f[1].min_corner[a] = bad;
        expect(broken.run(axis) == "box corners must be finite", "axis: a non-finite min corner" + where);
        broken = call;
        broken.f[1].max_corner[a] = bad;
        expect(broken.run(axis) == "box corners must be finite", "axis: a non-finite max corner" + where);
        broken = call;
        broken.f[2].min_corner[a] = broken.f[2].max_corner[a] = bad;  // the box without cells
        expect(broken.run(axis) == "", "axis: non-finite corners of a box without cells" + where);
      }
    }
  }
  {
    // 2^31 entries, from dims alone: strides 0 keep every box's span small, one address for all
    auto flat = [](int nx, int ny) {
      avr_box b = box(nx, ny, 1);
      b.jstride = b.kstride = 0;
      return b;
    };
    AxisCall call;
    call.f = {flat(65536, 32767), flat(65535, 1)};
    expect(call.run(2) == "" && call.plan.entries == 0x7fffffffu &&
               call.plan.boxes[1].plane_begin == 0x7fffffffu - 65535u,
           "axis: 2^31 - 1 entries pass");
    call.f[1] = flat(65536, 1);
    expect(call.run(2) == kTooMany, "axis: 2^31 entries are refused");
    call.f = {flat(65536, 32768)};
    expect(call.run(2) == kTooMany, "axis: one box of 2^31 entries is refused");
  }
  {
    AxisCall call;
    call.f = {box(4, 4, 4)};
    expect(call.run(3) == "axis must be 0 (x), 1 (y) or 2 (z)", "axis: axis 3");
    call.width = 0;
    expect(call.run(0) == "image width and height must be positive", "axis: no width");
    call.width = 65536;
    call.height = 32768;
    expect(call.run(0) == "image has more than 2^31-1 pixels", "axis: 2^31 pixels");
    call.width = call.height = 4;
    call.du = kNan;
    expect(call.run(0) == "the window must be finite", "axis: a NaN window");
    call.du = 1.0;
    call.origin_uv[1] = kInf;
    expect(call.run(0) == "the window must be finite", "axis: an infinite origin");
    call.origin_uv[1] = 0.0;
    call.level_dl = {1.0, kNan};
    expect(call.run(0) == "level_dl must be finite", "axis: a NaN path length");
    call.level_dl.assign(17, 1.0);
    expect(call.run(0) == "n_levels must lie in [1, 16]", "axis: seventeen levels");
    call.level_dl = {1.0};
    call.f[0].level = 1;
    expect(call.run(0) == "a box's level is not below n_levels", "axis: the box rules apply");
  }
}

// ---- joint histogram -----------------------------------------------------------------------
struct JointCall {
  std::vector<avr_box> x, y, s;  // y, s empty: absent
  std::vector<double> x_edges = {0.0, 1.0}, y_edges;
  int nx = -1, ny = -1;          // by default the edges' count - 1 (ny: 1 without y edges)
  bool null_x_edges = false, null_y_edges = false;
  int n_levels = 1;
  avr::JointHistogramPlan plan;
  std::string run() {
    return refusal([&] {
      plan = avr::plan_joint_histogram(
          x.data(), y.empty() ? nullptr : y.data(), s.empty() ? nullptr : s.data(), x.size(),
          null_x_edges ? nullptr : x_edges.data(), nx >= 0 ? nx : static_cast<int>(x_edges.size()) - 1,
          null_y_edges || y_edges.empty() ? nullptr : y_edges.data(),
          ny >= 0 ? ny : (y_edges.empty() ? 1 : static_cast<int>(y_edges.size()) - 1), n_levels);
    });
  }
};

std::vector<double> ramp(int n, double lo = 0.0, double step = 1.0) {
  std::vector<double> e;
  for (int i = 0; i <= n; ++i) e.push_back(lo + step * i);
  return e;
}

void joint_histogram() {
  {
    JointCall call;
    call.x = {box(130, 5, 3, 1, address(kBase)), box(4, 0, 4, 0, nullptr)};
    call.y = {box(130, 5, 3, 1, address(kBase + 0x100000)), box(4, 0, 4, 0, nullptr)};
    call.y[0].jstride = 132;
    call.n_levels = 2;
    call.x_edges = {-2.0, 0.0, 0.5, 6.0};
    call.y_edges = {1.0, 10.0, 100.0, 1000.0, 10000.0};
    expect(call.run() == "", "joint: x and y");
    const avr::JointHistogramArgs& args = call.plan.args;
    expect(args.x_scale == 3.0 / 8.0 && args.y_scale == 4.0 / 9999.0, "joint: scale = n / (e[n] - e[0])");
    expect(args.nx == 3 && args.ny == 4 && args.x_lo == -2.0 && args.x_hi == 6.0 && args.y_lo == 1.0 &&
               args.y_hi == 10000.0 && args.n_boxes == 2 && args.n_tiles == 2 * 2 * 1,
           "joint: the counts and bounds");
    expect(args.boxes == nullptr && args.tile_begin == nullptr && args.x_edges == nullptr &&
               args.y_edges == nullptr && args.cells == nullptr && args.sums == nullptr &&
               args.totals == nullptr, "joint: the device pointers are left null");
    expect(call.plan.tile_begin == std::vector<uint32_t>({0u, 4u, 4u}), "joint: the tile prefix");
    const avr::JointBoxDev& dev = call.plan.boxes[0];
    expect(dev.cells[0] == call.x[0].cells && dev.cells[1] == call.y[0].cells &&
               dev.cells[2] == call.x[0].cells && dev.jstride[0] == 130 && dev.jstride[1] == 132 &&
               dev.jstride[2] == 130 && dev.kstride[1] == 650 && dev.nx == 130 && dev.ny == 5 &&
               dev.nz == 3 && dev.level == 1, "joint: an absent field repeats x");
    expect(call.plan.boxes[1].nx == 0 && call.plan.boxes[1].ny == 0 && call.plan.boxes[1].cells[0] == nullptr,
           "joint: a box without cells stays zeroed");
    call.s = call.y;
    call.y.clear();
    call.y_edges.clear();
    expect(call.run() == "" && call.plan.boxes[0].cells[1] == call.x[0].cells &&
               call.plan.boxes[0].cells[2] == call.s[0].cells && call.plan.args.y_scale == 0.0 &&
               call.plan.args.ny == 1, "joint: x and s");
    call.ny = 2;
    expect(call.run() == "without scene_y there is one y bin", "joint: two y bins without y");
    call.ny = 0;
    expect(call.run() == "without scene_y there is one y bin", "joint: no y bin without y");
  }
  {
    JointCall call;
    call.x_edges = {-1e308, 1e308};
    expect(call.run() == "" && call.plan.args.x_scale == 0.0 && call.plan.args.x_lo == -1e308 &&
               call.plan.args.x_hi == 1e308, "joint: a scale that is not finite is 0");
  }
  for (int axis = 0; axis < 2; ++axis) {
    const std::string name = axis == 0 ? "x" : "y";
    JointCall call;
    call.x = {box(4, 4, 4)};
    call.y = {box(4, 4, 4)};
    call.y_edges = {0.0, 1.0};
    std::vector<double>& edges = axis == 0 ? call.x_edges : call.y_edges;
    int& n = axis == 0 ? call.nx : call.ny;
    (axis == 0 ? call.null_x_edges : call.null_y_edges) = true;
    expect(call.run() == name + "_edges is null", "joint: null " + name + " edges");
    (axis == 0 ? call.null_x_edges : call.null_y_edges) = false;
    n = 0;
    expect(call.run() == name + " bin count must lie in [1, 1024]", "joint: no " + name + " bin");
    edges = ramp(1025);
    n = 1025;
    expect(call.run() == name + " bin count must lie in [1, 1024]", "joint: 1025 " + name + " bins");
    n = 1024;
    expect(call.run() == "", "joint: 1024 " + name + " bins pass");
    n = -1;
    for (double bad : {kNan, kInf, -kInf}) {
      edges = {0.0, 1.0, bad, 3.0};
      expect(call.run() == name + "_edges must be finite", "joint: a non-finite " + name + " edge");
    }
    edges = {0.0, 1.0, 1.0, 3.0};
    expect(call.run() == name + "_edges must be strictly increasing", "joint: equal " + name + " edges");
    edges = {0.0, 2.0, 1.0, 3.0};
    expect(call.run() == name + "_edges must be strictly increasing", "joint: falling " + name + " edges");
    edges = {0.0, 1.0};
    call.n_levels = 0;
    expect(call.run() == "n_levels must lie in [1, 16]", "joint: no level");
    call.n_levels = 17;
    expect(call.run() == "n_levels must lie in [1, 16]", "joint: seventeen levels");
  }
  {
    // 1024 x 1024 = 2^20 bins pass.  No count of bins above 2^20 gets as far as the 2^20 rule: an
    // axis of 1025 bins is refused by its own rule first.
    JointCall call;
    call.x = {box(4, 4, 4)};
    call.y = {box(4, 4, 4)};
    call.x_edges = ramp(1024);
    call.y_edges = ramp(1025, -3.0, 0.5);
    call.ny = 1024;
    expect(call.run() == "" && call.plan.args.nx * call.plan.args.ny == 1 << 20, "joint: 2^20 bins pass");
    call.ny = 1025;
    expect(call.run() == "y bin count must lie in [1, 1024]", "joint: 1024 x 1025 bins are refused");
    call.y[0].dims[1] = 5;
    call.ny = 1024;
    expect(call.run() == "the scenes' boxes differ in dims or level", "joint: the box rules apply");
  }
}

// ---- slice ---------------------------------------------------------------------------------
struct SliceCall {
  std::vector<avr_box> boxes;
  std::vector<int32_t> global_index;  // empty: null
  double origin[3] = {0.5, 1.5, 2.5}, du[3] = {1.0, 0.0, 0.25}, dv[3] = {0.0, -1.0, 0.125};
  int width = 4, height = 4;
  avr::SlicePlan plan;
  std::string run() {
    return refusal([&] {
      plan = avr::plan_slice(boxes.data(), boxes.size(),
                             global_index.empty() ? nullptr : global_index.data(), origin, du, dv,
                             width, height);
    });
  }
};

void slice() {
  const char* const kLevelRule = "box level must lie in [0, 127]";
  SliceCall call;
  avr_box full = box(6, 5, 4, 127);
  full.jstride = 8;
  full.kstride = 48;
  for (int a = 0; a < 3; ++a) {
    full.min_corner[a] = -1.0 - a;
    full.max_corner[a] = 2.0 + a;
  }
  avr_box hollow = box(6, 0, 4, 3, nullptr);
  hollow.min_corner[0] = kNan;  // never looked at
  call.boxes = {full, hollow, box(1, 1, 1, 0)};
  expect(call.run() == "", "slice: accepted");
  bool plane = true;
  for (int a = 0; a < 3; ++a) {
    plane = plane && call.plan.plane.origin[a] == call.origin[a] && call.plan.plane.du[a] == call.du[a] &&
            call.plan.plane.dv[a] == call.dv[a];
  }
  expect(plane, "slice: the plane");
  {
    const avr::SliceBoxDev& dev = call.plan.boxes[0];
    expect(dev.global_index == 0 && dev.level == 127 && dev.cells == full.cells && dev.jstride == 8 &&
               dev.kstride == 48 && dev.n[0] == 6 && dev.n[1] == 5 && dev.n[2] == 4 && dev.minc[2] == -3.0 &&
               dev.maxc[1] == 3.0, "slice: a box with cells");
    const avr::SliceBoxDev& none = call.plan.boxes[1];
    expect(none.global_index == 1 && none.level == 3 && none.cells == nullptr && none.n[0] == 0 &&
               none.n[2] == 0 && none.minc[0] == 0.0 && none.maxc[0] == 0.0 && none.jstride == 0,
           "slice: a box without cells stays zeroed but for index and level");
    expect(call.plan.boxes[2].global_index == 2, "slice: the default index is the box's position");
  }
  call.global_index = {40, -7, 2000000000};
  expect(call.run() == "" && call.plan.boxes[0].global_index == 40 &&
             call.plan.boxes[1].global_index == -7 && call.plan.boxes[2].global_index == 2000000000,
         "slice: the given indices");
  call.boxes[0].level = 128;
  expect(call.run() == kLevelRule, "slice: level 128");
  call.boxes[0].level = 0;
  call.boxes[1].level = -1;
  expect(call.run() == kLevelRule, "slice: level -1 of a box without cells");
  call.boxes[1].level = 0;
  expect(call.run() == "", "slice: level 0");
  for (int v = 0; v < 3; ++v) {
    for (int a = 0; a < 3; ++a) {
      for (double bad : {kNan, kInf}) {
        SliceCall broken = call;
        (v == 0 ? broken.origin : v == 1 ? broken.du : broken.dv)[a] = bad;
        expect(broken.run() == "slice plane must be finite", "slice: a non-finite plane");
      }
    }
  }
  call.width = 0x7fffffff;
  call.height = 1;
  expect(call.run() == "", "slice: 2^31 - 1 pixels pass");
  call.width = 65536;
  call.height = 32768;
  expect(call.run() == "image has more than 2^31-1 pixels", "slice: 2^31 pixels");
  call.height = 0;
  expect(call.run() == "image width and height must be positive", "slice: no height");
  call.height = 4;
  call.width = -1;
  expect(call.run() == "image width and height must be positive", "slice: a negative width");
  call.width = 4;
  call.boxes[0].cells = nullptr;
  expect(call.run() == "box has no cell data", "slice: the box rules apply");
}

}  // namespace

int main() {
  derive_verifier();
  derive_plan();
  gradient();
  axis_projection();
  joint_histogram();
  slice();
  if (failures == 0) std::puts("ok");
  return failures == 0 ? 0 : 1;
}
