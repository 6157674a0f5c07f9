// The host plan of the structure functions (csrc/avr_field_plans.h: plan_structure_functions) as a
// plain C++ program, built with AddressSanitizer and UBSan and without HIP: every refusal message
// and which one wins when several rules are broken, the limits of 4096 lags and order 8, a lag of
// N_d - 1 admitted and one of N_d refused, dims of (2^31 - 1, 1, 1) admitted and 2^31 cells
// refused from the descriptors alone (with made-up addresses: nothing is allocated or read), the
// shared-byte rule to the byte for each output against each component and among the outputs, and
// the staged table and the launch shape written out by hand.  Prints "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

const double* address(uint64_t at) {
  return reinterpret_cast<const double*>(static_cast<uintptr_t>(at));
}

const char kNull[] = "null argument";
const char kComponents[] = "n_components must be 1 or 3";
const char kDirectionsGiven[] = "directions are given exactly when there are three components";
const char kDims[] = "dims must be at least 1";
const char kCells[] = "the grid has 2^31 cells or more";
const char kLags[] = "n_lags must lie in [1, 4096]";
const char kOrder[] = "max_order must lie in [1, 8]";
const char kPeriodic[] = "periodic must be 0 or 1";
const char kZero[] = "a lag is zero";
const char kLong[] = "a lag spans a grid length or more along an axis";
const char kFinite[] = "directions must be finite";
const char kOverlap[] = "an output array overlaps a component grid";
const char kOutputs[] = "two output arrays overlap";
const uint64_t kBase = uint64_t{1} << 40;
const uint64_t kApart = uint64_t{1} << 36;  // more than 2^31 cells of 8 bytes

// A call with everything in order -- three components of 6 x 5 x 7 cells, four lags, order 6 --
// to be spoilt one argument at a time.
struct Call {
  const double* grids[3] = {address(kBase), address(kBase + kApart), address(kBase + 2 * kApart)};
  int n_components = 3;
  int32_t dims[3] = {6, 5, 7};
  std::vector<int32_t> lags = {1, 0, 0, 0, -4, 0, 5, 4, -6, -2, 3, 1};
  std::vector<double> directions = {1.0, 0.0, 0.0, 0.0, -1.0, 0.0,
                                    0.5, 0.25, -0.75, -0.5, 0.75, 0.25};
  int n_lags = 4, max_order = 6, periodic = 0;
  const double* pairs = address(kBase + 3 * kApart);
  const double* sums = address(kBase + 4 * kApart);
  const double* totals = address(kBase + 5 * kApart);
  bool no_grids = false, no_dims = false, no_lags = false, no_directions = false;
  avr::StructureFunctionsPlan plan() const {
    return avr::plan_structure_functions(
        no_grids ? nullptr : grids, n_components, no_dims ? nullptr : dims,
        no_lags ? nullptr : lags.data(), no_directions ? nullptr : directions.data(), n_lags,
        max_order, periodic, pairs, sums, totals);
  }
};
template <class Change>
Call spoilt(Change&& change) {
  Call call;
  change(call);
  return call;
}
// ... and its counterpart of one component
Call scalar_call() {
  return spoilt([](Call& c) {
    c.n_components = 1;
    c.no_directions = true;
    c.grids[1] = c.grids[2] = nullptr;
  });
}

void test_the_plan_by_hand() {
  {
    const avr::StructureFunctionsPlan plan = Call().plan();
    const avr::StructureArgs& a = plan.args;
    expect(a.components[0] == nullptr && a.components[1] == nullptr &&
               a.components[2] == nullptr && a.lags == nullptr && a.pairs == nullptr &&
               a.sums == nullptr && a.totals == nullptr, "the plan leaves every address null");
    expect(a.dims[0] == 6 && a.dims[1] == 5 && a.dims[2] == 7 && a.n_cells == 210u, "the dims");
    expect(a.n_lags == 4 && a.max_order == 6 && a.periodic == 0, "the counts");
    expect(a.shares == 1u && plan.groups[0] == 4u && plan.groups[1] == 1u &&
               plan.groups[2] == 1u, "four lags, one share");
    // 256 = 4 + 6 (2 + 5 * 8)
    expect(a.stride[0] == 4u && a.stride[1] == 2u && a.stride[2] == 8u, "the stride of a lane");
    expect(plan.lags.size() == 4, "one row per lag");
    const int32_t l[4][3] = {{1, 0, 0}, {0, -4, 0}, {5, 4, -6}, {-2, 3, 1}};
    const double u[4][3] = {{1.0, 0.0, 0.0}, {0.0, -1.0, 0.0}, {0.5, 0.25, -0.75},
                            {-0.5, 0.75, 0.25}};
    for (int m = 0; m < 4; ++m) {
      for (int d = 0; d < 3; ++d) {
        expect(plan.lags[m].l[d] == l[m][d] && plan.lags[m].u[d] == u[m][d], "the staged table");
      }
      expect(plan.lags[m].pad_ == 0, "the padding is zero");
    }
    expect(sizeof(avr::StructureLagDev) == 40, "a row is three ints, a pad and three doubles");
    int visits = 0;
    avr::StructureArgs copy = plan.args;
    plan.visit_tables(&copy, [&](const avr::StructureLagDev** to,
                                 const avr::StructureLagDev* host, size_t count) {
      expect(to == &copy.lags && host == plan.lags.data() && count == 4, "the one table");
      ++visits;
    });
    expect(visits == 1, "one table is staged");
  }
  {
    const avr::StructureFunctionsPlan plan = spoilt([](Call& c) { c.periodic = 1; }).plan();
    expect(plan.args.periodic == 1, "periodic");
  }
  {
    const avr::StructureFunctionsPlan plan = scalar_call().plan();
    for (int m = 0; m < 4; ++m) {
      for (int d = 0; d < 3; ++d) expect(plan.lags[m].u[d] == 0.0, "no directions: zeros");
    }
  }
  // the launch shape: shares of 16384 cells, rows of 32768 shares
  expect(avr::kStructureGroupCells == 16384u && avr::kStructureLaneStride == 256u &&
             avr::kStructureShareRows == 32768u, "the named constants");
  struct Shape {
    int32_t dims[3];
    uint32_t cells, shares, rows, row_shares, stride[3];
  };
  const Shape shapes[] = {
      {{131, 5, 3}, 1965u, 1u, 1u, 1u, {125u, 1u, 0u}},
      {{256, 2, 2}, 1024u, 1u, 1u, 1u, {0u, 1u, 0u}},
      {{1000, 1, 1}, 1000u, 1u, 1u, 1u, {256u, 0u, 0u}},
      {{1, 1, 5}, 5u, 1u, 1u, 1u, {0u, 0u, 256u}},
      {{128, 128, 1}, 16384u, 1u, 1u, 1u, {0u, 2u, 0u}},
      {{128, 128, 2}, 32768u, 2u, 1u, 2u, {0u, 2u, 0u}},
      {{29, 33, 40}, 38280u, 3u, 1u, 3u, {24u, 8u, 0u}},
      {{1024, 1024, 512}, 1u << 29, 32768u, 1u, 32768u, {256u, 0u, 0u}},
      {{1024, 1024, 513}, 537919488u, 32832u, 2u, 32768u, {256u, 0u, 0u}},
      {{2147483647, 1, 1}, 2147483647u, 131072u, 4u, 32768u, {256u, 0u, 0u}}};
  for (const Shape& s : shapes) {
    const avr::StructureFunctionsPlan plan = spoilt([&](Call& c) {
      std::memcpy(c.dims, s.dims, sizeof(s.dims));
      const int axis = s.dims[0] > 1 ? 0 : 2;  // one lag, the longest the shape admits
      c.lags = {0, 0, 0};
      c.lags[axis] = -(s.dims[axis] - 1);
      c.n_lags = 1;
    }).plan();
    const avr::StructureArgs& a = plan.args;
    expect(a.n_cells == s.cells && a.shares == s.shares, "the shares");
    expect(plan.groups[0] == 1u && plan.groups[1] == s.row_shares && plan.groups[2] == s.rows,
           "the grid of workgroups");
    expect(static_cast<uint64_t>(a.shares) * avr::kStructureGroupCells >= s.cells &&
               static_cast<uint64_t>(a.shares - 1) * avr::kStructureGroupCells < s.cells,
           "every share has a cell, every cell a share");
    expect(static_cast<uint64_t>(plan.groups[1]) * plan.groups[2] >= a.shares &&
               plan.groups[1] <= 65535u && plan.groups[2] <= 65535u, "every share a workgroup");
    expect(a.stride[0] == s.stride[0] && a.stride[1] == s.stride[1] &&
               a.stride[2] == s.stride[2], "the stride by hand");
    expect(a.stride[0] < static_cast<uint32_t>(s.dims[0]) &&
               a.stride[1] < static_cast<uint32_t>(s.dims[1]) &&
               a.stride[0] + static_cast<uint64_t>(s.dims[0]) *
                       (a.stride[1] + static_cast<uint64_t>(s.dims[1]) * a.stride[2]) == 256u,
           "the stride adds up to 256 cells");
  }
}

void test_refusals() {
  const double inf = INFINITY, nan = NAN;
  // 1: null arguments
  expect_message(kNull, [] { spoilt([](Call& c) { c.no_grids = true; }).plan(); });
  expect_message(kNull, [] { spoilt([](Call& c) { c.grids[0] = nullptr; }).plan(); });
  expect_message(kNull, [] { spoilt([](Call& c) { c.no_dims = true; }).plan(); });
  expect_message(kNull, [] { spoilt([](Call& c) { c.no_lags = true; }).plan(); });
  expect_message(kNull, [] { spoilt([](Call& c) { c.pairs = nullptr; }).plan(); });
  expect_message(kNull, [] { spoilt([](Call& c) { c.sums = nullptr; }).plan(); });
  expect_message(kNull, [] { spoilt([](Call& c) { c.totals = nullptr; }).plan(); });
  // 2: the components and the directions
  for (int bad : {0, 2, 4, -1}) {
    expect_message(kComponents, [&] { spoilt([&](Call& c) { c.n_components = bad; }).plan(); });
  }
  expect_message(kDirectionsGiven, [] { spoilt([](Call& c) { c.no_directions = true; }).plan(); });
  expect_message(kDirectionsGiven, [] { spoilt([](Call& c) { c.n_components = 1; }).plan(); });
  expect_message(kNull, [] { spoilt([](Call& c) { c.grids[1] = nullptr; }).plan(); });
  expect_message(kNull, [] { spoilt([](Call& c) { c.grids[2] = nullptr; }).plan(); });
  scalar_call().plan();
  // 3: the dims and the cells
  for (int d = 0; d < 3; ++d) {
    for (int32_t bad : {0, -1, INT32_MIN}) {
      expect_message(kDims, [&] { spoilt([&](Call& c) { c.dims[d] = bad; }).plan(); });
    }
  }
  const int32_t most = INT32_MAX;  // 2^31 - 1
  for (int d = 0; d < 3; ++d) {    // admitted along any axis, with a lag of N_d - 1 there
    spoilt([&](Call& c) {
      c.dims[0] = c.dims[1] = c.dims[2] = 1;
      c.dims[d] = most;
      c.lags = {0, 0, 0, 0, 0, 0};
      c.lags[d] = most - 1;
      c.lags[3 + d] = -(most - 1);
      c.n_lags = 2;
    }).plan();
  }
  const int32_t too_many[][3] = {{1 << 30, 2, 1}, {1 << 16, 1 << 15, 1}, {1 << 11, 1 << 10, 1 << 10},
                                 {most, 2, 1}, {most, most, most}, {1, most, 2}, {2, 1, most}};
  for (const auto& dims : too_many) {
    expect_message(kCells, [&] {
      spoilt([&](Call& c) { std::memcpy(c.dims, dims, sizeof(dims)); }).plan();
    });
  }
  spoilt([](Call& c) { c.dims[0] = 1 << 10; c.dims[1] = 1 << 10; c.dims[2] = (1 << 11) - 1; })
      .plan();
  // 4, 5, 6: the counts
  for (int bad : {0, -1, 4097, 1 << 20}) {
    expect_message(kLags, [&] { spoilt([&](Call& c) { c.n_lags = bad; }).plan(); });
  }
  for (int bad : {0, -1, 9, 100}) {
    expect_message(kOrder, [&] { spoilt([&](Call& c) { c.max_order = bad; }).plan(); });
  }
  for (int good : {1, 8}) spoilt([&](Call& c) { c.max_order = good; }).plan();
  for (int bad : {-1, 2, 256}) {
    expect_message(kPeriodic, [&] { spoilt([&](Call& c) { c.periodic = bad; }).plan(); });
  }
  {
    const avr::StructureFunctionsPlan plan = spoilt([](Call& c) {
      c.n_lags = 4096;
      c.lags.assign(3 * 4096, 1);
      c.directions.assign(3 * 4096, 0.5);
      c.max_order = 8;
    }).plan();
    expect(plan.lags.size() == 4096 && plan.groups[0] == 4096u, "4096 lags are admitted");
  }
  // 7, 8: the lags
  for (int m = 0; m < 4; ++m) {
    expect_message(kZero, [&] {
      spoilt([&](Call& c) { c.lags[3 * m] = c.lags[3 * m + 1] = c.lags[3 * m + 2] = 0; }).plan();
    });
  }
  for (int periodic = 0; periodic <= 1; ++periodic) {
    for (int d = 0; d < 3; ++d) {
      const Call base;
      for (int sign : {1, -1}) {
        spoilt([&](Call& c) {
          c.periodic = periodic;
          c.lags[9 + d] = sign * (base.dims[d] - 1);
        }).plan();
        for (int32_t bad : {base.dims[d], base.dims[d] + 1, INT32_MAX}) {
          expect_message(kLong, [&] {
            spoilt([&](Call& c) {
              c.periodic = periodic;
              c.lags[9 + d] = sign * bad;
            }).plan();
          });
        }
      }
      expect_message(kLong, [&] {
        spoilt([&](Call& c) {
          c.periodic = periodic;
          c.lags[9 + d] = INT32_MIN;
        }).plan();
      });
    }
  }
  // 9: the directions
  for (int e = 0; e < 12; ++e) {
    for (double bad : {inf, -inf, nan}) {
      expect_message(kFinite, [&] { spoilt([&](Call& c) { c.directions[e] = bad; }).plan(); });
    }
  }
  spoilt([](Call& c) { c.directions.assign(12, 0.0); }).plan();  // only finite is asked for
  spoilt([](Call& c) { c.directions.assign(12, -1e300); }).plan();
}

void test_which_message_wins() {
  // every rule broken at once, then mended from the front
  Call call;
  call.n_components = 2;
  call.dims[1] = 0;
  call.n_lags = 0;
  call.max_order = 9;
  call.periodic = 2;
  call.lags[3] = call.lags[4] = call.lags[5] = 0;
  call.lags[0] = 6;
  call.directions[7] = NAN;
  call.sums = call.grids[0];
  call.totals = call.pairs;
  call.pairs = nullptr;
  expect_message(kNull, [&] { call.plan(); });
  call.pairs = call.totals;
  expect_message(kComponents, [&] { call.plan(); });
  call.n_components = 3;
  call.no_directions = true;
  expect_message(kDirectionsGiven, [&] { call.plan(); });
  call.no_directions = false;
  expect_message(kDims, [&] { call.plan(); });
  call.dims[1] = 1 << 30;
  expect_message(kCells, [&] { call.plan(); });
  call.dims[1] = 5;
  expect_message(kLags, [&] { call.plan(); });
  call.n_lags = 4;
  expect_message(kOrder, [&] { call.plan(); });
  call.max_order = 8;
  expect_message(kPeriodic, [&] { call.plan(); });
  call.periodic = 1;
  expect_message(kZero, [&] { call.plan(); });    // the zero lag is row 1, the long one row 0
  call.lags[4] = -4;
  expect_message(kLong, [&] { call.plan(); });
  call.lags[0] = 5;
  expect_message(kFinite, [&] { call.plan(); });
  call.directions[7] = 0.25;
  expect_message(kOverlap, [&] { call.plan(); });
  call.sums = address(kBase + 4 * kApart);
  expect_message(kOutputs, [&] { call.plan(); });
  call.totals = address(kBase + 5 * kApart);
  call.plan();
}

void test_shared_bytes() {
  const uint64_t cells = 6 * 5 * 7;
  const uint64_t grid_bytes = cells * 8;
  // the bytes of the outputs: pairs 4 * 8, sums 4 * 3 * 6 * 8, totals 16
  const uint64_t bytes[3] = {4 * 8, 4 * 3 * 6 * 8, 16};
  for (int c = 0; c < 3; ++c) {
    const uint64_t grid = kBase + static_cast<uint64_t>(c) * kApart;
    for (int out = 0; out < 3; ++out) {
      auto placed = [&](uint64_t at) {
        return spoilt([&](Call& call) {
          (out == 0 ? call.pairs : out == 1 ? call.sums : call.totals) = address(at);
        });
      };
      placed(grid - bytes[out]).plan();      // ends on the byte before the grid
      placed(grid + grid_bytes).plan();      // begins on the byte behind it
      for (uint64_t at : {grid - bytes[out] + 1, grid, grid + 8, grid + grid_bytes - 1}) {
        expect_message(kOverlap, [&] { placed(at).plan(); });
      }
    }
  }
  // with one component only its own grid counts
  {
    Call call = scalar_call();
    call.pairs = address(kBase + kApart);    // where the second grid of three would lie
    call.plan();
    call.pairs = address(kBase + 8);
    expect_message(kOverlap, [&] { call.plan(); });
  }
  // the sums of one component and order 1: 4 * 8 bytes
  {
    Call call = scalar_call();
    call.max_order = 1;
    call.sums = address(kBase - 32);
    call.plan();
    call.sums = address(kBase - 31);
    expect_message(kOverlap, [&] { call.plan(); });
  }
  // the components may alias each other
  spoilt([](Call& c) { c.grids[1] = c.grids[2] = c.grids[0]; }).plan();
  spoilt([](Call& c) { c.grids[1] = address(kBase + 8); }).plan();
  // among the outputs, to the byte
  const uint64_t pairs = kBase + 3 * kApart;
  spoilt([&](Call& c) { c.totals = address(pairs + 32); }).plan();
  spoilt([&](Call& c) { c.totals = address(pairs - 16); }).plan();
  for (uint64_t at : {pairs + 31, pairs, pairs - 15}) {
    expect_message(kOutputs, [&] { spoilt([&](Call& c) { c.totals = address(at); }).plan(); });
  }
  const uint64_t sums = kBase + 4 * kApart;
  spoilt([&](Call& c) { c.pairs = address(sums + bytes[1]); }).plan();
  spoilt([&](Call& c) { c.pairs = address(sums - 32); }).plan();
  for (uint64_t at : {sums + bytes[1] - 1, sums + 8, sums - 31}) {
    expect_message(kOutputs, [&] { spoilt([&](Call& c) { c.pairs = address(at); }).plan(); });
  }
  spoilt([&](Call& c) { c.totals = address(sums + bytes[1]); }).plan();
  expect_message(kOutputs, [&] {
    spoilt([&](Call& c) { c.totals = address(sums + bytes[1] - 1); }).plan();
  });
}

void test_one_cell_has_no_lag() {
  expect_message(kZero, [] {
    spoilt([](Call& c) {
      c.dims[0] = c.dims[1] = c.dims[2] = 1;
      c.n_lags = 1;
      c.lags = {0, 0, 0};
    }).plan();
  });
  expect_message(kLong, [] {
    spoilt([](Call& c) {
      c.dims[0] = c.dims[1] = c.dims[2] = 1;
      c.n_lags = 1;
      c.lags = {1, 0, 0};
    }).plan();
  });
}

}  // namespace

int main() {
  test_the_plan_by_hand();
  test_refusals();
  test_which_message_wins();
  test_shared_bytes();
  test_one_cell_has_no_lag();
  std::printf("ok\n");
  return 0;
}
