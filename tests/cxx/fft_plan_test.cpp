// The host plans of the power spectra (csrc/avr_field_plans.h: plan_fft3d, plan_spectrum_bins) as
// a plain C++ program, built with AddressSanitizer and UBSan and without HIP: every refusal
// message and which one wins when several rules are broken, the 1024, 2^31 and 2048 limits
// (reached with made-up addresses: nothing is allocated or read), the overlap rules to the byte,
// the passes' strides and column groups with their last, partial group, the launch shapes of the
// grids that tests/test_fft_lengths*.py transform (lines of 64 to 1024 in every pass, the two
// that stage 64 KiB among them), and the twiddle table against cos and sin.  Prints "ok".
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

const void* address(uint64_t at) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(at)); }

const char kDims[] = "dims must be powers of two in [1, 1024]";
const char kCells[] = "the grid has 2^31 cells or more";
const uint64_t kValues = uint64_t{1} << 40, kSpectrum = uint64_t{1} << 44;

// A call of plan_spectrum_bins with everything in order, to be spoilt one argument at a time.
struct Bins {
  int32_t dims[3] = {8, 4, 2};
  double g[3] = {1.0, 0.25, 4.0};
  std::vector<double> edges = {0.0, 1.0, 2.0, 4.5};
  int n_bins = 3;
  const void* spectrum = address(kSpectrum);
  const void* modes = address(uint64_t{1} << 45);
  const void* power = address(uint64_t{1} << 46);
  const void* totals = address(uint64_t{1} << 47);
  avr::SpectrumBinsPlan plan() const {
    return avr::plan_spectrum_bins(dims, g, edges.data(), n_bins, spectrum, modes, power, totals);
  }
};

void test_twiddles() {
  const double pi = std::acos(-1.0);
  for (int n : {2, 8, 1024}) {
    const std::vector<double> table = avr::fft_twiddles(n);
    expect(table.size() == static_cast<size_t>(n), "n / 2 pairs");
    for (int m = 0; m < n / 2; ++m) {
      const double theta = -(2.0 * pi * static_cast<double>(m)) / static_cast<double>(n);
      const double want[2] = {std::cos(theta), std::sin(theta)};
      expect(std::memcmp(&table[2 * m], want, sizeof(want)) == 0, "W[m] = (cos, sin) by bits");
    }
    expect(table[0] == 1.0 && table[1] == 0.0 && std::signbit(table[1]), "W[0] = (1, -0.0)");
  }
  expect(avr::fft_twiddles(1).empty(), "a line of one value has no twiddle");
  // W[n / 4] is what the C library gives for -pi / 2, not the exact -i
  const std::vector<double> eight = avr::fft_twiddles(8);
  expect(eight[4] == std::cos(-(2.0 * pi * 2.0) / 8.0) && eight[4] != 0.0 && eight[5] == -1.0,
         "W[n / 4] keeps its rounded cosine");
}

void test_column_groups() {
  struct Want {
    uint64_t columns;
    int n;
    uint32_t group, groups, last;
  };
  const Want cases[] = {
      {1, 1024, 1, 1, 1},        // nx = 1: one column per workgroup
      {2, 1024, 2, 1, 2},        // nx = 2: below the smallest group
      {4, 1024, 4, 1, 4},        {1024, 1024, 4, 256, 4},  // 4 lines of 1024: 64 KiB
      {1024, 512, 4, 256, 4},    {1024, 256, 8, 128, 8},   {1024, 2, 1024, 1, 1024},
      {1u << 20, 2, 1024, 1024, 1024},
      {10, 1024, 4, 3, 2},       // no multiple of the group: a last group of 2
      {9, 256, 8, 2, 1},         {1000, 64, 32, 32, 8},
  };
  for (const Want& want : cases) {
    const avr::FftColumnGroups got = avr::fft_column_groups(want.columns, want.n);
    expect(got.group == want.group && got.groups == want.groups && got.last == want.last,
           "column groups of " + std::to_string(want.columns) + " columns of " +
               std::to_string(want.n));
    expect(static_cast<uint64_t>(got.groups - 1) * got.group + got.last == want.columns,
           "the groups hold every column once");
    expect(static_cast<uint64_t>(got.group) * want.n * 16 <= 64 * 1024, "a group fits 64 KiB");
    expect(got.last >= 1 && got.last <= got.group, "the last group holds 1 .. group columns");
  }
}

void test_fft_plan() {
  {
    const int32_t dims[3] = {16, 8, 4};
    const avr::Fft3dPlan plan = avr::plan_fft3d(dims, address(kValues), address(kSpectrum));
    const avr::FftLinesDev& a = plan.args.lines;
    expect(plan.args.values == nullptr && plan.args.spectrum == nullptr &&
               a.twiddle[0] == nullptr, "the plan leaves every address null");
    expect(plan.twiddle[0].size() == 16 && plan.twiddle[1].size() == 8 &&
               plan.twiddle[2].size() == 4, "one table per axis");
    expect(a.nx == 16 && a.log2nx == 4 && a.x_lines == 32 && a.x_group == 32, "the x pass");
    const avr::FftPassDev& y = a.pass[0];
    expect(y.n == 8 && y.log2n == 3 && y.planes == 4 && y.columns == 16 && y.group == 16 &&
               y.groups == 1 && y.last == 16 && y.plane_stride == 128 && y.line_stride == 16,
           "the y pass");
    const avr::FftPassDev& z = a.pass[1];
    expect(z.n == 4 && z.log2n == 2 && z.planes == 1 && z.columns == 128 && z.group == 128 &&
               z.groups == 1 && z.last == 128 && z.line_stride == 128, "the z pass");
    int visited = 0;
    avr::FftLinesDev to{};
    plan.visit_tables(&to, [&](const double** where, const double* table, size_t count) {
      expect(where == &to.twiddle[visited] && table == plan.twiddle[visited].data() &&
                 count == plan.twiddle[visited].size(), "the tables are staged in axis order");
      ++visited;
    });
    expect(visited == 3, "three tables");
  }
  {  // the longest lines: 2 lines of 1024 along x, 4 columns of 1024 along y and z
    const int32_t dims[3] = {1024, 1024, 1024};  // 2^30 cells, the most the dims rule admits
    const avr::Fft3dPlan plan = avr::plan_fft3d(dims, address(kValues), address(kSpectrum));
    const avr::FftLinesDev& a = plan.args.lines;
    expect(a.x_lines == (1u << 20) && a.x_group == 2, "x: 2 lines of 1024");
    expect(a.pass[0].planes == 1024 && a.pass[0].group == 4 && a.pass[0].groups == 256 &&
               a.pass[0].last == 4, "y: 4 columns");
    expect(a.pass[1].columns == (1u << 20) && a.pass[1].groups == (1u << 18) &&
               a.pass[1].line_stride == (uint64_t{1} << 20), "z: 2^18 groups");
  }
  {  // axes of one value, and nx below the column group
    const int32_t dims[3] = {2, 1024, 1};
    const avr::Fft3dPlan plan = avr::plan_fft3d(dims, address(kValues), address(kSpectrum));
    const avr::FftLinesDev& a = plan.args.lines;
    expect(plan.twiddle[2].empty() && a.pass[1].n == 1 && a.pass[1].log2n == 0,
           "an axis of one value has no table");
    expect(a.x_group == 1024 && a.pass[0].group == 2 && a.pass[0].groups == 1 &&
               a.pass[0].last == 2, "two columns");
    const int32_t one[3] = {1, 1, 1};
    const avr::Fft3dPlan least = avr::plan_fft3d(one, address(kValues), address(kSpectrum));
    const avr::FftLinesDev& b = least.args.lines;
    expect(b.x_lines == 1 && b.x_group == 1 && b.log2nx == 0, "1 cell");
  }
  // the messages, and which one wins
  const int32_t wrong[][3] = {{0, 4, 4}, {4, -8, 4}, {4, 4, 3}, {2048, 4, 4}, {4, 4, 1 << 30},
                              {6, 2048, 0}};
  for (const auto& dims : wrong) {
    expect_message(kDims, [&] { avr::plan_fft3d(dims, address(kValues), address(kValues)); });
    Bins bins;
    std::memcpy(bins.dims, dims, sizeof(bins.dims));
    bins.n_bins = 0;
    expect_message(kDims, [&] { bins.plan(); });
  }
  // 2^31 cells: the dims rule keeps a grid at 2^30 cells, so the rule stands behind it unreached
  const int32_t most[3] = {1024, 1024, 1024};
  expect(avr::require_fft_dims(most) == (uint64_t{1} << 30), "2^30 cells are admitted");
  (void)kCells;
  // the overlap rule, to the byte: 64 cells are 512 bytes of input and 1024 of spectrum
  const int32_t dims[3] = {4, 4, 4};
  const char kOverlap[] = "the spectrum overlaps the input";
  expect_message(kOverlap, [&] { avr::plan_fft3d(dims, address(kValues), address(kValues)); });
  expect_message(kOverlap,
                 [&] { avr::plan_fft3d(dims, address(kValues), address(kValues + 511)); });
  expect_message(kOverlap,
                 [&] { avr::plan_fft3d(dims, address(kValues), address(kValues - 1023)); });
  avr::plan_fft3d(dims, address(kValues), address(kValues + 512));
  avr::plan_fft3d(dims, address(kValues), address(kValues - 1024));
}

// The shapes of tests/test_fft_lengths.py and tests/test_fft_lengths_gpu.py, written out by hand
// from kFftGroupElements = 2048 and kFftMinColumns = 4: per length N one grid whose x pass, one
// whose y pass and one whose z pass takes lines of N in two full groups (the y ones in two planes),
// and a cube.  If this fails because the group constants changed, choose those tests' shapes again
// (ROLES in test_fft_lengths.py) so that they keep what their comments say, then these values.
void test_length_shapes() {
  struct Pass {
    uint32_t group, groups, last, planes;
  };
  struct Want {
    int32_t dims[3];  // (nx, ny, nz)
    uint32_t x_lines, x_group;
    Pass y, z;
  };
  const Want cases[] = {
      // N = 64
      {{64, 64, 1}, 64, 32, {32, 2, 32, 1}, {2048, 2, 2048, 1}},
      {{64, 64, 2}, 128, 32, {32, 2, 32, 2}, {1024, 4, 1024, 1}},
      {{32, 2, 64}, 128, 64, {32, 1, 32, 64}, {32, 2, 32, 1}},
      // N = 128
      {{128, 32, 1}, 32, 16, {64, 2, 64, 1}, {2048, 2, 2048, 1}},
      {{32, 128, 2}, 256, 64, {16, 2, 16, 2}, {1024, 4, 1024, 1}},
      {{16, 2, 128}, 256, 128, {16, 1, 16, 128}, {16, 2, 16, 1}},
      // N = 256
      {{256, 16, 1}, 16, 8, {128, 2, 128, 1}, {2048, 2, 2048, 1}},
      {{16, 256, 2}, 512, 128, {8, 2, 8, 2}, {1024, 4, 1024, 1}},
      {{8, 2, 256}, 512, 256, {8, 1, 8, 256}, {8, 2, 8, 1}},
      // N = 512
      {{512, 8, 1}, 8, 4, {256, 2, 256, 1}, {2048, 2, 2048, 1}},
      {{8, 512, 2}, 1024, 256, {4, 2, 4, 2}, {1024, 4, 1024, 1}},
      {{4, 2, 512}, 1024, 512, {4, 1, 4, 512}, {4, 2, 4, 1}},
      // N = 1024
      {{1024, 4, 1}, 4, 2, {512, 2, 512, 1}, {2048, 2, 2048, 1}},
      {{8, 1024, 2}, 2048, 256, {4, 2, 4, 2}, {1024, 8, 1024, 1}},
      {{4, 2, 1024}, 2048, 512, {4, 1, 4, 1024}, {4, 2, 4, 1}},
      // the cube
      {{64, 64, 64}, 4096, 32, {32, 2, 32, 64}, {32, 128, 32, 1}},
  };
  const std::string again = "; the group constants changed: choose the shapes of "
                            "tests/test_fft_lengths.py again";
  for (const Want& want : cases) {
    const std::string name = std::to_string(want.dims[0]) + " x " + std::to_string(want.dims[1]) +
                             " x " + std::to_string(want.dims[2]);
    const avr::FftLinesDev a = avr::fft_lines(want.dims);
    expect(a.x_lines == want.x_lines && a.x_group == want.x_group,
           "the x pass of " + name + again);
    expect((static_cast<uint64_t>(a.x_group) << a.log2nx) * 16 <= 32 * 1024,
           "the x pass of " + name + " stages at most 32 KiB");
    const Pass* passes[2] = {&want.y, &want.z};
    for (int which = 0; which < 2; ++which) {
      const avr::FftPassDev& got = a.pass[which];
      const Pass& p = *passes[which];
      expect(got.group == p.group && got.groups == p.groups && got.last == p.last &&
                 got.planes == p.planes,
             std::string(which == 0 ? "the y pass of " : "the z pass of ") + name + again);
      expect(got.n == 1 || (static_cast<uint64_t>(got.group) << got.log2n) * 16 <= 64 * 1024,
             "a group of " + name + " fits 64 KiB");
    }
  }
  // the two launches that ask for all of the 64 KiB: 4 columns of 1024
  const int32_t along_y[3] = {8, 1024, 2}, along_z[3] = {4, 2, 1024};
  const avr::FftPassDev y = avr::fft_lines(along_y).pass[0], z = avr::fft_lines(along_z).pass[1];
  expect((static_cast<uint64_t>(y.group) << y.log2n) * 16 == 65536,
         "the y pass of 8 x 1024 x 2 stages exactly 65536 bytes" + again);
  expect((static_cast<uint64_t>(z.group) << z.log2n) * 16 == 65536,
         "the z pass of 4 x 2 x 1024 stages exactly 65536 bytes" + again);
}

void test_bins_plan() {
  {
    const Bins bins;
    const avr::SpectrumBinsPlan plan = bins.plan();
    const avr::SpectrumBinsArgs& a = plan.args;
    expect(plan.edges_sq == bins.edges && a.n_bins == 3 && a.n_modes == 64, "the edges");
    expect(a.log2n[0] == 3 && a.log2n[1] == 2 && a.log2n[2] == 1, "log2 of the dims");
    expect(a.g[0] == 1.0 && a.g[1] == 0.25 && a.g[2] == 4.0, "g");
    expect(a.spectrum == nullptr && a.edges_sq == nullptr && a.modes == nullptr &&
               a.power == nullptr && a.totals == nullptr, "the plan leaves every address null");
    expect(plan.groups == 1, "one workgroup");
  }
  {  // the workgroups at the group boundary: 16384 modes are one group, 32768 two
    struct Shape {
      int32_t dims[3];
      uint32_t modes, groups;
    };
    const Shape shapes[] = {{{1, 1, 1}, 1, 1}, {{64, 16, 16}, 16384, 1}, {{64, 32, 16}, 32768, 2}};
    for (const Shape& s : shapes) {
      Bins bins;
      std::memcpy(bins.dims, s.dims, sizeof(bins.dims));
      const avr::SpectrumBinsPlan plan = bins.plan();
      expect(plan.args.n_modes == s.modes && plan.groups == s.groups, "the launch shape");
    }
  }
  const double inf = INFINITY, nan = NAN;
  auto spoilt = [](auto&& change) {
    Bins bins;
    change(bins);
    return bins;
  };
  auto edges = [&](std::vector<double> e) {
    return spoilt([&](Bins& b) {
      b.n_bins = static_cast<int>(e.size()) - 1;
      b.edges = e;
    });
  };
  const char kBins[] = "n_bins must lie in [1, 2048]";
  const char kFinite[] = "edges_sq must be finite";
  const char kNegative[] = "edges_sq must not be negative";
  const char kIncreasing[] = "edges_sq must be strictly increasing";
  const char kLength[] = "inverse_length_sq must be finite and positive";
  const char kOverlap[] = "an output array overlaps the spectrum";
  expect_message(kBins, [&] { spoilt([](Bins& b) { b.n_bins = 0; }).plan(); });
  expect_message(kBins, [&] { spoilt([](Bins& b) { b.n_bins = -1; }).plan(); });
  {  // 2048 bins are admitted, 2049 are not (before an edge is read)
    Bins most;
    most.edges.resize(2049);
    for (int i = 0; i <= 2048; ++i) most.edges[i] = static_cast<double>(i);
    most.n_bins = 2048;
    expect(most.plan().edges_sq.size() == 2049, "2048 bins");
    most.n_bins = 2049;
    expect_message(kBins, [&] { most.plan(); });
  }
  expect_message(kFinite, [&] { edges({0.0, inf}).plan(); });
  expect_message(kFinite, [&] { edges({nan, 1.0}).plan(); });
  expect_message(kFinite, [&] { edges({-1.0, 3.0, 2.0, inf}).plan(); });  // finite before the rest
  expect_message(kNegative, [&] { edges({-1.0, 1.0}).plan(); });
  expect_message(kNegative, [&] { edges({-1.0, 3.0, 2.0}).plan(); });      // ... before the order
  expect_message(kIncreasing, [&] { edges({0.0, 1.0, 1.0}).plan(); });
  expect_message(kIncreasing, [&] { edges({2.0, 1.0}).plan(); });
  edges({0.0, 5e-324}).plan();
  edges({3.0, 4.0}).plan();
  for (double bad : {0.0, -1.0, inf, nan}) {
    for (int d = 0; d < 3; ++d) {
      expect_message(kLength, [&] { spoilt([&](Bins& b) { b.g[d] = bad; }).plan(); });
    }
  }
  // the edges before g, g before the overlap
  expect_message(kIncreasing, [&] {
    spoilt([](Bins& b) {
      b.edges[1] = 0.0;
      b.g[0] = 0.0;
      b.modes = b.spectrum;
    }).plan();
  });
  expect_message(kLength, [&] {
    spoilt([](Bins& b) {
      b.g[2] = -1.0;
      b.power = b.spectrum;
    }).plan();
  });
  // the overlap rule, to the byte: 64 modes are 1024 bytes, 3 bins are 24 bytes, the totals 16
  expect_message(kOverlap, [&] { spoilt([](Bins& b) { b.modes = b.spectrum; }).plan(); });
  expect_message(kOverlap, [&] { spoilt([](Bins& b) { b.power = address(kSpectrum + 1023); }).plan(); });
  expect_message(kOverlap, [&] { spoilt([](Bins& b) { b.power = address(kSpectrum - 23); }).plan(); });
  expect_message(kOverlap, [&] { spoilt([](Bins& b) { b.totals = address(kSpectrum - 15); }).plan(); });
  spoilt([](Bins& b) { b.power = address(kSpectrum + 1024); }).plan();
  spoilt([](Bins& b) { b.modes = address(kSpectrum - 24); }).plan();
  spoilt([](Bins& b) { b.totals = address(kSpectrum - 16); }).plan();
}

}  // namespace

int main() {
  test_twiddles();
  test_column_groups();
  test_fft_plan();
  test_length_shapes();
  test_bins_plan();
  std::printf("ok\n");
  return 0;
}
