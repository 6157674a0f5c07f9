// The host plans of the inverse transform and the per-mode operators (csrc/avr_field_plans.h:
// plan_ifft3d, plan_spectrum_helmholtz, plan_spectrum_inverse_laplacian) as a plain C++ program,
// built with AddressSanitizer and UBSan and without HIP: every refusal message and which one wins
// when several rules are broken, the overlap rules to the byte (with made-up addresses: nothing is
// allocated or read), the limits of h at DBL_MIN and at overflow, the inverse table against the
// forward one, and the x pass's cut.  Prints "ok".
#include <cfloat>
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
const char kDims[] = "dims must be powers of two in [1, 1024]";
const char kIfftOverlap[] = "the spectrum, values and imag overlap";
const char kPositive[] = "inverse_length must be finite and positive";
const char kSmall[] = "inverse_length is too small: its square underflows";
const char kLarge[] = "inverse_length is too large: a squared wave number overflows";
const char kSixOverlap[] = "two of the six spectra overlap";
const char kLength[] = "inverse_length_sq must be finite and positive";
const char kScale[] = "scale must be finite";
const uint64_t kBase = uint64_t{1} << 40;

// A call of plan_spectrum_helmholtz with everything in order, to be spoilt one argument at a time:
// 64 modes, 1024 bytes a spectrum, the six arrays 4096 bytes apart.
struct Split {
  int32_t dims[3] = {8, 4, 2};
  double h[3] = {1.0, 0.5, 2.0};
  const double* spectra[3] = {address(kBase), address(kBase + 4096), address(kBase + 8192)};
  const double* compressive[3] = {address(kBase + 12288), address(kBase + 16384),
                                  address(kBase + 20480)};
  avr::SpectrumHelmholtzPlan plan() const {
    return avr::plan_spectrum_helmholtz(dims, h, spectra, compressive);
  }
};
template <class Change>
Split spoilt(Change&& change) {
  Split split;
  change(split);
  return split;
}

// The workgroups of a streaming kernel at the group boundary: 16384 modes are one group, 32768 two.
struct GroupShape {
  int32_t dims[3];
  uint32_t modes, groups;
};
const GroupShape kGroupShapes[] = {{{1, 1, 1}, 1, 1}, {{64, 16, 16}, 16384, 1},
                                   {{64, 32, 16}, 32768, 2}};

void test_inverse_twiddles() {
  for (int n : {2, 8, 1024}) {
    const std::vector<double> w = avr::fft_twiddles(n), v = avr::fft_inverse_twiddles(n);
    expect(v.size() == w.size() && v.size() == static_cast<size_t>(n), "n / 2 pairs");
    for (int m = 0; m < n / 2; ++m) {
      const double want[2] = {w[2 * m], -w[2 * m + 1]};
      expect(std::memcmp(&v[2 * m], want, sizeof(want)) == 0, "V[m] = (W[m].re, -W[m].im) by bits");
    }
    expect(v[0] == 1.0 && v[1] == 0.0 && !std::signbit(v[1]), "V[0] = (1, +0.0)");
  }
  expect(avr::fft_inverse_twiddles(1).empty(), "a line of one value has no twiddle");
}

void test_x_cut() {
  // (nx, the lines there are) -> the lines a workgroup stages: 2048 elements, at least a line
  expect(avr::fft_x_group(1, 1) == 1 && avr::fft_x_group(4096, 1) == 2048, "nx = 1");
  expect(avr::fft_x_group(3, 2) == 3 && avr::fft_x_group(1u << 20, 2) == 1024, "nx = 2");
  expect(avr::fft_x_group(1, 1024) == 1 && avr::fft_x_group(1u << 20, 1024) == 2, "nx = 1024");
  // ... and the shared description of the lines and passes, member by member
  const int32_t shapes[][3] = {{1, 1024, 2}, {2, 1024, 2}, {1024, 2, 1}, {1024, 1024, 1024},
                               {16, 8, 4},   {1, 1, 1},    {8, 8, 8},    {1024, 4, 2}};
  for (const auto& dims : shapes) {
    const avr::Fft3dPlan forward = avr::plan_fft3d(dims, address(kBase), address(kBase << 1));
    const avr::Ifft3dPlan inverse =
        avr::plan_ifft3d(dims, address(kBase << 1), address(kBase), nullptr);
    const avr::FftLinesDev& f = forward.args.lines;
    const avr::FftLinesDev& i = inverse.args.lines;
    expect(i.nx == f.nx && i.log2nx == f.log2nx && i.x_lines == f.x_lines &&
               i.x_group == f.x_group, "the inverse x pass is cut as the forward one");
    expect((static_cast<uint64_t>(i.x_group) << i.log2nx) * 16 <= 64 * 1024, "a group fits 64 KiB");
    expect(std::memcmp(i.pass, f.pass, sizeof(f.pass)) == 0, "the strided passes are the same");
    for (int which = 0; which < 2; ++which) {
      const avr::FftPassDev &p = i.pass[which], &q = f.pass[which];
      expect(p.n == q.n && p.log2n == q.log2n && p.planes == q.planes &&
                 p.columns == q.columns && p.group == q.group && p.groups == q.groups &&
                 p.last == q.last && p.plane_stride == q.plane_stride &&
                 p.line_stride == q.line_stride, "... member by member");
    }
    expect(f.nx == dims[0] && f.x_lines == static_cast<uint32_t>(dims[1] * dims[2]) &&
               f.pass[0].n == dims[1] && f.pass[1].n == dims[2], "the description is the grid's");
    for (int d = 0; d < 3; ++d) {
      expect(f.twiddle[d] == nullptr && i.twiddle[d] == nullptr, "no address is set");
      expect(forward.twiddle[d] == avr::fft_twiddles(dims[d]) &&
                 inverse.twiddle[d] == avr::fft_inverse_twiddles(dims[d]),
             "the forward tables W, the inverse tables V");
    }
  }
}

void test_ifft_plan() {
  {
    const int32_t dims[3] = {16, 8, 4};
    const avr::Ifft3dPlan plan =
        avr::plan_ifft3d(dims, address(kBase), address(kBase + 8192), address(kBase + 12288));
    const avr::FftLinesDev& a = plan.args.lines;
    expect(plan.args.spectrum == nullptr && plan.args.values == nullptr &&
               plan.args.imag == nullptr && a.twiddle[0] == nullptr,
           "the plan leaves every address null");
    expect(plan.twiddle[0] == avr::fft_inverse_twiddles(16) &&
               plan.twiddle[1] == avr::fft_inverse_twiddles(8) &&
               plan.twiddle[2] == avr::fft_inverse_twiddles(4), "one inverse table per axis");
    expect(plan.args.scale == 1.0 / 512.0 && a.x_lines == 32 && a.x_group == 32,
           "the scale and x pass");
    expect(a.pass[0].n == 8 && a.pass[0].line_stride == 16 && a.pass[1].n == 4 &&
               a.pass[1].line_stride == 128, "the y and z passes");
    int visited = 0;
    avr::FftLinesDev to{};
    plan.visit_tables(&to, [&](const double** where, const double* table, size_t count) {
      expect(where == &to.twiddle[visited] && table == plan.twiddle[visited].data() &&
                 count == plan.twiddle[visited].size(), "the tables are staged in axis order");
      ++visited;
    });
    expect(visited == 3, "three tables");
    const int32_t most[3] = {1024, 1024, 1024};
    expect(avr::plan_ifft3d(most, address(kBase), address(kBase << 2), nullptr).args.scale ==
               std::ldexp(1.0, -30), "1 / 2^30");
    const int32_t one[3] = {1, 1, 1};
    const avr::Ifft3dPlan least = avr::plan_ifft3d(one, address(kBase), address(kBase + 16), nullptr);
    expect(least.args.scale == 1.0 && least.args.lines.x_group == 1 &&
               least.twiddle[0].empty() && least.args.lines.pass[0].n == 1 &&
               least.args.lines.pass[1].n == 1, "one cell");
  }
  // the dims before the overlap
  const int32_t wrong[][3] = {{0, 4, 4}, {4, -8, 4}, {4, 4, 3}, {2048, 4, 4}, {4, 4, 1 << 30}};
  for (const auto& dims : wrong) {
    expect_message(kDims, [&] { avr::plan_ifft3d(dims, address(kBase), address(kBase), nullptr); });
  }
  // the overlap rule, to the byte: 64 cells are 1024 bytes of spectrum and 512 of each grid
  const int32_t dims[3] = {4, 4, 4};
  const uint64_t s = kBase;
  struct Case {
    uint64_t values, imag;  // imag 0: none
    bool refused;
  };
  const Case cases[] = {
      {s, 0, true},           {s + 1023, 0, true},         {s - 511, 0, true},
      {s + 1024, 0, false},   {s - 512, 0, false},         {s + 1024, s + 1023, true},
      {s + 1024, s - 511, true},                           {s + 1024, s + 1024, true},
      {s + 1024, s + 1535, true},                          {s + 1024, s + 513, true},
      {s + 1024, s + 1536, false},                         {s - 512, s + 1024, false},
      {s + 2048, s + 1024, false},                         {s - 512, s - 1024, false},
      {s - 512, s - 1023, true},
  };
  for (const Case& c : cases) {
    auto call = [&] {
      avr::plan_ifft3d(dims, address(s), address(c.values), c.imag ? address(c.imag) : nullptr);
    };
    if (c.refused) {
      expect_message(kIfftOverlap, call);
    } else {
      call();
    }
  }
}

void test_helmholtz_plan() {
  {
    const Split split;
    const avr::HelmholtzArgs a = split.plan().args;
    expect(a.log2n[0] == 3 && a.log2n[1] == 2 && a.log2n[2] == 1 && a.n_modes == 64, "the dims");
    expect(split.plan().groups == 1, "one workgroup");
    expect(a.h[0] == 1.0 && a.h[1] == 0.5 && a.h[2] == 2.0, "h");
    for (int d = 0; d < 3; ++d) {
      expect(a.spectra[d] == nullptr && a.compressive[d] == nullptr,
             "the plan leaves every address null");
    }
  }
  for (const GroupShape& s : kGroupShapes) {
    const avr::SpectrumHelmholtzPlan plan = spoilt([&](Split& split) {
      std::memcpy(split.dims, s.dims, sizeof(split.dims));
      for (uint64_t d = 0; d < 3; ++d) {  // 32768 modes are 512 KiB a spectrum
        split.spectra[d] = address(kBase + (d << 20));
        split.compressive[d] = address(kBase + ((d + 3) << 20));
      }
    }).plan();
    expect(plan.args.n_modes == s.modes && plan.groups == s.groups, "the launch shape");
  }
  const double inf = INFINITY, nan = NAN;
  for (int d = 0; d < 3; ++d) {
    expect_message(kNull, [&] { spoilt([&](Split& s) { s.spectra[d] = nullptr; }).plan(); });
    expect_message(kNull, [&] { spoilt([&](Split& s) { s.compressive[d] = nullptr; }).plan(); });
    for (double bad : {0.0, -1.0, inf, nan, -inf}) {
      expect_message(kPositive, [&] { spoilt([&](Split& s) { s.h[d] = bad; }).plan(); });
    }
    // h^2 >= DBL_MIN: sqrt(DBL_MIN) = 2^-511 is exact, and admitted; the double below is not
    const double least = std::ldexp(1.0, -511);
    expect(least * least == DBL_MIN, "2^-511 squared is DBL_MIN");
    spoilt([&](Split& s) { s.h[d] = least; }).plan();
    expect_message(kSmall, [&] {
      spoilt([&](Split& s) { s.h[d] = std::nextafter(least, 0.0); }).plan();
    });
    expect_message(kSmall, [&] { spoilt([&](Split& s) { s.h[d] = 5e-324; }).plan(); });
    // (512 h)^2 finite: h = 2^502 gives 2^1022; 2^503 gives 2^1024, which is not
    spoilt([&](Split& s) { s.h[d] = std::ldexp(1.0, 502); }).plan();
    spoilt([&](Split& s) { s.h[d] = std::ldexp(1.4142135623730949, 502); }).plan();
    expect_message(kLarge, [&] { spoilt([&](Split& s) { s.h[d] = std::ldexp(1.0, 503); }).plan(); });
    expect_message(kLarge, [&] { spoilt([&](Split& s) { s.h[d] = DBL_MAX; }).plan(); });
  }
  // which one wins: a null array, then the dims, then h axis by axis (on an axis the sign before
  // the size), then the overlap
  expect_message(kNull, [&] {
    spoilt([](Split& s) {
      s.compressive[2] = nullptr;
      s.dims[0] = 3;
      s.h[0] = -1.0;
    }).plan();
  });
  expect_message(kDims, [&] {
    spoilt([](Split& s) {
      s.dims[1] = 2048;
      s.h[0] = 0.0;
      s.spectra[1] = s.spectra[0];
    }).plan();
  });
  expect_message(kSmall, [&] {
    spoilt([](Split& s) {
      s.h[0] = 1e-200;
      s.h[1] = -1.0;
    }).plan();
  });
  expect_message(kPositive, [&] {
    spoilt([&](Split& s) {
      s.h[0] = nan;
      s.h[2] = 1e300;
      s.spectra[1] = s.spectra[0];
    }).plan();
  });
  expect_message(kLarge, [&] {
    spoilt([](Split& s) {
      s.h[2] = 1e300;
      s.compressive[0] = s.spectra[0];
    }).plan();
  });
  // the overlap rule, to the byte, among the six: each holds 1024 bytes
  const Split in_order;
  const double* const* all[2] = {in_order.spectra, in_order.compressive};
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 6; ++j) {
      if (i == j) continue;
      const uintptr_t other = reinterpret_cast<uintptr_t>(all[j / 3][j % 3]);
      auto moved = [&](uint64_t to) {
        Split split;
        const double** arrays = i < 3 ? split.spectra : split.compressive;
        arrays[i % 3] = address(to);
        return split;
      };
      expect_message(kSixOverlap, [&] { moved(other).plan(); });
      expect_message(kSixOverlap, [&] { moved(other + 1023).plan(); });
      expect_message(kSixOverlap, [&] { moved(other - 1023).plan(); });
      if (j == 5) moved(other + 1024).plan();   // behind the last: no neighbour there
      if (j == 0) moved(other - 1024).plan();   // before the first
    }
  }
  // arrays that touch without sharing a byte
  spoilt([](Split& s) {
    for (int d = 0; d < 3; ++d) {
      s.spectra[d] = address(kBase + 2048 * d);
      s.compressive[d] = address(kBase + 2048 * d + 1024);
    }
  }).plan();
}

void test_inverse_laplacian_plan() {
  const int32_t dims[3] = {8, 4, 2};
  const double g[3] = {1.0, 0.25, 4.0};
  const double inf = INFINITY, nan = NAN;
  for (double scale : {1.0, -1.0, 0.0, -0.0, DBL_MAX, -5e-324}) {
    const avr::InverseLaplacianArgs a =
        avr::plan_spectrum_inverse_laplacian(dims, g, scale).args;
    expect(std::memcmp(&a.scale, &scale, sizeof(scale)) == 0 && a.n_modes == 64 &&
               a.log2n[0] == 3 && a.log2n[1] == 2 && a.log2n[2] == 1 && a.g[0] == 1.0 &&
               a.g[1] == 0.25 && a.g[2] == 4.0 && a.spectrum == nullptr, "the arguments");
  }
  for (const GroupShape& s : kGroupShapes) {
    const avr::InverseLaplacianPlan plan = avr::plan_spectrum_inverse_laplacian(s.dims, g, 1.0);
    expect(plan.args.n_modes == s.modes && plan.groups == s.groups, "the launch shape");
  }
  for (double bad : {0.0, -1.0, inf, nan}) {
    for (int d = 0; d < 3; ++d) {
      double spoilt_g[3] = {1.0, 0.25, 4.0};
      spoilt_g[d] = bad;
      expect_message(kLength, [&] { avr::plan_spectrum_inverse_laplacian(dims, spoilt_g, 1.0); });
      expect_message(kLength, [&] { avr::plan_spectrum_inverse_laplacian(dims, spoilt_g, nan); });
    }
  }
  for (double bad : {inf, -inf, nan}) {
    expect_message(kScale, [&] { avr::plan_spectrum_inverse_laplacian(dims, g, bad); });
  }
  const int32_t wrong[3] = {8, 6, 2};
  const double no_g[3] = {0.0, 0.0, 0.0};
  expect_message(kDims, [&] { avr::plan_spectrum_inverse_laplacian(wrong, no_g, inf); });
}

}  // namespace

int main() {
  test_inverse_twiddles();
  test_x_cut();
  test_ifft_plan();
  test_helmholtz_plan();
  test_inverse_laplacian_plan();
  std::printf("ok\n");
  return 0;
}
