// The host plans of the isolated potential (csrc/avr_field_plans.h: plan_isolated_green,
// plan_spectrum_multiply) as a plain C++ program, built with AddressSanitizer and UBSan and without
// HIP: every refusal message and which one wins when several rules are broken, the limits of the
// cell size at DBL_MIN and at overflow, the overlap rule to the byte (with made-up addresses:
// nothing is allocated or read), the cell count at 2^30 and 2^31, and the launch shape.  Prints
// "ok".
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

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
const char kCells[] = "the grid has 2^31 cells or more";
const char kPositive[] = "cell_size must be finite and positive";
const char kSmall[] = "cell_size is too small: its square underflows";
const char kLarge[] = "cell_size is too large: a squared distance overflows";
const char kFinite[] = "scale and self_value must be finite";
const char kOverlap[] = "the two spectra overlap";
const uint64_t kBase = uint64_t{1} << 40;

// A call of plan_isolated_green with everything in order, to be spoilt one argument at a time.
struct Green {
  int32_t dims[3] = {16, 4, 8};
  double size[3] = {0.5, 0.25, 1.0};
  double scale = -0.3, self_value = 1.5;
  const double* green = address(kBase);
  bool no_dims = false, no_size = false;
  avr::IsolatedGreenPlan plan() const {
    return avr::plan_isolated_green(no_dims ? nullptr : dims, no_size ? nullptr : size, scale,
                                    self_value, green);
  }
};
template <class Change>
Green spoilt(Change&& change) {
  Green call;
  change(call);
  return call;
}

void test_cell_count() {
  avr::require_cell_count(1);
  avr::require_cell_count(uint64_t{1} << 30);
  avr::require_cell_count((uint64_t{1} << 31) - 1);
  expect_message(kCells, [] { avr::require_cell_count(uint64_t{1} << 31); });
  expect_message(kCells, [] { avr::require_cell_count(uint64_t{1} << 33); });
  expect(avr::spectral_groups(1) == 1 && avr::spectral_groups(16384) == 1 &&
             avr::spectral_groups(16385) == 2 && avr::spectral_groups(uint64_t{1} << 30) == 65536,
         "16384 elements a workgroup");
}

void test_green_plan() {
  {
    const Green call;
    const avr::IsolatedGreenPlan plan = call.plan();
    const avr::IsolatedGreenArgs& a = plan.args;
    expect(a.green == nullptr, "the plan leaves the address null");
    expect(a.log2n[0] == 4 && a.log2n[1] == 2 && a.log2n[2] == 3 && a.n_cells == 512, "the dims");
    expect(a.size[0] == 0.5 && a.size[1] == 0.25 && a.size[2] == 1.0 && a.scale == -0.3 &&
               a.self_value == 1.5, "the sizes, scale and self_value");
    expect(plan.groups == 1, "one workgroup");
  }
  // the launch shape
  struct Shape {
    int32_t dims[3];
    uint32_t cells, groups;
  };
  const Shape shapes[] = {{{1, 1, 1}, 1u, 1u},
                          {{4, 1, 1}, 4u, 1u},
                          {{32, 32, 32}, 32768u, 2u},
                          {{4, 1024, 8}, 32768u, 2u},
                          {{64, 32, 16}, 32768u, 2u},
                          {{1024, 1024, 1024}, 1u << 30, 65536u}};
  for (const Shape& s : shapes) {
    const avr::IsolatedGreenPlan plan = spoilt([&](Green& c) {
      std::memcpy(c.dims, s.dims, sizeof(s.dims));
    }).plan();
    expect(plan.args.n_cells == s.cells && plan.groups == s.groups, "the launch shape");
    expect(static_cast<uint64_t>(plan.groups) * avr::kSpectralGroupElements >= s.cells &&
               static_cast<uint64_t>(plan.groups - 1) * avr::kSpectralGroupElements < s.cells,
           "every workgroup has a cell, every cell a workgroup");
    expect((1u << plan.args.log2n[0]) == static_cast<uint32_t>(s.dims[0]) &&
               (1u << plan.args.log2n[1]) == static_cast<uint32_t>(s.dims[1]) &&
               (1u << plan.args.log2n[2]) == static_cast<uint32_t>(s.dims[2]), "the shifts");
  }
  const double inf = INFINITY, nan = NAN;
  expect_message(kNull, [&] { spoilt([](Green& c) { c.no_dims = true; }).plan(); });
  expect_message(kNull, [&] { spoilt([](Green& c) { c.no_size = true; }).plan(); });
  expect_message(kNull, [&] { spoilt([](Green& c) { c.green = nullptr; }).plan(); });
  for (int d = 0; d < 3; ++d) {
    for (int32_t bad : {0, -4, 3, 12, 2048, 1 << 30}) {
      expect_message(kDims, [&] { spoilt([&](Green& c) { c.dims[d] = bad; }).plan(); });
    }
    for (double bad : {0.0, -1.0, inf, nan, -inf}) {
      expect_message(kPositive, [&] { spoilt([&](Green& c) { c.size[d] = bad; }).plan(); });
    }
    // size^2 >= DBL_MIN: sqrt(DBL_MIN) = 2^-511 is exact, and admitted; the double below is not
    const double least = std::ldexp(1.0, -511);
    expect(least * least == DBL_MIN, "2^-511 squared is DBL_MIN");
    spoilt([&](Green& c) { c.size[d] = least; }).plan();
    expect_message(kSmall, [&] {
      spoilt([&](Green& c) { c.size[d] = std::nextafter(least, 0.0); }).plan();
    });
    expect_message(kSmall, [&] { spoilt([&](Green& c) { c.size[d] = 5e-324; }).plan(); });
    // (512 size)^2 finite: size = 2^502 gives 2^1022; 2^503 gives 2^1024, which is not
    spoilt([&](Green& c) { c.size[d] = std::ldexp(1.0, 502); }).plan();
    spoilt([&](Green& c) { c.size[d] = std::ldexp(1.4142135623730949, 502); }).plan();
    expect_message(kLarge, [&] { spoilt([&](Green& c) { c.size[d] = std::ldexp(1.0, 503); }).plan(); });
    expect_message(kLarge, [&] { spoilt([&](Green& c) { c.size[d] = DBL_MAX; }).plan(); });
  }
  for (double bad : {inf, -inf, nan}) {
    expect_message(kFinite, [&] { spoilt([&](Green& c) { c.scale = bad; }).plan(); });
    expect_message(kFinite, [&] { spoilt([&](Green& c) { c.self_value = bad; }).plan(); });
  }
  for (double fine : {0.0, -0.0, DBL_MAX, -5e-324}) {
    const avr::IsolatedGreenArgs a = spoilt([&](Green& c) {
      c.scale = fine;
      c.self_value = -fine;
    }).plan().args;
    const double negated = -fine;
    expect(std::memcmp(&a.scale, &fine, sizeof(fine)) == 0 &&
               std::memcmp(&a.self_value, &negated, sizeof(fine)) == 0, "the bits are kept");
  }
  // which one wins: a null array, then the dims, then the size axis by axis (on an axis the sign
  // before the size), then scale and self_value
  expect_message(kNull, [&] {
    spoilt([&](Green& c) {
      c.green = nullptr;
      c.dims[0] = 3;
      c.size[0] = -1.0;
      c.scale = nan;
    }).plan();
  });
  expect_message(kDims, [&] {
    spoilt([&](Green& c) {
      c.dims[2] = 2048;
      c.size[0] = 0.0;
      c.self_value = inf;
    }).plan();
  });
  expect_message(kSmall, [&] {
    spoilt([&](Green& c) {
      c.size[0] = 1e-200;
      c.size[1] = -1.0;
      c.scale = inf;
    }).plan();
  });
  expect_message(kPositive, [&] {
    spoilt([&](Green& c) {
      c.size[0] = nan;
      c.size[2] = 1e300;
    }).plan();
  });
  expect_message(kLarge, [&] {
    spoilt([&](Green& c) {
      c.size[2] = 1e300;
      c.scale = nan;
    }).plan();
  });
}

void test_multiply_plan() {
  const int32_t dims[3] = {8, 4, 2};  // 64 modes: 1024 bytes a spectrum
  const uint64_t a = kBase;
  {
    const avr::SpectrumMultiplyPlan plan =
        avr::plan_spectrum_multiply(dims, address(a), address(a + 1024));
    expect(plan.args.a == nullptr && plan.args.b == nullptr, "the plan leaves the addresses null");
    expect(plan.args.n_modes == 64 && plan.groups == 1, "the modes and the launch shape");
  }
  struct Shape {
    int32_t dims[3];
    uint32_t modes, groups;
  };
  const Shape shapes[] = {{{1, 1, 1}, 1u, 1u},
                          {{4, 1, 1}, 4u, 1u},
                          {{128, 128, 1}, 16384u, 1u},
                          {{128, 128, 2}, 32768u, 2u},
                          {{1024, 1024, 1024}, 1u << 30, 65536u}};
  for (const Shape& s : shapes) {
    const avr::SpectrumMultiplyPlan plan =
        avr::plan_spectrum_multiply(s.dims, address(kBase), address(kBase << 2));
    expect(plan.args.n_modes == s.modes && plan.groups == s.groups, "the launch shape");
  }
  expect_message(kNull, [&] { avr::plan_spectrum_multiply(nullptr, address(a), address(a + 1024)); });
  expect_message(kNull, [&] { avr::plan_spectrum_multiply(dims, nullptr, address(a)); });
  expect_message(kNull, [&] { avr::plan_spectrum_multiply(dims, address(a), nullptr); });
  const int32_t wrong[][3] = {{0, 4, 4}, {4, -8, 4}, {4, 4, 3}, {2048, 4, 4}, {4, 4, 1 << 30}};
  for (const auto& bad : wrong) {
    // the dims before the overlap, a null array before the dims
    expect_message(kDims, [&] { avr::plan_spectrum_multiply(bad, address(a), address(a)); });
    expect_message(kNull, [&] { avr::plan_spectrum_multiply(bad, address(a), nullptr); });
  }
  // the overlap rule, to the byte
  struct Case {
    uint64_t b;
    bool refused;
  };
  const Case cases[] = {{a, true},         {a + 16, true},     {a + 1023, true},
                        {a - 1023, true},  {a - 16, true},     {a + 1024, false},
                        {a - 1024, false}, {a + 4096, false},  {a - 4096, false}};
  for (const Case& c : cases) {
    auto call = [&] { avr::plan_spectrum_multiply(dims, address(a), address(c.b)); };
    auto swapped = [&] { avr::plan_spectrum_multiply(dims, address(c.b), address(a)); };
    if (c.refused) {
      expect_message(kOverlap, call);
      expect_message(kOverlap, swapped);
    } else {
      call();
      swapped();
    }
  }
}

}  // namespace

int main() {
  test_cell_count();
  test_green_plan();
  test_multiply_plan();
  std::printf("ok\n");
  return 0;
}
