// The four-instruction bricklet offset of boxes with power-of-two bricklet counts
// (csrc/avr_brick_address.h: pow2_brick_shifts, pow2_brick_keys, pow2_brick_offset) as a plain C++
// program, built with AddressSanitizer and UBSan and without HIP: the one definition the march calls
// in its interior loops (as v_mul_u32_u24 and v_bfi_b32 there, as the same integer operations here)
// against the general formula of bricklet_offset (csrc/avr_kernels.hip), restated below, for every
// cell of a list of shapes and with the five fraction bits under the z index at 0, 13 and 31; the
// shapes that must not qualify; and the mode plan_frame (csrc/avr_host.cpp, compiled in) gives a
// box.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../amrvolumerenderer_amd/csrc/avr_brick_address.h"
#include "../../amrvolumerenderer_amd/csrc/avr_internal.h"

namespace {

void fail(const std::string& what) {
  std::fprintf(stderr, "FAILED: %s\n", what.c_str());
  std::exit(1);
}
void expect(bool condition, const std::string& what) {
  if (!condition) fail(what);
}

// bricklet_offset, as its comment in avr_kernels.hip states it: 128-byte bricklets of 8 x 4 x 4
// cells, x fastest inside, the bricklets z fastest, then y, then x
uint64_t general_offset(int i, int j, int k, int ny, int nz) {
  const uint64_t by = static_cast<uint64_t>(ny + 3) / 4, bz = static_cast<uint64_t>(nz + 3) / 4;
  return static_cast<uint64_t>(i & 7) + 8u * static_cast<uint64_t>(j & 3) +
         32u * static_cast<uint64_t>(k & 3) +
         128u * (static_cast<uint64_t>(k >> 2) + bz * (static_cast<uint64_t>(j >> 2) +
                                                       by * static_cast<uint64_t>(i >> 3)));
}
// ... and as the instructions evaluate it: i + 8 j + 32 k + y_pitch (j>>2) + x_pitch (i>>3) in 32
// bits, the two products of 24-bit operands
uint32_t pitched_offset(int i, int j, int k, int ny, int nz) {
  const uint32_t by = static_cast<uint32_t>(ny + 3) >> 2, bz = static_cast<uint32_t>(nz + 3) >> 2;
  const uint32_t y_pitch = bz * 128u - 32u, x_pitch = by * bz * 128u - 8u;
  const uint32_t ui = static_cast<uint32_t>(i), uj = static_cast<uint32_t>(j);
  uint32_t offset = (uj << 3) + ui;
  offset += static_cast<uint32_t>(k) << 5;
  offset += ((uj >> 2) & 0xffffffu) * (y_pitch & 0xffffffu);
  offset += ((ui >> 3) & 0xffffffu) * (x_pitch & 0xffffffu);
  return offset;
}

std::string name_of(int nx, int ny, int nz) {
  return std::to_string(nx) + " x " + std::to_string(ny) + " x " + std::to_string(nz);
}

// every `stride`-th cell in each direction, and the last one, of a qualifying shape
uint64_t cells_of(int nx, int ny, int nz, int want_sx, int want_sy, int stride) {
  const std::string name = name_of(nx, ny, nz);
  int sx = 0, sy = 0;
  expect(avr::pow2_brick_shifts(nx, ny, nz, &sx, &sy), name + " qualifies");
  expect(sx == want_sx && sy == want_sy, name + ": the shifts are " + std::to_string(sx) + ", " +
                                             std::to_string(sy));
  const avr::Pow2BrickKeys keys = avr::pow2_brick_keys(sx, sy);
  expect(keys.mul_x < (1u << 24) && keys.mul_y < (1u << 24), name + ": 24-bit multipliers");
  const uint32_t fractions[3] = {0u, 13u, 31u};
  uint64_t checked = 0;
  auto axis = [stride](int n, int v) { return v + stride < n ? v + stride : (v == n - 1 ? n : n - 1); };
  for (int i = 0; i < nx; i = axis(nx, i)) {
    for (int j = 0; j < ny; j = axis(ny, j)) {
      for (int k = 0; k < nz; k = axis(nz, k)) {
        const uint64_t want = general_offset(i, j, k, ny, nz);
        expect(want == pitched_offset(i, j, k, ny, nz), name + ": the two general forms agree");
        for (const uint32_t fraction : fractions) {
          const uint32_t z32 = (static_cast<uint32_t>(k) << 5) | fraction;
          const uint32_t got = avr::pow2_brick_offset(static_cast<uint32_t>(i),
                                                      static_cast<uint32_t>(j), z32, keys);
          if (got != want) {
            fail(name + " at (" + std::to_string(i) + ", " + std::to_string(j) + ", " +
                 std::to_string(k) + ") fraction " + std::to_string(fraction) + ": " +
                 std::to_string(got) + ", not " + std::to_string(want));
          }
          ++checked;
        }
      }
    }
  }
  return checked;
}

void shapes() {
  uint64_t checked = 0;
  checked += cells_of(8, 8, 8, 9, 8, 1);
  checked += cells_of(16, 16, 16, 11, 9, 1);
  checked += cells_of(64, 64, 64, 15, 11, 1);
  checked += cells_of(20, 16, 13, 11, 9, 1);    // partial bricklets in x and z
  checked += cells_of(256, 16, 16, 11, 9, 1);   // nx at its bound, 2^(sx-3)
  checked += cells_of(128, 128, 128, 17, 12, 5);  // the benchmark's boxes, sampled
  checked += cells_of(1, 1, 1, 7, 7, 1);
  checked += cells_of(16, 4, 16, 9, 9, 1);      // one bricklet in y: no y pitch bits at all
  checked += cells_of(4096, 16, 2048, 18, 16, 61);  // wide fields, sampled
  expect(checked > 3u * (512 + 4096 + 262144), "every cell of the small shapes was checked");

  const int rejected[][3] = {{257, 16, 16},   // nx above 2^(sx-3): the copies of i would overlap
                             {16, 24, 16},    // 6 bricklets in y
                             {16, 17, 16},    // 5 bricklets in y
                             {16, 16, 4},     // ny above 2^(sy-5): j<<3 would reach the y pitch bit
                             {8, 32, 8},      // the same
                             {16, 16, 20},    // 5 bricklets in z
                             {0, 16, 16},
                             {16, 16, 1 << 23}};  // the x pitch bit past what a 24-bit factor reaches
  for (const auto& shape : rejected) {
    int sx = -1, sy = -1;
    expect(!avr::pow2_brick_shifts(shape[0], shape[1], shape[2], &sx, &sy),
           name_of(shape[0], shape[1], shape[2]) + " does not qualify");
    expect(sx == -1 && sy == -1, "a shape that does not qualify leaves the shifts alone");
  }
}

// one box per entry through plan_frame; corners are lo + n * spacing
struct PlanCase {
  int nx, ny, nz;
  double lo, spacing;
  int want_mode;
};

void plans() {
  const PlanCase cases[] = {
      {8, 8, 8, 0.0, 0.125, avr::kPow2Bricks},
      {16, 16, 16, -0.5, 0.0625, avr::kPow2Bricks},
      {64, 64, 64, 0.25, 0.0078125, avr::kPow2Bricks},
      {20, 16, 13, 0.0, 0.03125, avr::kPow2Bricks},
      {256, 16, 16, -1.0, 0.0078125, avr::kPow2Bricks},
      {128, 128, 128, 0.0, 0.0078125, avr::kPow2Bricks},
      {257, 16, 16, -1.0, 0.0078125, avr::kPow2Multiply},
      {16, 24, 16, 0.0, 0.03125, avr::kPow2Multiply},
      {16, 17, 16, 0.0, 0.03125, avr::kPow2Multiply},
      {16, 16, 4, 0.0, 0.03125, avr::kPow2Multiply},
      {8, 32, 8, 0.0, 0.03125, avr::kPow2Multiply},
      {16, 16, 16, 0.0, 0.05, avr::kReciprocal},   // not a power-of-two spacing
      {8, 8, 8, 0.1, 0.1, avr::kReciprocal},
  };
  std::vector<avr_box> boxes;
  for (const PlanCase& c : cases) {
    avr_box box;
    std::memset(&box, 0, sizeof(box));
    const int n[3] = {c.nx, c.ny, c.nz};
    for (int axis = 0; axis < 3; ++axis) {
      box.min_corner[axis] = c.lo;
      box.max_corner[axis] = c.lo + n[axis] * c.spacing;
      box.dims[axis] = n[axis];
    }
    box.jstride = c.nx;
    box.kstride = static_cast<int64_t>(c.nx) * c.ny;
    // a made-up address that the plan does not read
    box.cells = reinterpret_cast<const double*>((uintptr_t{1} << 40) + (boxes.size() << 31));
    boxes.push_back(box);
  }
  avr_paint_params params{};
  params.width = 64;
  params.height = 48;
  params.scalar_range[1] = 1.0f;
  params.box_transparency = 0.5f;
  params.reference_sample_distance = 0.01f;
  for (int axis = 0; axis < 3; ++axis) {
    params.bounds_min[axis] = -2.0;
    params.bounds_max[axis] = 4.0;
  }
  avr_camera camera{};
  camera.eye[0] = 0.5f;
  camera.eye[1] = 0.6f;
  camera.eye[2] = 6.0f;
  camera.look_at[0] = camera.look_at[1] = camera.look_at[2] = 0.5f;
  camera.up[1] = 1.0f;
  camera.fov_y_degrees = 45.0f;
  camera.near_plane = 0.1f;
  camera.far_plane = 100.0f;
  avr_scalar_transform transform{};
  avr::FramePlan plan;
  avr::plan_frame(boxes.data(), static_cast<int>(boxes.size()), transform, params, camera, &plan);
  expect(plan.ready && plan.boxes.size() == boxes.size(), "the plan holds every box");
  for (size_t b = 0; b < boxes.size(); ++b) {
    const PlanCase& c = cases[b];
    const avr::BoxDev& dev = plan.boxes[b];
    const std::string name = name_of(c.nx, c.ny, c.nz) + " at spacing " + std::to_string(c.spacing);
    expect(dev.index_mode == c.want_mode, name + ": mode " + std::to_string(dev.index_mode) +
                                              ", not " + std::to_string(c.want_mode));
    int sx = 0, sy = 0;
    if (c.want_mode == avr::kPow2Bricks) {
      expect(avr::pow2_brick_shifts(c.nx, c.ny, c.nz, &sx, &sy) && dev.brick_sx == sx &&
                 dev.brick_sy == sy,
             name + ": the plan carries the shifts");
    } else {
      expect(dev.brick_sx == 0 && dev.brick_sy == 0, name + ": no shifts outside the mode");
    }
  }
}

}  // namespace

int main() {
  shapes();
  plans();
  std::puts("ok");
  return 0;
}
