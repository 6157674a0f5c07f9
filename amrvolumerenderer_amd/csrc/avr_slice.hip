// Slice images of the raw AMR field ("Slice"): a plane through the scene, per pixel
// the raw f64 value of the one cell that contains the pixel's point, the AMR level of its box and
// the box's index -- no interpolation, no transform, no classified volume.
//
//   slice_kernel          point location over the scene's boxes + one f64 gather per pixel
//   slice_outline_kernel  box boundaries of a slice's box image, drawn into its RGB8 picture
//
// One lane owns a pixel, one wave an 8 x 8 pixel tile.  A pixel's point is affine in (x, y) and
// every rounding of its evaluation is monotone, so the points of a tile lie in the axis-aligned
// box of its four corner pixels: the wave tests the scene's boxes against that box 64 at a time
// (one box per lane, then a ballot -- the pattern of the march's box cull), and its lanes test
// their own point only against the survivors.  The scene's boxes are disjoint and the containment
// test is half-open, so a lane is done with the first box that contains its point, and the wave
// leaves the loop when a ballot shows that every lane is done.  All arithmetic is IEEE binary64
// (the library is built with -ffp-contract=off: nothing is fused).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kSliceTile = 8;      // pixels per side of a wave's tile
constexpr int kSliceThreads = 256;  // four waves = 2 x 2 tiles = 16 x 16 pixels per workgroup

__device__ __forceinline__ double slice_point(const SlicePlaneDev& plane, int axis, double fx,
                                              double fy) {
  // the operand order of DESIGN.md: (origin + fx * du) + fy * dv
  return (plane.origin[axis] + fx * plane.du[axis]) + fy * plane.dv[axis];
}

__global__ __launch_bounds__(kSliceThreads) void slice_kernel(
    const SlicePlaneDev plane, const int width, const int height,
    const SliceBoxDev* __restrict__ boxes, const int n_boxes, double* __restrict__ value,
    int8_t* __restrict__ level, int32_t* __restrict__ box_index) {
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int tile_x0 = (static_cast<int>(blockIdx.x) * 2 + (wave & 1)) * kSliceTile;
  const int tile_y0 = (static_cast<int>(blockIdx.y) * 2 + (wave >> 1)) * kSliceTile;
  if (tile_x0 >= width || tile_y0 >= height) return;  // wave-uniform
  const int x = tile_x0 + (lane & (kSliceTile - 1));
  const int y = tile_y0 + (lane >> 3);
  const bool in_image = x < width && y < height;

  const double fx = static_cast<double>(x) + 0.5;
  const double fy = static_cast<double>(y) + 0.5;
  double p[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = slice_point(plane, a, fx, fy);

  // the tile's box: per axis the extremes over its four corner pixels (wave-uniform)
  double lo[3], hi[3];
  {
    const double x_first = static_cast<double>(tile_x0) + 0.5;
    const double x_last = static_cast<double>(tile_x0 + (kSliceTile - 1)) + 0.5;
    const double y_first = static_cast<double>(tile_y0) + 0.5;
    const double y_last = static_cast<double>(tile_y0 + (kSliceTile - 1)) + 0.5;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double c0 = slice_point(plane, a, x_first, y_first);
      const double c1 = slice_point(plane, a, x_last, y_first);
      const double c2 = slice_point(plane, a, x_first, y_last);
      const double c3 = slice_point(plane, a, x_last, y_last);
      const double m01 = (c1 < c0) ? c1 : c0, m23 = (c3 < c2) ? c3 : c2;
      const double x01 = (c1 > c0) ? c1 : c0, x23 = (c3 > c2) ? c3 : c2;
      lo[a] = (m23 < m01) ? m23 : m01;
      hi[a] = (x23 > x01) ? x23 : x01;
    }
  }

  int found = -1;              // position of the lane's box in `boxes`
  bool done = !in_image;
  for (int base = 0; base < n_boxes; base += 64) {
    bool candidate = false;
    if (base + lane < n_boxes) {
      const SliceBoxDev& b = boxes[base + lane];
      // [min, max) against the closed tile box [lo, hi]
      // (& not &&: the six corners are loaded together, not one after the other's compare)
      candidate = (b.minc[0] <= hi[0]) & (lo[0] < b.maxc[0]) & (b.minc[1] <= hi[1]) &
                  (lo[1] < b.maxc[1]) & (b.minc[2] <= hi[2]) & (lo[2] < b.maxc[2]);
    }
    unsigned long long pending = __builtin_amdgcn_ballot_w64(candidate);
    while (pending != 0) {
      const int position = base + __builtin_ctzll(pending);
      pending &= pending - 1;
      const SliceBoxDev& b = boxes[position];  // wave-uniform address
      const bool inside = (b.minc[0] <= p[0]) & (p[0] < b.maxc[0]) & (b.minc[1] <= p[1]) &
                          (p[1] < b.maxc[1]) & (b.minc[2] <= p[2]) & (p[2] < b.maxc[2]);
      if (!done && inside) {
        found = position;
        done = true;
      }
    }
    if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
  }
  if (!in_image) return;

  double v = 0.0;
  int lvl = -1, global = -1;
  if (found >= 0) {
    const SliceBoxDev& b = boxes[found];
    // i = min(int(floor((p - min) / (max - min) * n)), n - 1); p >= min, so i >= 0
    uint32_t cell[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double q = (p[a] - b.minc[a]) / (b.maxc[a] - b.minc[a]) * static_cast<double>(b.n[a]);
      const double top = static_cast<double>(b.n[a] - 1);
      const double f = floor(q);
      cell[a] = static_cast<uint32_t>(static_cast<int>((f < top) ? f : top));
    }
    const double __attribute__((address_space(1)))* cells =
        (const double __attribute__((address_space(1)))*)b.cells;
    v = cells[cell[0] + cell[1] * static_cast<uint32_t>(b.jstride) +
              cell[2] * static_cast<uint32_t>(b.kstride)];
    lvl = b.level;
    global = b.global_index;
  }
  const int64_t pixel = static_cast<int64_t>(y) * width + x;
  value[pixel] = v;
  level[pixel] = static_cast<int8_t>(lvl);
  box_index[pixel] = global;
}

// box: width x height, row 0 at the bottom; rgb8: rows top-down.  A pixel whose box differs from
// that of its right or upper neighbour gets (red, green, blue); the last column has no right
// neighbour and the top row no upper one.
__global__ __launch_bounds__(256) void slice_outline_kernel(const int32_t* __restrict__ box,
                                                            const int width, const int height,
                                                            const uint8_t red, const uint8_t green,
                                                            const uint8_t blue,
                                                            uint8_t* __restrict__ rgb8) {
  const int64_t n = static_cast<int64_t>(width) * height;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; p < n;
       p += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t y = p / width;
    const int64_t x = p - y * width;
    const int32_t mine = box[p];
    const bool edge = (x + 1 < width && box[p + 1] != mine) ||
                      (y + 1 < height && box[p + width] != mine);
    if (edge) {
      uint8_t* d = rgb8 + ((height - 1 - y) * width + x) * 3;
      d[0] = red;
      d[1] = green;
      d[2] = blue;
    }
  }
}

int check(const char* what) {
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string(what) + ": " + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

}  // namespace

int launch_slice(const SlicePlaneDev& plane, int width, int height, const SliceBoxDev* boxes_dev,
                 int n_boxes, double* value, int8_t* level, int32_t* box_index, void* stream_v) {
  const int span = 2 * kSliceTile;
  const dim3 grid(static_cast<unsigned>((width + span - 1) / span),
                  static_cast<unsigned>((height + span - 1) / span));
  hipLaunchKernelGGL(slice_kernel, grid, dim3(kSliceThreads), 0,
                     static_cast<hipStream_t>(stream_v), plane, width, height, boxes_dev, n_boxes,
                     value, level, box_index);
  return check("slice_kernel");
}

int launch_slice_outline(const int32_t* box_index, int width, int height, int red, int green,
                         int blue, uint8_t* rgb8, void* stream_v) {
  const int64_t n = static_cast<int64_t>(width) * height;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(slice_outline_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_v), box_index, width, height,
                     static_cast<uint8_t>(red), static_cast<uint8_t>(green),
                     static_cast<uint8_t>(blue), rgb8);
  return check("slice_outline_kernel");
}

}  // namespace avr
