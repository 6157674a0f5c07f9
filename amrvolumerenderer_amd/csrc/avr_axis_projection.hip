// On-axis projections of the raw AMR field with an optional weight field ("On-axis
// projection"): per pixel the line integral along x, y or z through every box that contains the
// pixel's line, cell by cell -- a cell's path length is its level's cell size.
//
//   axis_reduce_columns_kernel<AXIS, W>  stage 1, axes y and z: a lane owns two columns
//   axis_reduce_rows_kernel<W>           stage 1, axis x: 16 lanes share a row segment
//   axis_gather_kernel                   stage 2: a pixel adds the planes of the boxes on its line
//
// Stage 1 reads every cell once and writes, per box and per segment of kAxisSegment cells along
// the axis, the partial planes S = sum of vf (of vf * vw with a weight), Wt = sum of vw and n = the
// number of cells that count, shaped [dims_V][dims_U].  A cell counts when vf (and vw) is finite.
// Rows are read coalesced along x on all three axes, as f64 pairs where the host found both fields
// 16-byte aligned with even strides; the pairing changes the width of a load, never which cells a
// lane adds or in which order:
//   y, z  a lane adds its column's cells in ascending index along the axis;
//   x     lane l of the row's 16 adds the cells 2l + 32m + {0, 1}, m = 0..3, of the segment in
//         ascending order, then the 16 partial sums are added by a butterfly over lane distances
//         8, 4, 2, 1 (f64 addition commutes, so every lane ends with the same bits).
// Stage 2 adds a box's segments in ascending order, multiplies by the level's path length and adds
// the boxes in ascending box index.  No atomic touches an output: the result is a fixed function
// of the arguments.  All arithmetic is IEEE binary64, nothing fused (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_cell_tiles.h"
#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 128;      // y, z: cells along x of a tile (two per lane)
constexpr int kOuterBlock = 4;   // y, z: one wave per index on the axis that is neither x nor the axis
constexpr int kRowsJ = 16;       // x: rows along y of a tile (four per wave)
constexpr int kRowsK = 4;        // x: planes along z of a tile
constexpr int kGatherTile = 8;   // pixels per side of a wave's tile

typedef const double __attribute__((address_space(1))) const_global_double;
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef const double2_t __attribute__((address_space(1))) const_global_double2;

template <bool W>
__device__ __forceinline__ void add_cell(double vf, double vw, double& s, double& w, uint32_t& n) {
  bool counts = __builtin_isfinite(vf);
  if (W) counts = counts & __builtin_isfinite(vw);
  if (counts) {
    s += W ? vf * vw : vf;
    if (W) w += vw;
    n += 1u;
  }
}

// How a lane reads its two columns
enum Load { kPair, kTwo, kOne };

// The cells [0, count) along the axis of the lane's columns, ascending; `second` = distance of the
// second column from the first (kTwo).
template <bool W, int LOAD>
__device__ __forceinline__ void add_columns(const_global_double* f, const_global_double* w,
                                            uint32_t stride_f, uint32_t stride_w, int count,
                                            uint32_t second, double s[2], double wt[2],
                                            uint32_t n[2]) {
#pragma unroll 8
  for (int r = 0; r < count; ++r) {
    const_global_double* pf = f + static_cast<uint32_t>(r) * stride_f;
    const_global_double* pw = w + static_cast<uint32_t>(r) * stride_w;
    if (LOAD == kPair) {
      const double2_t vf = *(const_global_double2*)pf;
      double2_t vw = {0.0, 0.0};
      if (W) vw = *(const_global_double2*)pw;
      add_cell<W>(vf.x, vw.x, s[0], wt[0], n[0]);
      add_cell<W>(vf.y, vw.y, s[1], wt[1], n[1]);
    } else {
      add_cell<W>(pf[0], W ? pw[0] : 0.0, s[0], wt[0], n[0]);
      if (LOAD == kTwo) add_cell<W>(pf[second], W ? pw[second] : 0.0, s[1], wt[1], n[1]);
    }
  }
}

// AXIS 1 (y) or 2 (z).  One tile = one segment x kOuterBlock outer indices x kChunk cells along x.
template <int AXIS, bool W>
__global__ __launch_bounds__(kThreads) void axis_reduce_columns_kernel(const AxisReduceArgs a) {
  const uint32_t tile = blockIdx.x;
  const int b = locate_box(a.tile_begin, a.n_boxes, tile);
  const AxisBoxDev& box = a.boxes[b];
  const int nx = box.nx;
  const int n_axis = AXIS == 2 ? box.nz : box.ny;
  const int n_outer = AXIS == 2 ? box.ny : box.nz;
  const uint32_t chunks = static_cast<uint32_t>((nx + kChunk - 1) / kChunk);
  const uint32_t blocks = static_cast<uint32_t>((n_outer + kOuterBlock - 1) / kOuterBlock);
  uint32_t local = tile - a.tile_begin[b];
  const int chunk = static_cast<int>(local % chunks);
  local /= chunks;
  const int block = static_cast<int>(local % blocks);
  const int segment = static_cast<int>(local / blocks);

  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int wave = static_cast<int>(threadIdx.x) >> 6;
  const int outer = block * kOuterBlock + wave;
  if (outer >= n_outer) return;
  const bool paired = box.paired != 0;
  const int i0 = chunk * kChunk + (paired ? 2 * lane : lane);
  const int i1 = paired ? i0 + 1 : i0 + 64;
  if (i0 >= nx) return;
  const int first = segment * kAxisSegment;
  const int count = (n_axis - first < kAxisSegment) ? n_axis - first : kAxisSegment;

  const uint32_t axis_f = static_cast<uint32_t>(AXIS == 2 ? box.kstride_f : box.jstride_f);
  const uint32_t outer_f = static_cast<uint32_t>(AXIS == 2 ? box.jstride_f : box.kstride_f);
  const uint32_t axis_w = static_cast<uint32_t>(AXIS == 2 ? box.kstride_w : box.jstride_w);
  const uint32_t outer_w = static_cast<uint32_t>(AXIS == 2 ? box.jstride_w : box.kstride_w);
  const_global_double* f = (const_global_double*)box.cells_f + static_cast<uint32_t>(i0) +
                           static_cast<uint32_t>(outer) * outer_f +
                           static_cast<uint32_t>(first) * axis_f;
  const_global_double* w = (const_global_double*)box.cells_w + static_cast<uint32_t>(i0) +
                           static_cast<uint32_t>(outer) * outer_w +
                           static_cast<uint32_t>(first) * axis_w;
  double s[2] = {0.0, 0.0}, wt[2] = {0.0, 0.0};
  uint32_t n[2] = {0u, 0u};
  if (i1 >= nx) {
    add_columns<W, kOne>(f, w, axis_f, axis_w, count, 0u, s, wt, n);
  } else if (paired) {
    add_columns<W, kPair>(f, w, axis_f, axis_w, count, 0u, s, wt, n);
  } else {
    add_columns<W, kTwo>(f, w, axis_f, axis_w, count, 64u, s, wt, n);
  }

  // z: plane[j][i]; y: plane[i][k]
  const uint32_t plane = static_cast<uint32_t>(nx) * static_cast<uint32_t>(n_outer);
  const uint32_t at = box.plane_begin + static_cast<uint32_t>(segment) * plane;
  const uint32_t e0 = at + (AXIS == 2 ? static_cast<uint32_t>(outer) * static_cast<uint32_t>(nx) +
                                            static_cast<uint32_t>(i0)
                                      : static_cast<uint32_t>(i0) * static_cast<uint32_t>(n_outer) +
                                            static_cast<uint32_t>(outer));
  a.plane_s[e0] = s[0];
  if (W) a.plane_w[e0] = wt[0];
  a.plane_n[e0] = n[0];
  if (i1 < nx) {
    const uint32_t e1 = at + (AXIS == 2 ? static_cast<uint32_t>(outer) * static_cast<uint32_t>(nx) +
                                              static_cast<uint32_t>(i1)
                                        : static_cast<uint32_t>(i1) * static_cast<uint32_t>(n_outer) +
                                              static_cast<uint32_t>(outer));
    a.plane_s[e1] = s[1];
    if (W) a.plane_w[e1] = wt[1];
    a.plane_n[e1] = n[1];
  }
}

// Axis x.  One tile = one segment x kRowsK planes x kRowsJ rows; 16 lanes share a row's segment.
template <bool W>
__global__ __launch_bounds__(kThreads) void axis_reduce_rows_kernel(const AxisReduceArgs a) {
  const uint32_t tile = blockIdx.x;
  const int b = locate_box(a.tile_begin, a.n_boxes, tile);
  const AxisBoxDev& box = a.boxes[b];
  const int nx = box.nx, ny = box.ny, nz = box.nz;
  const uint32_t blocks_j = static_cast<uint32_t>((ny + kRowsJ - 1) / kRowsJ);
  const uint32_t blocks_k = static_cast<uint32_t>((nz + kRowsK - 1) / kRowsK);
  uint32_t local = tile - a.tile_begin[b];
  const int block_j = static_cast<int>(local % blocks_j);
  local /= blocks_j;
  const int block_k = static_cast<int>(local % blocks_k);
  const int segment = static_cast<int>(local / blocks_k);

  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int wave = static_cast<int>(threadIdx.x) >> 6;
  const int j = block_j * kRowsJ + wave * 4 + (lane >> 4);
  const int i_first = segment * kAxisSegment + 2 * (lane & 15);
  const bool paired = box.paired != 0;
  const uint32_t row_f = static_cast<uint32_t>(j) * static_cast<uint32_t>(box.jstride_f);
  const uint32_t row_w = static_cast<uint32_t>(j) * static_cast<uint32_t>(box.jstride_w);
  const_global_double* cells_f = (const_global_double*)box.cells_f;
  const_global_double* cells_w = (const_global_double*)box.cells_w;

  double s[kRowsK], wt[kRowsK];
  uint32_t n[kRowsK];
#pragma unroll
  for (int kk = 0; kk < kRowsK; ++kk) {
    const int k = block_k * kRowsK + kk;
    s[kk] = 0.0;
    wt[kk] = 0.0;
    n[kk] = 0u;
    if (j < ny && k < nz) {
      const_global_double* f = cells_f + row_f + static_cast<uint32_t>(k) * static_cast<uint32_t>(box.kstride_f);
      const_global_double* w = cells_w + row_w + static_cast<uint32_t>(k) * static_cast<uint32_t>(box.kstride_w);
#pragma unroll
      for (int m = 0; m < kAxisSegment / 32; ++m) {
        const int i = i_first + 32 * m;
        if (i + 1 < nx) {
          double f0, f1, w0 = 0.0, w1 = 0.0;
          if (paired) {
            const double2_t vf = *(const_global_double2*)(f + i);
            f0 = vf.x;
            f1 = vf.y;
            if (W) {
              const double2_t vw = *(const_global_double2*)(w + i);
              w0 = vw.x;
              w1 = vw.y;
            }
          } else {
            f0 = f[i];
            f1 = f[i + 1];
            if (W) {
              w0 = w[i];
              w1 = w[i + 1];
            }
          }
          add_cell<W>(f0, w0, s[kk], wt[kk], n[kk]);
          add_cell<W>(f1, w1, s[kk], wt[kk], n[kk]);
        } else if (i < nx) {
          add_cell<W>(f[i], W ? w[i] : 0.0, s[kk], wt[kk], n[kk]);
        }
      }
    }
  }
  // every lane takes part in the butterflies, whether its row exists or not
#pragma unroll
  for (int kk = 0; kk < kRowsK; ++kk) {
#pragma unroll
    for (int mask = 8; mask > 0; mask >>= 1) {
      s[kk] += __shfl_xor(s[kk], mask, 64);
      if (W) wt[kk] += __shfl_xor(wt[kk], mask, 64);
      n[kk] += __shfl_xor(n[kk], mask, 64);
    }
  }
  if ((lane & 15) != 0 || j >= ny) return;
  // plane[k][j]
  const uint32_t plane = static_cast<uint32_t>(ny) * static_cast<uint32_t>(nz);
  const uint32_t at = box.plane_begin + static_cast<uint32_t>(segment) * plane;
#pragma unroll
  for (int kk = 0; kk < kRowsK; ++kk) {
    const int k = block_k * kRowsK + kk;
    if (k < nz) {
      const uint32_t e = at + static_cast<uint32_t>(k) * static_cast<uint32_t>(ny) +
                         static_cast<uint32_t>(j);
      a.plane_s[e] = s[kk];
      if (W) a.plane_w[e] = wt[kk];
      a.plane_n[e] = n[kk];
    }
  }
}

// One lane owns a pixel, one wave an 8 x 8 pixel tile; the boxes are tested 64 at a time against
// the tile's (u, v) rectangle, as slice_kernel does in three dimensions.  u and v are monotone in
// x and y, roundings included, so a tile's lines lie in the rectangle of its corner pixels.
__global__ __launch_bounds__(kThreads) void axis_gather_kernel(const AxisGatherArgs a) {
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int tile_x0 = (static_cast<int>(blockIdx.x) * 2 + (wave & 1)) * kGatherTile;
  const int tile_y0 = (static_cast<int>(blockIdx.y) * 2 + (wave >> 1)) * kGatherTile;
  if (tile_x0 >= a.width || tile_y0 >= a.height) return;  // wave-uniform
  const int x = tile_x0 + (lane & (kGatherTile - 1));
  const int y = tile_y0 + (lane >> 3);
  const bool in_image = x < a.width && y < a.height;

  const double u = a.origin_u + (static_cast<double>(x) + 0.5) * a.du;
  const double v = a.origin_v + (static_cast<double>(y) + 0.5) * a.dv;
  double lo_u, hi_u, lo_v, hi_v;
  {
    const double u0 = a.origin_u + (static_cast<double>(tile_x0) + 0.5) * a.du;
    const double u1 = a.origin_u + (static_cast<double>(tile_x0 + (kGatherTile - 1)) + 0.5) * a.du;
    const double v0 = a.origin_v + (static_cast<double>(tile_y0) + 0.5) * a.dv;
    const double v1 = a.origin_v + (static_cast<double>(tile_y0 + (kGatherTile - 1)) + 0.5) * a.dv;
    lo_u = (u1 < u0) ? u1 : u0;
    hi_u = (u1 > u0) ? u1 : u0;
    lo_v = (v1 < v0) ? v1 : v0;
    hi_v = (v1 > v0) ? v1 : v0;
  }
  const bool weighted = a.plane_w != nullptr;

  double integral = 0.0, weight = 0.0, length = 0.0;
  for (int base = 0; base < a.n_boxes; base += 64) {
    bool candidate = false;
    if (base + lane < a.n_boxes) {
      const AxisPlaneDev& b = a.boxes[base + lane];
      // [min, max) against the closed tile rectangle [lo, hi]
      candidate = (b.min_u <= hi_u) & (lo_u < b.max_u) & (b.min_v <= hi_v) & (lo_v < b.max_v);
    }
    unsigned long long pending = __builtin_amdgcn_ballot_w64(candidate);
    while (pending != 0) {  // ascending box index
      const int position = base + __builtin_ctzll(pending);
      pending &= pending - 1;
      const AxisPlaneDev& b = a.boxes[position];  // wave-uniform address
      const bool inside = in_image & (b.min_u <= u) & (u < b.max_u) & (b.min_v <= v) & (v < b.max_v);
      if (inside) {
        // i = min(int(floor((p - min) / (max - min) * n)), n - 1); p >= min, so i >= 0
        const double qu = (u - b.min_u) / (b.max_u - b.min_u) * static_cast<double>(b.n_u);
        const double qv = (v - b.min_v) / (b.max_v - b.min_v) * static_cast<double>(b.n_v);
        const double top_u = static_cast<double>(b.n_u - 1), top_v = static_cast<double>(b.n_v - 1);
        const double fu = floor(qu), fv = floor(qv);
        const uint32_t iu = static_cast<uint32_t>(static_cast<int>((fu < top_u) ? fu : top_u));
        const uint32_t iv = static_cast<uint32_t>(static_cast<int>((fv < top_v) ? fv : top_v));
        const uint32_t plane = static_cast<uint32_t>(b.n_u) * static_cast<uint32_t>(b.n_v);
        uint32_t e = b.plane_begin + iv * static_cast<uint32_t>(b.n_u) + iu;
        double s = 0.0, w = 0.0;
        uint32_t n = 0u;
        for (int segment = 0; segment < b.segments; ++segment, e += plane) {
          s += a.plane_s[e];
          if (weighted) w += a.plane_w[e];
          n += a.plane_n[e];
        }
        integral += b.dl * s;
        weight += b.dl * w;
        length += b.dl * static_cast<double>(n);
      }
    }
  }
  if (!in_image) return;
  const int64_t pixel = static_cast<int64_t>(y) * a.width + x;
  a.integral[pixel] = integral;
  if (weighted) a.weight[pixel] = weight;
  a.length[pixel] = length;
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

uint32_t axis_projection_tiles(int axis, int nx, int ny, int nz) {
  const auto blocks = [](int n, int per) { return static_cast<uint64_t>((n + per - 1) / per); };
  uint64_t tiles;
  if (axis == 0) {
    tiles = blocks(nx, kAxisSegment) * blocks(nz, kRowsK) * blocks(ny, kRowsJ);
  } else if (axis == 1) {
    tiles = blocks(ny, kAxisSegment) * blocks(nz, kOuterBlock) * blocks(nx, kChunk);
  } else {
    tiles = blocks(nz, kAxisSegment) * blocks(ny, kOuterBlock) * blocks(nx, kChunk);
  }
  return tiles < (uint64_t{1} << 31) ? static_cast<uint32_t>(tiles) : UINT32_MAX;
}

int launch_axis_reduce(const AxisReduceArgs& args, int axis, bool weighted, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_tiles == 0) return AVR_OK;
  const dim3 grid(args.n_tiles), block(kThreads);
  if (axis == 0) {
    if (weighted) {
      hipLaunchKernelGGL(axis_reduce_rows_kernel<true>, grid, block, 0, stream, args);
    } else {
      hipLaunchKernelGGL(axis_reduce_rows_kernel<false>, grid, block, 0, stream, args);
    }
    return check("axis_reduce_rows_kernel");
  }
  if (axis == 1) {
    if (weighted) {
      hipLaunchKernelGGL((axis_reduce_columns_kernel<1, true>), grid, block, 0, stream, args);
    } else {
      hipLaunchKernelGGL((axis_reduce_columns_kernel<1, false>), grid, block, 0, stream, args);
    }
  } else {
    if (weighted) {
      hipLaunchKernelGGL((axis_reduce_columns_kernel<2, true>), grid, block, 0, stream, args);
    } else {
      hipLaunchKernelGGL((axis_reduce_columns_kernel<2, false>), grid, block, 0, stream, args);
    }
  }
  return check("axis_reduce_columns_kernel");
}

int launch_axis_gather(const AxisGatherArgs& args, void* stream_v) {
  const int span = 2 * kGatherTile;
  const dim3 grid(static_cast<unsigned>((args.width + span - 1) / span),
                  static_cast<unsigned>((args.height + span - 1) / span));
  hipLaunchKernelGGL(axis_gather_kernel, grid, dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream_v), args);
  return check("axis_gather_kernel");
}

}  // namespace avr
