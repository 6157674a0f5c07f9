// Velocity cubes ("Velocity cubes"): the on-axis projection of an emission field e
// split into channels of a bin field g ("velocity"), a cell's share optionally spread over the
// channels by a Gaussian of the cell's width s.
//
//   cube_reduce_columns_kernel<AXIS, S>  stage 1, axes y and z: a lane owns two columns
//   cube_reduce_rows_kernel<S>           stage 1, axis x: slabs staged through LDS, a lane owns a row
//   cube_gather_kernel                   stage 2: a pixel adds the planes of the boxes on its line
//
// The tiles, the segments of kAxisSegment cells, the rows read coalesced along x (as f64 pairs where
// the host found every field 16-byte aligned with even strides) and the entries of the partial
// planes are the on-axis projection's (avr_axis_projection.hip).  What is new is that the
// accumulator a cell adds to is chosen by the cell's g: a workgroup keeps the accumulators of its
// columns in LDS, laid out [channel][column] -- the lanes of a wave hit consecutive banks whatever
// channels their cells chose -- for one chunk of `chunk` channels (the grid's y index) plus under
// and over.  Only the lane that owns a column adds to its accumulators, in ascending cell order, so
// no atomic is needed and the bits do not depend on the launch.  For axis x the 16 cells x 64 rows
// of a slab are read coalesced by the whole workgroup into LDS (rows padded to 17 entries) and the
// first wave's lanes each walk one row of it: no lane walks a row of global memory by itself.
//
// Per cell, with e, g (and s) as read:
//   counts:   e and g finite (S: and s finite and >= 0); other cells add nothing, not even to n
//   sharp     (no s, or s == 0): e goes to the channel c with edges[c] <= g < edges[c + 1], the last
//             channel closed at the top -- f64 comparisons against the edges in LDS, the joint
//             histogram's search (a linear guess, a gallop, a binary search; the guess never
//             decides); g < edges[0] adds e to under, g > edges[nc] to over
//   broadened (s > 0): a_j = ((edges[j] - g) / s) * 0.70710678118654752440, q_j = -1 if a_j <= -6,
//             +1 if a_j >= 6, else erf(a_j); channel c gets e * (0.5 * (q_(c+1) - q_c)), under
//             e * (0.5 * (q_0 + 1)), over e * (0.5 * (1 - q_nc)).  a_j does not decrease with j, so a
//             chunk whose last edge has a <= -6 or whose first has a >= 6 gets only e * 0 terms,
//             which change no accumulator (none is ever -0), and is skipped; within a chunk every
//             q is evaluated once and serves the two channels it bounds.
// Stage 2 adds a box's segments in ascending order, multiplies by the level's path length and adds
// the boxes in ascending box index.  All arithmetic is IEEE binary64, nothing fused
// (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_cell_tiles.h"
#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
// the on-axis projection's tiles (axis_projection_tiles counts them):
constexpr int kChunk = 128;      // y, z: cells along x of a tile (two per lane)
constexpr int kOuterBlock = 4;   // y, z: one wave per index on the axis that is neither x nor the axis
constexpr int kRowsJ = 16;       // x: rows along y of a tile
constexpr int kRowsK = 4;        // x: planes along z of a tile
constexpr int kGatherTile = 8;   // pixels per side of a wave's tile
constexpr int kColumnsYZ = kOuterBlock * kChunk;  // columns of a tile, y and z
constexpr int kColumnsX = kRowsJ * kRowsK;        // ... and x
constexpr int kSlab = 16;                         // x: cells of a row staged at a time
constexpr int kSlabPitch = kSlab + 1;             // ... and the row's pitch in LDS: no bank shared
static_assert(kColumnsX == kCubeColumns[0] && kColumnsYZ == kCubeColumns[1] &&
                  kColumnsYZ == kCubeColumns[2], "the host sizes the LDS by these");
static_assert(kColumnsX == 64, "the first wave owns the rows of a tile");
static_assert(kColumnsX * kSlab == 4 * kThreads, "a lane stages four cells of a slab");
static_assert(kAxisSegment % kSlab == 0, "a segment is whole slabs");

typedef double __attribute__((address_space(3))) lds_double;
typedef const double __attribute__((address_space(1))) const_global_double;
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef const double2_t __attribute__((address_space(1))) const_global_double2;

// The bin of v among the n + 1 edges e (LDS), given e[0] <= v <= e[n]: the largest i in
// [0, n - 1] with e[i] <= v.  `lo` and `scale` only choose the first edge looked at.  The joint
// histogram's search (avr_joint_histogram.hip), restated here so that file stays as it is.
__device__ __forceinline__ int find_bin(const lds_double* e, int n, double lo, double scale,
                                        double v) {
  double q = (v - lo) * scale;
  q = (q < 0.0) ? 0.0 : q;
  const double top = static_cast<double>(n - 1);
  const int guess = (q < top) ? static_cast<int>(q) : n - 1;  // a NaN q lands on n - 1
  // invariant: e[first] <= v and (last == n or v < e[last])
  int first, last;
  if (v < e[guess]) {  // guess > 0 here, because e[0] <= v
    last = guess;
    int step = 1;
    for (;;) {
      const int probe = last - step;
      if (probe <= 0) {
        first = 0;
        break;
      }
      if (e[probe] <= v) {
        first = probe;
        break;
      }
      last = probe;
      step <<= 1;
    }
  } else {
    first = guess;
    int step = 1;
    for (;;) {
      const int probe = first + step;
      if (probe >= n) {
        last = n;
        break;
      }
      if (v < e[probe]) {
        last = probe;
        break;
      }
      first = probe;
      step <<= 1;
    }
  }
  while (last - first > 1) {
    const int mid = (first + last) >> 1;
    if (e[mid] <= v) {
      first = mid;
    } else {
      last = mid;
    }
  }
  return first;
}

// What a workgroup works on, the same for all of its lanes.
struct Chunk {
  const lds_double* edges;  // n_channels + 1
  int n_channels;
  int first, count;         // the chunk's channels
  bool totals;              // under and over are this workgroup's too
  double lo, hi, scale;
};

__device__ __forceinline__ double argument(const Chunk& c, int j, double g, double s) {
  return ((c.edges[j] - g) / s) * 0.70710678118654752440;
}
__device__ __forceinline__ double clamped_erf(double a) {
  return (a <= -6.0) ? -1.0 : (a >= 6.0) ? 1.0 : erf(a);
}
__device__ __forceinline__ double profile(const Chunk& c, int j, double g, double s) {
  return clamped_erf(argument(c, j, g, s));
}

// One cell of the column whose accumulators are acc[channel * COLUMNS], channel = 0 .. count - 1,
// then under and over.  Returns whether the cell counts.
template <bool S, int COLUMNS>
__device__ __forceinline__ bool add_cell(const Chunk& c, double e, double g, double s,
                                         lds_double* acc) {
  bool counts = __builtin_isfinite(e) & __builtin_isfinite(g);
  if (S) counts = counts & __builtin_isfinite(s) & (s >= 0.0);
  if (!counts) return false;
  if (!S || s == 0.0) {
    if (g < c.lo) {
      if (c.totals) acc[c.count * COLUMNS] += e;
    } else if (g > c.hi) {
      if (c.totals) acc[(c.count + 1) * COLUMNS] += e;
    } else {
      const int at = find_bin(c.edges, c.n_channels, c.lo, c.scale, g) - c.first;
      if (at >= 0 && at < c.count) acc[at * COLUMNS] += e;
    }
    return true;
  }
  if (c.totals) {
    acc[c.count * COLUMNS] += e * (0.5 * (profile(c, 0, g, s) + 1.0));
    acc[(c.count + 1) * COLUMNS] += e * (0.5 * (1.0 - profile(c, c.n_channels, g, s)));
  }
  // a does not decrease with j: every q of the chunk is +1, or every q is -1
  const double a_first = argument(c, c.first, g, s);
  if (a_first >= 6.0) return true;
  const double a_last = argument(c, c.first + c.count, g, s);
  if (a_last <= -6.0) return true;
  double below = clamped_erf(a_first);
  for (int at = 0; at < c.count; ++at) {
    const double above = profile(c, c.first + at + 1, g, s);
    acc[at * COLUMNS] += e * (0.5 * (above - below));
    below = above;
  }
  return true;
}

__device__ __forceinline__ Chunk load_chunk(const CubeReduceArgs& a, lds_double* lds) {
  for (int i = static_cast<int>(threadIdx.x); i <= a.n_channels; i += kThreads) lds[i] = a.edges[i];
  __syncthreads();
  Chunk c;
  c.edges = lds;
  c.n_channels = a.n_channels;
  c.first = a.channel_first + static_cast<int>(blockIdx.y) * a.chunk;
  const int left = a.channel_first + a.channel_count - c.first;
  c.count = left < a.chunk ? left : a.chunk;
  c.totals = a.totals != 0 && blockIdx.y == 0;
  c.lo = a.lo;
  c.hi = a.hi;
  c.scale = a.scale;
  return c;
}

// The column's accumulators -> entry `e` of the chunk's partial planes (and of under, over and n).
template <int COLUMNS>
__device__ __forceinline__ void write_column(const CubeReduceArgs& a, const Chunk& c,
                                             const lds_double* acc, uint32_t n, uint32_t e) {
  const size_t entries = a.entries;
  double* plane = a.planes + static_cast<size_t>(c.first - a.channel_first) * entries + e;
  for (int at = 0; at < c.count; ++at) plane[static_cast<size_t>(at) * entries] = acc[at * COLUMNS];
  if (c.totals) {
    a.under[e] = acc[c.count * COLUMNS];
    a.over[e] = acc[(c.count + 1) * COLUMNS];
    a.plane_n[e] = n;
  }
}

// AXIS 1 (y) or 2 (z).  One tile = one segment x kOuterBlock outer indices x kChunk cells along x.
template <int AXIS, bool S>
__global__ __launch_bounds__(kThreads) void cube_reduce_columns_kernel(const CubeReduceArgs a) {
  extern __shared__ double cube_lds[];  // [edges: nc + 1][accumulators: (chunk + 2) x kColumnsYZ]
  const Chunk c = load_chunk(a, (lds_double*)cube_lds);
  const uint32_t tile = blockIdx.x;
  const int b = locate_box(a.tile_begin, a.n_boxes, tile);
  const CubeBoxDev& box = a.boxes[b];
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
  if (outer >= n_outer) return;  // after the workgroup's only barrier
  const bool paired = box.paired != 0;
  const int i0 = chunk * kChunk + (paired ? 2 * lane : lane);
  const int i1 = paired ? i0 + 1 : i0 + 64;
  if (i0 >= nx) return;
  const bool second = i1 < nx;
  const bool pair = paired & second;
  const uint32_t step = paired ? 1u : 64u;
  const int first = segment * kAxisSegment;
  const int count = (n_axis - first < kAxisSegment) ? n_axis - first : kAxisSegment;

  const_global_double* cells[3];
  uint32_t stride[3];
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const uint32_t along = static_cast<uint32_t>(AXIS == 2 ? box.kstride[f] : box.jstride[f]);
    const uint32_t across = static_cast<uint32_t>(AXIS == 2 ? box.jstride[f] : box.kstride[f]);
    stride[f] = along;
    cells[f] = (const_global_double*)box.cells[f] + static_cast<uint32_t>(i0) +
               static_cast<uint32_t>(outer) * across + static_cast<uint32_t>(first) * along;
  }
  // the lane's two columns: consecutive lanes, consecutive banks
  lds_double* acc = (lds_double*)cube_lds + (a.n_channels + 1) + wave * kChunk + lane;
  for (int at = 0; at < c.count + 2; ++at) {
    acc[at * kColumnsYZ] = 0.0;
    acc[at * kColumnsYZ + 64] = 0.0;
  }
  uint32_t n0 = 0u, n1 = 0u;
  for (int r = 0; r < count; ++r) {
    const_global_double* pe = cells[0] + static_cast<uint32_t>(r) * stride[0];
    const_global_double* pg = cells[1] + static_cast<uint32_t>(r) * stride[1];
    const_global_double* ps = cells[2] + static_cast<uint32_t>(r) * stride[2];
    double e[2], g[2], s[2] = {0.0, 0.0};
    if (pair) {
      const double2_t ve = *(const_global_double2*)pe;
      const double2_t vg = *(const_global_double2*)pg;
      e[0] = ve.x, e[1] = ve.y, g[0] = vg.x, g[1] = vg.y;
      if (S) {
        const double2_t vs = *(const_global_double2*)ps;
        s[0] = vs.x, s[1] = vs.y;
      }
    } else {
      e[0] = pe[0], g[0] = pg[0];
      if (S) s[0] = ps[0];
      e[1] = second ? pe[step] : 0.0, g[1] = second ? pg[step] : 0.0;
      if (S) s[1] = second ? ps[step] : 0.0;
    }
    if (add_cell<S, kColumnsYZ>(c, e[0], g[0], s[0], acc)) n0 += 1u;
    if (second && add_cell<S, kColumnsYZ>(c, e[1], g[1], s[1], acc + 64)) n1 += 1u;
  }

  // z: plane[j][i]; y: plane[i][k]
  const uint32_t plane = static_cast<uint32_t>(nx) * static_cast<uint32_t>(n_outer);
  const uint32_t at = box.plane_begin + static_cast<uint32_t>(segment) * plane;
  const uint32_t e0 = at + (AXIS == 2 ? static_cast<uint32_t>(outer) * static_cast<uint32_t>(nx) +
                                            static_cast<uint32_t>(i0)
                                      : static_cast<uint32_t>(i0) * static_cast<uint32_t>(n_outer) +
                                            static_cast<uint32_t>(outer));
  write_column<kColumnsYZ>(a, c, acc, n0, e0);
  if (second) {
    const uint32_t e1 = at + (AXIS == 2 ? static_cast<uint32_t>(outer) * static_cast<uint32_t>(nx) +
                                              static_cast<uint32_t>(i1)
                                        : static_cast<uint32_t>(i1) * static_cast<uint32_t>(n_outer) +
                                              static_cast<uint32_t>(outer));
    write_column<kColumnsYZ>(a, c, acc + 64, n1, e1);
  }
}

// Axis x.  One tile = one segment x kRowsK planes x kRowsJ rows: 64 rows of up to 128 cells, staged
// a slab of kSlab cells at a time.  Row r of the tile is (j, k) = (16 block_j + (r & 15),
// 4 block_k + (r >> 4)).
template <bool S>
__global__ __launch_bounds__(kThreads) void cube_reduce_rows_kernel(const CubeReduceArgs a) {
  // [edges: nc + 1][accumulators: (chunk + 2) x 64][slab: 3 fields x 64 rows x kSlabPitch]
  extern __shared__ double cube_lds[];
  const Chunk c = load_chunk(a, (lds_double*)cube_lds);
  const uint32_t tile = blockIdx.x;
  const int b = locate_box(a.tile_begin, a.n_boxes, tile);
  const CubeBoxDev& box = a.boxes[b];
  const int nx = box.nx, ny = box.ny, nz = box.nz;
  const uint32_t blocks_j = static_cast<uint32_t>((ny + kRowsJ - 1) / kRowsJ);
  const uint32_t blocks_k = static_cast<uint32_t>((nz + kRowsK - 1) / kRowsK);
  uint32_t local = tile - a.tile_begin[b];
  const int block_j = static_cast<int>(local % blocks_j);
  local /= blocks_j;
  const int block_k = static_cast<int>(local % blocks_k);
  const int segment = static_cast<int>(local / blocks_k);
  const int first = segment * kAxisSegment;
  const int count = (nx - first < kAxisSegment) ? nx - first : kAxisSegment;
  const bool paired = box.paired != 0;

  const int t = static_cast<int>(threadIdx.x);
  lds_double* acc = (lds_double*)cube_lds + (a.n_channels + 1) + (t & 63);
  lds_double* slab = (lds_double*)cube_lds + (a.n_channels + 1) + (a.chunk + 2) * kColumnsX;
  constexpr int kField = kColumnsX * kSlabPitch;
  if (t < kColumnsX) {
    for (int at = 0; at < c.count + 2; ++at) acc[at * kColumnsX] = 0.0;
  }
  // staging: 8 lanes share a row's slab, two cells each, two rows per lane
  const int stage_i = 2 * (t & 7);
  // walking: lane t < 64 owns row t
  const int own_j = block_j * kRowsJ + (t & 15), own_k = block_k * kRowsK + ((t >> 4) & 3);
  const bool owner = t < kColumnsX && own_j < ny && own_k < nz;
  uint32_t n = 0u;
  for (int begin = 0; begin < count; begin += kSlab) {
    const int cells = (count - begin < kSlab) ? count - begin : kSlab;
    __syncthreads();  // the slab before this one has been walked
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int row = pass * 32 + (t >> 3);  // 8 consecutive lanes read 128 bytes of a row
      const int j = block_j * kRowsJ + (row & 15), k = block_k * kRowsK + (row >> 4);
      if (j < ny && k < nz && stage_i < cells) {
        const uint32_t i = static_cast<uint32_t>(first + begin + stage_i);
        const bool both = stage_i + 1 < cells;
#pragma unroll
        for (int f = 0; f < (S ? 3 : 2); ++f) {
          const_global_double* p = (const_global_double*)box.cells[f] + i +
                                   static_cast<uint32_t>(j) * static_cast<uint32_t>(box.jstride[f]) +
                                   static_cast<uint32_t>(k) * static_cast<uint32_t>(box.kstride[f]);
          lds_double* to = slab + f * kField + row * kSlabPitch + stage_i;
          if (paired && both) {  // first + begin + stage_i is even
            const double2_t v = *(const_global_double2*)p;
            to[0] = v.x;
            to[1] = v.y;
          } else {
            to[0] = p[0];
            if (both) to[1] = p[1];
          }
        }
      }
    }
    __syncthreads();
    if (owner) {
      const lds_double* row = slab + t * kSlabPitch;
      for (int i = 0; i < cells; ++i) {
        if (add_cell<S, kColumnsX>(c, row[i], row[kField + i], S ? row[2 * kField + i] : 0.0, acc)) {
          n += 1u;
        }
      }
    }
  }
  if (!owner) return;
  // plane[k][j]
  const uint32_t plane = static_cast<uint32_t>(ny) * static_cast<uint32_t>(nz);
  const uint32_t e = box.plane_begin + static_cast<uint32_t>(segment) * plane +
                     static_cast<uint32_t>(own_k) * static_cast<uint32_t>(ny) +
                     static_cast<uint32_t>(own_j);
  write_column<kColumnsX>(a, c, acc, n, e);
}

// axis_gather_kernel's pixel tiles and box test (avr_axis_projection.hip): one lane owns a pixel,
// one wave an 8 x 8 pixel tile, the boxes are tested 64 at a time against the tile's rectangle.
// The lane loops over the batch's channels and, with totals, over under, over and n.
__global__ __launch_bounds__(kThreads) void cube_gather_kernel(const CubeGatherArgs a) {
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
  const int64_t pixels = static_cast<int64_t>(a.width) * a.height;
  const int64_t pixel = static_cast<int64_t>(y) * a.width + x;
  // what = 0 .. channel_count - 1: a channel; then under, over, n
  const int n_what = a.channel_count + (a.totals != 0 ? 3 : 0);
  for (int what = 0; what < n_what; ++what) {  // wave-uniform
    const int total = what - a.channel_count;
    const double* planes = total < 0 ? a.planes + static_cast<size_t>(what) * a.entries
                           : total == 0 ? a.plane_under : a.plane_over;
    double sum = 0.0;
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
          if (total == 2) {
            uint32_t n = 0u;
            for (int segment = 0; segment < b.segments; ++segment, e += plane) n += a.plane_n[e];
            sum += b.dl * static_cast<double>(n);
          } else {
            double s = 0.0;
            for (int segment = 0; segment < b.segments; ++segment, e += plane) s += planes[e];
            sum += b.dl * s;
          }
        }
      }
    }
    if (in_image) {
      double* out = total < 0    ? a.cube + static_cast<int64_t>(a.channel_first + what) * pixels
                    : total == 0 ? a.under
                    : total == 1 ? a.over
                                 : a.length;
      out[pixel] = sum;
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

size_t velocity_cube_lds_bytes(int axis, int n_channels, int chunk) {
  size_t doubles = static_cast<size_t>(n_channels + 1) +
                   static_cast<size_t>(chunk + 2) * static_cast<size_t>(kCubeColumns[axis]);
  if (axis == 0) doubles += 3u * kColumnsX * kSlabPitch;
  return doubles * sizeof(double);
}

int launch_cube_reduce(const CubeReduceArgs& args, int axis, bool broadened, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_tiles == 0) return AVR_OK;
  const uint32_t chunks = static_cast<uint32_t>((args.channel_count + args.chunk - 1) / args.chunk);
  const dim3 grid(args.n_tiles, chunks), block(kThreads);
  const size_t bytes = velocity_cube_lds_bytes(axis, args.n_channels, args.chunk);
  if (axis == 0) {
    if (broadened) {
      hipLaunchKernelGGL(cube_reduce_rows_kernel<true>, grid, block, bytes, stream, args);
    } else {
      hipLaunchKernelGGL(cube_reduce_rows_kernel<false>, grid, block, bytes, stream, args);
    }
    return check("cube_reduce_rows_kernel");
  }
  if (axis == 1) {
    if (broadened) {
      hipLaunchKernelGGL((cube_reduce_columns_kernel<1, true>), grid, block, bytes, stream, args);
    } else {
      hipLaunchKernelGGL((cube_reduce_columns_kernel<1, false>), grid, block, bytes, stream, args);
    }
  } else {
    if (broadened) {
      hipLaunchKernelGGL((cube_reduce_columns_kernel<2, true>), grid, block, bytes, stream, args);
    } else {
      hipLaunchKernelGGL((cube_reduce_columns_kernel<2, false>), grid, block, bytes, stream, args);
    }
  }
  return check("cube_reduce_columns_kernel");
}

int launch_cube_gather(const CubeGatherArgs& args, void* stream_v) {
  const int span = 2 * kGatherTile;
  const dim3 grid(static_cast<unsigned>((args.width + span - 1) / span),
                  static_cast<unsigned>((args.height + span - 1) / span));
  hipLaunchKernelGGL(cube_gather_kernel, grid, dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream_v), args);
  return check("cube_gather_kernel");
}

}  // namespace avr
