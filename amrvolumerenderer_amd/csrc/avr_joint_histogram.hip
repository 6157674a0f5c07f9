// Joint histogram of the raw cells of two fields, per AMR level, with an optional summed third
// field ("Phase plot and profile"): the input of phase plots and profiles.
//
//   joint_histogram_kernel<HAS_Y, HAS_S, LDS>
//
// The fields are scenes with the same box list; a cell is read from each at its own strides.  The
// decomposition is that of the scan kernels (avr_cell_tiles.h, shared with avr_scene_stats.hip and
// avr_derive.hip): one tile = 4 k-planes x 4 j-rows x 128 cells of one box, rows
// read coalesced and as f64 pairs where every field allows it, 16 consecutive tiles per workgroup.
//
// Per cell, in this order: a non-finite vx, vy or vs counts as `nonfinite`; a vx or vy outside its
// edges as `outside`; otherwise bin (by, bx) of the box's level gets +1 and, with s, +vs.  A value
// v lies in bin i when e[i] <= v < e[i + 1], the last bin closed at the top: the bin is the result
// of f64 comparisons against the edges in LDS.  A linear guess picks where the comparisons start
// (a galloping then a binary search from there); it never decides a bin.
//
// LDS == true: the workgroup keeps 32-bit counts and f64 sums of the level it is on in LDS (its 16
// tiles hold at most 32768 cells) and adds the non-zero bins to the global per-level arrays when
// the level changes and at the end.  Otherwise every cell goes to the global arrays.  Counts are
// exact; sums are f64 additions in no fixed order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_cell_tiles.h"
#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTilesPerGroup = 16;  // tiles (2048 cells each) per workgroup

typedef double __attribute__((address_space(3))) lds_double;
typedef double __attribute__((address_space(1))) global_double;
typedef const double __attribute__((address_space(1))) const_global_double;

struct TileCoords {
  const JointBoxDev* box;
  CellTile at;
};

// Which box / tile does tile number `tile` belong to.
__device__ __forceinline__ TileCoords locate_tile(const JointBoxDev* boxes,
                                                  const uint32_t* tile_begin, int n_boxes,
                                                  uint32_t tile) {
  const int b = locate_box(tile_begin, n_boxes, tile);
  TileCoords t;
  t.box = &boxes[b];
  const CellTileShape shape = cell_tile_shape(t.box->nx, t.box->ny);
  t.at = cell_tile_of(shape, tile - tile_begin[b]);
  return t;
}

// Calls visit(vx, vy, vs) for every valid cell of the tile; a field that is absent reads as 0.
template <bool HAS_Y, bool HAS_S, typename F>
__device__ __forceinline__ void for_each_cell(const TileCoords& tile, F&& visit) {
  const JointBoxDev& box = *tile.box;
  const_global_double* cx = (const_global_double*)box.cells[0];
  const_global_double* cy = (const_global_double*)box.cells[HAS_Y ? 1 : 0];
  const_global_double* cs = (const_global_double*)box.cells[HAS_S ? 2 : 0];
  const uint32_t jx = static_cast<uint32_t>(box.jstride[0]), kx = static_cast<uint32_t>(box.kstride[0]);
  const uint32_t jy = static_cast<uint32_t>(box.jstride[1]), ky = static_cast<uint32_t>(box.kstride[1]);
  const uint32_t js = static_cast<uint32_t>(box.jstride[2]), ks = static_cast<uint32_t>(box.kstride[2]);
  const int t = static_cast<int>(threadIdx.x);
  if (box.paired) {  // every field: 16-byte aligned cells and even strides (set by the host)
    typedef double double2_t __attribute__((ext_vector_type(2)));
    typedef const double2_t __attribute__((address_space(1))) const_global_double2;
    const int i = tile.at.chunk * kClassifyChunk + (t & 63) * 2;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int row = pass * 4 + (t >> 6);
      const uint32_t j = static_cast<uint32_t>(tile.at.bj * kBrickY + (row & 3));
      const uint32_t k = static_cast<uint32_t>(tile.at.bk * kBrickZ + (row >> 2));
      if (i < box.nx && static_cast<int>(j) < box.ny && static_cast<int>(k) < box.nz) {
        const uint32_t ui = static_cast<uint32_t>(i);
        const uint32_t ax = ui + j * jx + k * kx;
        const uint32_t ay = ui + j * jy + k * ky;
        const uint32_t as = ui + j * js + k * ks;
        if (i + 1 < box.nx) {
          const double2_t vx = *(const_global_double2*)(cx + ax);
          double2_t vy = {0.0, 0.0}, vs = {0.0, 0.0};
          if (HAS_Y) vy = *(const_global_double2*)(cy + ay);
          if (HAS_S) vs = *(const_global_double2*)(cs + as);
          visit(vx.x, vy.x, vs.x);
          visit(vx.y, vy.y, vs.y);
        } else {
          visit(cx[ax], HAS_Y ? cy[ay] : 0.0, HAS_S ? cs[as] : 0.0);
        }
      }
    }
  } else {
    const int i = tile.at.chunk * kClassifyChunk + (t & 127);
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
      const int row = pass * 2 + (t >> 7);
      const uint32_t j = static_cast<uint32_t>(tile.at.bj * kBrickY + (row & 3));
      const uint32_t k = static_cast<uint32_t>(tile.at.bk * kBrickZ + (row >> 2));
      if (i < box.nx && static_cast<int>(j) < box.ny && static_cast<int>(k) < box.nz) {
        const uint32_t ui = static_cast<uint32_t>(i);
        visit(cx[ui + j * jx + k * kx], HAS_Y ? cy[ui + j * jy + k * ky] : 0.0,
              HAS_S ? cs[ui + j * js + k * ks] : 0.0);
      }
    }
  }
}

// The bin of v among the n + 1 edges e (LDS), given e[0] <= v <= e[n]: the largest i in
// [0, n - 1] with e[i] <= v.  `lo` and `scale` only choose the first edge looked at.
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

__device__ __forceinline__ void lds_add(lds_double* at, double v) {
  __hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The output arrays are ordinary (coarse-grained) device allocations: the hardware's f64 add.
__device__ __forceinline__ void global_add(double* at, double v) { unsafeAtomicAdd(at, v); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int mask = 32; mask > 0; mask >>= 1) v += __shfl_xor(v, mask, 64);
  return v;
}

template <bool HAS_Y, bool HAS_S, bool LDS>
__global__ __launch_bounds__(kThreads) void joint_histogram_kernel(const JointHistogramArgs a) {
  // [x edges: nx + 1][y edges: ny + 1 (HAS_Y)][sums: bins (LDS, HAS_S)][counts: bins x u32 (LDS)]
  extern __shared__ double joint_lds[];
  __shared__ uint32_t wave_totals[kThreads / 64][2];
  const int nx = a.nx, ny = a.ny;
  const int bins = nx * ny;
  lds_double* ex = (lds_double*)joint_lds;
  lds_double* ey = ex + (nx + 1);
  lds_double* local_sums = HAS_Y ? ey + (ny + 1) : ey;
  unsigned int* local_counts =
      reinterpret_cast<unsigned int*>(joint_lds + (nx + 1) + (HAS_Y ? ny + 1 : 0) +
                                      (HAS_S ? bins : 0));
  const int tid = static_cast<int>(threadIdx.x);
  for (int i = tid; i <= nx; i += kThreads) ex[i] = a.x_edges[i];
  if (HAS_Y) {
    for (int i = tid; i <= ny; i += kThreads) ey[i] = a.y_edges[i];
  }
  if (LDS) {
    for (int b = tid; b < bins; b += kThreads) {
      local_counts[b] = 0u;
      if (HAS_S) local_sums[b] = 0.0;
    }
  }
  __syncthreads();

  unsigned long long* cells = a.cells;
  double* sums = a.sums;
  // adds the workgroup's non-zero bins to the global arrays of `level` and clears them
  auto flush = [&](int level) {
    const size_t base = static_cast<size_t>(level) * static_cast<size_t>(bins);
    for (int b = tid; b < bins; b += kThreads) {
      const unsigned int c = local_counts[b];
      if (c != 0u) {
        atomicAdd(&cells[base + b], static_cast<unsigned long long>(c));
        local_counts[b] = 0u;
        if (HAS_S) {
          global_add(&sums[base + b], local_sums[b]);
          local_sums[b] = 0.0;
        }
      }
    }
  };

  uint32_t outside = 0, nonfinite = 0;
  int held_level = -1;  // LDS: the level whose bins the workgroup holds
  const uint32_t first = blockIdx.x * kTilesPerGroup;
  const uint32_t last = (first + kTilesPerGroup < a.n_tiles) ? first + kTilesPerGroup : a.n_tiles;
  for (uint32_t t = first; t < last; ++t) {
    const TileCoords tile = locate_tile(a.boxes, a.tile_begin, a.n_boxes, t);
    const int level = __builtin_amdgcn_readfirstlane(tile.box->level);
    if (LDS && level != held_level) {  // workgroup-uniform
      if (held_level >= 0) {
        __syncthreads();
        flush(held_level);
        __syncthreads();
      }
      held_level = level;
    }
    const size_t base = static_cast<size_t>(level) * static_cast<size_t>(bins);
    for_each_cell<HAS_Y, HAS_S>(tile, [&](double vx, double vy, double vs) {
      bool finite = __builtin_isfinite(vx);
      if (HAS_Y) finite = finite & __builtin_isfinite(vy);
      if (HAS_S) finite = finite & __builtin_isfinite(vs);
      if (!finite) {
        nonfinite += 1;
        return;
      }
      bool inside = (a.x_lo <= vx) & (vx <= a.x_hi);
      if (HAS_Y) inside = inside & (a.y_lo <= vy) & (vy <= a.y_hi);
      if (!inside) {
        outside += 1;
        return;
      }
      int bin = find_bin(ex, nx, a.x_lo, a.x_scale, vx);
      if (HAS_Y) bin += find_bin(ey, ny, a.y_lo, a.y_scale, vy) * nx;
      if (LDS) {
        atomicAdd(&local_counts[bin], 1u);
        if (HAS_S) lds_add(local_sums + bin, vs);
      } else {
        atomicAdd(&cells[base + bin], 1ull);
        if (HAS_S) global_add(&sums[base + bin], vs);
      }
    });
  }
  if (LDS && held_level >= 0) {
    __syncthreads();
    flush(held_level);
  }

  outside = wave_sum(outside);
  nonfinite = wave_sum(nonfinite);
  if ((tid & 63) == 0) {
    wave_totals[tid >> 6][0] = outside;
    wave_totals[tid >> 6][1] = nonfinite;
  }
  __syncthreads();
  if (tid < 2) {
    uint32_t total = 0;
    for (int w = 0; w < kThreads / 64; ++w) total += wave_totals[w][tid];
    if (total != 0u) atomicAdd(&a.totals[tid], static_cast<unsigned long long>(total));
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

size_t joint_histogram_lds_bytes(int nx, int ny, bool has_y, bool has_s, bool lds) {
  const size_t bins = static_cast<size_t>(nx) * static_cast<size_t>(ny);
  size_t bytes = static_cast<size_t>(nx + 1) * 8 + (has_y ? static_cast<size_t>(ny + 1) * 8 : 0);
  if (lds) bytes += bins * 4 + (has_s ? bins * 8 : 0);
  return bytes;
}

int launch_joint_histogram(const JointHistogramArgs& args, bool has_y, bool has_s, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_tiles == 0) return AVR_OK;
  const bool lds = joint_histogram_lds_bytes(args.nx, args.ny, has_y, has_s, true) <=
                   kJointHistogramLdsBudget;
  const size_t bytes = joint_histogram_lds_bytes(args.nx, args.ny, has_y, has_s, lds);
  const uint32_t groups = (args.n_tiles + kTilesPerGroup - 1) / kTilesPerGroup;
#define AVR_JOINT(Y, S, L)                                                                     \
  hipLaunchKernelGGL((joint_histogram_kernel<Y, S, L>), dim3(groups), dim3(kThreads), bytes, \
                     stream, args)
  if (has_y) {
    if (has_s) { if (lds) AVR_JOINT(true, true, true); else AVR_JOINT(true, true, false); }
    else       { if (lds) AVR_JOINT(true, false, true); else AVR_JOINT(true, false, false); }
  } else {
    if (has_s) { if (lds) AVR_JOINT(false, true, true); else AVR_JOINT(false, true, false); }
    else       { if (lds) AVR_JOINT(false, false, true); else AVR_JOINT(false, false, false); }
  }
#undef AVR_JOINT
  return check("joint_histogram_kernel");
}

}  // namespace avr
