// Particle groups ("Particle groups"): friends-of-friends groups of particles given
// as points.  Two inside particles are linked iff their squared distance, minimum image on a
// periodic axis, is at most b * b; a group is a connected component of the link graph, and the
// groups with at least min_members members are numbered 1..N by their smallest particle index.
//
//   group_cells_kernel     one lane per particle: its cell of the uniform grid over the box (none
//                          for an outside particle), its parent entry, the outside count
//   group_link_kernel      one lane per sorted slot: the link test against the later slots of its
//                          own cell and all slots of the 13 forward neighbour cells; a linked pair
//                          is united
//   group_flatten_kernel   parent = root; sizes[root] counts the members
//   group_count_kernel     qualifying roots (sizes >= min_members) per chunk of 256 particles
//   group_scan_kernel      one workgroup: exclusive prefix sum of the chunks' counts, and N
//   group_rank_kernel      a root's label: its rank + 1 if it qualifies, else 0; 0 outside
//   group_label_kernel     every other particle takes its root's label
//
// Between the first kernel and the rest the caller sorts the particles by cell, stably (plumbing:
// torch.sort in runtime.py), finds the first slot of every cell and gathers the points into sorted
// order.  The grid only finds the candidates: h >= b (1 + 2^-10) along every axis with more than
// one cell (the plan's rule), so a linked pair lies in the same or in adjacent cells, and whether a
// pair is linked is decided by the link test alone -- the result does not depend on the grid.
//
// The union-find is the clumps' (avr_clumps.hip, where termination and completeness are argued):
// lock-free, a non-root's entry is always a smaller index, a union links the larger of two roots
// under the smaller with atomicMin.  The root of a finished group is its smallest particle index
// whatever order the atomics resolved in, and ranking the qualifying roots in ascending order gives
// the canonical numbering: equal arguments give equal bits.  The only atomics are atomicMin on the
// 32-bit parent entries, atomicAdd on the 32-bit sizes and one 64-bit atomicAdd per workgroup with
// an outside particle.
//
// Every loop is bounded by a count known at launch -- a cell's slots are cut at n_inside, the 13
// neighbours, the chunks -- or is the find or the union.  No lane waits for a value another
// workgroup writes.  Stores: cells, parent, labels at p < n; sizes through atomicAdd at a root < n;
// chunk_counts at a chunk < n_chunks.  A slot's particle index that is not below n is passed over,
// so nothing is stored outside the arrays whatever `order` holds.  Arithmetic is IEEE binary64,
// round to nearest, nothing fused (-ffp-contract=off); / is the correctly rounded __ddiv_rn.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "avr_cell_tiles.h"
#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;  // of the one workgroup that scans the chunks' counts
static_assert(kGroupChunk == kThreads, "a chunk is one particle per lane");

typedef const double __attribute__((address_space(1))) const_global_double;
typedef const long long __attribute__((address_space(1))) const_global_i64;

// ---- the grid ------------------------------------------------------------------------------------

// The cell of x along axis d: floor((x - lo) / h), clamped in double to [0, dims - 1] before the
// conversion.  Monotone in x.
__device__ __forceinline__ int cell_along(const GroupGridDev& g, int d, double x) {
  double q = floor(__ddiv_rn(x - g.lo[d], g.h[d]));
  q = q < 0.0 ? 0.0 : q;
  q = q > g.top[d] ? g.top[d] : q;
  return static_cast<int>(q);
}

// Whether a particle is inside: every coordinate finite and, on a periodic axis, in [lo, hi).
__device__ __forceinline__ bool is_inside(const GroupGridDev& g, const double x[3]) {
  bool inside = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    inside = inside && __builtin_isfinite(x[d]);
    if (g.periodic[d] != 0) inside = inside && x[d] >= g.lo[d] && x[d] < g.hi[d];
  }
  return inside;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int mask = 32; mask > 0; mask >>= 1) v += __shfl_xor(v, mask, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void group_cells_kernel(const ParticleGroupCellsArgs a) {
  __shared__ uint32_t wave_totals[kThreads / 64];
  const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
  uint32_t outside = 0;
  if (p < a.n) {
    const_global_double* points = (const_global_double*)a.points;
    const double x[3] = {points[p * 3ull + 0], points[p * 3ull + 1], points[p * 3ull + 2]};
    uint32_t cell = kGroupOutside, parent = kGroupOutside;
    if (is_inside(a.grid, x)) {
      const uint32_t cx = static_cast<uint32_t>(cell_along(a.grid, 0, x[0]));
      const uint32_t cy = static_cast<uint32_t>(cell_along(a.grid, 1, x[1]));
      const uint32_t cz = static_cast<uint32_t>(cell_along(a.grid, 2, x[2]));
      cell = (cz * static_cast<uint32_t>(a.grid.dims[1]) + cy) *
                 static_cast<uint32_t>(a.grid.dims[0]) + cx;
      parent = p;
    } else {
      outside = 1u;
    }
    a.cells[p] = cell;
    a.parent[p] = parent;
  }
  // per lane, per wave, per workgroup: one 64-bit atomic per workgroup with an outside particle
  const int tid = static_cast<int>(threadIdx.x);
  outside = wave_sum(outside);
  if ((tid & 63) == 0) wave_totals[tid >> 6] = outside;
  __syncthreads();
  if (tid == 0) {
    uint32_t total = 0;
    for (int w = 0; w < kThreads / 64; ++w) total += wave_totals[w];
    if (total != 0u) atomicAdd(a.totals, static_cast<unsigned long long>(total));
  }
}

// ---- the union-find (avr_clumps.hip's, on particle indices) ----------------------------------------

__device__ __forceinline__ uint32_t load_parent(uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of inside particle x.  Every value an entry ever holds is at most its own index, and
// only a root holds its own: each step moves to a strictly smaller index, so the walk ends after
// fewer than n steps whatever other lanes write meanwhile.
__device__ __forceinline__ uint32_t find_root(uint32_t* parent, uint32_t x) {
  uint32_t p = load_parent(parent, x);
  while (p != x) {
    x = p;
    p = load_parent(parent, x);
  }
  return x;
}

// Puts inside particles u and v into one tree; avr_clumps.hip's unite, where it is argued that the
// loop ends without waiting for any other lane and that no union is lost.
__device__ __forceinline__ void unite(uint32_t* parent, uint32_t u, uint32_t v) {
  for (;;) {
    u = find_root(parent, u);
    v = find_root(parent, v);
    if (u == v) return;
    const uint32_t a = u > v ? u : v, b = u > v ? v : u;
    const uint32_t old = atomicMin(parent + a, b);
    if (old == a) return;
    u = old;
    v = b;
  }
}

// ---- link ------------------------------------------------------------------------------------------

// |xq - xp| along one axis, the minimum image on a periodic one.
__device__ __forceinline__ double separation(double xp, double xq, bool periodic, double length) {
  double s = fabs(xq - xp);
  if (periodic) {
    const double other = length - s;
    s = other < s ? other : s;
  }
  return s;
}

// The slots [first, last) against the particle `id` at `x`: the link test and, where it holds, the
// union.  first and last are cut at n_inside by the caller.
__device__ __forceinline__ void link_slots(const ParticleGroupsArgs& a, uint32_t id,
                                           const double x[3], uint32_t first, uint32_t last) {
  const_global_double* points = (const_global_double*)a.points;
  const_global_i64* order = (const_global_i64*)a.order;
  const bool px = a.grid.periodic[0] != 0, py = a.grid.periodic[1] != 0;
  const bool pz = a.grid.periodic[2] != 0;
  for (uint32_t s = first; s < last; ++s) {
    const double dx = separation(x[0], points[s * 3ull + 0], px, a.grid.length[0]);
    const double dy = separation(x[1], points[s * 3ull + 1], py, a.grid.length[1]);
    const double dz = separation(x[2], points[s * 3ull + 2], pz, a.grid.length[2]);
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 <= a.b2) {
      const unsigned long long other = static_cast<unsigned long long>(order[s]);
      if (other < a.n) unite(a.parent, id, static_cast<uint32_t>(other));
    }
  }
}

// Consecutive lanes hold consecutive slots, that is particles of the same or of adjacent cells:
// the ranges and the positions a wave's lanes load are largely the same addresses.
__global__ __launch_bounds__(kThreads) void group_link_kernel(const ParticleGroupsArgs a) {
  const uint32_t slot = blockIdx.x * kThreads + threadIdx.x;
  if (slot >= a.n_inside) return;
  const_global_double* points = (const_global_double*)a.points;
  const_global_i64* cell_begin = (const_global_i64*)a.cell_begin;
  const unsigned long long own = static_cast<unsigned long long>(
      ((const_global_i64*)a.order)[slot]);
  if (own >= a.n) return;
  const uint32_t id = static_cast<uint32_t>(own);
  const double x[3] = {points[slot * 3ull + 0], points[slot * 3ull + 1], points[slot * 3ull + 2]};
  const int nx = a.grid.dims[0], ny = a.grid.dims[1], nz = a.grid.dims[2];
  const int cx = cell_along(a.grid, 0, x[0]);
  const int cy = cell_along(a.grid, 1, x[1]);
  const int cz = cell_along(a.grid, 2, x[2]);
  const unsigned long long limit = a.n_inside;
  // the range of a cell's slots, cut at n_inside whatever cell_begin holds
  auto range = [&](int ix, int iy, int iz, uint32_t* first, uint32_t* last) {
    const uint32_t c = (static_cast<uint32_t>(iz) * static_cast<uint32_t>(ny) +
                        static_cast<uint32_t>(iy)) * static_cast<uint32_t>(nx) +
                       static_cast<uint32_t>(ix);
    const unsigned long long f = static_cast<unsigned long long>(cell_begin[c]);
    const unsigned long long l = static_cast<unsigned long long>(cell_begin[c + 1]);
    *first = static_cast<uint32_t>(f < limit ? f : limit);
    *last = static_cast<uint32_t>(l < limit ? l : limit);
  };
  // its own cell: the later slots
  {
    uint32_t first, last;
    range(cx, cy, cz, &first, &last);
    link_slots(a, id, x, slot + 1u > first ? slot + 1u : first, last);
  }
  // the 13 forward neighbours: (dz, dy, dx) after (0, 0, 0) in that order of significance
  for (int e = 14; e < 27; ++e) {
    int ix = cx + (e % 3 - 1), iy = cy + ((e / 3) % 3 - 1), iz = cz + (e / 9 - 1);
    // a periodic axis has at least three cells, so the wrapped neighbours are distinct cells
    if (ix < 0 || ix >= nx) {
      if (a.grid.periodic[0] == 0) continue;
      ix = ix < 0 ? nx - 1 : 0;
    }
    if (iy < 0 || iy >= ny) {
      if (a.grid.periodic[1] == 0) continue;
      iy = iy < 0 ? ny - 1 : 0;
    }
    if (iz < 0 || iz >= nz) {
      if (a.grid.periodic[2] == 0) continue;
      iz = iz < 0 ? nz - 1 : 0;
    }
    uint32_t first, last;
    range(ix, iy, iz, &first, &last);
    link_slots(a, id, x, first, last);
  }
}

// ---- flatten, count, scan, rank, label -----------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void group_flatten_kernel(const ParticleGroupsArgs a) {
  const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t held = load_parent(a.parent, p);
  if (held == kGroupOutside || held >= a.n) return;
  uint32_t root = p;
  if (held != p) {
    root = find_root(a.parent, held);
    a.parent[p] = root;  // only this lane writes entry p now: it is no root and never becomes one
  }
  atomicAdd(a.sizes + root, 1u);
}

__device__ __forceinline__ bool qualifies(const ParticleGroupsArgs& a, uint32_t p) {
  return p < a.n && a.parent[p] == p && a.sizes[p] >= a.min_members;
}

__global__ __launch_bounds__(kThreads) void group_count_kernel(const ParticleGroupsArgs a) {
  const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
  uint32_t total;
  block_exclusive_sum<kThreads, 1>(qualifies(a, p) ? 1u : 0u, 0, &total);
  if (threadIdx.x == 0) a.chunk_counts[blockIdx.x] = total;
}

// One workgroup: lane t sums the counts of chunks [t per, (t + 1) per), the workgroup scans the
// lanes' sums, and the lane writes the exclusive prefix sums of its chunks back.
__global__ __launch_bounds__(kScanThreads) void group_scan_kernel(const ParticleGroupsArgs a) {
  const uint32_t per = (a.n_chunks + kScanThreads - 1) / kScanThreads;
  const uint32_t first = threadIdx.x * per < a.n_chunks ? threadIdx.x * per : a.n_chunks;
  const uint32_t last = first + per < a.n_chunks ? first + per : a.n_chunks;
  uint32_t sum = 0;
  for (uint32_t c = first; c < last; ++c) sum += a.chunk_counts[c];
  uint32_t total;
  uint32_t running = block_exclusive_sum<kScanThreads, 1>(sum, 0, &total);
  for (uint32_t c = first; c < last; ++c) {
    const uint32_t count = a.chunk_counts[c];
    a.chunk_counts[c] = running;
    running += count;
  }
  if (threadIdx.x == 0) *a.n_groups = static_cast<unsigned long long>(total);
}

// Roots and outside particles: a qualifying root gets its rank + 1, every other of them 0.
__global__ __launch_bounds__(kThreads) void group_rank_kernel(const ParticleGroupsArgs a) {
  const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
  const bool counted = qualifies(a, p);
  uint32_t total;
  const uint32_t rank =
      a.chunk_counts[blockIdx.x] + block_exclusive_sum<kThreads, 1>(counted ? 1u : 0u, 0, &total);
  if (p >= a.n) return;
  const uint32_t held = a.parent[p];
  if (held == p || held >= a.n) a.labels[p] = counted ? static_cast<int32_t>(rank + 1u) : 0;
}

// Every other particle: its root's label, written by the launch before.
__global__ __launch_bounds__(kThreads) void group_label_kernel(const ParticleGroupsArgs a) {
  const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t held = a.parent[p];
  if (held != p && held < a.n) a.labels[p] = a.labels[held];
}

int launched(const char* kernel) {
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string(kernel) + ": " + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

}  // namespace

int launch_particle_group_cells(const ParticleGroupCellsArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n == 0) return AVR_OK;
  const dim3 grid((args.n + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(group_cells_kernel, grid, dim3(kThreads), 0, stream, args);
  return launched("group_cells_kernel");
}

int launch_particle_groups(const ParticleGroupsArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n == 0) return AVR_OK;
  const dim3 chunks(args.n_chunks), threads(kThreads);
  if (hipMemsetAsync(args.sizes, 0, static_cast<size_t>(args.n) * sizeof(uint32_t), stream) !=
      hipSuccess) {
    return launched("hipMemsetAsync(sizes)");
  }
  if (args.n_inside > 0) {
    const dim3 slots((args.n_inside + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(group_link_kernel, slots, threads, 0, stream, args);
  }
  hipLaunchKernelGGL(group_flatten_kernel, chunks, threads, 0, stream, args);
  hipLaunchKernelGGL(group_count_kernel, chunks, threads, 0, stream, args);
  hipLaunchKernelGGL(group_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, args);
  hipLaunchKernelGGL(group_rank_kernel, chunks, threads, 0, stream, args);
  hipLaunchKernelGGL(group_label_kernel, chunks, threads, 0, stream, args);
  return launched("particle group kernels");
}

}  // namespace avr
