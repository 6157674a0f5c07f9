// Clumps ("Clumps"): the connected components of the cells whose raw value lies in
// [lower, upper], across boxes and levels, numbered 1..N by their smallest cell ordinal, and the
// per-clump table of a label field.
//
//   clump_init_kernel      parent[ordinal] = the start of the cell's run of selected cells, or none
//   clump_merge_kernel     union with the +x, +y, +z neighbour and, at a face, with the ghost cell
//   clump_flatten_kernel   parent = root; roots counted per chunk of 1024 ordinals
//   clump_scan_kernel      one workgroup: exclusive prefix sum of the chunks' counts, and N
//   clump_rank_kernel      a root's entry becomes kClumpRanked | (label - 1)
//   clump_label_kernel     f64 labels into the output boxes at their own strides
//   clump_table_kernel<S>  cells (and sums of a field) per level and label
//   clump_link_kernel<P>   index extents (and the parent labels in a coarser ladder step) per label
//
// A cell's ordinal is cell_begin of its box + (k ny + j) nx + i; parent holds one uint32 per
// ordinal.  The union-find is lock-free and waits for nothing: a non-root's entry is always a
// smaller ordinal, so a walk towards the root strictly descends, and a union links the larger of
// two roots under the smaller with atomicMin.  The root of a finished clump is therefore its
// smallest ordinal whatever order the atomics resolved in, and ranking the roots in ascending
// order gives the canonical numbering: equal arguments give equal bits.
//
// init, merge and label walk the cells in the tiles of avr_cell_tiles.h (4 k-planes x 4 j-rows x
// 128 cells of one box, 16 consecutive tiles per workgroup), one cell per lane and pass, so that a
// wave holds 64 consecutive cells of one row: init links every run of selected cells inside a
// wave's 64 to the run's first cell by a ballot, before anything goes to memory, and merge then
// has no union to make along x but at a wave's last cell.  The ghost of a face cell is found by
// the same-or-coarser rule (avr_level_cells.h states it; unite_ghost writes the loop out, with
// the use of the hit inside it) among the boxes the host listed for the face.  Only cells of the
// scene's boxes are ever read.
//
// Every loop is bounded by a count known at launch, or is the find or the union below.  No lane
// waits for a value another workgroup writes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_cell_tiles.h"
#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTilesPerGroup = 16;  // tiles (2048 cells each) per workgroup
constexpr int kScanThreads = 1024;       // of the one workgroup that scans the chunks' counts
constexpr int kRowsPerPass = 2;          // 256 lanes = 2 rows of 128 cells
constexpr int kPasses = 8;               // 16 rows per tile
static_assert(kClumpChunk == 4 * kThreads, "a chunk is four ordinals per lane");

typedef double __attribute__((address_space(1))) global_double;
typedef const double __attribute__((address_space(1))) const_global_double;
typedef const ClumpBoxDev __attribute__((address_space(4))) constant_box;
typedef const JointBoxDev __attribute__((address_space(4))) constant_table_box;
typedef const ClumpLinkBoxDev __attribute__((address_space(4))) constant_link_box;
typedef const uint32_t __attribute__((address_space(4))) constant_u32;
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef const double2_t __attribute__((address_space(1))) const_global_double2;

// ---- the walk over the workgroup's tiles -------------------------------------------------------

// body(b, box, tile) for each of the workgroup's consecutive tiles: one search (scalar loads) for
// the first tile's box, then a walk along the boxes.
template <class Box, class F>
__device__ __forceinline__ void for_each_tile(Box* boxes, constant_u32* tile_begin, int n_boxes,
                                              uint32_t n_tiles, F&& body) {
  const uint32_t first = blockIdx.x * kTilesPerGroup;
  const uint32_t last = (first + kTilesPerGroup < n_tiles) ? first + kTilesPerGroup : n_tiles;
  int b = locate_box(tile_begin, n_boxes, first);
  uint32_t begin = tile_begin[b], end = tile_begin[b + 1];
  for (uint32_t t = first; t < last; ++t) {
    while (t >= end) {  // t < n_tiles = tile_begin[n_boxes]; boxes without tiles are passed over
      ++b;
      begin = end;
      end = tile_begin[b + 1];
    }
    body(b, boxes + b, cell_tile_of(boxes[b].nx, boxes[b].ny, t - begin));
  }
}

// One cell per lane and pass.  cell(i, j, k, valid) is called by every lane in every pass, in
// converged control flow: a wave's lanes hold 64 consecutive i of one row.
template <class F>
__device__ __forceinline__ void for_each_cell(const CellTile& at, int nx, int ny, int nz,
                                              F&& cell) {
  const int t = static_cast<int>(threadIdx.x);
  const int i = at.chunk * kClassifyChunk + (t & (kClassifyChunk - 1));
#pragma unroll
  for (int pass = 0; pass < kPasses; ++pass) {
    const int row = pass * kRowsPerPass + (t >> 7);
    const int j = at.bj * kBrickY + (row & 3);
    const int k = at.bk * kBrickZ + (row >> 2);
    cell(i, j, k, i < nx && j < ny && k < nz);
  }
}

__device__ __forceinline__ uint32_t ordinal_of(constant_box* box, int i, int j, int k) {
  return box->cell_begin +
         (static_cast<uint32_t>(k) * static_cast<uint32_t>(box->ny) + static_cast<uint32_t>(j)) *
             static_cast<uint32_t>(box->nx) +
         static_cast<uint32_t>(i);
}

// ---- init ----------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void clump_init_kernel(const ClumpArgs a) {
  const double lower = a.lower, upper = a.upper;
  uint32_t* parent = a.parent;
  const uint32_t lane = threadIdx.x & 63u;
  for_each_tile((constant_box*)a.boxes, (constant_u32*)a.tile_begin, a.n_boxes, a.n_tiles,
                [&](int, constant_box* box, const CellTile& at) {
    const_global_double* in = (const_global_double*)box->in;
    const uint32_t ji = static_cast<uint32_t>(box->jstride_in);
    const uint32_t ki = static_cast<uint32_t>(box->kstride_in);
    for_each_cell(at, box->nx, box->ny, box->nz, [&](int i, int j, int k, bool valid) {
      bool selected = false;
      if (valid) {
        const double v = in[static_cast<uint32_t>(i) + static_cast<uint32_t>(j) * ji +
                            static_cast<uint32_t>(k) * ki];
        selected = v >= lower && v <= upper;  // false for a NaN
      }
      // the first cell of the run of selected cells that ends at this lane: one above the highest
      // lane below this one that is not selected
      const unsigned long long mask = __ballot(selected);
      const unsigned long long gaps = ~mask & ((1ull << lane) - 1ull);
      const uint32_t start = gaps != 0 ? 64u - static_cast<uint32_t>(__clzll(gaps)) : 0u;
      if (valid) {
        const uint32_t x = ordinal_of(box, i, j, k);
        parent[x] = selected ? x - (lane - start) : kClumpNone;
      }
    });
  });
}

// ---- merge ---------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t load_parent(uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of selected cell x.  Every value an entry ever holds is at most its own ordinal, and
// only a root holds its own: each step moves to a strictly smaller ordinal, so the walk ends after
// fewer than n_cells steps whatever other lanes write meanwhile.
__device__ __forceinline__ uint32_t find_root(uint32_t* parent, uint32_t x) {
  uint32_t p = load_parent(parent, x);
  while (p != x) {
    x = p;
    p = load_parent(parent, x);
  }
  return x;
}

// Puts selected cells u and v, which are adjacent, into one tree.  With a > b the two roots found,
// atomicMin(parent[a], b) returns what a held.  If that is a, a was still a root and now hangs
// under b: done.  Otherwise a had been linked under old < a by another lane in between and now
// holds min(old, b); either way a is tied to one of old and b, and old and b remain to be united,
// which the next round does.  Termination: in every round that does not end the loop, the larger
// of the pair's roots is replaced by a root that is strictly smaller (old < a, and roots only ever
// move down), and ordinals are bounded below, so each union ends without waiting for any other
// lane.  Nothing is lost: take the forest's links together with each running union's current pair
// as a graph; a round replaces {a - old, a ~ b} by {a - min(old, b), old ~ b}, which connects the
// same cells, so what was connected stays connected and every united pair ends up in one tree.
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

// Unites cell x of box b with the cell that holds the ghost index (gx, gy, gz) of the box's level
// past face `face` (2 axis + side), if a box of the same or a coarser level holds it and that cell
// is selected.  The loop runs over the face's candidate list, whose length the host fixed.  It is
// find_same_or_coarser's loop with the ordinal formed at the hit, while the box record is at hand:
// this kernel is bound by dependent loads and its device code is kept as it was measured.
__device__ __forceinline__ void unite_ghost(const ClumpArgs& a, int b, int level, int face,
                                            long long gx, long long gy, long long gz,
                                            uint32_t x) {
  const uint32_t first = a.candidate_begin[6 * b + face];
  const uint32_t last = a.candidate_begin[6 * b + face + 1];
  int found_level = -1;
  uint32_t ghost = 0;
  for (uint32_t q = first; q < last; ++q) {
    const ClumpBoxDev& other = a.boxes[a.candidates[q]];
    if (other.level > level || other.level <= found_level) continue;
    long long ox = gx, oy = gy, oz = gz;
    for (int m = level; m > other.level; --m) {
      const long long r = a.levels->ratio[m - 1];
      ox = floor_div(ox, r);
      oy = floor_div(oy, r);
      oz = floor_div(oz, r);
    }
    ox -= other.lo[0];
    oy -= other.lo[1];
    oz -= other.lo[2];
    if (ox >= 0 && ox < other.nx && oy >= 0 && oy < other.ny && oz >= 0 && oz < other.nz) {
      found_level = other.level;
      ghost = other.cell_begin +
              (static_cast<uint32_t>(oz) * static_cast<uint32_t>(other.ny) +
               static_cast<uint32_t>(oy)) * static_cast<uint32_t>(other.nx) +
              static_cast<uint32_t>(ox);
    }
  }
  if (found_level >= 0 && load_parent(a.parent, ghost) != kClumpNone) unite(a.parent, x, ghost);
}

__global__ __launch_bounds__(kThreads) void clump_merge_kernel(const ClumpArgs a) {
  uint32_t* parent = a.parent;
  for_each_tile((constant_box*)a.boxes, (constant_u32*)a.tile_begin, a.n_boxes, a.n_tiles,
                [&](int b, constant_box* box, const CellTile& at) {
    const int nx = box->nx, ny = box->ny, nz = box->nz;
    const int level = box->level;
    const long long lx = box->lo[0], ly = box->lo[1], lz = box->lo[2];
    const uint32_t row = static_cast<uint32_t>(nx);
    const uint32_t plane = row * static_cast<uint32_t>(ny);
    for_each_cell(at, nx, ny, nz, [&](int i, int j, int k, bool valid) {
      if (!valid) return;
      const uint32_t x = ordinal_of(box, i, j, k);
      if (load_parent(parent, x) == kClumpNone) return;
      // along x init has linked the cells a wave holds; a wave's last cell meets the next wave's
      if ((i & 63) == 63 && i + 1 < nx && load_parent(parent, x + 1) != kClumpNone) {
        unite(parent, x, x + 1);
      }
      if (j + 1 < ny && load_parent(parent, x + row) != kClumpNone) unite(parent, x, x + row);
      if (k + 1 < nz && load_parent(parent, x + plane) != kClumpNone) unite(parent, x, x + plane);
      const long long gx = lx + i, gy = ly + j, gz = lz + k;
      if (i == 0) unite_ghost(a, b, level, 0, gx - 1, gy, gz, x);
      if (i == nx - 1) unite_ghost(a, b, level, 1, gx + 1, gy, gz, x);
      if (j == 0) unite_ghost(a, b, level, 2, gx, gy - 1, gz, x);
      if (j == ny - 1) unite_ghost(a, b, level, 3, gx, gy + 1, gz, x);
      if (k == 0) unite_ghost(a, b, level, 4, gx, gy, gz - 1, x);
      if (k == nz - 1) unite_ghost(a, b, level, 5, gx, gy, gz + 1, x);
    });
  });
}

// ---- flatten, scan, rank -------------------------------------------------------------------------

// One chunk of kClumpChunk consecutive ordinals per workgroup, four per lane (the buffer is padded
// to whole chunks; entries from n_cells on are read, never used).  Only this lane writes its four.
__global__ __launch_bounds__(kThreads) void clump_flatten_kernel(const ClumpArgs a) {
  uint32_t* parent = a.parent;
  const uint32_t base = blockIdx.x * kClumpChunk + threadIdx.x * 4u;
  const uint4 held = *reinterpret_cast<const uint4*>(parent + base);
  const uint32_t p[4] = {held.x, held.y, held.z, held.w};
  uint32_t roots = 0;
#pragma unroll
  for (uint32_t e = 0; e < 4; ++e) {
    const uint32_t x = base + e;
    if (x >= a.n_cells || p[e] == kClumpNone) continue;
    if (p[e] == x) {
      roots += 1;
    } else {
      parent[x] = find_root(parent, p[e]);
    }
  }
  uint32_t total;
  block_exclusive_sum<kThreads, 1>(roots, 0, &total);
  if (threadIdx.x == 0) a.chunk_roots[blockIdx.x] = total;
}

// One workgroup: lane t sums the counts of chunks [t per, (t + 1) per), the workgroup scans the
// lanes' sums, and the lane writes the exclusive prefix sums of its chunks back.
__global__ __launch_bounds__(kScanThreads) void clump_scan_kernel(const ClumpArgs a) {
  const uint32_t per = (a.n_chunks + kScanThreads - 1) / kScanThreads;
  const uint32_t first = threadIdx.x * per;
  const uint32_t last = first + per < a.n_chunks ? first + per : a.n_chunks;
  uint32_t sum = 0;
  for (uint32_t c = first; c < last; ++c) sum += a.chunk_roots[c];
  uint32_t total;
  uint32_t running = block_exclusive_sum<kScanThreads, 1>(sum, 0, &total);
  for (uint32_t c = first; c < last; ++c) {
    const uint32_t count = a.chunk_roots[c];
    a.chunk_roots[c] = running;
    running += count;
  }
  if (threadIdx.x == 0) *a.count = total;
}

__global__ __launch_bounds__(kThreads) void clump_rank_kernel(const ClumpArgs a) {
  uint32_t* parent = a.parent;
  const uint32_t base = blockIdx.x * kClumpChunk + threadIdx.x * 4u;
  const uint4 held = *reinterpret_cast<const uint4*>(parent + base);
  const uint32_t p[4] = {held.x, held.y, held.z, held.w};
  uint32_t roots = 0;
#pragma unroll
  for (uint32_t e = 0; e < 4; ++e) roots += (base + e < a.n_cells && p[e] == base + e) ? 1u : 0u;
  uint32_t total;
  uint32_t rank = a.chunk_roots[blockIdx.x] + block_exclusive_sum<kThreads, 1>(roots, 0, &total);
#pragma unroll
  for (uint32_t e = 0; e < 4; ++e) {
    if (base + e < a.n_cells && p[e] == base + e) parent[base + e] = kClumpRanked | rank++;
  }
}

// ---- labels --------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void clump_label_kernel(const ClumpArgs a) {
  const uint32_t* parent = a.parent;
  for_each_tile((constant_box*)a.boxes, (constant_u32*)a.tile_begin, a.n_boxes, a.n_tiles,
                [&](int, constant_box* box, const CellTile& at) {
    global_double* out = (global_double*)box->out;
    const uint32_t jo = static_cast<uint32_t>(box->jstride_out);
    const uint32_t ko = static_cast<uint32_t>(box->kstride_out);
    for_each_cell(at, box->nx, box->ny, box->nz, [&](int i, int j, int k, bool valid) {
      if (!valid) return;
      uint32_t p = parent[ordinal_of(box, i, j, k)];
      double label = 0.0;
      if (p != kClumpNone) {
        if ((p & kClumpRanked) == 0u) p = parent[p];  // a root's entry is always ranked
        label = static_cast<double>((p & ~kClumpRanked) + 1u);
      }
      out[static_cast<uint32_t>(i) + static_cast<uint32_t>(j) * jo + static_cast<uint32_t>(k) * ko] =
          label;
    });
  });
}

// ---- table ---------------------------------------------------------------------------------------

// The output arrays are ordinary (coarse-grained) device allocations: the hardware's f64 add.
__device__ __forceinline__ void global_add(double* at, double v) { unsafeAtomicAdd(at, v); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int mask = 32; mask > 0; mask >>= 1) v += __shfl_xor(v, mask, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
  for (int mask = 32; mask > 0; mask >>= 1) v = v + __shfl_xor(v, mask, 64);
  return v;
}

template <bool HAS_S>
__global__ __launch_bounds__(kThreads) void clump_table_kernel(const ClumpTableArgs a) {
  __shared__ uint32_t wave_totals[kThreads / 64][2];
  const int tid = static_cast<int>(threadIdx.x);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n = a.n_clumps;
  const double top = static_cast<double>(n);
  unsigned long long* cells = a.cells;
  double* sums = a.sums;
  uint32_t outside = 0, nonfinite = 0;
  for_each_tile((constant_table_box*)a.boxes, (constant_u32*)a.tile_begin, a.n_boxes, a.n_tiles,
                [&](int, constant_table_box* box, const CellTile& at) {
    const int nx = box->nx, ny = box->ny, nz = box->nz;
    const uint32_t level_base = static_cast<uint32_t>(box->level) * n;
    const_global_double* cl = (const_global_double*)box->cells[0];
    const_global_double* cs = (const_global_double*)box->cells[HAS_S ? 1 : 0];
    const uint32_t jl = static_cast<uint32_t>(box->jstride[0]), kl = static_cast<uint32_t>(box->kstride[0]);
    const uint32_t js = static_cast<uint32_t>(box->jstride[1]), ks = static_cast<uint32_t>(box->kstride[1]);
    // One cell of every lane, in converged control flow.  A wave whose counted lanes hold one
    // label adds once per array; otherwise every counted lane adds for itself.
    auto visit = [&](bool valid, double label, double vs) {
      const bool active = valid && __double_as_longlong(label) != 0ll;
      const bool integer = label >= 1.0 && label <= top && label == __builtin_floor(label);
      const bool finite = !HAS_S || __builtin_isfinite(vs);
      outside += (active && !integer) ? 1u : 0u;
      nonfinite += (active && integer && !finite) ? 1u : 0u;
      const bool counted = active && integer && finite;
      const uint32_t entry = counted ? level_base + static_cast<uint32_t>(label) - 1u : 0u;
      const unsigned long long mask = __ballot(counted);
      if (mask == 0ull) return;
      const int first = __ffsll(mask) - 1;
      const uint32_t shared = __shfl(entry, first, 64);
      if (__ballot(counted && entry != shared) == 0ull) {
        double sum = 0.0;
        if (HAS_S) sum = wave_sum(counted ? vs : 0.0);
        if (lane == static_cast<uint32_t>(first)) {
          atomicAdd(&cells[shared], static_cast<unsigned long long>(__popcll(mask)));
          if (HAS_S) global_add(&sums[shared], sum);
        }
      } else if (counted) {
        atomicAdd(&cells[entry], 1ull);
        if (HAS_S) global_add(&sums[entry], vs);
      }
    };
    if (box->paired) {  // both fields: 16-byte aligned cells and even strides (set by the host)
      const int i = at.chunk * kClassifyChunk + (tid & 63) * 2;
      const uint32_t ui = static_cast<uint32_t>(i);
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int row = pass * 4 + (tid >> 6);
        const uint32_t j = static_cast<uint32_t>(at.bj * kBrickY + (row & 3));
        const uint32_t k = static_cast<uint32_t>(at.bk * kBrickZ + (row >> 2));
        const bool valid = i < nx && static_cast<int>(j) < ny && static_cast<int>(k) < nz;
        const bool whole = valid && i + 1 < nx;
        double2_t vl = {0.0, 0.0}, vs = {0.0, 0.0};
        if (whole) {
          vl = *(const_global_double2*)(cl + (ui + j * jl + k * kl));
          if (HAS_S) vs = *(const_global_double2*)(cs + (ui + j * js + k * ks));
        } else if (valid) {
          vl.x = cl[ui + j * jl + k * kl];
          if (HAS_S) vs.x = cs[ui + j * js + k * ks];
        }
        visit(valid, vl.x, vs.x);
        visit(whole, vl.y, vs.y);
      }
    } else {
      for_each_cell(at, nx, ny, nz, [&](int i, int j, int k, bool valid) {
        double vl = 0.0, vs = 0.0;
        if (valid) {
          const uint32_t ui = static_cast<uint32_t>(i), uj = static_cast<uint32_t>(j);
          const uint32_t uk = static_cast<uint32_t>(k);
          vl = cl[ui + uj * jl + uk * kl];
          if (HAS_S) vs = cs[ui + uj * js + uk * ks];
        }
        visit(valid, vl, vs);
      });
    }
  });

  outside = wave_sum(outside);
  nonfinite = wave_sum(nonfinite);
  if (lane == 0u) {
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

// ---- links and extents ---------------------------------------------------------------------------

// What a wave has gathered for one label and not yet written ("Clump tree"): the
// ends are indices of the finest level, so the record outlives a change of box and of level.
// label 0: nothing is held.  Every member is the same in all lanes of the wave.
struct LinkRecord {
  uint32_t label;
  int32_t lo[3], hi[3];
  uint32_t parent_lo, parent_hi;
};

__device__ __forceinline__ void clear(LinkRecord& r, uint32_t label) {
  r.label = label;
  for (int a = 0; a < 3; ++a) {
    r.lo[a] = INT32_MAX;
    r.hi[a] = INT32_MIN;
  }
  r.parent_lo = UINT32_MAX;
  r.parent_hi = 0u;
}

__device__ __forceinline__ int32_t load_entry(const int32_t* at) {
  return __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t load_entry(const uint32_t* at) {
  return __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Combines record r into the outputs, reading before it writes: an entry is loaded, and the atomic
// is issued only if r's value would change what was loaded.  The load may be stale -- other waves
// combine into the same entry meanwhile -- and nothing is lost by that.  An entry of a minimum only
// ever falls: whatever it holds now is at most what was loaded.  So if v >= loaded, then v >=
// loaded >= current and atomicMin(entry, v) would have left the entry as it is: the skipped atomic
// was a no-op.  If v < loaded the atomic is issued and resolves against the current value, as it
// would have without the load.  A stale load can therefore only cost an atomic that turns out to
// be unneeded, never lose one; the same holds for a maximum with the order reversed.  The result
// is the minimum / maximum of integers over all cells, exact in whatever order the atomics
// resolve.  The eight loads are issued together, ahead of the atomics; no atomic returns a value.
template <bool HAS_PARENT>
__device__ __forceinline__ void combine_into(const ClumpLinkArgs& a, const LinkRecord& r) {
  const uint32_t n = a.n_clumps, e = r.label - 1u;  // 6 n < 2^31
  int32_t held_lo[3], held_hi[3];
  uint32_t held_parent_lo = 0u, held_parent_hi = 0u;
#pragma unroll
  for (uint32_t axis = 0; axis < 3; ++axis) {
    held_lo[axis] = load_entry(a.extent + (axis * n + e));
    held_hi[axis] = load_entry(a.extent + ((3u + axis) * n + e));
  }
  if (HAS_PARENT) {
    held_parent_lo = load_entry(a.parent_lo + e);
    held_parent_hi = load_entry(a.parent_hi + e);
  }
#pragma unroll
  for (uint32_t axis = 0; axis < 3; ++axis) {
    if (r.lo[axis] < held_lo[axis]) atomicMin(a.extent + (axis * n + e), r.lo[axis]);
    if (r.hi[axis] > held_hi[axis]) atomicMax(a.extent + ((3u + axis) * n + e), r.hi[axis]);
  }
  if (HAS_PARENT) {
    if (r.parent_lo < held_parent_lo) atomicMin(a.parent_lo + e, r.parent_lo);
    if (r.parent_hi > held_parent_hi) atomicMax(a.parent_hi + e, r.parent_hi);
  }
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  for (int mask = 32; mask > 0; mask >>= 1) {
    const uint32_t other = __shfl_xor(v, mask, 64);
    v = other < v ? other : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
  for (int mask = 32; mask > 0; mask >>= 1) {
    const uint32_t other = __shfl_xor(v, mask, 64);
    v = other > v ? other : v;
  }
  return v;
}
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// The table kernel's scan with a record carried by each wave instead of atomics per visit.  In a
// visit a wave's lanes hold cells of one row, `step` apart in i from lane 0's on, so j and k are
// the wave's, and among the counted lanes the first has the lowest i and the last the highest:
// while the counted lanes share a label, the visit's six ends follow from the ballot alone, and
// the parent label from one lane unless the lanes disagree (then two shuffle reductions).  The
// record goes to memory, through lane 0, when the shared label changes, when a visit is mixed and
// after the workgroup's last tile; in a mixed visit every counted lane combines its own cell.
template <bool HAS_PARENT>
__global__ __launch_bounds__(kThreads) void clump_link_kernel(const ClumpLinkArgs a) {
  __shared__ uint32_t wave_totals[kThreads / 64][2];
  const int tid = static_cast<int>(threadIdx.x);
  const uint32_t lane = threadIdx.x & 63u;
  const double top = static_cast<double>(a.n_clumps);
  const double parent_top = static_cast<double>(a.n_parents);
  uint32_t outside = 0, orphans = 0;
  LinkRecord held;
  clear(held, 0u);
  for_each_tile((constant_table_box*)a.boxes, (constant_u32*)a.tile_begin, a.n_boxes, a.n_tiles,
                [&](int b, constant_table_box* box, const CellTile& at) {
    const int nx = box->nx, ny = box->ny, nz = box->nz;
    constant_link_box* fine = (constant_link_box*)a.refined + b;
    const int32_t scale = fine->scale;
    const int32_t lo_x = fine->lo[0], lo_y = fine->lo[1], lo_z = fine->lo[2];
    const_global_double* cl = (const_global_double*)box->cells[0];
    const_global_double* cp = (const_global_double*)box->cells[HAS_PARENT ? 1 : 0];
    const uint32_t jl = static_cast<uint32_t>(box->jstride[0]), kl = static_cast<uint32_t>(box->kstride[0]);
    const uint32_t jp = static_cast<uint32_t>(box->jstride[1]), kp = static_cast<uint32_t>(box->kstride[1]);
    // One cell of every lane, in converged control flow: cell (i, j, k) of the box, lane 0 holding
    // the lowest i and lane m that + m step.
    auto visit = [&](bool valid, double label, double parent, int i, int j, int k, int step) {
      const bool active = valid && __double_as_longlong(label) != 0ll;
      const bool integer = label >= 1.0 && label <= top && label == __builtin_floor(label);
      const bool linked = !HAS_PARENT || (parent >= 1.0 && parent <= parent_top &&
                                          parent == __builtin_floor(parent));  // false for a NaN
      outside += (active && !integer) ? 1u : 0u;
      orphans += (active && integer && !linked) ? 1u : 0u;
      const bool counted = active && integer && linked;
      const unsigned long long mask = __ballot(counted);
      if (mask == 0ull) return;
      const uint32_t c = counted ? static_cast<uint32_t>(label) : 0u;
      const uint32_t p = (HAS_PARENT && counted) ? static_cast<uint32_t>(parent) : 0u;
      const int first = __ffsll(mask) - 1, last = 63 - __clzll(mask);
      const uint32_t shared = static_cast<uint32_t>(
          __builtin_amdgcn_readlane(static_cast<int>(c), first));
      const bool mixed = __ballot(counted && c != shared) != 0ull;
      if (held.label != 0u && (mixed || shared != held.label)) {
        if (lane == 0u) combine_into<HAS_PARENT>(a, held);
        clear(held, 0u);
      }
      if (mixed) {  // every counted lane for itself
        if (counted) {
          LinkRecord own;
          own.label = c;
          own.lo[0] = lo_x + i * scale;
          own.lo[1] = lo_y + j * scale;
          own.lo[2] = lo_z + k * scale;
          for (int axis = 0; axis < 3; ++axis) own.hi[axis] = own.lo[axis] + (scale - 1);
          own.parent_lo = own.parent_hi = p;
          combine_into<HAS_PARENT>(a, own);
        }
        return;
      }
      if (held.label == 0u) clear(held, shared);
      // lane 0 may hold no cell of the box: unsigned, so that only the counted ends must fit
      const uint32_t i0 = static_cast<uint32_t>(uniform(i)), us = static_cast<uint32_t>(scale);
      const uint32_t ux = static_cast<uint32_t>(lo_x);
      const int32_t x = static_cast<int32_t>(ux + (i0 + static_cast<uint32_t>(first * step)) * us);
      const int32_t x_end = static_cast<int32_t>(
          ux + (i0 + static_cast<uint32_t>(last * step)) * us + (us - 1u));
      const int32_t y = lo_y + uniform(j) * scale, z = lo_z + uniform(k) * scale;
      held.lo[0] = x < held.lo[0] ? x : held.lo[0];
      held.lo[1] = y < held.lo[1] ? y : held.lo[1];
      held.lo[2] = z < held.lo[2] ? z : held.lo[2];
      held.hi[0] = x_end > held.hi[0] ? x_end : held.hi[0];
      held.hi[1] = y + (scale - 1) > held.hi[1] ? y + (scale - 1) : held.hi[1];
      held.hi[2] = z + (scale - 1) > held.hi[2] ? z + (scale - 1) : held.hi[2];
      if (HAS_PARENT) {
        uint32_t least = static_cast<uint32_t>(
            __builtin_amdgcn_readlane(static_cast<int>(p), first));
        uint32_t most = least;
        if (__ballot(counted && p != least) != 0ull) {
          least = wave_min(counted ? p : UINT32_MAX);
          most = wave_max(p);
        }
        held.parent_lo = least < held.parent_lo ? least : held.parent_lo;
        held.parent_hi = most > held.parent_hi ? most : held.parent_hi;
      }
    };
    if (box->paired) {  // both fields: 16-byte aligned cells and even strides (set by the host)
      const int i = at.chunk * kClassifyChunk + (tid & 63) * 2;
      const uint32_t ui = static_cast<uint32_t>(i);
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int row = pass * 4 + (tid >> 6);
        const int j = at.bj * kBrickY + (row & 3), k = at.bk * kBrickZ + (row >> 2);
        const uint32_t uj = static_cast<uint32_t>(j), uk = static_cast<uint32_t>(k);
        const bool valid = i < nx && j < ny && k < nz;
        const bool whole = valid && i + 1 < nx;
        double2_t vl = {0.0, 0.0}, vp = {0.0, 0.0};
        if (whole) {
          vl = *(const_global_double2*)(cl + (ui + uj * jl + uk * kl));
          if (HAS_PARENT) vp = *(const_global_double2*)(cp + (ui + uj * jp + uk * kp));
        } else if (valid) {
          vl.x = cl[ui + uj * jl + uk * kl];
          if (HAS_PARENT) vp.x = cp[ui + uj * jp + uk * kp];
        }
        visit(valid, vl.x, vp.x, i, j, k, 2);
        visit(whole, vl.y, vp.y, i + 1, j, k, 2);
      }
    } else {
      for_each_cell(at, nx, ny, nz, [&](int i, int j, int k, bool valid) {
        double vl = 0.0, vp = 0.0;
        if (valid) {
          const uint32_t ui = static_cast<uint32_t>(i), uj = static_cast<uint32_t>(j);
          const uint32_t uk = static_cast<uint32_t>(k);
          vl = cl[ui + uj * jl + uk * kl];
          if (HAS_PARENT) vp = cp[ui + uj * jp + uk * kp];
        }
        visit(valid, vl, vp, i, j, k, 1);
      });
    }
  });
  if (held.label != 0u && lane == 0u) combine_into<HAS_PARENT>(a, held);

  outside = wave_sum(outside);
  orphans = wave_sum(orphans);
  if (lane == 0u) {
    wave_totals[tid >> 6][0] = outside;
    wave_totals[tid >> 6][1] = orphans;
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

int launch_clumps(const ClumpArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_tiles == 0 || args.n_cells == 0) return AVR_OK;
  const dim3 groups((args.n_tiles + kTilesPerGroup - 1) / kTilesPerGroup), chunks(args.n_chunks);
  hipLaunchKernelGGL(clump_init_kernel, groups, dim3(kThreads), 0, stream, args);
  hipLaunchKernelGGL(clump_merge_kernel, groups, dim3(kThreads), 0, stream, args);
  hipLaunchKernelGGL(clump_flatten_kernel, chunks, dim3(kThreads), 0, stream, args);
  hipLaunchKernelGGL(clump_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, args);
  hipLaunchKernelGGL(clump_rank_kernel, chunks, dim3(kThreads), 0, stream, args);
  hipLaunchKernelGGL(clump_label_kernel, groups, dim3(kThreads), 0, stream, args);
  return check("clump kernels");
}

int launch_clump_table(const ClumpTableArgs& args, bool has_field, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_tiles == 0) return AVR_OK;
  const dim3 groups((args.n_tiles + kTilesPerGroup - 1) / kTilesPerGroup);
  if (has_field) {
    hipLaunchKernelGGL(clump_table_kernel<true>, groups, dim3(kThreads), 0, stream, args);
  } else {
    hipLaunchKernelGGL(clump_table_kernel<false>, groups, dim3(kThreads), 0, stream, args);
  }
  return check("clump_table_kernel");
}

int launch_clump_links(const ClumpLinkArgs& args, bool has_parent, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_tiles == 0) return AVR_OK;
  const dim3 groups((args.n_tiles + kTilesPerGroup - 1) / kTilesPerGroup);
  if (has_parent) {
    hipLaunchKernelGGL(clump_link_kernel<true>, groups, dim3(kThreads), 0, stream, args);
  } else {
    hipLaunchKernelGGL(clump_link_kernel<false>, groups, dim3(kThreads), 0, stream, args);
  }
  return check("clump_link_kernel");
}

}  // namespace avr
