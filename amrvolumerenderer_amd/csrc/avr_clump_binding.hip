// Clump binding ("Clump binding"): the member cells of the wanted clumps of a label
// field as a list, what is looked up per member, and the gravitational self-energy of member
// segments by direct summation.
//
//   clump_members_kernel       keys (label - 1) << 32 | ordinal of the wanted clumps' cells, at
//                              slots taken from one cursor, in no fixed order
//   clump_member_data_kernel   per key: the cell's level and centre and/or a field's value there
//   clump_pair_kernel          per item the sum of m_i m_j / r_ij over its tile pairs, j > i
//   clump_pair_reduce_kernel   per segment the sum of its items' partials
//
// The members kernel walks the cells in the tiles of avr_cell_tiles.h as clump_table_kernel does
// (16 consecutive tiles per workgroup; 16-byte pairs where the host found a box aligned with even
// strides).  The only atomics of this file are integer additions: the cursor's, one per wave and
// tile, and the totals', one per workgroup.  No floating-point atomic: every sum is taken in an
// order the launch fixes, so equal arguments give equal bits.
//
// Every loop is bounded by a count known at launch.  No lane waits for a value another workgroup
// writes.  Built with -ffp-contract=off: nothing below is fused.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_cell_tiles.h"
#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTilesPerGroup = 16;  // tiles (2048 cells each) per workgroup
constexpr int kRowsPerPass = 2;          // 256 lanes = 2 rows of 128 cells
constexpr int kPasses = 8;               // 16 rows per tile
constexpr int kVisits = 8;               // of a tile by one wave: a cell of every lane each
static_assert(kClumpPairTile == kThreads, "a pair tile is one member per lane");

typedef double __attribute__((address_space(1))) global_double;
typedef const double __attribute__((address_space(1))) const_global_double;
typedef const JointBoxDev __attribute__((address_space(4))) constant_table_box;
typedef const ClumpMemberBoxDev __attribute__((address_space(4))) constant_member_box;
typedef const ClumpPairItem __attribute__((address_space(4))) constant_item;
typedef const IsoLevelsDev __attribute__((address_space(4))) constant_levels;
typedef const uint32_t __attribute__((address_space(4))) constant_u32;
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef const double2_t __attribute__((address_space(1))) const_global_double2;

// ---- the walk over the workgroup's tiles (as avr_clumps.hip's) ---------------------------------

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

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int mask = 32; mask > 0; mask >>= 1) v += __shfl_xor(v, mask, 64);
  return v;
}
// The butterfly: every lane ends with the same bits, whatever the lane.
__device__ __forceinline__ double wave_sum(double v) {
  for (int mask = 32; mask > 0; mask >>= 1) v = v + __shfl_xor(v, mask, 64);
  return v;
}

// ---- members -------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void clump_members_kernel(const ClumpMembersArgs a) {
  __shared__ uint32_t wave_totals[kThreads / 64];
  const int tid = static_cast<int>(threadIdx.x);
  const uint32_t lane = threadIdx.x & 63u;
  const double top = static_cast<double>(a.n_clumps);
  const uint8_t* wanted = a.wanted;
  const unsigned long long capacity = a.capacity;
  unsigned long long* keys = a.keys;
  unsigned long long* cursor = a.cursor;
  uint32_t outside = 0;
  for_each_tile((constant_table_box*)a.boxes, (constant_u32*)a.tile_begin, a.n_boxes, a.n_tiles,
                [&](int b, constant_table_box* box, const CellTile& at) {
    const int nx = box->nx, ny = box->ny, nz = box->nz;
    const uint32_t first_ordinal = ((constant_u32*)a.cell_begin)[b];
    const_global_double* cl = (const_global_double*)box->cells[0];
    const uint32_t jl = static_cast<uint32_t>(box->jstride[0]), kl = static_cast<uint32_t>(box->kstride[0]);
    // A wave's eight visits of the tile -- one cell of every lane each, in converged control flow
    // -- are classified first, and the wave's members of the whole tile then take consecutive
    // slots from the cursor, by visit and then by lane: one addition per wave and tile, by lane 0,
    // an eighth of what one per visit would send to the cursor's one address.
    uint32_t label_of[kVisits], ordinal_of[kVisits];
    unsigned long long members_of[kVisits];
    auto visit = [&](int v, bool valid, double label, int i, int j, int k) {
      const bool active = valid && __double_as_longlong(label) != 0ll;
      const bool integer = label >= 1.0 && label <= top && label == __builtin_floor(label);
      outside += (active && !integer) ? 1u : 0u;
      uint32_t c = 0u;
      bool member = false;
      if (active && integer) {
        c = static_cast<uint32_t>(label) - 1u;
        member = wanted[c] != 0;
      }
      label_of[v] = c;
      ordinal_of[v] =
          first_ordinal +
          (static_cast<uint32_t>(k) * static_cast<uint32_t>(ny) + static_cast<uint32_t>(j)) *
              static_cast<uint32_t>(nx) +
          static_cast<uint32_t>(i);  // read for a member only
      members_of[v] = __ballot(member);
    };
    if (box->paired) {  // 16-byte aligned cells and even strides (set by the host)
      const int i = at.chunk * kClassifyChunk + (tid & 63) * 2;
      const uint32_t ui = static_cast<uint32_t>(i);
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int row = pass * 4 + (tid >> 6);
        const int j = at.bj * kBrickY + (row & 3), k = at.bk * kBrickZ + (row >> 2);
        const uint32_t uj = static_cast<uint32_t>(j), uk = static_cast<uint32_t>(k);
        const bool valid = i < nx && j < ny && k < nz;
        const bool whole = valid && i + 1 < nx;
        double2_t vl = {0.0, 0.0};
        if (whole) {
          vl = *(const_global_double2*)(cl + (ui + uj * jl + uk * kl));
        } else if (valid) {
          vl.x = cl[ui + uj * jl + uk * kl];
        }
        visit(2 * pass, valid, vl.x, i, j, k);
        visit(2 * pass + 1, whole, vl.y, i + 1, j, k);
      }
    } else {
      int pass = 0;
      for_each_cell(at, nx, ny, nz, [&](int i, int j, int k, bool valid) {
        double vl = 0.0;
        if (valid) {
          vl = cl[static_cast<uint32_t>(i) + static_cast<uint32_t>(j) * jl +
                  static_cast<uint32_t>(k) * kl];
        }
        visit(pass++, valid, vl, i, j, k);
      });
    }
    uint32_t found = 0u;
#pragma unroll
    for (int v = 0; v < kVisits; ++v) found += static_cast<uint32_t>(__popcll(members_of[v]));
    if (found == 0u) return;  // the whole wave
    unsigned long long next = 0ull;
    if (lane == 0u) next = atomicAdd(cursor, static_cast<unsigned long long>(found));
    next = __shfl(next, 0, 64);
#pragma unroll
    for (int v = 0; v < kVisits; ++v) {
      const unsigned long long mask = members_of[v];
      const uint32_t before = __builtin_amdgcn_mbcnt_hi(
          static_cast<uint32_t>(mask >> 32),
          __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
      const unsigned long long slot = next + before;
      if (((mask >> lane) & 1ull) != 0ull && slot < capacity) {
        keys[slot] = (static_cast<unsigned long long>(label_of[v]) << 32) | ordinal_of[v];
      }
      next += static_cast<unsigned long long>(__popcll(mask));
    }
  });

  outside = wave_sum(outside);
  if (lane == 0u) wave_totals[tid >> 6] = outside;
  __syncthreads();
  if (tid == 0) {
    uint32_t total = 0;
    for (int w = 0; w < kThreads / 64; ++w) total += wave_totals[w];
    if (total != 0u) atomicAdd(&a.totals[0], static_cast<unsigned long long>(total));
  }
}

// ---- per member ----------------------------------------------------------------------------------

// One lane per key.  The key's ordinal names the box (a search of the boxes' first ordinals, at
// most ceil(log2 n_boxes) steps) and the cell in it.  A key whose ordinal names no cell -- the
// caller's keys are taken as they are -- reads nothing and gives level 255 and NaNs.
__global__ __launch_bounds__(kThreads) void clump_member_data_kernel(const ClumpMemberDataArgs a) {
  const uint32_t at = blockIdx.x * static_cast<uint32_t>(kThreads) + threadIdx.x;
  if (at >= a.n_members) return;
  const uint32_t n = a.n_members;
  const uint32_t ordinal = static_cast<uint32_t>(a.keys[at]);
  const bool known = ordinal < a.n_cells;
  uint32_t level = 255u;
  const double nan = __builtin_nan("");
  double centre[3] = {nan, nan, nan};
  double value = nan;
  if (known) {
    constant_u32* cell_begin = (constant_u32*)a.cell_begin;
    const int b = locate_box(cell_begin, a.n_boxes, ordinal);
    constant_member_box* box = (constant_member_box*)a.boxes + b;
    const uint32_t nx = static_cast<uint32_t>(box->nx), ny = static_cast<uint32_t>(box->ny);
    uint32_t local = ordinal - cell_begin[b];
    const uint32_t i = local % nx;
    local /= nx;
    const uint32_t j = local % ny, k = local / ny;
    level = static_cast<uint32_t>(box->level);
    if (a.centres != nullptr) {
      constant_levels* levels = (constant_levels*)a.levels;
      const int32_t index[3] = {box->lo[0] + static_cast<int32_t>(i),
                                box->lo[1] + static_cast<int32_t>(j),
                                box->lo[2] + static_cast<int32_t>(k)};
#pragma unroll
      for (int axis = 0; axis < 3; ++axis) {
        const double offset = (static_cast<double>(index[axis]) + 0.5) * levels->cell_size[level][axis];
        centre[axis] = levels->prob_lo[axis] + offset;
      }
    }
    if (a.values != nullptr) {
      const_global_double* cells = (const_global_double*)box->field;
      value = cells[i + j * static_cast<uint32_t>(box->jstride) +
                    k * static_cast<uint32_t>(box->kstride)];
    }
  }
  if (a.centres != nullptr) {
#pragma unroll
    for (uint32_t axis = 0; axis < 3; ++axis) {
      a.centres[static_cast<size_t>(axis) * n + at] = centre[axis];
    }
    a.levels_out[at] = static_cast<uint8_t>(level);
  }
  if (a.values != nullptr) a.values[at] = value;
}

// ---- pairs ---------------------------------------------------------------------------------------

struct alignas(32) PairMember {
  double x, y, z, m;
};

// One item: lane t holds member i = 256 i_tile + t of the segment in registers and adds, j tile by
// j tile and j ascending, m_i m_j / r_ij of every member j > i of the item's j tiles; a j tile is
// staged in LDS (8 KB) and read by all lanes at once, one address per read.  A lane past the
// segment's end and a staged slot past it hold m = 0 at the origin, and every term that is not a
// pair i < j < count of the segment is replaced by 0 / 1 before the division: no 0 / 0 arises, and
// +0.0 added leaves a sum as it is.  r_ij = sqrt((dx dx + dy dy) + dz dz); the product, the
// square root and the quotient are IEEE binary64 operations, correctly rounded.
__global__ __launch_bounds__(kThreads) void clump_pair_kernel(const ClumpPairArgs a) {
  __shared__ PairMember staged[kThreads];
  __shared__ double wave_sums[kThreads / 64];
  const uint32_t tid = threadIdx.x;
  constant_item* item = (constant_item*)a.items + blockIdx.x;
  const uint32_t begin = item->begin, count = item->count, i_tile = item->i_tile;
  const uint32_t j_first = item->j_tiles & 0xffffu, j_count = item->j_tiles >> 16;
  const_global_double* gx = (const_global_double*)a.x + begin;
  const_global_double* gy = (const_global_double*)a.y + begin;
  const_global_double* gz = (const_global_double*)a.z + begin;
  const_global_double* gm = (const_global_double*)a.m + begin;
  const uint32_t i = i_tile * kClumpPairTile + tid;
  const bool has_i = i < count;
  double xi = 0.0, yi = 0.0, zi = 0.0, mi = 0.0;
  if (has_i) {
    xi = gx[i];
    yi = gy[i];
    zi = gz[i];
    mi = gm[i];
  }
  double sum = 0.0;
  for (uint32_t t = 0; t < j_count; ++t) {
    const uint32_t j_tile = j_first + t;
    const uint32_t j = j_tile * kClumpPairTile + tid;
    PairMember mine = {0.0, 0.0, 0.0, 0.0};
    if (j < count) {
      mine.x = gx[j];
      mine.y = gy[j];
      mine.z = gz[j];
      mine.m = gm[j];
    }
    __syncthreads();  // the tile before has been read by every lane
    staged[tid] = mine;
    __syncthreads();
    // the staged slots that hold a member j > i of this lane: [from, until)
    const uint32_t left = count - j_tile * kClumpPairTile;  // > 0: the tile holds a member
    const uint32_t until = has_i ? (left < kClumpPairTile ? left : kClumpPairTile) : 0u;
    const uint32_t from = j_tile == i_tile ? tid + 1u : 0u;
#pragma unroll 4
    for (uint32_t s = 0; s < kClumpPairTile; ++s) {
      const PairMember other = staged[s];
      const double dx = xi - other.x, dy = yi - other.y, dz = zi - other.z;
      const double r2 = (dx * dx + dy * dy) + dz * dz;
      const bool pair = s >= from && s < until;
      const double above = pair ? mi * other.m : 0.0;
      const double below = pair ? __builtin_sqrt(r2) : 1.0;
      sum = sum + above / below;
    }
  }
  sum = wave_sum(sum);
  if ((tid & 63u) == 0u) wave_sums[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0u) {
    double total = wave_sums[0];
    for (int w = 1; w < kThreads / 64; ++w) total = total + wave_sums[w];
    a.partial[blockIdx.x] = total;
  }
}

// One wave per segment: lane t adds the segment's partials t, t + 64, ... in that order, then the
// butterfly; a segment without items (fewer than two members) gives +0.0.
__global__ __launch_bounds__(kThreads) void clump_pair_reduce_kernel(const ClumpPairArgs a) {
  const uint32_t segment = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (segment >= a.n_segments) return;  // the whole wave
  const uint32_t lane = threadIdx.x & 63u;
  constant_u32* partial_begin = (constant_u32*)a.partial_begin;
  const uint32_t begin = partial_begin[segment], end = partial_begin[segment + 1];
  const_global_double* partial = (const_global_double*)a.partial;
  double sum = 0.0;
  for (uint32_t p = begin + lane; p < end; p += 64u) sum = sum + partial[p];
  sum = wave_sum(sum);
  if (lane == 0u) a.w[segment] = sum;
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

int launch_clump_members(const ClumpMembersArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_tiles == 0) return AVR_OK;
  const dim3 groups((args.n_tiles + kTilesPerGroup - 1) / kTilesPerGroup);
  hipLaunchKernelGGL(clump_members_kernel, groups, dim3(kThreads), 0, stream, args);
  return check("clump_members_kernel");
}

int launch_clump_member_data(const ClumpMemberDataArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_members == 0) return AVR_OK;
  const dim3 groups((args.n_members + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(clump_member_data_kernel, groups, dim3(kThreads), 0, stream, args);
  return check("clump_member_data_kernel");
}

int launch_clump_pairs(const ClumpPairArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_segments == 0) return AVR_OK;
  if (args.n_items != 0) {
    hipLaunchKernelGGL(clump_pair_kernel, dim3(args.n_items), dim3(kThreads), 0, stream, args);
  }
  const dim3 waves((args.n_segments + kThreads / 64 - 1) / (kThreads / 64));
  hipLaunchKernelGGL(clump_pair_reduce_kernel, waves, dim3(kThreads), 0, stream, args);
  return check("clump pair kernels");
}

}  // namespace avr
