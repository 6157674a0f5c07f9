// Isosurfaces ("Isosurface"): marching tetrahedra over the cubes whose corners are
// cell centres, across boxes and levels, as a triangle soup in a canonical order.
//
//   iso_shell_kernel<S>      the one-cell ghost shell of every box: value, code byte, sample value
//   iso_cubes_kernel<S, E>   E = false: triangles and skipped cubes per chunk of 1024 cube bases
//                            E = true: the same count again, and the triangles at their offsets
//   iso_scan_kernel          one workgroup: exclusive prefix sum of the chunks' counts, T, skipped
//
// Box b enumerates the cube bases (i, j, k) in [-1, n - 1]^3; a base's ordinal is base_begin of
// its box + ((k + 1) (ny + 1) + (j + 1)) (nx + 1) + (i + 1), which is the output order.  One
// workgroup takes one chunk of 1024 consecutive ordinals in four passes of 256, so that a wave
// holds 64 consecutive bases, mostly of one row: the eight corner loads of a lane are rows its
// neighbouring lanes load as well (served by the cache), and a corner outside the box comes from
// the shell.  A triangle's place in the output is its chunk's prefix + the triangles of the lanes
// before its own in the chunk (wave shuffles, LDS across waves) + its number within the cube:
// no atomics, equal arguments give equal bits.
//
// The shell kernel finds a ghost by find_same_or_coarser (avr_level_cells.h) among the boxes the
// host listed for the box.  Only cells of the scene's boxes are ever read.  The shell is a surface
// term: that kernel is kept plain.
//
// Every loop is bounded by a count known at launch.  Arithmetic is IEEE binary64, round to
// nearest, nothing fused (-ffp-contract=off); / is the correctly rounded __ddiv_rn.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_cell_tiles.h"
#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;  // of the one workgroup that scans the chunks' counts
constexpr int kPasses = kIsoChunk / kThreads;
static_assert(kIsoChunk % kThreads == 0, "a chunk is a whole number of passes");

// The six Kuhn tetrahedra of a cube as paths of corner numbers (c = di + 2 dj + 4 dk) from corner
// 0 to corner 7, and whether the path's order of axes is an odd permutation of (x, y, z): the
// orientation of a tetrahedron's triangles flips with it.
constexpr int kTet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7},
                            {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
constexpr uint32_t kTetOdd[6] = {0, 1, 1, 0, 0, 1};
// Bit `mask` (bit n: path vertex n is inside): the last two vertices of the case's triangles are
// swapped in a tetrahedron of even order so that the normal points to the v < value side; in one
// of odd order the other cases are.  Cases 0 and 15 emit nothing.
constexpr uint32_t kSwapEven = 0x4d24u;  // cases 2, 5, 8, 10, 11, 14

// ---- the shell -----------------------------------------------------------------------------------

template <bool HAS_S>
__global__ __launch_bounds__(kThreads) void iso_shell_kernel(const IsoArgs a) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (t >= a.n_shell) return;
  const int b = locate_box(a.shell_begin, a.n_boxes, t);
  const IsoBoxDev& box = a.boxes[b];
  const int nx = box.nx, ny = box.ny, nz = box.nz;
  // the inverse of iso_shell_index
  uint64_t local = t - box.shell_begin;
  const uint64_t ex = static_cast<uint64_t>(nx) + 2, plane = ex * (static_cast<uint64_t>(ny) + 2);
  int i, j, k;
  if (local < 2 * plane) {
    k = local < plane ? -1 : nz;
    if (local >= plane) local -= plane;
    j = static_cast<int>(local / ex) - 1;
    i = static_cast<int>(local % ex) - 1;
  } else {
    local -= 2 * plane;
    const uint64_t rows = static_cast<uint64_t>(nz) * 2 * ex;
    if (local < rows) {
      k = static_cast<int>(local / (2 * ex));
      local %= 2 * ex;
      j = local < ex ? -1 : ny;
      if (local >= ex) local -= ex;
      i = static_cast<int>(local) - 1;
    } else {
      local -= rows;
      i = (local & 1) ? nx : -1;
      local >>= 1;
      j = static_cast<int>(local % static_cast<uint64_t>(ny));
      k = static_cast<int>(local / static_cast<uint64_t>(ny));
    }
  }
  const long long gx = static_cast<long long>(box.lo[0]) + i;
  const long long gy = static_cast<long long>(box.lo[1]) + j;
  const long long gz = static_cast<long long>(box.lo[2]) + k;
  const int level = box.level;
  const uint32_t first = a.candidate_begin[b], last = a.candidate_begin[b + 1];
  // the same level or a coarser one
  const LevelCell found = find_same_or_coarser(a.boxes, a.candidates, first, last, a.levels->ratio,
                                               level, gx, gy, gz);
  double value = 0.0, sample = 0.0;
  if (found.box >= 0) {
    const IsoBoxDev& other = a.boxes[found.box];
    value = other.in[found.i + found.j * static_cast<uint32_t>(other.jstride_in) +
                     found.k * static_cast<uint32_t>(other.kstride_in)];
    if (HAS_S) {
      sample = other.sample[found.i + found.j * static_cast<uint32_t>(other.jstride_sample) +
                            found.k * static_cast<uint32_t>(other.kstride_sample)];
    }
  }
  a.shell_value[t] = value;
  if (HAS_S) a.shell_sample[t] = sample;
  a.shell_code[t] = found.level < 0 ? kIsoAbsent : found.level == level ? kIsoSameLevel : kIsoCoarser;
}

// ---- the cubes -----------------------------------------------------------------------------------

// What a lane holds of its cube.
template <bool HAS_S>
struct Cube {
  double v[8], s[HAS_S ? 8 : 1];
  double p[3][2];  // the positions of the cube's two corner planes along every axis
  int level;
  bool surface;    // every corner present and the cube is this box's
  bool finite;
};

// The cube of base ordinal x < n_bases.  POSITIONS: also where its corners are.
template <bool HAS_S, bool POSITIONS>
__device__ __forceinline__ void load_cube(const IsoArgs& a, uint32_t x, Cube<HAS_S>* cube) {
  const int b = locate_box(a.base_begin, a.n_boxes, x);
  const IsoBoxDev& box = a.boxes[b];
  const int nx = box.nx, ny = box.ny, nz = box.nz;
  const uint32_t local = x - box.base_begin;
  const uint32_t row = static_cast<uint32_t>(nx) + 1u, rows = static_cast<uint32_t>(ny) + 1u;
  const int i = static_cast<int>(local % row) - 1;
  const int j = static_cast<int>((local / row) % rows) - 1;
  const int k = static_cast<int>(local / (row * rows)) - 1;
  const double* in = box.in;
  const double* sample = box.sample;
  const uint32_t ji = static_cast<uint32_t>(box.jstride_in), ki = static_cast<uint32_t>(box.kstride_in);
  const uint32_t js = static_cast<uint32_t>(box.jstride_sample);
  const uint32_t ks = static_cast<uint32_t>(box.kstride_sample);
  const uint64_t shell = box.shell_begin;
  bool present = true, decided = false, owned = false, finite = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int ci = i + (c & 1), cj = j + ((c >> 1) & 1), ck = k + (c >> 2);
    const bool own = ci >= 0 && ci < nx && cj >= 0 && cj < ny && ck >= 0 && ck < nz;
    uint32_t code = kIsoSameLevel;
    if (own) {
      const uint32_t ui = static_cast<uint32_t>(ci), uj = static_cast<uint32_t>(cj);
      const uint32_t uk = static_cast<uint32_t>(ck);
      cube->v[c] = in[ui + uj * ji + uk * ki];
      if (HAS_S) cube->s[c] = sample[ui + uj * js + uk * ks];
    } else {
      const uint64_t at = shell + iso_shell_index(nx, ny, nz, ci, cj, ck);
      cube->v[c] = a.shell_value[at];
      if (HAS_S) cube->s[c] = a.shell_sample[at];
      code = a.shell_code[at];
    }
    present = present && code != kIsoAbsent;
    // the owner holds the lowest-numbered corner that lies in a box of the cube's level
    if (!decided && code == kIsoSameLevel) {
      decided = true;
      owned = own;
    }
    finite = finite && __builtin_isfinite(cube->v[c]);
  }
  cube->surface = present && owned;
  cube->finite = finite;
  cube->level = box.level;
  if (POSITIONS) {
    const int base[3] = {i, j, k};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double dx = a.levels->cell_size[box.level][d];
      const double origin = a.levels->prob_lo[d];
      const long long g = static_cast<long long>(box.lo[d]) + base[d];
      cube->p[d][0] = origin + (static_cast<double>(g) + 0.5) * dx;
      cube->p[d][1] = origin + (static_cast<double>(g + 1) + 0.5) * dx;
    }
  }
}

// Bit c: corner c is inside (v >= value).
template <bool HAS_S>
__device__ __forceinline__ uint32_t inside_mask(const Cube<HAS_S>& cube, double value) {
  uint32_t m = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) m |= (cube.v[c] >= value ? 1u : 0u) << c;
  return m;
}

__device__ __forceinline__ uint32_t tet_mask(uint32_t corners, int tet) {
  return (corners & 1u) | ((corners >> kTet[tet][1]) & 1u) << 1 |
         ((corners >> kTet[tet][2]) & 1u) << 2 | ((corners >> 7) & 1u) << 3;
}

// The triangles of a cube whose corners' inside bits are `corners`: per tetrahedron none with no
// or all four vertices inside, two with two, else one.
__device__ __forceinline__ uint32_t cube_triangles(uint32_t corners) {
  uint32_t n = 0;
#pragma unroll
  for (int tet = 0; tet < 6; ++tet) {
    const uint32_t inside = __popc(tet_mask(corners, tet));
    n += (inside == 0u || inside == 4u) ? 0u : inside == 2u ? 2u : 1u;
  }
  return n;
}

template <typename T>
__device__ __forceinline__ T pick(uint32_t n, T a0, T a1, T a2, T a3) {
  return n == 0u ? a0 : n == 1u ? a1 : n == 2u ? a2 : a3;
}

// Writes the triangles of one cube from `at` on.
template <bool HAS_S>
__device__ __forceinline__ void emit_cube(const IsoArgs& a, const Cube<HAS_S>& cube,
                                          uint32_t corners, unsigned long long at) {
  const double value = a.value;
#pragma unroll
  for (int tet = 0; tet < 6; ++tet) {
    const uint32_t mask = tet_mask(corners, tet);
    const uint32_t inside = __popc(mask);
    if (inside == 0u || inside == 4u) continue;
    const uint32_t c1 = kTet[tet][1], c2 = kTet[tet][2];
    const double w0 = cube.v[0], w1 = cube.v[kTet[tet][1]], w2 = cube.v[kTet[tet][2]], w3 = cube.v[7];
    const double s0 = HAS_S ? cube.s[0] : 0.0, s1 = HAS_S ? cube.s[HAS_S ? kTet[tet][1] : 0] : 0.0;
    const double s2 = HAS_S ? cube.s[HAS_S ? kTet[tet][2] : 0] : 0.0, s3 = HAS_S ? cube.s[HAS_S ? 7 : 0] : 0.0;
    // the path vertices at the ends of the cut edges: vertex e runs from from[e] to to[e]
    const uint32_t outside_mask = ~mask & 15u;
    uint32_t from[4], to[4];
    if (inside == 2u) {
      const uint32_t ia = __ffs(mask) - 1u, ib = 31u - __clz(mask);
      const uint32_t op = __ffs(outside_mask) - 1u, oq = 31u - __clz(outside_mask);
      from[0] = ia; to[0] = op;
      from[1] = ia; to[1] = oq;
      from[2] = ib; to[2] = oq;
      from[3] = ib; to[3] = op;
    } else {
      const uint32_t lone = (inside == 1u ? __ffs(mask) : __ffs(outside_mask)) - 1u;
      from[0] = from[1] = from[2] = from[3] = lone;
      to[0] = lone == 0u ? 1u : 0u;
      to[1] = lone <= 1u ? 2u : 1u;
      to[2] = lone <= 2u ? 3u : 2u;
      to[3] = to[2];
    }
    const uint32_t swap = ((kSwapEven >> mask) & 1u) ^ kTetOdd[tet];
    const uint32_t second = swap ? 2u : 1u, third = swap ? 1u : 2u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e == 3 && inside != 2u) break;
      const uint32_t x = from[e], y = to[e];
      const double wx = pick(x, w0, w1, w2, w3), wy = pick(y, w0, w1, w2, w3);
      const uint32_t cx = pick(x, 0u, c1, c2, 7u), cy = pick(y, 0u, c1, c2, 7u);
      const bool x_low = wx < value;
      const double v_lo = x_low ? wx : wy, v_hi = x_low ? wy : wx;
      const uint32_t c_lo = x_low ? cx : cy, c_hi = x_low ? cy : cx;
      const double t = __ddiv_rn(value - v_lo, v_hi - v_lo);
      double point[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double p_lo = ((c_lo >> d) & 1u) ? cube.p[d][1] : cube.p[d][0];
        const double p_hi = ((c_hi >> d) & 1u) ? cube.p[d][1] : cube.p[d][0];
        point[d] = p_lo + t * (p_hi - p_lo);
      }
      double sampled = 0.0;
      if (HAS_S) {
        const double sx = pick(x, s0, s1, s2, s3), sy = pick(y, s0, s1, s2, s3);
        const double s_lo = x_low ? sx : sy, s_hi = x_low ? sy : sx;
        sampled = s_lo + t * (s_hi - s_lo);
      }
      // vertex e is corner e of triangle (0, 1, 2); vertices 0, 2, 3 make up triangle (0, 2, 3)
      if (e < 3) {
        const unsigned long long slot = at * 3ull + (e == 0 ? 0u : e == 1 ? second : third);
        a.vertices[slot * 3ull + 0] = point[0];
        a.vertices[slot * 3ull + 1] = point[1];
        a.vertices[slot * 3ull + 2] = point[2];
        if (HAS_S) a.samples[slot] = sampled;
      }
      if (inside == 2u && e != 1) {
        const unsigned long long slot = (at + 1ull) * 3ull + (e == 0 ? 0u : e == 2 ? second : third);
        a.vertices[slot * 3ull + 0] = point[0];
        a.vertices[slot * 3ull + 1] = point[1];
        a.vertices[slot * 3ull + 2] = point[2];
        if (HAS_S) a.samples[slot] = sampled;
      }
    }
    const uint8_t level = static_cast<uint8_t>(cube.level);
    a.levels_out[at] = level;
    if (inside == 2u) a.levels_out[at + 1ull] = level;
    at += inside == 2u ? 2ull : 1ull;
  }
}

template <bool HAS_S, bool EMIT>
__global__ __launch_bounds__(kThreads) void iso_cubes_kernel(const IsoArgs a) {
  // emit only what fits: T was written by the scan
  if (EMIT && a.counts[0] > a.capacity) return;
  const double value = a.value;
  const uint32_t first = blockIdx.x * kIsoChunk + threadIdx.x;
  unsigned long long offset = EMIT ? a.chunk_offset[blockIdx.x] : 0ull;
  uint32_t triangles = 0, skipped = 0;
  for (int pass = 0; pass < kPasses; ++pass) {
    const uint32_t x = first + static_cast<uint32_t>(pass) * kThreads;
    Cube<HAS_S> cube;
    uint32_t corners = 0, mine = 0;
    bool cut = false;
    if (x < a.n_bases) {
      load_cube<HAS_S, EMIT>(a, x, &cube);
      corners = inside_mask(cube, value);
      skipped += (cube.surface && !cube.finite) ? 1u : 0u;
      cut = cube.surface && cube.finite && corners != 0u && corners != 255u;
    }
    // a wave none of whose cubes straddles the value has nothing to count
    if (__ballot(cut) != 0ull && cut) mine = cube_triangles(corners);
    uint32_t total;
    const uint32_t before = block_exclusive_sum<kThreads, kPasses + 1>(mine, pass, &total);
    if (EMIT && mine != 0u) emit_cube<HAS_S>(a, cube, corners, offset + before);
    offset += total;
    triangles += total;
  }
  if (!EMIT) {
    uint32_t all_skipped;
    block_exclusive_sum<kThreads, kPasses + 1>(skipped, kPasses, &all_skipped);
    if (threadIdx.x == 0) {
      a.chunk_triangles[blockIdx.x] = triangles;
      a.chunk_skipped[blockIdx.x] = all_skipped;
    }
  }
}

// ---- the scan ------------------------------------------------------------------------------------

// One workgroup: lane t sums the counts of chunks [t per, (t + 1) per), the workgroup scans the
// lanes' sums, and the lane writes the exclusive prefix sums of its chunks (clump_scan_kernel with
// 64-bit sums: a scene holds up to 12 x 2^31 triangles).
__global__ __launch_bounds__(kScanThreads) void iso_scan_kernel(const IsoArgs a) {
  __shared__ unsigned long long wave_sums[kScanThreads / 64][2];
  const uint32_t per = (a.n_chunks + kScanThreads - 1) / kScanThreads;
  const uint32_t first = threadIdx.x * per;
  const uint32_t last = first + per < a.n_chunks ? first + per : a.n_chunks;
  unsigned long long sum = 0, skipped = 0;
  for (uint32_t c = first; c < last; ++c) {
    sum += a.chunk_triangles[c];
    skipped += a.chunk_skipped[c];
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long inclusive = sum, skipped_below = skipped;
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) {
    const unsigned long long below = __shfl_up(inclusive, step, 64);
    const unsigned long long more = __shfl_up(skipped_below, step, 64);
    if (lane >= static_cast<uint32_t>(step)) {
      inclusive += below;
      skipped_below += more;
    }
  }
  if (lane == 63u) {
    wave_sums[wave][0] = inclusive;
    wave_sums[wave][1] = skipped_below;
  }
  __syncthreads();
  unsigned long long running = inclusive - sum, total = 0, total_skipped = 0;
#pragma unroll
  for (uint32_t w = 0; w < kScanThreads / 64; ++w) {
    if (w < wave) running += wave_sums[w][0];
    total += wave_sums[w][0];
    total_skipped += wave_sums[w][1];
  }
  for (uint32_t c = first; c < last; ++c) {
    a.chunk_offset[c] = running;
    running += a.chunk_triangles[c];
  }
  if (threadIdx.x == 0) {
    a.counts[0] = total;
    a.counts[1] = total_skipped;
  }
}

}  // namespace

int launch_isosurface(const IsoArgs& args, bool has_sample, bool emit, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_bases == 0) return AVR_OK;
  const dim3 shell(static_cast<uint32_t>((args.n_shell + kThreads - 1) / kThreads));
  const dim3 chunks(args.n_chunks);
  // the count needs no sample values; only an emitting call has the shell kernel fetch them
  if (has_sample && emit) {
    hipLaunchKernelGGL(iso_shell_kernel<true>, shell, dim3(kThreads), 0, stream, args);
  } else {
    hipLaunchKernelGGL(iso_shell_kernel<false>, shell, dim3(kThreads), 0, stream, args);
  }
  hipLaunchKernelGGL((iso_cubes_kernel<false, false>), chunks, dim3(kThreads), 0, stream, args);
  hipLaunchKernelGGL(iso_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, args);
  if (emit) {
    if (has_sample) {
      hipLaunchKernelGGL((iso_cubes_kernel<true, true>), chunks, dim3(kThreads), 0, stream, args);
    } else {
      hipLaunchKernelGGL((iso_cubes_kernel<false, true>), chunks, dim3(kThreads), 0, stream, args);
    }
  }
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string("isosurface kernels: ") + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

}  // namespace avr
