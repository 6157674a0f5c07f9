// Rays ("Rays"): the leaf cells that a segment A -> B crosses, in order, with the
// entry and exit parameters, the level and the raw value of each, and the exact column integral
// sum value * ds that comes with them.
//
//   rays_kernel<MODE>    one lane per ray; MODE: what the one walk writes
//
// Two passes over the identical walk: the count pass writes every ray's count, status and clipped
// span, the host takes the exclusive scan, and the emit pass writes ray s's segments into the
// slots [offsets[s], offsets[s + 1]) that it owns -- never past that range nor past n_segments,
// whatever the offsets hold -- and the two sums.  The sums pass ("Off-axis
// projection") is the same walk once: per ray the count pass's three outputs and, accumulated in
// walk order over the leaf segments, sum w, sum v w and sum w over the finite values -- with a
// weight field sum (v q) w, sum q w and sum w where both are finite -- each stored once at the
// end of the walk and nothing per segment.  A lane keeps its cell (the geometry level l and
// the index G), steps through the face the ray leaves it by and finds the next cell through the
// streamlines' locator: the list of the block that holds G mapped to level 0, finest level first,
// walked once, with the candidate index of a level worked out when the walk reaches a box of it.
// Only cells of the scene's boxes are ever read.  Workgroups are one wave, so a wave's slot comes
// back when its own last ray is done; the segment stores are scattered, each lane to its own
// packed range.
//
// Ray transfer ("Ray transfer") is three further modes of the one walk: the
// walk's field is the source function S, and per leaf segment the opacity a, the bin field g and the
// width s are read at the same cell as the sums pass reads its weight.  Per counted segment and
// channel c, nearest segment first,
//   dtau = ((a * w) * share) * rdv[c]
//   I[c] = I[c] + (S * (-expm1(-dtau))) * exp(-tau[c]),  then  tau[c] = tau[c] + dtau
// with the velocity cube's shares (avr_velocity_cube.hip).  Grey: one channel, share and rdv 1, I
// and tau in registers, no LDS.  With channels the accumulator a segment adds to is chosen by its
// g, so a one-wave workgroup keeps I and tau of one chunk of channels (the grid's y index) in
// dynamic LDS as [channel][2][lane] -- a wave's lanes on consecutive banks, each lane at its own
// entries only: no barrier but the one after the tables, no atomic -- behind the chunk's edges and
// reciprocals.  Every chunk repeats the walk for its own channels; a channel's arithmetic does not
// depend on the chunk that holds it.  Chunk 0 writes the per-ray outputs and under and over; every
// chunk its channels, one coalesced store per channel and array, [channel][ray].
//
// Every loop is bounded by a count known at launch: max_trips, the levels, a block's list, a
// chunk's channels (the LDS size is the plan's, ray_transfer_lds_bytes, for lanes of 64).  No
// atomics: equal arguments give equal bits.  Arithmetic is IEEE binary64, round to nearest,
// nothing fused (-ffp-contract=off); / and sqrt are the correctly rounded __ddiv_rn and
// __dsqrt_rn.  A maximum or minimum is written as the comparison the definition names.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 64;  // one wave: its slot is free again when its own last ray has ended
constexpr int kRayCount = 0, kRayEmit = 1, kRaySums = 2;  // rays_kernel's modes
constexpr int kRayGrey = 3, kRaySharp = 4, kRayBroadened = 5;  // ... of a transfer
static_assert(kRayGrey + kTransferSharp == kRaySharp && kRayGrey + kTransferBroadened == kRayBroadened,
              "a form is a mode");

typedef double __attribute__((address_space(3))) lds_double;

__device__ __forceinline__ int floor_div(int a, int r) {
  const int q = a / r;
  return (a % r != 0 && a < 0) ? q - 1 : q;
}

// floor(q) within [lo, hi]; lo for a q that is not finite.
__device__ __forceinline__ int clamped_floor(double q, int lo, int hi) {
  if (!__builtin_isfinite(q)) return lo;
  const double f = floor(q);
  if (f < static_cast<double>(lo)) return lo;
  if (f > static_cast<double>(hi)) return hi;
  return static_cast<int>(f);
}

// T(l, d, g): the parameter at which the ray meets the plane of index g of level l along axis d.
__device__ __forceinline__ double plane_t(const IsoLevelsDev& levels, int l, int d, int g, double a,
                                          double dir) {
  const double x = levels.prob_lo[d] + static_cast<double>(g) * levels.cell_size[l][d];
  return __ddiv_rn(x - a, dir);
}

// The cell a trip crosses: its geometry (l, g), the recorded level (-1: absent) and its value's
// address (null: absent); box: the box that holds it, set with the address.
struct RayCell {
  int l, level;
  int g[3];
  const double* at;
  int box;
};

// The candidate of level m for the level-c index g taken to hold p: below c the index mapped down,
// above c the point's index clamped to the children of g.
__device__ __forceinline__ void candidate(const IsoLevelsDev& levels, int c, const int g[3],
                                          const double p[3], int m, int out[3]) {
  if (m <= c) {
    out[0] = g[0];
    out[1] = g[1];
    out[2] = g[2];
    for (int k = c; k > m; --k) {
      const int r = levels.ratio[k - 1];
      out[0] = floor_div(out[0], r);
      out[1] = floor_div(out[1], r);
      out[2] = floor_div(out[2], r);
    }
    return;
  }
  int refine = 1;  // r_c ... r_(m - 1): at most 2^30, and g's children stay inside [-2^30, 2^30)
  for (int k = c; k < m; ++k) refine *= levels.ratio[k];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double q = __ddiv_rn(p[d] - levels.prob_lo[d], levels.cell_size[m][d]);
    const int first = g[d] * refine;
    out[d] = clamped_floor(q, first, first + (refine - 1));
  }
}

// Locate(c, g, p); z: g mapped to level 0, inside [bound_lo, bound_hi].
__device__ __forceinline__ RayCell locate(const RayArgs& a, const IsoLevelsDev& levels, int c,
                                          const int g[3], const int z[3], const double p[3]) {
  RayCell cell;
  const StreamLocatorDev& locator = a.locator;
  const uint32_t bx = (static_cast<uint32_t>(z[0]) - static_cast<uint32_t>(locator.origin[0])) >> locator.shift;
  const uint32_t by = (static_cast<uint32_t>(z[1]) - static_cast<uint32_t>(locator.origin[1])) >> locator.shift;
  const uint32_t bz = (static_cast<uint32_t>(z[2]) - static_cast<uint32_t>(locator.origin[2])) >> locator.shift;
  const uint32_t n0 = static_cast<uint32_t>(locator.n[0]), n1 = static_cast<uint32_t>(locator.n[1]);
  uint32_t first = 0, last = 0;
  if (bx < n0 && by < n1 && bz < static_cast<uint32_t>(locator.n[2])) {
    const uint32_t block = (bz * n1 + by) * n0 + bx;
    first = a.block_begin[block];
    last = a.block_begin[block + 1];
  }
  int at = -1;  // the level cell.g is the candidate of
  for (uint32_t e = first; e < last; ++e) {
    const int b = a.block_boxes[e];
    const CoverBoxDev& box = a.boxes[b];
    const int m = box.level;
    if (m != at) {
      candidate(levels, c, g, p, m, cell.g);
      at = m;
    }
    // the unsigned difference also refuses an index below the box's first
    const uint32_t i = static_cast<uint32_t>(cell.g[0]) - static_cast<uint32_t>(box.lo[0]);
    const uint32_t j = static_cast<uint32_t>(cell.g[1]) - static_cast<uint32_t>(box.lo[1]);
    const uint32_t k = static_cast<uint32_t>(cell.g[2]) - static_cast<uint32_t>(box.lo[2]);
    if (i < static_cast<uint32_t>(box.nx) && j < static_cast<uint32_t>(box.ny) &&
        k < static_cast<uint32_t>(box.nz)) {
      cell.l = cell.level = m;
      cell.box = b;
      cell.at = box.cells + (i + j * static_cast<uint32_t>(box.jstride) +
                             k * static_cast<uint32_t>(box.kstride));
      return cell;
    }
  }
  // absent: the finest level's geometry
  const int finest = a.n_levels - 1;
  if (at != finest) candidate(levels, c, g, p, finest, cell.g);
  cell.l = finest;
  cell.level = -1;
  cell.box = -1;
  cell.at = nullptr;
  return cell;
}

// A lane's share of a transfer.
struct TransferLane {
  const RayTransferPart* args;
  lds_double* acc;          // the lane's accumulators, [channel][2][lane] from here; grey: unused
  const lds_double* edges;  // the chunk's count + 1 edges
  const lds_double* rdv;    // the chunk's count reciprocals
  int first, count;         // the chunk's channels
  bool head, tail;          // the chunk holds channel 0 / the last channel
};

// The value of the cell `cell` in another scene's table: box by box the walk's boxes.
__device__ __forceinline__ double same_cell(const CoverBoxDev* boxes, const RayCell& cell) {
  const CoverBoxDev& other = boxes[cell.box];
  const uint32_t i = static_cast<uint32_t>(cell.g[0]) - static_cast<uint32_t>(other.lo[0]);
  const uint32_t j = static_cast<uint32_t>(cell.g[1]) - static_cast<uint32_t>(other.lo[1]);
  const uint32_t k = static_cast<uint32_t>(cell.g[2]) - static_cast<uint32_t>(other.lo[2]);
  return other.cells[i + j * static_cast<uint32_t>(other.jstride) +
                     k * static_cast<uint32_t>(other.kstride)];
}

__device__ __forceinline__ double clamped_erf(double a) {
  return (a <= -6.0) ? -1.0 : (a >= 6.0) ? 1.0 : erf(a);
}
__device__ __forceinline__ double profile_argument(double edge, double g, double s) {
  return __ddiv_rn(edge - g, s) * 0.70710678118654752440;
}

// One counted segment's step of one channel: its intensity at p[0], its optical depth at p[kThreads].
__device__ __forceinline__ void add_channel(lds_double* p, double source, double dtau) {
  const double tau = p[kThreads];
  p[0] = p[0] + (source * (-expm1(-dtau))) * exp(-tau);
  p[kThreads] = tau + dtau;
}

// One leaf segment of length w whose source function is `source`.  Returns whether it counts.
template <int MODE>
__device__ __forceinline__ bool transfer_segment(const TransferLane& x, const RayCell& cell,
                                                 double source, double w, double* intensity,
                                                 double* tau, double* under, double* over) {
  const RayTransferPart& t = *x.args;
  const double opacity = same_cell(t.opacity_boxes, cell);
  bool counts = __builtin_isfinite(source) & __builtin_isfinite(opacity) & (opacity >= 0.0);
  double g = 0.0, s = 0.0;
  if (MODE != kRayGrey) {
    g = same_cell(t.bin_boxes, cell);
    counts = counts & __builtin_isfinite(g);
  }
  if (MODE == kRayBroadened) {
    s = same_cell(t.width_boxes, cell);
    counts = counts & __builtin_isfinite(s) & (s >= 0.0);
  }
  if (!counts) return false;
  const double aw = opacity * w;
  if (MODE == kRayGrey) {  // share 1, rdv 1: dtau is a w
    *intensity = *intensity + (source * (-expm1(-aw))) * exp(-*tau);
    *tau = *tau + aw;
    return true;
  }
  if (MODE == kRaySharp || s == 0.0) {  // share 1 for one of the channels, under or over
    if (g < t.lo) {
      if (x.head) *under = *under + aw;
    } else if (g > t.hi) {
      if (x.head) *over = *over + aw;
    } else if (g >= x.edges[0] && (x.tail || g < x.edges[x.count])) {
      // the largest channel of the chunk whose lower edge is not above g
      int first = 0, last = x.count;
      while (last - first > 1) {
        const int mid = (first + last) >> 1;
        if (x.edges[mid] <= g) {
          first = mid;
        } else {
          last = mid;
        }
      }
      add_channel(x.acc + first * (2 * kThreads), source, aw * x.rdv[first]);
    }
    return true;
  }
  if (x.head) {
    *under = *under + aw * (0.5 * (clamped_erf(profile_argument(t.lo, g, s)) + 1.0));
    *over = *over + aw * (0.5 * (1.0 - clamped_erf(profile_argument(t.hi, g, s))));
  }
  // the argument does not decrease with the edge: a chunk wholly outside the window has shares of 0
  const double a_first = profile_argument(x.edges[0], g, s);
  if (a_first >= 6.0) return true;
  if (profile_argument(x.edges[x.count], g, s) <= -6.0) return true;
  double below = clamped_erf(a_first);
  for (int at = 0; at < x.count; ++at) {
    const double above = clamped_erf(profile_argument(x.edges[at + 1], g, s));
    const double share = 0.5 * (above - below);
    // a share of 0 adds +-0 to sums that are never -0
    if (share != 0.0) add_channel(x.acc + at * (2 * kThreads), source, (aw * share) * x.rdv[at]);
    below = above;
  }
  return true;
}

// The grid's y index numbers the chunks of a.transfer.chunk channels; only the sharp and the
// broadened mode have more than one, and LDS.
template <int MODE>
__global__ __launch_bounds__(kThreads) void rays_kernel(const RayArgs a) {
  TransferLane x;
  if constexpr (MODE >= kRayGrey) {
    extern __shared__ double transfer_lds[];  // [edges: chunk + 1][rdv: chunk][chunk][2][lane]
    const RayTransferPart& t = a.transfer;
    x.args = &t;
    x.acc = nullptr;
    x.edges = x.rdv = nullptr;
    x.first = 0;
    x.count = 1;
    x.head = x.tail = true;
    if (MODE != kRayGrey) {
      lds_double* lds = (lds_double*)transfer_lds;
      x.first = static_cast<int>(blockIdx.y) * t.chunk;
      const int left = t.n_channels - x.first;
      x.count = left < t.chunk ? left : t.chunk;
      x.head = blockIdx.y == 0;
      x.tail = x.first + x.count == t.n_channels;
      for (int i = static_cast<int>(threadIdx.x); i <= x.count; i += kThreads) {
        lds[i] = t.edges[x.first + i];
      }
      for (int i = static_cast<int>(threadIdx.x); i < x.count; i += kThreads) {
        lds[t.chunk + 1 + i] = t.rdv[x.first + i];
      }
      __syncthreads();  // the workgroup's only barrier: before any lane leaves
      x.edges = lds;
      x.rdv = lds + (t.chunk + 1);
      x.acc = lds + (2 * t.chunk + 1) + threadIdx.x;
    }
  }
  const uint32_t ray = blockIdx.x * kThreads + threadIdx.x;
  if (ray >= a.n_rays) return;
  const IsoLevelsDev& levels = *a.levels;
  double A[3], D[3];
  bool finite = true, still = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    A[d] = a.start[ray * 3ull + d];
    const double b = a.end[ray * 3ull + d];
    finite = finite && __builtin_isfinite(A[d]) && __builtin_isfinite(b);
    D[d] = b - A[d];
    still = still && D[d] == 0.0;
  }
  const double nan = __builtin_nan("");
  uint32_t count = 0, status = kRayTruncated;
  double t_enter = 0.0, t_leave = 1.0;
  // the emit pass: the slots [slot, slot_end) are the ray's own
  unsigned long long slot = 0, slot_end = 0;
  double integral = 0.0, covered = 0.0, length = 0.0;
  double weight = 0.0, counted = 0.0;  // the sums pass
  double tau = 0.0, under = 0.0, over = 0.0;  // transfer: with `integral` as the grey intensity
  if constexpr (MODE >= kRaySharp) {
    for (int at = 0; at < x.count; ++at) {
      x.acc[at * (2 * kThreads)] = 0.0;
      x.acc[at * (2 * kThreads) + kThreads] = 0.0;
    }
  }
  if (MODE == kRayEmit) {
    const long long begin = a.offsets[ray], end = a.offsets[ray + 1ull];
    if (begin >= 0 && begin <= end && static_cast<unsigned long long>(end) <= a.n_segments) {
      slot = static_cast<unsigned long long>(begin);
      slot_end = static_cast<unsigned long long>(end);
    }
  }
  if (MODE != kRayCount) length = __dsqrt_rn((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
  if (!finite || still) {
    status = kRayInvalid;
  } else if (a.locator.n[0] == 0) {
    status = kRayMiss;  // a scene without cells
  } else {
    // the clip against the level-0 box
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int lo = a.bound_lo[d], hi = a.bound_hi[d] + 1;
      if (D[d] == 0.0) {
        const double x_lo = levels.prob_lo[d] + static_cast<double>(lo) * levels.cell_size[0][d];
        const double x_hi = levels.prob_lo[d] + static_cast<double>(hi) * levels.cell_size[0][d];
        if (!(x_lo <= A[d] && A[d] < x_hi)) status = kRayMiss;
      } else {
        const double t_near = plane_t(levels, 0, d, D[d] > 0.0 ? lo : hi, A[d], D[d]);
        const double t_far = plane_t(levels, 0, d, D[d] > 0.0 ? hi : lo, A[d], D[d]);
        t_enter = t_near > t_enter ? t_near : t_enter;
        t_leave = t_far < t_leave ? t_far : t_leave;
      }
    }
    if (!(t_enter < t_leave)) status = kRayMiss;
  }
  if (status == kRayTruncated) {
    // the walk
    double t_cur = t_enter;
    double p[3];
    int c = 0, g[3], z[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      p[d] = A[d] + t_cur * D[d];
      const double q = __ddiv_rn(p[d] - levels.prob_lo[d], levels.cell_size[0][d]);
      g[d] = z[d] = clamped_floor(q, a.bound_lo[d], a.bound_hi[d]);
    }
    for (uint32_t trip = 0; trip < a.max_trips; ++trip) {
      const RayCell cell = locate(a, levels, c, g, z, p);
      double t_out = 0.0;
      int exit_axis = -1;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        if (D[d] != 0.0) {
          const double t = plane_t(levels, cell.l, d, D[d] > 0.0 ? cell.g[d] + 1 : cell.g[d], A[d],
                                   D[d]);
          if (exit_axis < 0 || t < t_out) {
            t_out = t;
            exit_axis = d;
          }
        }
      }
      const double ahead = t_out > t_cur ? t_out : t_cur;
      const double t_next = ahead < t_leave ? ahead : t_leave;
      if (t_next > t_cur) {
        if (MODE == kRayEmit) {
          const unsigned long long at = slot + count;
          if (at < slot_end) {
            const double v = cell.at != nullptr ? *cell.at : nan;
            a.t0[at] = t_cur;
            a.t1[at] = t_next;
            a.level[at] = static_cast<int8_t>(cell.level);
            a.value[at] = v;
            if (cell.at != nullptr) {
              const double w = (t_next - t_cur) * length;
              covered = covered + w;
              if (__builtin_isfinite(v)) integral = integral + v * w;
            }
          }
        }
        if (MODE == kRaySums && cell.at != nullptr) {
          const double v = *cell.at;
          const double w = (t_next - t_cur) * length;
          covered = covered + w;
          if (a.weight_boxes == nullptr) {
            if (__builtin_isfinite(v)) {
              integral = integral + v * w;
              counted = counted + w;
            }
          } else {
            // the same cell of the weight's box, whose level, dims and index are the field's
            const CoverBoxDev& other = a.weight_boxes[cell.box];
            const uint32_t i = static_cast<uint32_t>(cell.g[0]) - static_cast<uint32_t>(other.lo[0]);
            const uint32_t j = static_cast<uint32_t>(cell.g[1]) - static_cast<uint32_t>(other.lo[1]);
            const uint32_t k = static_cast<uint32_t>(cell.g[2]) - static_cast<uint32_t>(other.lo[2]);
            const double q = other.cells[i + j * static_cast<uint32_t>(other.jstride) +
                                         k * static_cast<uint32_t>(other.kstride)];
            if (__builtin_isfinite(v) && __builtin_isfinite(q)) {
              integral = integral + (v * q) * w;
              weight = weight + q * w;
              counted = counted + w;
            }
          }
        }
        if constexpr (MODE >= kRayGrey) {
          if (cell.at != nullptr) {
            const double w = (t_next - t_cur) * length;
            covered = covered + w;
            if (transfer_segment<MODE>(x, cell, *cell.at, w, &integral, &tau, &under, &over)) {
              counted = counted + w;
            }
          }
        }
        ++count;
      }
      if (!(t_out < t_leave)) {
        status = kRayComplete;
        break;
      }
      // through the exit face; a step out of the level-0 box happens by rounding only
      c = cell.l;
      g[0] = cell.g[0];
      g[1] = cell.g[1];
      g[2] = cell.g[2];
      const double along = exit_axis == 0 ? D[0] : (exit_axis == 1 ? D[1] : D[2]);
      const int step = along > 0.0 ? 1 : -1;
      if (exit_axis == 0) g[0] += step;
      if (exit_axis == 1) g[1] += step;
      if (exit_axis == 2) g[2] += step;
      z[0] = g[0];
      z[1] = g[1];
      z[2] = g[2];
      for (int m = c; m > 0; --m) {
        const int r = levels.ratio[m - 1];
        z[0] = floor_div(z[0], r);
        z[1] = floor_div(z[1], r);
        z[2] = floor_div(z[2], r);
      }
      if (z[0] < a.bound_lo[0] || z[0] > a.bound_hi[0] || z[1] < a.bound_lo[1] ||
          z[1] > a.bound_hi[1] || z[2] < a.bound_lo[2] || z[2] > a.bound_hi[2]) {
        status = kRayComplete;
        break;
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) p[d] = A[d] + t_next * D[d];
      t_cur = t_next;
    }
  }
  if (MODE == kRayEmit || MODE == kRaySums) {
    a.integral[ray] = integral;
    a.covered[ray] = covered;
  }
  if (MODE == kRaySums) {
    if (a.weight_boxes != nullptr) a.weight[ray] = weight;
    a.counted[ray] = counted;
  }
  if constexpr (MODE >= kRayGrey) {
    const RayTransferPart& t = *x.args;
    const size_t n = a.n_rays;
    if (MODE == kRayGrey) {
      t.intensity[ray] = integral;
      t.tau[ray] = tau;
    } else {
      double* intensity = t.intensity + static_cast<size_t>(x.first) * n + ray;
      double* depth = t.tau + static_cast<size_t>(x.first) * n + ray;
      for (int at = 0; at < x.count; ++at) {
        intensity[static_cast<size_t>(at) * n] = x.acc[at * (2 * kThreads)];
        depth[static_cast<size_t>(at) * n] = x.acc[at * (2 * kThreads) + kThreads];
      }
    }
    if (x.head) {
      a.counted[ray] = counted;
      a.covered[ray] = covered;
      if (MODE != kRayGrey) {
        t.outside[ray] = under;
        t.outside[n + ray] = over;
      }
    }
  }
  // the count pass's three outputs; of a transfer's chunks the first writes them
  if (MODE != kRayEmit && (MODE < kRayGrey || x.head)) {
    const bool walked = status == kRayComplete || status == kRayTruncated;
    a.counts[ray] = count;
    a.status[ray] = static_cast<uint8_t>(status);
    a.span[ray * 2ull + 0] = walked ? t_enter : nan;
    a.span[ray * 2ull + 1] = walked ? t_leave : nan;
  }
}

template <int MODE>
int launch_mode(const RayArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_rays == 0) return AVR_OK;
  const dim3 grid(static_cast<uint32_t>((static_cast<uint64_t>(args.n_rays) + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(rays_kernel<MODE>, grid, dim3(kThreads), 0, stream, args);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string("rays kernel: ") + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

}  // namespace

int launch_rays(const RayArgs& args, bool emit, void* stream) {
  return emit ? launch_mode<kRayEmit>(args, stream) : launch_mode<kRayCount>(args, stream);
}

int launch_ray_sums(const RayArgs& args, void* stream) {
  return launch_mode<kRaySums>(args, stream);
}

int launch_ray_transfer(const RayArgs& args, int form, uint32_t n_chunks, size_t bytes,
                        void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_rays == 0) return AVR_OK;
  const dim3 grid(static_cast<uint32_t>((static_cast<uint64_t>(args.n_rays) + kThreads - 1) / kThreads),
                  n_chunks);
  if (form == kTransferGrey) {
    hipLaunchKernelGGL(rays_kernel<kRayGrey>, grid, dim3(kThreads), bytes, stream, args);
  } else if (form == kTransferSharp) {
    hipLaunchKernelGGL(rays_kernel<kRaySharp>, grid, dim3(kThreads), bytes, stream, args);
  } else {
    hipLaunchKernelGGL(rays_kernel<kRayBroadened>, grid, dim3(kThreads), bytes, stream, args);
  }
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string("ray transfer kernel: ") + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

}  // namespace avr
