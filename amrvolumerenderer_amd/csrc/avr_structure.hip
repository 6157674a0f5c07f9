// Structure functions ("Structure functions"): the moments S_p = <|dv|^p> of the
// increments of one or three real f64 grids [nz][ny][nx] over a table of integer lag vectors.
//
//   structure_functions_kernel<C, PERIODIC>   C = 1: the moments of |dv|; C = 3: of the
//                                             longitudinal, the transverse and the whole increment
//
// A workgroup takes one lag and one share of kStructureGroupCells consecutive cells; the lag is the
// fast-running block index, so the workgroups resident together read one share's lines.  A lane
// walks cells 256 apart -- a wave's centre loads are contiguous runs of 512 bytes, its partner
// loads the same runs shifted and broken only where a row ends or wraps -- and carries (i, j, k)
// along by the plan's decomposition of 256, so that nothing is divided in the loop.  The partner's
// index is formed by comparing before adding: no intermediate leaves 32 bits for N_d up to 2^31 -
// 1.  Every difference, product, sum and square root is rounded on its own (-ffp-contract=off, no
// fma; the f64 square root is the correctly rounded one), so a pair's terms are fixed by bits; a
// pair that is outside or not finite adds an exact zero.  The K P <= 24 partial sums and the three
// counters stay in registers; at the end one wave reduction, one LDS step and one global atomic per
// non-zero sum and counter -- the order of these adds is the schedule's, which is what the
// summation bound of the section allows.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxOrder = kStructureMaxOrder;
static_assert(kThreads == kStructureLaneStride, "the plan decomposes this stride");
static_assert(kStructureGroupCells % kThreads == 0, "a lane takes whole trips");

typedef const StructureLagDev __attribute__((address_space(4))) constant_lag;

// One axis of a lag: whether the partner of index `at` exists, and the offset in cells to it.
// PERIODIC: the lag wrapped into [0, n) and `turn` = n - that; an index from `turn` on wraps once.
// Otherwise the indices [first, last) have a partner and the offset is the lag's own.
struct AxisShift {
  uint32_t first, last;  // not PERIODIC: the indices with a partner; PERIODIC: (turn, unused)
  uint32_t step, wrapped_step;  // in cells, modulo 2^32: added to the centre's index
};
template <bool PERIODIC>
__device__ __forceinline__ AxisShift axis_shift(int32_t lag, int32_t n, uint32_t cells_per_index) {
  AxisShift s;
  if (PERIODIC) {
    const uint32_t forward = static_cast<uint32_t>(lag < 0 ? lag + n : lag);  // in [0, n)
    s.first = static_cast<uint32_t>(n) - forward;                             // in [1, n]
    s.last = 0u;
    s.step = forward * cells_per_index;
    s.wrapped_step = 0u - s.first * cells_per_index;
  } else {
    s.first = lag < 0 ? static_cast<uint32_t>(-lag) : 0u;
    s.last = lag < 0 ? static_cast<uint32_t>(n) : static_cast<uint32_t>(n - lag);
    s.step = static_cast<uint32_t>(lag) * cells_per_index;
    s.wrapped_step = s.step;
  }
  return s;
}
// The offset to the partner along one axis; clears *inside where there is none.
template <bool PERIODIC>
__device__ __forceinline__ uint32_t partner_step(const AxisShift& s, uint32_t at, bool* inside) {
  if (PERIODIC) return at >= s.first ? s.wrapped_step : s.step;
  *inside = *inside & (at >= s.first) & (at < s.last);
  return s.step;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int mask = 32; mask > 0; mask >>= 1) v = v + __shfl_xor(v, mask, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int mask = 32; mask > 0; mask >>= 1) v += __shfl_xor(v, mask, 64);
  return v;
}

// The output arrays are ordinary (coarse-grained) device allocations: the hardware's f64 add.
__device__ __forceinline__ void global_add(double* at, double v) { unsafeAtomicAdd(at, v); }

template <int C, bool PERIODIC>
__global__ __launch_bounds__(kThreads) void structure_functions_kernel(const StructureArgs a) {
  constexpr int K = C;  // kinds: |dv|, or longitudinal, transverse, magnitude
  __shared__ double wave_sums[kWaves][K * kMaxOrder];
  __shared__ uint32_t wave_counts[kWaves][3];
  const uint32_t share = blockIdx.y + kStructureShareRows * blockIdx.z;
  if (share >= a.shares) return;  // the last grid row's spare workgroups (workgroup-uniform)
  const int m = static_cast<int>(blockIdx.x);
  const int P = a.max_order;
  const uint32_t nx = static_cast<uint32_t>(a.dims[0]), ny = static_cast<uint32_t>(a.dims[1]);
  constant_lag* lag = (constant_lag*)a.lags + m;
  const AxisShift sx = axis_shift<PERIODIC>(lag->l[0], a.dims[0], 1u);
  const AxisShift sy = axis_shift<PERIODIC>(lag->l[1], a.dims[1], nx);
  const AxisShift sz = axis_shift<PERIODIC>(lag->l[2], a.dims[2], nx * ny);
  const double ux = C == 3 ? lag->u[0] : 0.0, uy = C == 3 ? lag->u[1] : 0.0;
  const double uz = C == 3 ? lag->u[2] : 0.0;
  const double* __restrict__ vx = a.components[0];
  const double* __restrict__ vy = a.components[C == 3 ? 1 : 0];
  const double* __restrict__ vz = a.components[C == 3 ? 2 : 0];

  const uint32_t first = share * kStructureGroupCells;
  const uint32_t left = a.n_cells - first;
  const uint32_t count = left < kStructureGroupCells ? left : kStructureGroupCells;
  // the lane's first cell, decoded once; afterwards (i, j, k) advance by the plan's stride
  uint32_t cell = first + threadIdx.x;
  uint32_t i = cell % nx;
  const uint32_t row = cell / nx;
  uint32_t j = row % ny, k = row / ny;

  double sums[K][kMaxOrder];
#pragma unroll
  for (int kind = 0; kind < K; ++kind) {
#pragma unroll
    for (int p = 0; p < kMaxOrder; ++p) sums[kind][p] = 0.0;
  }
  uint32_t pairs = 0, outside = 0, nonfinite = 0;
  for (uint32_t e = threadIdx.x; e < count; e += kThreads) {
    bool inside = true;
    uint32_t partner = cell + partner_step<PERIODIC>(sx, i, &inside);
    partner += partner_step<PERIODIC>(sy, j, &inside);
    partner += partner_step<PERIODIC>(sz, k, &inside);
    if (!inside) partner = cell;  // nothing is read outside the grid
    double amount[K];
    bool finite;
    if constexpr (C == 1) {
      const double delta = vx[partner] - vx[cell];
      amount[0] = __builtin_fabs(delta);
      finite = __builtin_isfinite(amount[0]);
    } else {
      const double dx = vx[partner] - vx[cell];
      const double dy = vy[partner] - vy[cell];
      const double dz = vz[partner] - vz[cell];
      double m2 = dx * dx + dy * dy;
      m2 = m2 + dz * dz;
      double along = dx * ux + dy * uy;
      along = along + dz * uz;
      const double tx = dx - along * ux, ty = dy - along * uy, tz = dz - along * uz;
      double t2 = tx * tx + ty * ty;
      t2 = t2 + tz * tz;
      amount[0] = __builtin_fabs(along);
      amount[1] = __builtin_sqrt(t2);
      amount[2] = __builtin_sqrt(m2);
      finite = __builtin_isfinite(m2);
    }
    const bool counted = inside & finite;
    pairs += counted ? 1u : 0u;
    outside += inside ? 0u : 1u;
    nonfinite += (inside & !finite) ? 1u : 0u;
#pragma unroll
    for (int kind = 0; kind < K; ++kind) {
      const double value = counted ? amount[kind] : 0.0;  // an exact zero: the sums keep their bits
      double power = value;
#pragma unroll
      for (int p = 0; p < kMaxOrder; ++p) {
        if (p >= P) break;  // workgroup-uniform
        if (p > 0) power = power * value;
        sums[kind][p] = sums[kind][p] + power;
      }
    }
    // the next cell of this lane, kThreads further on: one carry per axis at the most
    cell += kThreads;
    i += a.stride[0];
    uint32_t carry = i >= nx ? 1u : 0u;
    i -= carry != 0u ? nx : 0u;
    j += a.stride[1] + carry;
    carry = j >= ny ? 1u : 0u;
    j -= carry != 0u ? ny : 0u;
    k += a.stride[2] + carry;
  }

  const int tid = static_cast<int>(threadIdx.x);
  const int wave = tid >> 6;
#pragma unroll
  for (int kind = 0; kind < K; ++kind) {
#pragma unroll
    for (int p = 0; p < kMaxOrder; ++p) {
      if (p >= P) break;
      const double total = wave_sum(sums[kind][p]);
      if ((tid & 63) == 0) wave_sums[wave][kind * kMaxOrder + p] = total;
    }
  }
  pairs = wave_sum(pairs);
  outside = wave_sum(outside);
  nonfinite = wave_sum(nonfinite);
  if ((tid & 63) == 0) {
    wave_counts[wave][0] = pairs;
    wave_counts[wave][1] = outside;
    wave_counts[wave][2] = nonfinite;
  }
  __syncthreads();
  if (tid < K * kMaxOrder) {
    const int kind = tid / kMaxOrder, p = tid % kMaxOrder;
    if (p < P) {
      double total = wave_sums[0][tid];
      for (int w = 1; w < kWaves; ++w) total = total + wave_sums[w][tid];
      if (total != 0.0) {
        global_add(&a.sums[(static_cast<size_t>(m) * K + kind) * static_cast<size_t>(P) + p],
                   total);
      }
    }
  } else if (tid >= 64 && tid < 64 + 3) {  // another wave: the counters
    const int which = tid - 64;
    uint32_t total = 0;
    for (int w = 0; w < kWaves; ++w) total += wave_counts[w][which];
    if (total != 0u) {
      unsigned long long* at = which == 0 ? a.pairs + m : a.totals + (which - 1);
      atomicAdd(at, static_cast<unsigned long long>(total));
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

int launch_structure_functions(const StructureArgs& args, int n_components,
                               const uint32_t groups[3], void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const dim3 grid(groups[0], groups[1], groups[2]);
#define AVR_STRUCTURE(C, PERIODIC)                                                            \
  hipLaunchKernelGGL((structure_functions_kernel<C, PERIODIC>), grid, dim3(kThreads), 0, stream, \
                     args)
  if (n_components == 3) {
    if (args.periodic != 0) AVR_STRUCTURE(3, true); else AVR_STRUCTURE(3, false);
  } else {
    if (args.periodic != 0) AVR_STRUCTURE(1, true); else AVR_STRUCTURE(1, false);
  }
#undef AVR_STRUCTURE
  return check("structure_functions_kernel");
}

}  // namespace avr
