// Per-mode kernels on spectra ("Power spectrum", "Inverse transform, Helmholtz split,
// potential" and "Isolated potential"); the transforms themselves are avr_fft.hip's.
//
//   spectrum_bins_kernel               |F|^2 of every mode added to the bin of its wave number
//   spectrum_helmholtz_kernel          three spectra -> their solenoidal (in place) and compressive
//                                      parts
//   spectrum_inverse_laplacian_kernel  one spectrum scaled by scale / q in place, 0 at q == 0
//   spectrum_multiply_kernel           a <- a b, the complex product mode by mode
//   isolated_green_kernel              the open-boundary Green's grid scale / r of a padded grid: the
//                                      same cut over cells, 8-byte stores, nothing loaded
//
// All stream: a workgroup takes kModesPerGroup consecutive modes (the launches take the count of
// workgroups from their plans), a lane one mode per trip, read and written as 16-byte (re, im)
// values by the same lane, so a wave's accesses are contiguous runs of 1 KiB.  The mode's index is
// decoded by shifts (every dimension is a power of two).  Every product, sum and quotient is
// rounded on its own (-ffp-contract=off, no fma); the f64 division is the correctly rounded one.
// The bin kernel alone uses LDS and atomics -- its bins' sums depend on the order of the adds; the
// other four use neither, and equal arguments give equal bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kModesPerGroup = 16384;  // 64 per lane; of the bin kernel a 32-bit count each
static_assert(kModesPerGroup == kSpectralGroupElements, "the plans count groups of this size");

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef double __attribute__((address_space(3))) lds_double;

// The workgroup's share of n modes or cells: `count` of them from `first` on.
struct GroupRange {
  uint32_t first, count;
};
__device__ __forceinline__ GroupRange group_range(uint32_t n) {
  const uint32_t first = blockIdx.x * kModesPerGroup;
  const uint32_t left = n - first;
  return {first, left < kModesPerGroup ? left : kModesPerGroup};
}

// The indices along x, y and z of the mode or cell `index` of a grid of 2^px by 2^py by .. values.
struct AxisIndices {
  uint32_t x, y, z;
};
__device__ __forceinline__ AxisIndices axis_indices(uint32_t index, int px, int py) {
  return {index & ((1u << px) - 1u), (index >> px) & ((1u << py) - 1u), index >> (px + py)};
}

// The signed wave number of index k along an axis of 2^p modes (numpy.fft.fftfreq's convention).
__device__ __forceinline__ int signed_mode(uint32_t k, int p) {
  const int n = 1 << p;
  return (static_cast<int>(k) < (n >> 1) || n == 1) ? static_cast<int>(k)
                                                     : static_cast<int>(k) - n;
}

// ... with the Nyquist rule: the mode k == n / 2 of an axis of n >= 2 counts as 0, which keeps the
// projector Hermitian.
__device__ __forceinline__ int projector_mode(uint32_t k, int p) {
  const int n = 1 << p;
  return (n >= 2 && static_cast<int>(k) == (n >> 1)) ? 0 : signed_mode(k, p);
}

// q = sum_d m_d^2 g[d] of the signed wave numbers (mx, my, mz); the grouping is part of the
// contract: every product on its own, x and y added first, then z.
__device__ __forceinline__ double shell_q(int mx, int my, int mz, const double g[3]) {
  const double x = static_cast<double>(mx), y = static_cast<double>(my);
  const double z = static_cast<double>(mz);
  double q = (x * x) * g[0] + (y * y) * g[1];
  q = q + (z * z) * g[2];
  return q;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int mask = 32; mask > 0; mask >>= 1) v += __shfl_xor(v, mask, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void spectrum_bins_kernel(const SpectrumBinsArgs a) {
  // [edges: n + 1][sums: n][counts: n x u32]
  extern __shared__ double bins_lds[];
  __shared__ uint32_t wave_totals[kThreads / 64][2];
  const int n = a.n_bins;
  lds_double* edges = (lds_double*)bins_lds;
  lds_double* local_sums = edges + (n + 1);
  unsigned int* local_counts = reinterpret_cast<unsigned int*>(bins_lds + (2 * n + 1));
  const int tid = static_cast<int>(threadIdx.x);
  for (int i = tid; i <= n; i += kThreads) edges[i] = a.edges_sq[i];
  for (int b = tid; b < n; b += kThreads) {
    local_sums[b] = 0.0;
    local_counts[b] = 0u;
  }
  __syncthreads();

  const double lowest = edges[0], highest = edges[n];
  const int px = a.log2n[0], py = a.log2n[1], pz = a.log2n[2];
  const double2_t* __restrict__ spectrum = reinterpret_cast<const double2_t*>(a.spectrum);
  uint32_t outside = 0, nonfinite = 0;
  const GroupRange range = group_range(a.n_modes);
  for (uint32_t e = threadIdx.x; e < range.count; e += kThreads) {
    const uint32_t mode = range.first + e;
    const double2_t f = spectrum[mode];
    const double power = f.x * f.x + f.y * f.y;
    if (!__builtin_isfinite(power)) {
      nonfinite += 1;
      continue;
    }
    const AxisIndices k = axis_indices(mode, px, py);
    const double q =
        shell_q(signed_mode(k.x, px), signed_mode(k.y, py), signed_mode(k.z, pz), a.g);
    if (!((lowest <= q) & (q <= highest))) {
      outside += 1;
      continue;
    }
    // the largest i in [0, n - 1] with E[i] <= q: E[lo] <= q and (hi == n or q < E[hi])
    int lo = 0, hi = n;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (edges[mid] <= q) {
        lo = mid;
      } else {
        hi = mid;
      }
    }
    atomicAdd(&local_counts[lo], 1u);
    __hip_atomic_fetch_add(local_sums + lo, power, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  for (int b = tid; b < n; b += kThreads) {
    const unsigned int c = local_counts[b];
    if (c != 0u) {
      atomicAdd(&a.modes[b], static_cast<unsigned long long>(c));
      // an ordinary (coarse-grained) device allocation: the hardware's f64 add
      unsafeAtomicAdd(&a.power[b], static_cast<double>(local_sums[b]));
    }
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

__global__ __launch_bounds__(kThreads) void spectrum_helmholtz_kernel(const HelmholtzArgs a) {
  const int px = a.log2n[0], py = a.log2n[1], pz = a.log2n[2];
  double2_t* fx = reinterpret_cast<double2_t*>(a.spectra[0]);
  double2_t* fy = reinterpret_cast<double2_t*>(a.spectra[1]);
  double2_t* fz = reinterpret_cast<double2_t*>(a.spectra[2]);
  double2_t* cx = reinterpret_cast<double2_t*>(a.compressive[0]);
  double2_t* cy = reinterpret_cast<double2_t*>(a.compressive[1]);
  double2_t* cz = reinterpret_cast<double2_t*>(a.compressive[2]);
  const GroupRange range = group_range(a.n_modes);
  for (uint32_t e = threadIdx.x; e < range.count; e += kThreads) {
    const uint32_t mode = range.first + e;
    const double2_t vx = fx[mode], vy = fy[mode], vz = fz[mode];
    const AxisIndices k = axis_indices(mode, px, py);
    const double kx = static_cast<double>(projector_mode(k.x, px)) * a.h[0];
    const double ky = static_cast<double>(projector_mode(k.y, py)) * a.h[1];
    const double kz = static_cast<double>(projector_mode(k.z, pz)) * a.h[2];
    // on the scaled wave numbers, each rounded before its square: not shell_q's q
    double q = kx * kx + ky * ky;
    q = q + kz * kz;
    // q == 0, the mean flow and the Nyquist-only modes: solenoidal, their bits kept
    double2_t sx = vx, sy = vy, sz = vz;
    double2_t ox = {0.0, 0.0}, oy = {0.0, 0.0}, oz = {0.0, 0.0};
    if (q != 0.0) {
      double2_t d = kx * vx + ky * vy;
      d = d + kz * vz;
      const double2_t s = d / q;
      ox = kx * s;
      oy = ky * s;
      oz = kz * s;
      sx = vx - ox;
      sy = vy - oy;
      sz = vz - oz;
    }
    fx[mode] = sx;
    fy[mode] = sy;
    fz[mode] = sz;
    cx[mode] = ox;
    cy[mode] = oy;
    cz[mode] = oz;
  }
}

__global__ __launch_bounds__(kThreads) void spectrum_inverse_laplacian_kernel(
    const InverseLaplacianArgs a) {
  const int px = a.log2n[0], py = a.log2n[1], pz = a.log2n[2];
  double2_t* spectrum = reinterpret_cast<double2_t*>(a.spectrum);
  const GroupRange range = group_range(a.n_modes);
  for (uint32_t e = threadIdx.x; e < range.count; e += kThreads) {
    const uint32_t mode = range.first + e;
    const double2_t f = spectrum[mode];
    const AxisIndices k = axis_indices(mode, px, py);
    const double q =
        shell_q(signed_mode(k.x, px), signed_mode(k.y, py), signed_mode(k.z, pz), a.g);
    double2_t out = {0.0, 0.0};
    if (q != 0.0) {
      const double r = a.scale / q;
      out = f * r;
    }
    spectrum[mode] = out;
  }
}

__global__ __launch_bounds__(kThreads) void spectrum_multiply_kernel(
    const SpectrumMultiplyArgs a) {
  double2_t* left = reinterpret_cast<double2_t*>(a.a);
  const double2_t* right = reinterpret_cast<const double2_t*>(a.b);
  const GroupRange range = group_range(a.n_modes);
  for (uint32_t e = threadIdx.x; e < range.count; e += kThreads) {
    const uint32_t mode = range.first + e;
    const double2_t u = left[mode], v = right[mode];
    double2_t out;
    out.x = u.x * v.x - u.y * v.y;
    out.y = u.x * v.y + u.y * v.x;
    left[mode] = out;
  }
}

// The offset of index i of an axis of 2^p cells from the nearer image of the origin, in cells.
__device__ __forceinline__ uint32_t image_offset(uint32_t i, int p) {
  const uint32_t back = (1u << p) - i;
  return i < back ? i : back;
}

__global__ __launch_bounds__(kThreads) void isolated_green_kernel(const IsolatedGreenArgs a) {
  const int px = a.log2n[0], py = a.log2n[1];
  const GroupRange range = group_range(a.n_cells);
  for (uint32_t e = threadIdx.x; e < range.count; e += kThreads) {
    const uint32_t cell = range.first + e;
    const AxisIndices i = axis_indices(cell, px, py);
    const double x = static_cast<double>(image_offset(i.x, px)) * a.size[0];
    const double y = static_cast<double>(image_offset(i.y, py)) * a.size[1];
    const double z = static_cast<double>(image_offset(i.z, a.log2n[2])) * a.size[2];
    double r2 = x * x + y * y;
    r2 = r2 + z * z;
    // the origin divides by zero like every other lane and then takes self_value: no branch
    const double g = a.scale / __builtin_sqrt(r2);
    a.green[cell] = r2 == 0.0 ? a.self_value : g;
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

int launch_spectrum_bins(const SpectrumBinsArgs& args, uint32_t groups, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const size_t n = static_cast<size_t>(args.n_bins);
  const size_t bytes = (n + 1) * 8 + n * 8 + n * 4;
  hipLaunchKernelGGL(spectrum_bins_kernel, dim3(groups), dim3(kThreads), bytes, stream, args);
  return check("spectrum_bins_kernel");
}

int launch_spectrum_helmholtz(const HelmholtzArgs& args, uint32_t groups, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  hipLaunchKernelGGL(spectrum_helmholtz_kernel, dim3(groups), dim3(kThreads), 0, stream, args);
  return check("spectrum_helmholtz_kernel");
}

int launch_spectrum_inverse_laplacian(const InverseLaplacianArgs& args, uint32_t groups,
                                      void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  hipLaunchKernelGGL(spectrum_inverse_laplacian_kernel, dim3(groups), dim3(kThreads), 0, stream,
                     args);
  return check("spectrum_inverse_laplacian_kernel");
}

int launch_spectrum_multiply(const SpectrumMultiplyArgs& args, uint32_t groups, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  hipLaunchKernelGGL(spectrum_multiply_kernel, dim3(groups), dim3(kThreads), 0, stream, args);
  return check("spectrum_multiply_kernel");
}

int launch_isolated_green(const IsolatedGreenArgs& args, uint32_t groups, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  hipLaunchKernelGGL(isolated_green_kernel, dim3(groups), dim3(kThreads), 0, stream, args);
  return check("isolated_green_kernel");
}

}  // namespace avr
