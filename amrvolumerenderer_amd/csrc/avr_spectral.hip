// Per-mode operators on spectra ("Inverse transform, Helmholtz split, potential" and
// "Isolated potential"):
//
//   spectrum_helmholtz_kernel          three spectra -> their solenoidal (in place) and compressive
//                                      parts
//   spectrum_inverse_laplacian_kernel  one spectrum scaled by scale / q in place, 0 at q == 0
//   spectrum_multiply_kernel           a <- a b, the complex product mode by mode
//   isolated_green_kernel              the open-boundary Green's grid scale / r of a padded grid: the
//                                      same cut over cells, 8-byte stores, nothing loaded
//
// All stream: a workgroup takes kModesPerGroup consecutive modes, a lane one mode per trip, read
// and written as 16-byte (re, im) values by the same lane, so a wave's accesses are contiguous
// runs of 1 KiB and equal arguments give equal bits.  The mode's index is decoded by shifts (every
// dimension is a power of two).  Every product, sum and quotient is rounded on its own
// (-ffp-contract=off, no fma); the f64 division is the correctly rounded one.  No LDS, no atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kModesPerGroup = 16384;  // 64 per lane
static_assert(kModesPerGroup == kSpectralGroupElements, "the plans count groups of this size");

typedef double double2_t __attribute__((ext_vector_type(2)));

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

__global__ __launch_bounds__(kThreads) void spectrum_helmholtz_kernel(const HelmholtzArgs a) {
  const int px = a.log2n[0], py = a.log2n[1], pz = a.log2n[2];
  double2_t* fx = reinterpret_cast<double2_t*>(a.spectra[0]);
  double2_t* fy = reinterpret_cast<double2_t*>(a.spectra[1]);
  double2_t* fz = reinterpret_cast<double2_t*>(a.spectra[2]);
  double2_t* cx = reinterpret_cast<double2_t*>(a.compressive[0]);
  double2_t* cy = reinterpret_cast<double2_t*>(a.compressive[1]);
  double2_t* cz = reinterpret_cast<double2_t*>(a.compressive[2]);
  const uint32_t first = blockIdx.x * kModesPerGroup;
  const uint32_t left = a.n_modes - first;
  const uint32_t count = left < kModesPerGroup ? left : kModesPerGroup;
  for (uint32_t e = threadIdx.x; e < count; e += kThreads) {
    const uint32_t mode = first + e;
    const double2_t vx = fx[mode], vy = fy[mode], vz = fz[mode];
    const double kx = static_cast<double>(projector_mode(mode & ((1u << px) - 1u), px)) * a.h[0];
    const double ky =
        static_cast<double>(projector_mode((mode >> px) & ((1u << py) - 1u), py)) * a.h[1];
    const double kz = static_cast<double>(projector_mode(mode >> (px + py), pz)) * a.h[2];
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
  const uint32_t first = blockIdx.x * kModesPerGroup;
  const uint32_t left = a.n_modes - first;
  const uint32_t count = left < kModesPerGroup ? left : kModesPerGroup;
  for (uint32_t e = threadIdx.x; e < count; e += kThreads) {
    const uint32_t mode = first + e;
    const double2_t f = spectrum[mode];
    const double mx = static_cast<double>(signed_mode(mode & ((1u << px) - 1u), px));
    const double my = static_cast<double>(signed_mode((mode >> px) & ((1u << py) - 1u), py));
    const double mz = static_cast<double>(signed_mode(mode >> (px + py), pz));
    double q = (mx * mx) * a.g[0] + (my * my) * a.g[1];
    q = q + (mz * mz) * a.g[2];
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
  const uint32_t first = blockIdx.x * kModesPerGroup;
  const uint32_t rest = a.n_modes - first;
  const uint32_t count = rest < kModesPerGroup ? rest : kModesPerGroup;
  for (uint32_t e = threadIdx.x; e < count; e += kThreads) {
    const uint32_t mode = first + e;
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
  const uint32_t first = blockIdx.x * kModesPerGroup;
  const uint32_t rest = a.n_cells - first;
  const uint32_t count = rest < kModesPerGroup ? rest : kModesPerGroup;
  for (uint32_t e = threadIdx.x; e < count; e += kThreads) {
    const uint32_t cell = first + e;
    const double x = static_cast<double>(image_offset(cell & ((1u << px) - 1u), px)) * a.size[0];
    const double y =
        static_cast<double>(image_offset((cell >> px) & ((1u << py) - 1u), py)) * a.size[1];
    const double z = static_cast<double>(image_offset(cell >> (px + py), a.log2n[2])) * a.size[2];
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

int launch_spectrum_helmholtz(const HelmholtzArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const uint32_t groups = (args.n_modes + kModesPerGroup - 1) / kModesPerGroup;
  hipLaunchKernelGGL(spectrum_helmholtz_kernel, dim3(groups), dim3(kThreads), 0, stream, args);
  return check("spectrum_helmholtz_kernel");
}

int launch_spectrum_inverse_laplacian(const InverseLaplacianArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const uint32_t groups = (args.n_modes + kModesPerGroup - 1) / kModesPerGroup;
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
