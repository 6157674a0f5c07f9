// Power spectra ("Power spectrum"): the forward, unnormalised 3-D transform of a real
// f64 grid and the shell sums of its spectrum.
//
//   fft_x_kernel          real [nz][ny][nx] -> complex [nz][ny][nx][2], transformed along x
//   fft_column_kernel     one strided pass (y, then z) in place on the spectrum
//   spectrum_bins_kernel  |F|^2 of every mode added to the bin of its wave number
//   ifft_x_kernel         the inverse's last pass: complex lines along x -> real grids, scaled
//                         (the inverse's z and y passes are fft_column_kernel with conjugate tables)
//
// A line is transformed as the definition states it: the input permuted by bit reversal of the
// log2(n)-bit index, then stages s = 1 .. log2(n) of radix-2 decimation in time, in stage s for
// every block of 2 half elements (half = 2^(s - 1)) and every j in [0, half)
//   a = v[block + j], b = v[block + j + half], w = W[j * (n >> s)],
//   t = (w.re b.re - w.im b.im, w.re b.im + w.im b.re),  v[block + j] = a + t,  v[.. + half] = a - t
// with every product and sum rounded on its own (-ffp-contract=off, no fma).  Each butterfly reads
// and writes its own two elements, so the order of the butterflies within a stage does not show in
// the bits; no table entry is replaced by a constant.
//
// Whole lines live in LDS, `lines` of them side by side as [line][n] complex values (16 bytes
// each; at most 4096 of them, 64 KiB).  Position `at` of line `l` is kept at at ^ key with key =
// (l & 7) ^ (at >> (log2(n) - 3)) (the second term from n = 64 on, the first from n = 8 on): the
// key changes only the low three bits, so it permutes every aligned run of 8 elements in itself and
// a butterfly's 16 adjacent lanes still cover 256 contiguous bytes, while the 8 elements that the
// bit-reversed store of 8 adjacent inputs writes -- n / 8 apart -- and the elements that adjacent
// columns write at one position -- n apart -- fall on 8 different 16-byte bank groups instead of
// one (MI355X LDS: 16-byte stores go 8 lanes at a time over 32 banks of 4 bytes).
//
// The x pass reads `x_group` whole lines, a contiguous run of reals, and writes the same run of
// complex values.  A strided pass stages `group` adjacent columns: lane e handles column e % cols
// of element e / cols, so every global access of a wave is made of runs of cols 16-byte elements;
// a workgroup reads all its lines before it writes any and no other workgroup touches them.
// Element offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kModesPerGroup = 16384;  // of the bin kernel: 64 per lane, a 32-bit count each

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef double __attribute__((address_space(3))) lds_double;

__device__ __forceinline__ uint32_t reverse_bits(uint32_t index, int p) {
  return p == 0 ? 0u : __brev(index) >> (32 - p);
}

// Where position `at` of line `line` lies within the line's n = 2^p elements.
__device__ __forceinline__ uint32_t swizzle(uint32_t at, uint32_t line, int p) {
  uint32_t key = 0;
  if (p >= 3) key = line & 7u;
  if (p >= 6) key ^= at >> (p - 3);
  return at ^ key;
}

// Stages 1 .. p on `lines` lines of 2^p elements in v; w: the n / 2 twiddles.  Ends with every
// lane past the last stage's writes.
__device__ __forceinline__ void line_stages(double2_t* v, uint32_t lines, int p,
                                            const double2_t* __restrict__ w) {
  const uint32_t butterflies = (lines << p) >> 1;
  for (int s = 1; s <= p; ++s) {
    __syncthreads();
    const uint32_t half = 1u << (s - 1);
    for (uint32_t b = threadIdx.x; b < butterflies; b += kThreads) {
      const uint32_t line = b >> (p - 1), within = b & ((1u << (p - 1)) - 1u);
      const uint32_t j = within & (half - 1u);
      const uint32_t at = ((within >> (s - 1)) << s) + j;
      const double2_t tw = w[j << (p - s)];
      const uint32_t ia = (line << p) + swizzle(at, line, p);
      const uint32_t ib = (line << p) + swizzle(at + half, line, p);
      const double2_t a = v[ia], x = v[ib];
      double2_t t;
      t.x = tw.x * x.x - tw.y * x.y;
      t.y = tw.x * x.y + tw.y * x.x;
      v[ia] = a + t;
      v[ib] = a - t;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void fft_x_kernel(const FftArgs a) {
  extern __shared__ double2_t fft_lds[];
  const int p = a.log2nx;
  const uint32_t first = blockIdx.x * a.x_group;
  const uint32_t left = a.x_lines - first;
  const uint32_t lines = left < a.x_group ? left : a.x_group;
  const uint32_t elements = lines << p;
  const size_t base = static_cast<size_t>(first) << p;
  const double* __restrict__ in = a.values + base;
  for (uint32_t e = threadIdx.x; e < elements; e += kThreads) {
    const uint32_t line = e >> p, index = e & ((1u << p) - 1u);
    double2_t value;
    value.x = in[e];
    value.y = 0.0;
    fft_lds[(line << p) + swizzle(reverse_bits(index, p), line, p)] = value;
  }
  line_stages(fft_lds, lines, p, reinterpret_cast<const double2_t*>(a.twiddle[0]));
  double2_t* out = reinterpret_cast<double2_t*>(a.spectrum) + base;
  for (uint32_t e = threadIdx.x; e < elements; e += kThreads) {
    const uint32_t line = e >> p, k = e & ((1u << p) - 1u);
    out[e] = fft_lds[(line << p) + swizzle(k, line, p)];
  }
}

__global__ __launch_bounds__(kThreads) void fft_column_kernel(double2_t* spectrum,
                                                              const double2_t* __restrict__ w,
                                                              const FftPassDev pass) {
  extern __shared__ double2_t fft_lds[];
  const int p = pass.log2n;
  const uint32_t plane = blockIdx.x / pass.groups, group = blockIdx.x - plane * pass.groups;
  const uint32_t cols = group + 1u == pass.groups ? pass.last : pass.group;
  const uint32_t elements = cols << p;
  double2_t* at = spectrum + (static_cast<size_t>(plane) * pass.plane_stride +
                              static_cast<size_t>(group) * pass.group);
  for (uint32_t e = threadIdx.x; e < elements; e += kThreads) {
    const uint32_t index = e / cols, c = e - index * cols;
    fft_lds[(c << p) + swizzle(reverse_bits(index, p), c, p)] =
        at[static_cast<size_t>(index) * pass.line_stride + c];
  }
  line_stages(fft_lds, cols, p, w);
  for (uint32_t e = threadIdx.x; e < elements; e += kThreads) {
    const uint32_t k = e / cols, c = e - k * cols;
    at[static_cast<size_t>(k) * pass.line_stride + c] = fft_lds[(c << p) + swizzle(k, c, p)];
  }
}

// The inverse's x pass ("Inverse transform, Helmholtz split, potential"): x_group
// whole lines of complex input, the stages with the conjugate table V, then re * scale to `values`
// and, where asked for, im * scale to `imag`.  Launched for nx == 1 as well: the scale and split.
__global__ __launch_bounds__(kThreads) void ifft_x_kernel(const IfftArgs a) {
  extern __shared__ double2_t fft_lds[];
  const int p = a.log2nx;
  const uint32_t first = blockIdx.x * a.x_group;
  const uint32_t left = a.x_lines - first;
  const uint32_t lines = left < a.x_group ? left : a.x_group;
  const uint32_t elements = lines << p;
  const size_t base = static_cast<size_t>(first) << p;
  const double2_t* __restrict__ in = reinterpret_cast<const double2_t*>(a.spectrum) + base;
  for (uint32_t e = threadIdx.x; e < elements; e += kThreads) {
    const uint32_t line = e >> p, index = e & ((1u << p) - 1u);
    fft_lds[(line << p) + swizzle(reverse_bits(index, p), line, p)] = in[e];
  }
  line_stages(fft_lds, lines, p, reinterpret_cast<const double2_t*>(a.twiddle[0]));
  double* __restrict__ values = a.values + base;
  double* __restrict__ imag = a.imag != nullptr ? a.imag + base : nullptr;
  const double scale = a.scale;
  for (uint32_t e = threadIdx.x; e < elements; e += kThreads) {
    const uint32_t line = e >> p, k = e & ((1u << p) - 1u);
    const double2_t value = fft_lds[(line << p) + swizzle(k, line, p)];
    values[e] = value.x * scale;
    if (imag != nullptr) imag[e] = value.y * scale;
  }
}

// The signed wave number of index k along an axis of 2^p modes (numpy.fft.fftfreq's convention).
__device__ __forceinline__ double signed_mode(uint32_t k, int p) {
  const int n = 1 << p;
  const int m = (static_cast<int>(k) < (n >> 1) || n == 1) ? static_cast<int>(k)
                                                            : static_cast<int>(k) - n;
  return static_cast<double>(m);
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
  const int px = a.log2n[0], py = a.log2n[1];
  const double2_t* __restrict__ spectrum = reinterpret_cast<const double2_t*>(a.spectrum);
  uint32_t outside = 0, nonfinite = 0;
  const uint32_t first = blockIdx.x * kModesPerGroup;
  const uint32_t left = a.n_modes - first;
  const uint32_t count = left < kModesPerGroup ? left : kModesPerGroup;
  for (uint32_t e = threadIdx.x; e < count; e += kThreads) {
    const uint32_t mode = first + e;
    const double2_t f = spectrum[mode];
    const double power = f.x * f.x + f.y * f.y;
    if (!__builtin_isfinite(power)) {
      nonfinite += 1;
      continue;
    }
    const double mx = signed_mode(mode & ((1u << px) - 1u), px);
    const double my = signed_mode((mode >> px) & ((1u << py) - 1u), py);
    const double mz = signed_mode(mode >> (px + py), a.log2n[2]);
    double q = (mx * mx) * a.g[0] + (my * my) * a.g[1];
    q = q + (mz * mz) * a.g[2];
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

int check(const char* what) {
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string(what) + ": " + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

}  // namespace

int launch_fft3d(const FftArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const uint32_t x_groups = (args.x_lines + args.x_group - 1) / args.x_group;
  const size_t x_bytes = (static_cast<size_t>(args.x_group) << args.log2nx) * sizeof(double2_t);
  hipLaunchKernelGGL(fft_x_kernel, dim3(x_groups), dim3(kThreads), x_bytes, stream, args);
  int status = check("fft_x_kernel");
  for (int which = 0; which < 2 && status == AVR_OK; ++which) {
    const FftPassDev& pass = args.pass[which];
    if (pass.n == 1) continue;  // the identity
    const size_t bytes = (static_cast<size_t>(pass.group) << pass.log2n) * sizeof(double2_t);
    hipLaunchKernelGGL(fft_column_kernel, dim3(pass.planes * pass.groups), dim3(kThreads), bytes,
                       stream, reinterpret_cast<double2_t*>(args.spectrum),
                       reinterpret_cast<const double2_t*>(args.twiddle[which + 1]), pass);
    status = check("fft_column_kernel");
  }
  return status;
}

int launch_ifft3d(const IfftArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  int status = AVR_OK;
  for (int which = 1; which >= 0 && status == AVR_OK; --which) {  // z, then y
    const FftPassDev& pass = args.pass[which];
    if (pass.n == 1) continue;  // the identity
    const size_t bytes = (static_cast<size_t>(pass.group) << pass.log2n) * sizeof(double2_t);
    hipLaunchKernelGGL(fft_column_kernel, dim3(pass.planes * pass.groups), dim3(kThreads), bytes,
                       stream, reinterpret_cast<double2_t*>(args.spectrum),
                       reinterpret_cast<const double2_t*>(args.twiddle[which + 1]), pass);
    status = check("fft_column_kernel");
  }
  if (status != AVR_OK) return status;
  const uint32_t x_groups = (args.x_lines + args.x_group - 1) / args.x_group;
  const size_t x_bytes = (static_cast<size_t>(args.x_group) << args.log2nx) * sizeof(double2_t);
  hipLaunchKernelGGL(ifft_x_kernel, dim3(x_groups), dim3(kThreads), x_bytes, stream, args);
  return check("ifft_x_kernel");
}

int launch_spectrum_bins(const SpectrumBinsArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const uint32_t groups = (args.n_modes + kModesPerGroup - 1) / kModesPerGroup;
  const size_t n = static_cast<size_t>(args.n_bins);
  const size_t bytes = (n + 1) * 8 + n * 8 + n * 4;
  hipLaunchKernelGGL(spectrum_bins_kernel, dim3(groups), dim3(kThreads), bytes, stream, args);
  return check("spectrum_bins_kernel");
}

}  // namespace avr
