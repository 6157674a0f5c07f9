// The transforms ("Power spectrum" and "Inverse transform, Helmholtz split,
// potential"): the forward, unnormalised 3-D transform of a real f64 grid and the normalised
// inverse of a spectrum.  The per-mode kernels on a spectrum are avr_spectral.hip's.
//
//   fft_x_kernel          real [nz][ny][nx] -> complex [nz][ny][nx][2], transformed along x
//   fft_column_kernel     one strided pass (y, then z) in place on the spectrum
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

typedef double double2_t __attribute__((ext_vector_type(2)));

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
  const int p = a.lines.log2nx;
  const uint32_t first = blockIdx.x * a.lines.x_group;
  const uint32_t left = a.lines.x_lines - first;
  const uint32_t lines = left < a.lines.x_group ? left : a.lines.x_group;
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
  line_stages(fft_lds, lines, p, reinterpret_cast<const double2_t*>(a.lines.twiddle[0]));
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
  const int p = a.lines.log2nx;
  const uint32_t first = blockIdx.x * a.lines.x_group;
  const uint32_t left = a.lines.x_lines - first;
  const uint32_t lines = left < a.lines.x_group ? left : a.lines.x_group;
  const uint32_t elements = lines << p;
  const size_t base = static_cast<size_t>(first) << p;
  const double2_t* __restrict__ in = reinterpret_cast<const double2_t*>(a.spectrum) + base;
  for (uint32_t e = threadIdx.x; e < elements; e += kThreads) {
    const uint32_t line = e >> p, index = e & ((1u << p) - 1u);
    fft_lds[(line << p) + swizzle(reverse_bits(index, p), line, p)] = in[e];
  }
  line_stages(fft_lds, lines, p, reinterpret_cast<const double2_t*>(a.lines.twiddle[0]));
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

int check(const char* what) {
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string(what) + ": " + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

// One strided pass, pass[which] (y or z), in place on `spectrum`; a line of one value is skipped.
int launch_column_pass(const FftLinesDev& lines, int which, double* spectrum, hipStream_t stream) {
  const FftPassDev& pass = lines.pass[which];
  if (pass.n == 1) return AVR_OK;
  const size_t bytes = (static_cast<size_t>(pass.group) << pass.log2n) * sizeof(double2_t);
  hipLaunchKernelGGL(fft_column_kernel, dim3(pass.planes * pass.groups), dim3(kThreads), bytes,
                     stream, reinterpret_cast<double2_t*>(spectrum),
                     reinterpret_cast<const double2_t*>(lines.twiddle[which + 1]), pass);
  return check("fft_column_kernel");
}

// The x pass of either direction: `kernel` over groups of x_group whole lines.
template <class Args>
int launch_x_pass(void (*kernel)(Args), const Args& args, const char* name, hipStream_t stream) {
  const FftLinesDev& lines = args.lines;
  const uint32_t groups = (lines.x_lines + lines.x_group - 1) / lines.x_group;
  const size_t bytes = (static_cast<size_t>(lines.x_group) << lines.log2nx) * sizeof(double2_t);
  hipLaunchKernelGGL(kernel, dim3(groups), dim3(kThreads), bytes, stream, args);
  return check(name);
}

}  // namespace

int launch_fft3d(const FftArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  int status = launch_x_pass(fft_x_kernel, args, "fft_x_kernel", stream);
  for (int which = 0; which < 2 && status == AVR_OK; ++which) {  // y, then z
    status = launch_column_pass(args.lines, which, args.spectrum, stream);
  }
  return status;
}

int launch_ifft3d(const IfftArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  int status = AVR_OK;
  for (int which = 1; which >= 0 && status == AVR_OK; --which) {  // z, then y
    status = launch_column_pass(args.lines, which, args.spectrum, stream);
  }
  if (status != AVR_OK) return status;
  return launch_x_pass(ifft_x_kernel, args, "ifft_x_kernel", stream);
}

}  // namespace avr
