// Derived fields ("Derived fields"): one new f64 field per cell from a postfix program
// over up to six fields of the same cells, constants and the cell's position, size and level.
//
//   derive_kernel<F>      F = the number of input fields, 0 .. 6
//
// The inputs are scenes with the same box list; a cell is read from each at its own strides and the
// result is written to the output scene at its own.  The decomposition is that of the scan kernels
// (avr_cell_tiles.h, shared with avr_scene_stats.hip and avr_joint_histogram.hip; the walk over a
// tile's rows is this file's own, batched): one tile = 4 k-planes x 4 j-rows x 128 cells of one
// box, rows read coalesced and as f64 pairs where every input and the output allow it, 16
// consecutive tiles per workgroup.
//
// The program is read through the constant address space, so every wave reads it with scalar loads
// and branches on scalar values: the interpreter never diverges.  Per tile a lane first issues the
// loads of every field for four passes (a pass is 4 rows of cell pairs, or 2 rows of single cells),
// then interprets the program once per pass.  The value stack is registers: the top in `top`, the
// seven slots below it in s0 .. s6, chosen by a switch on the (uniform) stack pointer, so that
// nothing is indexed at run time and nothing becomes scratch.  The box table, the tile prefix sums
// and the program are all read through the constant address space: scalar loads, once per tile.
//
// Arithmetic is IEEE binary64, round to nearest, nothing fused (-ffp-contract=off), denormals
// kept; / and sqrt are the correctly rounded __ddiv_rn and __dsqrt_rn.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "avr_cell_tiles.h"
#include "avr_internal.h"

namespace avr {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTilesPerGroup = 16;  // tiles (2048 cells each) per workgroup
constexpr int kBatch = 4;                // passes whose loads are in flight together

typedef double __attribute__((address_space(1))) global_double;
typedef const double __attribute__((address_space(1))) const_global_double;
typedef const DeriveProgramDev __attribute__((address_space(4))) constant_program;
typedef const DeriveBoxDev __attribute__((address_space(4))) constant_box;
typedef const uint32_t __attribute__((address_space(4))) constant_u32;
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef double2_t __attribute__((address_space(1))) global_double2;
typedef const double2_t __attribute__((address_space(1))) const_global_double2;

// The cells (consecutive along x) a lane holds in one pass are a V: a double, or a pair of them.
// Everything below takes and returns V by value and never forms the address of one, so that every
// V is a register from the start.
template <class V>
__device__ __forceinline__ V splat(double v);
template <>
__device__ __forceinline__ double splat<double>(double v) {
  return v;
}
template <>
__device__ __forceinline__ double2_t splat<double2_t>(double v) {
  double2_t r = {v, v};
  return r;
}

template <class F>
__device__ __forceinline__ double map1(double a, F f) {
  return f(a);
}
template <class F>
__device__ __forceinline__ double2_t map1(double2_t a, F f) {
  double2_t r = {f(a.x), f(a.y)};
  return r;
}
template <class F>
__device__ __forceinline__ double map2(double a, double b, F f) {
  return f(a, b);
}
template <class F>
__device__ __forceinline__ double2_t map2(double2_t a, double2_t b, F f) {
  double2_t r = {f(a.x, b.x), f(a.y, b.y)};
  return r;
}
template <class F>
__device__ __forceinline__ double map3(double a, double b, double c, F f) {
  return f(a, b, c);
}
template <class F>
__device__ __forceinline__ double2_t map3(double2_t a, double2_t b, double2_t c, F f) {
  double2_t r = {f(a.x, b.x, c.x), f(a.y, b.y, c.y)};
  return r;
}

template <class V>
__device__ __forceinline__ V field_get(uint32_t field, V f0, V f1, V f2, V f3, V f4, V f5) {
  const V lo = (field == 0) ? f0 : (field == 1) ? f1 : f2;
  const V hi = (field == 3) ? f3 : (field == 4) ? f4 : f5;
  return (field < 3) ? lo : hi;
}

struct TileCoords {
  constant_box* box;
  CellTile at;
};

// What the built-ins of a pass are made of: the box's values are uniform, (i, j, k) the lane's.
struct CellFrame {
  double origin[3];
  double size[3];
  double level;
  int i;          // of the lane's first cell
  uint32_t j, k;
};

__device__ __forceinline__ double x_of(const CellFrame& f, double) {
  return f.origin[0] + (static_cast<double>(f.i) + 0.5) * f.size[0];
}
__device__ __forceinline__ double2_t x_of(const CellFrame& f, double2_t) {
  double2_t r = {f.origin[0] + (static_cast<double>(f.i) + 0.5) * f.size[0],
                 f.origin[0] + (static_cast<double>(f.i + 1) + 0.5) * f.size[0]};
  return r;
}

template <class V>
__device__ __forceinline__ V builtin_value(const CellFrame& f, uint32_t which) {
  if (which == kDeriveX) return x_of(f, V());
  double r;
  if (which == kDeriveY) {
    r = f.origin[1] + (static_cast<double>(f.j) + 0.5) * f.size[1];
  } else if (which == kDeriveZ) {
    r = f.origin[2] + (static_cast<double>(f.k) + 0.5) * f.size[2];
  } else if (which == kDeriveDx) {
    r = f.size[0];
  } else if (which == kDeriveDy) {
    r = f.size[1];
  } else if (which == kDeriveDz) {
    r = f.size[2];
  } else if (which == kDeriveCellVolume) {
    r = (f.size[0] * f.size[1]) * f.size[2];
  } else {
    r = f.level;
  }
  return splat<V>(r);
}

// The program over the cells of one pass.  The host has checked it: every operand index is in
// range, the stack never underflows or holds more than kDeriveMaxDepth values, and one value is
// left at the end.
template <class V>
__device__ __forceinline__ V interpret(constant_program* program, int n_instructions, V f0, V f1,
                                       V f2, V f3, V f4, V f5, const CellFrame& frame) {
  // The stack below its top.  The slots are plain local values that only this function names, and
  // a slot is chosen by a switch on the uniform slot number: a scalar branch to four register
  // moves.  (Behind a reference or an array the same switch is merged into one access through a
  // computed address, which is scratch.)
  V s0 = splat<V>(0.0), s1 = s0, s2 = s0, s3 = s0, s4 = s0, s5 = s0, s6 = s0, top = s0;
#define AVR_SLOT_GET(dst, slot) \
  switch (slot) {               \
    case 0: dst = s0; break;    \
    case 1: dst = s1; break;    \
    case 2: dst = s2; break;    \
    case 3: dst = s3; break;    \
    case 4: dst = s4; break;    \
    case 5: dst = s5; break;    \
    default: dst = s6; break;   \
  }
  int sp = 0;  // values on the stack, `top` included
  // the next instruction's word is asked for before this one is carried out
  uint32_t next = program->code[0];
  for (int pc = 0; pc < n_instructions; ++pc) {
    const uint32_t word = __builtin_amdgcn_readfirstlane(next);
    next = program->code[(pc + 1) & (kDeriveMaxInstructions - 1)];
    const uint32_t op = word & 0xffu, operand = word >> 8;
    if (op <= kDeriveBuiltin) {  // a push
      switch (sp - 1) {          // -1: nothing to keep
        case 0: s0 = top; break;
        case 1: s1 = top; break;
        case 2: s2 = top; break;
        case 3: s3 = top; break;
        case 4: s4 = top; break;
        case 5: s5 = top; break;
        case 6: s6 = top; break;
        default: break;
      }
      ++sp;
      if (op == kDeriveConst) {
        top = splat<V>(program->constants[operand]);
      } else if (op == kDeriveField) {
        top = field_get(operand, f0, f1, f2, f3, f4, f5);
      } else {
        top = builtin_value<V>(frame, operand);
      }
    } else if (op == kDeriveNeg) {
      top = map1(top, [](double v) { return -v; });
    } else if (op == kDeriveSquare) {
      top = map1(top, [](double v) { return v * v; });
    } else if (op == kDeriveSqrt) {
      top = map1(top, [](double v) { return __dsqrt_rn(v); });
    } else if (op == kDeriveAbs) {
      top = map1(top, [](double v) { return __builtin_fabs(v); });
    } else if (op == kDeriveWhere) {  // c a b -> (c != 0) ? a : b
      V cond, yes;
      AVR_SLOT_GET(cond, sp - 3)
      AVR_SLOT_GET(yes, sp - 2)
      top = map3(cond, yes, top, [](double c, double a, double b) { return (c != 0.0) ? a : b; });
      sp -= 2;
    } else {  // a b -> a op b
      V left;
      AVR_SLOT_GET(left, sp - 2)
      sp -= 1;
      switch (op) {
        case kDeriveAdd: top = map2(left, top, [](double x, double y) { return x + y; }); break;
        case kDeriveSub: top = map2(left, top, [](double x, double y) { return x - y; }); break;
        case kDeriveMul: top = map2(left, top, [](double x, double y) { return x * y; }); break;
        case kDeriveDiv:
          top = map2(left, top, [](double x, double y) { return __ddiv_rn(x, y); });
          break;
        case kDeriveMin:
          top = map2(left, top, [](double x, double y) { return (x < y || x != x) ? x : y; });
          break;
        case kDeriveMax:
          top = map2(left, top, [](double x, double y) { return (x > y || x != x) ? x : y; });
          break;
        case kDeriveLt: top = map2(left, top, [](double x, double y) { return (x < y) ? 1.0 : 0.0; }); break;
        case kDeriveLe: top = map2(left, top, [](double x, double y) { return (x <= y) ? 1.0 : 0.0; }); break;
        case kDeriveGt: top = map2(left, top, [](double x, double y) { return (x > y) ? 1.0 : 0.0; }); break;
        case kDeriveGe: top = map2(left, top, [](double x, double y) { return (x >= y) ? 1.0 : 0.0; }); break;
        case kDeriveEq: top = map2(left, top, [](double x, double y) { return (x == y) ? 1.0 : 0.0; }); break;
        default: top = map2(left, top, [](double x, double y) { return (x != y) ? 1.0 : 0.0; }); break;
      }
    }
  }
#undef AVR_SLOT_GET
  return top;
}

// A field of a pass: the lane's cells at element `at`; `whole` is false for the last cell of an odd
// row, which is read alone.
__device__ __forceinline__ double load_cells(const_global_double* cells, uint32_t at, bool,
                                             double) {
  return cells[at];
}
__device__ __forceinline__ double2_t load_cells(const_global_double* cells, uint32_t at, bool whole,
                                                double2_t) {
  if (whole) return *(const_global_double2*)(cells + at);
  double2_t r = {cells[at], 0.0};
  return r;
}

__device__ __forceinline__ void store_cells(global_double* out, uint32_t at, bool, double v) {
  out[at] = v;
}
__device__ __forceinline__ void store_cells(global_double* out, uint32_t at, bool whole,
                                            double2_t v) {
  if (whole) {
    *(global_double2*)(out + at) = v;
  } else {
    out[at] = v.x;
  }
}

// One tile with N cells per lane and pass: N == 2 needs every input and the output 16-byte aligned
// with even strides (box.paired).
template <class V, int N, int F>
__device__ __forceinline__ void derive_tile(const DeriveArgs& a, const TileCoords& tile) {
  // the box's descriptor, once per tile and through the constant address space: scalar loads into
  // SGPRs that no store of this kernel can make the compiler read again
  constant_box* box = tile.box;
  const int nx = box->nx, ny = box->ny, nz = box->nz;
  const_global_double* c0 = (const_global_double*)box->cells[F > 0 ? 0 : 0];
  const_global_double* c1 = (const_global_double*)box->cells[F > 1 ? 1 : 0];
  const_global_double* c2 = (const_global_double*)box->cells[F > 2 ? 2 : 0];
  const_global_double* c3 = (const_global_double*)box->cells[F > 3 ? 3 : 0];
  const_global_double* c4 = (const_global_double*)box->cells[F > 4 ? 4 : 0];
  const_global_double* c5 = (const_global_double*)box->cells[F > 5 ? 5 : 0];
#define AVR_STRIDES(f)                                                       \
  const uint32_t jf##f = static_cast<uint32_t>(box->jstride[F > f ? f : 0]); \
  const uint32_t kf##f = static_cast<uint32_t>(box->kstride[F > f ? f : 0]);
  AVR_STRIDES(0)
  AVR_STRIDES(1)
  AVR_STRIDES(2)
  AVR_STRIDES(3)
  AVR_STRIDES(4)
  AVR_STRIDES(5)
#undef AVR_STRIDES
  constexpr int kLanesPerRow = kClassifyChunk / N;      // 64 or 128
  constexpr int kRowsPerPass = kThreads / kLanesPerRow;  // 4 or 2
  constexpr int kPasses = 16 / kRowsPerPass;             // 4 or 8
  const int t = static_cast<int>(threadIdx.x);
  const int i = tile.at.chunk * kClassifyChunk + (t % kLanesPerRow) * N;
  constant_program* program = (constant_program*)a.program;
  CellFrame frame;
  const int level = box->level;
  frame.origin[0] = box->origin[0];
  frame.origin[1] = box->origin[1];
  frame.origin[2] = box->origin[2];
  frame.size[0] = program->cell_size[level][0];
  frame.size[1] = program->cell_size[level][1];
  frame.size[2] = program->cell_size[level][2];
  frame.level = static_cast<double>(level);
  frame.i = i;
  global_double* out = (global_double*)box->out;
  const uint32_t jo = static_cast<uint32_t>(box->jstride[kDeriveMaxFields]);
  const uint32_t ko = static_cast<uint32_t>(box->kstride[kDeriveMaxFields]);
  const uint32_t ui = static_cast<uint32_t>(i);
  const bool whole = i + N - 1 < nx;
  const V zero = splat<V>(0.0);
#define AVR_DERIVE_LOAD(p)                                                                       \
  const int row##p = ((p)*kRowsPerPass) + first_row;                                                \
  const uint32_t j##p = static_cast<uint32_t>(tile.at.bj * kBrickY + (row##p & 3));                 \
  const uint32_t k##p = static_cast<uint32_t>(tile.at.bk * kBrickZ + (row##p >> 2));                \
  const bool valid##p =                                                                          \
      i < nx && static_cast<int>(j##p) < ny && static_cast<int>(k##p) < nz;                      \
  V f0_##p = zero, f1_##p = zero, f2_##p = zero, f3_##p = zero, f4_##p = zero, f5_##p = zero;    \
  if (valid##p) {                                                                                \
    if (F > 0) f0_##p = load_cells(c0, ui + j##p * jf0 + k##p * kf0, whole, V());        \
    if (F > 1) f1_##p = load_cells(c1, ui + j##p * jf1 + k##p * kf1, whole, V());        \
    if (F > 2) f2_##p = load_cells(c2, ui + j##p * jf2 + k##p * kf2, whole, V());        \
    if (F > 3) f3_##p = load_cells(c3, ui + j##p * jf3 + k##p * kf3, whole, V());        \
    if (F > 4) f4_##p = load_cells(c4, ui + j##p * jf4 + k##p * kf4, whole, V());        \
    if (F > 5) f5_##p = load_cells(c5, ui + j##p * jf5 + k##p * kf5, whole, V());        \
  }
#define AVR_DERIVE_RUN(p)                                                                        \
  {                                                                                              \
    frame.j = j##p;                                                                              \
    frame.k = k##p;                                                                              \
    const V value = interpret<V>(program, a.n_instructions, f0_##p, f1_##p, f2_##p, f3_##p,     \
                                 f4_##p, f5_##p, frame);                                         \
    if (valid##p) store_cells(out, ui + j##p * jo + k##p * ko, whole, value);                    \
  }
  for (int batch = 0; batch < kPasses / kBatch; ++batch) {
    const int first_row = batch * kBatch * kRowsPerPass + t / kLanesPerRow;
    // every load of the batch, before any interpretation
    AVR_DERIVE_LOAD(0)
    AVR_DERIVE_LOAD(1)
    AVR_DERIVE_LOAD(2)
    AVR_DERIVE_LOAD(3)
    AVR_DERIVE_RUN(0)
    AVR_DERIVE_RUN(1)
    AVR_DERIVE_RUN(2)
    AVR_DERIVE_RUN(3)
  }
#undef AVR_DERIVE_LOAD
#undef AVR_DERIVE_RUN
}

// F = the number of input fields: a kernel per count, so that a program of few fields holds few
// registers and more waves (more loads in flight) fit a SIMD.
template <int F>
__global__ __launch_bounds__(kThreads) void derive_kernel(const DeriveArgs a) {
  constant_box* boxes = (constant_box*)a.boxes;
  constant_u32* tile_begin = (constant_u32*)a.tile_begin;
  const uint32_t first = blockIdx.x * kTilesPerGroup;
  const uint32_t last = (first + kTilesPerGroup < a.n_tiles) ? first + kTilesPerGroup : a.n_tiles;
  // the workgroup's tiles are consecutive: one search (scalar loads) for the first, then a walk
  // along the boxes
  int b = locate_box(tile_begin, a.n_boxes, first);
  uint32_t begin = tile_begin[b], end = tile_begin[b + 1];
  for (uint32_t t = first; t < last; ++t) {
    while (t >= end) {  // t < n_tiles = tile_begin[n_boxes]; boxes without tiles are passed over
      ++b;
      begin = end;
      end = tile_begin[b + 1];
    }
    const TileCoords tile = {boxes + b, cell_tile_of(boxes[b].nx, boxes[b].ny, t - begin)};
    if (tile.box->paired) {
      derive_tile<double2_t, 2, F>(a, tile);
    } else {
      derive_tile<double, 1, F>(a, tile);
    }
  }
}

}  // namespace

int launch_derive(const DeriveArgs& args, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_tiles == 0) return AVR_OK;
  const uint32_t groups = (args.n_tiles + kTilesPerGroup - 1) / kTilesPerGroup;
#define AVR_DERIVE(F) \
  case F: hipLaunchKernelGGL(derive_kernel<F>, dim3(groups), dim3(kThreads), 0, stream, args); break
  switch (args.n_fields) {
    AVR_DERIVE(0);
    AVR_DERIVE(1);
    AVR_DERIVE(2);
    AVR_DERIVE(3);
    AVR_DERIVE(4);
    AVR_DERIVE(5);
    AVR_DERIVE(6);
    default: set_error("derive_kernel: more than six fields"); return AVR_ERR_INVALID_ARGUMENT;
  }
#undef AVR_DERIVE
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string("derive_kernel: ") + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

}  // namespace avr
