// Gradient fields ("Gradient fields"): the difference of one field along one axis,
// per cell, across boxes and levels.
//
//   gradient_halo_kernel<AXIS>          stage 1: the ghost cells of every box's two faces
//   gradient_kernel<AXIS>               stage 2: one difference per cell
//
// Stage 1 takes one lane per face cell and side.  The ghost of a level-l box is a level-l index G
// next to the face; its value is that of the cell find_same_or_coarser (avr_level_cells.h) gives
// for G, else the mean of its r^3 children if every one of them lies in a box of level l + 1, else
// it is absent.  Only the boxes the host listed for the face are tested.  Value and presence go to
// two planes per box, presence as a byte of its own: a NaN is data.  Faces are a surface term:
// this kernel is kept plain.
//
// Stage 2 is the cell scan of avr_derive.hip (avr_cell_tiles.h): one tile = 4 k-planes x 4 j-rows x
// 128 cells of one box, rows read coalesced and as f64 pairs where input and output allow it, 16
// consecutive tiles per workgroup.  Next to its own cells a lane loads its two neighbours along
// the axis: along x the one cell before and the one after its own (the lines its neighbouring
// lanes load, served by the cache), along y and z the same cells of the rows one stride below and
// above.  At a face of the box the neighbour comes from the face planes instead; nothing outside
// the box's own view is ever addressed.  Every cell is written once by one lane, from values only
// that lane read: no atomics, equal arguments give equal bits.
//
// Arithmetic is IEEE binary64, round to nearest, nothing fused (-ffp-contract=off), denormals
// kept; / is the correctly rounded __ddiv_rn.
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
typedef const uint8_t __attribute__((address_space(1))) const_global_u8;
typedef const GradientBoxDev __attribute__((address_space(4))) constant_box;
typedef const uint32_t __attribute__((address_space(4))) constant_u32;
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef double2_t __attribute__((address_space(1))) global_double2;
typedef const double2_t __attribute__((address_space(1))) const_global_double2;

// ---- stage 1 ------------------------------------------------------------------------------------

struct Index3 {
  long long x, y, z;
};

__device__ __forceinline__ bool box_holds(const GradientBoxDev& box, const Index3& g) {
  return g.x >= box.lo[0] && g.x < static_cast<long long>(box.lo[0]) + box.nx &&
         g.y >= box.lo[1] && g.y < static_cast<long long>(box.lo[1]) + box.ny &&
         g.z >= box.lo[2] && g.z < static_cast<long long>(box.lo[2]) + box.nz;
}

// the cell at index g of a box that holds it
__device__ __forceinline__ double box_cell(const GradientBoxDev& box, const Index3& g) {
  const uint32_t i = static_cast<uint32_t>(g.x - box.lo[0]);
  const uint32_t j = static_cast<uint32_t>(g.y - box.lo[1]);
  const uint32_t k = static_cast<uint32_t>(g.z - box.lo[2]);
  return box.in[i + j * static_cast<uint32_t>(box.jstride_in) +
                k * static_cast<uint32_t>(box.kstride_in)];
}

template <int AXIS>
__global__ __launch_bounds__(kThreads) void gradient_halo_kernel(const GradientArgs a) {
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= 2u * a.n_faces) return;
  const uint32_t side = t >= a.n_faces ? 1u : 0u;
  const uint32_t entry = t - side * a.n_faces;
  const int b = locate_box(a.face_begin, a.n_boxes, entry);
  const GradientBoxDev& box = a.boxes[b];
  const uint32_t local = entry - box.face_begin;
  // the face's cells are numbered along the lower of the two other axes first
  const uint32_t n_u = static_cast<uint32_t>(AXIS == 0 ? box.ny : box.nx);
  const long long u = local % n_u, v = local / n_u;
  const long long along = side ? (AXIS == 0 ? box.nx : AXIS == 1 ? box.ny : box.nz) : -1;
  Index3 ghost;
  ghost.x = box.lo[0] + (AXIS == 0 ? along : u);
  ghost.y = box.lo[1] + (AXIS == 1 ? along : AXIS == 0 ? u : v);
  ghost.z = box.lo[2] + (AXIS == 2 ? along : v);
  const int level = box.level;
  const uint32_t first = a.candidate_begin[2 * b + side], last = a.candidate_begin[2 * b + side + 1];

  // the same level or a coarser one
  const LevelCell found = find_same_or_coarser(a.boxes, a.candidates, first, last, a.levels->ratio,
                                               level, ghost.x, ghost.y, ghost.z);
  double value = 0.0;
  if (found.box >= 0) {
    const GradientBoxDev& other = a.boxes[found.box];
    value = other.in[found.i + found.j * static_cast<uint32_t>(other.jstride_in) +
                     found.k * static_cast<uint32_t>(other.kstride_in)];
  }
  bool present = found.box >= 0;
  // one level finer: every child, added in ascending k, then j, then i
  if (!present && level + 1 < a.n_levels && first < last) {
    const long long r = a.levels->ratio[level];
    const long long children = r * r * r;
    double sum = 0.0;
    uint32_t hit = first;   // the candidate that held the child before
    long long n = 0;
    for (; n < children; ++n) {
      Index3 child;
      child.x = ghost.x * r + n % r;
      child.y = ghost.y * r + (n / r) % r;
      child.z = ghost.z * r + n / (r * r);
      const GradientBoxDev* holder = &a.boxes[a.candidates[hit]];
      if (holder->level != level + 1 || !box_holds(*holder, child)) {
        holder = nullptr;
        for (uint32_t q = first; q < last; ++q) {
          const GradientBoxDev& other = a.boxes[a.candidates[q]];
          if (other.level == level + 1 && box_holds(other, child)) {
            holder = &other;
            hit = q;
            break;
          }
        }
      }
      if (holder == nullptr) break;
      sum = sum + box_cell(*holder, child);
    }
    if (n == children) {
      present = true;
      value = __ddiv_rn(sum, static_cast<double>(children));
    }
  }
  a.face_value[t] = present ? value : 0.0;
  a.face_present[t] = present ? 1 : 0;
}

// ---- stage 2 ------------------------------------------------------------------------------------

// The cells (consecutive along x) a lane holds in one pass are a V: a double, or a pair of them.
// Their presence is a mask, bit c for cell c.
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
// The same cells of a face plane, whose rows begin at any element: 8-byte loads.
__device__ __forceinline__ double load_face(const_global_double* plane, uint32_t at, bool, double) {
  return plane[at];
}
__device__ __forceinline__ double2_t load_face(const_global_double* plane, uint32_t at, bool whole,
                                               double2_t) {
  double2_t r = {plane[at], whole ? plane[at + 1] : 0.0};
  return r;
}
__device__ __forceinline__ uint32_t load_present(const_global_u8* flags, uint32_t at, bool,
                                                 double) {
  return flags[at];
}
__device__ __forceinline__ uint32_t load_present(const_global_u8* flags, uint32_t at, bool whole,
                                                 double2_t) {
  const uint32_t first = flags[at];
  return whole ? first | static_cast<uint32_t>(flags[at + 1]) << 1 : first;
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

// own value f, low neighbour l and high neighbour h, each with whether it is there
__device__ __forceinline__ double difference(double f, double l, bool has_l, double h, bool has_h,
                                             double dx, double two_dx) {
  const double high = has_h ? h : f, low = has_l ? l : f;
  const double quotient = __ddiv_rn(high - low, (has_l && has_h) ? two_dx : dx);
  return (has_l || has_h) ? quotient : 0.0;
}
__device__ __forceinline__ double differences(double f, double l, uint32_t has_l, double h,
                                              uint32_t has_h, double dx, double two_dx) {
  return difference(f, l, has_l & 1u, h, has_h & 1u, dx, two_dx);
}
__device__ __forceinline__ double2_t differences(double2_t f, double2_t l, uint32_t has_l,
                                                 double2_t h, uint32_t has_h, double dx,
                                                 double two_dx) {
  double2_t r = {difference(f.x, l.x, has_l & 1u, h.x, has_h & 1u, dx, two_dx),
                 difference(f.y, l.y, has_l & 2u, h.y, has_h & 2u, dx, two_dx)};
  return r;
}

// Along x the neighbours of a lane's cells are the one cell before them, the cells themselves and
// the one cell after them.
__device__ __forceinline__ double low_along_x(double, double before) { return before; }
__device__ __forceinline__ double2_t low_along_x(double2_t f, double before) {
  double2_t r = {before, f.x};
  return r;
}
__device__ __forceinline__ double high_along_x(double, double after, bool) { return after; }
__device__ __forceinline__ double2_t high_along_x(double2_t f, double after, bool whole) {
  double2_t r = {whole ? f.y : after, after};
  return r;
}

struct TileCoords {
  constant_box* box;
  CellTile at;
};

// What a lane holds of one pass before the arithmetic.
template <class V>
struct Pass {
  V f, low, high;
  uint32_t has_low, has_high;  // bit c: the neighbour of cell c is there
  uint32_t out_at;
  bool valid;
};

// One tile with N cells per lane and pass: N == 2 needs input and output 16-byte aligned with even
// strides (box.paired).
template <int AXIS, class V, int N>
__device__ __forceinline__ void gradient_tile(const GradientArgs& a, const TileCoords& tile) {
  // the box's descriptor, once per tile and through the constant address space: scalar loads
  constant_box* box = tile.box;
  const int nx = box->nx, ny = box->ny, nz = box->nz;
  const_global_double* in = (const_global_double*)box->in;
  global_double* out = (global_double*)box->out;
  const uint32_t ji = static_cast<uint32_t>(box->jstride_in);
  const uint32_t ki = static_cast<uint32_t>(box->kstride_in);
  const uint32_t jo = static_cast<uint32_t>(box->jstride_out);
  const uint32_t ko = static_cast<uint32_t>(box->kstride_out);
  const double dx = box->dx, two_dx = 2.0 * dx;
  const uint32_t face = box->face_begin;
  const_global_double* value_lo = (const_global_double*)a.face_value + face;
  const_global_double* value_hi = value_lo + a.n_faces;
  const_global_u8* present_lo = (const_global_u8*)a.face_present + face;
  const_global_u8* present_hi = present_lo + a.n_faces;
  constexpr int kLanesPerRow = kClassifyChunk / N;       // 64 or 128
  constexpr int kRowsPerPass = kThreads / kLanesPerRow;  // 4 or 2
  constexpr int kPasses = 16 / kRowsPerPass;             // 4 or 8
  constexpr uint32_t kAll = (1u << N) - 1u;
  const int t = static_cast<int>(threadIdx.x);
  const int i = tile.at.chunk * kClassifyChunk + (t % kLanesPerRow) * N;
  const uint32_t ui = static_cast<uint32_t>(i);
  const bool whole = i + N - 1 < nx;
  const int cells = whole ? N : 1;  // of this lane that lie in the row
  const V zero = V();
  for (int batch = 0; batch < kPasses / kBatch; ++batch) {
    Pass<V> pass[kBatch];
    // every load of the batch, before any arithmetic
#pragma unroll
    for (int p = 0; p < kBatch; ++p) {
      Pass<V>& s = pass[p];
      const int row = (batch * kBatch + p) * kRowsPerPass + t / kLanesPerRow;
      const uint32_t j = static_cast<uint32_t>(tile.at.bj * kBrickY + (row & 3));
      const uint32_t k = static_cast<uint32_t>(tile.at.bk * kBrickZ + (row >> 2));
      s.valid = i < nx && static_cast<int>(j) < ny && static_cast<int>(k) < nz;
      s.f = s.low = s.high = zero;
      s.has_low = s.has_high = 0;
      s.out_at = ui + j * jo + k * ko;
      if (!s.valid) continue;
      const uint32_t at = ui + j * ji + k * ki;
      s.f = load_cells(in, at, whole, V());
      if (AXIS == 0) {
        const uint32_t plane = j + k * static_cast<uint32_t>(ny);
        double before, after;
        uint32_t has_before = 1, has_after = 1;
        if (i > 0) {
          before = in[at - 1];
        } else {
          before = value_lo[plane];
          has_before = present_lo[plane];
        }
        if (i + cells < nx) {
          after = in[at + static_cast<uint32_t>(cells)];
        } else {
          after = value_hi[plane];
          has_after = present_hi[plane];
        }
        s.low = low_along_x(s.f, before);
        s.high = high_along_x(s.f, after, whole);
        // the cells between the lane's ends have both neighbours
        s.has_low = (kAll & ~1u) | has_before;
        s.has_high = whole ? ((kAll >> 1) | has_after << (N - 1)) : has_after;
      } else {
        const uint32_t index = AXIS == 1 ? j : k;
        const int n = AXIS == 1 ? ny : nz;
        const uint32_t stride = AXIS == 1 ? ji : ki;
        const uint32_t plane = ui + (AXIS == 1 ? k : j) * static_cast<uint32_t>(nx);
        if (index > 0) {
          s.low = load_cells(in, at - stride, whole, V());
          s.has_low = kAll;
        } else {
          s.low = load_face(value_lo, plane, whole, V());
          s.has_low = load_present(present_lo, plane, whole, V());
        }
        if (static_cast<int>(index) + 1 < n) {
          s.high = load_cells(in, at + stride, whole, V());
          s.has_high = kAll;
        } else {
          s.high = load_face(value_hi, plane, whole, V());
          s.has_high = load_present(present_hi, plane, whole, V());
        }
      }
    }
#pragma unroll
    for (int p = 0; p < kBatch; ++p) {
      const Pass<V>& s = pass[p];
      const V value = differences(s.f, s.low, s.has_low, s.high, s.has_high, dx, two_dx);
      if (s.valid) store_cells(out, s.out_at, whole, value);
    }
  }
}

template <int AXIS>
__global__ __launch_bounds__(kThreads) void gradient_kernel(const GradientArgs a) {
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
      gradient_tile<AXIS, double2_t, 2>(a, tile);
    } else {
      gradient_tile<AXIS, double, 1>(a, tile);
    }
  }
}

}  // namespace

int launch_gradient(const GradientArgs& args, int axis, void* stream_v) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (args.n_tiles == 0) return AVR_OK;
  const uint32_t halo_groups = static_cast<uint32_t>((2ull * args.n_faces + kThreads - 1) / kThreads);
  const uint32_t groups = (args.n_tiles + kTilesPerGroup - 1) / kTilesPerGroup;
#define AVR_GRADIENT(A)                                                                          \
  case A:                                                                                        \
    hipLaunchKernelGGL(gradient_halo_kernel<A>, dim3(halo_groups), dim3(kThreads), 0, stream,    \
                       args);                                                                    \
    hipLaunchKernelGGL(gradient_kernel<A>, dim3(groups), dim3(kThreads), 0, stream, args);       \
    break
  switch (axis) {
    AVR_GRADIENT(0);
    AVR_GRADIENT(1);
    AVR_GRADIENT(2);
    default: set_error("gradient_kernel: axis must be 0, 1 or 2"); return AVR_ERR_INVALID_ARGUMENT;
  }
#undef AVR_GRADIENT
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error(std::string("gradient_kernel: ") + hipGetErrorString(err));
    return AVR_ERR_RUNTIME;
  }
  return AVR_OK;
}

}  // namespace avr
