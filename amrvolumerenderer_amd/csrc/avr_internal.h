// Internal types shared by the host prologue (avr_host.cpp), the kernels (avr_kernels.hip)
// and the C ABI (avr_capi.cpp).  Not part of the public boundary (include/avr_hip.h).
#ifndef AVR_INTERNAL_H
#define AVR_INTERNAL_H

#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <variant>
#include <vector>

#include "../../include/avr_hip.h"

// host and device where the compiler is hipcc
#if defined(__HIP__)
#define AVR_HD __host__ __device__
#else
#define AVR_HD
#endif

#include "avr_level_cells.h"  // kFieldMaxLevels; after AVR_HD, which it would otherwise define
#include "avr_brick_address.h"  // pow2_brick_shifts, pow2_brick_offset

namespace avr {

constexpr int kTableSize = 256;  // kColorTableSize, Common/VolumePainter.cpp:35
constexpr int kMaxLdsTables = 16;  // transfer-function tables staged in LDS per launch (4 KiB each)

// Cell index = floor((pos - min) / dx) with an IEEE divide in the reference
// (Common/VolumePainter.cpp:846-852).  The same integer is obtained cheaper when provable:
enum IndexMode : int32_t {
  kPow2Multiply = 0,  // dx is a power of two: (pos - min) * (1/dx) IS the correctly rounded quotient,
                      // and so is fma(pos, 1/dx, -min/dx): scaling by 2^k commutes with rounding
                      // (the host admits the mode only for magnitudes where nothing is subnormal)
  kReciprocal = 1,    // q = (pos - min) * RN(1/dx) is within 2^-22 * q of the rounded quotient, so
                      // floor(q) is the reference's index unless q is within near_tol of an
                      // integer; those samples take the exact divide
  kExactDivide = 2,   // degenerate spacing (dx <= 0 or not finite): always the exact divide
  kPow2Bricks = 3,    // kPow2Multiply, and the box's y and z bricklet counts are powers of two as
                      // well (pow2_brick_shifts, avr_brick_address.h): in a launch whose boxes all
                      // have this mode the interior loops of the march build the bricklet offset in
                      // four instructions; in any other launch the box is marched as kPow2Multiply
};

// Per-box constants of VolumePainter::paint's host prologue (Common/VolumePainter.cpp:571-692),
// laid out for wave-uniform scalar loads (one 128-byte record per box).
struct alignas(16) BoxDev {
  float minc[3];
  float maxc[3];
  float dx, dy, dz;       // (maxCornerF - minCornerF) / float(n)   (:678-686)
  float mesh_eps;         // 1e-4 * |diag|                          (:688-692)
  float sample_dist;      // max(0.5 * minSpacing, 1e-5)            (:600)
  int32_t nx, ny, nz;
  int32_t lut;            // index of this box's transfer-function table
  int32_t rect[4];        // conservative screen rectangle x0,y0,x1,y1 (inclusive); x1 < x0 = off-screen
  int32_t index_mode;     // how (pos - min) / dx is evaluated, see IndexMode
  const double* cells;    // values(validBox.smallEnd(), component)
  int32_t jstride;        // element strides (Array4); the box spans < 2^28 elements
  int32_t kstride;
  float inv_dx, inv_dy, inv_dz;  // RN(1 / dx)
  float near_tol;         // kReciprocal: |q - rint(q)| <= near_tol sends the sample to the exact divide
  int32_t brick_sy;       // kPow2Bricks: bit of the y bricklet pitch (pow2_brick_shifts), else 0
  uint64_t cls_offset;    // byte offset of this box's classified bricklets in the frame's buffer
  float nmin_inv[3];      // kPow2Multiply: -(minc * inv_d), exact (a power-of-two scaling)
  int32_t brick_sx;       // kPow2Bricks: bit of the x bricklet pitch, else 0
};
static_assert(sizeof(BoxDev) == 144, "BoxDev is read with scalar loads: keep it a multiple of 16 bytes");

// A speculative frame's bookkeeping on the device (render_runs_kernel; all arrays by position in
// the global layer order).
struct MarchSpecDev {
  const uint8_t* classified;  // != 0: this frame's classify pass covered the box; nullptr: every box
  uint8_t* visited;           // out: set for every box some wave marched; nullptr: not recorded
  uint8_t* missed;            // out: boxes a ray needed that `classified` left out
  uint32_t* miss_count;       // out: one per (wave, box) miss
  uint32_t* host_miss_flag;   // out, host-mapped or nullptr: set to 1 on a miss
  const uint32_t* gate;       // nullptr, or: the launch does nothing unless *gate != 0
  uint8_t* dirty_blocks_out;  // out, or nullptr: per workgroup of the grid, 1 = it met an unclassified box
  const uint8_t* dirty_blocks;  // gated launch: nullptr, or only these workgroups run again
};

// Frame constants (camera basis, scalar mapping); passed to kernels by value (kernarg -> SGPRs).
struct FrameConsts {
  int32_t width, height;
  float aspect, tan_half_fov, inv_width, inv_height;
  float fwd[3], right[3], up[3], eye[3];
  float range_min, inverse_range, clip_start;
  int32_t apply_clip;
  int32_t log_scale, normalize;
  double positive_floor, norm_min, inv_norm_span;
};

// Classified volume: every cell's transfer-function table index (uint8) in 128-byte bricklets
// of 8 x 4 x 4 cells (x fastest inside a bricklet; bricklets z-fastest, then y, then x inside the
// box: see bricklet_offset in avr_kernels.hip).
constexpr int kBrickX = 8, kBrickY = 4, kBrickZ = 4, kBrickBytes = 128;
constexpr int kClassifyChunk = 128;  // cells of one x-row handled by one classify workgroup
// the standard API path of the scalar mapping (normalise on, scalarRange {0,1}, no log, no soft clip)
inline bool standard_transform(const FrameConsts& fc) {
  return !fc.log_scale && fc.normalize && !fc.apply_clip && fc.range_min == 0.0f &&
         fc.inverse_range == 1.0f;
}
// Whether classify_wave_kernel (a wave per quarter tile, avr_kernels.hip) can classify the box:
// every quarter tile of it lies wholly inside and is read by 16-byte loads at 32-bit byte
// offsets, which is what classify_kernel asks of a tile before it takes its straight-line path.
// A box without cells has no tiles and fits any launch.
inline bool classify_wave_box(const BoxDev& box, const FrameConsts& fc) {
  if (box.nx <= 0 || box.ny <= 0 || box.nz <= 0) return true;
  return standard_transform(fc) && (reinterpret_cast<uintptr_t>(box.cells) & 15u) == 0 &&
         (box.jstride & 1) == 0 && (box.kstride & 1) == 0 && box.jstride < (1 << 27) &&
         box.nx % (kClassifyChunk / 4) == 0 && box.ny % kBrickY == 0 && box.nz % kBrickZ == 0;
}

// How the image's pixels are dealt to the N pieces of the direct-send exchange (one piece per
// rank of the compositing group).
//   kPiecesContiguous  the reference's partition: piece k = pixels [k * floor(P/N), ...), the
//                      last piece takes the remainder (getPieceRange, DirectSendBase.cpp:59-74).
//                      What Compositor::compose promises its caller, so the plugin keeps it.
//   kPiecesRowBands    bands of `band_rows` image rows dealt round-robin: band b belongs to piece
//                      b % N.  The scene covers a compact part of the screen, so contiguous
//                      pieces leave some ranks with nothing to receive and fold and others with
//                      everything (config-4, N = 8: 36.5 MB against 0); dealt bands give every
//                      rank the same share of every region.  Per-pixel results do not depend on
//                      which rank folds a pixel, so the gathered image is the same bit for bit;
//                      only the frame driver (whose caller sees the gathered image, never the
//                      pieces) uses it.
// A piece's rows are numbered 0, 1, ... in image order ("piece rows"); with contiguous pieces a
// piece row IS the image row (blocks count rows from the image's row 0 there).
enum PieceLayout : int32_t { kPiecesContiguous = 0, kPiecesRowBands = 1 };
struct PieceMapDev {
  int32_t layout = kPiecesContiguous;
  int32_t band_rows = 1;
  int32_t n_pieces = 1;
  int32_t width = 0, height = 0;
  int32_t pad_ = 0;
  int64_t piece_size = 0;  // kPiecesContiguous: floor(P / N)
};
AVR_HD inline int piece_of_row(const PieceMapDev& m, int y) { return (y / m.band_rows) % m.n_pieces; }
// position of image row y among the rows of its piece (kPiecesRowBands)
AVR_HD inline int piece_row_of(const PieceMapDev& m, int y) {
  return (y / (m.band_rows * m.n_pieces)) * m.band_rows + y % m.band_rows;
}
// image row of piece row j of piece k (kPiecesRowBands)
AVR_HD inline int image_row_of(const PieceMapDev& m, int k, int j) {
  return ((j / m.band_rows) * m.n_pieces + k) * m.band_rows + j % m.band_rows;
}
// number of rows of piece k (kPiecesRowBands)
AVR_HD inline int piece_row_count(const PieceMapDev& m, int k) {
  const int cycle = m.band_rows * m.n_pieces;
  const int rest = m.height % cycle - k * m.band_rows;  // rows of the last, partial cycle left for k
  return (m.height / cycle) * m.band_rows + (rest <= 0 ? 0 : (rest < m.band_rows ? rest : m.band_rows));
}

// Sparse run layers: a run's layer is stored only inside the run's screen rectangle, cut into
// one block per DirectSend piece (include/avr_hip.h, "frame plan").
struct RunRectDev {
  int32_t x0, y0, x1, y1;  // inclusive; x1 < x0 = empty
};
struct RunBlockDev {
  int64_t offset;     // float offset of the block in the send / recv buffer (unused if empty)
  int32_t first_row;  // piece row (contiguous pieces: image row) stored in the block's first row
  int32_t span_base;  // < 0: every row holds the run rectangle's x0..x1; else the block's rows are
                      // entries span_base + (row - first_row) of the span table
};
// One row of a block of a tightened frame plan (avr_frame_plan_tighten): only the pixels
// x0..x1 of the row are stored, starting `rel` floats after the block's offset; the others are
// known to be empty (conservative per-row extent of the run's boxes on screen).  8 bytes per row:
// the two span tables of a frame travel with its descriptors (hundreds of KB at 16).
struct RunSpanDev {
  uint16_t x0, x1;  // inclusive; x1 < x0 = nothing stored for this row
  uint32_t rel;
};
constexpr int kMaxTightenedWidth = 65535;            // x0 / x1 are 16 bit
constexpr int64_t kMaxTightenedBlockFloats = 0xffffffffLL;  // rel is 32 bit

// One unit of march work: a screen super-tile of one run.  Runs are independent (each has its
// own layer, started from the empty pixel), so a rank's runs are marched by different
// workgroups; a frame's critical path is then one run's rays, not all of a rank's boxes.
struct MarchItemDev {
  uint32_t slot;  // Morton index of the super-tile; kNoMarchItem = padding
  uint32_t run;
};
constexpr uint32_t kNoMarchItem = 0xffffffffu;

// Host results for one frame over a list of boxes.
struct FramePlan {
  FrameConsts consts;
  std::vector<BoxDev> boxes;        // same order as the input boxes
  std::vector<float> tables;        // n_tables * 1024 floats
  int n_tables = 0;
  std::vector<uint32_t> classify_tile_begin;  // n_boxes + 1: prefix sum of classify workgroups
  uint64_t classified_bytes = 0;              // size of the frame's classified buffer
  bool ready = false;                         // set by plan_frame
  // the march's work items (build_march_items) of the frame plan this prologue belongs to: they
  // follow from the plan alone, so a camera that repeats does not sort them again (35-45 us of the
  // host's 0.1 ms per frame at N = 8)
  std::vector<MarchItemDev> march_items;
  bool march_items_ready = false;
};

// Screen tiling of the march kernel: workgroup = 16 x 16 pixels, super-tile = 2 x 2 workgroups
// (Morton order inside); the (super-tile, run) items are dealt round-robin to the 8 XCDs in the
// host's cost order.
constexpr int kTile = 16;
constexpr int kSuperTileSide = 2;
constexpr int kSuperTileTiles = kSuperTileSide * kSuperTileSide;
constexpr int kXcds = 8;
// The march items of a frame: for every run the super-tiles its screen rectangle touches, most
// expensive first (estimated samples), padded with kNoMarchItem to a multiple of kXcds.
void build_march_items(const FramePlan& plan, const int32_t* box_order, const int32_t* run_end,
                       int n_runs, const std::vector<RunRectDev>& run_rects,
                       std::vector<MarchItemDev>* items);

// ---- host prologue (avr_host.cpp) ---------------------------------------------------------
void build_color_table(float alpha_scale, float normalization_factor, const float scalar_range[2],
                       const avr_colormap_point* colormap, int colormap_count, float* out_table);
void box_sampling(const avr_box& box, const avr_paint_params& params, float* sample_distance,
                  float* normalization_factor, float* alpha_scale);
float box_depth_hint(const avr_box& box, const avr_camera& camera);
float reference_sample_distance(const avr_box* boxes, int n_boxes, const double bounds_min[3],
                                const double bounds_max[3]);
int layer_order(const float* hints, const int32_t* owner, const int32_t* local_index, int n_layers,
                int32_t* order_out, int32_t* run_end_out);
// Conservative screen rectangle of a box (x0,y0,x1,y1 inclusive; x1 < x0 = off-screen).
void box_screen_rect(const avr_box& box, const avr_camera& camera, int width, int height,
                     int32_t rect[4]);
// The image rows a caller wants extents for: lo <= y <= hi and, with period > 1, only the rows of
// the bands dealt to one piece ((y / band_rows) % period == phase).
struct RowSet {
  int32_t band_rows = 1, period = 1, phase = 0;
  int32_t lo = 0, hi = 0x7fffffff;
};
// Calls f(a, b) for every maximal interval [a, b] of rows of the set inside [lo, hi].
template <typename F>
inline void for_rows(const RowSet& set, int lo, int hi, F&& f) {
  lo = lo > set.lo ? lo : set.lo;
  hi = hi < set.hi ? hi : set.hi;
  if (hi < lo) return;
  if (set.period <= 1) {
    f(lo, hi);
    return;
  }
  int band = lo / set.band_rows;
  band += ((set.phase - band) % set.period + set.period) % set.period;  // first band of the phase
  for (; band * set.band_rows <= hi; band += set.period) {
    const int a = band * set.band_rows, b = a + set.band_rows - 1;
    f(a > lo ? a : lo, b < hi ? b : hi);
  }
}
// A box on screen: its conservative rectangle and the projected corners whose convex hull bounds
// its projection (`whole`: the box reaches behind the eye, every row keeps the whole rectangle).
struct BoxFootprint {
  int32_t rect[4];  // x0, y0, x1, y1 inclusive; x1 < x0 = off-screen
  bool whole = false;
  double px[8], py[8];
};
void box_footprints(const avr_box* boxes, int n_boxes, const avr_camera& camera, int width,
                    int height, BoxFootprint* out);
// Merges (min / max) the box's conservative extent on every row of `rows` inside its rectangle
// into x0[y - y_base], x1[y - y_base]; an entry with x1 < x0 is empty.
void merge_footprint_rows(const BoxFootprint& footprint, const RowSet& rows, int y_base,
                          int32_t* x0, int32_t* x1);
// Per-row extent inside that rectangle (rows rect[1]..rect[3]; x1 < x0 = nothing on the row).
void box_row_spans(const avr_box& box, const avr_camera& camera, int width, int height,
                   const int32_t rect[4], std::vector<int32_t>* row_x0,
                   std::vector<int32_t>* row_x1);
// Fills plan for the given boxes; throws std::invalid_argument / std::runtime_error.
void plan_frame(const avr_box* boxes, int n_boxes, const avr_scalar_transform& transform,
                const avr_paint_params& params, const avr_camera& camera, FramePlan* plan);

// What a frame's pixels are.  The march, the layers' encoding and the fold depend on it; the plan,
// the exchange and the gather carry every kind alike.
enum class FrameKind : int {
  kVolume,        // emission-absorption through the transfer function: Layer5 pixels, blended
  kMaxIntensity,  // the largest table index along the ray; the fold takes the maximum
  kProjection,    // column and length of the raw f64 cells along the ray; the fold adds
};

// ---- kernel launchers (avr_kernels.hip); all asynchronous on `stream` (hipStream_t) ---------
struct RenderLaunch {
  FrameConsts consts;
  const BoxDev* boxes_dev;      // scene descriptors for this frame
  const float* tables_dev;      // n_tables * 1024 floats
  int n_tables;
  const int32_t* order_dev;     // box indices in global layer order
  const int32_t* order_rects_dev;  // their conservative screen rectangles (x0, y0, x1, y1), same order
  const MarchSpecDev* spec_dev = nullptr;  // a speculative frame's bookkeeping (staged per launch)
  bool spec_is_repair = false;             // ... of its gated second march (a kernel name of its own)
  const uint32_t* classify_gate = nullptr;  // launch_classify: the gated small-grid kernel
  const int32_t* run_end_dev;   // one-past-last position per run
  int n_order, n_runs, n_pieces;
  const RunRectDev* run_rects_dev;    // n_runs
  const RunBlockDev* run_blocks_dev;  // n_runs x n_pieces
  const RunSpanDev* run_spans_dev;    // rows of the blocks with span_base >= 0 (may be null)
  PieceMapDev pieces;                 // which piece a pixel's row belongs to
  float* out_layers;
  unsigned long long* samples_out;  // may be null
  unsigned long long* counters;     // diagnostics (4 x uint64), only read when samples_out is set
  uint8_t* classified;              // frame's classified buffer (FramePlan::classified_bytes)
  const uint32_t* tile_begin_dev;   // n_boxes + 1 prefix of classify workgroups
  int n_boxes;
  uint32_t n_classify_tiles;
  uint32_t classify_lds_pad;  // bytes of LDS each classify workgroup claims beyond its own
                              // (0 = none): caps its occupancy beside the march
  int classify_stream_stores;  // the classified bricklets are written through to memory as a
                               // stream (their reader is a frame away) instead of stored plainly
  bool classify_by_wave = false;  // every box takes classify_wave_kernel (classify_wave_box)
  const MarchItemDev* items_dev;  // n_items entries (multiple of kXcds)
  uint32_t n_items;
  int only_mode;                        // the IndexMode shared by every box, or -1
  int workgroups_per_cu;                // resident march workgroups per CU (0 = uncapped)
  // A frame in depth-ordered chunks (avr_classify_plan_chunked / avr_march_plan_chunked): the
  // classify launch takes the n_classify_boxes boxes listed in box_list_dev (tile_begin_dev is
  // then the chunk's prefix), the march launch the positions [pos_begin, pos_end) of the global
  // layer order, its run accumulators resumed from what the launch before stored.
  const int32_t* box_list_dev = nullptr;
  int n_classify_boxes = 0;
  int pos_begin = 0, pos_end = -1;      // pos_end < 0: n_order
  int resume = 0;
  // occlusion culling between the chunks (avr_render_plan_culled): the march launch of chunk k
  // flags the boxes behind it that a ray may still sample (indexed by position in the global layer
  // order), the classify launch of chunk k + 1 leaves out the others (indexed like its box list)
  uint8_t* visible_out = nullptr;
  const uint8_t* visible_in = nullptr;
  // kMaxIntensity (render_runs_max_kernel) and kProjection (render_runs_sum_kernel: no classify
  // pass, the raw cells, no tables) are one launch each: no chunks, no culling, no speculation
  FrameKind kind = FrameKind::kVolume;
};
// classify pass (cells -> table indices) and march; the march reads what the classify pass of
// the same frame wrote into `classified`
// Copies `bytes` (rounded up to 16; both blocks are that large) from device-mapped pinned host
// memory to device memory.
int launch_upload(const void* host_mapped, void* dev, size_t bytes, void* stream);
int launch_stall(int milliseconds, void* stream);  // test hook: a bounded busy kernel
int launch_classify(const RenderLaunch& launch, void* stream);
int launch_march(const RenderLaunch& launch, void* stream);
int launch_blend(int kind, const void* top, const void* bottom, void* out, int64_t n, void* stream);
int launch_blend_regions(int kind, const void* top, int64_t tb, int64_t te, const void* bottom,
                         int64_t bb, int64_t be, void* out, void* stream);
int launch_encode_u8(const float* rgba, uint32_t* out, int64_t n, void* stream);
int launch_decode_u8(const uint32_t* in, float* rgba, int64_t n, void* stream);
// The two pieces a fold writes (piece order; either may be null), each kind with its own types:
// kVolume the Layer5 piece and its RGB8 bytes, kMaxIntensity the index piece (-1 = no sample) and
// the winner's RGB8 bytes, kProjection the f64 column and length pieces.
template <FrameKind KIND, typename FIRST, typename SECOND>
struct FoldPair {
  static constexpr FrameKind kKind = KIND;
  using First = FIRST;
  using Second = SECOND;
  FIRST* first = nullptr;
  SECOND* second = nullptr;
};
// The outputs of one fold: one kind's pair (the alternative's index is the kind).
using FoldOut = std::variant<FoldPair<FrameKind::kVolume, float, uint8_t>,
                             FoldPair<FrameKind::kMaxIntensity, int16_t, uint8_t>,
                             FoldPair<FrameKind::kProjection, double, double>>;
template <FrameKind KIND>
using FoldOutputs = std::variant_alternative_t<static_cast<size_t>(KIND), FoldOut>;
struct FoldLaunch {
  int width;
  PieceMapDev pieces;
  int piece;                           // this rank's piece
  int64_t piece_begin, piece_end;      // contiguous pieces: the image's pixel range; row bands: [0, n)
  int n_runs;                          // global runs, in order
  const RunRectDev* run_rects_dev;     // n_runs
  const RunBlockDev* run_blocks_dev;   // n_runs: block of this rank's piece in the recv buffer
  const RunSpanDev* run_spans_dev;     // rows of the blocks with span_base >= 0 (may be null)
  const float* recv;
  FoldOut out;
  // Blocks whose offset in the receive layout lies in [own_begin, own_end) -- the rank's own runs
  // -- are read own_delta floats away from there: from the send buffer the march stored them in
  // (avr_fold_plan_own).  own_begin == own_end: everything from recv.
  int64_t own_begin = 0, own_end = 0, own_delta = 0;
  int max_workgroups = 0;              // grid cap (0: the default, 2048)
  int flip_height = 0;                 // > 0: the RGB8 output is the whole image, rows top-down (one rank)
};
// Picture of a column projection (width x height f64 column and length, row 0 at the bottom):
// per pixel the quantity (column, or column / length if mean; log10 if log_scale) of pixels with
// length > 0 (and a quantity > 0 under log) -> table entry clamp(floor((q - lo) / (hi - lo) * 255),
// 0, 255) -> rgb_table's 3 bytes, (0, 0, 0) otherwise; rgb8 rows top-down.  range (device, 2 f64):
// [lo, hi] -- computed there first if auto_range (min / max over the pixels that take part, (0, 1)
// if none), with partial (device, 2 * kProjectionRangeWorkgroups f64) as scratch.
constexpr int kProjectionRangeWorkgroups = 256;
int launch_projection_colorize(const double* column, const double* length, int width, int height,
                               int mean, int log_scale, double* range, int auto_range,
                               double* partial, const uint8_t* rgb_table, uint8_t* rgb8,
                               void* stream);
int launch_fold_plan(const FoldLaunch& launch, void* stream);
int launch_fold_runs(const float* const* slices_dev, int n_slices, float* out, int64_t n,
                     void* stream);
int launch_downsample(const float* src, int tw, int th, int block, float* dst, void* stream);
int launch_quantize(const float* src, int w, int h, int stride, uint8_t* dst, void* stream);
int launch_flip_rows(const uint8_t* src, int64_t row_bytes, int h, uint8_t* dst, void* stream);
// Gathered, piece-major rows (row bands: piece 0's rows, then piece 1's, ...) -> image order;
// flip != 0 also turns the image upside down (bottom-up image -> top-down file rows).
// own (may be null): piece own_piece is read from there instead of from src.
int launch_assemble_rows(const PieceMapDev& pieces, const uint8_t* src, int64_t row_bytes, int flip,
                         uint8_t* dst, void* stream, const uint8_t* own = nullptr, int own_piece = -1);

constexpr uint32_t kScanWorkgroups = 2048;  // grid of the grid-stride cell scans
// scene statistics (avr_scene_stats.hip).  partial_dev: kScanWorkgroups x 32 bytes of scratch;
// out_dev: 32 bytes {min, max, min positive (double), finite count (int64)}.
int launch_scalar_stats(const BoxDev* boxes_dev, const uint32_t* tile_begin_dev, int n_boxes,
                        uint32_t n_tiles, void* partial_dev, void* out_dev, void* stream);
int launch_histogram(const FrameConsts& consts, const BoxDev* boxes_dev,
                     const uint32_t* tile_begin_dev, int n_boxes, uint32_t n_tiles,
                     float range_min, float range_max, int bin_count, uint64_t* counts_dev,
                     void* stream);
// BoxDev records + classify tiling of a box list without any camera (scene statistics).
void plan_cells(const avr_box* boxes, int n_boxes, const avr_scalar_transform& transform,
                FramePlan* plan);
// The scalar-transform part of BuildSceneGeometry (SceneBuilder.cpp:315-443); throws
// std::runtime_error like the reference.
void scene_transform_from_stats(const double stats[3], int64_t finite_count, bool log_scale,
                                bool normalize_to_data_range, avr_scalar_transform* transform,
                                double processed[2], float processed_range[2],
                                float scalar_range[2]);

// Slice images (avr_slice.hip).  A box as the slice kernel reads it: the f64 corners of avr_box
// (the containment test is done in binary64, unlike the march's float prologue), the cell
// addressing and what a pixel reports.  A box without cells has max = min: it contains no point.
struct alignas(16) SliceBoxDev {
  double minc[3];
  double maxc[3];
  int32_t n[3];
  int32_t level;
  const double* cells;
  int32_t jstride;        // element strides (Array4); the box spans < 2^28 elements
  int32_t kstride;
  int32_t global_index;   // what the box image holds for this box
  int32_t pad_[3];
};
static_assert(sizeof(SliceBoxDev) == 96, "SliceBoxDev: 16-byte multiple for scalar loads");
// Pixel (x, y) samples (origin + (x + 0.5) * du) + (y + 0.5) * dv, scene coordinates.
struct SlicePlaneDev {
  double origin[3], du[3], dv[3];
};
int launch_slice(const SlicePlaneDev& plane, int width, int height, const SliceBoxDev* boxes_dev,
                 int n_boxes, double* value, int8_t* level, int32_t* box_index, void* stream);
int launch_slice_outline(const int32_t* box_index, int width, int height, int red, int green,
                         int blue, uint8_t* rgb8, void* stream);

// Joint histogram (avr_joint_histogram.hip).  A box as that kernel reads it: the cells of the x,
// y and s fields (an absent field repeats x) with each field's own strides, the dims and the level
// they share.
struct alignas(16) JointBoxDev {
  const double* cells[3];
  int32_t jstride[3];     // element strides (Array4); every field spans < 2^28 elements
  int32_t kstride[3];
  int32_t nx, ny, nz;
  int32_t level;          // 0 .. n_levels - 1
  int32_t paired;         // every field: cells 16-byte aligned, both strides even
  int32_t pad_[3];
};
static_assert(sizeof(JointBoxDev) == 80, "JointBoxDev: 16-byte multiple for scalar loads");
constexpr int kJointHistogramMaxBins = 1024;          // per axis
constexpr int kJointHistogramMaxCells = 1 << 20;      // nx * ny
// Dynamic LDS of one workgroup (edges + counts + sums) up to which the bins are kept in LDS; above
// it every cell goes to the global arrays.  64 KiB: what a kernel gets without asking for more,
// and at least two workgroups (8 waves) per CU at the limit.
constexpr size_t kJointHistogramLdsBudget = 64 * 1024;
struct JointHistogramArgs {
  const JointBoxDev* boxes;
  const uint32_t* tile_begin;   // n_boxes + 1: prefix sum of the boxes' tiles
  int32_t n_boxes;
  uint32_t n_tiles;
  const double* x_edges;        // nx + 1, device
  const double* y_edges;        // ny + 1, device (null without y)
  int32_t nx, ny;
  double x_lo, x_hi, x_scale;   // e[0], e[n] and nx / (e[n] - e[0]) (0 if that is not finite)
  double y_lo, y_hi, y_scale;
  unsigned long long* cells;    // [n_levels][ny][nx], added to
  double* sums;                 // the same shape (null without s), added to
  unsigned long long* totals;   // [2]: outside, nonfinite, added to
};
size_t joint_histogram_lds_bytes(int nx, int ny, bool has_y, bool has_s, bool lds);
int launch_joint_histogram(const JointHistogramArgs& args, bool has_y, bool has_s, void* stream);

// On-axis projection (avr_axis_projection.hip).  Stage 1 reduces every box's columns along the
// axis into partial planes, one per segment of kAxisSegment cells: S (f64), Wt (f64, with a
// weight) and n (u32), each [segments][dims_V][dims_U] at `plane_begin`.  Stage 2 gathers them per
// pixel.  A box as stage 1 reads it:
constexpr int kAxisSegment = 128;      // cells of a column that one partial sum covers
struct alignas(16) AxisBoxDev {
  const double* cells_f;
  const double* cells_w;  // == cells_f without a weight (not read)
  int32_t jstride_f, kstride_f;  // element strides (Array4); every field spans < 2^28 elements
  int32_t jstride_w, kstride_w;
  int32_t nx, ny, nz;
  int32_t paired;         // both fields: cells 16-byte aligned, both strides even
  uint32_t plane_begin;   // first entry of the box's partial planes
  int32_t pad_[3];
};
static_assert(sizeof(AxisBoxDev) == 64, "AxisBoxDev: 16-byte multiple for scalar loads");
// ... and as stage 2 reads it: the f64 corners of avr_box on the image axes (max = min for a box
// without cells: it contains no line), the plane's shape and the level's path length.
struct alignas(16) AxisPlaneDev {
  double min_u, max_u, min_v, max_v;
  double dl;
  int32_t n_u, n_v;
  int32_t segments;
  uint32_t plane_begin;
  int32_t pad_[2];
};
static_assert(sizeof(AxisPlaneDev) == 64, "AxisPlaneDev: 16-byte multiple for scalar loads");
struct AxisReduceArgs {
  const AxisBoxDev* boxes;
  const uint32_t* tile_begin;   // n_boxes + 1: prefix sum of the boxes' tiles
  int32_t n_boxes;
  uint32_t n_tiles;
  double* plane_s;
  double* plane_w;              // null without a weight
  uint32_t* plane_n;
};
struct AxisGatherArgs {
  const AxisPlaneDev* boxes;
  int32_t n_boxes;
  int32_t width, height;
  double origin_u, origin_v, du, dv;
  const double* plane_s;
  const double* plane_w;        // null without a weight
  const uint32_t* plane_n;
  double* integral;
  double* weight;               // null without a weight
  double* length;
};
// tiles of one box in stage 1 for `axis` (0 = x, 1 = y, 2 = z); UINT32_MAX if they do not fit 31 bits
uint32_t axis_projection_tiles(int axis, int nx, int ny, int nz);
int launch_axis_reduce(const AxisReduceArgs& args, int axis, bool weighted, void* stream);
int launch_axis_gather(const AxisGatherArgs& args, void* stream);

// Derived fields (avr_derive.hip).  A program is postfix: one word per instruction, the opcode in
// the low byte and the operand index (of a constant, a field or a built-in) above it.
enum DeriveOp : uint32_t {
  kDeriveConst = 0,   // push constants[operand]
  kDeriveField = 1,   // push the cell of field `operand`
  kDeriveBuiltin = 2, // push built-in `operand` (DeriveBuiltin)
  kDeriveAdd = 3, kDeriveSub = 4, kDeriveMul = 5, kDeriveDiv = 6,
  kDeriveNeg = 7, kDeriveSquare = 8, kDeriveSqrt = 9, kDeriveAbs = 10,
  kDeriveMin = 11, kDeriveMax = 12,
  kDeriveLt = 13, kDeriveLe = 14, kDeriveGt = 15, kDeriveGe = 16, kDeriveEq = 17, kDeriveNe = 18,
  kDeriveWhere = 19,
  kDeriveOpCount = 20
};
enum DeriveBuiltin : uint32_t {
  kDeriveX = 0, kDeriveY = 1, kDeriveZ = 2, kDeriveDx = 3, kDeriveDy = 4, kDeriveDz = 5,
  kDeriveCellVolume = 6, kDeriveLevel = 7, kDeriveBuiltinCount = 8
};
constexpr int kDeriveMaxFields = 6;
constexpr int kDeriveMaxInstructions = 64;
constexpr int kDeriveMaxConstants = 16;
constexpr int kDeriveMaxDepth = 8;
// A box as the kernel reads it: the cells of the input fields and of the output (entry
// kDeriveMaxFields of the strides), each with its own strides, the dims and the level they share,
// and the physical position of the box's low corner.
struct alignas(16) DeriveBoxDev {
  const double* cells[kDeriveMaxFields];  // null from n_fields on (not read)
  double* out;
  double origin[3];
  int32_t jstride[kDeriveMaxFields + 1];  // element strides (Array4); every field spans < 2^28
  int32_t kstride[kDeriveMaxFields + 1];
  int32_t nx, ny, nz;
  int32_t level;          // 0 .. n_levels - 1
  int32_t paired;         // every input and the output: cells 16-byte aligned, both strides even
  int32_t pad_[1];
};
static_assert(sizeof(DeriveBoxDev) == 160, "DeriveBoxDev: 16-byte multiple for scalar loads");
// The program and the per-level cell sizes, staged in device memory: the kernel indexes them at
// run time, which a copy in the kernel's arguments does not allow without scratch.
struct alignas(16) DeriveProgramDev {
  uint32_t code[kDeriveMaxInstructions];
  double constants[kDeriveMaxConstants];
  double cell_size[kFieldMaxLevels][3];
};
struct DeriveArgs {
  const DeriveBoxDev* boxes;
  const uint32_t* tile_begin;   // n_boxes + 1: prefix sum of the boxes' tiles
  const DeriveProgramDev* program;
  int32_t n_boxes;
  uint32_t n_tiles;
  int32_t n_fields, n_instructions;
};
int launch_derive(const DeriveArgs& args, void* stream);

// Gradient fields (avr_gradient.hip).  Stage 1 (halo) fills, per box, the two face planes of the
// axis: one f64 and one presence byte per face cell, the face's cells numbered along the lower of
// the two other axes first.  Stage 2 (difference) streams every cell once and reads the planes at
// the box's two faces.  A box as both kernels read it:
struct alignas(16) GradientBoxDev {
  const double* in;
  double* out;
  double dx;              // the cell size of the box's level along the axis
  int32_t jstride_in, kstride_in;    // element strides (Array4); every field spans < 2^28
  int32_t jstride_out, kstride_out;
  int32_t nx, ny, nz;     // 0 for a box without cells
  int32_t level;          // 0 .. n_levels - 1
  int32_t lo[3];          // the index of the box's first cell in its level's index space
  int32_t paired;         // input and output: cells 16-byte aligned, both strides even
  uint32_t face_begin;    // first entry of the box's face planes
  int32_t pad_[1];
};
static_assert(sizeof(GradientBoxDev) == 80, "GradientBoxDev: 16-byte multiple for scalar loads");
struct LevelRatiosDev {
  int32_t ratio[kFieldMaxLevels];  // ratio[l]: level l -> l + 1 (1 from n_levels - 1 on)
};
struct GradientArgs {
  const GradientBoxDev* boxes;
  const uint32_t* tile_begin;   // n_boxes + 1: prefix sum of the boxes' tiles (difference)
  const uint32_t* face_begin;   // n_boxes + 1: prefix sum of the boxes' face cells (halo)
  // CSR over (box, side): the boxes whose cells can hold a ghost of that face, in scene order
  const uint32_t* candidate_begin;  // 2 n_boxes + 1; entry 2 b + side
  const int32_t* candidates;
  const LevelRatiosDev* levels;
  int32_t n_boxes, n_levels;
  uint32_t n_tiles;
  uint32_t n_faces;             // face cells of one side, all boxes
  double* face_value;           // [2][n_faces]: the low planes, then the high planes
  uint8_t* face_present;        // the same shape
};
int launch_gradient(const GradientArgs& args, int axis, void* stream);

// Clumps (avr_clumps.hip): the connected components of the cells whose value lies in [lower,
// upper].  Every cell has an ordinal, cell_begin of its box + (k ny + j) nx + i, and a 32-bit
// parent entry at that ordinal: kClumpNone for a cell that is not selected, else the ordinal of a
// selected cell of the same clump that is not larger (a root holds its own).  A box as the kernels
// read it:
constexpr uint32_t kClumpNone = 0xffffffffu;
constexpr uint32_t kClumpChunk = 1024;   // consecutive ordinals whose roots one workgroup counts
constexpr uint32_t kClumpRanked = 0x80000000u;  // a root's entry once numbered: this | (label - 1)
constexpr int64_t kClumpTableMaxEntries = int64_t{1} << 28;  // n_clumps * n_levels stays below it
struct alignas(16) ClumpBoxDev {
  const double* in;
  double* out;
  int32_t jstride_in, kstride_in;    // element strides (Array4); every field spans < 2^28
  int32_t jstride_out, kstride_out;
  int32_t nx, ny, nz;     // 0 for a box without cells
  int32_t level;          // 0 .. n_levels - 1
  int32_t lo[3];          // the index of the box's first cell in its level's index space
  int32_t paired;         // input and output: cells 16-byte aligned, both strides even
  uint32_t cell_begin;    // the ordinal of the box's first cell
  int32_t pad_[3];
};
static_assert(sizeof(ClumpBoxDev) == 80, "ClumpBoxDev: 16-byte multiple for scalar loads");
struct ClumpArgs {
  const ClumpBoxDev* boxes;
  const uint32_t* tile_begin;   // n_boxes + 1: prefix sum of the boxes' tiles
  // CSR over (box, axis, side), entry 6 b + 2 axis + side: the boxes of the same or a coarser
  // level whose cells can hold a ghost of that face, in scene order
  const uint32_t* candidate_begin;  // 6 n_boxes + 1
  const int32_t* candidates;
  const LevelRatiosDev* levels;
  int32_t n_boxes, n_levels;
  uint32_t n_tiles;
  uint32_t n_cells;             // < 2^31
  uint32_t n_chunks;            // ceil(n_cells / kClumpChunk)
  double lower, upper;
  uint32_t* parent;             // n_chunks * kClumpChunk entries
  uint32_t* chunk_roots;        // n_chunks: roots per chunk, then their exclusive prefix sum
  unsigned long long* count;    // the number of clumps
};
int launch_clumps(const ClumpArgs& args, void* stream);
// The table of a label field: a JointBoxDev holds the labels as field 0 and the summed field as
// field 1 (the labels again without one).
struct ClumpTableArgs {
  const JointBoxDev* boxes;
  const uint32_t* tile_begin;   // n_boxes + 1: prefix sum of the boxes' tiles
  int32_t n_boxes;
  uint32_t n_tiles;
  uint32_t n_clumps;            // 1 .. 2^28 - 1
  unsigned long long* cells;    // [n_levels][n_clumps], added to
  double* sums;                 // the same shape (null without a field), added to
  unsigned long long* totals;   // [2]: outside, nonfinite, added to
};
int launch_clump_table(const ClumpTableArgs& args, bool has_field, void* stream);
// The links and extents of a label field ("Clump tree"): a JointBoxDev holds the
// labels as field 0 and the parent labels as field 1 (the labels again without a parent scene);
// beside it, per box, where the box lies in the index space of the finest level, n_levels - 1.
struct alignas(16) ClumpLinkBoxDev {
  int32_t lo[3];          // box_index_lo * scale: the finest-level index of the box's first cell
  int32_t scale;          // R_l: finest-level cells per cell of the box's level, per axis
};
static_assert(sizeof(ClumpLinkBoxDev) == 16, "ClumpLinkBoxDev: one 16-byte scalar load");
struct ClumpLinkArgs {
  const JointBoxDev* boxes;
  const ClumpLinkBoxDev* refined;  // n_boxes, beside boxes
  const uint32_t* tile_begin;   // n_boxes + 1: prefix sum of the boxes' tiles
  int32_t n_boxes;
  uint32_t n_tiles;
  uint32_t n_clumps;            // 1 .. 2^28 - 1
  uint32_t n_parents;           // 1 .. 2^28 - 1 with a parent scene, else 0
  int32_t* extent;              // [6][n_clumps]: lows of x, y, z (min), then highs (max)
  uint32_t* parent_lo;          // [n_clumps] (null without a parent scene), min
  uint32_t* parent_hi;          // the same, max
  unsigned long long* totals;   // [2]: labels outside, parent labels outside; added to
};
int launch_clump_links(const ClumpLinkArgs& args, bool has_parent, void* stream);
// The member cells of the wanted clumps of a label field (avr_clump_binding.hip; DESIGN.md 7,
// "Clump binding"): a JointBoxDev holds the labels as every field.  A member's key is
// (label - 1) << 32 | cell ordinal.
struct ClumpMembersArgs {
  const JointBoxDev* boxes;
  const uint32_t* tile_begin;   // n_boxes + 1: prefix sum of the boxes' tiles
  const uint32_t* cell_begin;   // n_boxes + 1: prefix sum of the boxes' cells
  int32_t n_boxes;
  uint32_t n_tiles;
  uint32_t n_clumps;            // 1 .. 2^28 - 1
  const uint8_t* wanted;        // [n_clumps]
  unsigned long long capacity;  // of keys, 1 .. 2^31 - 1
  unsigned long long* keys;     // written at slots below capacity, in no fixed order
  unsigned long long* cursor;   // the next free slot: added to; in the end the number of members
  unsigned long long* totals;   // [1]: labels outside, added to
};
int launch_clump_members(const ClumpMembersArgs& args, void* stream);
// What is looked up per member key: the level, the centre and a field's value of the key's cell.
struct alignas(16) ClumpMemberBoxDev {
  const double* field;    // the field's cells (null without a field)
  int32_t jstride, kstride;
  int32_t nx, ny, nz;     // 0 for a box without cells
  int32_t level;
  int32_t lo[3];          // the index of the box's first cell in its level's index space
  int32_t pad_;
};
static_assert(sizeof(ClumpMemberBoxDev) == 48, "ClumpMemberBoxDev: 16-byte multiple");
struct IsoLevelsDev;
struct ClumpMemberDataArgs {
  const ClumpMemberBoxDev* boxes;
  const uint32_t* cell_begin;   // n_boxes + 1: prefix sum of the boxes' cells
  const IsoLevelsDev* levels;   // cell_size and prob_lo
  int32_t n_boxes;
  uint32_t n_cells;             // < 2^31; a key whose ordinal is not below it names no cell
  uint32_t n_members;           // < 2^31
  const unsigned long long* keys;
  double* values;               // [n_members] (null without a field)
  double* centres;              // [3][n_members] (null: neither centres nor levels are written)
  uint8_t* levels_out;          // [n_members] (null exactly when centres is)
};
int launch_clump_member_data(const ClumpMemberDataArgs& args, void* stream);
// The self-energy of member segments by direct summation (avr_clump_binding.hip; DESIGN.md 7,
// "Clump binding"): a segment's members are cut into tiles of kClumpPairTile, and an item is one
// workgroup's share of the tile pairs (i_tile, j_tile), j_tile >= i_tile: one i tile against
// at most kClumpPairMaxChunk consecutive j tiles.  One segment's items, and so its partials, are
// contiguous.
constexpr uint32_t kClumpPairTile = 256;
constexpr uint32_t kClumpPairMaxChunk = 64;                   // j tiles of one item
constexpr uint64_t kClumpPairMaxSegment = uint64_t{1} << 22;  // members of one segment
// Items of one call: 1 GiB of item table and 0.5 GiB of partials at the limit.  One segment of
// 2^22 members makes 2.1 M items, so a call takes 31 of them.
constexpr uint64_t kClumpPairMaxItems = uint64_t{1} << 26;
struct alignas(16) ClumpPairItem {
  uint32_t begin;     // the segment's first member
  uint32_t count;     // the segment's members, 2 .. 2^22
  uint32_t i_tile;
  uint32_t j_tiles;   // the first j tile | the number of j tiles (1 .. 64) << 16
};
static_assert(sizeof(ClumpPairItem) == 16, "ClumpPairItem: one 16-byte scalar load");
struct ClumpPairArgs {
  const ClumpPairItem* items;       // n_items
  const uint32_t* partial_begin;    // n_segments + 1: prefix sum of the segments' items
  uint32_t n_items;                 // < 2^26
  uint32_t n_segments;              // 1 .. 2^28 - 1
  const double* x;                  // the members' centres and masses, all segments
  const double* y;
  const double* z;
  const double* m;
  double* partial;                  // n_items: written by the pair kernel, read by the reduction
  double* w;                        // n_segments: written
};
int launch_clump_pairs(const ClumpPairArgs& args, void* stream);

// Isosurfaces (avr_isosurface.hip): marching tetrahedra over the cubes of cell centres.  Box b
// enumerates the cube bases (i, j, k) in [-1, n - 1]^3 of its own index space; a base's ordinal is
// base_begin of its box + ((k + 1) (ny + 1) + (j + 1)) (nx + 1) + (i + 1), which is the output
// order.  The cells of the box's one-cell ghost shell are numbered by iso_shell_index, from
// shell_begin of the box on.  A box as the kernels read it:
constexpr uint32_t kIsoChunk = 1024;     // consecutive base ordinals one workgroup counts and emits
constexpr uint64_t kIsoMaxCapacity = uint64_t{1} << 36;  // 12 triangles x 2^31 bases stay below it
constexpr uint8_t kIsoAbsent = 0, kIsoCoarser = 1, kIsoSameLevel = 2;  // a shell cell's code byte
struct alignas(16) IsoBoxDev {
  const double* in;
  const double* sample;   // the sample field's cells, or `in` again without one
  uint64_t shell_begin;   // the number of the box's first shell cell
  int32_t jstride_in, kstride_in;      // element strides (Array4); every field spans < 2^28
  int32_t jstride_sample, kstride_sample;
  int32_t nx, ny, nz;     // 0 for a box without cells
  int32_t level;          // 0 .. n_levels - 1
  int32_t lo[3];          // the index of the box's first cell in its level's index space
  uint32_t base_begin;    // the ordinal of the box's first cube base
  int32_t pad_[2];
};
static_assert(sizeof(IsoBoxDev) == 80, "IsoBoxDev: 16-byte multiple");
struct IsoLevelsDev {
  double cell_size[kFieldMaxLevels][3];
  double prob_lo[3];
  int32_t ratio[kFieldMaxLevels];  // ratio[l]: level l -> l + 1 (1 from n_levels - 1 on)
};
// The number of the shell cell (i, j, k) of a box of n cells, one coordinate at least outside [0,
// n): the two k-planes of (nx + 2) (ny + 2) cells, then per k the two j-rows of nx + 2, then per
// (k, j) the two cells at i = -1 and i = nx.
AVR_HD inline uint64_t iso_shell_index(int nx, int ny, int nz, int i, int j, int k) {
  const uint64_t ex = static_cast<uint64_t>(nx) + 2, ey = static_cast<uint64_t>(ny) + 2;
  const uint64_t a = static_cast<uint64_t>(i + 1), b = static_cast<uint64_t>(j + 1);
  if (k < 0 || k >= nz) return (k < 0 ? 0 : ex * ey) + b * ex + a;
  const uint64_t rows = 2 * ex * ey;
  if (j < 0 || j >= ny) return rows + static_cast<uint64_t>(k) * 2 * ex + (j < 0 ? 0 : ex) + a;
  return rows + static_cast<uint64_t>(nz) * 2 * ex +
         (static_cast<uint64_t>(k) * static_cast<uint64_t>(ny) + static_cast<uint64_t>(j)) * 2 +
         (i < 0 ? 0 : 1);
}
AVR_HD inline uint64_t iso_shell_cells(int nx, int ny, int nz) {
  const uint64_t ex = static_cast<uint64_t>(nx) + 2, ey = static_cast<uint64_t>(ny) + 2;
  return 2 * ex * ey + static_cast<uint64_t>(nz) * 2 * ex +
         static_cast<uint64_t>(nz) * static_cast<uint64_t>(ny) * 2;
}
struct IsoArgs {
  const IsoBoxDev* boxes;
  const uint32_t* base_begin;   // n_boxes + 1: prefix sum of the boxes' cube bases
  const uint64_t* shell_begin;  // n_boxes + 1: prefix sum of the boxes' shell cells
  const uint32_t* candidate_begin;  // n_boxes + 1: CSR over boxes, the boxes of the same or a
  const int32_t* candidates;        // coarser level that can hold a cell of the box's shell
  const IsoLevelsDev* levels;
  int32_t n_boxes, n_levels;
  uint32_t n_bases;             // < 2^31
  uint32_t n_chunks;            // ceil(n_bases / kIsoChunk)
  uint64_t n_shell;
  double value;
  uint64_t capacity;            // triangles the outputs hold
  double* shell_value;          // [n_shell]
  double* shell_sample;         // [n_shell], null without a sample scene
  uint8_t* shell_code;          // [n_shell]
  uint32_t* chunk_triangles;    // [n_chunks]
  uint32_t* chunk_skipped;      // [n_chunks]
  unsigned long long* chunk_offset;  // [n_chunks]: triangles before the chunk
  unsigned long long* counts;   // [2]: T, skipped
  double* vertices;             // [capacity][3][3]
  uint8_t* levels_out;          // [capacity]
  double* samples;              // [capacity][3], null without a sample scene
};
// Counts always; emits when emit is set (the kernel itself leaves the outputs alone if T exceeds
// the capacity).
int launch_isosurface(const IsoArgs& args, bool has_sample, bool emit, void* stream);

// Streamlines (avr_streamlines.hip): RK4 field lines of three congruent scenes through the leaf
// cells, one lane per seed.  A box as the kernel reads it: field 0..2 are the velocity components,
// field 3 the sample field (the first component again without one).
constexpr uint32_t kStreamMaxSteps = 1u << 20;
constexpr int64_t kStreamMaxBlocks = int64_t{1} << 24;   // of the locator
constexpr int64_t kStreamMaxEntries = int64_t{1} << 28;  // of the locator's lists, all blocks
constexpr uint8_t kStreamMaxStepsReached = 0, kStreamOutside = 1, kStreamStagnant = 2,
                  kStreamNonFinite = 3;  // a line's status byte
struct alignas(16) StreamBoxDev {
  const double* cells[4];
  int32_t jstride[4];     // element strides (Array4); every field spans < 2^28 elements
  int32_t kstride[4];
  int32_t nx, ny, nz;     // 0 for a box without cells
  int32_t level;          // 0 .. n_levels - 1
  int32_t lo[3];          // the index of the box's first cell in its level's index space
  int32_t pad_[1];
};
static_assert(sizeof(StreamBoxDev) == 96, "StreamBoxDev: 16-byte multiple");
// The locator: a uniform grid of n[0] x n[1] x n[2] blocks of (1 << shift)^3 level-0 cells from
// the level-0 index `origin` on, which covers every box mapped to level 0 by floor division.  Block
// (bx, by, bz) has the number (bz n[1] + by) n[0] + bx; its list is entries [begin[number],
// begin[number + 1]): the boxes of any level whose cells, mapped to level 0, meet the block, finest
// level first, then in scene order.  n[0] == 0: the scene has no cells.
struct StreamLocatorDev {
  int32_t origin[3];
  int32_t n[3];
  int32_t shift;
  int32_t pad_;
};
struct StreamArgs {
  const StreamBoxDev* boxes;
  const uint32_t* block_begin;  // blocks + 1
  const int32_t* block_boxes;
  const IsoLevelsDev* levels;   // cell sizes, prob_lo and ratios as the isosurfaces stage them
  StreamLocatorDev locator;
  int32_t n_levels;
  uint32_t n_seeds;
  uint32_t max_steps;           // <= kStreamMaxSteps; n_seeds * (max_steps + 1) < 2^32
  double step, direction;       // direction: +1.0 or -1.0
  const double* seeds;          // [n_seeds][3]
  double* points;               // [n_seeds][max_steps + 1][3]
  double* samples;              // [n_seeds][max_steps + 1], null without a sample scene
  uint32_t* counts;             // [n_seeds]
  uint8_t* status;              // [n_seeds]
};
int launch_streamlines(const StreamArgs& args, bool has_sample, void* stream);

// Covering grids (avr_covering_grid.hip): a field resampled to the cells of one level L over a
// region of nx x ny x nz cells from the level-L index `lo` on, one lane per output cell.  The
// output is cut into the tiles of avr_cell_tiles.h (128 cells along x by 4 rows by 4 planes,
// numbered as cell_tile_of numbers a box's); tile t has the candidate list [candidate_begin[t],
// candidate_begin[t + 1]): every box, in scene order, whose cells hold a cell of the tile, an
// ancestor or a descendant of one.  A box as the kernel reads it:
struct alignas(16) CoverBoxDev {
  const double* cells;
  int32_t jstride, kstride;  // element strides (Array4); the field spans < 2^28 elements
  int32_t nx, ny, nz;     // 0 for a box without cells
  int32_t level;          // 0 .. n_levels - 1
  int32_t lo[3];          // the index of the box's first cell in its level's index space
  int32_t pad_[1];
};
static_assert(sizeof(CoverBoxDev) == 48, "CoverBoxDev: 16-byte multiple");
struct CoverLevelsDev {
  double weight[kFieldMaxLevels];   // [m], L < m <= finest: w_m = 1 / f64(R_m^3); 0.0 elsewhere
  int32_t refine[kFieldMaxLevels];  // [m], L < m <= finest: R_m = ratio[L] ... ratio[m - 1]; else 1
  int32_t ratio[kFieldMaxLevels];   // ratio[l]: level l -> l + 1 (1 from n_levels - 1 on)
};
struct CoverArgs {
  const CoverBoxDev* boxes;
  const uint32_t* candidate_begin;  // n_tiles + 1
  const int32_t* candidates;
  const CoverLevelsDev* levels;
  int32_t level;          // L
  int32_t finest;         // the finest level that has a box with cells (-1: none has)
  int32_t lo[3];
  int32_t nx, ny, nz;     // nx * ny * nz < 2^31
  uint32_t n_tiles;
  double fill;
  double* values;         // [nz][ny][nx]
  double* coverage;       // the same shape, or null
  int8_t* cell_level;     // the same shape, or null
};
int launch_covering_grid(const CoverArgs& args, void* stream);

// Grid fields (avr_grid_field.hip): a uniform grid of level L over the region of nx x ny x nz
// cells from the level-L index `lo` on, written onto every cell of a scene's boxes -- the inverse
// of the covering grid.  The output is streamed in the tiles of avr_cell_tiles.h, as derive_kernel
// streams it.  A box as the kernel reads it:
struct alignas(16) GridBoxDev {
  double* out;
  int32_t jstride, kstride;  // element strides (Array4); the box spans < 2^28 elements
  int32_t nx, ny, nz;     // 0 for a box without cells
  int32_t level;          // 0 .. n_levels - 1
  int32_t lo[3];          // the index of the box's first cell in its level's index space
  int32_t paired;         // cells 16-byte aligned, both strides even: f64 pairs store
};
static_assert(sizeof(GridBoxDev) == 48, "GridBoxDev: 16-byte multiple for scalar loads");
constexpr int32_t kGridSame = 0, kGridFiner = 1, kGridCoarser = -1;
struct GridLevelsDev {
  // [l]: R = the product of the ratios between level l and L (1 for l == L), held at 2^32
  int64_t refine[kFieldMaxLevels];
  double two_r[kFieldMaxLevels];      // [l]: f64(2 R)
  int32_t direction[kFieldMaxLevels];  // [l]: kGridSame, kGridFiner (l > L) or kGridCoarser (l < L)
};
struct GridFieldArgs {
  const GridBoxDev* boxes;
  const uint32_t* tile_begin;   // n_boxes + 1: prefix sum of the boxes' tiles
  const GridLevelsDev* levels;
  const double* grid;           // [nz][ny][nx]
  unsigned long long* totals;   // [2]: outside, partial; added into
  int32_t n_boxes;
  uint32_t n_tiles;
  int32_t level;                // L
  int32_t lo[3];
  int32_t nx, ny, nz;           // nx * ny * nz < 2^31
  int32_t interpolation;        // 0 constant, 1 linear
  int32_t periodic;             // 0 clamped, 1 wrapped
  double fill;
};
int launch_grid_field(const GridFieldArgs& args, void* stream);

// Particle fields (avr_particles.hip; DESIGN.md 7, "Particle fields"): particles deposited onto the
// cells of a scene's boxes.  particle_cells_kernel finds every particle's leaf through the
// streamlines' locator and writes its contributions (cell ordinal, share), one (nearest grid point)
// or eight (cloud in cell) per particle; the caller sorts them by cell, stably;
// particle_clear_kernel writes +0.0 to every cell and particle_sum_kernel adds each cell's run of
// shares in list order.  A box as the first kernel reads it:
constexpr long long kParticleOutside = 0xFFFFFFFFll;  // the cell of an outside particle's entries
constexpr int kParticleNgp = 0, kParticleCic = 1;     // the methods
constexpr int kParticleSum = 0, kParticleDensity = 1;  // the quantities
struct alignas(16) ParticleBoxDev {
  int32_t nx, ny, nz;     // 0 for a box without cells
  int32_t level;          // 0 .. n_levels - 1
  int32_t lo[3];          // the index of the box's first cell in its level's index space
  int32_t pad_;
};
static_assert(sizeof(ParticleBoxDev) == 32, "ParticleBoxDev: 16-byte multiple");
struct ParticleCellsArgs {
  const ParticleBoxDev* boxes;
  const uint32_t* cell_begin;   // n_boxes + 1: prefix sum of the boxes' cells, in scene order
  const uint32_t* block_begin;  // blocks + 1
  const int32_t* block_boxes;
  const IsoLevelsDev* levels;   // cell sizes, prob_lo and ratios as the isosurfaces stage them
  StreamLocatorDev locator;
  int32_t n_levels;
  uint32_t n;                   // particles: < 2^31 (ngp), < 2^28 (cic)
  int32_t paired;               // cells and shares 16-byte aligned: a lane's entries store as pairs
  const double* points;         // [n][3]
  const double* values;         // [n], or null: every value is 1.0
  long long* cells;             // [n][C], C = 1 or 8
  double* shares;               // [n][C]
  uint8_t* levels_out;          // [n], or null
  unsigned long long* totals;   // [2]: outside particles, rerouted corner shares; added into
};
int launch_particle_cells(const ParticleCellsArgs& args, int method, void* stream);
struct ParticleLevelsDev {
  double volume[kFieldMaxLevels];  // [l]: (dx_l * dy_l) * dz_l (1.0 from n_levels on)
};
// The output's boxes are GridBoxDev (lo unused).
struct ParticleDepositArgs {
  const GridBoxDev* boxes;
  const uint32_t* tile_begin;   // n_boxes + 1: prefix sum of the boxes' tiles
  const uint32_t* cell_begin;   // n_boxes + 1: prefix sum of the boxes' cells
  const ParticleLevelsDev* levels;
  int32_t n_boxes;
  uint32_t n_tiles;
  uint32_t n_cells;             // < 2^31; an ordinal that is not below it names no cell
  uint32_t n;                   // contributions, < 2^31
  const long long* cells;       // [n], ascending
  const double* shares;         // [n]
};
// The clear, then (with n > 0) the sum.
int launch_particle_deposit(const ParticleDepositArgs& args, int quantity, void* stream);

// Particle groups (avr_particle_groups.hip; DESIGN.md 7, "Particle groups"): friends-of-friends
// groups of particles.  group_cells_kernel gives every particle a cell of a uniform grid over the
// box and a parent entry; the caller sorts the particles by cell, stably; group_link_kernel tests
// every pair of particles in the same or adjacent cells and unites the linked ones in the clumps'
// lock-free union-find; flatten, count, scan, rank and label turn the roots into labels 1..N.  The
// grid as both kernels read it (the plan fills it):
constexpr uint32_t kGroupOutside = 0xffffffffu;  // the cell and the parent entry of an outside particle
constexpr uint32_t kGroupChunk = 256;            // particles whose qualifying roots one workgroup counts
constexpr int kGroupMaxDim = 1024;               // cells along an axis, at most
struct GroupGridDev {
  double lo[3], hi[3];
  double h[3];        // (hi - lo) / dims
  double length[3];   // hi - lo
  double top[3];      // f64(dims - 1): the clamp of a cell index
  int32_t dims[3];    // 1 .. 1024, product < 2^27
  int32_t periodic[3];
};
struct ParticleGroupCellsArgs {
  GroupGridDev grid;
  uint32_t n;                  // particles, < 2^31
  const double* points;        // [n][3]
  uint32_t* cells;             // [n]
  uint32_t* parent;            // [n]
  unsigned long long* totals;  // [1]: outside particles; added into
};
int launch_particle_group_cells(const ParticleGroupCellsArgs& args, void* stream);
struct ParticleGroupsArgs {
  GroupGridDev grid;
  double b2;                     // b * b
  uint32_t n, n_inside;          // n_inside <= n < 2^31
  uint32_t n_chunks;             // ceil(n / kGroupChunk)
  uint32_t n_cells;              // the product of dims
  uint32_t min_members;          // 1 .. 2^31 - 1
  const double* points;          // [n][3], in sorted order
  const long long* order;        // [n]: the particle in sorted slot i
  const long long* cell_begin;   // [n_cells + 1]: the first sorted slot of each cell
  uint32_t* parent;              // [n]: group_cells_kernel's on entry, roots on return
  int32_t* labels;               // [n]
  uint32_t* sizes;               // [n]: the members at a root's entry, 0 elsewhere
  uint32_t* chunk_counts;        // [n_chunks]: scratch
  unsigned long long* n_groups;  // [1]
};
// The sizes' clear, the link (with n_inside > 0), then flatten, count, scan, rank, label.
int launch_particle_groups(const ParticleGroupsArgs& args, void* stream);

// Ray transfer (avr_rays.hip; DESIGN.md 7, "Ray transfer"): emission and absorption along the same
// walk, front to back.  The walk's field is the source function S; the opacity a, the bin field g
// and the width s are read at the same cell through their own box tables.  Grey (no g) keeps its
// sums in registers; with channels a one-wave workgroup holds the intensity and the optical depth
// of one chunk of channels in LDS, [channel][2][lane], behind the chunk's edges and reciprocals.
constexpr int kTransferGrey = 0, kTransferSharp = 1, kTransferBroadened = 2;  // the forms
constexpr int kTransferMaxChannels = 1024;
constexpr int kTransferChunk = 16;     // channels of a chunk unless the context was told otherwise
                                       // (measured: DESIGN.md 7, "Ray transfer")
constexpr int kTransferMaxChunk = 32;  // 2 x 32 x 64 doubles of LDS, and the tables
struct RayTransferPart {
  const CoverBoxDev* opacity_boxes;  // box by box the source's
  const CoverBoxDev* bin_boxes;      // ... or null (grey)
  const CoverBoxDev* width_boxes;    // ... or null (grey, sharp)
  const double* edges;               // [n_channels + 1]; null for grey
  const double* rdv;                 // [n_channels]: 1 / (edges[c + 1] - edges[c]); null for grey
  int32_t n_channels;                // 1 for grey
  int32_t chunk;                     // channels per chunk (the grid's y index numbers the chunks)
  double lo, hi;                     // edges[0], edges[n_channels]
  double* intensity;                 // [n_channels][n_rays]
  double* tau;                       // [n_channels][n_rays]
  double* outside;                   // [2][n_rays]: under, over; null for grey
};
// Rays (avr_rays.hip): the leaf cells a segment A -> B crosses, in order, one lane per ray.  A box
// as the kernel reads it is a CoverBoxDev; the locator is the streamlines'.
constexpr uint64_t kRayMaxTrips = uint64_t{1} << 30;
constexpr uint64_t kRayMaxSegments = uint64_t{1} << 40;  // the packed arrays' capacity
constexpr uint8_t kRayComplete = 0, kRayMiss = 1, kRayTruncated = 2, kRayInvalid = 3;
struct RayArgs {
  const CoverBoxDev* boxes;
  const uint32_t* block_begin;  // blocks + 1
  const int32_t* block_boxes;
  const IsoLevelsDev* levels;   // cell sizes, prob_lo and ratios as the isosurfaces stage them
  StreamLocatorDev locator;
  int32_t bound_lo[3];          // [Blo, Bhi]: the boxes mapped to level 0 (the locator's box);
  int32_t bound_hi[3];          // refined to level n_levels - 1 it lies inside [-2^30, 2^30]
  int32_t n_levels;
  uint32_t n_rays;
  uint32_t max_trips;           // 1 .. 2^30
  const double* start;          // [n_rays][3]
  const double* end;            // [n_rays][3]
  // the count pass
  uint32_t* counts;             // [n_rays]
  uint8_t* status;              // [n_rays]
  double* span;                 // [n_rays][2]: t_enter, t_leave
  // the emit pass: ray s owns the slots [offsets[s], offsets[s + 1]) below n_segments
  const long long* offsets;     // [n_rays + 1]
  uint64_t n_segments;
  double* t0;                   // [n_segments]
  double* t1;                   // [n_segments]
  int8_t* level;                // [n_segments]
  double* value;                // [n_segments]
  double* integral;             // [n_rays]
  double* covered;              // [n_rays]
  // the sums pass: the count pass's three arrays, integral and covered, and
  const CoverBoxDev* weight_boxes;  // the weight field's boxes, box by box the field's; or null
  double* weight;               // [n_rays]; written with weight_boxes only
  double* counted;              // [n_rays]
  // a transfer: the count pass's three arrays, counted and covered, and (behind everything the
  // other modes read, whose offsets stay)
  RayTransferPart transfer;
};
int launch_rays(const RayArgs& args, bool emit, void* stream);
int launch_ray_sums(const RayArgs& args, void* stream);

// The dynamic LDS of a one-wave workgroup: the chunk's edges and reciprocals, then the intensity
// and the optical depth as [channel][2][lane].
inline size_t ray_transfer_lds_bytes(int form, int chunk) {
  if (form == kTransferGrey) return 0;
  return (static_cast<size_t>(2 * chunk + 1) + static_cast<size_t>(chunk) * 2 * 64) * sizeof(double);
}
int launch_ray_transfer(const RayArgs& args, int form, uint32_t n_chunks, size_t lds_bytes,
                        void* stream);

// Power spectra (avr_fft.hip, avr_spectral.hip; DESIGN.md 7, "Power spectrum"): the forward,
// unnormalised 3-D transform of a real f64 grid [nz][ny][nx] into an interleaved complex spectrum
// [nz][ny][nx][2], one radix-2 pass per axis with whole lines in LDS, and the shell sums of a
// spectrum, a streaming kernel (launched with the `groups` of its plan, as every one is).
constexpr int kFftMaxLength = 1024;       // per axis; a power of two
constexpr int kFftGroupElements = 2048;   // complex elements a workgroup stages (32 KiB) ...
constexpr int kFftMinColumns = 4;         // ... but never fewer adjacent columns than this (64-byte
                                          // runs): 4 lines of 1024 are 64 KiB, the most ever staged
constexpr int kSpectrumMaxBins = 2048;    // 20 bytes of LDS per bin
constexpr uint32_t kSpectralGroupElements = 16384;  // cells or modes a workgroup of 256 lanes takes
// One strided pass (y or z): `planes` planes of `columns` adjacent lines each; element e of the
// line in column c of plane q is the complex at q * plane_stride + e * line_stride + c.  A
// workgroup stages `group` adjacent columns, the last of a plane's `groups` only `last`.
struct FftPassDev {
  int32_t n, log2n;          // the line's length 2^log2n; n == 1: the pass is not launched
  uint32_t planes, columns;
  uint32_t group, groups, last;
  uint32_t pad_;
  uint64_t plane_stride, line_stride;  // in complex elements
};
// The lines and passes of a 3-D transform, forward or inverse: the same cut for both.
struct FftLinesDev {
  const double* twiddle[3];  // per axis (x, y, z), n / 2 pairs: forward W[m] = (cos, sin)(-(2 pi m)
                             // / n), inverse V[m] = (W[m].re, -W[m].im)
  int32_t nx, log2nx;
  uint32_t x_lines;          // ny * nz
  uint32_t x_group;          // lines a workgroup of the x pass stages
  FftPassDev pass[2];        // y, z; the inverse launches z first
};
struct FftArgs {
  const double* values;      // [nz][ny][nx]
  double* spectrum;          // [nz][ny][nx][2]
  FftLinesDev lines;
};
int launch_fft3d(const FftArgs& args, void* stream);
struct SpectrumBinsArgs {
  const double* spectrum;    // [nz][ny][nx][2]
  const double* edges_sq;    // n_bins + 1
  int32_t log2n[3];          // x, y, z
  int32_t n_bins;
  uint32_t n_modes;          // nx * ny * nz < 2^31
  uint32_t pad_;
  double g[3];               // 1 / L_d^2
  unsigned long long* modes; // [n_bins], added to
  double* power;             // [n_bins], added to
  unsigned long long* totals;  // (outside, nonfinite), added to
};
int launch_spectrum_bins(const SpectrumBinsArgs& args, uint32_t groups, void* stream);

// Inverse transform, Helmholtz split, potential (avr_fft.hip, avr_spectral.hip; DESIGN.md 7,
// "Inverse transform, Helmholtz split, potential"): the normalised inverse of a complex spectrum
// into real grids -- the strided passes along z, then y, in place (fft_column_kernel with the
// conjugate tables), then the x pass, which scales and splits -- and two per-mode operators.
struct IfftArgs {
  double* spectrum;          // [nz][ny][nx][2]; the strided passes overwrite it
  double* values;            // [nz][ny][nx]: re / (nx ny nz)
  double* imag;              // [nz][ny][nx]: im / (nx ny nz); or null
  double scale;              // 1.0 / f64(nx ny nz), a power of two
  FftLinesDev lines;         // with the inverse tables
};
int launch_ifft3d(const IfftArgs& args, void* stream);
struct HelmholtzArgs {
  double* spectra[3];        // (vx, vy, vz) [nz][ny][nx][2]: read, then the solenoidal part
  double* compressive[3];    // written
  int32_t log2n[3];          // x, y, z
  uint32_t n_modes;          // nx * ny * nz < 2^31
  double h[3];               // 1 / L_d
};
int launch_spectrum_helmholtz(const HelmholtzArgs& args, uint32_t groups, void* stream);
struct InverseLaplacianArgs {
  double* spectrum;          // [nz][ny][nx][2], in place
  int32_t log2n[3];
  uint32_t n_modes;
  double g[3];               // 1 / L_d^2
  double scale;
};
int launch_spectrum_inverse_laplacian(const InverseLaplacianArgs& args, uint32_t groups,
                                      void* stream);

// Isolated potential (avr_spectral.hip; DESIGN.md 7, "Isolated potential"): the open-boundary
// Green's function on a zero-padded grid and the product of two spectra, both streaming.
struct IsolatedGreenArgs {
  double* green;             // [Pz][Py][Px], written
  int32_t log2n[3];          // x, y, z of the padded grid
  uint32_t n_cells;          // Px * Py * Pz < 2^31
  double size[3];            // the cell's (dx, dy, dz)
  double scale;              // G = scale / sqrt(r2) ...
  double self_value;         // ... but this at r2 == 0
};
int launch_isolated_green(const IsolatedGreenArgs& args, uint32_t groups, void* stream);
struct SpectrumMultiplyArgs {
  double* a;                 // [nz][ny][nx][2]: read, then a b
  const double* b;           // [nz][ny][nx][2]
  uint32_t n_modes;          // nx * ny * nz < 2^31
  uint32_t pad_;
};
int launch_spectrum_multiply(const SpectrumMultiplyArgs& args, uint32_t groups, void* stream);

// Structure functions (avr_structure.hip; DESIGN.md 7, "Structure functions"): the moments of the
// increments of one or three real f64 grids [nz][ny][nx] over a table of integer lag vectors, one
// workgroup per (lag, share of cells), the lag the fast-running block index.
constexpr int kStructureMaxLags = 4096;
constexpr int kStructureMaxOrder = 8;
constexpr uint32_t kStructureGroupCells = 16384;  // the cells a workgroup of 256 lanes takes for one lag
constexpr uint32_t kStructureLaneStride = 256;    // the distance between a lane's consecutive cells
constexpr uint32_t kStructureShareRows = 32768;   // shares per grid row: share = y + this * z, so that
                                                  // no grid dimension passes 65535 below 2^31 cells
// One lag: the partner of the cell (i, j, k) is (i + l[0], j + l[1], k + l[2]); u is the direction
// the longitudinal increment is taken along (three components; zeros with one).
struct StructureLagDev {
  int32_t l[3];
  int32_t pad_;
  double u[3];
};
struct StructureArgs {
  const double* components[3];  // [nz][ny][nx] each; [1] and [2] null with one component
  const StructureLagDev* lags;  // [n_lags]
  int32_t dims[3];              // nx, ny, nz
  int32_t n_lags;
  int32_t max_order;            // P
  int32_t periodic;
  uint32_t n_cells;             // nx * ny * nz < 2^31
  uint32_t shares;              // ceil(n_cells / kStructureGroupCells)
  uint32_t stride[3];           // kStructureLaneStride = stride[0] + nx (stride[1] + ny stride[2]),
                                // stride[0] < nx, stride[1] < ny: how a lane's (i, j, k) advance
  uint32_t pad_;
  unsigned long long* pairs;    // [n_lags], added to
  double* sums;                 // [n_lags][K][P], K = 1 or 3, added to
  unsigned long long* totals;   // (outside, nonfinite), added to
};
int launch_structure_functions(const StructureArgs& args, int n_components,
                               const uint32_t groups[3], void* stream);

// Velocity cubes (avr_velocity_cube.hip; DESIGN.md 7, "Velocity cubes"): the on-axis projection of
// an emission field e split into channels of a bin field g, optionally broadened by a width field
// s.  The tiles, the segments of kAxisSegment cells, the entries of a partial plane and the gather's
// box records (AxisPlaneDev) are the on-axis projection's.  Stage 1 writes, per batch of channels,
// the partial planes [channel in batch][entries] and, with `totals`, under [entries], over
// [entries] (f64) and n [entries] (u32); a workgroup keeps its columns' accumulators of one chunk
// of channels in LDS, laid out [channel][column], and the grid's y index numbers the chunks of
// the batch.  Stage 2 gathers them per pixel.
constexpr int kCubeMaxChannels = 1024;
constexpr uint64_t kCubeScratchEntries = uint64_t{1} << 27;  // f64 entries of the channel planes
constexpr int kCubeColumns[3] = {64, 512, 512};   // columns of one tile, per axis
constexpr int kCubeChunk[3] = {32, 8, 8};         // channels a workgroup keeps in LDS, per axis
struct alignas(16) CubeBoxDev {
  const double* cells[3];   // e, g, s (s == g without a width field: not read)
  int32_t jstride[3];       // element strides (Array4); every field spans < 2^28 elements
  int32_t kstride[3];
  int32_t nx, ny, nz;
  int32_t paired;           // every field: cells 16-byte aligned, both strides even
  uint32_t plane_begin;     // first entry of the box's partial planes
  int32_t pad_[3];
};
static_assert(sizeof(CubeBoxDev) == 80, "CubeBoxDev: 16-byte multiple for scalar loads");
struct CubeReduceArgs {
  const CubeBoxDev* boxes;
  const uint32_t* tile_begin;   // n_boxes + 1: prefix sum of the boxes' tiles
  int32_t n_boxes;
  uint32_t n_tiles;
  const double* edges;          // n_channels + 1, device
  int32_t n_channels;
  int32_t channel_first;        // the batch: channels [channel_first, channel_first + channel_count)
  int32_t channel_count;
  int32_t chunk;                // channels per workgroup: min(kCubeChunk[axis], the largest batch)
  int32_t totals;               // != 0: the workgroups of the batch's first chunk write under, over, n
  uint32_t entries;             // of one partial plane, all boxes
  double lo, hi, scale;         // e[0], e[n] and n / (e[n] - e[0]) (0 if that is not finite)
  double* planes;               // [channel_count][entries]
  double* under;                // [entries]
  double* over;                 // [entries]
  uint32_t* plane_n;            // [entries]
};
struct CubeGatherArgs {
  const AxisPlaneDev* boxes;
  int32_t n_boxes;
  int32_t width, height;
  int32_t channel_first, channel_count;
  int32_t totals;               // != 0: under, over and length are written too
  uint32_t entries;
  double origin_u, origin_v, du, dv;
  const double* planes;
  const double* plane_under;
  const double* plane_over;
  const uint32_t* plane_n;
  double* cube;                 // [n_channels][height][width]
  double* under;                // [height][width]
  double* over;
  double* length;
};
// dynamic LDS of a stage 1 workgroup: the edges, chunk + 2 accumulators per column and, for axis x,
// the staged slab of the three fields
size_t velocity_cube_lds_bytes(int axis, int n_channels, int chunk);
int launch_cube_reduce(const CubeReduceArgs& args, int axis, bool broadened, void* stream);
int launch_cube_gather(const CubeGatherArgs& args, void* stream);

// Wireframe overlay (avr_overlay.hip): the 12 edges of the bounds box projected by the host.
struct OverlayEdge {
  float sx, sy, ex, ey;   // projected end points (pixels)
  float dx, dy, len_sq;   // end - start, squared length
  int32_t x_begin, x_end, y_begin, y_end;  // pixel rectangle the reference loops over
  int32_t point;          // degenerate edge: a single full-coverage sample
};
struct OverlayPlan {
  OverlayEdge edges[12];
  int32_t n_edges;
  float pixel_radius;
};
// renderBoundingBoxLayer's host part (VolumeRenderer.cpp:139-232, 265-288).
void plan_overlay(const double bounds_min[3], const double bounds_max[3], const avr_camera& camera,
                  int sqrt_antialiasing, int width, int height, OverlayPlan* plan);
// computeTightBounds (VolumeRenderer.cpp:791-848) over replicated box metadata.
void tight_bounds(const avr_box* boxes, int n_boxes, const double fallback_min[3],
                  const double fallback_max[3], double out_min[3], double out_max[3]);
// image / rgb8 hold the pixels [pixel_begin, pixel_end) of the image, or -- pieces != nullptr with
// row bands -- the rows of piece `piece` in order (pixel_begin = 0, pixel_end = its pixel count).
int launch_overlay(const OverlayPlan& plan, int width, int64_t pixel_begin, int64_t pixel_end,
                   const PieceMapDev* pieces, int piece, float* image, uint8_t* rgb8, void* stream);

// ---- visibility ordering (avr_visibility.cpp) -----------------------------------------------
struct VisBox {
  float lo[3], hi[3];
  int owner;
  float min_depth, max_depth;
};
struct VisPair {
  int i, j, axis;
  int b_below_a;  // 0: a.max == b.min on `axis` (a below b); 1: b.max == a.min
};
void visibility_pairs(const std::vector<VisBox>& boxes, std::vector<VisPair>* pairs);
}  // namespace avr
struct avr_visibility_graph;
namespace avr {
avr_visibility_graph* visibility_graph_create(const avr_box* all_boxes, const int32_t* owner,
                                              int n_boxes, int n_ranks);
void visibility_graph_destroy(avr_visibility_graph* graph);
int visibility_rank_count(const avr_visibility_graph* graph);
// Fills rank_order[n_ranks]; returns false (and the default order) when the graph ordering fails.
bool visibility_order(avr_visibility_graph* graph, const avr_camera& camera, float aspect,
                      const char* dot_prefix, int32_t* rank_order, int* n_splits);

void set_error(const std::string& message);
// Deadline (ms) of every host wait on device work, AVR_FRAME_TIMEOUT_MS (default 30000; 0: none):
// a frame of several ranks contains collectives, and a peer that died or whose calls differ must
// end in an error on this rank, not in a hang (DirectSendBase.cpp:206-220, 277 completes or errors).
int frame_timeout_ms();
void set_frame_timeout_ms(int ms);  // < 0: back to the environment's value
// While one is alive on a thread, that thread's waits take the DEFAULT deadline (30 s) when nobody
// set one: the calls of a renderer of several ranks and of a communicator.  A deadline that was
// asked for (avr_set_frame_timeout_ms / AVR_FRAME_TIMEOUT_MS) holds everywhere; without either, a
// single-rank context waits forever, as a plain HIP synchronise would.
class CollectiveScope {
 public:
  explicit CollectiveScope(bool collective);
  ~CollectiveScope();
  CollectiveScope(const CollectiveScope&) = delete;
  CollectiveScope& operator=(const CollectiveScope&) = delete;

 private:
  bool on_;
};
struct DeadlineExceeded : std::runtime_error {
  using std::runtime_error::runtime_error;
};
// Polling host waits (hipEvent_t / hipStream_t) that throw DeadlineExceeded naming `what`.
void wait_event_deadline(void* hip_event, const char* what);
void wait_stream_deadline(void* hip_stream, const char* what);
// The context's HIP stream (hipStream_t; created on first use) with its device made current.
void* context_stream(avr_context* ctx);
// The context's owner bounds the frames in flight itself: a descriptor batch that repeats then
// leaves no packet at all on the stream (by default its event is still recorded, which is what
// keeps the host a few batches ahead of the GPU at most).
void context_set_lean_descriptors(avr_context* ctx, bool lean);
// One rank's fold normally takes one workgroup per CU (it runs beside the next frame's paint
// kernels); `whole`: the next fold of this context takes the whole grid (nothing else is running).
void context_set_fold_whole_grid(avr_context* ctx, bool whole);
// How many descriptor batches the host may stage ahead of the context's stream (1 .. 9; default 4).
void context_set_descriptor_lead(avr_context* ctx, int batches);
// Whether the context's classify passes stream their bricklets to memory (RenderLaunch).
void context_set_classify_stream_stores(avr_context* ctx, bool stream);

// The sizing pass of the stager (stage_tables, avr_context.h) over a plan's visit_tables: what
// StagingRing::begin is given.  An empty table counts as the one element it is staged as.
struct StagingSize {
  size_t bytes = 0;
  int items = 0;
  template <class T>
  void operator()(const T** /*device*/, const T* /*host*/, size_t count) {
    bytes += (count != 0 ? count : 1) * sizeof(T);
    ++items;
  }
};

// Flags of the events that only ORDER work between this library's streams on ONE device (a
// frame's classified volume -> its march -> its fold; the descriptor ring's slots): recorded
// without the system-scope fence.  Whoever waits on them is another queue of the same GPU (the
// kernel's own end-of-kernel release makes its writes visible there) or the host asking only
// WHETHER the work is through (buffer re-use), never reading what it wrote -- results reach the
// host through a stream / renderer synchronise, which fences.  Measured (tools/microbench/
// packet_gap.hip): a record costs 3.0 us of stream time with the fence and 1.2 us without; with
// two to three records between a frame's kernels and the next frame's: config-2 0.381 -> 0.376 ms,
// config-4 0.992 -> 0.978 ms at fixed reserves.  (hipEventDisableTiming | hipEventDisableSystemFence)
inline unsigned ordering_event_flags() { return 0x2u | 0x20000000u; }

}  // namespace avr

#endif
