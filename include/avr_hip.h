/*
 * avr_hip.h -- C ABI of the MI355X (gfx950) volume-rendering hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types, no exceptions.
 * Every entry point cites the reference interface (file:line under the amrVolumeRenderer tree)
 * it replaces.  All image/cell pointers are DEVICE pointers (HBM) unless a parameter says
 * "host".  Every function returns 0 on success or a negative avr_status; the message of the
 * last failure on the calling thread is available from avr_last_error().
 *
 * There is no CPU fallback behind this ABI: without a HIP device every compute entry point
 * fails with AVR_ERR_NO_DEVICE.
 *
 * Pixel layouts (same as the reference's image buffers):
 *   depth-sort image : 5 floats / pixel  (premultiplied r, g, b, a, depth)   -- ImageRGBAFloatColorDepthSort
 *   float image      : 4 floats / pixel  (premultiplied r, g, b, a)          -- ImageRGBAFloatColorOnly
 *   ubyte image      : 1 uint32 / pixel  (bytes r, g, b, a in memory order)  -- ImageRGBAUByteColorOnly
 * Pixel index p = y * width + x, image origin bottom-left (Common/VolumePainter.cpp:738-739).
 */
#ifndef AVR_HIP_H
#define AVR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  AVR_OK = 0,
  AVR_ERR_INVALID_ARGUMENT = -1, /* std::invalid_argument in the reference API */
  AVR_ERR_RUNTIME = -2,          /* std::runtime_error (HIP failure, bad image type, ...) */
  AVR_ERR_NO_DEVICE = -3,
  AVR_ERR_OUT_OF_MEMORY = -4
} avr_status;

typedef struct avr_context avr_context;
typedef struct avr_scene avr_scene;

/* volume::AmrBox (Common/VolumeTypes.hpp:69-76).  `cells` = address of
 * values(validBox.smallEnd(), component): x fastest, then jstride, kstride (amrex::Array4). */
typedef struct {
  double min_corner[3];
  double max_corner[3];
  int32_t dims[3];
  int32_t level;        /* informational (AMR level); not read by the kernels */
  const double *cells;  /* device pointer */
  int64_t jstride;
  int64_t kstride;
} avr_box;

/* volume::ScalarTransform (Common/VolumeTypes.hpp:21-31): the fields the path reads. */
typedef struct {
  int32_t log_scale_input;
  int32_t normalize_to_unit_range;
  double positive_floor;
  double normalization_min;
  double inverse_normalization_span;
} avr_scalar_transform;

/* volume::CameraParameters (Common/VolumeTypes.hpp:83-90). */
typedef struct {
  double eye[3];
  double look_at[3];
  double up[3];
  float fov_y_degrees;
  float near_plane;
  float far_plane;
} avr_camera;

/* volume::ColorMapControlPoint (Common/VolumeTypes.hpp:92-98). */
typedef struct {
  float value, red, green, blue, alpha;
} avr_colormap_point;

/* The scalar arguments of VolumePainter::paint (Common/VolumePainter.hpp:19-31):
 * image size, scalarRange, boxTransparency, referenceSampleDistance, bounds, colorMap.
 * (rank, numProcs, antialiasing are unused by the reference: VolumePainter.cpp:561-562.) */
typedef struct {
  int32_t width;
  int32_t height;
  float scalar_range[2];
  float box_transparency;
  float reference_sample_distance;
  double bounds_min[3];
  double bounds_max[3];
  const avr_colormap_point *colormap; /* host pointer; NULL/0 = default jet map */
  int32_t colormap_count;
} avr_paint_params;

/* ---- library / context ------------------------------------------------------------------ */

/* Message of the last failure on this thread ("" if none). */
const char *avr_last_error(void);

/* ABI version of this header (bumped on incompatible change).
 *   2 (round 5): for ranks of several the RGB8 bytes of a frame reach rank 0's rgb8_out one frame
 *     late by default (avr_renderer_set_deferred_gather, avr_renderer_outputs_complete) and
 *     avr_renderer_synchronize is collective while such a gather is pending; the test hooks and
 *     diagnostics moved to avr_hip_debug.h; avr_context_set_cu_mask_pattern is gone.
 *     (Added since, compatibly: avr_classify_plan_flagged / _positions, avr_march_plan_speculative,
 *     avr_renderer_set_visibility_speculation, avr_renderer_speculation_state.)
 *   1: rounds 1-4. */
#define AVR_ABI_VERSION 2
int avr_abi_version(void);

/* Deadline, in milliseconds, of every host wait on device work inside this library (0 = wait
 * forever; < 0 = back to the default).  Default: the environment's AVR_FRAME_TIMEOUT_MS; without
 * it 30000 for the calls that involve other ranks (a renderer of several ranks or with a
 * communicator, the avr_comm_* / avr_exchange* / avr_gather* calls) and NONE for single-rank
 * contexts and renderers, which wait as long as a plain HIP synchronise would.
 * The frame of a rank of several contains collectives; the reference's exchange either completes
 * or errors (MPI_Waitany / MPI_Waitall, DirectSend/Base/DirectSendBase.cpp:206-220, 277).  Here a
 * wait that outlasts the deadline -- a peer that died, ranks whose calls differ -- makes the call
 * return AVR_ERR_RUNTIME with avr_last_error() naming what did not finish (stream, frame); the
 * renderer is then failed for good (every later call returns the error at once; destroy it). */
int avr_set_frame_timeout_ms(int milliseconds);

/* Creates a context bound to HIP device `device_id` with its own stream.  Replaces the
 * function-local static VolumePainter / DirectSendBase instances of
 * VolumeRenderer/VolumeRenderer.cpp:909-927 (one context per rank = per GPU). */
int avr_context_create(int device_id, avr_context **out_ctx);
void avr_context_destroy(avr_context *ctx);

/* The same with the context's own stream created in the device's most urgent priority class
 * (high_priority != 0) or in the default class. */
int avr_context_create_with_priority(int device_id, int high_priority, avr_context **out_ctx);

/* The stream the context launches on (hipStream_t as void*), for ordering other work against it. */
void *avr_context_stream(avr_context *ctx);

/* Use an externally owned HIP stream (hipStream_t passed as void*; NULL = the context's own).
 * All launches of the context go to this stream; nothing in this ABI synchronises the stream
 * except avr_context_synchronize and the *_host readbacks. */
int avr_context_set_stream(avr_context *ctx, void *hip_stream);
int avr_context_synchronize(avr_context *ctx);

/* Resident march workgroups per CU for the launches of this context: 0 (default) = as many as
 * fit (7 by the kernel's registers), 1..7 = capped (the launch reserves 160 KiB / n of LDS per
 * workgroup).  Round 1's frame driver capped its 8-per-CU march at 5 to leave room for the
 * classify pass of the next frame; the present driver leaves the march uncapped and holds the
 * classify pass back instead (avr_context_set_classify_lds_reserve; DESIGN.md section 3, "What
 * the two kernels compete for").  Never changes results. */
int avr_context_set_march_occupancy(avr_context *ctx, int workgroups_per_cu);

/* LDS (bytes, 0 = none) each classify workgroup of this context's launches claims beyond the
 * 2 KiB it stages bricklets in: caps how many of them a CU holds at once.  Beside the march the
 * classify pass takes memory-system time from the march in proportion to the bandwidth it
 * reaches, whatever its arithmetic, occupancy or cache policy (profiles/experiments_rounds_1_to_3.md section 3); the
 * renderer's frame driver uses this to make both kernels of a frame take equally long
 * (avr_renderer_set_classify_share).  Never changes results. */
#define AVR_CLASSIFY_LDS_RESERVE_MAX 61440
int avr_context_set_classify_lds_reserve(avr_context *ctx, int bytes);

/* ---- host-side per-frame quantities (no device work) ------------------------------------- */

/* buildColorTable (Common/VolumePainter.cpp:442-516): 256 RGBA entries to host memory. */
int avr_build_color_table(float alpha_scale, float normalization_factor,
                          const float scalar_range[2], const avr_colormap_point *colormap,
                          int colormap_count, float out_table_host[1024]);

/* sampleDistance / normalizationFactor / alphaScale of one box (VolumePainter.cpp:571-613). */
int avr_box_sampling(const avr_box *box, const avr_paint_params *params, float *sample_distance,
                     float *normalization_factor, float *alpha_scale);

/* computeBoxDepthHint (VolumeRenderer/VolumeRenderer.cpp:541-553). */
int avr_box_depth_hint(const avr_box *box, const avr_camera *camera, float *out_hint);

/* The conservative footprint of a box on a width x height image that the frame plans are built
 * from (host only): its screen rectangle rect[4] = {x0, y0, x1, y1} inclusive (x1 < x0: off
 * screen) -- the march only traces the rays of those pixels -- and, for every image row y, the
 * columns row_x0[y] .. row_x1[y] of the tightened layout (avr_frame_plan_tighten; row_x1 < row_x0:
 * nothing on that row; rows outside the rectangle are empty).  row_x0 / row_x1: height entries
 * each, or NULL.  For the parity tests: every pixel the reference's K1 leaves non-empty for the
 * box (VolumePainter.cpp:802-837: slab hit in front of the eye) must lie inside both. */
int avr_box_footprint(const avr_box *box, const avr_camera *camera, int width, int height,
                      int32_t rect[4], int32_t *row_x0, int32_t *row_x1);

/* referenceSampleDistance of renderSingleTrial (VolumeRenderer/VolumeRenderer.cpp:1138-1190)
 * over the boxes given (the caller reduces with MAX over ranks when boxes are distributed:
 * pass the already-reduced coarsest spacing through avr_paint_params instead). */
int avr_reference_sample_distance(const avr_box *boxes, int n_boxes, const double bounds_min[3],
                                  const double bounds_max[3], float *out_distance);

/* Global layer order of DirectSendBase::composeLayered (DirectSend/Base/DirectSendBase.cpp:
 * 363-410): sorts layers by (hint, owner, local_index); order_out[n] = layer ids,
 * run_end_out[r] = one-past-last position of run r (maximal same-owner stretch); *n_runs_out. */
int avr_layer_order(const float *hints, const int32_t *owner, const int32_t *local_index,
                    int n_layers, int32_t *order_out, int32_t *run_end_out, int *n_runs_out);

/* getPieceRange (DirectSend/Base/DirectSendBase.cpp:59-74). */
int avr_piece_range(int64_t image_size, int piece_index, int num_pieces, int64_t *begin,
                    int64_t *end);

/* ---- painter ----------------------------------------------------------------------------- */

/* VolumePainter::paint (Common/VolumePainter.hpp:19-31, .cpp:548-961) for ONE box: writes
 * width*height depth-sort pixels to out_rgbad (device).  If samples_out (device, 1 x uint64)
 * is non-NULL the number of executed cell fetches is ADDED to it. */
int avr_paint_box(avr_context *ctx, const avr_box *box, const avr_scalar_transform *transform,
                  const avr_paint_params *params, const avr_camera *camera, float *out_rgbad,
                  uint64_t *samples_out);

/* Maximum-intensity projection (MIP) of one box: per pixel, the largest transfer-function table
 * index over the samples avr_paint_box's march takes in the box if its accumulator never
 * saturated -- the same ray, slab bounds, start distance, step, inside test and index clamp, every
 * sample up to the exit point; the index is the byte the classify pass stores for the sample's
 * cell (VolumePainter.cpp:870-883, NaN / Inf / soft-clip rules included), -1 where no sample is
 * taken.  width*height int16 values to out_index (device), in avr_paint_box's pixel order
 * (p = y * width + x, row 0 at the bottom).  samples_out: every sample taken is ADDED to it.
 * box_transparency has no effect (it only scales alpha). */
int avr_paint_box_max(avr_context *ctx, const avr_box *box, const avr_scalar_transform *transform,
                      const avr_paint_params *params, const avr_camera *camera, int16_t *out_index,
                      uint64_t *samples_out);

/* Line-integral (column) projection of one box's raw field: per pixel, over the samples
 * avr_paint_box_max takes in the box (the same ray, slab bounds, start distance, step, inside test
 * and index clamp), the f64 sum S of the finite raw cell values v = cells[i + j*jstride +
 * k*kstride] in march order (no scalar transform, no table) and their number n; then
 * column = f64(step) * S and length = f64(step) * n, step = the box's sample distance.  Both are 0
 * where no finite sample is taken.  width*height f64 values each to column and length (device), in
 * avr_paint_box's pixel order (p = y * width + x, row 0 at the bottom).  samples_out: every sample
 * taken, finite or not, is ADDED to it.  The classified volume is not used; box_transparency, the
 * colour map and the scalar range have no effect.  The cells are read on the context's stream. */
int avr_paint_box_projection(avr_context *ctx, const avr_box *box, const avr_paint_params *params,
                             const avr_camera *camera, double *column, double *length,
                             uint64_t *samples_out);

/* Quantities of avr_projection_colorize */
#define AVR_PROJECTION_COLUMN 0 /* column */
#define AVR_PROJECTION_MEAN 1   /* column / length */

/* Picture of a column projection: column, length as avr_renderer_render_projection returns them
 * (width*height f64, device).  A pixel takes part if length > 0 and, with log_scale, its quantity
 * q > 0 (q = column, or column / length for AVR_PROJECTION_MEAN; log10 of it with log_scale).
 * It gets table entry clamp(floor((q - lo) / (hi - lo) * 255), 0, 255) (entry 0 if hi <= lo); its
 * three bytes of rgb_table (256 x RGB8, device) go to rgb8_out (device, rows top-down as
 * avr_renderer_render writes them); other pixels get (0,0,0).  range (device, 2 f64) holds
 * [lo, hi]; with auto_range it is first set to the min and max of q over the pixels that take part
 * ((0, 1) if none).  Asynchronous on the context's stream. */
int avr_projection_colorize(avr_context *ctx, const double *column, const double *length, int width,
                            int height, int quantity, int log_scale, double *range, int auto_range,
                            const uint8_t *rgb_table, uint8_t *rgb8_out);

/* A scene = the rank's local boxes (geometry.localBoxes, VolumeRenderer.cpp:1201) with one
 * scalar transform (geometry.scalarTransform).  Descriptors are copied to the device; cell
 * data stays where `cells` points. */
int avr_scene_create(avr_context *ctx, const avr_box *boxes, int n_boxes,
                     const avr_scalar_transform *transform, avr_scene **out_scene);
void avr_scene_destroy(avr_scene *scene);

/* Off by default: every frame's classify pass re-reads the f64 cells, as the reference's
 * per-sample fetch does.  When enabled, a classified volume is kept across frames for as long as
 * what it was derived from is unchanged -- the boxes (cell pointers, strides, dimensions), the
 * scalar transform and the scalar range -- so that a camera moving over a static data set only
 * pays for the march.  The cells are the caller's memory: after changing them in place call
 * avr_scene_invalidate.  Results are identical either way. */
int avr_scene_set_classification_cache(avr_scene *scene, int enabled);
int avr_scene_invalidate(avr_scene *scene);

/* Fused replacement of the per-box loop + owner-side run fold
 * (VolumeRenderer.cpp:1201-1219 + DirectSendBase.cpp:413-426): first a streaming classify pass
 * turns every f64 cell of the scene into its transfer-function table index (the per-sample
 * arithmetic of VolumePainter.cpp:870-883 is a pure function of the cell), then one thread per
 * pixel marches the local boxes box_order[0..n) (indices into the scene, already in global
 * layer order) and folds each run (run_end[r] = one-past-last position of run r in box_order)
 * with the depth-sort blend, in order.  Run r's layer is written for ALL pixels in dense "send
 * layout": the image is cut in n_pieces DirectSend pieces (avr_piece_range) and
 *     out[ piece_offset(k) + (r * piece_len(k) + (p - piece_begin(k))) * 5 .. +5 ]
 * with piece_offset(k) = 5 * n_runs * piece_begin(k); for n_pieces == 1 this is simply
 * out[r][p][5].  The result is bit-identical to painting every box into its own layer and
 * blending (empty pixels are an exact identity of the blend).
 * samples_out as in avr_paint_box. */
int avr_render_runs(avr_context *ctx, const avr_scene *scene, const avr_paint_params *params,
                    const avr_camera *camera, const int32_t *box_order, int n_order,
                    const int32_t *run_end, int n_runs, int n_pieces, float *out_layers,
                    uint64_t *samples_out);

/* ---- frame plan: layered DirectSend with one sparse exchange ------------------------------ */

/* One frame's compositing plan, identical on every rank.  Replaces the per-frame allgather of
 * layer counts / depth hints, the global sort and the run grouping of
 * DirectSendBase::composeLayered (DirectSend/Base/DirectSendBase.cpp:329-410) -- depth hints
 * depend only on box corners and the camera, so every rank derives them from the replicated box
 * metadata -- and adds, per run, the conservative screen rectangle of its boxes: pixels outside
 * it hold the empty layer pixel (0,0,0,0,+inf), an exact identity of the blend, and are neither
 * stored nor sent.
 *
 *   all_boxes[n_boxes]  metadata of every box of the scene (cells may be NULL), level-major;
 *   owner[n_boxes]      owning rank; a rank's local index of a box is its position among the
 *                       boxes it owns (geometry.localBoxes order);
 *   group_order         rank at position k of the ordered MPI group of Compositor::compose
 *                       (Common/Compositor.hpp:19-40); NULL = identity.  Position k holds
 *                       pixel piece k (DirectSendBase.cpp:76-130).  Pixel values do not depend
 *                       on it (SURVEY.md 8c probe 1).
 * Exchange layout (floats; 5 per pixel):
 *   send buffer = for peer rank s = 0..n-1: for local run r: block(piece of s, r)
 *   recv buffer = for source rank s = 0..n-1: for run r of s: block(my piece, r)
 *   block(k, r) = rows [max(rect.y0, first row of piece k), min(rect.y1, last row of piece k)]
 *                 x columns [rect.x0, rect.x1] of run r, row-major.
 * so one all-to-all (split sizes from avr_frame_plan_splits) replaces the N(N-1) messages per
 * run of the reference. */
typedef struct avr_frame_plan avr_frame_plan;

typedef struct {
  int32_t n_ranks, rank;
  int32_t n_runs_total;   /* global runs, all ranks */
  int32_t n_local_runs;   /* runs owned by this rank */
  int32_t n_local_boxes;
  int64_t n_pixels;       /* render width * height */
  int64_t piece_begin;    /* this rank's DirectSend piece [begin, end) */
  int64_t piece_end;
  int64_t send_floats;    /* total size of the send / recv buffers */
  int64_t recv_floats;
  int32_t piece_layout;   /* AVR_PIECES_CONTIGUOUS / AVR_PIECES_ROW_BANDS (see below) */
  int32_t band_rows;
} avr_frame_plan_info;

/* How the image is dealt to the ranks' pieces.  AVR_PIECES_CONTIGUOUS is the reference's
 * partition (DirectSendBase.cpp:59-74) and what Compositor::compose promises its caller.
 * AVR_PIECES_ROW_BANDS deals bands of band_rows image rows round-robin (band b -> piece b % N):
 * every rank then receives and folds the same share of every screen region (contiguous pieces of
 * a scene that covers a third of the image leave some ranks with nothing and others with
 * everything).  Per-pixel results do not depend on which rank folds a pixel, so the gathered
 * image is identical; piece_begin is 0 and piece_end the piece's pixel count there (its rows in
 * image order), the gathered buffer is piece-major, and avr_assemble_rows restores image order.
 * Used by the frame driver (avr_renderer), whose caller only ever sees the gathered image. */
#define AVR_PIECES_CONTIGUOUS 0
#define AVR_PIECES_ROW_BANDS 1

/* One run as seen by the exchange (for inspection and tests). */
typedef struct {
  int32_t owner;          /* owning rank */
  int32_t local_run;      /* index among the owner's runs */
  int32_t first_layer;    /* position of its first layer in the global order */
  int32_t n_layers;
  int32_t rect[4];        /* x0, y0, x1, y1 inclusive; x1 < x0 = empty */
} avr_run_info;

int avr_frame_plan_create(const avr_box *all_boxes, const int32_t *owner, int n_boxes,
                          int n_ranks, int rank, const int32_t *group_order,
                          const avr_paint_params *params, const avr_camera *camera,
                          avr_frame_plan **out_plan);
/* The same with a piece layout (avr_frame_plan_create = AVR_PIECES_CONTIGUOUS). */
int avr_frame_plan_create_pieces(const avr_box *all_boxes, const int32_t *owner, int n_boxes,
                                 int n_ranks, int rank, const int32_t *group_order,
                                 const avr_paint_params *params, const avr_camera *camera,
                                 int piece_layout, int band_rows, avr_frame_plan **out_plan);
/* The same plan for layers that are only known as images with a depth hint -- the generic
 * Compositor::compose(Image*, MPI_Group, MPI_Comm) of a LayeredImageInterface
 * (DirectSend/Base/DirectSendBase.cpp:316-458): hints[l] / owner[l] for ALL layers of all ranks in
 * rank-major order (what the reference's MPI_Allgatherv of the depth hints delivers, :354-361; a
 * layer's local index is its position among its owner's layers).  Every run covers the whole
 * image.  Use with avr_pack_layers, avr_exchange, avr_fold_plan. */
int avr_layered_plan_create(const float *hints, const int32_t *owner, int n_layers, int n_ranks,
                            int rank, const int32_t *group_order, int width, int height,
                            avr_frame_plan **out_plan);
/* Owner-side run fold of already painted layers (DirectSendBase.cpp:413-426) into the send buffer
 * of a layered plan: local_layers[i] = device pointer to this rank's layer i (width*height*5
 * floats), host array. */
int avr_pack_layers(avr_context *ctx, const avr_frame_plan *plan, const float *const *local_layers,
                    int n_local_layers, float *send_buffer);
void avr_frame_plan_destroy(avr_frame_plan *plan);
int avr_frame_plan_get_info(const avr_frame_plan *plan, avr_frame_plan_info *out);
/* all_to_all split sizes in floats, indexed by peer rank (n_ranks entries each). */
int avr_frame_plan_splits(const avr_frame_plan *plan, int64_t *send_splits, int64_t *recv_splits);
/* Global layer order: layer_box[l] = index into all_boxes of the l-th layer; n_boxes entries. */
int avr_frame_plan_layers(const avr_frame_plan *plan, int32_t *layer_box);
/* runs[n_runs_total] in global order. */
int avr_frame_plan_runs(const avr_frame_plan *plan, avr_run_info *runs);
/* Tightens the exchange layout of a plan made by avr_frame_plan_create: instead of its whole
 * screen rectangle, every row of a run stores only the conservative extent of the run's boxes on
 * that row (the convex hull of each box's projected corners, +2 pixels); what lies outside is the
 * cleared layer pixel -- the exact identity of the depth-sort blend (DirectSendBase.cpp:400-446
 * blends it like any other) -- on the sender and the receiver alike, so results do not change
 * while send_floats / recv_floats and the splits shrink (config-4: the rectangles are 48-72 %
 * filled).  Sizes still follow from the replicated metadata: EVERY rank must tighten the plan of
 * a frame or none.  all_boxes as given to avr_frame_plan_create.  The march counts, in the 5th
 * diagnostic counter (avr_context_set_march_counters, avr_hip_debug.h), non-empty pixels it found outside a span:
 * always 0.  avr_frame_plan_send_block / recv_block do not apply to a tightened plan. */
int avr_frame_plan_tighten(avr_frame_plan *plan, const avr_box *all_boxes, int n_boxes);

/* Offset (floats) of block(piece of `peer`, local run r) in the send buffer and of
 * block(my piece, global run g) in the recv buffer; -1 when the block is empty.
 * first_row receives the image row of the block's first row. */
int avr_frame_plan_send_block(const avr_frame_plan *plan, int peer, int local_run,
                              int64_t *offset, int32_t *first_row, int32_t *n_rows);
int avr_frame_plan_recv_block(const avr_frame_plan *plan, int global_run, int64_t *offset,
                              int32_t *first_row, int32_t *n_rows);

/* Classify + march of this rank's runs into the sparse send buffer (send_floats floats).
 * The scene must hold this rank's boxes in local-index order.  samples_out as avr_paint_box. */
int avr_render_plan(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan,
                    float *send_buffer, uint64_t *samples_out);

/* The two halves of avr_render_plan as separate calls, for pipelining frames: the classify pass
 * of frame i+1 (any context / stream) may run while frame i is still marched.  `slot`
 * (0 .. AVR_CLASSIFIED_SLOTS-1) selects one of the scene's classified volumes (each allocated
 * when first used); the caller orders march(slot) after classify(slot) of the same frame and
 * classify(slot) after the previous march(slot).  Two slots are enough to overlap; with three
 * the classify stream can run a frame further ahead, so that neither stream waits for a launch
 * on the other (avr_renderer does). */
#define AVR_CLASSIFIED_SLOTS 3
int avr_classify_plan(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan,
                      int slot);
int avr_march_plan(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan, int slot,
                   float *send_buffer, uint64_t *samples_out);

/* Maximum-intensity frames (avr_paint_box_max per pixel and box): avr_render_plan and
 * avr_march_plan with the MIP march.  The same plan, classified volume and send layout; a run's
 * layer pixel is (RGB of table entry i, 1, i) for the run's largest index i and the cleared pixel
 * (0,0,0,0,+inf) where it takes no sample, so that tightening, avr_exchange_peers and the gathers
 * carry it unchanged.  Fold with the avr_fold_plan*_max calls below.  No chunks, no speculation. */
int avr_render_plan_max(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan,
                        float *send_buffer, uint64_t *samples_out);
int avr_march_plan_max(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan, int slot,
                       float *send_buffer, uint64_t *samples_out);

/* Column-projection frames (avr_paint_box_projection per pixel and box): the march of the plan
 * over the scene's raw cells -- no classify pass; the classified volume (slot: as
 * avr_march_plan_max, not read) is neither read nor written.  A run's layer pixel is
 * (column lo, column hi, length lo, 1, length hi) -- the 32-bit halves of its f64 sums over its boxes
 * in order, column = sum of f64(step) * S_b, length = sum of f64(step) * n_b -- where length > 0,
 * and the cleared pixel (0,0,0,0,+inf) elsewhere, so that tightening, avr_exchange_peers and the
 * gathers carry it unchanged.  Fold with the avr_fold_plan*_projection calls.  No chunks, no
 * speculation.  The cells are read by the march, on the context's stream. */
int avr_render_plan_projection(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan,
                               float *send_buffer, uint64_t *samples_out);
int avr_march_plan_projection(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan,
                              int slot, float *send_buffer, uint64_t *samples_out);

/* ONE frame in n_chunks (2 .. AVR_MAX_FRAME_CHUNKS) depth-ordered chunks, for the caller who waits
 * for every frame (the reference's Render() returns after one: VolumeRenderer.cpp:1103-1339): the
 * rank's boxes are cut, in global layer order, into chunks of equal classify work; chunk k is
 * classified by launch k of avr_classify_plan_chunked (which then records chunk_events[k],
 * hipEvent_t as void*, on its stream) and marched by launch k of avr_march_plan_chunked (which
 * first makes its stream wait for chunk_events[k]) -- so chunk k is marched while chunk k + 1 is
 * still being classified and the frame's latency is one chunk's classify pass plus the march, not
 * the whole pass plus the march.  The run accumulators are carried from launch to launch through
 * the send buffer: the run's left fold (DirectSendBase.cpp:413-426) is cut, never re-associated,
 * so the results equal avr_march_plan's bit for bit.  chunk_events may be NULL when both calls go
 * to one stream.  first_alone != 0: nothing else runs beside chunk 0's classify launch, so it
 * takes no LDS reserve (avr_context_set_classify_lds_reserve).  Not with a cached classification. */
#define AVR_MAX_FRAME_CHUNKS 16
int avr_classify_plan_chunked(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan,
                              int slot, int n_chunks, void *const *chunk_events, int first_alone);
int avr_march_plan_chunked(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan,
                           int slot, float *send_buffer, uint64_t *samples_out, int n_chunks,
                           void *const *chunk_events);

/* The same frame with OCCLUSION CULLING between its chunks, one call: classify 0, march 0,
 * classify 1, march 1 ... on the context's stream.  The march skips a box at every pixel whose run
 * accumulator is opaque and in front of the box (the blend would return the accumulator unchanged:
 * the reference's early exit `accumA < 1`, VolumePainter.cpp:837, carried from box to box); the
 * march launch of chunk k evaluates that same test for every box behind it and flags the boxes
 * some ray may still sample (visibility: device, n_chunks * n_local_boxes bytes of scratch), and
 * the classify launch of chunk k + 1 leaves out the others -- their f64 cells are not even read.
 * With the reference's default boxTransparency = 0 most rays saturate in the first boxes, and a
 * frame reads a fraction of its cells.  Results equal avr_render_plan's bit for bit: a box is left
 * out only where the march provably never reads it (proof with the kernel, avr_kernels.hip). */
int avr_render_plan_culled(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan,
                           int slot, float *send_buffer, uint64_t *samples_out, int n_chunks,
                           uint8_t *visibility);

/* SPECULATIVE frames: occlusion culling from one frame to the next, exact.  With the reference's
 * default boxTransparency = 0 (VolumeRenderer.hpp:36) most rays saturate in the first boxes they
 * cross (VolumePainter.cpp:837 carried from box to box: the march skips a box wherever the run
 * accumulator in front of it is opaque), so a frame reads the f64 cells of boxes no ray samples.
 * A frame of the same plan as an earlier one may therefore classify only the boxes that earlier
 * frame's march sampled (`visited`, recorded by avr_march_plan_speculative):
 *   avr_classify_plan_flagged(flags = that frame's visited[])      the covered boxes only
 *   avr_march_plan_speculative(classified = the same flags, ...)   checks every box it needs
 * The march that needs a box the flags left out (the cells changed, say) raises missed[position]
 * and miss_count, leaves the box out and goes on; with a less opaque accumulator it can only need
 * MORE boxes than the true frame, so the raised flags cover everything the true frame needs, and
 * the caller queues, unconditionally, the repair behind it on the same stream:
 *   avr_classify_plan_flagged(flags = missed, gate = miss_count)   a small grid, idle unless *gate
 *   avr_march_plan_speculative(classified = NULL, gate = miss_count, ...)   the whole march again
 * Both do nothing when no flag was raised (the usual case: two launches of a few microseconds).
 * Results equal avr_classify_plan + avr_march_plan bit for bit either way.  All arrays are device
 * memory of plan->info.n_local_boxes entries, indexed by the position of a box among this rank's
 * boxes in the plan's global layer order (opaque to the caller: flags one call wrote are what the
 * next one reads); visited / missed / miss_count are cleared by the caller.
 * host_miss_flag: NULL, or device-visible host memory that the march sets to 1 on a miss. */
typedef struct avr_speculation {
  const uint8_t *classified; /* != 0: classified this frame; NULL: every box is */
  uint8_t *visited;          /* out (or NULL): 1 for every box some ray sampled */
  uint8_t *missed;           /* out: boxes needed but not classified (NULL only if classified is) */
  uint32_t *miss_count;      /* out: raised with every miss */
  uint32_t *host_miss_flag;  /* out, or NULL */
  const uint32_t *gate;      /* NULL, or: the march does nothing unless *gate != 0 */
  const uint8_t *classified_host; /* instead of `classified`: the same flags in HOST memory, copied
                                     with the launch's descriptors (a caller who decides per frame) */
  uint8_t *dirty_workgroups; /* NULL, or device memory of avr_march_plan_workgroups(plan) bytes, cleared
                                by the caller: the checking march marks the workgroups that met an
                                unclassified box, the gated march (same pointer) redoes only those --
                                every other layer pixel is final after the first pass */
} avr_speculation;
/* An upper bound of the workgroups of this rank's march launch of the plan: the bytes to give
 * dirty_workgroups. */
int avr_march_plan_workgroups(const avr_frame_plan *plan, int64_t *workgroups);
int avr_classify_plan_flagged(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan,
                              int slot, const uint8_t *flags, const uint32_t *gate);
int avr_march_plan_speculative(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan,
                               int slot, float *send_buffer, const avr_speculation *speculation);
/* The flagged classify pass for a caller who has the flags on the HOST (copied from `visited` a few
 * frames ago): positions[0 .. n_positions) ascending -- a launch of exactly those boxes' tiles
 * (avr_classify_plan_flagged launches a workgroup per tile of every box and lets the unflagged ones
 * return: a sixth of config-4's flagged pass).  The march is then given the same set as flags. */
int avr_classify_plan_positions(avr_context *ctx, const avr_scene *scene, const avr_frame_plan *plan,
                                int slot, const int32_t *positions, int n_positions);

/* Receiver side of composeLayered (DirectSendBase.cpp:400-446) for this rank's piece: folds
 * the runs in global order from the received buffer (recv_floats floats; with one rank the send
 * buffer itself) into out_piece[(piece_end - piece_begin) * 5]; pixels no run covers become the
 * cleared layer pixel (DirectSendBase.cpp:450-455).  If out_rgb8 is non-NULL the piece is also
 * written as RGB8 (Color::GetComponentAsByte, 3 bytes per pixel, same pixel order); out_piece
 * may then be NULL when only the bytes are wanted (20 of the 23 bytes stored per pixel). */
int avr_fold_plan(avr_context *ctx, const avr_frame_plan *plan, const float *recv_buffer,
                  float *out_piece, uint8_t *out_rgb8);
/* The same fold with the blocks of the rank's OWN runs read where the march stored them -- in
 * own_send_buffer, the rank's send buffer (its block for itself has the same layout there as in
 * the receive buffer) -- instead of from recv_buffer: with avr_exchange_peers a rank's data for
 * itself is never copied (one kernel and one gap less on the compositing stream of every frame,
 * which at N = 8 has five kernels to run in 0.15 ms).  own_send_buffer NULL: avr_fold_plan. */
int avr_fold_plan_own(avr_context *ctx, const avr_frame_plan *plan, const float *recv_buffer,
                      const float *own_send_buffer, float *out_piece, uint8_t *out_rgb8);
/* One rank (the piece is the image): the fold with its bytes written as the output file's rows,
 * top-down (SavePPM.cpp:25) -- avr_fold_plan + avr_assemble_rows(flip) in one pass over the
 * pixels.  out_rgb8_image: width * height * 3 bytes; out_piece as avr_fold_plan (may be NULL). */
int avr_fold_plan_image(avr_context *ctx, const avr_frame_plan *plan, const float *recv_buffer,
                        float *out_piece, uint8_t *out_rgb8_image);

/* The max fold of a maximum-intensity frame (avr_render_plan_max): per pixel of the piece, the
 * largest index among the covering runs that took a sample (max is exact and order-free).
 * out_index (may be NULL): the piece's int16 indices, -1 where no run took a sample, in the order
 * of avr_fold_plan's out_piece; out_rgb8 (may be NULL): Color::GetComponentAsByte of the RGB of
 * that table entry, (0,0,0) for -1.  _own and _image as avr_fold_plan_own / avr_fold_plan_image
 * (the image's bytes top-down; out_index stays in piece order). */
int avr_fold_plan_max(avr_context *ctx, const avr_frame_plan *plan, const float *recv_buffer,
                      int16_t *out_index, uint8_t *out_rgb8);
int avr_fold_plan_own_max(avr_context *ctx, const avr_frame_plan *plan, const float *recv_buffer,
                          const float *own_send_buffer, int16_t *out_index, uint8_t *out_rgb8);
int avr_fold_plan_image_max(avr_context *ctx, const avr_frame_plan *plan, const float *recv_buffer,
                            int16_t *out_index, uint8_t *out_rgb8_image);

/* The sum fold of a column-projection frame (avr_render_plan_projection): per pixel of the piece,
 * the column and length of the covering runs that took a finite sample, added in fold (global
 * run) order in f64.  out_column / out_length (either may be NULL): the piece's f64 values, 0
 * where no run took a finite sample, in the order of avr_fold_plan's out_piece.  _own as
 * avr_fold_plan_own; _image: one rank's whole image (the same order: row 0 at the bottom). */
int avr_fold_plan_projection(avr_context *ctx, const avr_frame_plan *plan, const float *recv_buffer,
                             double *out_column, double *out_length);
int avr_fold_plan_own_projection(avr_context *ctx, const avr_frame_plan *plan, const float *recv_buffer,
                                 const float *own_send_buffer, double *out_column, double *out_length);
int avr_fold_plan_image_projection(avr_context *ctx, const avr_frame_plan *plan,
                                   const float *recv_buffer, double *out_column, double *out_length);

/* ---- image algebra ----------------------------------------------------------------------- */

/* Features::blend over n pixels, out = blend(top, bottom); out may alias top or bottom.
 * ImageRGBAFloatColorDepthSort.hpp:13-27 / ImageRGBAFloatColorOnly.hpp:19-26 /
 * ImageRGBAUByteColorOnly.hpp:19-34 (uint8 wrap-around preserved). */
int avr_blend_depthsort_f32x5(avr_context *ctx, const float *top, const float *bottom,
                              float *out, int64_t n_pixels);
int avr_blend_rgba_f32x4(avr_context *ctx, const float *top, const float *bottom, float *out,
                         int64_t n_pixels);
int avr_blend_rgba_u8x4(avr_context *ctx, const uint32_t *top, const uint32_t *bottom,
                        uint32_t *out, int64_t n_pixels);

/* ImageColorOnly<F>::blend with pixel regions (Common/ImageColorOnly.hpp:119-199): top covers
 * [tb,te), bottom [bb,be), out covers [min(tb,bb), max(te,be)); the regions must touch or
 * overlap.  kind: 0 depth-sort, 1 float, 2 ubyte.  out must not alias the inputs. */
int avr_blend_regions(avr_context *ctx, int kind, const void *top, int64_t tb, int64_t te,
                      const void *bottom, int64_t bb, int64_t be, void *out);

/* Color::GetComponentAsByte / SetComponentFromByte over n RGBA pixels
 * (Common/Color.hpp:66-91, ImageRGBAUByteColorOnly.cpp:16-39). */
int avr_encode_rgba_u8(avr_context *ctx, const float *rgba, uint32_t *out, int64_t n_pixels);
int avr_decode_rgba_u8(avr_context *ctx, const uint32_t *in, float *rgba, int64_t n_pixels);

/* Receiver-side fold of DirectSendBase::composeLayered (DirectSendBase.cpp:400-446) for one
 * piece of n_pixels pixels: slices[r] (device pointers, host array) are the piece's pixels of
 * global run r in global order; out = fold_left(blend, slices).  n_slices == 0 writes the
 * cleared layer (0,0,0,0,+inf) (DirectSendBase.cpp:450-455). */
int avr_fold_runs_depthsort(avr_context *ctx, const float *const *slices_host, int n_slices,
                            float *out, int64_t n_pixels);

/* ---- frame tail --------------------------------------------------------------------------- */

/* downsampleImage (VolumeRenderer/VolumeRenderer.cpp:479-528): block x block box mean of a
 * (target_w*block) x (target_h*block) depth-sort image; depth := +inf. */
int avr_downsample_depthsort(avr_context *ctx, const float *src, int target_w, int target_h,
                             int block, float *dst);

/* SavePPM/SavePNG pixel bytes (Common/SavePPM.cpp:17-36, Common/Color.hpp:86-90): RGB8 from an
 * image of `stride` floats per pixel, rows written top-down (y = h-1 .. 0). dst = w*h*3 bytes. */
int avr_quantize_rgb8(avr_context *ctx, const float *src, int w, int h, int stride,
                      uint8_t *dst);

/* Rows of an h-row byte image in reverse order: the composited image has its origin bottom-left,
 * the output file's rows run top-down (Common/SavePPM.cpp:25, Common/SavePNG.cpp:64-71). */
int avr_flip_rows(avr_context *ctx, const uint8_t *src, int64_t row_bytes, int h, uint8_t *dst);

/* ---- rank communicator: the DirectSend exchange and the gather over RCCL / xGMI ----------- */

/* One communicator per rank (= per GPU, one process per rank).  Replaces the MPI communicator +
 * group handed to Compositor::compose (Common/Compositor.hpp:35-37): the image-fragment exchange
 * of DirectSendBase::PostSends / PostReceives (DirectSend/Base/DirectSendBase.cpp:76-177) and
 * ImageFull::Gather (Common/ImageColorOnly.hpp:220-270) become one grouped ncclSend / ncclRecv
 * round each, on device buffers, launched on the calling context's stream.
 *
 * avr_comm_unique_id is called on ONE rank; the caller distributes the id to the others by its
 * own means (the reference's host already has MPI: MPI_Bcast of 128 bytes; torch.distributed's
 * store in the Python layer); then every rank calls avr_comm_create (collective). */
typedef struct avr_comm avr_comm;
#define AVR_COMM_ID_BYTES 128
int avr_comm_unique_id(char id_out[AVR_COMM_ID_BYTES]);
int avr_comm_create(int device_id, const char id[AVR_COMM_ID_BYTES], int rank, int n_ranks,
                    avr_comm **out_comm);
/* In-process rehearsal of an N-rank frame on ONE GPU: n_ranks connected communicators for n_ranks
 * host threads of this process (host-synchronous device copies).  Not a performance path -- RCCL
 * cannot place two ranks on one device, and this keeps the N-rank frame testable there. */
int avr_comm_create_local(int n_ranks, avr_comm **out_comms /* [n_ranks] */);
/* ONE rank of an N-rank frame played alone (timing studies of a rank's share on a single GPU,
 * tools/rank_share.py): only the block a rank keeps for itself moves, the peers' blocks of the
 * receive buffer keep whatever they held.  Frames rendered this way are not images. */
int avr_comm_create_solo(int rank, int n_ranks, avr_comm **out_comm);
/* The same, with the rank's collectives played through RCCL to ITSELF (a one-rank communicator
 * made here): avr_exchange sends and receives every peer's block -- the smaller of its two sizes
 * -- as one grouped ncclSend / ncclRecv round, avr_gather likewise.  What a one-GPU box can show
 * of the real round: its launch on the host, its kernel beside the paint kernels, its bytes
 * through HBM; not the links.  percent (1..100): the share of every peer's block avr_exchange
 * moves -- on the node the N - 1 blocks travel over N - 1 links at once, here one after the other
 * over one connection, so 100 overstates how long the round's kernel runs.  percent 0 = "one link":
 * only the largest peer block travels, whole, and the root's gather receives one peer's piece --
 * what the busiest of a rank's N - 1 links carries; RCCL works off the operations for ONE peer one
 * after the other (~13 us each, measured), a serialisation the node, with one peer per link, does
 * not have.  Timing only. */
int avr_comm_create_solo_rccl(int device_id, int rank, int n_ranks, int percent,
                              avr_comm **out_comm);
/* Rehearsal of the N-rank frame across PROCESSES that share one GPU (RCCL refuses two ranks on
 * one device): the ranks meet in the POSIX shared-memory segment `name` ("/something"; whoever
 * comes first creates it, rank 0 removes the name when it is destroyed), capacity_bytes of staging
 * per rank -- at least a rank's largest send buffer, piece or image.  Blocks travel device ->
 * the sender's region -> device with the plans, offsets and ordering of the RCCL flavour; every
 * call is host-synchronous and a peer that does not arrive within 120 s fails the call instead of
 * hanging it.  Collective (the call returns when every rank has attached).  Not a performance
 * path: it exists so that the whole multi-process flow -- control plane, frame driver, bench --
 * runs where one GPU is all there is. */
int avr_comm_create_shared(const char *name, int rank, int n_ranks, size_t capacity_bytes,
                           avr_comm **out_comm);
void avr_comm_destroy(avr_comm *comm);
int avr_comm_rank(const avr_comm *comm);
int avr_comm_size(const avr_comm *comm);

/* Control plane of the communicator: a small host-side allgather among the ranks -- what the
 * reference does with MPI_Allgather on MPI_COMM_WORLD for its layer counts and depth hints
 * (DirectSend/Base/DirectSendBase.cpp:329-361).  Used for the agreement check of a new frame plan
 * (avr_frame_plan_agree) and for the decisions of the frame driver's co-run search, which all
 * ranks of a frame take together; never per frame.
 * avr_comm_set_control hands over the caller's own (the reference's host: MPI_Allgather of
 * bytes_per_rank bytes; bench.py: gloo): allgather(user, mine, all, bytes_per_rank) fills
 * all[rank * bytes_per_rank ...] for every rank and returns 0.  Without one, the RCCL flavour runs
 * a grouped round of tiny ncclSend / ncclRecv in band on the given context's stream (host-blocking,
 * with the deadline of avr_set_frame_timeout_ms); the rehearsal flavours meet in their own memory.
 * The caller's allgather runs under the same deadline: it is called on a helper thread over copies
 * of the buffers, and a round that outlasts the deadline returns AVR_ERR_RUNTIME (the renderer
 * that asked is failed for good) while the helper is left behind in the caller's collective -- so
 * a caller's allgather should still carry a timeout of its own (MPI: a communicator error
 * handler; gloo: the process group's timeout) to end that thread. */
#define AVR_CONTROL_MAX_BYTES 2048
typedef int (*avr_control_allgather_fn)(void *user, const void *mine, void *all, int bytes_per_rank);
int avr_comm_set_control(avr_comm *comm, avr_control_allgather_fn allgather, void *user);
/* Collective, host-blocking: bytes (a multiple of 4, <= AVR_CONTROL_MAX_BYTES) of every rank into
 * all[n_ranks * bytes].  ctx: the context whose stream carries the in-band round (RCCL flavour
 * without a caller's control plane); may be NULL otherwise. */
int avr_comm_control_allgather(avr_comm *comm, avr_context *ctx, const void *mine, void *all,
                               int bytes);
long avr_comm_control_rounds(const avr_comm *comm); /* control-plane calls so far (diagnostics) */
/* Do the ranks' plans of one frame describe ONE exchange?  Collective over the control plane: every
 * rank contributes a digest of the plan's replicated part (image, pieces, group order, runs, layer
 * order) mixed with settings_digest (whatever else the caller requires to be equal on all ranks)
 * and its send / receive block sizes; every rank then checks the whole matrix -- rank a's block
 * for rank b must be what b expects from a -- and so every rank reaches the same verdict:
 * AVR_OK, or AVR_ERR_RUNTIME (naming the first pair that disagrees) on ALL of them, before
 * anything has been queued.  A grouped ncclSend / ncclRecv round whose two sides disagree on a
 * size never ends; the reference finds out from the metadata message of every transfer
 * (Common/Image.cpp:62-90).  The frame driver calls it once per new plan (avr_renderer_set_plan_check). */
int avr_frame_plan_agree(const avr_frame_plan *plan, avr_comm *comm, avr_context *ctx,
                         uint64_t settings_digest);

/* The sparse all-to-all of one frame (layout: "frame plan" above): block for peer s of `send` goes
 * to rank s, `recv` receives the blocks of all ranks for this rank's piece.  Collective; on the
 * context's stream. */
int avr_exchange(avr_context *ctx, const avr_frame_plan *plan, avr_comm *comm, const float *send,
                 float *recv);
/* avr_exchange without the copy of the rank's block for itself: recv holds the peers' blocks
 * only, the rank's own stay in send (avr_fold_plan_own reads them there; send must then live until
 * that fold has run). */
int avr_exchange_peers(avr_context *ctx, const avr_frame_plan *plan, avr_comm *comm,
                       const float *send, float *recv);
/* Classic direct send of ONE image per rank -- DirectSendBase::compose(localImage, sendGroup,
 * recvGroup, comm) for a plain (not layered) image, DirectSend/Base/DirectSendBase.cpp:76-177,
 * 257-281: every rank's image (n_pixels * bytes_per_pixel bytes, device) is cut into the n pieces of
 * avr_piece_range; piece k goes to the rank at position k of group_order (NULL = rank order).
 * Received: `slices` = n blocks of this rank's own piece (its pixel count * bytes_per_pixel bytes
 * each), block j cut from the image of the rank at group position j -- the order in which
 * ProcessIncomingImages blends them (:179-255: the lower position on top).  One grouped ncclSend /
 * ncclRecv round on the context's stream; fold the blocks with avr_blend_regions. */
int avr_exchange_pieces(avr_context *ctx, avr_comm *comm, const int32_t *group_order,
                        int64_t n_pixels, int bytes_per_pixel, const void *image, void *slices);
/* ImageFull::Gather: every rank's piece (bytes_per_pixel bytes per pixel: 20 for the depth-sort
 * image, 3 for its RGB8 bytes) lands at its pixel range in `full` on rank `root` (full is ignored
 * elsewhere).  Collective; on the context's stream. */
int avr_gather(avr_context *ctx, const avr_frame_plan *plan, avr_comm *comm, const void *piece,
               int bytes_per_pixel, void *full, int root);
/* The same gather described without a plan: begin / end [n_ranks] = where each rank's piece sits in
 * `full`, in pixels (avr_frame_plan_piece_ranges of the frame the pieces belong to).  skip_own: the
 * root does not copy its own piece into `full` (avr_assemble_rows_own reads it where it is).
 * avr_exchange_peers_gather: avr_exchange_peers with such a gather -- of an EARLIER frame's pieces
 * -- riding in the same grouped ncclSend / ncclRecv round: the frame driver's compositing stream
 * then carries ONE RCCL launch per frame (the reference's Gather is a second collective after the
 * compositing, Common/ImageColorOnly.hpp:220-270; frames are independent, so frame f's bytes may
 * travel to the root while frame f + 1 is exchanged).  rider may be NULL. */
typedef struct {
  const void *piece;       /* this rank's piece (device) */
  int32_t bytes_per_pixel;
  int32_t root;
  void *full;              /* on the root: the gathered, piece-major buffer (device) */
  const int64_t *begin;    /* [n_ranks] */
  const int64_t *end;      /* [n_ranks] */
  int32_t skip_own;
} avr_gather_op;
int avr_frame_plan_piece_ranges(const avr_frame_plan *plan, int64_t *begin_out, int64_t *end_out);
int avr_gather_run(avr_context *ctx, avr_comm *comm, const avr_gather_op *op);
int avr_exchange_peers_gather(avr_context *ctx, const avr_frame_plan *plan, avr_comm *comm,
                              const float *send, float *recv, const avr_gather_op *rider);

/* ---- frame driver -------------------------------------------------------------------------- */

/* VolumeRenderer::RenderParameters (VolumeRenderer/VolumeRenderer.hpp:33-44), the fields the hot
 * path reads.  draw_bounds: the reference always blends the wireframe of the tight bounds over the
 * final image (VolumeRenderer.cpp:1311-1314); 0 leaves it out. */
typedef struct {
  int32_t width, height;
  float box_transparency;
  int32_t antialiasing;
  int32_t use_visibility_graph;
  int32_t draw_bounds;
  int32_t write_visibility_graph;
} avr_render_params;

/* One rank's share of VolumeRenderer::renderSingleTrial (VolumeRenderer.cpp:1103-1339) from the
 * per-box loop to the 8-bit image, pipelined over three HIP streams of its own: frame i+1 is
 * classified while frame i is marched and frame i-1 is exchanged, folded and gathered.
 *   all_boxes / owner   metadata of EVERY box of the scene (replicated on all ranks), level-major;
 *                       the boxes of `rank` must carry their cell pointers (HBM);
 *   comm                NULL for one rank.
 * Replaces the function-local static VolumePainter / DirectSendBase pair of
 * VolumeRenderer.cpp:909-927 together with the loop that drives them. */
typedef struct avr_renderer avr_renderer;
int avr_renderer_create(int device_id, int rank, int n_ranks, avr_comm *comm,
                        const avr_box *all_boxes, const int32_t *owner, int n_boxes,
                        const avr_scalar_transform *transform, const double bounds_min[3],
                        const double bounds_max[3], const float scalar_range[2],
                        const avr_colormap_point *colormap, int colormap_count,
                        avr_renderer **out_renderer);
void avr_renderer_destroy(avr_renderer *renderer);
/* march_workgroups_per_cu: -1 default (uncapped), 0..8 as avr_context_set_march_occupancy.  cache_classification: avr_scene_set_classification_cache. */
int avr_renderer_set_options(avr_renderer *renderer, int march_workgroups_per_cu,
                             int cache_classification);
/* geometry.scalarRange of the scene (VolumeRenderer.hpp:74-89) for the frames that follow. */
int avr_renderer_set_scalar_range(avr_renderer *renderer, const float scalar_range[2]);
/* avr_scene_invalidate for the renderer's scene: call after changing cell data in place while
 * cache_classification is on. */
int avr_renderer_invalidate(avr_renderer *renderer);
/* How a frame's two paint kernels are laid out on the streams:
 *   0  back to back on the march stream;
 *   1  side by side: the classify pass of frame i+1 on its own stream beside the march of frame i;
 *   2  paired: every frame's classify pass and march back to back on ONE stream, the even frames
 *      on stream M, the odd ones on a second stream -- the classify pass of frame i+1 still runs
 *      beside the march of frame i, but a march never queues behind its predecessor, so its tail
 *      runs beside whatever the other stream has next (a rank of eight of config-4: 0.165 ->
 *      0.145 ms; one rank: 0.986 -> 1.015 ms);
 *  -1  (default) whichever the driver measures to be fastest (avr_renderer_set_classify_share).
 * Never changes results. */
int avr_renderer_set_overlap(avr_renderer *renderer, int overlap_classify);
/* A frame re-uses the classified volume and the send buffer of the frame three before it.
 * 0: the frame's streams wait for that frame on the GPU (two wait packets; the host runs a few
 * frames ahead).  1: the HOST waits inside avr_renderer_render until that frame's march and
 * exchange / fold are through and queues no wait -- at most three frames in flight, and a
 * descriptor batch that repeats (same camera and parameters) leaves no packet at all on the
 * streams: for the short frames of a rank of several every packet between two kernels counts
 * (a rank of eight of config-4: 0.187 -> 0.164 ms).  -1 (default): 1 for more than one rank,
 * 0 for one rank (whose 1 ms frames hide the packets and lose 1-2 % to the shorter queue).
 * Never changes results. */
int avr_renderer_set_host_backpressure(avr_renderer *renderer, int mode);
/* How the classify pass and the march of this rank share the GPU is measured by the driver on
 * the running pipeline, unless fixed here and / or by avr_renderer_set_overlap: the candidates --
 * back to back on one stream, or side by side with an LDS reserve of 0, 2, 4 ... KiB per classify
 * workgroup (avr_context_set_classify_lds_reserve) -- are each held for a few frames whose
 * period is timed with HIP events on the march stream, and the best is kept (re-timed now and
 * then; searched again when it drifts).  bytes >= 0 fixes the reserve of the side-by-side mode,
 * -1 (default) leaves it to the driver.  Never changes results.
 * avr_renderer_corun_state: what the last frame used, whether the search has settled, and the
 * number of timed windows so far. */
int avr_renderer_set_classify_share(avr_renderer *renderer, int bytes);
int avr_renderer_corun_state(const avr_renderer *renderer, int *overlap_out,
                             int *reserve_bytes_out, int *settled_out, long *windows_out);
/* Whether the driver tightens the exchange layout (avr_frame_plan_tighten) of every plan it makes
 * (default 1; the 32 most recently used plans are kept, so a camera that repeats pays nothing).
 * The same on every rank.  Never changes results. */
int avr_renderer_set_tighten(avr_renderer *renderer, int enabled);
/* How the image is dealt to the ranks' pieces: AVR_PIECES_ROW_BANDS with bands of 8 rows by
 * default (the caller only sees the gathered image), AVR_PIECES_CONTIGUOUS for the reference's
 * partition.  band_rows: a power of two.  The same on every rank.  Never changes results. */
int avr_renderer_set_piece_layout(avr_renderer *renderer, int piece_layout, int band_rows);
int avr_renderer_reference_sample_distance(const avr_renderer *renderer, float *out);
/* Ranks of several, fail-fast and tuned as ONE system (round 4).
 * avr_renderer_set_plan_check (default 1): the first frame of a NEW plan (and the first after one
 *   of the setters the ranks must agree on) runs avr_frame_plan_agree over the communicator's
 *   control plane before anything is queued; ranks whose plans or settings differ all get
 *   AVR_ERR_RUNTIME there instead of hanging in the exchange.  0: no check (a caller whose camera
 *   never repeats and who vouches for its ranks).
 * avr_renderer_set_corun_coordination (default -1 = on for ranks of several): the co-run search
 *   (avr_renderer_set_classify_share) holds the same candidate on every rank in the same frames
 *   and decides on the MAXIMUM of the ranks' window periods (one 4-byte control-plane allgather
 *   per window, three frames after the window's last); the held candidate is re-timed every
 *   half second.  0: every rank searches on its own (round 3).  A run that wants no search at all
 *   fixes layout and reserve: avr_renderer_set_overlap + avr_renderer_set_classify_share.
 * avr_renderer_failure: NULL, or what did not finish within the deadline of
 *   avr_set_frame_timeout_ms (stream, rank, frame, stage, co-run state); the renderer is then
 *   failed: every call returns AVR_ERR_RUNTIME with that message, avr_renderer_destroy releases
 *   host memory only (device memory and streams of a hung GPU queue are left to process exit). */
/* avr_renderer_set_deferred_gather (default -1 = on for ranks of several; the same on every rank):
 *   the RGB8 pieces of frame f travel to rank 0 inside the grouped round of frame f + 1
 *   (avr_exchange_peers_gather) instead of in a gather round of their own -- ONE RCCL launch per
 *   frame.  Rank 0's rgb8_out of frame f is then complete when the compositing stream has passed
 *   the NEXT frame's round, or after avr_renderer_synchronize -- which, while such a gather is
 *   pending, runs it and is therefore collective (every rank synchronises after the same frame);
 *   the caller's rgb8_out buffer must stay valid until then.  Frames with want_image or
 *   antialiasing gather at once as before.  0: every frame gathers at once. */
int avr_renderer_set_deferred_gather(avr_renderer *renderer, int mode);
/* How a frame's two paint kernels are launched.  -1 / 1 (default): one launch each.  k in
 * [2, AVR_MAX_FRAME_CHUNKS]: every frame in k depth-ordered chunks, chunk i marched while chunk
 * i + 1 is classified (avr_classify_plan_chunked; only where the two kernels run on two streams,
 * never with a cached classification).  Built to shorten the frame of a caller who waits for every
 * frame -- the reference's call shape, one Render() per frame
 * (VolumeRenderer/VolumeRenderer.cpp:1103-1339) -- and measured not to on this GPU
 * (profiles/r5_latency/), hence off by default.  Scheduling only: never changes results. */
int avr_renderer_set_frame_chunks(avr_renderer *renderer, int chunks);
/* Occlusion culling (avr_render_plan_culled; one rank).  k in [2, AVR_MAX_FRAME_CHUNKS]: every
 * frame is classified and marched in k depth-ordered chunks on one stream, each classify launch
 * leaving out the boxes no ray can still sample (the reference's default boxTransparency = 0,
 * VolumeRenderer.hpp:36, saturates rays early).  -1 / 0 (default): never -- exact, but measured
 * not to pay on the configurations of BASELINE.json (profiles/r5_opaque/).  Never changes results. */
int avr_renderer_set_occlusion_culling(avr_renderer *renderer, int chunks);
int avr_renderer_last_frame_chunks(const avr_renderer *renderer); /* what the last frame took */
/* Visibility speculation (avr_classify_plan_positions / avr_march_plan_speculative; one rank).
 * -1 / 1 (default): the driver remembers, per box, the last frame whose rays sampled it (a march
 * that records the boxes it samples, the flags read on the host a few frames later); while at most
 * 85 % of the rank's boxes were sampled in the last 24 frames (and the classify work that saves is
 * worth 0.15 ms: not the short, march-bound frames of config-2 / config-3), a frame classifies only those, its
 * march checks every box it needs, and a repair pass (two gated launches that do nothing as a
 * rule) redoes the frame when the set was wrong -- the cells changed, the camera turned: results
 * never change.  The reference's default boxTransparency = 0: config-4's rays sample 58 of 176
 * boxes, the classify pass takes 0.18 instead of 0.55 ms, the frame 0.43 instead of 0.63.  A
 * translucent frame (every box sampled) is observed once and then left alone but for one observing
 * frame in 512; repairs in more than half of 32 frames suspend it (64 frames, doubling).
 * 0: never.
 * avr_renderer_speculation_state: state -1 off / 0 observing / 1 waiting for an observation /
 * 2 speculating / 3 not worth it (asleep) / 4 suspended after repairs; frames speculated and
 * repaired so far; the fraction of boxes in the present set (-1: nothing observed yet). */
int avr_renderer_set_visibility_speculation(avr_renderer *renderer, int mode);
int avr_renderer_speculation_state(const avr_renderer *renderer, int *state,
                                   int64_t *speculative_frames, int64_t *repaired_frames,
                                   float *sampled_fraction);
int avr_renderer_set_plan_check(avr_renderer *renderer, int mode);
/* One rank (default -1 = on): instead of timing every candidate of the co-run search, the driver
 * reads off each frame's two kernel durations which of the two is the longer one side by side and
 * bisects the LDS reserve to where they take equally long -- where the frame is shortest, because
 * the two trade one resource linearly (profiles/r5_corun_gap/) -- then holds it: some 100 frames
 * instead of 640.  Frames shorter than 0.35 ms, a held candidate that drifts, and mode 0 take the
 * full search.  Scheduling only. */
int avr_renderer_set_corun_balance(avr_renderer *renderer, int mode);
int avr_renderer_set_corun_coordination(avr_renderer *renderer, int mode);
const char *avr_renderer_failure(const avr_renderer *renderer);
/* One frame, asynchronously.  group_order: rank order of the compositing group, NULL = from the
 * visibility graph (VolumeRenderer.cpp:1235-1241).  input_stream: a HIP stream whose queued work
 * produces the cell data (or zeroes samples_out); the classify pass, and with it the march, is
 * ordered after it.  NULL means "nothing to wait for", NOT the legacy default stream (whose handle
 * is 0 as well): the driver's streams are non-blocking and never order themselves after that one
 * implicitly, so a caller that fills cells on the default stream passes AVR_DEFAULT_STREAM.
 * samples_out (device, may be NULL) as avr_paint_box.  want_image (the SAME on every rank: it
 * adds a gather of the float pieces): also deliver the gathered -- with antialiasing downsampled
 * and overlaid -- depth-sort image.  On rank 0: rgb8_out (device, width*height*3 bytes, rows
 * top-down = the output file's pixel bytes, required) and, with want_image, image_out (device,
 * width*height*5 floats, origin bottom-left).  Other ranks pass NULL for both.  The outputs are
 * complete when the compositing stream (avr_renderer_stream(r, 2)) reaches this point:
 * avr_renderer_synchronize, or order your stream after it -- for ranks of several the RGB8 bytes
 * of a frame without want_image arrive one frame later (avr_renderer_set_deferred_gather). */
#define AVR_DEFAULT_STREAM ((void *)(intptr_t)-1) /* input_stream: the legacy default (null) stream */
int avr_renderer_render(avr_renderer *renderer, const avr_render_params *render,
                        const avr_camera *camera, const int32_t *group_order, void *input_stream,
                        uint64_t *samples_out, int want_image, uint8_t *rgb8_out, float *image_out);
/* A maximum-intensity frame (avr_paint_box_max over the whole scene): classify pass, MIP march
 * (avr_march_plan_max), the same exchange, the max fold (avr_fold_plan_own_max), the same gather.
 * rgb8_out as avr_renderer_render: the colour of the pixel's largest index, (0,0,0) where no box
 * takes a sample, rows top-down.  index_out (may be NULL; rank 0 only, NULL elsewhere):
 * width*height int16 indices, -1 for none, in image_out's order (row 0 at the bottom); for N > 1
 * the indices are gathered to rank 0 in every MIP frame.  Same completion rules as
 * avr_renderer_render (a MIP frame's bytes are never deferred).  Frame chunks, occlusion culling
 * and visibility speculation (which rest on opacity) are not used and not fed; the classified
 * volume and its cache are shared with volume frames, which may alternate with MIP frames.
 * render->antialiasing > 1 or draw_bounds: AVR_ERR_INVALID_ARGUMENT. */
int avr_renderer_render_max(avr_renderer *renderer, const avr_render_params *render,
                            const avr_camera *camera, const int32_t *group_order, void *input_stream,
                            uint64_t *samples_out, uint8_t *rgb8_out, int16_t *index_out);
/* A column-projection frame (avr_paint_box_projection over the whole scene): the projection march
 * (avr_march_plan_projection, no classify pass), the same exchange, the sum fold
 * (avr_fold_plan_own_projection), and a gather of the f64 pieces to rank 0.  column_out and
 * length_out (rank 0: required; NULL elsewhere): width*height f64 each, row 0 at the bottom.
 * samples_out: as avr_renderer_render (every sample, finite or not).  The frame neither reads nor
 * invalidates the classified volume or its cache, and does not feed or consult the co-run balance,
 * speculation, frame chunks or occlusion culling; volume and MIP frames may alternate with it.
 * It is ordered behind the frames queued before it on the renderer's streams.  The march reads
 * the caller's cells on the march stream after input_stream's work (as avr_renderer_render): they
 * must stay unchanged until the frame is complete on the compositing stream
 * (avr_renderer_synchronize).  render->antialiasing > 1 or draw_bounds: AVR_ERR_INVALID_ARGUMENT. */
int avr_renderer_render_projection(avr_renderer *renderer, const avr_render_params *render,
                                   const avr_camera *camera, const int32_t *group_order,
                                   void *input_stream, uint64_t *samples_out, double *column_out,
                                   double *length_out);
/* Plans a frame ahead of time: makes the frame plan of (render, camera, group_order) -- visibility
 * order (VolumeRenderer.cpp:1235-1241), global layer order and exchange layout
 * (DirectSendBase.cpp:400-446), for N > 1 tightened to the runs' per-row extents -- and keeps it
 * with the renderer's plans, where avr_renderer_render finds it.  Host geometry only (0.1 ms for
 * 176 boxes at N = 8, which is most of what a rank's 0.15 ms frame leaves the host): a caller whose
 * camera never repeats (a scripted fly-through) calls it for frame f + 1 on ANOTHER thread while
 * frame f is being queued.  Safe beside avr_renderer_render / avr_renderer_synchronize of the same
 * renderer; not beside its setters or avr_renderer_destroy.  Calling it is never required and never
 * changes results. */
int avr_renderer_prepare(avr_renderer *renderer, const avr_render_params *render,
                         const avr_camera *camera, const int32_t *group_order);
int avr_renderer_synchronize(avr_renderer *renderer);
/* How many of the frames rendered so far have their outputs (rgb8_out, image_out) written once the
 * compositing stream (avr_renderer_stream(r, 2)) has passed everything queued up to now: all of
 * them, or -- ranks of several with the deferred gather -- all but the last.  A caller that orders
 * its own stream after the compositing stream reads frame `*complete_out - 1` and older; the last
 * frame's bytes follow with the next frame's round or with avr_renderer_synchronize.  frames_out
 * (may be NULL): frames rendered so far. */
int avr_renderer_outputs_complete(const avr_renderer *renderer, uint64_t *complete_out,
                                  uint64_t *frames_out);
/* which: 0 classify, 1 march, 2 exchange / fold / gather / tail (hipStream_t as void*). */
void *avr_renderer_stream(avr_renderer *renderer, int which);
/* The plan of the last frame rendered (runs, piece, exchange volume). */
int avr_renderer_plan_info(const avr_renderer *renderer, avr_frame_plan_info *out);
/* Kernel timing for the benchmark: while enabled every frame records HIP events around its
 * classify pass and its march on the streams they are launched on.  avr_renderer_timings drains
 * the streams and returns the averages per frame since timing was enabled: each kernel's own
 * duration and the length of the union of their execution intervals (they overlap by design). */
/* Host seconds spent inside avr_renderer_render since the last reset, by section: plan,
 * classify call, march call, exchange, fold (+ piece overlay), gather + frame tail; and the number
 * of frames they cover.  (A host that runs ahead of the GPU waits inside these calls for a staging
 * slot: under back-pressure the sum approaches the GPU's frame time.) */
int avr_renderer_host_profile(avr_renderer *renderer, double seconds_out[6], long *frames_out,
                              int reset);
int avr_renderer_set_timing(avr_renderer *renderer, int enabled);
int avr_renderer_timings(avr_renderer *renderer, double *classify_ms, double *march_ms,
                         double *busy_ms, int *frames);

/* ---- visibility ordering ------------------------------------------------ */

/* BuildVisibilityOrderedGroup (Common/VisibilityOrdering.cpp:63-632; called from
 * VolumeRenderer/VolumeRenderer.cpp:1235-1241): the order of the ranks in the MPI group handed to
 * Compositor::compose, from a topological sort of the face-adjacency graph of all boxes oriented
 * by the view direction (cycles are broken by splitting a box).  Host only.
 *
 * The graph object holds the replicated box metadata (what the reference allgathers every
 * frame: corners as floats and owners, rank-major) and the camera-independent list of
 * face-adjacent pairs.  owner[b] = owning rank of all_boxes[b]; the relative order of a rank's
 * boxes is their localBoxes order. */
typedef struct avr_visibility_graph avr_visibility_graph;
int avr_visibility_graph_create(const avr_box *all_boxes, const int32_t *owner, int n_boxes,
                                int n_ranks, avr_visibility_graph **out_graph);
void avr_visibility_graph_destroy(avr_visibility_graph *graph);

/* rank_order_out[n_ranks] = rank at each position of the ordered group.
 * use_visibility_graph == 0 or a failed ordering yields the default order 0..n-1
 * (*succeeded_out = 0 on failure, where the reference prints its warning).  aspect = width /
 * height as float (VolumeRenderer.cpp:1114).  dot_prefix (may be NULL): every graph iteration is
 * also written to "<dot_prefix><counter>.dot" in the reference's format
 * (writeVisibilityGraph, VisibilityOrdering.cpp:318-350; the reference's prefix is
 * "visibility_graph_", written by rank 0).  n_splits_out (may be NULL): boxes split to break
 * cycles. */
int avr_visibility_order(avr_visibility_graph *graph, const avr_camera *camera, float aspect,
                         int use_visibility_graph, const char *dot_prefix,
                         int32_t *rank_order_out, int *succeeded_out, int *n_splits_out);

/* ---- wireframe overlay ------------------------------------------------- */

/* computeTightBounds (VolumeRenderer/VolumeRenderer.cpp:791-848) over the (replicated) box
 * metadata: component-wise min / max of the corners, rounded to float as the reference's
 * MPI_FLOAT reduction does; the fallback bounds when there is no box.  Host only. */
int avr_tight_bounds(const avr_box *all_boxes, int n_boxes, const double fallback_min[3],
                     const double fallback_max[3], double out_min[3], double out_max[3]);

/* renderBoundingBoxLayer (VolumeRenderer/VolumeRenderer.cpp:139-335): white anti-aliased
 * wireframe of [bounds_min, bounds_max] blended, in the reference's edge order, over the pixels
 * [pixel_begin, pixel_end) of a width x height depth-sort image (image = those pixels, 5 floats
 * each, in place).  Pixels are independent, so a rank can overlay its own piece.  If rgb8 is
 * non-NULL the overlaid pixels are also written as RGB8 (3 bytes per pixel, same order). */
int avr_bbox_overlay(avr_context *ctx, const double bounds_min[3], const double bounds_max[3],
                     const avr_camera *camera, int sqrt_antialiasing, int width, int height,
                     int64_t pixel_begin, int64_t pixel_end, float *image, uint8_t *rgb8);
/* The same on this rank's piece of a frame plan (either piece layout): piece = the piece's pixels
 * as avr_fold_plan delivers them, rgb8 (may be NULL) its 8-bit twin. */
int avr_bbox_overlay_piece(avr_context *ctx, const avr_frame_plan *plan, const double bounds_min[3],
                           const double bounds_max[3], const avr_camera *camera, float *piece,
                           uint8_t *rgb8);
/* Gathered pieces (piece-major: piece 0's pixels, then piece 1's, ... as avr_gather delivers them)
 * -> the image in row order; flip != 0: rows top-down (the output file's order; pieces hold the
 * bottom-up image of the renderer).  With contiguous pieces the gathered buffer already is the
 * image, so this is a (flipped) copy -- avr_flip_rows generalised to AVR_PIECES_ROW_BANDS. */
int avr_assemble_rows(avr_context *ctx, const avr_frame_plan *plan, const void *gathered,
                      int bytes_per_pixel, int flip, void *image);
/* The same with this rank's own piece read where its fold wrote it (own_piece, device) instead of
 * from the gathered buffer: the root of a gather with skip_own saves a device copy per frame.  With
 * contiguous pieces only if the pieces are whole rows. */
int avr_assemble_rows_own(avr_context *ctx, const avr_frame_plan *plan, const void *gathered,
                          const void *own_piece, int bytes_per_pixel, int flip, void *image);

/* ---- scene statistics -------------------------------------------------- */

/* reduceLocalScalarStats (VolumeRenderer/SceneBuilder.cpp:53-97) over the scene's boxes: one
 * streaming pass.  stats_host[0..2] = min, max, min positive over the finite cells (+inf, -inf,
 * +inf when there is none), *finite_count_host = their number.  Synchronises the stream. */
int avr_scene_scalar_stats(avr_context *ctx, const avr_scene *scene, double stats_host[3],
                           int64_t *finite_count_host);

/* The scalar-transform part of BuildSceneGeometry (SceneBuilder.cpp:315-443) from statistics
 * already reduced over all ranks (host only): positive floor / processed range for log
 * scaling, normalisation to the data range (SetSceneNormalizationRange, :427-443).
 * processed[2] = processed min/max in double, processed_range / scalar_range as the float
 * pairs of SceneGeometry.  AVR_ERR_RUNTIME where the reference throws std::runtime_error. */
int avr_scene_transform_from_stats(const double stats[3], int64_t finite_count, int log_scale,
                                   int normalize_to_data_range, avr_scalar_transform *transform,
                                   double processed[2], float processed_range[2],
                                   float scalar_range[2]);

/* The binning of ComputeSceneHistogram (SceneBuilder.cpp:445-577): every cell of the scene is
 * transformed, clamped to [range_min, range_max] and counted; counts_dev[bin_count] (device,
 * uint64) is ADDED to (the caller zeroes it and sums over ranks). */
int avr_scene_histogram(avr_context *ctx, const avr_scene *scene,
                        const avr_scalar_transform *transform, float range_min, float range_max,
                        int bin_count, uint64_t *counts_dev);

/* ---- joint histogram of two raw fields ("Phase plot and profile") --------------- */

/* Joint histogram of the raw f64 cells of scene_x and scene_y, per AMR level, with the cells of
 * scene_s summed per bin.  scene_y may be NULL (one y bin: ny must be 1, y_edges is not read) and
 * so may scene_s (sums_dev is not written).  The scenes belong to ctx and hold the same box list:
 * the same number of boxes and, per position, the same dims and level -- the cells at one
 * (box, i, j, k) are one cell's values of the fields; each scene keeps its own strides.
 * x_edges[nx + 1] and y_edges[ny + 1] (host) are finite and strictly increasing, 1 <= nx, ny <=
 * 1024, nx * ny <= 2^20.  A value v lies in bin i when e[i] <= v < e[i + 1]; the last bin is
 * closed at the top (v == e[n] lies in bin n - 1).  The bin is decided by f64 comparisons against
 * the edges as given, nothing else.  Per cell, in this order:
 *   vx, vy or vs not finite            totals[1] += 1   (nonfinite)
 *   vx or vy outside [e[0], e[n]]      totals[0] += 1   (outside)
 *   otherwise, l = the box's level     cells[(l * ny + by) * nx + bx] += 1,
 *                                      sums [(l * ny + by) * nx + bx] += vs
 * with no transform and no normalisation.  0 <= level < n_levels <= 16 for every box.
 * cells_dev (uint64 [n_levels][ny][nx]), sums_dev (f64, the same shape) and totals_dev (uint64
 * [2]) are device arrays that are ADDED to (the caller zeroes them and sums over ranks).  Counts
 * are exact; a sum is made of f64 additions in no fixed order.  Everything is checked on the host
 * before any device work: AVR_ERR_INVALID_ARGUMENT leaves the outputs untouched.  Asynchronous
 * on the context's stream. */
int avr_scene_joint_histogram(avr_context *ctx, const avr_scene *scene_x, const avr_scene *scene_y,
                              const avr_scene *scene_s, const double *x_edges, int nx,
                              const double *y_edges, int ny, int n_levels, uint64_t *cells_dev,
                              double *sums_dev, uint64_t *totals_dev);

/* ---- slice images of the raw field ("Slice") ------------------------------------ */

/* A plane through the scene: pixel (x, y), row 0 at the bottom, samples the point
 *   P[a] = (origin[a] + (x + 0.5) * du[a]) + (y + 0.5) * dv[a]      (binary64, nothing fused)
 * in the scene's coordinates.  A box contains P when min_corner[a] <= P[a] < max_corner[a] on all
 * three axes; the scene's boxes must be disjoint (the first that contains P is taken).  In it the
 * cell is i_a = min(int(floor((P[a] - min[a]) / (max[a] - min[a]) * dims[a])), dims[a] - 1), and
 *   value[p] = cells[i + j*jstride + k*kstride] as it is (NaN and Inf included), 0.0 on a miss,
 *   level[p] = the box's level (0..127), -1 on a miss,
 *   box[p]   = global_index[b] of the scene's box b (host array, one per box of the scene; null:
 *              b itself), -1 on a miss,
 * p = y * width + x; all three on the device.  No transform, no classified volume.  Asynchronous
 * on the context's stream. */
int avr_slice_scene(avr_context *ctx, const avr_scene *scene, const double origin[3],
                    const double du[3], const double dv[3], int width, int height,
                    const int32_t *global_index, double *value, int8_t *level, int32_t *box);

/* Box outlines of a slice: every pixel of `box` (avr_slice_scene's, row 0 at the bottom) whose
 * entry differs from that of its right or its upper neighbour -- the last column has no right
 * neighbour, the top row no upper one -- gets (red, green, blue) in rgb8 (width*height*3 bytes,
 * device, rows top-down as avr_projection_colorize writes them); other pixels are left alone. */
int avr_slice_outline(avr_context *ctx, const int32_t *box, int width, int height, int red,
                      int green, int blue, uint8_t *rgb8);

/* ---- on-axis projections of the raw field ("On-axis projection") ---------------- */

/* The line integral along axis (0 = x, 1 = y, 2 = z) of the raw f64 cells of scene_f, cell by
 * cell, optionally weighted by the cells of scene_w (NULL: no weight).  The scenes belong to ctx
 * and hold the same box list as avr_scene_joint_histogram requires; each keeps its own strides.
 * The image axes (U, V) are (y, z), (z, x), (x, y).  Pixel (x, y), row 0 at the bottom, owns the
 * line u = origin_uv[0] + (x + 0.5) * du, v = origin_uv[1] + (y + 0.5) * dv (binary64, nothing
 * fused) in the scene's coordinates.  Box b contains it when min[U] <= u < max[U] and min[V] <=
 * v < max[V]; EVERY such box contributes the column of its dims[axis] cells at
 * i_U = min(int(floor((u - min[U]) / (max[U] - min[U]) * dims[U])), dims[U] - 1), i_V likewise:
 *   without scene_w, per cell with vf finite:         S += vf,      n += 1
 *   with scene_w, per cell with vf and vw finite:     S += vf * vw, Wt += vw, n += 1
 * and, with dl = level_dl[the box's level] (host, n_levels <= 16 finite entries),
 *   integral[p] = sum_b dl * S_b,  weight[p] = sum_b dl * Wt_b,  length[p] = sum_b dl * f64(n_b),
 * p = y * width + x, f64 on the device, all 0 where no box contains the line; weight_dev is given
 * exactly when scene_w is.  The outputs are overwritten.  The f64 additions of a column run in an
 * order fixed by the box's dims and the axis, the boxes are added in ascending index and no
 * atomic touches an output: equal arguments give equal bits.  Everything is checked on the host
 * before any device work: AVR_ERR_INVALID_ARGUMENT leaves the outputs untouched.  Asynchronous on
 * the context's stream; the context keeps the per-box partial planes (grow-only scratch). */
int avr_scene_axis_projection(avr_context *ctx, const avr_scene *scene_f, const avr_scene *scene_w,
                              int axis, const double origin_uv[2], double du, double dv, int width,
                              int height, const double *level_dl, int n_levels,
                              double *integral_dev, double *weight_dev, double *length_dev);

/* ---- derived fields ("Derived fields") -------------------------------------------- */

/* A new field from a per-cell program over up to six fields of the same cells.  `inputs` are
 * n_inputs (0..6) scenes of ctx and `out` a scene of ctx over cells the caller allocated, all with
 * the same box list as avr_scene_joint_histogram requires (equal dims and levels; each keeps its own
 * strides); the cells of out's boxes are overwritten.  The program is postfix, one word per
 * instruction (1..64): opcode in the low byte, operand index in the bits above it.
 *   0 CONST c   push constants[c] (n_constants <= 16)     1 FIELD f   push the cell of inputs[f]
 *   2 BUILTIN b push 0 x, 1 y, 2 z, 3 dx, 4 dy, 5 dz, 6 cell_volume, 7 level
 *   3 ADD  4 SUB  5 MUL  6 DIV   a b -> a op b            7 NEG  8 SQUARE (a * a)  9 SQRT  10 ABS
 *   11 MIN  a b -> (a < b || a != a) ? a : b              12 MAX  a b -> (a > b || a != a) ? a : b
 *   13 LT  14 LE  15 GT  16 GE  17 EQ  18 NE   a b -> 1.0 or 0.0 (with a NaN: 0.0, NE 1.0)
 *   19 WHERE  c a b -> (c != 0.0) ? a : b (a NaN c selects a)
 * Everything is binary64, round to nearest, nothing fused, denormals kept; DIV and SQRT are
 * correctly rounded.  With (dx, dy, dz) = level_cell_size[3 * level .. ] (host, n_levels <= 16) of
 * the box's level and origin = box_origin[3 * b ..] (host) of box b, cell (i, j, k) of the box has
 * x = origin[0] + (f64(i) + 0.5) * dx (a multiply, then an add), y and z likewise, cell_volume =
 * (dx * dy) * dz and level = f64(the box's level).  The stack holds at most 8 values.
 * Everything is checked on the host before any device work: AVR_ERR_INVALID_ARGUMENT for counts
 * over the limits, an unknown opcode, an operand index out of range, a program that underflows
 * the stack, goes deeper than 8 or does not end with exactly one value, scenes that are not
 * congruent with `out`, a box level >= n_levels, n_levels > 16, origins or cell sizes that are not
 * finite, and an output box whose cells overlap an input box's cells -- and `out` is untouched.
 * Asynchronous on the context's stream; invalidates out's cached classification. */
int avr_scene_derive(avr_context *ctx, const avr_scene *const *inputs, int n_inputs, avr_scene *out,
                     const uint32_t *instructions, int n_instructions, const double *constants,
                     int n_constants, const double *box_origin, const double *level_cell_size,
                     int n_levels);

/* ---- gradient fields ("Gradient fields") ------------------------------------------ */

/* The difference of the raw f64 cells of `in` along axis (0 = x, 1 = y, 2 = z), per cell, written
 * to `out`: scenes of ctx with the same box list as avr_scene_joint_histogram requires (equal dims
 * and levels; each keeps its own strides), `out` over cells the caller allocated.  The boxes are
 * the leaves of an AMR hierarchy: box b of level l starts at the integer index box_index_lo[3 * b
 * ..] (host) of level l's index space, level_ratio[l] >= 2 (host, n_levels - 1 entries) refines
 * level l to l + 1 (an index maps down by floor division, a cell's children are r * G + (0 .. r -
 * 1)^3) and level_cell_size[l] (host, n_levels <= 16) is a cell's size along the axis.  A cell's
 * neighbour on either side is the next cell of its box or, past the box's face, the ghost G (a
 * level-l index): the cell of the box of the highest level m <= l that contains G mapped to level
 * m; else (0.0 + the r^3 children of G, added in ascending k, then j, then i) / f64(r^3) if every
 * child lies in a box of level l + 1; else the neighbour is absent.  With own value f, low
 * neighbour L and high neighbour H:  both (H - L) / (2.0 * dx); only H (H - f) / dx; only L
 * (f - L) / dx; neither 0.0 -- binary64, round to nearest, nothing fused, the division correctly
 * rounded; non-finite values propagate.  Only the cells of the scene's boxes are read, never the
 * rest of an allocation a box is a view of.  No atomics: equal arguments give equal bits.
 * Everything is checked on the host before any device work: AVR_ERR_INVALID_ARGUMENT for an axis
 * outside 0..2, scenes that are not congruent, a box level >= n_levels, n_levels > 16, a ratio
 * below 2, a cell size that is not finite and positive, a box index range outside [-2^30, 2^30),
 * an output box whose cells share a byte with an input box's, and two boxes of one level that
 * overlap in index space -- and `out` is untouched.  Asynchronous on the context's stream; the
 * context keeps the face planes (grow-only scratch); invalidates out's cached classification. */
int avr_scene_gradient(avr_context *ctx, const avr_scene *in, avr_scene *out, int axis,
                       const int32_t *box_index_lo, const int32_t *level_ratio,
                       const double *level_cell_size, int n_levels);

/* ---- clumps ("Clumps") ------------------------------------------------------------ */

/* The connected components ("clumps") of the cells of `in` whose raw f64 value v satisfies
 * v >= lower && v <= upper (no transform; a NaN is never selected, +Inf only by upper = +Inf, -Inf
 * only by lower = -Inf), labelled into `out`: scenes of ctx with the same box list as
 * avr_scene_gradient requires, `out` over cells the caller allocated, and the same hierarchy
 * description (box_index_lo, level_ratio, n_levels <= 16; host).  Two selected cells are adjacent
 * if they are face neighbours inside a box, or if one is the cell found for the other's ghost:
 * past a box's face the ghost G (a level-l index) is mapped to levels m = l, l - 1, ..., 0 by
 * floor division and the first level-m box that contains the mapped index gives the neighbour; a
 * finer neighbour is never searched for (it finds the coarse cell from its own side), and a ghost
 * no such box contains has no neighbour there.  A cell's ordinal is cell_begin[b] + (k * ny + j) *
 * nx + i, cell_begin the prefix sum of nx * ny * nz over the scene's boxes in scene order; clumps
 * are numbered 1..N in ascending order of their smallest ordinal.  `out` gets f64(label) for a
 * selected cell and +0.0 otherwise, *count_dev (device) gets N.  Only the cells of the scene's
 * boxes are read, never the rest of an allocation a box is a view of.  The numbering is canonical:
 * equal arguments give equal bits, whatever order the atomics inside resolve in.
 * Everything is checked on the host before any device work: AVR_ERR_INVALID_ARGUMENT for a NaN
 * bound or lower > upper, n_levels outside [1, 16], scenes that are not congruent, a box level >=
 * n_levels, a ratio below 2, a box index range outside [-2^30, 2^30), two boxes of one level that
 * overlap in index space, an output box whose cells share a byte with an input box's, and 2^31
 * cells or more ("scene has too many cells for 32-bit labels") -- and `out` and *count_dev are
 * untouched.  Asynchronous on the context's stream; the context keeps 4 bytes per cell of
 * grow-only scratch; invalidates out's cached classification. */
int avr_scene_clumps(avr_context *ctx, const avr_scene *in, avr_scene *out, double lower,
                     double upper, const int32_t *box_index_lo, const int32_t *level_ratio,
                     int n_levels, uint64_t *count_dev);

/* The table of a label field: for every cell of `labels` (a scene of ctx, as avr_scene_clumps
 * writes one; any f64 cells are taken), in this order: a label whose bits are +0.0 is skipped; a
 * label that is not an integer in [1, n_clumps] adds 1 to totals_dev[0]; with `field` (a scene of
 * ctx with the same box list, or NULL) a field value vs that is not finite adds 1 to
 * totals_dev[1]; otherwise cells_dev[l * n_clumps + label - 1] += 1 (uint64) for the box's level
 * l and, with a field, sums_dev[the same entry] += vs (f64).  cells_dev and sums_dev (NULL exactly
 * when field is) are [n_levels][n_clumps] on the device, totals_dev two uint64; all are added to,
 * as avr_scene_joint_histogram's are.  Counts are exact; a sum is made of f64 additions in no
 * fixed order.  AVR_ERR_INVALID_ARGUMENT, before any device work and with the outputs untouched:
 * n_clumps < 1, n_levels outside [1, 16], n_clumps * n_levels >= 2^28, scenes that are not
 * congruent, a box level >= n_levels.  Asynchronous on the context's stream. */
int avr_scene_clump_table(avr_context *ctx, const avr_scene *labels, const avr_scene *field,
                          uint64_t n_clumps, int n_levels, uint64_t *cells_dev, double *sums_dev,
                          uint64_t *totals_dev);

/* The links and extents of a label field ("Clump tree").  `labels` is a label scene
 * of ctx as avr_scene_clumps writes one, `parents` (or NULL) the label scene of a selection that
 * contains it -- the same field over a lower threshold -- with the same box list; box_index_lo,
 * level_ratio and n_levels as avr_scene_clumps takes them.  With R_l = ratio[l] * ... *
 * ratio[n_levels - 2] (R of the last level is 1), a cell of level l whose index in its level is
 * (I, J, K) covers [I R_l, (I + 1) R_l - 1] per axis in the index space of level n_levels - 1.
 * For every cell, in this order: a label whose bits are +0.0 is skipped; a label that is not an
 * integer in [1, n_clumps] adds 1 to totals_dev[0] and the cell is done; with `parents`, a parent
 * label that is not an integer in [1, n_parents] (+0.0 and NaN included) adds 1 to totals_dev[1]
 * and the cell contributes nothing; otherwise, with c the label and p the parent label,
 * extent_dev[a * n_clumps + c - 1] = min(., low end along axis a), extent_dev[(3 + a) * n_clumps +
 * c - 1] = max(., high end) (int32 [6][n_clumps]) and, with `parents`, parent_lo_dev[c - 1] =
 * min(., p), parent_hi_dev[c - 1] = max(., p) (uint32 [n_clumps], NULL exactly when parents is).
 * Every output is combined into, never initialised: start lows and parent_lo at the type's
 * maximum, highs at INT32_MIN, parent_hi and totals_dev (two uint64, added to) at 0.  All results
 * are minima and maxima of integers: exact, equal bits for equal arguments.
 * AVR_ERR_INVALID_ARGUMENT, before any device work and with the outputs untouched, in this
 * order: n_clumps outside [1, 2^28); n_parents outside [1, 2^28) with parents, not 0 without;
 * n_levels outside [1, 16]; the box rules on the labels; a ratio below 2; an index range that
 * leaves [-2^30, 2^30); a refined index range, I R_l .. (I + n) R_l - 1, that leaves it; scenes
 * that are not congruent.  Nothing is launched for a scene without cells.  Asynchronous on the
 * context's stream. */
int avr_scene_clump_links(avr_context *ctx, const avr_scene *labels, const avr_scene *parents,
                          uint64_t n_clumps, uint64_t n_parents, const int32_t *box_index_lo,
                          const int32_t *level_ratio, int n_levels, int32_t *extent_dev,
                          uint32_t *parent_lo_dev, uint32_t *parent_hi_dev, uint64_t *totals_dev);

/* The member cells of the wanted clumps of a label field ("Clump binding").
 * `labels` is a label scene of ctx as avr_scene_clumps writes one; wanted_dev holds one byte per
 * label, wanted_dev[c - 1].  For every cell, in this order: a label whose bits are +0.0 is
 * skipped; a label that is not an integer in [1, n_clumps] adds 1 to totals_dev[0] (one uint64,
 * added to); a cell whose label c has wanted_dev[c - 1] != 0 is a member, and its key is
 * (c - 1) << 32 | ordinal with the cell ordinals of avr_scene_clumps: the cells of the boxes in
 * scene order, (k ny + j) nx + i inside a box.  A member takes the next free slot s of
 * count_dev[0] (one uint64, cleared by the call) and writes keys_dev[s] if s < capacity: the keys
 * arrive in no fixed order -- sorted ascending they are the canonical list, by label and then by
 * ordinal -- and nothing is written at or past keys_dev[capacity].  count_dev[0] ends as the
 * number of members, whatever the capacity.  AVR_ERR_INVALID_ARGUMENT, before any device work and
 * with the outputs untouched, in this order: n_clumps outside [1, 2^28); capacity outside
 * [1, 2^31); the box rules (a level in [0, 16)); 2^31 cells or more.  Nothing is launched for a
 * scene without cells.  Asynchronous on the context's stream. */
int avr_scene_clump_members(avr_context *ctx, const avr_scene *labels, uint64_t n_clumps,
                            const uint8_t *wanted_dev, uint64_t capacity, uint64_t *keys_dev,
                            uint64_t *count_dev, uint64_t *totals_dev);

/* What is looked up per member key.  The low 32 bits of keys_dev[n] (n < n_members) are a cell
 * ordinal of `scene` (a scene of ctx; only its boxes' dims and levels are used).  With
 * centres_dev and levels_dev (given together or both NULL): levels_dev[n] = the level of the
 * cell's box and centres_dev[a * n_members + n] = prob_lo[a] + (f64(I_a) + 0.5) * dx_l[a] -- one
 * addition, one multiplication, one addition, unfused -- where I_a = box_index_lo[b][a] + the
 * cell's index along axis a in its box.  With `field` (a scene of ctx with the same box list) and
 * values_dev (given together or both NULL): values_dev[n] = the raw f64 value of that cell of the
 * field.  An ordinal that names no cell of the scene reads nothing and gives level 255 and NaNs.
 * box_index_lo, level_ratio, level_cell_size, prob_lo and n_levels as avr_scene_isosurface takes
 * them.  AVR_ERR_INVALID_ARGUMENT, before any device work and with the outputs untouched: no
 * output group asked for, or half of one; then in this order: n_members >= 2^31; n_levels outside
 * [1, 16]; a NULL array; the box rules and scenes that are not congruent; 2^31 cells or more; a
 * ratio below 2; an index range that leaves [-2^30, 2^30); a cell size that is not finite and
 * positive, an origin that is not finite.  Nothing is launched for n_members == 0.  Asynchronous
 * on the context's stream. */
int avr_scene_clump_member_data(avr_context *ctx, const avr_scene *scene, const uint64_t *keys_dev,
                                uint64_t n_members, const avr_scene *field, double *values_dev,
                                const int32_t *box_index_lo, const int32_t *level_ratio,
                                const double *level_cell_size, const double *prob_lo,
                                int n_levels, double *centres_dev, uint8_t *levels_dev);

/* The self-energy of member segments by direct summation ("Clump binding").  Segment
 * s holds the members offsets_host[s] .. offsets_host[s + 1] - 1 of the device arrays x_dev,
 * y_dev, z_dev (centres) and m_dev (masses, >= 0); w_dev[s] = sum over its pairs i < j of
 * m_i m_j / r_ij, r_ij = sqrt((dx dx + dy dy) + dz dz), every operation IEEE binary64, correctly
 * rounded and unfused; +0.0 for a segment of fewer than two members.  Two members at one point
 * divide by zero as IEEE does.  The sum is taken in an order that the offsets alone fix: equal
 * arguments give equal bits, and no term passes through more than depth_host[s] rounded additions
 * (int64 [n_segments] on the host, or NULL; 0 for a segment without pairs; never more than the
 * segment's members + 64).  The partial sums live in a grow-only scratch block of the context.
 * AVR_ERR_INVALID_ARGUMENT, before any device work and with the outputs untouched, in this order:
 * offsets that do not ascend from 0; a segment of more than 2^22 members; 2^31 members or more;
 * n_segments >= 2^28; 2^26 work items or more (an item is one row of 256 members against at most
 * 64 * 256 others: a segment of N members makes about N^2 / 2^23 + N / 2^9 of them, 2.1 M at
 * N = 2^22, so a call takes 31 such segments).  Nothing is launched for n_segments == 0.  Asynchronous on the context's
 * stream. */
int avr_clump_pair_energy(avr_context *ctx, const int64_t *offsets_host, uint64_t n_segments,
                          const double *x_dev, const double *y_dev, const double *z_dev,
                          const double *m_dev, double *w_dev, int64_t *depth_host);

/* ---- isosurfaces ("Isosurface") --------------------------------------------------- */

/* The isosurface field == value of `field` (a scene of ctx; raw f64 cells, no transform) by
 * marching tetrahedra, as a triangle soup in a canonical order.  A cube has the centres of eight
 * cells of one level l as corners, C + (di, dj, dk) with corner number c = di + 2 dj + 4 dk; the
 * value at a level-l index G is that of the level-m box, m = l, l - 1, ..., 0, that contains G
 * mapped to level m by floor division (the first hit wins; finer cells are never searched), and a
 * G no such box contains is absent.  A corner always sits at prob_lo[d] + (f64(G[d]) + 0.5) *
 * level_cell_size[l][d].  A cube is a surface cube iff every corner is present and one at least
 * lies in a level-l box; it belongs to the box that holds its lowest-numbered such corner.  A
 * surface cube with a non-finite corner emits nothing and counts as skipped.  Each cube is split
 * into the six tetrahedra (0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7); a corner
 * is inside iff v >= value; a tetrahedron with one or three inside vertices emits one triangle,
 * with two the quad as two; the normal (v1 - v0) x (v2 - v0) points to the v < value side.  A
 * vertex on the edge from L (v_L < value) to H is P_L + t (P_H - P_L), t = (value - v_L) / (v_H -
 * v_L), IEEE binary64 with nothing fused; with `sample` (a scene of ctx with the same box list,
 * or NULL) its sample value is s_L + t (s_H - s_L).  Triangles are ordered by owner box in scene
 * order, then by cube base k, j, i ascending over [-1, n - 1], then tetrahedron, then triangle:
 * equal arguments give equal bits.  The hierarchy description (box_index_lo, level_ratio,
 * n_levels <= 16; host) is avr_scene_gradient's; level_cell_size holds (dx, dy, dz) per level,
 * prob_lo three values (host).
 * counts_dev (device, two uint64) always gets T, the number of triangles, and the number of
 * skipped cubes.  Iff T <= capacity the triangles are written: vertices_dev f64 [T][3][3],
 * levels_dev u8 [T] (the owner box's level) and, with sample, samples_dev f64 [T][3]; the arrays
 * hold `capacity` triangles.  capacity == 0 is the count-only call: the three arrays are not
 * looked at and may be NULL.
 * Everything is checked on the host before any device work: AVR_ERR_INVALID_ARGUMENT for a value
 * that is not finite, n_levels outside [1, 16], a cell size that is not finite and positive, a
 * prob_lo that is not finite, capacity >= 2^36, samples_dev given without sample or the reverse,
 * scenes that are not congruent, a box level >= n_levels, a ratio below 2, a box index range
 * outside [-2^30, 2^30), two boxes of one level that overlap in index space, an output array that
 * shares a byte with an input box's cells, and 2^31 cube bases or more -- and every output is
 * untouched.  Asynchronous on the context's stream; the context keeps grow-only scratch (9 or 17
 * bytes per cell of the boxes' ghost shells, 16 bytes per 1024 cube bases). */
int avr_scene_isosurface(avr_context *ctx, const avr_scene *field, const avr_scene *sample,
                         double value, const int32_t *box_index_lo, const int32_t *level_ratio,
                         const double *level_cell_size, const double *prob_lo, int n_levels,
                         uint64_t capacity, double *vertices_dev, uint8_t *levels_dev,
                         double *samples_dev, uint64_t *counts_dev);

/* ---- streamlines ("Streamlines") ---------------------------------------------------- */

/* Field lines of the vector field (vx, vy, vz) -- three scenes of ctx with the same box list; raw
 * f64 cells, no transform -- from n_seeds seeds (seeds_dev: device, f64 [n][3], physical units)
 * by classical RK4 along the unit vector, IEEE binary64 with nothing fused, / and sqrt correctly
 * rounded.  The hierarchy description (box_index_lo, level_ratio, n_levels <= 16; host) is
 * avr_scene_gradient's; level_cell_size holds (dx, dy, dz) per level, prob_lo three values (host).
 * The leaf of a point P: for l = n_levels - 1, ..., 0, q[d] = (P[d] - prob_lo[d]) / dx[l][d]; a q[d]
 * that is not finite or lies outside [-2^30, 2^30) makes P outside; else the first level whose
 * boxes contain G = floor(q) gives the leaf (box, G, l); none: outside.  The value at P with leaf
 * level l: u = q - 0.5, C = floor(u), w = u - f64(C); the corners C + (di, dj, dk) are found as
 * avr_scene_isosurface finds a cube's (level l, then l - 1, ..., 0 by floor division; the first
 * hit wins; finer cells are never searched); with all eight present and every value finite the
 * value is trilinear -- a = v0 + w[0] * (v1 - v0) along x for the four (dj, dk), then the same
 * form along y, then z -- else it is the leaf cell's own value.  The three components share one
 * decision: trilinear iff all eight corners are present and all 24 values finite, else all three
 * from the leaf cell, and a leaf velocity with a component that is not finite ends the line.
 * D(P) = direction * V / |V|, |V| = sqrt((vx * vx + vy * vy) + vz * vz); |V| == 0 is stagnant.
 * A step from P with leaf level l: h = step * min_d dx[l][d]; k1 = D(P), k2 = D(P + (0.5 * h) *
 * k1), k3 = D(P + (0.5 * h) * k2), k4 = D(P + h * k3); P' = P + (h / 6.0) * (((k1 + 2.0 * k2) +
 * 2.0 * k3) + k4).  If one of the four evaluations is outside, stagnant or not finite (the first
 * stage that fails decides; within a stage in that order) no step is taken and the line ends at P
 * with that status; P' is appended even if it is outside itself, and the next step then ends the
 * line.  Line s: a seed that is outside (a NaN coordinate included) gives counts_dev[s] = 0 and
 * status 1; else point 0 is the seed and steps follow until one ends the line or max_steps were
 * taken.  status_dev[s] (device, u8): 0 max_steps reached, 1 outside, 2 stagnant, 3 not finite;
 * counts_dev[s] (device, u32) in 0 .. max_steps + 1; points_dev (device, f64 [n][max_steps + 1][3])
 * holds the line's points and, with `sample` (a scene of ctx with the same box list, or NULL),
 * samples_dev (device, f64 [n][max_steps + 1]) the sample field at every point by the same rule
 * on its own (trilinear iff its eight corners are present and finite, else the leaf value,
 * whatever it is), NaN at a final point that is outside.  Slots past a line's count are left
 * untouched.  Equal arguments give equal bits.  n_seeds == 0 succeeds without a launch.
 * Everything is checked on the host before any device work, in this order:
 * AVR_ERR_INVALID_ARGUMENT for a step that is not finite or not in (0, 1], a direction other than
 * +1 and -1, max_steps > 2^20, n_seeds * (max_steps + 1) >= 2^32, n_levels outside [1, 16], a
 * cell size that is not finite and positive, a prob_lo that is not finite, samples_dev given
 * without sample or the reverse, scenes that are not congruent, a box level >= n_levels, a ratio
 * below 2, a box index range outside [-2^30, 2^30), two boxes of one level that overlap in index
 * space, an output array or the seeds sharing a byte with an input box's cells, and a locator of
 * 2^28 list entries or more -- and every output is untouched.  Stateless; asynchronous on the
 * context's stream. */
int avr_scene_streamlines(avr_context *ctx, const avr_scene *vx, const avr_scene *vy,
                          const avr_scene *vz, const avr_scene *sample, const double *seeds_dev,
                          uint64_t n_seeds, double step, int direction, uint64_t max_steps,
                          const int32_t *box_index_lo, const int32_t *level_ratio,
                          const double *level_cell_size, const double *prob_lo, int n_levels,
                          double *points_dev, double *samples_dev, uint32_t *counts_dev,
                          uint8_t *status_dev);

/* ---- covering grids ("Covering grid") ----------------------------------------------- */

/* `field` (a scene of ctx; raw f64 cells, no transform; its boxes are the uncovered cells of the
 * loaded levels) resampled to the cells of level `level`: output cell (i, j, k) has the level-
 * `level` index G = lo + (i, j, k), 0 <= (i, j, k) < dims (lo, dims: host, three values each; the
 * region may reach past the data and lo may be negative).  The hierarchy description
 * (box_index_lo, level_ratio, n_levels <= 16; host) is avr_scene_gradient's; n_levels counts the
 * levels up to the finer of `level` and the finest level of a box, so `level` may be finer than
 * every box.  Three rules, in order:
 *  1. if a box of a level m <= level contains G mapped to level m by floor division, the box of
 *     the highest such m gives the cell's stored double with its bits kept (a NaN, an infinity
 *     and -0.0 are data), coverage 1.0 and cell level m;
 *  2. else, from num = den = +0.0, for every m = level + 1, ..., finest box level in that order:
 *     R_m = level_ratio[level] * ... * level_ratio[m - 1], w_m = 1.0 / f64(R_m^3); s = +0.0 and
 *     n = 0; for kk, then jj, then ii ascending over [G R_m, (G + 1) R_m), a level-m box that
 *     holds (ii, jj, kk) adds its cell, s = s + v, and one to n; with n > 0, num = num + w_m * s
 *     (one rounded multiply, one rounded add, nothing fused), den = den + w_m * f64(n) and the
 *     cell level is m.  With den > 0 the value is num / den and the coverage den;
 *  3. else the value is `fill` with its bits kept, the coverage 0.0 and the cell level -1.
 * values_dev (device, f64 [dims[2]][dims[1]][dims[0]]) gets the values; coverage_dev (f64) and
 * level_dev (i8) of the same shape get the coverage and the cell level, and either may be NULL:
 * they depend on the boxes alone, not on the field's values.  Equal arguments give equal bits.
 * Everything is checked on the host before any device work, in this order:
 * AVR_ERR_INVALID_ARGUMENT for n_levels outside [1, 16], level outside [0, n_levels), a box level
 * >= n_levels (and the other box rules), a ratio below 2, a box index range outside [-2^30,
 * 2^30), two boxes of one level that overlap in index space, a dims below 1, a region that leaves
 * [-2^30, 2^30) at `level` or, multiplied up, at the finest box level, 2^31 cells or more, an
 * output array that shares a byte with a box's cells, and candidate lists of 2^31 entries or more
 * -- and every output is untouched.  Stateless; asynchronous on the context's stream. */
int avr_scene_covering_grid(avr_context *ctx, const avr_scene *field, int level, const int32_t *lo,
                            const int32_t *dims, const int32_t *box_index_lo,
                            const int32_t *level_ratio, int n_levels, double fill,
                            double *values_dev, double *coverage_dev, int8_t *level_dev);

/* ---- grid fields ("Grid fields") ------------------------------------------------------ */

/* The inverse of avr_scene_covering_grid: the uniform grid grid_dev (device, f64
 * [dims[2]][dims[1]][dims[0]], fewer than 2^31 cells) of the level-`level` cells G = lo + (i, j, k)
 * written onto every cell of the boxes of `out` (a scene of ctx, whose cells are overwritten).  The
 * hierarchy description (box_index_lo, level_ratio, n_levels <= 16; host) is
 * avr_scene_covering_grid's.  For the cell with index I of a box of level l, per axis, with R the
 * product of the ratios between l and `level`:
 *  l == level: G = I; grid[G - lo] with its bits kept if G lies in the region, else `fill`;
 *  l > level, interpolation 0 (constant): G = floor_div(I, R), then as above;
 *  l > level, interpolation 1 (linear): p = I - G R, c = 2 p + 1 - R, t = f64(|c|) / f64(2 R), the
 *    neighbour N = G - 1 for c < 0 and G + 1 otherwise; an N that leaves the region wraps into it
 *    (periodic 1) or becomes G (periodic 0); `fill` if G is outside the region on any axis, else
 *    the eight values combined along x, then y, then z, each step a + t * (b - a) (one subtract,
 *    one multiply, one add, nothing fused, also for t == 0);
 *  l < level: s = +0.0, n = 0 and, for kk, then jj, then ii ascending over the part of [I R,
 *    (I + 1) R) inside the region, s = s + grid[...], n += 1; s / f64(n) with n > 0, else `fill`.
 * `fill` keeps its bits.  totals_dev (device, i64 [2]) is added into: the cells that got `fill`,
 * and the cells with l < level and 0 < n < R^3.  Equal arguments give equal bits.
 * Everything is checked on the host before any device work, in this order:
 * AVR_ERR_INVALID_ARGUMENT for n_levels outside [1, 16], level outside [0, n_levels), a box level
 * >= n_levels (and the other box rules), a ratio below 2, a box index range outside [-2^30,
 * 2^30), a dims below 1, a region that leaves [-2^30, 2^30) at `level` or, multiplied up, at the
 * finest box level, 2^31 cells or more, an interpolation or periodic outside {0, 1}, and a grid or
 * totals that share a byte with a box's cells -- and `out` and the totals are untouched.
 * Asynchronous on the context's stream. */
int avr_scene_grid_field(avr_context *ctx, avr_scene *out, const double *grid_dev, int level,
                         const int32_t *lo, const int32_t *dims, const int32_t *box_index_lo,
                         const int32_t *level_ratio, int n_levels, int interpolation, int periodic,
                         double fill, int64_t *totals_dev);

/* ---- particle fields ("Particle fields") ---------------------------------------------- */

/* The contributions of n particles to the cells of the boxes of `scene` (a scene of ctx; only its
 * boxes' dims and levels are read, never its cells).  points_dev: device, f64 [n][3], physical
 * units; values_dev: device, f64 [n], or NULL for a value of 1.0 each.  The hierarchy description
 * (box_index_lo, level_ratio, level_cell_size, prob_lo, n_levels <= 16; host) is
 * avr_scene_streamlines'.  A particle's leaf is the streamlines' leaf of a point P (levels from the
 * finest, q = (P - prob_lo) / dx_l, each q finite and inside [-2^30, 2^30)); a particle without one
 * is outside.  A cell's ordinal is avr_scene_clumps': the cells of the boxes in scene order, (k ny
 * + j) nx + i inside a box.
 *  method 0 (nearest grid point), C = 1: (cell, share) = (the leaf's ordinal, v), v's bits kept.
 *  method 1 (cloud in cell), C = 8: at the leaf's level l, u = q - 0.5, B = floor(u), w = u -
 *    f64(B); for dk, then dj, then di ascending (entry c = 4 dk + 2 dj + di) the weight along an axis
 *    is w for a 1 and 1.0 - w for a 0, share = ((wx * wy) * wz) * v (nothing fused, also for a weight
 *    of 0), and the cell is the ordinal of the level-l index B + (di, dj, dk) under the
 *    same-or-coarser rule of the streamlines' corners, or, where that rule finds none (a domain
 *    face, a hole, a region that finer cells cover), the leaf's own: the share is rerouted.
 * cells_dev (i64 [n][C]) and shares_dev (f64 [n][C]) are written particle-major; an outside
 * particle's entries are (0xFFFFFFFF, +0.0).  levels_dev (u8 [n], or NULL) gets the leaf's level,
 * 255 outside.  totals_dev (i64 [2]) is added into: outside particles, rerouted shares.  Equal
 * arguments give equal bits.  Everything is checked on the host before any device work, in this
 * order: AVR_ERR_INVALID_ARGUMENT for n_levels outside [1, 16], a null array (all but totals_dev may
 * be NULL with n == 0), a method outside {0, 1}, n >= 2^31 (2^28 with method 1), a cell size that is
 * not finite and positive, a prob_lo that is not finite, a box level >= n_levels (and the other box
 * rules), a ratio below 2, a box index range outside [-2^30, 2^30), two boxes of one level that
 * overlap in index space, 2^31 cells or more, a locator past its limits, and an output that shares
 * a byte with another output, the points or the values -- and every output and the totals are
 * untouched.  n == 0 launches nothing.  Asynchronous on the context's stream. */
int avr_scene_particle_cells(avr_context *ctx, const avr_scene *scene, const double *points_dev,
                             uint64_t n, const double *values_dev, int method,
                             const int32_t *box_index_lo, const int32_t *level_ratio,
                             const double *level_cell_size, const double *prob_lo, int n_levels,
                             int64_t *cells_dev, double *shares_dev, uint8_t *levels_dev,
                             int64_t *totals_dev);

/* Contributions added onto the cells of the boxes of `out` (a scene of ctx, whose cells are
 * overwritten and whose classification is forgotten).  cells_sorted_dev (device, i64 [n]) and
 * shares_sorted_dev (device, f64 [n]) are avr_scene_particle_cells' entries sorted by cell, equal
 * cells in their list order (a stable sort).  Every cell of every box gets s = +0.0, then s = s +
 * share over the entries that name its ordinal, in ascending position; its value is s (quantity
 * 0, sum) or s / vol_l (quantity 1, density; one division, vol_l = (dx_l * dy_l) * dz_l of the
 * box's level, from level_cell_size, f64 [n_levels][3], host).  A cell no entry names holds +0.0.
 * An entry whose cell names no cell of `out` (0xFFFFFFFF among them) is skipped.  The order is not
 * checked: each maximal run of equal cells is summed on its own, and a cell named by several runs
 * keeps one run's sum.  AVR_ERR_INVALID_ARGUMENT, before any device work and in this order, for
 * n_levels outside [1, 16], a null array (both may be NULL with n_contributions == 0), a quantity
 * outside {0, 1}, n_contributions >= 2^31, a cell size that is not finite and positive, the box
 * rules, 2^31 cells or more, and cells or shares that share a byte with a box's cells -- and `out`
 * is untouched.  n_contributions == 0 still clears.  Asynchronous on the context's stream. */
int avr_scene_particle_deposit(avr_context *ctx, avr_scene *out, const int64_t *cells_sorted_dev,
                               const double *shares_sorted_dev, uint64_t n_contributions,
                               int quantity, const double *level_cell_size, int n_levels);

/* ---- particle groups ("Particle groups") ---------------------------------------------- */

/* Friends-of-friends groups of n particles, in two calls with a sort by the caller between them.
 * The box lo, hi (host, f64 [3], finite, lo < hi), the flags periodic (host, i32 [3]) and the grid
 * dims (host, i32 [3]: each in [1, 1024], product below 2^27, at least 3 on a periodic axis) are
 * the same in both.  A particle is outside if a coordinate is not finite or, on a periodic axis,
 * not in [lo, hi).  The grid is an accelerator only: h_d = (hi_d - lo_d) / dims_d, a particle's cell
 * along d is floor((x - lo_d) / h_d) clamped in double to [0, dims_d - 1], and its cell is (cz ny +
 * cy) nx + cx.
 *
 * This call: points_dev (device, f64 [n][3]) -> cells_dev (u32 [n], the cell, 0xFFFFFFFF outside),
 * parent_dev (u32 [n], the particle's own index, 0xFFFFFFFF outside) and totals_dev (u64 [1]), to
 * which the number of outside particles is added.  AVR_ERR_INVALID_ARGUMENT, before any device work
 * and in this order, for a null array (the four device arrays may be NULL with n == 0), n >= 2^31,
 * lo or hi not finite or lo >= hi, a dim outside [1, 1024], 2^27 cells or more, fewer than 3 cells
 * on a periodic axis, and an output that shares a byte with another output or the points -- and
 * every output is untouched.  n == 0 launches nothing.  Asynchronous on the context's stream. */
int avr_particle_group_cells(avr_context *ctx, const double *points_dev, uint64_t n,
                             const double *lo, const double *hi, const int32_t *dims,
                             const int32_t *periodic, uint32_t *cells_dev, uint32_t *parent_dev,
                             uint64_t *totals_dev);

/* The groups.  The caller has sorted the particles by cells_dev, stably: order_dev (device, i64
 * [n]) names the particle in each sorted slot, points_sorted_dev (f64 [n][3]) holds the points in
 * that order, cell_begin_dev (i64 [cells + 1]) the first slot of every cell, and the first n_inside
 * slots are the inside particles.  parent_dev is avr_particle_group_cells' output for the same
 * points, box and dims.  Inside particles p, q are linked iff (dx dx + dy dy) + dz dz <= b b, with
 * per axis a = |x_q - x_p| and, on a periodic axis, a = min(a, (hi - lo) - a); IEEE binary64,
 * nothing fused.  A group is a connected component of the links and its root its smallest particle
 * index; the groups of at least min_members members are numbered 1..N by ascending root.
 * labels_dev (i32 [n]) gets each particle's group, 0 for none; parent_dev each inside particle's
 * root; sizes_dev (u32 [n]) the member count at every root's index and 0 elsewhere; n_groups_dev
 * (u64 [1]) N.  Equal arguments give equal bits, and the result does not depend on dims.
 * COST: every pair of particles in the same or in adjacent cells is tested, which is quadratic in
 * a cell's occupancy; the caller must bound that number itself (the Python api counts it exactly
 * from the cell ranges and refuses above max_pair_tests).
 * AVR_ERR_INVALID_ARGUMENT, before any device work and in this order, for a null array (all device
 * arrays but n_groups_dev may be NULL with n == 0), n >= 2^31, n_inside > n, b not finite and
 * positive, the box and dims rules above, h_d < b (1 + 2^-10) on an axis with dims_d > 1,
 * min_members outside [1, 2^31), and an output that shares a byte with another output or an input
 * -- and every output is untouched.  n == 0 launches nothing but sets n_groups to 0.  The scan's
 * scratch is a grow-only block of the context.  Asynchronous on the context's stream. */
int avr_particle_groups(avr_context *ctx, const double *points_sorted_dev, const int64_t *order_dev,
                        const int64_t *cell_begin_dev, uint64_t n, uint64_t n_inside, double b,
                        const double *lo, const double *hi, const int32_t *dims,
                        const int32_t *periodic, int64_t min_members, uint32_t *parent_dev,
                        int32_t *labels_dev, uint32_t *sizes_dev, uint64_t *n_groups_dev);

/* ---- rays ("Rays") -------------------------------------------------------------------- */

/* Line-outs: for each of n_rays segments A -> B (start_dev, end_dev: device, f64 [n][3], physical
 * units) every leaf cell of `field` (a scene of ctx; raw f64 cells, no transform) that the segment
 * crosses, in order, as (t0, t1, level, value) with P(t) = A + t (B - A), and the sums
 * integral = sum value * (t1 - t0) |B - A| over the leaf segments with a finite value and covered =
 * sum (t1 - t0) |B - A| over the leaf segments.  The definition -- the clip against the scene's
 * level-0 index bounding box, Locate, the walk from face to face, absent stretches walked at the
 * finest cell size as level -1 with a NaN value -- is DESIGN.md 7, "Rays"; IEEE binary64 with
 * nothing fused, / and sqrt correctly rounded.  The hierarchy description (box_index_lo,
 * level_ratio, n_levels <= 16; host) is avr_scene_gradient's; level_cell_size holds (dx, dy, dz) per
 * level, prob_lo three values (host).
 * Two passes.  offsets_dev == NULL is the count pass: counts_dev (device, u32 [n]) gets the number
 * of segments of every ray, status_dev (u8 [n]) 0 complete, 1 the ray misses the scene's box, 2
 * max_trips trips were made (the segments found so far are kept), 3 an end point is not finite or
 * A == B, and span_dev (f64 [n][2]) t_enter and t_leave of the clip, NaN for status 1 and 3; the
 * other output arrays are not looked at.  With offsets_dev (device, i64 [n + 1], the exclusive
 * scan of the counts and their total) it is the emit pass: the identical walk writes ray s's
 * segments to t0_dev, t1_dev, value_dev (f64) and level_dev (i8), arrays of n_segments entries, at
 * offsets_dev[s] on, and integral_dev and covered_dev (f64 [n]); counts_dev, status_dev and
 * span_dev are not looked at.  A ray never writes outside [offsets[s], offsets[s + 1]) nor past
 * n_segments, whatever offsets_dev holds.  Equal arguments give equal bits.  n_rays == 0 succeeds
 * without a launch.
 * Everything is checked on the host before any device work, in this order:
 * AVR_ERR_INVALID_ARGUMENT for a NULL field or one that is not a scene of ctx, max_trips outside
 * [1, 2^30], n_rays >= 2^32, n_segments > 2^40 (emit pass), n_levels outside [1, 16], a required
 * array that is NULL (level_cell_size, prob_lo, level_ratio with n_levels > 1, box_index_lo with
 * boxes; with n_rays > 0 the end points and the outputs of the pass that runs), a cell size that is not finite and
 * positive, a prob_lo that is not finite, a box level >= n_levels (and the other box rules), a
 * ratio below 2, a box index range outside [-2^30, 2^30), two boxes of one level that overlap in
 * index space, an output array, start_dev, end_dev or offsets_dev sharing a byte with an input
 * box's cells, a locator of 2^28 list entries or more, and a level-0 bounding box of the scene
 * that, refined to level n_levels - 1, leaves [-2^30, 2^30] -- and every output is untouched.
 * Stateless; asynchronous on the context's stream. */
int avr_scene_rays(avr_context *ctx, const avr_scene *field, const double *start_dev,
                   const double *end_dev, uint64_t n_rays, uint64_t max_trips,
                   const int32_t *box_index_lo, const int32_t *level_ratio,
                   const double *level_cell_size, const double *prob_lo, int n_levels,
                   const int64_t *offsets_dev, uint64_t n_segments, uint32_t *counts_dev,
                   uint8_t *status_dev, double *span_dev, double *t0_dev, double *t1_dev,
                   int8_t *level_dev, double *value_dev, double *integral_dev,
                   double *covered_dev);

/* ---- per-ray sums ("Off-axis projection") --------------------------------------------- */

/* The sums of avr_scene_rays' walk in one pass, nothing stored per segment: for each of n_rays
 * segments A -> B the clip, Locate, the trips and the status rules are those of DESIGN.md 7,
 * "Rays", and over the emitted segments of leaf cells, in walk order from +0.0, with w = (t1 - t0)
 * |B - A|: covered = sum w; without `weight` (NULL), where the value v is finite, integral = sum
 * v w and counted = sum w; with `weight` (a scene of ctx whose boxes are, box by box, the field's
 * in level, dims and corner) and q the weight's value in the same cell, where v and q are both
 * finite, integral = sum (v q) w, weight = sum q w and counted = sum w.  counts_dev (device, u32
 * [n]), status_dev (u8 [n]) and span_dev (f64 [n][2]) get what avr_scene_rays' count pass writes,
 * integral_dev and covered_dev (f64 [n]) -- without `weight` -- what its emit pass writes, by
 * bits; weight_dev (f64 [n]) is NULL exactly when `weight` is; counted_dev is f64 [n].  The
 * hierarchy arguments are avr_scene_rays'.  Equal arguments give equal bits.  n_rays == 0 succeeds
 * without a launch.
 * Everything is checked on the host before any device work, in avr_scene_rays' order with its
 * messages (there is no n_segments; with n_rays > 0 every array named above must be there, and
 * weight_dev must be there exactly with `weight`: "null argument"); after the field's box rules a
 * weight scene whose boxes differ from the field's in number, level, dims or corner is refused,
 * then a weight box that breaks the box rules; and no output, nor start_dev or end_dev, may share a
 * byte with a cell of either scene -- AVR_ERR_INVALID_ARGUMENT, and every output is untouched.
 * Stateless; asynchronous on the context's stream. */
int avr_scene_ray_sums(avr_context *ctx, const avr_scene *field, const avr_scene *weight,
                       const double *start_dev, const double *end_dev, uint64_t n_rays,
                       uint64_t max_trips, const int32_t *box_index_lo,
                       const int32_t *level_ratio, const double *level_cell_size,
                       const double *prob_lo, int n_levels, uint32_t *counts_dev,
                       uint8_t *status_dev, double *span_dev, double *integral_dev,
                       double *weight_dev, double *counted_dev, double *covered_dev);

/* ---- power spectra ("Power spectrum") ------------------------------------------------ */

/* The twiddle table the transform's kernels use for a line of n values, as n / 2 pairs: table[2 m]
 * = cos t and table[2 m + 1] = sin t with t = -(2.0 pi m) / n evaluated in that order in double,
 * by the C library's cos and sin.  Host only: no context, no device work.
 * AVR_ERR_INVALID_ARGUMENT for a NULL table and for an n that is not a power of two in [2, 1024]. */
int avr_fft_twiddles(int n, double *table);

/* The forward, unnormalised 3-D discrete Fourier transform F[k] = sum_n x[n] exp(-2 pi i k n / N)
 * of the real grid values_dev (device, f64 [dims[2]][dims[1]][dims[0]], dims = (nx, ny, nz)) into
 * spectrum_dev (device, f64 [dims[2]][dims[1]][dims[0]][2], (re, im) interleaved).  The imaginary
 * part starts at +0.0; every line is transformed along x, then along y, then along z.  One line of
 * N = 2^p values: the input permuted by bit reversal of the p-bit index, then stages s = 1 .. p of
 * radix-2 decimation in time -- with half = 2^(s - 1) and step = N / 2^s, for every block of
 * 2 half elements and every j in [0, half): a = v[block + j], b = v[block + j + half], w =
 * W[j step] (avr_fft_twiddles), t = (w.re b.re - w.im b.im, w.re b.im + w.im b.re), each component
 * two rounded multiplies and one rounded add or subtract with nothing fused, v[block + j] = a + t
 * and v[block + j + half] = a - t.  N = 1 is the identity.  Equal arguments give equal bits.
 * Everything is checked on the host before any device work, in this order:
 * AVR_ERR_INVALID_ARGUMENT for a NULL argument, a dims that is not a power of two in [1, 1024],
 * 2^31 cells or more, and a spectrum that shares a byte with the input -- and the spectrum is
 * untouched.  Stateless; asynchronous on the context's stream. */
int avr_field_fft(avr_context *ctx, const double *values_dev, const int32_t *dims,
                  double *spectrum_dev);

/* Shell sums of a spectrum (spectrum_dev as avr_field_fft writes it, dims = (nx, ny, nz)).  The
 * mode at (kz, ky, kx) has per axis the signed wave number m_d = k_d if k_d < N_d / 2 or N_d == 1,
 * else k_d - N_d; q = f64(mx)^2 g[0] + f64(my)^2 g[1], then + f64(mz)^2 g[2], with g =
 * inverse_length_sq (host, 3 doubles: 1 / L_d^2), each term one multiply of the exact integer
 * square; p = re re + im im.  edges_sq (host, n_bins + 1 doubles) are the squared edges E[i] =
 * (e[i] / (2 pi))^2: E[i] <= q < E[i + 1] puts the mode in bin i, q == E[n_bins] in the last bin,
 * decided by f64 comparisons alone.  Per mode, in this order: p not finite adds one to
 * totals_dev[1] (nonfinite); else q outside the edges adds one to totals_dev[0] (outside); else
 * modes_dev[bin] += 1 and power_dev[bin] += p (f64 additions in no fixed order).  modes_dev (u64
 * [n_bins]), power_dev (f64 [n_bins]) and totals_dev (u64 [2]) are device arrays that are ADDED
 * to, as avr_scene_joint_histogram's are.  Everything is checked on the host before any device
 * work, in this order: AVR_ERR_INVALID_ARGUMENT for a NULL argument, a dims that is not a power of
 * two in [1, 1024], 2^31 cells or more, n_bins outside [1, 2048], an edge that is not finite, a
 * negative E[0], edges that do not strictly increase, a g that is not finite and positive, and an
 * output that shares a byte with the spectrum -- and every output is untouched.  Stateless;
 * asynchronous on the context's stream. */
int avr_spectrum_bins(avr_context *ctx, const double *spectrum_dev, const int32_t *dims,
                      const double *inverse_length_sq, const double *edges_sq, int n_bins,
                      uint64_t *modes_dev, double *power_dev, uint64_t *totals_dev);

/* ---- inverse transform, Helmholtz split, potential --------------------------------- */

/* The normalised inverse 3-D transform x[n] = (1 / N) sum_k F[k] exp(+2 pi i k n / N) of
 * spectrum_dev (device, f64 [dims[2]][dims[1]][dims[0]][2], as avr_field_fft writes it) into the
 * real grids values_dev (the real part) and, unless NULL, imag_dev (the imaginary part), both
 * device f64 [dims[2]][dims[1]][dims[0]].  One line is transformed as avr_field_fft states it --
 * bit reversal, the stages, the same butterfly, nothing fused -- with the table V[m] = (W[m].re,
 * -W[m].im) in place of W; every line is transformed along z, then y, then x, and after the x pass
 * both components are multiplied by s = 1.0 / f64(nx ny nz), an exact power of two.  The strided
 * passes run in place: what spectrum_dev holds after the call is unspecified.  Equal arguments give
 * equal bits.  Everything is checked on the host before any device work, in this order:
 * AVR_ERR_INVALID_ARGUMENT for a NULL argument other than imag_dev, a dims that is not a power of
 * two in [1, 1024], 2^31 cells or more, and any byte shared among the three arrays -- and every
 * array is untouched.  Stateless; asynchronous on the context's stream. */
int avr_field_ifft(avr_context *ctx, double *spectrum_dev, const int32_t *dims, double *values_dev,
                   double *imag_dev);

/* The Helmholtz split of the spectra of (vx, vy, vz) -- spectra_dev (host array of three device
 * spectra as avr_field_fft writes them), read and then overwritten with the solenoidal part S --
 * and its compressive part C into compressive_dev (three more device spectra).  Per mode, m_d is
 * avr_spectrum_bins' signed wave number with the Nyquist rule added (N_d >= 2 and k_d == N_d / 2:
 * m_d = 0, which keeps the projector Hermitian), kappa_d = f64(m_d) h[d] with h = inverse_length
 * (host, 3 doubles: 1 / L_d), q = kx kx + ky ky, then + kz kz.  q == 0: every C_d = (+0.0, +0.0)
 * and S_d = F_d with its bits kept.  Else, for the real and the imaginary component separately:
 * d = kx Fx + ky Fy, then + kz Fz; s = d / q (one correctly rounded division); C_d = kappa_d s;
 * S_d = F_d - C_d; nothing fused.  Values that are not finite propagate by IEEE rules.  Equal
 * arguments give equal bits.  Everything is checked on the host before any device work, in this
 * order: AVR_ERR_INVALID_ARGUMENT for a NULL argument or array, a dims that is not a power of two
 * in [1, 1024], 2^31 cells or more, per axis an h that is not finite and positive, an h whose
 * square is below DBL_MIN, an h with (512 h)^2 not finite, and a byte shared between any two of
 * the six arrays -- and every array is untouched.  Stateless; asynchronous on the context's
 * stream. */
int avr_spectrum_helmholtz(avr_context *ctx, double *const spectra_dev[3], const int32_t *dims,
                           const double inverse_length[3], double *const compressive_dev[3]);

/* The inverse Laplacian of a spectrum in place: with avr_spectrum_bins' q (no Nyquist rule; g =
 * inverse_length_sq, host, 3 doubles), a mode with q == 0 becomes (+0.0, +0.0), every other one
 * (re r, im r) with r = scale / q.  Equal arguments give equal bits.  Everything is checked on the
 * host before any device work, in this order: AVR_ERR_INVALID_ARGUMENT for a NULL argument, a dims
 * that is not a power of two in [1, 1024], 2^31 cells or more, a g that is not finite and
 * positive, and a scale that is not finite -- and the spectrum is untouched.  Stateless;
 * asynchronous on the context's stream. */
int avr_spectrum_inverse_laplacian(avr_context *ctx, double *spectrum_dev, const int32_t *dims,
                                   const double *inverse_length_sq, double scale);

/* ---- isolated potential ------------------------------------------------------------ */

/* The open-boundary Green's function of a zero-padded grid: green_dev (device, f64
 * [padded_dims[2]][padded_dims[1]][padded_dims[0]]) is written, nothing is read.  For the cell
 * (k, j, i), per axis s_d = min(i_d, P_d - i_d) as an integer and x_d = f64(s_d) * cell_size[d]
 * (host, 3 doubles: dx, dy, dz); r2 = x x + y y, then + z z; G = scale / sqrt(r2), one correctly
 * rounded square root and one correctly rounded division, nothing fused; the single cell with
 * r2 == 0, (0, 0, 0), holds self_value.  Equal arguments give equal bits.  Everything is checked on
 * the host before any device work, in this order: AVR_ERR_INVALID_ARGUMENT for a NULL argument, a
 * padded_dims that is not a power of two in [1, 1024], 2^31 cells or more, per axis a cell_size
 * that is not finite and positive, one whose square is below DBL_MIN, one with (512 cell_size)^2
 * not finite, and a scale or self_value that is not finite -- and the grid is untouched.
 * Stateless; asynchronous on the context's stream. */
int avr_isolated_green(avr_context *ctx, const int32_t *padded_dims, const double *cell_size,
                       double scale, double self_value, double *green_dev);

/* The product of two spectra in place: a_dev and b_dev (device, f64
 * [dims[2]][dims[1]][dims[0]][2], as avr_field_fft writes them); every mode of a_dev becomes
 * (a.re b.re - a.im b.im, a.re b.im + a.im b.re), each from two products and one addition, nothing
 * fused; b_dev is only read.  Values that are not finite propagate by IEEE rules.  Equal arguments
 * give equal bits.  Everything is checked on the host before any device work, in this order:
 * AVR_ERR_INVALID_ARGUMENT for a NULL argument, a dims that is not a power of two in [1, 1024],
 * 2^31 cells or more, and any byte shared between the two spectra -- and both are untouched.
 * Stateless; asynchronous on the context's stream. */
int avr_spectrum_multiply(avr_context *ctx, double *a_dev, const double *b_dev,
                          const int32_t *dims);

/* ---- structure functions ----------------------------------------------------------- */

/* The moments of the increments of n_components (1 or 3) real grids over n_lags integer lag
 * vectors.  components_dev: host array of n_components device grids, f64
 * [dims[2]][dims[1]][dims[0]] with dims = (nx, ny, nz), every one at least 1; the grids may alias
 * each other.  lags (host, 3 n_lags int32: lx, ly, lz per lag); directions (host, 3 n_lags
 * doubles: ux, uy, uz per lag) with three components, NULL with one.  The partner of the centre
 * cell c = (i, j, k) under lag m is q = c + l_m: with periodic every axis wraps once, without it a
 * pair whose partner leaves the grid on any axis adds one to totals_dev[0] (outside) and nothing
 * else.  Per component delta_d = v_d[q] - v_d[c].  One component: a = |delta|, K = 1 kind.  Three:
 * m2 = dx dx + dy dy, then + dz dz; L = dx ux + dy uy, then + dz uz; t_d = delta_d - L u_d; T2 =
 * tx tx + ty ty, then + tz tz; K = 3 kinds a_0 = |L| (longitudinal), a_1 = sqrt(T2) (transverse),
 * a_2 = sqrt(m2) (magnitude).  Every operation is one rounded f64 operation, nothing fused, the
 * square roots correctly rounded.  A pair whose a (one component) or m2 (three; an overflowing
 * square included) is not finite adds one to totals_dev[1] (nonfinite) and nothing else.  Every
 * other pair adds one to pairs_dev[m] and, with w_1 = a and w_p = w_(p-1) a, w_p to sums_dev[(m K
 * + kind) max_order + p - 1] for p = 1 .. max_order (f64 additions in no fixed order).  pairs_dev
 * (u64 [n_lags]), sums_dev (f64 [n_lags][K][max_order]) and totals_dev (u64 [2]) are device
 * arrays that are ADDED to, as avr_spectrum_bins' are.  Every ordered lag visits every centre
 * once: l and -l give the same pairs.  Everything is checked on the host before any device work,
 * in this order: AVR_ERR_INVALID_ARGUMENT for a NULL argument, n_components other than 1 or 3,
 * directions not given exactly with three components, a NULL grid, a dims below 1, 2^31 cells or
 * more, n_lags outside [1, 4096], max_order outside [1, 8], periodic other than 0 or 1, a lag
 * that is zero, a lag with |l_d| >= N_d on an axis (in both boundary modes), a direction that is
 * not finite, an output that shares a byte with a grid, and two outputs that share a byte -- and
 * every output is untouched.  Stateless; asynchronous on the context's stream. */
int avr_grid_structure_functions(avr_context *ctx, const double *const *components_dev,
                                 int n_components, const int32_t *dims, const int32_t *lags,
                                 const double *directions, int n_lags, int max_order,
                                 int periodic, uint64_t *pairs_dev, double *sums_dev,
                                 uint64_t *totals_dev);

/* ---- velocity cubes ("Velocity cubes") ---------------------------------------------- */

/* The on-axis projection of the raw f64 cells of scene_e ("emission") split into n_channels
 * channels of the cells of scene_g ("velocity": any field), a cell's share optionally spread over
 * the channels by a Gaussian of width scene_s (NULL: none; a 1-sigma width in the units of g).  The
 * scenes belong to ctx and hold the same box list as avr_scene_joint_histogram requires; each keeps
 * its own strides.  Axis, window, pixel lines, box containment, cell index, level_dl and row order
 * are avr_scene_axis_projection's.  edges (host): n_channels + 1 finite, strictly increasing f64, 1
 * <= n_channels <= 1024.  A cell counts when e and g are finite and, with scene_s, s is finite and
 * >= 0; other cells add nothing.  Without scene_s, or where s == 0, the cell's e goes to the
 * channel c with edges[c] <= g < edges[c + 1] (the last channel closed at the top; f64 comparisons
 * only), to under if g < edges[0], to over if g > edges[n_channels].  Where s > 0, with a_j =
 * ((edges[j] - g) / s) * 0.70710678118654752440 (three rounded operations) and q_j = -1 if a_j <=
 * -6, +1 if a_j >= 6, else erf(a_j): channel c gets e * (0.5 * (q_(c+1) - q_c)), under e * (0.5 *
 * (q_0 + 1)), over e * (0.5 * (1 - q_nc)).  Per pixel p = y * width + x, with dl = level_dl[the
 * box's level]: cube[c][p], under[p] and over[p] = sum_b dl * (the sum of the box's terms on the
 * line), length[p] = sum_b dl * f64(the cells that count); f64 on the device, 0 where no box
 * contains the line, all overwritten.  A column's terms are added in ascending cell order within
 * segments of 128 cells, the segments and then the boxes in ascending order; no atomic touches an
 * output or a partial sum: equal arguments give equal bits.  Everything is checked on the host
 * before any device work, in this order: AVR_ERR_INVALID_ARGUMENT for a NULL argument, scenes of
 * another context or box count, an axis not in 0..2, a non-positive image size, a non-finite
 * window, n_levels outside [1, 16], a non-finite level_dl, n_channels outside [1, 1024], edges not
 * finite or not strictly increasing, n_channels * width * height >= 2^31, boxes that differ in
 * dims or level or whose level is >= n_levels, partial planes of one channel past the scratch
 * bound (2^27 entries), an output that shares a byte with an input box's cells or with another
 * output -- and every output is untouched.  Asynchronous on the context's stream; the context
 * keeps the partial planes of one batch of channels (grow-only scratch, at most 1 GiB of channel
 * planes) and loops over the batches. */
int avr_scene_velocity_cube(avr_context *ctx, const avr_scene *scene_e, const avr_scene *scene_g,
                            const avr_scene *scene_s, int axis, const double origin_uv[2],
                            double du, double dv, int width, int height, const double *level_dl,
                            int n_levels, const double *edges, int n_channels, double *cube_dev,
                            double *under_dev, double *over_dev, double *length_dev);

/* The bound on (channels of a batch) x (entries of a partial plane) of avr_scene_velocity_cube,
 * in f64 entries: 1 .. 2^27, 0 restores the default of 2^27.  A smaller bound only cuts the
 * channels into more batches (the results do not change); it is there for tests and for callers
 * short of memory. */
int avr_context_set_velocity_cube_scratch_entries(avr_context *ctx, uint64_t entries);

/* Ray transfer ("Ray transfer"): emission and absorption along the rays of
 * avr_scene_ray_sums, front to back.  source (the source function S), opacity (the absorption
 * coefficient a per unit length; with channels integrated over the line), bin_or_null (the field g
 * the channels bin: a line-of-sight velocity) and width_or_null (a 1-sigma width s in the units of
 * g; only with a bin scene) are scenes of this context over the same boxes: box by box the
 * source's level, dims and corner.  The rays, max_trips, the hierarchy's arguments, counts_dev,
 * status_dev, span_dev and covered_dev are avr_scene_ray_sums'.  edges_or_null: n_channels + 1
 * finite, strictly increasing channel edges on the host, 1 <= n_channels <= 1024, given exactly
 * with a bin scene; without one (grey) n_channels is 1.  A leaf segment of length w counts when S
 * and a are finite and a >= 0 (and g is finite, and s is finite and >= 0); counted_dev f64
 * [n_rays] sums w over those.  Per counted segment and channel c, nearest segment first,
 *   dtau = ((a * w) * share) * rdv[c],   rdv[c] = 1.0 / (edges[c + 1] - edges[c])  (grey: 1)
 *   I[c] = I[c] + (S * (-expm1(-dtau))) * exp(-tau[c]),   then   tau[c] = tau[c] + dtau
 * with the shares of avr_scene_velocity_cube: sharp (no width scene, or s == 0) 1 for the channel
 * with edges[c] <= g < edges[c + 1], the last closed at the top; broadened the Gaussian's part of
 * the channel; grey 1.  intensity_dev and tau_dev: f64 [n_channels][n_rays].
 * outside_dev_or_null: f64 [2][n_rays], sum (a * w) * share below edges[0] and above
 * edges[n_channels], given exactly with a bin scene.  Rays that miss or are invalid get +0.0 in
 * every channel.  The results do not depend on avr_context_set_ray_transfer_chunk.  n_rays == 0
 * succeeds without a launch.  Everything is validated before any device work: a null argument, a
 * scene of another context, a broken rule of avr_scene_ray_sums (the weight scene's read per
 * scene), a broken channel rule, n_channels x n_rays >= 2^31, or an output, start_dev or end_dev
 * that shares a byte with a cell of any of the scenes -- AVR_ERR_INVALID_ARGUMENT, and every
 * output is untouched.  Stateless; asynchronous on the context's stream. */
int avr_scene_ray_transfer(avr_context *ctx, const avr_scene *source, const avr_scene *opacity,
                           const avr_scene *bin_or_null, const avr_scene *width_or_null,
                           const double *start_dev, const double *end_dev, uint64_t n_rays,
                           uint64_t max_trips, const int32_t *box_index_lo,
                           const int32_t *level_ratio, const double *level_cell_size,
                           const double *prob_lo, int n_levels, const double *edges_or_null,
                           int n_channels, uint32_t *counts_dev, uint8_t *status_dev,
                           double *span_dev, double *intensity_dev, double *tau_dev,
                           double *outside_dev_or_null, double *counted_dev, double *covered_dev);

/* The channels a workgroup of avr_scene_ray_transfer keeps in LDS at a time: 1 .. 32, 0 restores
 * the default of 16.  Every chunk of channels repeats the walk, and fewer workgroups fit a CU with
 * a larger chunk; the results do not change.  It is there for tests and for timing. */
int avr_context_set_ray_transfer_chunk(avr_context *ctx, int channels);

#ifdef __cplusplus
}
#endif
#endif /* AVR_HIP_H */
