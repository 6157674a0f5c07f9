// C ABI of the MI355X volume-rendering path (include/avr_hip.h).  Thin: validates, runs the
// host prologue (avr_host.cpp), stages the per-frame descriptors and launches the kernels
// (avr_kernels.hip) on the context's stream; what a frame stages and launches is planned on the
// host (avr_frame_launch.h).  No CPU compute fallback exists behind it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <exception>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/avr_hip_debug.h"
#include "avr_context.h"
#include "avr_internal.h"
#include "avr_plan.h"

namespace avr {

static_assert((hipEventDisableTiming | hipEventDisableSystemFence) == (0x2u | 0x20000000u),
              "avr::ordering_event_flags spells the flags out (avr_internal.h has no HIP header)");

namespace {
thread_local std::string g_last_error;
}

void set_error(const std::string& message) { g_last_error = message; }
const std::string& last_error() { return g_last_error; }

// Every host wait on device work has a deadline (AVR_FRAME_TIMEOUT_MS, default 30 s; 0 = none): the
// frame of a rank of several contains collectives, and a peer that died, or whose calls differ from
// this rank's, would otherwise leave the wait -- and the job -- hanging.  The reference's exchange
// either completes or errors (MPI_Waitany / MPI_Waitall, DirectSendBase.cpp:206-220, 277); so does
// this one: the wait throws, the C ABI call returns AVR_ERR_RUNTIME naming what did not finish.
namespace {
std::atomic<int> g_timeout_override{-1};
thread_local int t_collective_depth = 0;
}
void set_frame_timeout_ms(int ms) { g_timeout_override.store(ms < 0 ? -1 : ms); }
CollectiveScope::CollectiveScope(bool collective) : on_(collective) {
  if (on_) ++t_collective_depth;
}
CollectiveScope::~CollectiveScope() {
  if (on_) --t_collective_depth;
}
// A deadline somebody asked for (avr_set_frame_timeout_ms, AVR_FRAME_TIMEOUT_MS) holds for every
// wait; the DEFAULT of 30 s only where a collective is involved (a renderer of several ranks, a
// communicator's own calls): a single-rank context waiting for a deep queue of long frames, or
// for a GPU it shares with other processes, waits as long as it takes.
int frame_timeout_ms() {
  const int forced = g_timeout_override.load(std::memory_order_relaxed);
  if (forced >= 0) return forced;
  static const int value = [] {
    const char* text = std::getenv("AVR_FRAME_TIMEOUT_MS");
    if (text == nullptr || text[0] == '\0') return -1;
    const long parsed = std::strtol(text, nullptr, 10);
    return static_cast<int>(std::min<long>(std::max<long>(parsed, 0), 3600000));
  }();
  if (value >= 0) return value;
  return t_collective_depth > 0 ? 30000 : 0;
}

// Host waits poll the event instead of blocking in hipEventSynchronize / hipStreamSynchronize:
// a blocking wait that outlasts the runtime's spin phase sleeps on an interrupt, and waking from
// it was measured to take milliseconds on this platform -- by then a pipelined renderer's queue
// has run dry (5-7 ms stalls every few frames at 1.3 ms per frame, tools/host_stalls.py).
void wait_event_deadline(void* event_v, const char* what) {
  hipEvent_t event = static_cast<hipEvent_t>(event_v);
  const int limit_ms = frame_timeout_ms();
  std::chrono::steady_clock::time_point deadline{};
  for (unsigned spins = 0;; ++spins) {
    const hipError_t status = hipEventQuery(event);
    if (status == hipSuccess) return;
    if (status != hipErrorNotReady) hip_check(status, what);
    (void)hipGetLastError();  // hipErrorNotReady is not an error here
    if (spins > 64) std::this_thread::yield();
    if (limit_ms > 0 && (spins & 255u) == 255u) {
      const auto now = std::chrono::steady_clock::now();
      if (deadline == std::chrono::steady_clock::time_point{}) {
        deadline = now + std::chrono::milliseconds(limit_ms);
      } else if (now > deadline) {
        throw DeadlineExceeded(std::string(what) + " did not finish within " +
                               std::to_string(limit_ms) + " ms (AVR_FRAME_TIMEOUT_MS)");
      }
    }
  }
}

// Waits until everything queued on `stream` so far has finished.
void wait_stream_deadline(void* stream_v, const char* what) {
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  hipEvent_t event = nullptr;
  hip_check(hipEventCreateWithFlags(&event, hipEventDisableTiming), "hipEventCreate");
  const hipError_t recorded = hipEventRecord(event, stream);
  if (recorded != hipSuccess) {
    (void)hipEventDestroy(event);
    hip_check(recorded, what);
  }
  try {
    wait_event_deadline(event, what);
  } catch (const DeadlineExceeded&) {
    throw;  // the event is still pending on a stream that does not move: it is leaked, not destroyed
  } catch (...) {
    (void)hipEventDestroy(event);
    throw;
  }
  (void)hipEventDestroy(event);
}

}  // namespace avr

using avr::bind_device;
using avr::guarded;
using avr::require;

using avr::kClassify;
using avr::kMarch;

namespace {

constexpr avr::FrameKind kVolume = avr::FrameKind::kVolume;

// The shape of a frame call (avr::FrameChunks, avr_frame_launch.h, which says what the shapes are)
// with what only the device and the runtime can use: the caller's events and device arrays.
struct ChunkCall {
  int count = 1;
  hipEvent_t const* events = nullptr;  // count events, or null (both calls on one stream)
  bool first_alone = false;
  uint8_t* visibility = nullptr;       // avr_render_plan_culled: count * n_order bytes
  const uint8_t* classify_flags = nullptr;
  const uint32_t* classify_gate = nullptr;
  const int32_t* classify_positions = nullptr;
  int n_classify_positions = 0;
  const avr_speculation* speculation = nullptr;

  avr::FrameChunks shape() const {
    avr::FrameChunks host;
    host.count = count;
    host.first_alone = first_alone;
    host.events = events != nullptr;
    host.culled = visibility != nullptr;
    host.flags = classify_flags != nullptr;
    host.classify_positions = classify_positions;
    host.n_classify_positions = n_classify_positions;
    host.speculation = speculation;
    return host;
  }
};

using VolumeOut = avr::FoldOutputs<avr::FrameKind::kVolume>;
using MaxOut = avr::FoldOutputs<avr::FrameKind::kMaxIntensity>;
using SumOut = avr::FoldOutputs<avr::FrameKind::kProjection>;

// One frame's device work for a list of boxes: the classify pass and/or the march, queued on the
// context's stream.  Every rule, count, table and the list of launches is the frame's launch plan
// (avr_frame_launch.h, host only, tested without a GPU) -- it is also where a frame's kind enters
// the native layer, so what the kinds other than kVolume exclude is checked there and nowhere
// below.  What is left here needs the device: the scene's classified slot and its key, the staging
// of the plan's tables, the caller's addresses, and the launches and events in the plan's order.
int render(avr_context* ctx, avr_scene* scene, const avr::RenderRequest& frame,
           const ChunkCall& chunks = ChunkCall{}) {
  avr::FrameLaunchPlan& plan = ctx->frame_launch;
  if (!plan.open(frame, chunks.shape(), ctx->classify_lds_pad, ctx->classify_stream_stores,
                 ctx->march_workgroups_per_cu)) {
    return AVR_OK;
  }
  const int slot = frame.to.slot;
  uint8_t* classified =
      plan.needs_classified
          ? scene->classified_slot(slot, plan.prologue->classified_bytes, ctx->stream)
          : nullptr;
  if ((plan.phases & kClassify) && scene->cache_classification) {
    std::vector<uint64_t> key = avr::classification_key(*plan.prologue);
    if (key == scene->classified_key[slot]) {
      plan.phases &= ~kClassify;  // the slot already holds exactly this classification
      if (plan.phases == 0) return AVR_OK;
    } else {
      scene->classified_key[slot] = std::move(key);
    }
  }
  plan.finish();

  avr::RenderLaunch launch = plan.launch;
  avr::MarchSpecDev spec{};
  if (chunks.speculation != nullptr) spec = avr::speculation_record(*chunks.speculation);
  avr::stage_tables(ctx, plan, &launch, &spec);
  launch.classified = classified;
  launch.out_layers = frame.to.out_layers;
  launch.samples_out = reinterpret_cast<unsigned long long*>(frame.to.samples_out);
  launch.counters = reinterpret_cast<unsigned long long*>(ctx->march_counters);
  if (plan.flagged) {
    launch.visible_in = chunks.classify_flags;  // (null with positions: all of them)
    launch.classify_gate = chunks.classify_gate;
  }
  if (plan.phases & kMarch) ctx->last_only_mode = launch.only_mode;
  if (plan.visibility_bytes != 0) {
    avr::hip_check(hipMemsetAsync(chunks.visibility, 0, plan.visibility_bytes, ctx->stream),
                   "hipMemsetAsync(visibility)");
  }
  for (const avr::FrameStep& step : plan.steps) {
    if (step.wait_event >= 0) {
      avr::hip_check(hipStreamWaitEvent(ctx->stream, chunks.events[step.wait_event], 0),
                     "hipStreamWaitEvent(chunk)");
    }
    if (step.launches) {
      avr::RenderLaunch one = launch;
      step.apply(chunks.visibility, &one);
      const int status = step.march ? avr::launch_march(one, ctx->stream)
                                    : avr::launch_classify(one, ctx->stream);
      if (status != AVR_OK) return status;
    }
    if (step.record_event >= 0) {
      avr::hip_check(hipEventRecord(chunks.events[step.record_event], ctx->stream),
                     "hipEventRecord(chunk)");
    }
  }
  return AVR_OK;
}

// The run tables of a fold, staged in one batch: rectangles, blocks and, for a tightened plan, the
// blocks' rows (`spans` null or empty: none, and the launch's address stays null).
struct FoldTables {
  const std::vector<avr::RunRectDev>& rects;
  const std::vector<avr::RunBlockDev>& blocks;
  const std::vector<avr::RunSpanDev>* spans;
  template <class Visit>
  void visit_tables(avr::FoldLaunch* to, Visit&& visit) const {
    visit(&to->run_rects_dev, rects.data(), rects.size());
    visit(&to->run_blocks_dev, blocks.data(), blocks.size());
    if (spans != nullptr && !spans->empty()) visit(&to->run_spans_dev, spans->data(), spans->size());
  }
};
void stage_fold_tables(avr_context* ctx, const std::vector<avr::RunRectDev>& rects,
                       const std::vector<avr::RunBlockDev>& blocks,
                       const std::vector<avr::RunSpanDev>* spans, avr::FoldLaunch* launch) {
  launch->run_spans_dev = nullptr;
  avr::stage_tables(ctx, FoldTables{rects, blocks, spans}, launch);
}

}  // namespace

namespace avr {
void* context_stream(avr_context* ctx) {
  bind_device(ctx);
  return ctx->stream;
}
void context_set_classify_stream_stores(avr_context* ctx, bool stream) {
  ctx->classify_stream_stores = stream;
}
void context_set_lean_descriptors(avr_context* ctx, bool lean) { ctx->staging.set_lean(lean); }
void context_set_descriptor_lead(avr_context* ctx, int batches) { ctx->staging.set_ahead(batches); }
void context_set_fold_whole_grid(avr_context* ctx, bool whole) { ctx->fold_whole_grid = whole; }
}  // namespace avr

extern "C" {

const char* avr_last_error(void) { return avr::g_last_error.c_str(); }

int avr_abi_version(void) { return AVR_ABI_VERSION; }

int avr_debug_stall_stream(void* hip_stream, int milliseconds) {
  return guarded([&]() -> int {
    require(milliseconds >= 1 && milliseconds <= 2000, "milliseconds must be in [1, 2000]");
    return avr::launch_stall(milliseconds, hip_stream);
  });
}

int avr_set_frame_timeout_ms(int milliseconds) {
  avr::set_frame_timeout_ms(milliseconds);
  return AVR_OK;
}

int avr_context_create(int device_id, avr_context** out_ctx) {
  return guarded([&]() -> int {
    require(out_ctx != nullptr, "null out_ctx");
    *out_ctx = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
      avr::set_error("no HIP device available (this library has no CPU fallback)");
      return AVR_ERR_NO_DEVICE;
    }
    require(device_id >= 0 && device_id < count, "device_id out of range");
    avr::hip_check(hipSetDevice(device_id), "hipSetDevice");
    auto* ctx = new avr_context();
    ctx->device = device_id;
    ctx->stream = ctx->own_stream;
    *out_ctx = ctx;
    return AVR_OK;
  });
}

int avr_context_create_with_priority(int device_id, int high_priority, avr_context** out_ctx) {
  const int status = avr_context_create(device_id, out_ctx);
  if (status == AVR_OK) (*out_ctx)->priority = high_priority ? 1 : 0;
  return status;
}

void* avr_context_stream(avr_context* ctx) {
  try {
    return avr::context_stream(ctx);
  } catch (const std::exception& e) {
    avr::set_error(e.what());
    return nullptr;
  }
}

void avr_context_destroy(avr_context* ctx) {
  if (ctx == nullptr) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->own_stream != nullptr) (void)hipStreamSynchronize(ctx->own_stream);
  ctx->staging.release();
  ctx->max_layers.release();
  if (ctx->colorize_scratch != nullptr) (void)hipFree(ctx->colorize_scratch);
  ctx->axis_planes.release();
  ctx->gradient_planes.release();
  ctx->clump_parents.release();
  ctx->iso_scratch.release();
  ctx->group_counts.release();
  if (ctx->own_stream != nullptr) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

int avr_context_set_stream(avr_context* ctx, void* hip_stream) {
  return guarded([&]() -> int {
    require(ctx != nullptr, "null context");
    avr::hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->staging.drain();
    // NULL: back to the context's own stream (created on first use)
    ctx->stream = (hip_stream != nullptr) ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return AVR_OK;
  });
}

int avr_context_set_march_occupancy(avr_context* ctx, int workgroups_per_cu) {
  return guarded([&]() -> int {
    require(ctx != nullptr, "null context");
    require(workgroups_per_cu >= 0 && workgroups_per_cu <= 8, "workgroups_per_cu must be in [0, 8]");
    ctx->march_workgroups_per_cu = (workgroups_per_cu == 8) ? 0 : workgroups_per_cu;
    return AVR_OK;
  });
}

int avr_context_set_classify_lds_reserve(avr_context* ctx, int bytes) {
  return guarded([&]() -> int {
    require(ctx != nullptr, "null context");
    require(bytes >= 0 && bytes <= AVR_CLASSIFY_LDS_RESERVE_MAX,
            "bytes must be in [0, AVR_CLASSIFY_LDS_RESERVE_MAX]");
    ctx->classify_lds_pad = static_cast<uint32_t>(bytes);
    return AVR_OK;
  });
}

int avr_context_set_march_counters(avr_context* ctx, uint64_t* counters_dev) {
  return guarded([&]() -> int {
    require(ctx != nullptr, "null context");
    ctx->march_counters = counters_dev;
    return AVR_OK;
  });
}

int avr_context_last_march_mode(const avr_context* ctx, int* only_mode_out) {
  return guarded([&]() -> int {
    require(ctx != nullptr && only_mode_out != nullptr, "null argument");
    *only_mode_out = ctx->last_only_mode;
    return AVR_OK;
  });
}

int avr_context_synchronize(avr_context* ctx) {
  return guarded([&]() -> int {
    bind_device(ctx);
    avr::wait_stream(ctx->stream, "avr_context_synchronize");
    return AVR_OK;
  });
}

int avr_build_color_table(float alpha_scale, float normalization_factor,
                          const float scalar_range[2], const avr_colormap_point* colormap,
                          int colormap_count, float out_table_host[1024]) {
  return guarded([&]() -> int {
    require(scalar_range != nullptr && out_table_host != nullptr, "null argument");
    require(colormap_count >= 0 && (colormap_count == 0 || colormap != nullptr),
            "invalid color map");
    avr::build_color_table(alpha_scale, normalization_factor, scalar_range, colormap,
                           colormap_count, out_table_host);
    return AVR_OK;
  });
}

int avr_box_sampling(const avr_box* box, const avr_paint_params* params, float* sample_distance,
                     float* normalization_factor, float* alpha_scale) {
  return guarded([&]() -> int {
    require(box != nullptr && params != nullptr && sample_distance != nullptr &&
                normalization_factor != nullptr && alpha_scale != nullptr,
            "null argument");
    avr::box_sampling(*box, *params, sample_distance, normalization_factor, alpha_scale);
    return AVR_OK;
  });
}

int avr_box_depth_hint(const avr_box* box, const avr_camera* camera, float* out_hint) {
  return guarded([&]() -> int {
    require(box != nullptr && camera != nullptr && out_hint != nullptr, "null argument");
    *out_hint = avr::box_depth_hint(*box, *camera);
    return AVR_OK;
  });
}

int avr_reference_sample_distance(const avr_box* boxes, int n_boxes, const double bounds_min[3],
                                  const double bounds_max[3], float* out_distance) {
  return guarded([&]() -> int {
    require(n_boxes >= 0 && (n_boxes == 0 || boxes != nullptr), "invalid box list");
    require(bounds_min != nullptr && bounds_max != nullptr && out_distance != nullptr,
            "null argument");
    *out_distance = avr::reference_sample_distance(boxes, n_boxes, bounds_min, bounds_max);
    return AVR_OK;
  });
}

int avr_layer_order(const float* hints, const int32_t* owner, const int32_t* local_index,
                    int n_layers, int32_t* order_out, int32_t* run_end_out, int* n_runs_out) {
  return guarded([&]() -> int {
    require(n_layers >= 0 && n_runs_out != nullptr, "invalid argument");
    if (n_layers == 0) {
      *n_runs_out = 0;
      return AVR_OK;
    }
    require(hints != nullptr && owner != nullptr && local_index != nullptr &&
                order_out != nullptr && run_end_out != nullptr,
            "null argument");
    *n_runs_out = avr::layer_order(hints, owner, local_index, n_layers, order_out, run_end_out);
    return AVR_OK;
  });
}

int avr_piece_range(int64_t image_size, int piece_index, int num_pieces, int64_t* begin,
                    int64_t* end) {
  return guarded([&]() -> int {
    require(begin != nullptr && end != nullptr, "null argument");
    require(num_pieces >= 1 && piece_index >= 0 && piece_index < num_pieces && image_size >= 0,
            "invalid piece");
    const int64_t piece_size = image_size / num_pieces;
    *begin = piece_size * piece_index;
    *end = (piece_index < num_pieces - 1) ? (*begin + piece_size) : image_size;
    return AVR_OK;
  });
}

namespace {
// One box as one dense run in one contiguous piece: what the avr_paint_box calls render.
struct OneBoxRun {
  const int32_t order[1] = {0};
  const int32_t run_end[1] = {1};
  std::vector<avr::RunRectDev> rects;
  std::vector<avr::RunBlockDev> blocks;
  avr::PieceMapDev pieces;
};
int paint_one_box(avr_context* ctx, int phases, avr::FrameKind kind, const avr_box* box,
                  const avr_scalar_transform& transform, const avr_paint_params& params,
                  const avr_camera& camera, float* out_layers, uint64_t* samples_out,
                  OneBoxRun* run) {
  avr::dense_run_tables(params.width, params.height, 1, 1, &run->rects, &run->blocks);
  run->pieces = avr::make_piece_map(AVR_PIECES_CONTIGUOUS, 1, 1, params.width, params.height);
  return render(ctx, &ctx->scratch_scene,
                {phases, kind, {box, 1, transform, params, camera},
                 {run->order, 1, run->run_end, 1, 1, run->rects, run->blocks, nullptr, run->pieces},
                 {0, out_layers, samples_out, nullptr}});
}

// The same into the context's scratch layer (grown as needed), then the fold of that one run into
// `out`: a maximum-intensity index image or a projection's f64 images.
int paint_and_fold_one_box(avr_context* ctx, int phases, const avr_box* box,
                           const avr_scalar_transform& transform, const avr_paint_params& params,
                           const avr_camera& camera, uint64_t* samples_out, const avr::FoldOut& out) {
  require(params.width > 0 && params.height > 0, "image width and height must be positive");
  const int64_t n_pixels = static_cast<int64_t>(params.width) * params.height;
  const size_t bytes = static_cast<size_t>(n_pixels) * 5 * sizeof(float);
  ctx->max_layers.reserve(bytes, ctx->stream, "avr_paint_box (scratch layer)",
                          "hipMalloc(scratch layer)");
  float* layer = static_cast<float*>(ctx->max_layers.data);
  OneBoxRun run;
  const int status = paint_one_box(ctx, phases, static_cast<avr::FrameKind>(out.index()), box,
                                   transform, params, camera, layer, samples_out, &run);
  if (status != AVR_OK) return status;
  avr::FoldLaunch launch;
  stage_fold_tables(ctx, run.rects, run.blocks, nullptr, &launch);
  launch.pieces = run.pieces;
  launch.piece = 0;
  launch.width = params.width;
  launch.piece_begin = 0;
  launch.piece_end = n_pixels;
  launch.n_runs = 1;
  launch.recv = layer;
  launch.out = out;
  return avr::launch_fold_plan(launch, ctx->stream);
}
}  // namespace

int avr_paint_box(avr_context* ctx, const avr_box* box, const avr_scalar_transform* transform,
                  const avr_paint_params* params, const avr_camera* camera, float* out_rgbad,
                  uint64_t* samples_out) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(box != nullptr && transform != nullptr && params != nullptr && camera != nullptr,
            "null argument");
    require(params->width > 0 && params->height > 0, "image width and height must be positive");
    OneBoxRun run;
    return paint_one_box(ctx, kClassify | kMarch, kVolume, box, *transform, *params,
                         *camera, out_rgbad, samples_out, &run);
  });
}

int avr_paint_box_max(avr_context* ctx, const avr_box* box, const avr_scalar_transform* transform,
                      const avr_paint_params* params, const avr_camera* camera, int16_t* out_index,
                      uint64_t* samples_out) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(box != nullptr && transform != nullptr && params != nullptr && camera != nullptr &&
                out_index != nullptr,
            "null argument");
    // the layer -> index image: the max fold over the one run
    return paint_and_fold_one_box(ctx, kClassify | kMarch, box, *transform, *params, *camera,
                                  samples_out, MaxOut{out_index, nullptr});
  });
}

int avr_paint_box_projection(avr_context* ctx, const avr_box* box, const avr_paint_params* params,
                             const avr_camera* camera, double* column, double* length,
                             uint64_t* samples_out) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(box != nullptr && params != nullptr && camera != nullptr && column != nullptr &&
                length != nullptr,
            "null argument");
    const avr_scalar_transform transform{};  // (no classify pass: the raw values are summed)
    // the layer -> f64 images: the sum fold over the one run (a pixel no box covers stays 0)
    return paint_and_fold_one_box(ctx, kMarch, box, transform, *params, *camera, samples_out,
                                  SumOut{column, length});
  });
}

int avr_projection_colorize(avr_context* ctx, const double* column, const double* length, int width,
                            int height, int quantity, int log_scale, double* range, int auto_range,
                            const uint8_t* rgb_table, uint8_t* rgb8_out) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(column != nullptr && length != nullptr && range != nullptr && rgb_table != nullptr &&
                rgb8_out != nullptr,
            "null argument");
    require(width > 0 && height > 0, "image width and height must be positive");
    require(quantity == AVR_PROJECTION_COLUMN || quantity == AVR_PROJECTION_MEAN, "unknown quantity");
    if (auto_range && ctx->colorize_scratch == nullptr) {
      void* block = nullptr;
      avr::hip_check(hipMalloc(&block, 2 * avr::kProjectionRangeWorkgroups * sizeof(double)),
                     "hipMalloc(projection range)");
      ctx->colorize_scratch = static_cast<double*>(block);
    }
    return avr::launch_projection_colorize(column, length, width, height,
                                           quantity == AVR_PROJECTION_MEAN ? 1 : 0,
                                           log_scale ? 1 : 0, range, auto_range ? 1 : 0,
                                           ctx->colorize_scratch, rgb_table, rgb8_out, ctx->stream);
  });
}

int avr_scene_create(avr_context* ctx, const avr_box* boxes, int n_boxes,
                     const avr_scalar_transform* transform, avr_scene** out_scene) {
  return guarded([&]() -> int {
    require(ctx != nullptr && out_scene != nullptr && transform != nullptr, "null argument");
    require(n_boxes >= 0 && (n_boxes == 0 || boxes != nullptr), "invalid box list");
    auto* scene = new avr_scene();
    scene->ctx = ctx;
    scene->boxes.assign(boxes, boxes + n_boxes);
    scene->transform = *transform;
    *out_scene = scene;
    return AVR_OK;
  });
}

void avr_scene_destroy(avr_scene* scene) { delete scene; }

int avr_render_runs(avr_context* ctx, const avr_scene* scene, const avr_paint_params* params,
                    const avr_camera* camera, const int32_t* box_order, int n_order,
                    const int32_t* run_end, int n_runs, int n_pieces, float* out_layers,
                    uint64_t* samples_out) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(scene != nullptr && params != nullptr && camera != nullptr, "null argument");
    require(n_runs >= 0 && n_pieces >= 1, "invalid run description");
    require(params->width > 0 && params->height > 0, "image width and height must be positive");
    std::vector<avr::RunRectDev> rects;
    std::vector<avr::RunBlockDev> blocks;
    avr::dense_run_tables(params->width, params->height, n_runs, n_pieces, &rects, &blocks);
    const avr::PieceMapDev pieces =
        avr::make_piece_map(AVR_PIECES_CONTIGUOUS, 1, n_pieces, params->width, params->height);
    return render(ctx, const_cast<avr_scene*>(scene),
                  {kClassify | kMarch, kVolume,
                   {scene->boxes.data(), static_cast<int>(scene->boxes.size()), scene->transform,
                    *params, *camera},
                   {box_order, n_order, run_end, n_runs, n_pieces, rects, blocks, nullptr, pieces},
                   {0, out_layers, samples_out, nullptr}});
  });
}

int avr_frame_plan_create_pieces(const avr_box* all_boxes, const int32_t* owner, int n_boxes,
                                 int n_ranks, int rank, const int32_t* group_order,
                                 const avr_paint_params* params, const avr_camera* camera,
                                 int piece_layout, int band_rows, avr_frame_plan** out_plan) {
  return guarded([&]() -> int {
    require(out_plan != nullptr && params != nullptr && camera != nullptr, "null argument");
    *out_plan = nullptr;
    require(params->colormap_count >= 0 && (params->colormap_count == 0 || params->colormap),
            "invalid color map");
    auto* plan = new avr_frame_plan();
    try {
      avr::build_frame_plan(all_boxes, owner, n_boxes, n_ranks, rank, group_order, *params, *camera,
                            piece_layout, band_rows, plan);
    } catch (...) {
      delete plan;
      throw;
    }
    *out_plan = plan;
    return AVR_OK;
  });
}

int avr_frame_plan_create(const avr_box* all_boxes, const int32_t* owner, int n_boxes, int n_ranks,
                          int rank, const int32_t* group_order, const avr_paint_params* params,
                          const avr_camera* camera, avr_frame_plan** out_plan) {
  return avr_frame_plan_create_pieces(all_boxes, owner, n_boxes, n_ranks, rank, group_order, params,
                                      camera, AVR_PIECES_CONTIGUOUS, 1, out_plan);
}

int avr_layered_plan_create(const float* hints, const int32_t* owner, int n_layers, int n_ranks,
                            int rank, const int32_t* group_order, int width, int height,
                            avr_frame_plan** out_plan) {
  return guarded([&]() -> int {
    require(out_plan != nullptr, "null argument");
    *out_plan = nullptr;
    auto* plan = new avr_frame_plan();
    try {
      plan->params.width = width;
      plan->params.height = height;
      avr::build_layer_plan(n_layers, hints, owner, nullptr, n_ranks, rank, group_order, width,
                            height, AVR_PIECES_CONTIGUOUS, 1, plan);
    } catch (...) {
      delete plan;
      throw;
    }
    *out_plan = plan;
    return AVR_OK;
  });
}

int avr_pack_layers(avr_context* ctx, const avr_frame_plan* plan, const float* const* local_layers,
                    int n_local_layers, float* send_buffer) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(plan != nullptr, "null plan");
    require(n_local_layers == plan->info.n_local_boxes, "layer count does not match the plan");
    require(n_local_layers == 0 || local_layers != nullptr, "null layer list");
    require(plan->info.send_floats == 0 || send_buffer != nullptr, "null send buffer");
    require(plan->pieces.layout == avr::kPiecesContiguous,
            "avr_pack_layers needs the reference's contiguous pieces");
    const int n_ranks = plan->info.n_ranks;
    const int64_t width = plan->params.width;
    int start = 0;
    std::vector<const float*> slices;
    for (int r = 0; r < plan->info.n_local_runs; ++r) {
      const int end = plan->local_run_end[static_cast<size_t>(r)];
      const avr::RunRectDev& rect = plan->local_rects[static_cast<size_t>(r)];
      require(rect.x0 == 0 && rect.x1 == width - 1, "avr_pack_layers needs a full-width layered plan");
      for (int piece = 0; piece < n_ranks; ++piece) {
        const size_t at = static_cast<size_t>(r) * n_ranks + static_cast<size_t>(piece);
        const int rows = plan->send_block_rows[at];
        if (rows == 0) continue;
        const int64_t first_pixel = static_cast<int64_t>(plan->send_blocks[at].first_row) * width;
        slices.clear();
        for (int l = start; l < end; ++l) {
          const int32_t local = plan->local_order[static_cast<size_t>(l)];
          require(local >= 0 && local < n_local_layers && local_layers[local] != nullptr,
                  "invalid local layer");
          slices.push_back(local_layers[local] + first_pixel * 5);
        }
        // owner-side fold of the run's layers, in order (DirectSendBase.cpp:413-426), over the
        // block's whole rows
        ctx->staging.begin(slices.size() * sizeof(float*), 1);
        const float* const* slices_dev = ctx->staging.add(slices.data(), slices.size());
        ctx->staging.commit(ctx->stream);
        const int status = avr::launch_fold_runs(slices_dev, static_cast<int>(slices.size()),
                                                 send_buffer + plan->send_blocks[at].offset,
                                                 static_cast<int64_t>(rows) * width, ctx->stream);
        if (status != AVR_OK) return status;
      }
      start = end;
    }
    return AVR_OK;
  });
}

void avr_frame_plan_destroy(avr_frame_plan* plan) { delete plan; }

int avr_frame_plan_get_info(const avr_frame_plan* plan, avr_frame_plan_info* out) {
  return guarded([&]() -> int {
    require(plan != nullptr && out != nullptr, "null argument");
    *out = plan->info;
    return AVR_OK;
  });
}

int avr_frame_plan_splits(const avr_frame_plan* plan, int64_t* send_splits, int64_t* recv_splits) {
  return guarded([&]() -> int {
    require(plan != nullptr && send_splits != nullptr && recv_splits != nullptr, "null argument");
    std::copy(plan->send_splits.begin(), plan->send_splits.end(), send_splits);
    std::copy(plan->recv_splits.begin(), plan->recv_splits.end(), recv_splits);
    return AVR_OK;
  });
}

int avr_frame_plan_layers(const avr_frame_plan* plan, int32_t* layer_box) {
  return guarded([&]() -> int {
    require(plan != nullptr && (plan->layer_box.empty() || layer_box != nullptr), "null argument");
    std::copy(plan->layer_box.begin(), plan->layer_box.end(), layer_box);
    return AVR_OK;
  });
}

int avr_frame_plan_runs(const avr_frame_plan* plan, avr_run_info* runs) {
  return guarded([&]() -> int {
    require(plan != nullptr && (plan->runs.empty() || runs != nullptr), "null argument");
    std::copy(plan->runs.begin(), plan->runs.end(), runs);
    return AVR_OK;
  });
}

int avr_box_footprint(const avr_box* box, const avr_camera* camera, int width, int height,
                      int32_t rect[4], int32_t* row_x0, int32_t* row_x1) {
  return guarded([&]() -> int {
    require(box != nullptr && camera != nullptr && rect != nullptr, "null argument");
    require(width > 0 && height > 0, "image width and height must be positive");
    require((row_x0 == nullptr) == (row_x1 == nullptr), "row_x0 and row_x1 go together");
    avr::box_screen_rect(*box, *camera, width, height, rect);
    if (row_x0 == nullptr) return AVR_OK;
    for (int y = 0; y < height; ++y) {
      row_x0[y] = 0;
      row_x1[y] = -1;
    }
    std::vector<int32_t> x0, x1;
    avr::box_row_spans(*box, *camera, width, height, rect, &x0, &x1);
    for (size_t r = 0; r < x0.size(); ++r) {
      row_x0[rect[1] + static_cast<int>(r)] = x0[r];
      row_x1[rect[1] + static_cast<int>(r)] = x1[r];
    }
    return AVR_OK;
  });
}

int avr_frame_plan_tighten(avr_frame_plan* plan, const avr_box* all_boxes, int n_boxes) {
  return guarded([&]() -> int {
    require(plan != nullptr && n_boxes >= 0 && (n_boxes == 0 || all_boxes != nullptr),
            "invalid argument");
    avr::tighten_frame_plan(all_boxes, n_boxes, plan);
    return AVR_OK;
  });
}

int avr_frame_plan_send_block(const avr_frame_plan* plan, int peer, int local_run, int64_t* offset,
                              int32_t* first_row, int32_t* n_rows) {
  return guarded([&]() -> int {
    require(plan != nullptr && offset != nullptr && first_row != nullptr && n_rows != nullptr,
            "null argument");
    require(peer >= 0 && peer < plan->info.n_ranks && local_run >= 0 &&
                local_run < plan->info.n_local_runs,
            "block index out of range");
    require(!plan->tightened, "a tightened plan has no rectangular blocks");
    const size_t at = static_cast<size_t>(local_run) * plan->info.n_ranks +
                      static_cast<size_t>(plan->piece_of_rank[static_cast<size_t>(peer)]);
    *n_rows = plan->send_block_rows[at];
    *first_row = plan->send_blocks[at].first_row;
    *offset = (*n_rows > 0) ? plan->send_blocks[at].offset : -1;
    return AVR_OK;
  });
}

int avr_frame_plan_recv_block(const avr_frame_plan* plan, int global_run, int64_t* offset,
                              int32_t* first_row, int32_t* n_rows) {
  return guarded([&]() -> int {
    require(plan != nullptr && offset != nullptr && first_row != nullptr && n_rows != nullptr,
            "null argument");
    require(global_run >= 0 && global_run < plan->info.n_runs_total, "run index out of range");
    require(!plan->tightened, "a tightened plan has no rectangular blocks");
    const size_t at = static_cast<size_t>(global_run);
    *n_rows = plan->recv_block_rows[at];
    *first_row = plan->recv_blocks[at].first_row;
    *offset = (*n_rows > 0) ? plan->recv_blocks[at].offset : -1;
    return AVR_OK;
  });
}

static int plan_phase(avr_context* ctx, int phases, avr::FrameKind kind, const avr_scene* scene,
                      const avr_frame_plan* plan, int slot, float* send_buffer,
                      uint64_t* samples_out, const ChunkCall& chunks = ChunkCall{}) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(scene != nullptr && plan != nullptr, "null argument");
    require(chunks.count == 1 || !scene->cache_classification,
            "a cached classification is not classified in chunks");
    require((chunks.classify_flags == nullptr && chunks.classify_positions == nullptr) ||
                !scene->cache_classification,
            "a cached classification is not classified by flags");
    require(static_cast<int>(scene->boxes.size()) == plan->info.n_local_boxes,
            "the scene does not hold this rank's boxes of the plan");
    if (plan->info.n_local_runs == 0) return AVR_OK;
    return render(ctx, const_cast<avr_scene*>(scene),
                  {phases, kind,
                   {scene->boxes.data(), static_cast<int>(scene->boxes.size()), scene->transform,
                    plan->params, plan->camera},
                   {plan->local_order.data(), static_cast<int>(plan->local_order.size()),
                    plan->local_run_end.data(), plan->info.n_local_runs, plan->info.n_ranks,
                    plan->local_rects, plan->send_blocks,
                    ((phases & kMarch) && plan->tightened) ? &plan->send_spans : nullptr, plan->pieces},
                   {slot, send_buffer, samples_out, &const_cast<avr_frame_plan*>(plan)->prologue}},
                  chunks);
  });
}

int avr_scene_set_classification_cache(avr_scene* scene, int enabled) {
  return guarded([&]() -> int {
    require(scene != nullptr, "null scene");
    scene->cache_classification = enabled != 0;
    for (auto& key : scene->classified_key) key.clear();
    return AVR_OK;
  });
}

int avr_scene_invalidate(avr_scene* scene) {
  return guarded([&]() -> int {
    require(scene != nullptr, "null scene");
    for (auto& key : scene->classified_key) key.clear();
    return AVR_OK;
  });
}

int avr_render_plan(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan,
                    float* send_buffer, uint64_t* samples_out) {
  return plan_phase(ctx, kClassify | kMarch, kVolume, scene, plan, 0, send_buffer, samples_out);
}

int avr_render_plan_max(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan,
                        float* send_buffer, uint64_t* samples_out) {
  return plan_phase(ctx, kClassify | kMarch, avr::FrameKind::kMaxIntensity, scene, plan, 0,
                    send_buffer, samples_out);
}

int avr_march_plan_max(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan, int slot,
                       float* send_buffer, uint64_t* samples_out) {
  return plan_phase(ctx, kMarch, avr::FrameKind::kMaxIntensity, scene, plan, slot, send_buffer,
                    samples_out);
}

int avr_render_plan_projection(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan,
                               float* send_buffer, uint64_t* samples_out) {
  return plan_phase(ctx, kMarch, avr::FrameKind::kProjection, scene, plan, 0, send_buffer,
                    samples_out);
}

int avr_march_plan_projection(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan,
                              int slot, float* send_buffer, uint64_t* samples_out) {
  return plan_phase(ctx, kMarch, avr::FrameKind::kProjection, scene, plan, slot, send_buffer,
                    samples_out);
}

int avr_classify_plan(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan,
                      int slot) {
  return plan_phase(ctx, kClassify, kVolume, scene, plan, slot, nullptr, nullptr);
}

int avr_march_plan(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan, int slot,
                   float* send_buffer, uint64_t* samples_out) {
  return plan_phase(ctx, kMarch, kVolume, scene, plan, slot, send_buffer, samples_out);
}

int avr_classify_plan_chunked(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan,
                              int slot, int n_chunks, void* const* chunk_events, int first_alone) {
  ChunkCall chunks;
  chunks.count = n_chunks;
  chunks.events = reinterpret_cast<hipEvent_t const*>(chunk_events);
  chunks.first_alone = first_alone != 0;
  return plan_phase(ctx, kClassify, kVolume, scene, plan, slot, nullptr, nullptr, chunks);
}

int avr_march_plan_chunked(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan,
                           int slot, float* send_buffer, uint64_t* samples_out, int n_chunks,
                           void* const* chunk_events) {
  ChunkCall chunks;
  chunks.count = n_chunks;
  chunks.events = reinterpret_cast<hipEvent_t const*>(chunk_events);
  return plan_phase(ctx, kMarch, kVolume, scene, plan, slot, send_buffer, samples_out, chunks);
}

int avr_classify_plan_flagged(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan,
                              int slot, const uint8_t* flags, const uint32_t* gate) {
  return guarded([&]() -> int {
    require(flags != nullptr, "null flags");
    ChunkCall chunks;
    chunks.classify_flags = flags;
    chunks.classify_gate = gate;
    return plan_phase(ctx, kClassify, kVolume, scene, plan, slot, nullptr, nullptr, chunks);
  });
}

int avr_march_plan_workgroups(const avr_frame_plan* plan, int64_t* workgroups) {
  return guarded([&]() -> int {
    require(plan != nullptr && workgroups != nullptr, "null argument");
    *workgroups = avr::march_workgroups_bound(plan->params.width, plan->params.height, plan->info.n_local_runs);
    return AVR_OK;
  });
}

int avr_classify_plan_positions(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan,
                                int slot, const int32_t* positions, int n_positions) {
  return guarded([&]() -> int {
    require(positions != nullptr && n_positions >= 0, "null positions");
    if (n_positions == 0) return AVR_OK;
    ChunkCall chunks;
    chunks.classify_positions = positions;
    chunks.n_classify_positions = n_positions;
    return plan_phase(ctx, kClassify, kVolume, scene, plan, slot, nullptr, nullptr, chunks);
  });
}

int avr_march_plan_speculative(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan,
                               int slot, float* send_buffer, const avr_speculation* speculation) {
  return guarded([&]() -> int {
    require(speculation != nullptr, "null speculation");
    ChunkCall chunks;
    chunks.speculation = speculation;
    return plan_phase(ctx, kMarch, kVolume, scene, plan, slot, send_buffer, nullptr, chunks);
  });
}

int avr_render_plan_culled(avr_context* ctx, const avr_scene* scene, const avr_frame_plan* plan,
                           int slot, float* send_buffer, uint64_t* samples_out, int n_chunks,
                           uint8_t* visibility) {
  return guarded([&]() -> int {
    require(visibility != nullptr && n_chunks >= 2, "a culled frame needs chunks and a visibility buffer");
    ChunkCall chunks;
    chunks.count = n_chunks;
    chunks.visibility = visibility;
    chunks.first_alone = true;
    return plan_phase(ctx, kClassify | kMarch, kVolume, scene, plan, slot, send_buffer, samples_out,
                      chunks);
  });
}

int avr_fold_plan(avr_context* ctx, const avr_frame_plan* plan, const float* recv_buffer,
                  float* out_piece, uint8_t* out_rgb8) {
  return avr_fold_plan_own(ctx, plan, recv_buffer, nullptr, out_piece, out_rgb8);
}

namespace {
// to_image (one rank, volume and maximum-intensity frames): the RGB8 output is the whole image,
// rows top-down.
int fold_plan(avr_context* ctx, const avr_frame_plan* plan, const float* recv_buffer,
              const float* own_send_buffer, const avr::FoldOut& out, bool to_image = false);
}

int avr_fold_plan_own(avr_context* ctx, const avr_frame_plan* plan, const float* recv_buffer,
                      const float* own_send_buffer, float* out_piece, uint8_t* out_rgb8) {
  return fold_plan(ctx, plan, recv_buffer, own_send_buffer, VolumeOut{out_piece, out_rgb8});
}

int avr_fold_plan_image(avr_context* ctx, const avr_frame_plan* plan, const float* recv_buffer,
                        float* out_piece, uint8_t* out_rgb8_image) {
  return fold_plan(ctx, plan, recv_buffer, nullptr, VolumeOut{out_piece, out_rgb8_image}, true);
}

int avr_fold_plan_max(avr_context* ctx, const avr_frame_plan* plan, const float* recv_buffer,
                      int16_t* out_index, uint8_t* out_rgb8) {
  return fold_plan(ctx, plan, recv_buffer, nullptr, MaxOut{out_index, out_rgb8});
}

int avr_fold_plan_own_max(avr_context* ctx, const avr_frame_plan* plan, const float* recv_buffer,
                          const float* own_send_buffer, int16_t* out_index, uint8_t* out_rgb8) {
  return fold_plan(ctx, plan, recv_buffer, own_send_buffer, MaxOut{out_index, out_rgb8});
}

int avr_fold_plan_image_max(avr_context* ctx, const avr_frame_plan* plan, const float* recv_buffer,
                            int16_t* out_index, uint8_t* out_rgb8_image) {
  return fold_plan(ctx, plan, recv_buffer, nullptr, MaxOut{out_index, out_rgb8_image}, true);
}

int avr_fold_plan_projection(avr_context* ctx, const avr_frame_plan* plan, const float* recv_buffer,
                             double* out_column, double* out_length) {
  return fold_plan(ctx, plan, recv_buffer, nullptr, SumOut{out_column, out_length});
}

int avr_fold_plan_own_projection(avr_context* ctx, const avr_frame_plan* plan, const float* recv_buffer,
                                 const float* own_send_buffer, double* out_column, double* out_length) {
  return fold_plan(ctx, plan, recv_buffer, own_send_buffer, SumOut{out_column, out_length});
}

int avr_fold_plan_image_projection(avr_context* ctx, const avr_frame_plan* plan,
                                   const float* recv_buffer, double* out_column, double* out_length) {
  if (plan != nullptr && plan->info.n_ranks != 1) {
    avr::set_error("avr_fold_plan_image_projection is for one rank's whole image");
    return AVR_ERR_INVALID_ARGUMENT;
  }
  return fold_plan(ctx, plan, recv_buffer, nullptr, SumOut{out_column, out_length});
}

namespace {
int fold_plan(avr_context* ctx, const avr_frame_plan* plan, const float* recv_buffer,
              const float* own_send_buffer, const avr::FoldOut& out, bool to_image) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(plan != nullptr, "null argument");
    const bool has_rgb8 = std::visit(
        [](auto o) { return std::is_same_v<decltype(o.second), uint8_t*> && o.second != nullptr; }, out);
    require(!to_image || (plan->info.n_ranks == 1 && has_rgb8),
            "avr_fold_plan_image is for one rank's whole image");
    // (a rank whose piece is empty -- more ranks than pixels, or row bands on a short image --
    // has nothing to fold and may pass empty buffers)
    if (plan->info.piece_end <= plan->info.piece_begin) return AVR_OK;
    require(std::visit([](auto o) { return o.first != nullptr || o.second != nullptr; }, out),
            "null argument");
    require(plan->info.recv_floats == 0 || recv_buffer != nullptr, "null receive buffer");
    avr::FoldLaunch launch;
    stage_fold_tables(ctx, plan->global_rects, plan->recv_blocks,
                      plan->tightened ? &plan->recv_spans : nullptr, &launch);
    launch.pieces = plan->pieces;
    launch.piece = plan->piece_of_rank[static_cast<size_t>(plan->info.rank)];
    launch.width = plan->params.width;
    launch.piece_begin = plan->info.piece_begin;
    launch.piece_end = plan->info.piece_end;
    launch.n_runs = plan->info.n_runs_total;
    launch.recv = recv_buffer;
    launch.out = out;
    // One rank folds the whole image while the next frame's paint kernels start, and nothing
    // waits for it: one workgroup per CU keeps it out of their way (0.997 -> 0.980 ms per frame).
    // A rank of several folds its piece on the stream that also carries the exchange and the
    // gather, five kernels per frame: there it should be through quickly.
    // (A frame that found its renderer's pipeline empty has nothing to stay out of the way of,
    // and somebody is waiting for it: the whole grid, 63 -> ~15 us for 2048^2.)
    launch.max_workgroups = (plan->info.n_ranks == 1 && !ctx->fold_whole_grid) ? 256 : 0;
    {
      static const int forced = [] {  // A/B only (tools/ab_env_share.sh)
        const char* text = std::getenv("AVR_FOLD_WORKGROUPS");
        return text != nullptr ? std::atoi(text) : 0;
      }();
      if (forced > 0) launch.max_workgroups = forced;
    }
    launch.flip_height = to_image ? plan->params.height : 0;
    if (own_send_buffer != nullptr) {
      // the rank's block for itself: where the receive layout has it and where the march put it
      const int me = plan->info.rank;
      int64_t send_at = 0, recv_at = 0;
      for (int s = 0; s < me; ++s) {
        send_at += plan->send_splits[static_cast<size_t>(s)];
        recv_at += plan->recv_splits[static_cast<size_t>(s)];
      }
      const int64_t own = plan->recv_splits[static_cast<size_t>(me)];
      if (plan->send_splits[static_cast<size_t>(me)] != own) {
        throw std::runtime_error(
            "frame plan: a rank's block for itself differs between send and receive layout");
      }
      launch.own_begin = recv_at;
      launch.own_end = recv_at + own;
      // (two allocations: the distance is taken between addresses, not between pointers)
      launch.own_delta = (reinterpret_cast<intptr_t>(own_send_buffer + send_at) -
                          reinterpret_cast<intptr_t>(recv_buffer + recv_at)) /
                         static_cast<intptr_t>(sizeof(float));
    }
    return avr::launch_fold_plan(launch, ctx->stream);
  });
}
}  // namespace

int avr_visibility_graph_create(const avr_box* all_boxes, const int32_t* owner, int n_boxes,
                                int n_ranks, avr_visibility_graph** out_graph) {
  return guarded([&]() -> int {
    require(out_graph != nullptr, "null out_graph");
    *out_graph = nullptr;
    require(n_ranks >= 1, "n_ranks must be positive");
    require(n_boxes >= 0 && (n_boxes == 0 || (all_boxes != nullptr && owner != nullptr)),
            "invalid box list");
    for (int b = 0; b < n_boxes; ++b) {
      require(owner[b] >= 0 && owner[b] < n_ranks, "box owner out of range");
    }
    *out_graph = avr::visibility_graph_create(all_boxes, owner, n_boxes, n_ranks);
    return AVR_OK;
  });
}

void avr_visibility_graph_destroy(avr_visibility_graph* graph) {
  avr::visibility_graph_destroy(graph);
}

int avr_visibility_order(avr_visibility_graph* graph, const avr_camera* camera, float aspect,
                         int use_visibility_graph, const char* dot_prefix,
                         int32_t* rank_order_out, int* succeeded_out, int* n_splits_out) {
  return guarded([&]() -> int {
    require(graph != nullptr && camera != nullptr && rank_order_out != nullptr, "null argument");
    if (succeeded_out != nullptr) *succeeded_out = 1;
    if (n_splits_out != nullptr) *n_splits_out = 0;
    if (!use_visibility_graph) {
      const int n = avr::visibility_rank_count(graph);
      for (int r = 0; r < n; ++r) rank_order_out[r] = r;
      return AVR_OK;
    }
    const bool ok = avr::visibility_order(graph, *camera, aspect, dot_prefix, rank_order_out,
                                          n_splits_out);
    if (succeeded_out != nullptr) *succeeded_out = ok ? 1 : 0;
    return AVR_OK;
  });
}

int avr_tight_bounds(const avr_box* all_boxes, int n_boxes, const double fallback_min[3],
                     const double fallback_max[3], double out_min[3], double out_max[3]) {
  return guarded([&]() -> int {
    require(n_boxes >= 0 && (n_boxes == 0 || all_boxes != nullptr), "invalid box list");
    require(fallback_min != nullptr && fallback_max != nullptr && out_min != nullptr &&
                out_max != nullptr, "null argument");
    avr::tight_bounds(all_boxes, n_boxes, fallback_min, fallback_max, out_min, out_max);
    return AVR_OK;
  });
}

int avr_bbox_overlay(avr_context* ctx, const double bounds_min[3], const double bounds_max[3],
                     const avr_camera* camera, int sqrt_antialiasing, int width, int height,
                     int64_t pixel_begin, int64_t pixel_end, float* image, uint8_t* rgb8) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(bounds_min != nullptr && bounds_max != nullptr && camera != nullptr, "null argument");
    if (width <= 0 || height <= 0) return AVR_OK;  // VolumeRenderer.cpp:145-147
    require(pixel_begin >= 0 && pixel_begin <= pixel_end &&
                pixel_end <= static_cast<int64_t>(width) * height, "invalid pixel range");
    if (pixel_end == pixel_begin) return AVR_OK;
    require(image != nullptr, "null image");
    avr::OverlayPlan plan;
    avr::plan_overlay(bounds_min, bounds_max, *camera, sqrt_antialiasing, width, height, &plan);
    return avr::launch_overlay(plan, width, pixel_begin, pixel_end, nullptr, 0, image, rgb8,
                               ctx->stream);
  });
}

int avr_bbox_overlay_piece(avr_context* ctx, const avr_frame_plan* plan, const double bounds_min[3],
                           const double bounds_max[3], const avr_camera* camera, float* piece,
                           uint8_t* rgb8) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(plan != nullptr && bounds_min != nullptr && bounds_max != nullptr && camera != nullptr,
            "null argument");
    const int64_t begin = plan->info.piece_begin, end = plan->info.piece_end;
    if (end <= begin) return AVR_OK;
    require(piece != nullptr, "null image");
    avr::OverlayPlan overlay;
    avr::plan_overlay(bounds_min, bounds_max, *camera, 1, plan->params.width, plan->params.height,
                      &overlay);
    return avr::launch_overlay(overlay, plan->params.width, begin, end, &plan->pieces,
                               plan->piece_of_rank[static_cast<size_t>(plan->info.rank)], piece,
                               rgb8, ctx->stream);
  });
}

int avr_assemble_rows(avr_context* ctx, const avr_frame_plan* plan, const void* gathered,
                      int bytes_per_pixel, int flip, void* image) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(plan != nullptr && bytes_per_pixel > 0, "invalid argument");
    if (plan->info.n_pixels == 0) return AVR_OK;
    require(gathered != nullptr && image != nullptr && gathered != image, "invalid image pointers");
    return avr::launch_assemble_rows(plan->pieces, static_cast<const uint8_t*>(gathered),
                                     static_cast<int64_t>(plan->params.width) * bytes_per_pixel,
                                     flip, static_cast<uint8_t*>(image), ctx->stream);
  });
}

int avr_assemble_rows_own(avr_context* ctx, const avr_frame_plan* plan, const void* gathered,
                          const void* own_piece, int bytes_per_pixel, int flip, void* image) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(plan != nullptr && bytes_per_pixel > 0, "invalid argument");
    if (plan->info.n_pixels == 0) return AVR_OK;
    require(gathered != nullptr && image != nullptr && gathered != image, "invalid image pointers");
    const int mine = plan->piece_of_rank[static_cast<size_t>(plan->info.rank)];
    return avr::launch_assemble_rows(plan->pieces, static_cast<const uint8_t*>(gathered),
                                     static_cast<int64_t>(plan->params.width) * bytes_per_pixel,
                                     flip, static_cast<uint8_t*>(image), ctx->stream,
                                     static_cast<const uint8_t*>(own_piece), mine);
  });
}

namespace {
// The box records and tile prefix of a scan over every cell of `scene`, staged on the context.
struct StagedCells {
  avr::FramePlan plan;
  const avr::BoxDev* boxes_dev = nullptr;
  const uint32_t* tiles_dev = nullptr;
};
void stage_cells(avr_context* ctx, const avr_scene* scene, const avr_scalar_transform& transform,
                 StagedCells* cells) {
  avr::FramePlan& plan = cells->plan;
  avr::plan_cells(scene->boxes.data(), static_cast<int>(scene->boxes.size()), transform, &plan);
  ctx->staging.begin(plan.boxes.size() * sizeof(avr::BoxDev) +
                         plan.classify_tile_begin.size() * sizeof(uint32_t), 2);
  cells->boxes_dev = ctx->staging.add(plan.boxes.data(), plan.boxes.size());
  cells->tiles_dev =
      ctx->staging.add(plan.classify_tile_begin.data(), plan.classify_tile_begin.size());
  ctx->staging.commit(ctx->stream);
}
}  // namespace

int avr_scene_scalar_stats(avr_context* ctx, const avr_scene* scene, double stats_host[3],
                           int64_t* finite_count_host) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(scene != nullptr && stats_host != nullptr && finite_count_host != nullptr,
            "null argument");
    void* scratch = nullptr;
    avr::hip_check(hipMalloc(&scratch, (static_cast<size_t>(avr::kScanWorkgroups) + 1) * 32),
                   "hipMalloc");
    struct { double lo, hi, lo_positive; long long finite; } result{};
    int status = AVR_OK;
    try {
      StagedCells cells;
      stage_cells(ctx, scene, scene->transform, &cells);
      char* out_dev = static_cast<char*>(scratch) + static_cast<size_t>(avr::kScanWorkgroups) * 32;
      status = avr::launch_scalar_stats(cells.boxes_dev, cells.tiles_dev,
                                        static_cast<int>(cells.plan.boxes.size()),
                                        cells.plan.classify_tile_begin.back(), scratch, out_dev,
                                        ctx->stream);
      if (status == AVR_OK) {
        avr::hip_check(hipMemcpyAsync(&result, out_dev, sizeof(result), hipMemcpyDeviceToHost,
                                      ctx->stream), "hipMemcpyAsync");
        avr::wait_stream(ctx->stream, "avr_scene_scalar_stats");
      }
    } catch (...) {
      (void)hipFree(scratch);
      throw;
    }
    (void)hipFree(scratch);
    stats_host[0] = result.lo;
    stats_host[1] = result.hi;
    stats_host[2] = result.lo_positive;
    *finite_count_host = result.finite;
    return status;
  });
}

int avr_scene_transform_from_stats(const double stats[3], int64_t finite_count, int log_scale,
                                   int normalize_to_data_range, avr_scalar_transform* transform,
                                   double processed[2], float processed_range[2],
                                   float scalar_range[2]) {
  return guarded([&]() -> int {
    require(stats != nullptr && transform != nullptr && processed != nullptr &&
                processed_range != nullptr && scalar_range != nullptr, "null argument");
    avr::scene_transform_from_stats(stats, finite_count, log_scale != 0,
                                    normalize_to_data_range != 0, transform, processed,
                                    processed_range, scalar_range);
    return AVR_OK;
  });
}

int avr_scene_histogram(avr_context* ctx, const avr_scene* scene,
                        const avr_scalar_transform* transform, float range_min, float range_max,
                        int bin_count, uint64_t* counts_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(scene != nullptr && transform != nullptr && counts_dev != nullptr, "null argument");
    require(bin_count > 0, "binCount must be positive");  // SceneBuilder.cpp:448-450
    const float width = range_max - range_min;
    if (!(width > 0.0f) || !std::isfinite(width)) return AVR_OK;  // (:470-472): empty histogram
    StagedCells cells;
    stage_cells(ctx, scene, *transform, &cells);
    return avr::launch_histogram(cells.plan.consts, cells.boxes_dev, cells.tiles_dev,
                                 static_cast<int>(cells.plan.boxes.size()),
                                 cells.plan.classify_tile_begin.back(), range_min, range_max,
                                 bin_count, counts_dev, ctx->stream);
  });
}

int avr_slice_outline(avr_context* ctx, const int32_t* box, int width, int height, int red,
                      int green, int blue, uint8_t* rgb8) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(box != nullptr && rgb8 != nullptr, "null argument");
    require(width > 0 && height > 0, "image width and height must be positive");
    require(red >= 0 && red <= 255 && green >= 0 && green <= 255 && blue >= 0 && blue <= 255,
            "colour components must lie in [0, 255]");
    return avr::launch_slice_outline(box, width, height, red, green, blue, rgb8, ctx->stream);
  });
}

static int blend_common(avr_context* ctx, int kind, const void* top, const void* bottom, void* out,
                        int64_t n_pixels) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(n_pixels >= 0, "negative pixel count");
    if (n_pixels == 0) return AVR_OK;
    require(top != nullptr && bottom != nullptr && out != nullptr, "null image");
    return avr::launch_blend(kind, top, bottom, out, n_pixels, ctx->stream);
  });
}

int avr_blend_depthsort_f32x5(avr_context* ctx, const float* top, const float* bottom, float* out,
                              int64_t n_pixels) {
  return blend_common(ctx, 0, top, bottom, out, n_pixels);
}

int avr_blend_rgba_f32x4(avr_context* ctx, const float* top, const float* bottom, float* out,
                         int64_t n_pixels) {
  return blend_common(ctx, 1, top, bottom, out, n_pixels);
}

int avr_blend_rgba_u8x4(avr_context* ctx, const uint32_t* top, const uint32_t* bottom,
                        uint32_t* out, int64_t n_pixels) {
  return blend_common(ctx, 2, top, bottom, out, n_pixels);
}

int avr_blend_regions(avr_context* ctx, int kind, const void* top, int64_t tb, int64_t te,
                      const void* bottom, int64_t bb, int64_t be, void* out) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(kind >= 0 && kind <= 2, "unknown image kind");
    require(tb <= te && bb <= be, "invalid region");
    // the reference asserts the regions touch or overlap (ImageColorOnly.hpp:129-130)
    require(tb <= be && bb <= te, "regions neither overlap nor touch");
    const int64_t n = (te > be ? te : be) - (tb < bb ? tb : bb);
    if (n == 0) return AVR_OK;
    require(out != nullptr && (te == tb || top != nullptr) && (be == bb || bottom != nullptr),
            "null image");
    return avr::launch_blend_regions(kind, top, tb, te, bottom, bb, be, out, ctx->stream);
  });
}

int avr_encode_rgba_u8(avr_context* ctx, const float* rgba, uint32_t* out, int64_t n_pixels) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(n_pixels >= 0, "negative pixel count");
    if (n_pixels == 0) return AVR_OK;
    require(rgba != nullptr && out != nullptr, "null image");
    return avr::launch_encode_u8(rgba, out, n_pixels, ctx->stream);
  });
}

int avr_decode_rgba_u8(avr_context* ctx, const uint32_t* in, float* rgba, int64_t n_pixels) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(n_pixels >= 0, "negative pixel count");
    if (n_pixels == 0) return AVR_OK;
    require(rgba != nullptr && in != nullptr, "null image");
    return avr::launch_decode_u8(in, rgba, n_pixels, ctx->stream);
  });
}

int avr_fold_runs_depthsort(avr_context* ctx, const float* const* slices_host, int n_slices,
                            float* out, int64_t n_pixels) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(n_slices >= 0 && n_pixels >= 0, "invalid argument");
    if (n_pixels == 0) return AVR_OK;
    require(out != nullptr && (n_slices == 0 || slices_host != nullptr), "null argument");
    for (int s = 0; s < n_slices; ++s) require(slices_host[s] != nullptr, "null slice");
    ctx->staging.begin(static_cast<size_t>(n_slices) * sizeof(float*), 1);
    const float* const* slices_dev = ctx->staging.add(slices_host, static_cast<size_t>(n_slices));
    ctx->staging.commit(ctx->stream);
    return avr::launch_fold_runs(slices_dev, n_slices, out, n_pixels, ctx->stream);
  });
}

int avr_downsample_depthsort(avr_context* ctx, const float* src, int target_w, int target_h,
                             int block, float* dst) {
  return guarded([&]() -> int {
    bind_device(ctx);
    // downsampleImage throws for sqrtAA <= 1 (VolumeRenderer.cpp:483-487)
    require(block > 1, "downsample expects a block size > 1");
    require(target_w >= 0 && target_h >= 0, "invalid target size");
    if (target_w == 0 || target_h == 0) return AVR_OK;
    require(src != nullptr && dst != nullptr, "null image");
    return avr::launch_downsample(src, target_w, target_h, block, dst, ctx->stream);
  });
}

int avr_flip_rows(avr_context* ctx, const uint8_t* src, int64_t row_bytes, int h, uint8_t* dst) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(row_bytes >= 0 && h >= 0, "invalid image description");
    if (row_bytes == 0 || h == 0) return AVR_OK;
    require(src != nullptr && dst != nullptr && src != dst, "invalid image pointers");
    return avr::launch_flip_rows(src, row_bytes, h, dst, ctx->stream);
  });
}

int avr_quantize_rgb8(avr_context* ctx, const float* src, int w, int h, int stride, uint8_t* dst) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(w >= 0 && h >= 0 && stride >= 3, "invalid image description");
    if (w == 0 || h == 0) return AVR_OK;
    require(src != nullptr && dst != nullptr, "null image");
    return avr::launch_quantize(src, w, h, stride, dst, ctx->stream);
  });
}

}  // extern "C"
