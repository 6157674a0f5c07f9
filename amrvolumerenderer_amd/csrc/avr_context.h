// What the C ABI's source files share (avr_capi.cpp, avr_field_products.cpp): the context and the
// scene behind the ABI's handles, the staging ring with the stager of a plan's tables
// (stage_tables), the grow-only device buffer, and the helpers every entry point begins with.  Internal to those files: it includes the HIP runtime.
#ifndef AVR_CONTEXT_H
#define AVR_CONTEXT_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "avr_frame_launch.h"
#include "avr_internal.h"

namespace avr {

const std::string& last_error();  // what set_error was given last on this thread (avr_capi.cpp)

class HipFailure : public std::runtime_error {
 public:
  using std::runtime_error::runtime_error;
};

inline void hip_check(hipError_t err, const char* what) {
  if (err != hipSuccess) {
    throw HipFailure(std::string(what) + ": " + hipGetErrorString(err));
  }
}

inline void wait_event(hipEvent_t event, const char* what) { wait_event_deadline(event, what); }
inline void wait_stream(hipStream_t stream, const char* what) { wait_stream_deadline(stream, what); }

// Per-call descriptors (box table, transfer-function tables, run tables, ...) travel to the
// device in ONE asynchronous copy per call: they are packed into a pinned host block and copied
// to its device twin by a small kernel.  A ring of blocks lets the host run several calls ahead of the GPU
// without waiting (a block is re-used only after the copy that read it has completed).
class StagingRing {
 public:
  // Nine: a speculative frame (avr_renderer.cpp) stages three batches on the march's context -- the
  // checking march, the gated classify pass, the gated march -- whose flag buffers rotate with the
  // frame's slot, so the batches repeat with period nine: every slot then always sees the same
  // batch (not copied again, below), and the host may run three such frames ahead.  (With four the
  // host waited 0.38 ms per frame here for a block of the frame before.)
  static constexpr int kSlots = 9;
  static constexpr size_t kAlign = 256;

  ~StagingRing() { release(); }

  void release() {
    for (Slot& slot : slots_) {
      if (slot.dev != nullptr) (void)hipFree(slot.dev);
      if (slot.host != nullptr) (void)hipHostFree(slot.host);
      if (slot.done != nullptr) (void)hipEventDestroy(slot.done);
      slot = Slot{};
    }
  }

  // The owner keeps the host from running ahead by other means (the frame driver's host-side
  // back-pressure): a skipped copy then leaves no packet at all on the consumer stream.
  void set_lean(bool lean) { lean_ = lean; }

  // Starts a batch with room for `bytes` in `items` arrays.
  // How many batches the host may run ahead of the consumer (1 .. kSlots; default 4: what the
  // ring was when it had four blocks -- the frame driver's feedback loops, the co-run search among
  // them, are timed for that lead; a speculating march context takes all nine).
  void set_ahead(int batches) { ahead_ = std::min(std::max(batches, 1), kSlots); }

  void begin(size_t bytes, int items) {
    if (ahead_ < kSlots) {
      Slot& behind = slots_[(next_ + kSlots - ahead_) % kSlots];
      if (behind.pending) {
        wait_event(behind.done, "hipEventQuery(staging)");
        behind.pending = false;
      }
    }
    current_ = &slots_[next_];
    next_ = (next_ + 1) % kSlots;
    if (current_->done == nullptr) {
      hip_check(hipEventCreateWithFlags(&current_->done, avr::ordering_event_flags()), "hipEventCreate");
    }
    if (current_->pending) {
      wait_event(current_->done, "hipEventQuery(staging)");
      current_->pending = false;
    }
    const size_t need = bytes + static_cast<size_t>(items + 1) * kAlign;
    if (need > current_->capacity) {
      if (current_->dev != nullptr) (void)hipFree(current_->dev);
      if (current_->host != nullptr) (void)hipHostFree(current_->host);
      current_->dev = current_->host = nullptr;
      current_->capacity = 0;
      current_->shadow.clear();
      size_t cap = 1 << 16;
      while (cap < need) cap *= 2;
      hip_check(hipMalloc(&current_->dev, cap), "hipMalloc(staging)");
      hip_check(hipHostMalloc(&current_->host, cap, hipHostMallocMapped), "hipHostMalloc(staging)");
      hip_check(hipHostGetDevicePointer(&current_->host_mapped, current_->host, 0),
                "hipHostGetDevicePointer(staging)");
      current_->capacity = cap;
    }
    used_ = 0;
  }

  // Adds one array to the batch; returns where it will be on the device.
  template <typename T>
  const T* add(const T* src, size_t count) {
    used_ = (used_ + kAlign - 1) / kAlign * kAlign;
    const size_t bytes = count * sizeof(T);
    if (used_ + bytes > current_->capacity) throw std::runtime_error("staging batch overflow");
    if (bytes != 0) std::memcpy(static_cast<char*>(current_->host) + used_, src, bytes);
    const T* device = reinterpret_cast<const T*>(static_cast<char*>(current_->dev) + used_);
    used_ += bytes;
    return device;
  }

  // One copy for the whole batch, ordered on `stream` before the kernels that read it.  The
  // copy is a kernel reading the pinned block through its device mapping: hipMemcpyAsync from
  // pinned memory was measured to block the host until the stream had drained, every few frames
  // (5-7 ms with five 1.3 ms frames queued; tools/host_stalls.py), and a launch never does.
  void commit(hipStream_t stream) {
    // A batch that equals what this slot's device twin already holds is not copied again: while
    // camera and parameters repeat, a slot sees the same batch every kSlots calls, and the copy
    // kernel with its event are two packets less between two kernels of the consumer stream (a
    // rank of eight: 27 us from one march to the next, of a 0.19 ms frame).  The twin is intact:
    // begin() has waited for the slot's previous copy, and nothing else writes it.
    static const bool always_copy = std::getenv("AVR_ALWAYS_UPLOAD") != nullptr;  // A/B only
    if (!always_copy && used_ != 0 && used_ == current_->shadow.size() &&
        std::memcmp(current_->host, current_->shadow.data(), used_) == 0) {
      // The slot's event is what keeps the host at most kSlots batches ahead of the consumer;
      // unless the owner bounds the frames in flight itself (set_lean), it is still recorded.
      if (!lean_) {
        hip_check(hipEventRecord(current_->done, stream), "hipEventRecord(staging)");
        current_->pending = true;
      }
      return;
    }
    if (used_ != 0) {
      const int status = launch_upload(current_->host_mapped, current_->dev, used_, stream);
      if (status != AVR_OK) throw HipFailure(last_error());
    }
    hip_check(hipEventRecord(current_->done, stream), "hipEventRecord(staging)");
    current_->pending = true;
    current_->shadow.assign(static_cast<const char*>(current_->host),
                            static_cast<const char*>(current_->host) + used_);
  }

  // Blocks until every committed batch has been copied (before the context's stream changes).
  void drain() {
    for (Slot& slot : slots_) {
      if (slot.pending) {
        wait_event(slot.done, "hipEventQuery(staging)");
        slot.pending = false;
      }
    }
  }

 private:
  struct Slot {
    void* dev = nullptr;
    void* host = nullptr;
    void* host_mapped = nullptr;  // device address of `host`
    size_t capacity = 0;
    hipEvent_t done = nullptr;      // the copy has run: the pinned block may be refilled
    bool pending = false;
    std::vector<char> shadow;       // what the device twin holds (host copy of the last batch copied)
  };
  bool lean_ = false;
  int ahead_ = 4;
  Slot slots_[kSlots];
  Slot* current_ = nullptr;
  int next_ = 0;
  size_t used_ = 0;
};

// A device buffer that only grows: a call that fits in it re-uses it.
struct DeviceBuffer {
  void* data = nullptr;
  size_t capacity = 0;

  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { release(); }

  // Room for `bytes`.  Growing waits for `stream` first (`what` names the wait): work queued there
  // may still use the old block.  Returns whether it grew -- the old contents are then gone.
  bool reserve(size_t bytes, hipStream_t stream, const char* what, const char* malloc_label) {
    if (bytes <= capacity) return false;
    wait_stream(stream, what);
    release();
    hip_check(hipMalloc(&data, bytes), malloc_label);
    capacity = bytes;
    return true;
  }
  void release() {
    if (data != nullptr) (void)hipFree(data);
    data = nullptr;
    capacity = 0;
  }
};

}  // namespace avr

struct avr_scene {
  avr_context* ctx = nullptr;
  std::vector<avr_box> boxes;
  avr_scalar_transform transform{};
  // classified volumes (allocated on first use, grow-only; a frame of the same scene never
  // reallocates): two let the classify pass of frame i+1 overlap the march of frame i, the third
  // lets it run ahead so that neither stream waits for the other's launch (avr_renderer)
  avr::DeviceBuffer classified[AVR_CLASSIFIED_SLOTS];
  int device = 0;
  // optional re-use of a slot's classified volume across frames (avr_scene_set_classification_cache):
  // what the classify pass of the slot's current contents depended on
  bool cache_classification = false;
  std::vector<uint64_t> classified_key[AVR_CLASSIFIED_SLOTS];

  uint8_t* classified_slot(int slot, size_t bytes, hipStream_t stream) {
    if (classified[slot].reserve(bytes, stream, "classified_slot", "hipMalloc(classified)")) {
      classified_key[slot].clear();
    }
    return static_cast<uint8_t*>(classified[slot].data);
  }
};

struct avr_context {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  avr::StagingRing staging;
  avr_scene scratch_scene;         // classified storage of avr_paint_box
  avr::FrameLaunchPlan frame_launch;           // host scratch of render(): its vectors keep their capacity
  int priority = 0;                            // 1: own stream in the highest priority class
  int march_workgroups_per_cu = 0;             // 0 = uncapped
  uint32_t classify_lds_pad = 0;               // avr_context_set_classify_lds_reserve
  bool classify_stream_stores = false;         // context_set_classify_stream_stores
  bool fold_whole_grid = false;                // context_set_fold_whole_grid
  uint64_t* march_counters = nullptr;          // diagnostics (avr_context_set_march_counters)
  int last_only_mode = -2;                     // ... (avr_context_last_march_mode; -2: no march yet)
  avr::DeviceBuffer max_layers;                // layer of avr_paint_box_max
  double* colorize_scratch = nullptr;           // avr_projection_colorize's range reduction
  avr::DeviceBuffer axis_planes;               // avr_scene_axis_projection's partial planes
  avr::DeviceBuffer cube_planes;               // avr_scene_velocity_cube's partial planes
  uint64_t cube_scratch_entries = avr::kCubeScratchEntries;  // avr_context_set_velocity_cube_scratch_entries
  int ray_transfer_chunk = avr::kTransferChunk;  // avr_context_set_ray_transfer_chunk
  avr::DeviceBuffer gradient_planes;           // avr_scene_gradient's face planes
  avr::DeviceBuffer clump_parents;             // avr_scene_clumps' parent entries and chunk counts
  avr::DeviceBuffer clump_pair_partials;       // avr_clump_pair_energy's partial sums, one per item
  avr::DeviceBuffer iso_scratch;               // avr_scene_isosurface's shells and chunk counts
  avr::DeviceBuffer group_counts;              // avr_particle_groups' counts per chunk
};

namespace avr {

// Runs `body`, mapping exceptions to status codes (no exception crosses the ABI).
template <typename F>
int guarded(F&& body) {
  try {
    return body();
  } catch (const std::invalid_argument& e) {
    set_error(e.what());
    return AVR_ERR_INVALID_ARGUMENT;
  } catch (const std::bad_alloc&) {
    set_error("out of host memory");
    return AVR_ERR_OUT_OF_MEMORY;
  } catch (const std::exception& e) {
    set_error(e.what());
    return AVR_ERR_RUNTIME;
  } catch (...) {
    set_error("unknown failure");
    return AVR_ERR_RUNTIME;
  }
}

inline void require(bool condition, const char* message) {
  if (!condition) throw std::invalid_argument(message);
}

// The second pass over a plan's visit_tables: adds every table to the batch that StagingSize sized
// and writes where it will be on the device into the launch arguments.
struct StagingFill {
  StagingRing* ring;
  template <class T>
  void operator()(const T** device, const T* host, size_t count) const {
    static const T kUnread{};  // an empty table's one element: no count or range leads to it
    *device = count != 0 ? ring->add(host, count) : ring->add(&kUnread, 1);
  }
};

// Stages the tables of `plan` in one batch on the context's stream and sets their addresses in
// `args` (the arguments visit_tables takes).  Two rules meet here.  A table the plan names is
// never null on the device: an empty one is one unread element (the field products' rule).  A
// table the plan does NOT name keeps the null its argument had: a frame's launchers branch on that
// (avr_frame_launch.h, "absent is null"), so a plan must not name a table its call does without.
template <class Plan, class... Args>
void stage_tables(avr_context* ctx, const Plan& plan, Args*... args) {
  StagingSize size;
  plan.visit_tables(args..., size);
  ctx->staging.begin(size.bytes, size.items);
  plan.visit_tables(args..., StagingFill{&ctx->staging});
  ctx->staging.commit(ctx->stream);
}

inline void bind_device(avr_context* ctx) {
  require(ctx != nullptr, "null context");
  hip_check(hipSetDevice(ctx->device), "hipSetDevice");
  if (ctx->stream == nullptr) {  // no external stream was supplied: create the context's own
    if (ctx->priority != 0) {
      int least = 0, greatest = 0;  // numerically lower = more urgent
      hip_check(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange");
      hip_check(hipStreamCreateWithPriority(&ctx->own_stream, hipStreamNonBlocking, greatest),
                "hipStreamCreateWithPriority");
    } else {
      hip_check(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking), "hipStreamCreate");
    }
    ctx->stream = ctx->own_stream;
  }
}

}  // namespace avr

#endif
