// The host plan of one frame's device work (the classify pass and/or the march of a list of boxes):
// everything render() (avr_capi.cpp) works out before its first HIP call -- the rules on the
// request, the classification key, where a chunked frame is cut, the tables of a flagged or
// positioned classify pass, the march's work items, every launch argument that is not a device
// address, and the ordered list of launches with what each overrides.  Host only and free of HIP
// and of the C ABI's handles, like avr_field_plans.h: it works on the ABI's plain arguments and the
// host prologue (plan_frame, build_march_items: avr_host.cpp), throws std::invalid_argument with
// the message the C ABI reports, and is tested as a plain C++ program
// (tests/cxx/frame_launch_test.cpp).
//
// What the plan hands to render(), the field plans' rule with one difference:
//  - `launch`, the RenderLaunch the kernels are launched with: every field that is not a device
//    address is filled, every address is null.  render() copies it and fills only addresses.
//  - visit_tables(launch, spec, visit): the tables the call stages, named once, in staging order.
//    ABSENT IS NULL, NOT PADDED: the launchers branch on box_list_dev, run_spans_dev, spec_dev,
//    visible_in and classify_gate being null, so a table the call does without is not visited and
//    its address stays null.  (A table that IS visited with count 0 is staged as the field
//    products' are, as one element nothing reads: avr_context.h, StagingFill.)
//  - `steps`, the launches in order.  A step says classify or march, whether it launches at all,
//    which event to wait for before it or to record behind it, and what a chunk overrides.
#ifndef AVR_FRAME_LAUNCH_H
#define AVR_FRAME_LAUNCH_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "avr_internal.h"

namespace avr {

enum FramePhase : int { kClassify = 1, kMarch = 2 };

// What a frame call is asked for, in parts that a caller fills in one expression each.
struct FrameBoxes {  // the boxes and how they are seen
  const avr_box* boxes;
  int n_boxes;
  const avr_scalar_transform& transform;
  const avr_paint_params& params;
  const avr_camera& camera;
};
struct FrameRuns {  // their global layer order cut into runs, the runs' tables, the exchange's pieces
  const int32_t* box_order;
  int n_order;
  const int32_t* run_end;
  int n_runs, n_pieces;
  const std::vector<RunRectDev>& rects;
  const std::vector<RunBlockDev>& blocks;  // n_runs x n_pieces
  const std::vector<RunSpanDev>* spans;    // a tightened plan's, or null
  const PieceMapDev& pieces;
};
struct FrameTarget {  // the classified slot the frame uses, and where the results go
  int slot;
  float* out_layers;
  uint64_t* samples_out;  // may be null
  FramePlan* cached;  // null, or the host prologue kept from a frame's classify call to its march
};
struct RenderRequest {
  int phases;  // FramePhase bits
  // kMaxIntensity: one march launch, never chunked, culled or speculative.  kProjection: the same,
  // over the raw cells: march only, the classified volume is neither read nor made.
  FrameKind kind;
  FrameBoxes in;
  FrameRuns runs;
  FrameTarget to;
};
// The shape of the call, as far as the host sees it: a frame cut into depth-ordered chunks of its
// global layer order (chunk k is classified by launch k of the classify call, which records event
// k behind it, and marched by launch k of the march call, which waits for event k first), culled
// (one call queues classify 0, march 0, classify 1 ...; march k flags the boxes behind chunk k that
// a ray may still sample in visibility[k * n_order + position], classify k + 1 leaves out the boxes
// of its chunk whose flag is 0), flagged or positioned (the classify pass takes only the positions
// of the layer order whose device flag is set, or the positions listed here), speculative.
struct FrameChunks {
  int count = 1;
  bool first_alone = false;  // classify: chunk 0 has the GPU to itself (no LDS reserve)
  bool events = false;       // the caller gave an event per chunk
  bool culled = false;       // ... a visibility buffer of count * n_order bytes
  bool flags = false;        // ... device flags by position
  const int32_t* classify_positions = nullptr;  // or the positions themselves, ascending
  int n_classify_positions = 0;
  const avr_speculation* speculation = nullptr;
};

inline void require_frame(bool condition, const char* message) {
  if (!condition) throw std::invalid_argument(message);
}

// Upper bound of the march's workgroups: a work item per super-tile of the screen and run, padded
// to whole rounds of the XCDs, four workgroups each (build_march_items, avr_host.cpp).
inline int64_t march_workgroups_bound(int width, int height, int n_runs) {
  const int64_t span = kTile * kSuperTileSide;
  const int64_t super_tiles = ((width + span - 1) / span) * ((height + span - 1) / span);
  const int64_t items = (super_tiles * std::max(n_runs, 0) + kXcds - 1) / kXcds * kXcds;
  return items * kSuperTileTiles;
}

// Everything classify_kernel reads besides the cells themselves: a slot that was classified under
// an equal key holds exactly this frame's classification.
inline std::vector<uint64_t> classification_key(const FramePlan& plan) {
  std::vector<uint64_t> key;
  auto bits = [](double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
  };
  const FrameConsts& fc = plan.consts;
  key.reserve(12 + plan.boxes.size() * 4);
  for (double v : {static_cast<double>(fc.range_min), static_cast<double>(fc.inverse_range),
                   static_cast<double>(fc.clip_start), fc.positive_floor, fc.norm_min,
                   fc.inv_norm_span}) {
    key.push_back(bits(v));
  }
  key.push_back(static_cast<uint64_t>(fc.apply_clip) | (static_cast<uint64_t>(fc.log_scale) << 8) |
                (static_cast<uint64_t>(fc.normalize) << 16));
  for (const BoxDev& dev : plan.boxes) {
    key.push_back(reinterpret_cast<uint64_t>(dev.cells));
    key.push_back((static_cast<uint64_t>(static_cast<uint32_t>(dev.jstride)) << 32) |
                  static_cast<uint32_t>(dev.kstride));
    key.push_back((static_cast<uint64_t>(dev.nx) << 42) | (static_cast<uint64_t>(dev.ny) << 21) |
                  static_cast<uint64_t>(dev.nz));
    key.push_back(dev.cls_offset);
  }
  return key;
}

// Positions [bounds[k], bounds[k + 1]) of the global layer order for chunk k: equal shares of the
// classify pass's work (tiles = cells), so that classifying chunk k + 1 takes about as long as
// any other; a function of the plan alone -- the classify and the march call cut alike.
inline void chunk_bounds(const FramePlan& plan, const int32_t* box_order, int n_order, int n_chunks,
                         std::vector<int>* bounds) {
  bounds->assign(static_cast<size_t>(n_chunks) + 1, n_order);
  (*bounds)[0] = 0;
  auto tiles_of = [&](int position) -> uint64_t {
    const size_t b = static_cast<size_t>(box_order[position]);
    return plan.classify_tile_begin[b + 1] - plan.classify_tile_begin[b];
  };
  uint64_t total = 0;
  for (int i = 0; i < n_order; ++i) total += tiles_of(i);
  uint64_t seen = 0;
  int k = 1;
  for (int i = 0; i < n_order && k < n_chunks; ++i) {
    seen += tiles_of(i);
    while (k < n_chunks && seen * static_cast<uint64_t>(n_chunks) >= total * static_cast<uint64_t>(k)) {
      (*bounds)[static_cast<size_t>(k++)] = i + 1;
    }
  }
}

// A speculative march's record as the kernel reads it, from what the caller gave.  The first pass
// marks, the gated pass reads: one array, a byte per workgroup of the grid.  (Flags given on the
// host are staged with the call: visit_tables sets `classified` then.)
inline MarchSpecDev speculation_record(const avr_speculation& given) {
  MarchSpecDev spec{};
  spec.classified = given.classified;
  spec.visited = given.visited;
  spec.missed = given.missed;
  spec.miss_count = given.miss_count;
  spec.host_miss_flag = given.host_miss_flag;
  spec.gate = given.gate;
  spec.dirty_blocks_out = given.gate == nullptr ? given.dirty_workgroups : nullptr;
  spec.dirty_blocks = given.gate != nullptr ? given.dirty_workgroups : nullptr;
  return spec;
}

// One launch of the call, in order.
struct FrameStep {
  bool march = false;     // else a classify launch
  // false: nothing is launched, the step's event is still waited for or recorded.  An empty chunk
  // classifies nothing; the march of chunk k is launched when it has boxes, or k is 0 (the first
  // launch stores every pixel of the runs' layers, the later ones resume them), or the frame is
  // culled (every chunk's march flags the boxes of the chunks behind it -- flags left at 0 would
  // mean "nobody samples them").
  bool launches = true;
  int wait_event = -1;    // >= 0: the stream waits for this event of the caller's before the step
  int record_event = -1;  // >= 0: ... records it behind the step
  // What a chunk's launch overrides in the call's RenderLaunch (`chunk`; a frame in one piece
  // launches it as it stands).  Classify: its part of the staged box list and of the chunks' prefix
  // sums, its counts, its LDS reserve, and what the march of the chunk before found still visible
  // of its boxes (a byte offset into the visibility buffer; < 0: null).
  bool chunk = false;
  int box_list_at = 0, prefix_at = 0;
  int n_classify_boxes = 0;
  uint32_t n_classify_tiles = 0;
  uint32_t classify_lds_pad = 0;
  int64_t visible_in_at = -1;
  // March: its positions, whether it resumes the run accumulators, and where it flags the boxes
  // behind it (< 0: null, the last chunk's).
  int pos_begin = 0, pos_end = -1, resume = 0;
  int64_t visible_out_at = -1;

  // `to`: a copy of the call's launch arguments with its addresses set.
  void apply(uint8_t* visibility, RenderLaunch* to) const {
    if (!chunk) return;
    if (march) {
      to->visible_out = visible_out_at >= 0 ? visibility + visible_out_at : nullptr;
      to->pos_begin = pos_begin;
      to->pos_end = pos_end;
      to->resume = resume;
    } else {
      to->visible_in = visible_in_at >= 0 ? visibility + visible_in_at : nullptr;
      to->box_list_dev += box_list_at;
      to->tile_begin_dev += prefix_at;
      to->n_classify_boxes = n_classify_boxes;
      to->n_classify_tiles = n_classify_tiles;
      to->classify_lds_pad = classify_lds_pad;
    }
  }
};

// The plan of one call.  Its vectors keep their capacity from frame to frame (a context holds
// one); it refers to the request's arrays, so it is good for as long as they are.  A call is
// planned in two steps, because a classification cache hit, which only the entry point can see,
// drops the classify pass before the march items are built or anything else is worked out:
//   if (!plan.open(request, chunks, ...)) return;   the request's rules; the host prologue
//   ... the entry point may clear kClassify in plan.phases (and returns if nothing is left)
//   plan.finish();                                  everything else
struct FrameLaunchPlan {
  int phases = 0;                   // FramePhase bits still to do
  const FramePlan* prologue = nullptr;  // the request's cached one, or `uncached`
  bool needs_classified = false;    // the frame reads or writes a classified slot (not kProjection)
  RenderLaunch launch{};
  bool chunked = false, flagged = false, positioned = false;
  std::vector<int> bounds;                 // chunked: count + 1 positions
  std::vector<uint32_t> chunk_tile_begin;  // chunk k: entries bounds[k] + k .. bounds[k + 1] + k
  // a flagged classify pass: the local boxes in layer order as ONE list under its own prefix sum
  std::vector<uint32_t> listed_tile_begin;
  std::vector<int32_t> listed_boxes;
  // the boxes' screen rectangles in layer order: what the march's cull reads 64 at a time
  std::vector<int32_t> order_rects;
  const std::vector<MarchItemDev>* items = nullptr;  // the cached prologue's, or `uncached_items`
  size_t visibility_bytes = 0;      // culled: what the call clears of the visibility buffer first
  std::vector<FrameStep> steps;

  bool open(const RenderRequest& frame, const FrameChunks& shape, uint32_t classify_lds_pad,
            bool classify_stream_stores, int march_workgroups_per_cu) {
    request_ = &frame;
    chunks_ = shape;
    phases = frame.phases;
    workgroups_per_cu_ = march_workgroups_per_cu;
    chunked = flagged = positioned = false;
    visibility_bytes = 0;
    steps.clear();
    const FrameRuns& runs = frame.runs;
    require_frame(runs.n_runs >= 0 && runs.n_order >= 0 && runs.n_pieces >= 1, "invalid run description");
    require_frame(shape.count >= 1 && shape.count <= AVR_MAX_FRAME_CHUNKS, "invalid chunk count");
    require_frame(shape.count == 1 || phases == kClassify || phases == kMarch || shape.culled,
                  "a chunked frame is classified and marched by separate calls (or by avr_render_plan_culled)");
    require_frame(frame.to.slot >= 0 && frame.to.slot < AVR_CLASSIFIED_SLOTS, "classified slot out of range");
    require_frame(frame.kind == FrameKind::kVolume || (shape.count == 1 && shape.speculation == nullptr),
                  "a maximum-intensity or column-projection march is one launch: no chunks, no speculation");
    require_frame(frame.kind != FrameKind::kProjection || phases == kMarch,
                  "a column-projection march has no classify pass");
    FramePlan& plan = frame.to.cached != nullptr ? *frame.to.cached : uncached_;
    if (frame.to.cached == nullptr) uncached_.ready = false;
    if (plan.boxes.size() != static_cast<size_t>(frame.in.n_boxes) || !plan.ready) {
      plan_frame(frame.in.boxes, frame.in.n_boxes, frame.in.transform, frame.in.params,
                 frame.in.camera, &plan);
      plan.march_items_ready = false;
    }
    prologue = &plan;
    if (runs.n_runs == 0) {
      phases = 0;
      return false;
    }
    require_frame(plan.n_tables <= kMaxLdsTables,
                  "too many distinct sampling levels for the LDS transfer-function cache");
    launch = RenderLaunch{};
    launch.consts = plan.consts;
    launch.n_boxes = frame.in.n_boxes;
    launch.n_classify_tiles = plan.classify_tile_begin.back();
    launch.classify_lds_pad = classify_lds_pad;
    // (streamed only when the classified volume is more than the 256 MB memory-side cache holds:
    // config-2's 134 MB, stored plainly, are still there when its march comes a frame later --
    // 0.378 ms per frame against 0.465 streamed; config-4's 370 MB are not, 0.967 -> 0.958)
    launch.classify_stream_stores =
        (classify_stream_stores && plan.classified_bytes > (256ull << 20)) ? 1 : 0;
    // (decided for the frame's boxes, so for every chunk and every list of them)
    launch.classify_by_wave = true;
    for (const BoxDev& dev : plan.boxes) {
      if (!classify_wave_box(dev, plan.consts)) launch.classify_by_wave = false;
    }
    needs_classified = frame.kind != FrameKind::kProjection;
    return true;
  }

  void finish() {
    const RenderRequest& frame = *request_;
    const FrameRuns& runs = frame.runs;
    const FrameChunks& shape = chunks_;
    FramePlan& plan = frame.to.cached != nullptr ? *frame.to.cached : uncached_;
    if (phases & kMarch) {
      require_frame(frame.to.out_layers != nullptr, "null output image");
      require_frame(runs.n_runs == 0 || (runs.run_end != nullptr), "null run_end");
      require_frame(runs.n_order == 0 || (runs.box_order != nullptr), "null box_order");
      require_frame(runs.rects.size() == static_cast<size_t>(runs.n_runs) &&
                        runs.blocks.size() == static_cast<size_t>(runs.n_runs) * runs.n_pieces,
                    "run tables do not match the runs");
      // scratch, reused across frames; a frame plan's prologue keeps its own (the items depend on
      // the plan alone: a camera that repeats does not sort them again)
      const bool keep_items = frame.to.cached != nullptr;
      std::vector<MarchItemDev>& work = keep_items ? plan.march_items : uncached_items_;
      if (!(keep_items && plan.march_items_ready)) {
        int previous = 0;
        for (int r = 0; r < runs.n_runs; ++r) {
          require_frame(runs.run_end[r] >= previous && runs.run_end[r] <= runs.n_order,
                        "run_end must be non-decreasing");
          previous = runs.run_end[r];
        }
        require_frame(runs.run_end[runs.n_runs - 1] == runs.n_order, "runs must cover box_order");
        require_box_order(0, runs.n_order);
        build_march_items(plan, runs.box_order, runs.run_end, runs.n_runs, runs.rects, &work);
        plan.march_items_ready = keep_items;
      }
      items = &work;
    }
    // chunked: the positions of every chunk, and for the classify call the chunks' box lists (the
    // local boxes in global layer order ARE the lists: chunk k is box_order[bounds[k] .. bounds[k+1]))
    // with one prefix sum of classify workgroups per chunk
    chunked = shape.count > 1;
    if (chunked) {
      require_frame(runs.n_order == 0 || runs.box_order != nullptr, "null box_order");
      require_box_order(0, runs.n_order);
      chunk_bounds(plan, runs.box_order, runs.n_order, shape.count, &bounds);
      if (phases & kClassify) {
        chunk_tile_begin.clear();
        chunk_tile_begin.reserve(static_cast<size_t>(runs.n_order + shape.count));
        for (int k = 0; k < shape.count; ++k) {
          uint32_t sum = 0;
          chunk_tile_begin.push_back(0u);
          for (int i = bounds[static_cast<size_t>(k)]; i < bounds[static_cast<size_t>(k) + 1]; ++i) {
            sum += classify_tiles_at(plan, i);
            chunk_tile_begin.push_back(sum);
          }
        }
      }
    }
    positioned = (phases & kClassify) && shape.classify_positions != nullptr;
    flagged = (phases & kClassify) && (shape.flags || positioned);
    if (flagged) {
      require_frame(shape.count == 1, "a flagged classify pass is not cut into chunks");
      require_frame(runs.n_order == 0 || runs.box_order != nullptr, "null box_order");
      require_frame(!(positioned && shape.flags), "flags or positions, not both");
      const int n_listed = positioned ? shape.n_classify_positions : runs.n_order;
      require_frame(n_listed >= 0 && n_listed <= runs.n_order, "too many positions");
      listed_tile_begin.clear();
      listed_boxes.clear();
      listed_tile_begin.reserve(static_cast<size_t>(n_listed) + 1);
      listed_boxes.reserve(static_cast<size_t>(n_listed));
      uint32_t sum = 0;
      listed_tile_begin.push_back(0u);
      int previous = -1;
      for (int i = 0; i < n_listed; ++i) {
        const int position = positioned ? shape.classify_positions[i] : i;
        require_frame(position > previous && position < runs.n_order,
                      "positions must ascend within the layer order");
        previous = position;
        require_box_order(position, position + 1);
        sum += classify_tiles_at(plan, position);
        listed_tile_begin.push_back(sum);
        listed_boxes.push_back(runs.box_order[position]);
      }
      launch.n_classify_boxes = static_cast<int>(listed_boxes.size());
      launch.n_classify_tiles = listed_tile_begin.back();
    }
    if (phases & kMarch) {
      launch.n_tables = plan.n_tables;
      order_rects.resize(static_cast<size_t>(runs.n_order) * 4);
      for (int i = 0; i < runs.n_order; ++i) {
        const BoxDev& dev = plan.boxes[static_cast<size_t>(runs.box_order[i])];
        std::copy(dev.rect, dev.rect + 4, order_rects.begin() + static_cast<std::ptrdiff_t>(i) * 4);
      }
      launch.n_order = runs.n_order;
      launch.n_runs = runs.n_runs;
      launch.n_pieces = runs.n_pieces;
      launch.pieces = runs.pieces;
      if (shape.speculation != nullptr) {
        require_frame(shape.count == 1 && frame.to.samples_out == nullptr,
                      "a speculative march is one launch and counts no samples");
        const avr_speculation& given = *shape.speculation;
        require_frame(given.classified == nullptr || given.classified_host == nullptr,
                      "the flags are on the device or on the host, not both");
        const bool checks = given.classified != nullptr || given.classified_host != nullptr;
        require_frame(!checks || (given.missed != nullptr && given.miss_count != nullptr),
                      "a speculative march that checks flags needs somewhere to report misses");
        if (given.dirty_workgroups != nullptr) {
          require_frame(static_cast<int64_t>(items->size()) * kSuperTileTiles <=
                            march_workgroups_bound(frame.in.params.width, frame.in.params.height,
                                                   runs.n_runs),
                        "more march workgroups than avr_march_plan_workgroups promised");
        }
        launch.spec_is_repair = given.gate != nullptr;
      }
      launch.n_items = static_cast<uint32_t>(items->size());
      launch.workgroups_per_cu = workgroups_per_cu_;
      launch.kind = frame.kind;
      launch.only_mode = plan.boxes.empty() ? -1 : plan.boxes[0].index_mode;
      for (const BoxDev& dev : plan.boxes) {
        if (dev.index_mode != launch.only_mode) launch.only_mode = -1;
      }
    }
    list_steps();
  }

  // The tables the call stages, in order; `spec` is the speculative march's record with the
  // caller's addresses (speculation_record), staged as it stands once its host flags are.
  template <class Visit>
  void visit_tables(RenderLaunch* to, MarchSpecDev* spec, Visit&& visit) const {
    const FrameRuns& runs = request_->runs;
    const FramePlan& plan = *prologue;
    const size_t n_order = static_cast<size_t>(runs.n_order);
    visit(&to->boxes_dev, plan.boxes.data(), plan.boxes.size());
    if (phases & kClassify) {
      // (a chunked or flagged pass never reads the whole scene's prefix: its own supersedes it
      // below.  It stays staged: the ring skips the copy of a batch equal to the slot's last, and
      // the speculating driver counts on its period of nine identical batches.)
      visit(&to->tile_begin_dev, plan.classify_tile_begin.data(), plan.classify_tile_begin.size());
      if (chunked) {
        visit(&to->tile_begin_dev, chunk_tile_begin.data(), chunk_tile_begin.size());
        visit(&to->box_list_dev, runs.box_order, n_order);
      }
      if (flagged) {
        visit(&to->tile_begin_dev, listed_tile_begin.data(), listed_tile_begin.size());
        visit(&to->box_list_dev, listed_boxes.data(), listed_boxes.size());
      }
    }
    if (phases & kMarch) {
      visit(&to->tables_dev, plan.tables.data(), plan.tables.size());
      visit(&to->order_dev, runs.box_order, n_order);
      visit(&to->order_rects_dev, order_rects.data(), order_rects.size());
      visit(&to->run_end_dev, runs.run_end, static_cast<size_t>(runs.n_runs));
      visit(&to->run_rects_dev, runs.rects.data(), runs.rects.size());
      visit(&to->run_blocks_dev, runs.blocks.data(), runs.blocks.size());
      if (runs.spans != nullptr && !runs.spans->empty()) {
        visit(&to->run_spans_dev, runs.spans->data(), runs.spans->size());
      }
      if (chunks_.speculation != nullptr) {
        if (chunks_.speculation->classified_host != nullptr) {
          visit(&spec->classified, chunks_.speculation->classified_host, n_order);
        }
        visit(&to->spec_dev, static_cast<const MarchSpecDev*>(spec), size_t{1});
      }
      visit(&to->items_dev, items->data(), items->size());
    }
  }

 private:
  uint32_t classify_tiles_at(const FramePlan& plan, int position) const {
    const size_t b = static_cast<size_t>(request_->runs.box_order[position]);
    return plan.classify_tile_begin[b + 1] - plan.classify_tile_begin[b];
  }
  void require_box_order(int begin, int end) const {
    const int32_t* order = request_->runs.box_order;
    for (int i = begin; i < end; ++i) {
      require_frame(order[i] >= 0 && order[i] < request_->in.n_boxes, "box_order entry out of range");
    }
  }
  void list_steps() {
    const FrameChunks& shape = chunks_;
    if (!chunked) {
      for (int phase : {kClassify, kMarch}) {
        if (!(phases & phase)) continue;
        FrameStep step;
        step.march = phase == kMarch;
        steps.push_back(step);
      }
      return;
    }
    const int64_t n_order = request_->runs.n_order;
    if (shape.culled) visibility_bytes = static_cast<size_t>(shape.count) * static_cast<size_t>(n_order);
    for (int k = 0; k < shape.count; ++k) {
      const int first = bounds[static_cast<size_t>(k)], last = bounds[static_cast<size_t>(k) + 1];
      if (phases & kClassify) {
        FrameStep step;
        step.chunk = true;
        step.launches = last > first;
        if (shape.events) step.record_event = k;
        if (shape.culled && k > 0) step.visible_in_at = (k - 1) * n_order + first;
        step.box_list_at = first;
        step.n_classify_boxes = last - first;
        step.prefix_at = first + k;
        step.n_classify_tiles = chunk_tile_begin[static_cast<size_t>(last + k)];
        step.classify_lds_pad = (k == 0 && shape.first_alone) ? 0u : launch.classify_lds_pad;
        steps.push_back(step);
      }
      if (phases & kMarch) {
        FrameStep step;
        step.march = step.chunk = true;
        step.launches = last > first || k == 0 || shape.culled;
        if (shape.events && !(phases & kClassify)) step.wait_event = k;
        if (shape.culled && k + 1 < shape.count) step.visible_out_at = k * n_order;
        step.pos_begin = first;
        step.pos_end = last;
        step.resume = k > 0 ? 1 : 0;
        steps.push_back(step);
      }
    }
  }

  const RenderRequest* request_ = nullptr;
  FrameChunks chunks_;
  int workgroups_per_cu_ = 0;
  FramePlan uncached_;                         // the prologue of a call without a cached one
  std::vector<MarchItemDev> uncached_items_;   // ... and its march items
};

}  // namespace avr

#endif
