// What a frame's launch plan (csrc/avr_frame_launch.h) hands to render(), as a plain C++ program
// built with AddressSanitizer and UBSan and without HIP, linked with the host prologue
// (csrc/avr_host.cpp).  The scene: three boxes at a 64x48 image -- box 0 of 8x4x4 cells (one
// classify tile), box 1 of 136x4x4 (two: a row spans two 128-cell classify chunks), box 2 without
// cells, off to the side (no tile, off screen) -- in the layer order {1, 2, 0}, two runs ({1, 2}
// and {0}) over two pieces.  Cell pointers are made-up addresses that nothing reads.  Checked:
//  - a plain volume frame (classify|march, classify, march), a maximum-intensity frame and a
//    projection: the tables visit_tables names (argument, element size, count, order), every
//    address still null after the visits, every other launch argument against a value written out
//    here, the launches in order;
//  - chunked frames of 2, 3 and AVR_MAX_FRAME_CHUNKS chunks: the cuts against brute force, the
//    prefix layout, the steps of the classify call, the march call and the culled call;
//  - flagged and positioned classify passes, speculative marches, and every refusal by message;
//  - the classification key, and that a cached prologue keeps its march items.
// Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../amrvolumerenderer_amd/csrc/avr_frame_launch.h"

namespace {

using avr::kClassify;
using avr::kMarch;

void fail(const std::string& what) {
  std::fprintf(stderr, "FAILED: %s\n", what.c_str());
  std::exit(1);
}
void expect(bool condition, const std::string& what) {
  if (!condition) fail(what);
}
template <class F>
void expect_refused(const std::string& message, F&& call) {
  try {
    call();
  } catch (const std::invalid_argument& e) {
    expect(message == e.what(), "refused with \"" + std::string(e.what()) + "\", not \"" + message + "\"");
    return;
  }
  fail("not refused: " + message);
}
template <class T>
T* address(int bit) { return reinterpret_cast<T*>(uintptr_t{1} << bit); }

// ---- the scene ------------------------------------------------------------------------------
constexpr uint32_t kPad = 4096;     // the context's three settings, as render() passes them
constexpr bool kStream = true;
constexpr int kPerCu = 3;
const uint32_t kTiles[3] = {1, 2, 0};        // classify tiles per box
const int32_t kOrder[3] = {1, 2, 0};         // tiles by position: 2, 0, 1
const int32_t kRunEnd[2] = {2, 3};

struct Scene {
  std::vector<avr_box> boxes;
  avr_scalar_transform transform{};
  avr_paint_params params{};
  avr_camera camera{};
  std::vector<int32_t> order{kOrder, kOrder + 3};
  std::vector<int32_t> run_end{kRunEnd, kRunEnd + 2};
  std::vector<avr::RunRectDev> rects;
  std::vector<avr::RunBlockDev> blocks;
  std::vector<avr::RunSpanDev> spans;
  avr::PieceMapDev pieces;

  explicit Scene(int width = 64, int height = 48) {
    const int dims[3][3] = {{8, 4, 4}, {136, 4, 4}, {0, 0, 0}};
    const double lo[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.5, 0.0}, {50.0, 0.0, 0.0}};
    const double size[3][3] = {{1.0, 0.5, 0.5}, {1.0625, 0.5, 0.5}, {1.0, 1.0, 1.0}};
    for (int b = 0; b < 3; ++b) {
      avr_box box{};
      for (int d = 0; d < 3; ++d) {
        box.dims[d] = dims[b][d];
        box.min_corner[d] = lo[b][d];
        box.max_corner[d] = lo[b][d] + size[b][d];
      }
      box.jstride = dims[b][0];
      box.kstride = dims[b][0] * dims[b][1];
      if (dims[b][0] > 0) box.cells = address<const double>(40 + b);
      boxes.push_back(box);
    }
    transform.normalize_to_unit_range = 1;
    transform.inverse_normalization_span = 1.0;
    params.width = width;
    params.height = height;
    params.scalar_range[1] = 1.0f;
    params.box_transparency = 0.8f;
    params.reference_sample_distance = 0.01f;
    params.bounds_max[0] = params.bounds_max[1] = params.bounds_max[2] = 1.0;
    camera.eye[0] = 0.5; camera.eye[1] = 0.5; camera.eye[2] = 4.0;
    camera.look_at[0] = 0.5; camera.look_at[1] = 0.5; camera.look_at[2] = 0.25;
    camera.up[1] = 1.0;
    camera.fov_y_degrees = 45.0f; camera.near_plane = 0.1f; camera.far_plane = 100.0f;
    // both runs cover the screen: every super-tile of it is a march item of each
    rects = {{0, 0, width - 1, height - 1}, {0, 0, width - 1, height - 1}};
    blocks = {{0, 0, -1}, {1000, 0, -1}, {2000, 0, -1}, {3000, 0, -1}};
    pieces.n_pieces = 2;
    pieces.width = width;
    pieces.height = height;
    pieces.piece_size = static_cast<int64_t>(width) * height / 2;
  }
  avr::RenderRequest request(int phases, avr::FrameKind kind = avr::FrameKind::kVolume,
                             avr::FramePlan* cached = nullptr, bool with_spans = false) const {
    return {phases, kind,
            {boxes.data(), static_cast<int>(boxes.size()), transform, params, camera},
            {order.data(), 3, run_end.data(), 2, 2, rects, blocks, with_spans ? &spans : nullptr, pieces},
            {1, address<float>(50), nullptr, cached}};
  }
};

bool plan_call(avr::FrameLaunchPlan* plan, const avr::RenderRequest& request,
               const avr::FrameChunks& shape = avr::FrameChunks{}) {
  if (!plan->open(request, shape, kPad, kStream, kPerCu)) return false;
  plan->finish();
  return true;
}

// ---- the tables a plan names ----------------------------------------------------------------
struct Table {
  const void* to;
  size_t element, count;
  const void* from;
  uint64_t hash;
  bool operator==(const Table& o) const {
    return to == o.to && element == o.element && count == o.count && from == o.from && hash == o.hash;
  }
};
struct Recorder {
  std::vector<Table> tables;
  template <class T>
  void operator()(const T** device, const T* host, size_t count) {
    uint64_t hash = 1469598103934665603ull;
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(host);
    for (size_t i = 0; i < count * sizeof(T); ++i) hash = (hash ^ bytes[i]) * 1099511628211ull;
    tables.push_back({device, sizeof(T), count, host, hash});
  }
};
struct Want {
  const void* to;
  size_t element, count;
  const void* from;  // the host table, where the test can name it; else null
};
bool all_null(const avr::RenderLaunch& l) {
  return l.boxes_dev == nullptr && l.tables_dev == nullptr && l.order_dev == nullptr &&
         l.order_rects_dev == nullptr && l.spec_dev == nullptr && l.classify_gate == nullptr &&
         l.run_end_dev == nullptr && l.run_rects_dev == nullptr && l.run_blocks_dev == nullptr &&
         l.run_spans_dev == nullptr && l.out_layers == nullptr && l.samples_out == nullptr &&
         l.counters == nullptr && l.classified == nullptr && l.tile_begin_dev == nullptr &&
         l.items_dev == nullptr && l.box_list_dev == nullptr && l.visible_out == nullptr &&
         l.visible_in == nullptr;
}
// The plan's tables are `want`, in order; the sizing pass counts them; no visit sets an address or
// changes the plan.
void expect_tables(const std::string& name, const avr::FrameLaunchPlan& plan,
                   const std::vector<Want>& want, avr::RenderLaunch* launch, avr::MarchSpecDev* spec) {
  const avr::MarchSpecDev spec_before = *spec;
  Recorder first, second;
  plan.visit_tables(launch, spec, first);
  expect(first.tables.size() == want.size(), name + ": " + std::to_string(first.tables.size()) + " tables");
  size_t bytes = 0;
  for (size_t t = 0; t < want.size(); ++t) {
    const Table& got = first.tables[t];
    const std::string where = name + ": table " + std::to_string(t);
    expect(got.to == want[t].to, where + " goes to another argument");
    expect(got.element == want[t].element, where + " has elements of " + std::to_string(got.element) + " bytes");
    expect(got.count == want[t].count, where + " has " + std::to_string(got.count) + " entries");
    expect(want[t].from == nullptr || got.from == want[t].from, where + " is another host table");
    bytes += (want[t].count != 0 ? want[t].count : 1) * want[t].element;
  }
  avr::StagingSize size;
  plan.visit_tables(launch, spec, size);
  expect(size.items == static_cast<int>(want.size()), name + ": the sizing pass's item count");
  expect(size.bytes == bytes, name + ": the sizing pass counts " + std::to_string(size.bytes) + " bytes");
  plan.visit_tables(launch, spec, second);
  expect(first.tables == second.tables, name + ": the plan changed under a visit");
  expect(all_null(*launch), name + ": an address of the launch is set");
  expect(std::memcmp(&spec_before, spec, sizeof(*spec)) == 0, name + ": a visit changed the spec record");
}

// ---- a frame in one piece ---------------------------------------------------------------------
void expect_step_plain(const std::string& name, const avr::FrameStep& step, bool march) {
  expect(step.march == march && step.launches && !step.chunk && step.wait_event == -1 &&
             step.record_event == -1, name + ": not a plain launch");
}
void test_whole_frames() {
  const Scene scene;
  for (avr::FrameKind kind : {avr::FrameKind::kVolume, avr::FrameKind::kMaxIntensity}) {
    for (int phases : {kClassify | kMarch, int{kClassify}, int{kMarch}}) {
      const std::string name = "frame kind " + std::to_string(static_cast<int>(kind)) + " phases " + std::to_string(phases);
      avr::FrameLaunchPlan plan;
      const avr::RenderRequest request = scene.request(phases, kind);
      expect(plan_call(&plan, request), name + ": nothing to do");
      const avr::FramePlan& pro = *plan.prologue;
      expect(pro.boxes.size() == 3 && pro.classify_tile_begin == std::vector<uint32_t>({0, 1, 3, 3}),
             name + ": the scene's tiles are not 1, 2, 0");
      expect(pro.boxes[0].rect[2] >= pro.boxes[0].rect[0] && pro.boxes[1].rect[2] >= pro.boxes[1].rect[0] &&
                 pro.boxes[2].rect[2] < pro.boxes[2].rect[0], name + ": boxes 0, 1 on screen, box 2 off");
      avr::RenderLaunch launch = plan.launch;
      avr::MarchSpecDev spec{};
      expect(all_null(launch), name + ": the plan holds an address");
      std::vector<Want> want = {{&launch.boxes_dev, sizeof(avr::BoxDev), 3, pro.boxes.data()}};
      if (phases & kClassify) want.push_back({&launch.tile_begin_dev, 4, 4, pro.classify_tile_begin.data()});
      if (phases & kMarch) {
        want.push_back({&launch.tables_dev, 4, static_cast<size_t>(pro.n_tables) * 1024, pro.tables.data()});
        want.push_back({&launch.order_dev, 4, 3, scene.order.data()});
        want.push_back({&launch.order_rects_dev, 4, 12, plan.order_rects.data()});
        want.push_back({&launch.run_end_dev, 4, 2, scene.run_end.data()});
        want.push_back({&launch.run_rects_dev, 16, 2, scene.rects.data()});
        want.push_back({&launch.run_blocks_dev, 16, 4, scene.blocks.data()});
        want.push_back({&launch.items_dev, 8, 8, plan.items->data()});
      }
      expect_tables(name, plan, want, &launch, &spec);
      // every launch argument that is not an address
      const avr::RenderLaunch& l = plan.launch;
      expect(std::memcmp(&l.consts, &pro.consts, sizeof(l.consts)) == 0, name + ": consts");
      expect(l.consts.width == 64 && l.consts.height == 48, name + ": image size");
      expect(l.n_boxes == 3 && l.n_classify_tiles == 3, name + ": boxes and tiles");
      expect(l.classify_lds_pad == kPad, name + ": the LDS reserve");
      expect(l.classify_stream_stores == 0, name + ": a volume below 256 MB is not streamed");
      expect(l.n_classify_boxes == 0 && l.pos_begin == 0 && l.pos_end == -1 && l.resume == 0 &&
                 !l.spec_is_repair, name + ": a whole frame overrides something");
      expect(plan.needs_classified, name + ": takes a classified slot");
      if (phases & kMarch) {
        expect(l.n_tables == pro.n_tables && l.n_tables >= 1, name + ": n_tables");
        expect(l.n_order == 3 && l.n_runs == 2 && l.n_pieces == 2, name + ": run counts");
        expect(std::memcmp(&l.pieces, &scene.pieces, sizeof(l.pieces)) == 0, name + ": pieces");
        // 2 x 2 super-tiles of 32 pixels, two runs: 8 items, a whole round of the XCDs
        expect(l.n_items == 8 && plan.items->size() == 8, name + ": march items");
        expect(l.workgroups_per_cu == kPerCu && l.kind == kind, name + ": occupancy cap and kind");
        // box 2 has no cells (exact divide), boxes 0 and 1 have power-of-two cells
        expect(pro.boxes[2].index_mode == avr::kExactDivide && pro.boxes[0].index_mode != avr::kExactDivide &&
                   l.only_mode == -1, name + ": only_mode of a mixed scene");
        for (int i = 0; i < 3; ++i) {
          expect(std::memcmp(&plan.order_rects[static_cast<size_t>(i) * 4], pro.boxes[static_cast<size_t>(kOrder[i])].rect, 16) == 0,
                 name + ": order_rects");
        }
      }
      size_t s = 0;
      if (phases & kClassify) expect_step_plain(name, plan.steps.at(s++), false);
      if (phases & kMarch) expect_step_plain(name, plan.steps.at(s++), true);
      expect(plan.steps.size() == s && plan.visibility_bytes == 0, name + ": the launches");
    }
  }
  {  // a projection: march only, the raw cells -- no classify table, no classified slot
    avr::FrameLaunchPlan plan;
    const avr::RenderRequest request = scene.request(kMarch, avr::FrameKind::kProjection);
    expect(plan_call(&plan, request), "projection: nothing to do");
    avr::RenderLaunch launch = plan.launch;
    avr::MarchSpecDev spec{};
    expect_tables("projection", plan,
                  {{&launch.boxes_dev, sizeof(avr::BoxDev), 3, nullptr},
                   {&launch.tables_dev, 4, static_cast<size_t>(plan.prologue->n_tables) * 1024, nullptr},
                   {&launch.order_dev, 4, 3, nullptr}, {&launch.order_rects_dev, 4, 12, nullptr},
                   {&launch.run_end_dev, 4, 2, nullptr}, {&launch.run_rects_dev, 16, 2, nullptr},
                   {&launch.run_blocks_dev, 16, 4, nullptr}, {&launch.items_dev, 8, 8, nullptr}},
                  &launch, &spec);
    expect(!plan.needs_classified, "projection: takes a classified slot");
    expect(plan.launch.kind == avr::FrameKind::kProjection && plan.launch.n_items == 8 &&
               plan.launch.n_order == 3, "projection: launch arguments");
    expect(plan.steps.size() == 1, "projection: one launch");
    expect_step_plain("projection", plan.steps[0], true);
  }
  {  // a tightened plan's spans are staged when there are any; an empty table stays null
    Scene tight;
    avr::FrameLaunchPlan plan;
    const avr::RenderRequest empty = tight.request(kMarch, avr::FrameKind::kVolume, nullptr, true);
    expect(plan_call(&plan, empty), "spans: nothing to do");
    Recorder seen;
    avr::RenderLaunch launch = plan.launch;
    avr::MarchSpecDev spec{};
    plan.visit_tables(&launch, &spec, seen);
    expect(seen.tables.size() == 8, "empty spans are named");
    tight.spans = {{0, 63, 0}, {0, 31, 320}, {1, 0, 0}};
    expect(plan_call(&plan, empty), "spans: nothing to do");
    seen.tables.clear();
    plan.visit_tables(&launch, &spec, seen);
    expect(seen.tables.size() == 9 && seen.tables[7].to == &launch.run_spans_dev &&
               seen.tables[7].element == 8 && seen.tables[7].count == 3, "spans: after the blocks");
  }
  {  // one box: only_mode is its mode; no runs: nothing to do
    Scene one;
    one.order = {0};
    one.run_end = {1};
    avr::FrameLaunchPlan plan;
    avr::RenderRequest request = {kMarch, avr::FrameKind::kVolume,
                                  {one.boxes.data(), 1, one.transform, one.params, one.camera},
                                  {one.order.data(), 1, one.run_end.data(), 1, 2, one.rects, one.blocks, nullptr, one.pieces},
                                  {0, address<float>(50), nullptr, nullptr}};
    one.rects.resize(1);
    one.blocks.resize(2);
    expect(plan_call(&plan, request), "one box: nothing to do");
    expect(plan.launch.only_mode == plan.prologue->boxes[0].index_mode && plan.launch.only_mode >= 0,
           "one box: only_mode");
    avr::RenderRequest none = {kClassify | kMarch, avr::FrameKind::kVolume,
                               {one.boxes.data(), 1, one.transform, one.params, one.camera},
                               {nullptr, 0, nullptr, 0, 1, one.rects, one.blocks, nullptr, one.pieces},
                               {0, nullptr, nullptr, nullptr}};
    expect(!plan_call(&plan, none) && plan.phases == 0 && plan.steps.empty(), "no runs: something to do");
  }
  {  // the 256 MB rule: 128 x 256 x 128 bricklets of 128 bytes are 512 MB
    Scene big;
    big.boxes.resize(1);
    big.boxes[0].dims[0] = big.boxes[0].dims[1] = 1024;
    big.boxes[0].dims[2] = 512;
    big.boxes[0].jstride = big.boxes[0].kstride = 0;  // (nothing reads a cell)
    big.order = {0};
    big.run_end = {1};
    big.rects.resize(1);
    big.blocks.resize(2);
    const avr::RenderRequest request = {int{kClassify}, avr::FrameKind::kVolume,
                                        {big.boxes.data(), 1, big.transform, big.params, big.camera},
                                        {big.order.data(), 1, big.run_end.data(), 1, 2, big.rects, big.blocks, nullptr, big.pieces},
                                        {0, nullptr, nullptr, nullptr}};
    avr::FrameLaunchPlan plan;
    expect(plan.open(request, avr::FrameChunks{}, 0, true, 0), "big: nothing to do");
    expect(plan.prologue->classified_bytes == (512ull << 20), "big: 512 MB");
    expect(plan.launch.classify_stream_stores == 1 && plan.launch.classify_lds_pad == 0, "big: streamed");
    expect(plan.open(request, avr::FrameChunks{}, 0, false, 0), "big: nothing to do");
    expect(plan.launch.classify_stream_stores == 0, "big: streamed without the setting");
  }
}

// ---- chunks -----------------------------------------------------------------------------------
uint32_t tiles_at(int position) { return kTiles[kOrder[position]]; }

void test_chunks() {
  const Scene scene;
  for (int count : {2, 3, AVR_MAX_FRAME_CHUNKS}) {
    const std::string name = std::to_string(count) + " chunks";
    // the cuts, by brute force: bound k is the first position count at which the tiles seen,
    // times the chunk count, reach the total times k
    std::vector<int> bounds(static_cast<size_t>(count) + 1, 3);
    bounds[0] = 0;
    for (int k = 1; k < count; ++k) {
      for (int p = 1; p <= 3; ++p) {
        uint64_t seen = 0;
        for (int i = 0; i < p; ++i) seen += tiles_at(i);
        if (seen * static_cast<uint64_t>(count) >= 3ull * static_cast<uint64_t>(k)) {
          bounds[static_cast<size_t>(k)] = p;
          break;
        }
      }
    }
    bool has_empty = false;
    for (int k = 0; k < count; ++k) {
      expect(bounds[static_cast<size_t>(k)] <= bounds[static_cast<size_t>(k) + 1], name + ": bounds descend");
      has_empty = has_empty || bounds[static_cast<size_t>(k)] == bounds[static_cast<size_t>(k) + 1];
    }
    expect(count < 3 || has_empty, name + ": no empty chunk");

    for (int with_events = 0; with_events < 2; ++with_events) {
      for (int first_alone = 0; first_alone < 2; ++first_alone) {
        // the classify call
        avr::FrameChunks shape;
        shape.count = count;
        shape.events = with_events != 0;
        shape.first_alone = first_alone != 0;
        avr::FrameLaunchPlan plan;
        const avr::RenderRequest classify = scene.request(kClassify);
        expect(plan_call(&plan, classify, shape), name + ": nothing to classify");
        expect(plan.bounds == bounds && plan.bounds.front() == 0 && plan.bounds.back() == 3, name + ": bounds");
        expect(plan.chunk_tile_begin.size() == static_cast<size_t>(3 + count), name + ": prefix entries");
        avr::RenderLaunch launch = plan.launch;
        avr::MarchSpecDev spec{};
        expect_tables(name + " classify", plan,
                      {{&launch.boxes_dev, sizeof(avr::BoxDev), 3, nullptr},
                       {&launch.tile_begin_dev, 4, 4, plan.prologue->classify_tile_begin.data()},
                       {&launch.tile_begin_dev, 4, static_cast<size_t>(3 + count), plan.chunk_tile_begin.data()},
                       {&launch.box_list_dev, 4, 3, scene.order.data()}},
                      &launch, &spec);
        expect(plan.steps.size() == static_cast<size_t>(count), name + ": classify steps");
        for (int k = 0; k < count; ++k) {
          const int first = bounds[static_cast<size_t>(k)], last = bounds[static_cast<size_t>(k) + 1];
          uint32_t sum = 0;
          expect(plan.chunk_tile_begin[static_cast<size_t>(first + k)] == 0, name + ": a chunk's prefix begins at bounds[k] + k");
          for (int i = first; i < last; ++i) {
            sum += tiles_at(i);
            expect(plan.chunk_tile_begin[static_cast<size_t>(i + 1 + k)] == sum, name + ": a chunk's prefix");
          }
          const avr::FrameStep& step = plan.steps[static_cast<size_t>(k)];
          const std::string where = name + " classify step " + std::to_string(k);
          expect(!step.march && step.chunk, where + ": kind");
          expect(step.launches == (last > first), where + ": an empty chunk classifies nothing");
          expect(step.record_event == (with_events ? k : -1) && step.wait_event == -1,
                 where + ": its event is recorded whether it launches or not");
          expect(step.box_list_at == first && step.n_classify_boxes == last - first &&
                     step.prefix_at == first + k && step.n_classify_tiles == sum, where + ": its list");
          expect(step.classify_lds_pad == ((k == 0 && first_alone) ? 0u : kPad), where + ": LDS reserve");
          expect(step.visible_in_at == -1, where + ": visible_in without culling");
        }
        // the march call
        const avr::RenderRequest march = scene.request(kMarch);
        expect(plan_call(&plan, march, shape), name + ": nothing to march");
        expect(plan.bounds == bounds, name + ": the march call cuts like the classify call");
        launch = plan.launch;
        Recorder seen;
        plan.visit_tables(&launch, &spec, seen);
        expect(seen.tables.size() == 8 && launch.box_list_dev == nullptr, name + ": the march call's tables");
        expect(plan.steps.size() == static_cast<size_t>(count), name + ": march steps");
        for (int k = 0; k < count; ++k) {
          const int first = bounds[static_cast<size_t>(k)], last = bounds[static_cast<size_t>(k) + 1];
          const avr::FrameStep& step = plan.steps[static_cast<size_t>(k)];
          const std::string where = name + " march step " + std::to_string(k);
          expect(step.march && step.chunk, where + ": kind");
          expect(step.launches == (last > first || k == 0), where + ": launched with boxes, or first");
          expect(step.wait_event == (with_events ? k : -1) && step.record_event == -1, where + ": waits");
          expect(step.pos_begin == first && step.pos_end == last && step.resume == (k > 0 ? 1 : 0),
                 where + ": positions and resume");
          expect(step.visible_out_at == -1, where + ": visible_out without culling");
        }
      }
    }
    // the culled call: classify 0, march 0, classify 1, march 1 ... on one stream
    avr::FrameChunks shape;
    shape.count = count;
    shape.culled = true;
    shape.first_alone = true;
    avr::FrameLaunchPlan plan;
    const avr::RenderRequest both = scene.request(kClassify | kMarch);
    expect(plan_call(&plan, both, shape), name + ": nothing to do");
    expect(plan.visibility_bytes == static_cast<size_t>(count) * 3, name + ": visibility bytes");
    expect(plan.steps.size() == static_cast<size_t>(2 * count), name + ": culled steps");
    avr::RenderLaunch staged = plan.launch;  // as render() has it after staging
    staged.box_list_dev = address<const int32_t>(33);
    staged.tile_begin_dev = address<const uint32_t>(34);
    uint8_t* const visibility = address<uint8_t>(35);
    for (int k = 0; k < count; ++k) {
      const int first = bounds[static_cast<size_t>(k)], last = bounds[static_cast<size_t>(k) + 1];
      const avr::FrameStep& c = plan.steps[static_cast<size_t>(2 * k)];
      const avr::FrameStep& m = plan.steps[static_cast<size_t>(2 * k) + 1];
      const std::string where = name + " culled chunk " + std::to_string(k);
      expect(!c.march && m.march && c.chunk && m.chunk, where + ": classify, then march");
      expect(c.launches == (last > first) && m.launches, where + ": every chunk's march is launched");
      expect(c.wait_event == -1 && c.record_event == -1 && m.wait_event == -1 && m.record_event == -1,
             where + ": no events");
      expect(c.classify_lds_pad == (k == 0 ? 0u : kPad), where + ": only chunk 0 is alone");
      expect(c.visible_in_at == (k > 0 ? int64_t{k - 1} * 3 + first : -1), where + ": visible_in");
      expect(m.visible_out_at == (k + 1 < count ? int64_t{k} * 3 : -1), where + ": visible_out");
      expect(m.resume == (k > 0 ? 1 : 0) && m.pos_begin == first && m.pos_end == last, where + ": march");
      avr::RenderLaunch one = staged;
      c.apply(visibility, &one);
      expect(one.box_list_dev == staged.box_list_dev + first && one.tile_begin_dev == staged.tile_begin_dev + first + k &&
                 one.n_classify_boxes == last - first && one.n_classify_tiles == c.n_classify_tiles &&
                 one.classify_lds_pad == c.classify_lds_pad &&
                 one.visible_in == (k > 0 ? visibility + (k - 1) * 3 + first : nullptr),
             where + ": the classify launch's overrides");
      one = staged;
      m.apply(visibility, &one);
      expect(one.visible_out == (k + 1 < count ? visibility + k * 3 : nullptr) && one.pos_begin == first &&
                 one.pos_end == last && one.resume == m.resume && one.box_list_dev == staged.box_list_dev,
             where + ": the march launch's overrides");
    }
  }
  avr::FrameLaunchPlan plan;
  avr::FrameChunks shape;
  {  // a run without boxes: every chunk is empty, and the march of chunk 0 is still launched (it
     // stores every pixel of the run's layer)
    Scene empty;
    empty.run_end = {0};
    empty.rects.resize(1);
    empty.blocks.resize(2);
    const avr::RenderRequest march = {int{kMarch}, avr::FrameKind::kVolume,
                                      {empty.boxes.data(), 3, empty.transform, empty.params, empty.camera},
                                      {nullptr, 0, empty.run_end.data(), 1, 2, empty.rects, empty.blocks, nullptr, empty.pieces},
                                      {0, address<float>(50), nullptr, nullptr}};
    shape.count = 2;
    expect(plan_call(&plan, march, shape), "no boxes: nothing to march");
    expect(plan.bounds == std::vector<int>({0, 0, 0}) && plan.steps.size() == 2 && plan.steps[0].launches &&
               plan.steps[0].resume == 0 && !plan.steps[1].launches, "no boxes: only chunk 0 marches");
  }
  // refusals
  shape.count = AVR_MAX_FRAME_CHUNKS + 1;
  const avr::RenderRequest classify = scene.request(kClassify);
  const avr::RenderRequest both = scene.request(kClassify | kMarch);
  expect_refused("invalid chunk count", [&] { plan_call(&plan, classify, shape); });
  shape.count = 0;
  expect_refused("invalid chunk count", [&] { plan_call(&plan, classify, shape); });
  shape.count = 2;
  expect_refused("a chunked frame is classified and marched by separate calls (or by avr_render_plan_culled)",
                 [&] { plan_call(&plan, both, shape); });
  Scene bad;
  bad.order = {1, 3, 0};
  const avr::RenderRequest bad_classify = bad.request(kClassify);
  expect_refused("box_order entry out of range", [&] { plan_call(&plan, bad_classify, shape); });
}

// ---- flagged and positioned classify passes ---------------------------------------------------
void test_listed() {
  const Scene scene;
  const avr::RenderRequest classify = scene.request(kClassify);
  avr::FrameLaunchPlan plan;
  {
    avr::FrameChunks shape;
    shape.flags = true;
    expect(plan_call(&plan, classify, shape), "flagged: nothing to do");
    expect(plan.flagged && !plan.positioned, "flagged: shape");
    expect(plan.listed_tile_begin == std::vector<uint32_t>({0, 2, 2, 3}) &&
               plan.listed_boxes == std::vector<int32_t>({1, 2, 0}), "flagged: the list");
    avr::RenderLaunch launch = plan.launch;
    avr::MarchSpecDev spec{};
    expect_tables("flagged", plan,
                  {{&launch.boxes_dev, sizeof(avr::BoxDev), 3, nullptr},
                   {&launch.tile_begin_dev, 4, 4, plan.prologue->classify_tile_begin.data()},
                   {&launch.tile_begin_dev, 4, 4, plan.listed_tile_begin.data()},
                   {&launch.box_list_dev, 4, 3, plan.listed_boxes.data()}},
                  &launch, &spec);
    expect(plan.launch.n_classify_boxes == 3 && plan.launch.n_classify_tiles == 3, "flagged: counts");
    expect(plan.steps.size() == 1, "flagged: one launch");
    expect_step_plain("flagged", plan.steps[0], false);
  }
  {
    const int32_t positions[2] = {0, 2};
    avr::FrameChunks shape;
    shape.classify_positions = positions;
    shape.n_classify_positions = 2;
    expect(plan_call(&plan, classify, shape), "positioned: nothing to do");
    expect(plan.flagged && plan.positioned, "positioned: shape");
    expect(plan.listed_tile_begin == std::vector<uint32_t>({0, 2, 3}) &&
               plan.listed_boxes == std::vector<int32_t>({1, 0}), "positioned: the list");
    expect(plan.launch.n_classify_boxes == 2 && plan.launch.n_classify_tiles == 3, "positioned: counts");
    expect(plan.launch.visible_in == nullptr, "positioned: visible_in");
    shape.n_classify_positions = 1;
    shape.classify_positions = positions + 1;
    expect(plan_call(&plan, classify, shape), "one position: nothing to do");
    expect(plan.launch.n_classify_boxes == 1 && plan.launch.n_classify_tiles == 1 &&
               plan.listed_boxes == std::vector<int32_t>({0}), "one position: the listed total");
    avr::RenderLaunch launch = plan.launch;
    avr::MarchSpecDev spec{};
    expect_tables("one position", plan,
                  {{&launch.boxes_dev, sizeof(avr::BoxDev), 3, nullptr}, {&launch.tile_begin_dev, 4, 4, nullptr},
                   {&launch.tile_begin_dev, 4, 2, nullptr}, {&launch.box_list_dev, 4, 1, nullptr}},
                  &launch, &spec);
  }
  const int32_t descending[2] = {2, 0}, beyond[2] = {0, 3}, many[4] = {0, 1, 2, 3}, some[1] = {1};
  auto positioned = [&](const int32_t* positions, int n, bool flags = false, int count = 1) {
    avr::FrameChunks shape;
    shape.classify_positions = positions;
    shape.n_classify_positions = n;
    shape.flags = flags;
    shape.count = count;
    plan_call(&plan, classify, shape);
  };
  expect_refused("positions must ascend within the layer order", [&] { positioned(descending, 2); });
  expect_refused("positions must ascend within the layer order", [&] { positioned(beyond, 2); });
  expect_refused("too many positions", [&] { positioned(many, 4); });
  expect_refused("flags or positions, not both", [&] { positioned(some, 1, true); });
  expect_refused("a flagged classify pass is not cut into chunks", [&] { positioned(nullptr, 0, true, 2); });
  Scene bad;
  bad.order = {1, -1, 0};
  const avr::RenderRequest bad_classify = bad.request(kClassify);
  expect_refused("box_order entry out of range", [&] {
    avr::FrameChunks shape;
    shape.flags = true;
    plan_call(&plan, bad_classify, shape);
  });
}

// ---- speculation ------------------------------------------------------------------------------
void test_speculation() {
  for (int extra = 0; extra < 2; ++extra) {  // 64x48, and 65x49: one pixel past a super-tile edge
    const Scene scene(64 + extra, 48 + extra);
    const avr::RenderRequest march = scene.request(kMarch);
    const std::string name = extra ? "65x49" : "64x48";
    // super-tiles of 32 pixels: 2 x 2 (3 x 2), times two runs, rounded up to a multiple of the 8
    // XCDs, four workgroups each
    const int64_t bound = extra ? 64 : 32;
    expect(avr::march_workgroups_bound(64 + extra, 48 + extra, 2) == bound, name + ": workgroup bound");
    avr_speculation given{};
    given.classified = address<const uint8_t>(20);
    given.visited = address<uint8_t>(21);
    given.missed = address<uint8_t>(22);
    given.miss_count = address<uint32_t>(23);
    given.host_miss_flag = address<uint32_t>(24);
    given.dirty_workgroups = address<uint8_t>(25);
    avr::FrameChunks shape;
    shape.speculation = &given;
    avr::FrameLaunchPlan plan;
    // the checking march
    expect(plan_call(&plan, march, shape), name + ": nothing to march");
    expect(static_cast<int64_t>(plan.launch.n_items) * 4 == bound, name + ": every super-tile of both runs");
    expect(!plan.launch.spec_is_repair, name + ": the checking march is no repair");
    avr::MarchSpecDev spec = avr::speculation_record(given);
    expect(spec.classified == given.classified && spec.visited == given.visited && spec.missed == given.missed &&
               spec.miss_count == given.miss_count && spec.host_miss_flag == given.host_miss_flag &&
               spec.gate == nullptr && spec.dirty_blocks_out == given.dirty_workgroups &&
               spec.dirty_blocks == nullptr, name + ": the checking march marks");
    avr::RenderLaunch launch = plan.launch;
    expect_tables(name + " checking", plan,
                  {{&launch.boxes_dev, sizeof(avr::BoxDev), 3, nullptr}, {&launch.tables_dev, 4, static_cast<size_t>(plan.prologue->n_tables) * 1024, nullptr},
                   {&launch.order_dev, 4, 3, nullptr}, {&launch.order_rects_dev, 4, 12, nullptr},
                   {&launch.run_end_dev, 4, 2, nullptr}, {&launch.run_rects_dev, 16, 2, nullptr},
                   {&launch.run_blocks_dev, 16, 4, nullptr},
                   {&launch.spec_dev, sizeof(avr::MarchSpecDev), 1, &spec},
                   {&launch.items_dev, 8, plan.launch.n_items, nullptr}},
                  &launch, &spec);
    // the gated repair march
    given.classified = nullptr;
    given.gate = given.miss_count;
    expect(plan_call(&plan, march, shape), name + ": nothing to repair");
    expect(plan.launch.spec_is_repair, name + ": the gated march is the repair");
    spec = avr::speculation_record(given);
    expect(spec.classified == nullptr && spec.gate == given.miss_count && spec.dirty_blocks_out == nullptr &&
               spec.dirty_blocks == given.dirty_workgroups, name + ": the gated march reads");
    // flags on the host travel with the call, in front of the record they go into
    const uint8_t host_flags[3] = {1, 0, 1};
    given.gate = nullptr;
    given.classified_host = host_flags;
    expect(plan_call(&plan, march, shape), name + ": nothing to march");
    spec = avr::speculation_record(given);
    launch = plan.launch;
    Recorder seen;
    plan.visit_tables(&launch, &spec, seen);
    expect(seen.tables.size() == 10 && seen.tables[7].to == &spec.classified && seen.tables[7].element == 1 &&
               seen.tables[7].count == 3 && seen.tables[7].from == host_flags &&
               seen.tables[8].to == &launch.spec_dev, name + ": host flags, then the record");
    given.classified = address<const uint8_t>(20);
    expect_refused("the flags are on the device or on the host, not both", [&] { plan_call(&plan, march, shape); });
    given.classified_host = nullptr;
    given.missed = nullptr;
    expect_refused("a speculative march that checks flags needs somewhere to report misses",
                   [&] { plan_call(&plan, march, shape); });
    given.missed = address<uint8_t>(22);
    avr::RenderRequest counted = scene.request(kMarch);
    counted.to.samples_out = address<uint64_t>(26);
    expect_refused("a speculative march is one launch and counts no samples",
                   [&] { plan_call(&plan, counted, shape); });
  }
}

// ---- kind rules, slot range, the rest of the request's rules ----------------------------------
void test_refusals() {
  const Scene scene;
  avr::FrameLaunchPlan plan;
  avr::FramePlan cached;
  const char* one_launch = "a maximum-intensity or column-projection march is one launch: no chunks, no speculation";
  for (avr::FrameKind kind : {avr::FrameKind::kMaxIntensity, avr::FrameKind::kProjection}) {
    const avr::RenderRequest march = scene.request(kMarch, kind, &cached);
    avr::FrameChunks shape;
    shape.count = 2;
    expect_refused(one_launch, [&] { plan_call(&plan, march, shape); });
    avr_speculation given{};
    shape.count = 1;
    shape.speculation = &given;
    expect_refused(one_launch, [&] { plan_call(&plan, march, shape); });
  }
  for (int phases : {kClassify | kMarch, int{kClassify}}) {
    const avr::RenderRequest request = scene.request(phases, avr::FrameKind::kProjection, &cached);
    expect_refused("a column-projection march has no classify pass", [&] { plan_call(&plan, request); });
  }
  for (int slot : {-1, AVR_CLASSIFIED_SLOTS}) {
    avr::RenderRequest request = scene.request(kMarch, avr::FrameKind::kVolume, &cached);
    request.to.slot = slot;
    expect_refused("classified slot out of range", [&] { plan_call(&plan, request); });
  }
  expect(!cached.ready && cached.boxes.empty(), "a refused request made the prologue");
  {
    avr::RenderRequest request = scene.request(kMarch);
    request.runs.n_pieces = 0;
    expect_refused("invalid run description", [&] { plan_call(&plan, request); });
    request.runs.n_pieces = 2;
    request.to.out_layers = nullptr;
    expect_refused("null output image", [&] { plan_call(&plan, request); });
    request.to.out_layers = address<float>(50);
    request.runs.run_end = nullptr;
    expect_refused("null run_end", [&] { plan_call(&plan, request); });
    request.runs.run_end = scene.run_end.data();
    request.runs.box_order = nullptr;
    expect_refused("null box_order", [&] { plan_call(&plan, request); });
  }
  {
    Scene bad;
    bad.blocks.pop_back();
    const avr::RenderRequest tables = bad.request(kMarch);
    expect_refused("run tables do not match the runs", [&] { plan_call(&plan, tables); });
    bad = Scene();
    bad.run_end = {2, 1};
    const avr::RenderRequest descending = bad.request(kMarch);
    expect_refused("run_end must be non-decreasing", [&] { plan_call(&plan, descending); });
    bad.run_end = {1, 2};
    const avr::RenderRequest short_runs = bad.request(kMarch);
    expect_refused("runs must cover box_order", [&] { plan_call(&plan, short_runs); });
    bad.run_end = {2, 3};
    bad.order = {1, 2, 3};
    const avr::RenderRequest range = bad.request(kMarch);
    expect_refused("box_order entry out of range", [&] { plan_call(&plan, range); });
  }
}

// ---- the classification key -------------------------------------------------------------------
std::vector<uint64_t> key_of(const Scene& scene) {
  avr::FrameLaunchPlan plan;
  const avr::RenderRequest request = scene.request(kClassify);
  expect(plan.open(request, avr::FrameChunks{}, kPad, kStream, kPerCu), "key: nothing to do");
  return avr::classification_key(*plan.prologue);
}
void test_key() {
  const Scene scene;
  const std::vector<uint64_t> key = key_of(scene);
  expect(key.size() == 7 + 3 * 4, "key: length");
  expect(key == key_of(Scene()), "key: equal requests differ");
  Scene other;
  other.params.scalar_range[0] = 0.125f;
  expect(key != key_of(other), "key: range_min");
  other = Scene();
  other.transform.log_scale_input = 1;
  expect(key != key_of(other), "key: the log flag");
  other = Scene();
  other.boxes[1].cells = address<const double>(45);
  expect(key != key_of(other), "key: a box's cells");
  other = Scene();
  other.boxes[0].jstride = 16;
  other.boxes[0].kstride = 64;
  expect(key != key_of(other), "key: jstride");
  other = Scene();
  other.boxes[0].dims[2] = 3;  // (the same bricklets: only the dimension differs)
  expect(key != key_of(other), "key: a dimension");
  avr::FrameLaunchPlan plan;
  const avr::RenderRequest request = scene.request(kClassify);
  expect(plan.open(request, avr::FrameChunks{}, kPad, kStream, kPerCu), "key: nothing to do");
  avr::FramePlan moved = *plan.prologue;
  moved.boxes[1].cls_offset += 128;
  expect(key != avr::classification_key(moved), "key: cls_offset");
}

// ---- the cached prologue ----------------------------------------------------------------------
void test_cached() {
  const Scene scene;
  avr::FramePlan cached;
  avr::FrameLaunchPlan plan;
  const avr::RenderRequest classify = scene.request(kClassify, avr::FrameKind::kVolume, &cached);
  const avr::RenderRequest march = scene.request(kMarch, avr::FrameKind::kVolume, &cached);
  expect(plan_call(&plan, classify), "cached: nothing to classify");
  expect(cached.ready && plan.prologue == &cached && !cached.march_items_ready, "cached: the classify call makes the prologue");
  expect(plan_call(&plan, march), "cached: nothing to march");
  expect(cached.march_items_ready && plan.items == &cached.march_items && cached.march_items.size() == 8,
         "cached: the march call makes the items");
  const avr::MarchItemDev* data = cached.march_items.data();
  const std::vector<uint32_t> slots = {cached.march_items[0].slot, cached.march_items[7].slot};
  cached.march_items[0].run = 12345;  // a rebuild would put the run back
  expect(plan_call(&plan, march), "cached: nothing to march");
  expect(cached.march_items.data() == data && cached.march_items[0].run == 12345 &&
             cached.march_items[0].slot == slots[0] && cached.march_items[7].slot == slots[1] &&
             plan.launch.n_items == 8, "cached: the items were built again");
  // without a cached prologue the plan keeps its own, and builds the items every call
  avr::FrameLaunchPlan own;
  const avr::RenderRequest uncached = scene.request(kMarch);
  expect(plan_call(&own, uncached) && own.prologue != &cached && own.items != &cached.march_items &&
             own.items->size() == 8, "uncached: the plan's own prologue and items");
}

}  // namespace

int main() {
  test_whole_frames();
  test_chunks();
  test_listed();
  test_speculation();
  test_refusals();
  test_key();
  test_cached();
  std::printf("ok\n");
  return 0;
}
