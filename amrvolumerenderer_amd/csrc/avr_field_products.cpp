// C ABI of the field products (include/avr_hip.h): the joint histogram, slice images, on-axis
// projections, derived fields, gradient fields, clumps, their table, links, members and pair
// energies, isosurfaces, streamlines, covering grids, grid fields, particle fields, particle groups, rays, per-ray sums, ray transfer, power spectra, inverse transforms, the per-mode operators, structure functions and velocity cubes.  Every rule on a call's plain arguments and boxes, what it
// stages in which order, the counts it launches with and its scratch layout are its plan's
// (avr_field_plans.h, host only, tested without a GPU); what is left here needs the device.  The
// stager of a plan's tables (stage_tables) is avr_context.h's, shared with the frame path.
#include "avr_context.h"
#include "avr_field_plans.h"

using avr::bind_device;
using avr::guarded;
using avr::require;
using avr::stage_tables;

namespace {

// Where a part of a context scratch block lies; null for an optional part the call does without.
template <class T>
T* scratch_part(const avr::DeviceBuffer& block, const avr::ScratchPart& part) {
  if (!part.present) return nullptr;
  return reinterpret_cast<T*>(static_cast<char*>(block.data) + part.offset);
}

// A field of a product over several scenes that share a box list (the box rules themselves are
// avr_field_boxes.h's).
void require_field_scene(const avr_context* ctx, const avr_scene* field, size_t n_boxes) {
  require(field->ctx == ctx && field->boxes.size() == n_boxes,
          "the scenes must belong to the context and hold the same number of boxes");
}

}  // namespace

// The entry points below read the same way, top to bottom: bind the device; refuse null
// handles and device pointers; refuse scenes of another context or box count (require_field_scene);
// make the plan, which holds every rule on the plain arguments and the boxes; the call's side
// effects on its outputs (a written scene's classification keys, a cleared count); return where
// there is nothing to launch; copy the plan's launch arguments, stage its tables (stage_tables)
// and set the remaining addresses -- the scratch block's parts, the caller's arrays; launch.  The
// plan fills every launch argument that is not a device address, the entry point only addresses.
extern "C" {

int avr_scene_joint_histogram(avr_context* ctx, const avr_scene* scene_x, const avr_scene* scene_y,
                              const avr_scene* scene_s, const double* x_edges, int nx,
                              const double* y_edges, int ny, int n_levels, uint64_t* cells_dev,
                              double* sums_dev, uint64_t* totals_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(scene_x != nullptr && cells_dev != nullptr && totals_dev != nullptr, "null argument");
    require(scene_s == nullptr || sums_dev != nullptr, "a summed field needs sums_dev");
    const size_t n_boxes = scene_x->boxes.size();
    for (const avr_scene* field : {scene_x, scene_y, scene_s}) {
      if (field != nullptr) require_field_scene(ctx, field, n_boxes);
    }
    const avr::JointHistogramPlan plan = avr::plan_joint_histogram(
        scene_x->boxes.data(), scene_y != nullptr ? scene_y->boxes.data() : nullptr,
        scene_s != nullptr ? scene_s->boxes.data() : nullptr, n_boxes, x_edges, nx, y_edges, ny,
        n_levels);
    if (plan.args.n_tiles == 0) return AVR_OK;
    avr::JointHistogramArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.cells = reinterpret_cast<unsigned long long*>(cells_dev);
    args.sums = scene_s != nullptr ? sums_dev : nullptr;
    args.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    return avr::launch_joint_histogram(args, scene_y != nullptr, scene_s != nullptr, ctx->stream);
  });
}

int avr_slice_scene(avr_context* ctx, const avr_scene* scene, const double origin[3],
                    const double du[3], const double dv[3], int width, int height,
                    const int32_t* global_index, double* value, int8_t* level, int32_t* box) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(scene != nullptr && origin != nullptr && du != nullptr && dv != nullptr &&
                value != nullptr && level != nullptr && box != nullptr, "null argument");
    const avr::SlicePlan plan = avr::plan_slice(scene->boxes.data(), scene->boxes.size(),
                                                global_index, origin, du, dv, width, height);
    avr::SliceArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    return avr::launch_slice(plan.plane, args.width, args.height, args.boxes, args.n_boxes, value,
                             level, box, ctx->stream);
  });
}

int avr_scene_axis_projection(avr_context* ctx, const avr_scene* scene_f, const avr_scene* scene_w,
                              int axis, const double origin_uv[2], double du, double dv, int width,
                              int height, const double* level_dl, int n_levels,
                              double* integral_dev, double* weight_dev, double* length_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(scene_f != nullptr && origin_uv != nullptr && level_dl != nullptr &&
                integral_dev != nullptr && length_dev != nullptr, "null argument");
    require((scene_w != nullptr) == (weight_dev != nullptr),
            "weight_dev is given exactly when scene_w is");
    const bool weighted = scene_w != nullptr;
    const size_t n_boxes = scene_f->boxes.size();
    require_field_scene(ctx, scene_f, n_boxes);
    if (weighted) require_field_scene(ctx, scene_w, n_boxes);
    const avr::AxisProjectionPlan plan = avr::plan_axis_projection(
        scene_f->boxes.data(), weighted ? scene_w->boxes.data() : nullptr, n_boxes, axis, origin_uv,
        du, dv, width, height, level_dl, n_levels);
    ctx->axis_planes.reserve(plan.scratch.total, ctx->stream, "avr_scene_axis_projection",
                             "hipMalloc(axis planes)");
    avr::AxisReduceArgs reduce = plan.reduce;
    avr::AxisGatherArgs gather = plan.gather;
    stage_tables(ctx, plan, &reduce, &gather);
    reduce.plane_s = scratch_part<double>(ctx->axis_planes, plan.scratch.s);
    reduce.plane_w = scratch_part<double>(ctx->axis_planes, plan.scratch.w);
    reduce.plane_n = scratch_part<uint32_t>(ctx->axis_planes, plan.scratch.n);
    const int status = avr::launch_axis_reduce(reduce, axis, weighted, ctx->stream);
    if (status != AVR_OK) return status;
    gather.plane_s = reduce.plane_s;
    gather.plane_w = reduce.plane_w;
    gather.plane_n = reduce.plane_n;
    gather.integral = integral_dev;
    gather.weight = weight_dev;
    gather.length = length_dev;
    return avr::launch_axis_gather(gather, ctx->stream);
  });
}

int avr_scene_derive(avr_context* ctx, const avr_scene* const* inputs, int n_inputs, avr_scene* out,
                     const uint32_t* instructions, int n_instructions, const double* constants,
                     int n_constants, const double* box_origin, const double* level_cell_size,
                     int n_levels) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(out != nullptr && instructions != nullptr && level_cell_size != nullptr,
            "null argument");
    avr::require_derive_input_count(n_inputs);
    require(n_inputs == 0 || inputs != nullptr, "null argument");
    require(out->ctx == ctx, "the scenes must belong to the context");
    const size_t n_boxes = out->boxes.size();
    const avr_box* input_boxes[avr::kDeriveMaxFields] = {};
    for (int f = 0; f < n_inputs; ++f) {
      require(inputs[f] != nullptr, "null argument");
      require_field_scene(ctx, inputs[f], n_boxes);
      input_boxes[f] = inputs[f]->boxes.data();
    }
    const avr::DerivePlan plan = avr::plan_derive(
        input_boxes, n_inputs, out->boxes.data(), n_boxes, instructions, n_instructions, constants,
        n_constants, box_origin, level_cell_size, n_levels);
    for (auto& key : out->classified_key) key.clear();
    if (plan.args.n_tiles == 0) return AVR_OK;
    avr::DeriveArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    return avr::launch_derive(args, ctx->stream);
  });
}

int avr_scene_gradient(avr_context* ctx, const avr_scene* in, avr_scene* out, int axis,
                       const int32_t* box_index_lo, const int32_t* level_ratio,
                       const double* level_cell_size, int n_levels) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(in != nullptr && out != nullptr && level_cell_size != nullptr, "null argument");
    require(out->ctx == ctx, "the scenes must belong to the context");
    const size_t n_boxes = out->boxes.size();
    require_field_scene(ctx, in, n_boxes);
    const avr::GradientPlan plan =
        avr::plan_gradient(in->boxes.data(), out->boxes.data(), n_boxes, axis, box_index_lo,
                           level_ratio, level_cell_size, n_levels);
    for (auto& key : out->classified_key) key.clear();
    if (plan.args.n_tiles == 0) return AVR_OK;
    ctx->gradient_planes.reserve(plan.scratch.total, ctx->stream, "avr_scene_gradient",
                                 "hipMalloc(gradient planes)");
    avr::GradientArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.face_value = scratch_part<double>(ctx->gradient_planes, plan.scratch.face_value);
    args.face_present = scratch_part<uint8_t>(ctx->gradient_planes, plan.scratch.face_present);
    return avr::launch_gradient(args, axis, ctx->stream);
  });
}

int avr_scene_clumps(avr_context* ctx, const avr_scene* in, avr_scene* out, double lower,
                     double upper, const int32_t* box_index_lo, const int32_t* level_ratio,
                     int n_levels, uint64_t* count_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(in != nullptr && out != nullptr && count_dev != nullptr, "null argument");
    require(out->ctx == ctx, "the scenes must belong to the context");
    const size_t n_boxes = out->boxes.size();
    require_field_scene(ctx, in, n_boxes);
    const avr::ClumpPlan plan = avr::plan_clumps(in->boxes.data(), out->boxes.data(), n_boxes,
                                                 lower, upper, box_index_lo, level_ratio, n_levels);
    for (auto& key : out->classified_key) key.clear();
    avr::hip_check(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), ctx->stream), "hipMemsetAsync");
    if (plan.args.n_tiles == 0) return AVR_OK;
    ctx->clump_parents.reserve(plan.scratch.total, ctx->stream, "avr_scene_clumps",
                               "hipMalloc(clump parents)");
    avr::ClumpArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.parent = scratch_part<uint32_t>(ctx->clump_parents, plan.scratch.parent);
    args.chunk_roots = scratch_part<uint32_t>(ctx->clump_parents, plan.scratch.chunk_roots);
    args.count = reinterpret_cast<unsigned long long*>(count_dev);
    return avr::launch_clumps(args, ctx->stream);
  });
}

int avr_scene_clump_table(avr_context* ctx, const avr_scene* labels, const avr_scene* field,
                          uint64_t n_clumps, int n_levels, uint64_t* cells_dev, double* sums_dev,
                          uint64_t* totals_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(labels != nullptr && cells_dev != nullptr && totals_dev != nullptr, "null argument");
    require((field != nullptr) == (sums_dev != nullptr), "sums_dev is given exactly when field is");
    const size_t n_boxes = labels->boxes.size();
    require_field_scene(ctx, labels, n_boxes);
    if (field != nullptr) require_field_scene(ctx, field, n_boxes);
    const avr::ClumpTablePlan plan = avr::plan_clump_table(
        labels->boxes.data(), field != nullptr ? field->boxes.data() : nullptr, n_boxes, n_clumps,
        n_levels);
    if (plan.args.n_tiles == 0) return AVR_OK;
    avr::ClumpTableArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.cells = reinterpret_cast<unsigned long long*>(cells_dev);
    args.sums = sums_dev;
    args.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    return avr::launch_clump_table(args, field != nullptr, ctx->stream);
  });
}

int avr_scene_clump_links(avr_context* ctx, const avr_scene* labels, const avr_scene* parents,
                          uint64_t n_clumps, uint64_t n_parents, const int32_t* box_index_lo,
                          const int32_t* level_ratio, int n_levels, int32_t* extent_dev,
                          uint32_t* parent_lo_dev, uint32_t* parent_hi_dev, uint64_t* totals_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(labels != nullptr && extent_dev != nullptr && totals_dev != nullptr, "null argument");
    require((parents != nullptr) == (parent_lo_dev != nullptr) &&
                (parents != nullptr) == (parent_hi_dev != nullptr),
            "parent_lo_dev and parent_hi_dev are given exactly when parents is");
    const size_t n_boxes = labels->boxes.size();
    require_field_scene(ctx, labels, n_boxes);
    if (parents != nullptr) require_field_scene(ctx, parents, n_boxes);
    const avr::ClumpLinksPlan plan = avr::plan_clump_links(
        labels->boxes.data(), parents != nullptr ? parents->boxes.data() : nullptr, n_boxes,
        n_clumps, n_parents, box_index_lo, level_ratio, n_levels);
    if (plan.args.n_tiles == 0) return AVR_OK;
    avr::ClumpLinkArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.extent = extent_dev;
    args.parent_lo = parent_lo_dev;
    args.parent_hi = parent_hi_dev;
    args.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    return avr::launch_clump_links(args, parents != nullptr, ctx->stream);
  });
}

int avr_scene_clump_members(avr_context* ctx, const avr_scene* labels, uint64_t n_clumps,
                            const uint8_t* wanted_dev, uint64_t capacity, uint64_t* keys_dev,
                            uint64_t* count_dev, uint64_t* totals_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(labels != nullptr && wanted_dev != nullptr && keys_dev != nullptr &&
                count_dev != nullptr && totals_dev != nullptr, "null argument");
    const size_t n_boxes = labels->boxes.size();
    require_field_scene(ctx, labels, n_boxes);
    const avr::ClumpMembersPlan plan =
        avr::plan_clump_members(labels->boxes.data(), n_boxes, n_clumps, capacity);
    avr::hip_check(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), ctx->stream), "hipMemsetAsync");
    if (plan.args.n_tiles == 0) return AVR_OK;
    avr::ClumpMembersArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.wanted = wanted_dev;
    args.keys = reinterpret_cast<unsigned long long*>(keys_dev);
    args.cursor = reinterpret_cast<unsigned long long*>(count_dev);
    args.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    return avr::launch_clump_members(args, ctx->stream);
  });
}

int avr_scene_clump_member_data(avr_context* ctx, const avr_scene* scene, const uint64_t* keys_dev,
                                uint64_t n_members, const avr_scene* field, double* values_dev,
                                const int32_t* box_index_lo, const int32_t* level_ratio,
                                const double* level_cell_size, const double* prob_lo, int n_levels,
                                double* centres_dev, uint8_t* levels_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(scene != nullptr, "null argument");
    require((field != nullptr) == (values_dev != nullptr),
            "values_dev is given exactly when field is");
    require((centres_dev != nullptr) == (levels_dev != nullptr),
            "centres_dev and levels_dev are given together");
    require(values_dev != nullptr || centres_dev != nullptr, "no output is asked for");
    require(n_members == 0 || keys_dev != nullptr, "null argument");
    const size_t n_boxes = scene->boxes.size();
    require_field_scene(ctx, scene, n_boxes);
    if (field != nullptr) require_field_scene(ctx, field, n_boxes);
    const avr::ClumpMemberDataPlan plan = avr::plan_clump_member_data(
        scene->boxes.data(), field != nullptr ? field->boxes.data() : nullptr, n_boxes, n_members,
        box_index_lo, level_ratio, level_cell_size, prob_lo, n_levels);
    if (n_members == 0) return AVR_OK;
    avr::ClumpMemberDataArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.keys = reinterpret_cast<const unsigned long long*>(keys_dev);
    args.values = values_dev;
    args.centres = centres_dev;
    args.levels_out = levels_dev;
    return avr::launch_clump_member_data(args, ctx->stream);
  });
}

int avr_clump_pair_energy(avr_context* ctx, const int64_t* offsets_host, uint64_t n_segments,
                          const double* x_dev, const double* y_dev, const double* z_dev,
                          const double* m_dev, double* w_dev, int64_t* depth_host) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(offsets_host != nullptr, "null argument");
    require(n_segments == 0 || w_dev != nullptr, "null argument");
    const avr::ClumpPairsPlan plan = avr::plan_clump_pairs(offsets_host, n_segments);
    require(offsets_host[n_segments] == 0 || (x_dev != nullptr && y_dev != nullptr &&
                                              z_dev != nullptr && m_dev != nullptr),
            "null argument");
    if (depth_host != nullptr) std::copy(plan.depth.begin(), plan.depth.end(), depth_host);
    if (n_segments == 0) return AVR_OK;
    ctx->clump_pair_partials.reserve(plan.scratch_bytes, ctx->stream, "avr_clump_pair_energy",
                                     "hipMalloc(clump pair partials)");
    avr::ClumpPairArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.x = x_dev;
    args.y = y_dev;
    args.z = z_dev;
    args.m = m_dev;
    args.partial = static_cast<double*>(ctx->clump_pair_partials.data);
    args.w = w_dev;
    return avr::launch_clump_pairs(args, ctx->stream);
  });
}

int avr_scene_isosurface(avr_context* ctx, const avr_scene* field, const avr_scene* sample,
                         double value, const int32_t* box_index_lo, const int32_t* level_ratio,
                         const double* level_cell_size, const double* prob_lo, int n_levels,
                         uint64_t capacity, double* vertices_dev, uint8_t* levels_dev,
                         double* samples_dev, uint64_t* counts_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(field != nullptr && level_cell_size != nullptr && prob_lo != nullptr &&
                counts_dev != nullptr, "null argument");
    const size_t n_boxes = field->boxes.size();
    require_field_scene(ctx, field, n_boxes);
    if (sample != nullptr) require_field_scene(ctx, sample, n_boxes);
    const avr::IsoPlan plan = avr::plan_isosurface(
        field->boxes.data(), sample != nullptr ? sample->boxes.data() : nullptr, n_boxes, value,
        box_index_lo, level_ratio, level_cell_size, prob_lo, n_levels, capacity, vertices_dev,
        levels_dev, samples_dev, counts_dev);
    avr::hip_check(hipMemsetAsync(counts_dev, 0, 2 * sizeof(uint64_t), ctx->stream),
                   "hipMemsetAsync");
    if (plan.args.n_bases == 0) return AVR_OK;
    const bool has_sample = sample != nullptr, emit = capacity > 0;
    ctx->iso_scratch.reserve(plan.scratch.total, ctx->stream, "avr_scene_isosurface",
                             "hipMalloc(isosurface scratch)");
    avr::IsoArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    const avr::IsoScratch& scratch = plan.scratch;
    args.shell_value = scratch_part<double>(ctx->iso_scratch, scratch.shell_value);
    args.shell_sample = scratch_part<double>(ctx->iso_scratch, scratch.shell_sample);
    args.chunk_offset = scratch_part<unsigned long long>(ctx->iso_scratch, scratch.chunk_offset);
    args.chunk_triangles = scratch_part<uint32_t>(ctx->iso_scratch, scratch.chunk_triangles);
    args.chunk_skipped = scratch_part<uint32_t>(ctx->iso_scratch, scratch.chunk_skipped);
    args.shell_code = scratch_part<uint8_t>(ctx->iso_scratch, scratch.shell_code);
    args.counts = reinterpret_cast<unsigned long long*>(counts_dev);
    args.vertices = vertices_dev;
    args.levels_out = levels_dev;
    args.samples = has_sample ? samples_dev : nullptr;
    return avr::launch_isosurface(args, has_sample, emit, ctx->stream);
  });
}

int avr_scene_streamlines(avr_context* ctx, const avr_scene* vx, const avr_scene* vy,
                          const avr_scene* vz, const avr_scene* sample, const double* seeds_dev,
                          uint64_t n_seeds, double step, int direction, uint64_t max_steps,
                          const int32_t* box_index_lo, const int32_t* level_ratio,
                          const double* level_cell_size, const double* prob_lo, int n_levels,
                          double* points_dev, double* samples_dev, uint32_t* counts_dev,
                          uint8_t* status_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(vx != nullptr && vy != nullptr && vz != nullptr && level_cell_size != nullptr &&
                prob_lo != nullptr, "null argument");
    const size_t n_boxes = vx->boxes.size();
    require_field_scene(ctx, vx, n_boxes);
    require_field_scene(ctx, vy, n_boxes);
    require_field_scene(ctx, vz, n_boxes);
    if (sample != nullptr) require_field_scene(ctx, sample, n_boxes);
    const avr::StreamPlan plan = avr::plan_streamlines(
        vx->boxes.data(), vy->boxes.data(), vz->boxes.data(),
        sample != nullptr ? sample->boxes.data() : nullptr, n_boxes, n_seeds, step, direction,
        max_steps, box_index_lo, level_ratio, level_cell_size, prob_lo, n_levels, seeds_dev,
        points_dev, samples_dev, counts_dev, status_dev);
    if (n_seeds == 0) return AVR_OK;
    avr::StreamArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.seeds = seeds_dev;
    args.points = points_dev;
    args.samples = sample != nullptr ? samples_dev : nullptr;
    args.counts = counts_dev;
    args.status = status_dev;
    return avr::launch_streamlines(args, sample != nullptr, ctx->stream);
  });
}

int avr_scene_covering_grid(avr_context* ctx, const avr_scene* field, int level, const int32_t* lo,
                            const int32_t* dims, const int32_t* box_index_lo,
                            const int32_t* level_ratio, int n_levels, double fill,
                            double* values_dev, double* coverage_dev, int8_t* level_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(field != nullptr && lo != nullptr && dims != nullptr && values_dev != nullptr,
            "null argument");
    const size_t n_boxes = field->boxes.size();
    require_field_scene(ctx, field, n_boxes);
    const avr::CoveringGridPlan plan = avr::plan_covering_grid(
        field->boxes.data(), n_boxes, level, lo, dims, box_index_lo, level_ratio, n_levels, fill,
        values_dev, coverage_dev, level_dev);
    avr::CoverArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.values = values_dev;
    args.coverage = coverage_dev;
    args.cell_level = level_dev;
    return avr::launch_covering_grid(args, ctx->stream);
  });
}

int avr_scene_grid_field(avr_context* ctx, avr_scene* out, const double* grid_dev, int level,
                         const int32_t* lo, const int32_t* dims, const int32_t* box_index_lo,
                         const int32_t* level_ratio, int n_levels, int interpolation, int periodic,
                         double fill, int64_t* totals_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(out != nullptr && grid_dev != nullptr && lo != nullptr && dims != nullptr &&
                totals_dev != nullptr, "null argument");
    const size_t n_boxes = out->boxes.size();
    require_field_scene(ctx, out, n_boxes);
    const avr::GridFieldPlan plan = avr::plan_grid_field(
        out->boxes.data(), n_boxes, level, lo, dims, box_index_lo, level_ratio, n_levels,
        interpolation, periodic, fill, grid_dev, totals_dev);
    for (auto& key : out->classified_key) key.clear();
    if (plan.args.n_tiles == 0) return AVR_OK;
    avr::GridFieldArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.grid = grid_dev;
    args.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    return avr::launch_grid_field(args, ctx->stream);
  });
}

int avr_scene_particle_cells(avr_context* ctx, const avr_scene* scene, const double* points_dev,
                             uint64_t n, const double* values_dev, int method,
                             const int32_t* box_index_lo, const int32_t* level_ratio,
                             const double* level_cell_size, const double* prob_lo, int n_levels,
                             int64_t* cells_dev, double* shares_dev, uint8_t* levels_dev,
                             int64_t* totals_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(scene != nullptr, "null argument");
    const size_t n_boxes = scene->boxes.size();
    require_field_scene(ctx, scene, n_boxes);
    const avr::ParticleCellsPlan plan = avr::plan_particle_cells(
        scene->boxes.data(), n_boxes, n, method, box_index_lo, level_ratio, level_cell_size,
        prob_lo, n_levels, points_dev, values_dev, cells_dev, shares_dev, levels_dev, totals_dev);
    if (n == 0) return AVR_OK;
    avr::ParticleCellsArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.points = points_dev;
    args.values = values_dev;
    args.cells = reinterpret_cast<long long*>(cells_dev);
    args.shares = shares_dev;
    args.levels_out = levels_dev;
    args.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    return avr::launch_particle_cells(args, method, ctx->stream);
  });
}

int avr_scene_particle_deposit(avr_context* ctx, avr_scene* out, const int64_t* cells_sorted_dev,
                               const double* shares_sorted_dev, uint64_t n_contributions,
                               int quantity, const double* level_cell_size, int n_levels) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(out != nullptr, "null argument");
    const size_t n_boxes = out->boxes.size();
    require_field_scene(ctx, out, n_boxes);
    const avr::ParticleDepositPlan plan = avr::plan_particle_deposit(
        out->boxes.data(), n_boxes, n_contributions, quantity, level_cell_size, n_levels,
        cells_sorted_dev, shares_sorted_dev);
    for (auto& key : out->classified_key) key.clear();
    if (plan.args.n_tiles == 0) return AVR_OK;
    avr::ParticleDepositArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.cells = reinterpret_cast<const long long*>(cells_sorted_dev);
    args.shares = shares_sorted_dev;
    return avr::launch_particle_deposit(args, quantity, ctx->stream);
  });
}

int avr_particle_group_cells(avr_context* ctx, const double* points_dev, uint64_t n,
                             const double* lo, const double* hi, const int32_t* dims,
                             const int32_t* periodic, uint32_t* cells_dev, uint32_t* parent_dev,
                             uint64_t* totals_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    const avr::ParticleGroupCellsPlan plan = avr::plan_particle_group_cells(
        n, lo, hi, dims, periodic, points_dev, cells_dev, parent_dev, totals_dev);
    if (n == 0) return AVR_OK;
    avr::ParticleGroupCellsArgs args = plan.args;
    args.points = points_dev;
    args.cells = cells_dev;
    args.parent = parent_dev;
    args.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    return avr::launch_particle_group_cells(args, ctx->stream);
  });
}

int avr_particle_groups(avr_context* ctx, const double* points_sorted_dev,
                        const int64_t* order_dev, const int64_t* cell_begin_dev, uint64_t n,
                        uint64_t n_inside, double b, const double* lo, const double* hi,
                        const int32_t* dims, const int32_t* periodic, int64_t min_members,
                        uint32_t* parent_dev, int32_t* labels_dev, uint32_t* sizes_dev,
                        uint64_t* n_groups_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    const avr::ParticleGroupsPlan plan = avr::plan_particle_groups(
        n, n_inside, b, lo, hi, dims, periodic, min_members, points_sorted_dev, order_dev,
        cell_begin_dev, parent_dev, labels_dev, sizes_dev, n_groups_dev);
    if (n == 0) {
      avr::hip_check(hipMemsetAsync(n_groups_dev, 0, sizeof(uint64_t), ctx->stream),
                     "hipMemsetAsync");
      return AVR_OK;
    }
    ctx->group_counts.reserve(plan.scratch.total, ctx->stream, "avr_particle_groups",
                              "hipMalloc(particle group counts)");
    avr::ParticleGroupsArgs args = plan.args;
    args.points = points_sorted_dev;
    args.order = reinterpret_cast<const long long*>(order_dev);
    args.cell_begin = reinterpret_cast<const long long*>(cell_begin_dev);
    args.parent = parent_dev;
    args.labels = labels_dev;
    args.sizes = sizes_dev;
    args.chunk_counts = scratch_part<uint32_t>(ctx->group_counts, plan.scratch.chunk_counts);
    args.n_groups = reinterpret_cast<unsigned long long*>(n_groups_dev);
    return avr::launch_particle_groups(args, ctx->stream);
  });
}

int avr_scene_rays(avr_context* ctx, const avr_scene* field, const double* start_dev,
                   const double* end_dev, uint64_t n_rays, uint64_t max_trips,
                   const int32_t* box_index_lo, const int32_t* level_ratio,
                   const double* level_cell_size, const double* prob_lo, int n_levels,
                   const int64_t* offsets_dev, uint64_t n_segments, uint32_t* counts_dev,
                   uint8_t* status_dev, double* span_dev, double* t0_dev, double* t1_dev,
                   int8_t* level_dev, double* value_dev, double* integral_dev,
                   double* covered_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    // the scene first, without which nothing can be looked at; every other rule, a null
    // level_cell_size or prob_lo included, is plan_rays' in its documented order
    require(field != nullptr, "null argument");
    const size_t n_boxes = field->boxes.size();
    require_field_scene(ctx, field, n_boxes);
    const bool emit = offsets_dev != nullptr;
    const avr::RayPlan plan = avr::plan_rays(
        field->boxes.data(), n_boxes, n_rays, max_trips, box_index_lo, level_ratio,
        level_cell_size, prob_lo, n_levels, start_dev, end_dev, offsets_dev,
        emit ? n_segments : 0, counts_dev, status_dev, span_dev, t0_dev, t1_dev, level_dev,
        value_dev, integral_dev, covered_dev);
    if (n_rays == 0) return AVR_OK;
    avr::RayArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.start = start_dev;
    args.end = end_dev;
    if (emit) {
      args.offsets = reinterpret_cast<const long long*>(offsets_dev);
      args.t0 = t0_dev;
      args.t1 = t1_dev;
      args.level = level_dev;
      args.value = value_dev;
      args.integral = integral_dev;
      args.covered = covered_dev;
    } else {
      args.counts = counts_dev;
      args.status = status_dev;
      args.span = span_dev;
    }
    return avr::launch_rays(args, emit, ctx->stream);
  });
}

int avr_scene_ray_sums(avr_context* ctx, const avr_scene* field, const avr_scene* weight,
                       const double* start_dev, const double* end_dev, uint64_t n_rays,
                       uint64_t max_trips, const int32_t* box_index_lo,
                       const int32_t* level_ratio, const double* level_cell_size,
                       const double* prob_lo, int n_levels, uint32_t* counts_dev,
                       uint8_t* status_dev, double* span_dev, double* integral_dev,
                       double* weight_dev, double* counted_dev, double* covered_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    // as avr_scene_rays: the scenes first, every other rule is plan_ray_sums' in its order
    require(field != nullptr, "null argument");
    const size_t n_boxes = field->boxes.size();
    require_field_scene(ctx, field, n_boxes);
    if (weight != nullptr) require_field_scene(ctx, weight, weight->boxes.size());
    const avr::RaySumsPlan plan = avr::plan_ray_sums(
        field->boxes.data(), n_boxes, weight != nullptr ? weight->boxes.data() : nullptr,
        weight != nullptr ? weight->boxes.size() : 0, n_rays, max_trips, box_index_lo,
        level_ratio, level_cell_size, prob_lo, n_levels, start_dev, end_dev, counts_dev,
        status_dev, span_dev, integral_dev, weight_dev, counted_dev, covered_dev);
    if (n_rays == 0) return AVR_OK;
    avr::RayArgs args = plan.walk.args;
    stage_tables(ctx, plan, &args);
    args.start = start_dev;
    args.end = end_dev;
    args.counts = counts_dev;
    args.status = status_dev;
    args.span = span_dev;
    args.integral = integral_dev;
    args.weight = weight_dev;
    args.counted = counted_dev;
    args.covered = covered_dev;
    return avr::launch_ray_sums(args, ctx->stream);
  });
}

int avr_context_set_ray_transfer_chunk(avr_context* ctx, int channels) {
  return guarded([&]() -> int {
    require(ctx != nullptr, "null argument");
    require(channels >= 0 && channels <= avr::kTransferMaxChunk,
            "the chunk holds at most 32 channels");
    ctx->ray_transfer_chunk = channels == 0 ? avr::kTransferChunk : channels;
    return AVR_OK;
  });
}

int avr_scene_ray_transfer(avr_context* ctx, const avr_scene* source, const avr_scene* opacity,
                           const avr_scene* bin, const avr_scene* width, const double* start_dev,
                           const double* end_dev, uint64_t n_rays, uint64_t max_trips,
                           const int32_t* box_index_lo, const int32_t* level_ratio,
                           const double* level_cell_size, const double* prob_lo, int n_levels,
                           const double* edges, int n_channels, uint32_t* counts_dev,
                           uint8_t* status_dev, double* span_dev, double* intensity_dev,
                           double* tau_dev, double* outside_dev, double* counted_dev,
                           double* covered_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    // as avr_scene_ray_sums: the scenes first, every other rule is plan_ray_transfer's in its order
    require(source != nullptr && opacity != nullptr, "null argument");
    const size_t n_boxes = source->boxes.size();
    require_field_scene(ctx, source, n_boxes);
    for (const avr_scene* other : {opacity, bin, width}) {
      if (other != nullptr) require_field_scene(ctx, other, other->boxes.size());
    }
    const avr::RayTransferPlan plan = avr::plan_ray_transfer(
        source->boxes.data(), n_boxes, opacity->boxes.data(), opacity->boxes.size(),
        bin != nullptr ? bin->boxes.data() : nullptr, bin != nullptr ? bin->boxes.size() : 0,
        width != nullptr ? width->boxes.data() : nullptr,
        width != nullptr ? width->boxes.size() : 0, n_rays, max_trips, box_index_lo, level_ratio,
        level_cell_size, prob_lo, n_levels, edges, n_channels, ctx->ray_transfer_chunk, start_dev,
        end_dev, counts_dev, status_dev, span_dev, intensity_dev, tau_dev, outside_dev,
        counted_dev, covered_dev);
    if (n_rays == 0) return AVR_OK;
    avr::RayArgs args = plan.walk.args;
    stage_tables(ctx, plan, &args);
    args.start = start_dev;
    args.end = end_dev;
    args.counts = counts_dev;
    args.status = status_dev;
    args.span = span_dev;
    args.counted = counted_dev;
    args.covered = covered_dev;
    args.transfer.intensity = intensity_dev;
    args.transfer.tau = tau_dev;
    args.transfer.outside = outside_dev;
    return avr::launch_ray_transfer(args, plan.form, plan.n_chunks, plan.lds_bytes, ctx->stream);
  });
}

int avr_fft_twiddles(int n, double* table) {
  return guarded([&]() -> int {
    require(table != nullptr, "null argument");
    require(n >= 2 && avr::fft_length_ok(n), "n must be a power of two in [2, 1024]");
    const std::vector<double> made = avr::fft_twiddles(n);
    std::copy(made.begin(), made.end(), table);
    return AVR_OK;
  });
}

int avr_field_fft(avr_context* ctx, const double* values_dev, const int32_t* dims,
                  double* spectrum_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(values_dev != nullptr && dims != nullptr && spectrum_dev != nullptr, "null argument");
    const avr::Fft3dPlan plan = avr::plan_fft3d(dims, values_dev, spectrum_dev);
    avr::FftArgs args = plan.args;
    stage_tables(ctx, plan, &args.lines);
    args.values = values_dev;
    args.spectrum = spectrum_dev;
    return avr::launch_fft3d(args, ctx->stream);
  });
}

int avr_spectrum_bins(avr_context* ctx, const double* spectrum_dev, const int32_t* dims,
                      const double* inverse_length_sq, const double* edges_sq, int n_bins,
                      uint64_t* modes_dev, double* power_dev, uint64_t* totals_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(spectrum_dev != nullptr && dims != nullptr && inverse_length_sq != nullptr &&
                edges_sq != nullptr && modes_dev != nullptr && power_dev != nullptr &&
                totals_dev != nullptr, "null argument");
    const avr::SpectrumBinsPlan plan = avr::plan_spectrum_bins(
        dims, inverse_length_sq, edges_sq, n_bins, spectrum_dev, modes_dev, power_dev, totals_dev);
    avr::SpectrumBinsArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    args.spectrum = spectrum_dev;
    args.modes = reinterpret_cast<unsigned long long*>(modes_dev);
    args.power = power_dev;
    args.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    return avr::launch_spectrum_bins(args, plan.groups, ctx->stream);
  });
}

int avr_field_ifft(avr_context* ctx, double* spectrum_dev, const int32_t* dims, double* values_dev,
                   double* imag_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(spectrum_dev != nullptr && dims != nullptr && values_dev != nullptr, "null argument");
    const avr::Ifft3dPlan plan = avr::plan_ifft3d(dims, spectrum_dev, values_dev, imag_dev);
    avr::IfftArgs args = plan.args;
    stage_tables(ctx, plan, &args.lines);
    args.spectrum = spectrum_dev;
    args.values = values_dev;
    args.imag = imag_dev;
    return avr::launch_ifft3d(args, ctx->stream);
  });
}

int avr_spectrum_helmholtz(avr_context* ctx, double* const spectra_dev[3], const int32_t* dims,
                           const double inverse_length[3], double* const compressive_dev[3]) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(spectra_dev != nullptr && dims != nullptr && inverse_length != nullptr &&
                compressive_dev != nullptr, "null argument");
    const avr::SpectrumHelmholtzPlan plan =
        avr::plan_spectrum_helmholtz(dims, inverse_length, spectra_dev, compressive_dev);
    avr::HelmholtzArgs args = plan.args;
    for (int d = 0; d < 3; ++d) {
      args.spectra[d] = spectra_dev[d];
      args.compressive[d] = compressive_dev[d];
    }
    return avr::launch_spectrum_helmholtz(args, plan.groups, ctx->stream);
  });
}

int avr_spectrum_inverse_laplacian(avr_context* ctx, double* spectrum_dev, const int32_t* dims,
                                   const double* inverse_length_sq, double scale) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(spectrum_dev != nullptr && dims != nullptr && inverse_length_sq != nullptr,
            "null argument");
    const avr::InverseLaplacianPlan plan =
        avr::plan_spectrum_inverse_laplacian(dims, inverse_length_sq, scale);
    avr::InverseLaplacianArgs args = plan.args;
    args.spectrum = spectrum_dev;
    return avr::launch_spectrum_inverse_laplacian(args, plan.groups, ctx->stream);
  });
}

int avr_isolated_green(avr_context* ctx, const int32_t* padded_dims, const double* cell_size,
                       double scale, double self_value, double* green_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(padded_dims != nullptr && cell_size != nullptr && green_dev != nullptr,
            "null argument");
    const avr::IsolatedGreenPlan plan =
        avr::plan_isolated_green(padded_dims, cell_size, scale, self_value, green_dev);
    avr::IsolatedGreenArgs args = plan.args;
    args.green = green_dev;
    return avr::launch_isolated_green(args, plan.groups, ctx->stream);
  });
}

int avr_spectrum_multiply(avr_context* ctx, double* a_dev, const double* b_dev,
                          const int32_t* dims) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(a_dev != nullptr && b_dev != nullptr && dims != nullptr, "null argument");
    const avr::SpectrumMultiplyPlan plan = avr::plan_spectrum_multiply(dims, a_dev, b_dev);
    avr::SpectrumMultiplyArgs args = plan.args;
    args.a = a_dev;
    args.b = b_dev;
    return avr::launch_spectrum_multiply(args, plan.groups, ctx->stream);
  });
}

int avr_grid_structure_functions(avr_context* ctx, const double* const* components_dev,
                                 int n_components, const int32_t* dims, const int32_t* lags,
                                 const double* directions, int n_lags, int max_order,
                                 int periodic, uint64_t* pairs_dev, double* sums_dev,
                                 uint64_t* totals_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(components_dev != nullptr && dims != nullptr && lags != nullptr &&
                pairs_dev != nullptr && sums_dev != nullptr && totals_dev != nullptr,
            "null argument");
    const avr::StructureFunctionsPlan plan = avr::plan_structure_functions(
        components_dev, n_components, dims, lags, directions, n_lags, max_order, periodic,
        pairs_dev, sums_dev, totals_dev);
    avr::StructureArgs args = plan.args;
    stage_tables(ctx, plan, &args);
    for (int c = 0; c < n_components; ++c) args.components[c] = components_dev[c];
    args.pairs = reinterpret_cast<unsigned long long*>(pairs_dev);
    args.sums = sums_dev;
    args.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    return avr::launch_structure_functions(args, n_components, plan.groups, ctx->stream);
  });
}

int avr_context_set_velocity_cube_scratch_entries(avr_context* ctx, uint64_t entries) {
  return guarded([&]() -> int {
    require(ctx != nullptr, "null argument");
    require(entries <= avr::kCubeScratchEntries, "the scratch bound is at most 2^27 entries");
    ctx->cube_scratch_entries = entries == 0 ? avr::kCubeScratchEntries : entries;
    return AVR_OK;
  });
}

int avr_scene_velocity_cube(avr_context* ctx, const avr_scene* scene_e, const avr_scene* scene_g,
                            const avr_scene* scene_s, int axis, const double origin_uv[2],
                            double du, double dv, int width, int height, const double* level_dl,
                            int n_levels, const double* edges, int n_channels, double* cube_dev,
                            double* under_dev, double* over_dev, double* length_dev) {
  return guarded([&]() -> int {
    bind_device(ctx);
    require(scene_e != nullptr && scene_g != nullptr && origin_uv != nullptr &&
                level_dl != nullptr && edges != nullptr && cube_dev != nullptr &&
                under_dev != nullptr && over_dev != nullptr && length_dev != nullptr,
            "null argument");
    const bool broadened = scene_s != nullptr;
    const size_t n_boxes = scene_e->boxes.size();
    require_field_scene(ctx, scene_e, n_boxes);
    require_field_scene(ctx, scene_g, n_boxes);
    if (broadened) require_field_scene(ctx, scene_s, n_boxes);
    const avr::VelocityCubePlan plan = avr::plan_velocity_cube(
        scene_e->boxes.data(), scene_g->boxes.data(),
        broadened ? scene_s->boxes.data() : nullptr, n_boxes, axis, origin_uv, du, dv, width,
        height, level_dl, n_levels, edges, n_channels, cube_dev, under_dev, over_dev, length_dev,
        ctx->cube_scratch_entries);
    ctx->cube_planes.reserve(plan.scratch.total, ctx->stream, "avr_scene_velocity_cube",
                             "hipMalloc(cube planes)");
    avr::CubeReduceArgs reduce = plan.reduce;
    avr::CubeGatherArgs gather = plan.gather;
    stage_tables(ctx, plan, &reduce, &gather);
    reduce.planes = scratch_part<double>(ctx->cube_planes, plan.scratch.planes);
    reduce.under = scratch_part<double>(ctx->cube_planes, plan.scratch.under);
    reduce.over = scratch_part<double>(ctx->cube_planes, plan.scratch.over);
    reduce.plane_n = scratch_part<uint32_t>(ctx->cube_planes, plan.scratch.n);
    gather.planes = reduce.planes;
    gather.plane_under = reduce.under;
    gather.plane_over = reduce.over;
    gather.plane_n = reduce.plane_n;
    gather.cube = cube_dev;
    gather.under = under_dev;
    gather.over = over_dev;
    gather.length = length_dev;
    // one batch's gather has read the planes before the next batch's reduce overwrites them: both
    // run on the context's stream
    for (int32_t batch = 0; batch < plan.n_batches; ++batch) {
      plan.set_batch(batch, &reduce, &gather);
      int status = avr::launch_cube_reduce(reduce, axis, broadened, ctx->stream);
      if (status != AVR_OK) return status;
      status = avr::launch_cube_gather(gather, ctx->stream);
      if (status != AVR_OK) return status;
    }
    return AVR_OK;
  });
}

}  // extern "C"
