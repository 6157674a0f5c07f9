"""Public entry points with the reference's option surface.

  api::Render(AmrData, RenderOptions)    VolumeRenderer/VolumeRendererApi.hpp:22-54
  python render(plotfile, **kwargs)      python/amrVolumeRenderer/module.cpp:264-303

Both entries run end to end: `render` / `run` read an AMReX plotfile without AMReX
(plotfile.py: Header, Cell_H, FAB files; our own convexify -- see DESIGN.md 6e for the one known
divergence from amrex::convexify's box list), build the scene statistics and the scalar transform
with the HIP scan kernels, and hand the fields of VolumeRenderer::SceneGeometry
(VolumeRenderer/VolumeRenderer.hpp:74-89) to `render_scene`; `render_amr_data` is api::Render
over plain per-level box lists and cell arrays (an amrex::MultiFab cannot be taken without AMReX).
Arguments are validated exactly as the reference does.
"""
from __future__ import annotations

import contextlib
import math
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

from .derive import (DerivedProgram, add_field, compile_expression, derived_fields,
                     evaluate_program, remove_field)
from .clumps import add_clump_field, clump_fields, remove_clump_field, threshold_ladder
from .gradient import add_gradient_field, gradient_fields, remove_gradient_field
from .gridfields import (add_array_field, add_helmholtz_field, add_potential_field, grid_fields,
                         remove_grid_field)
from .particles import add_particle_field, particle_fields, remove_particle_field
from .groups import linking_length
from .types import AmrBox, CameraParameters, ColorMapControlPoint, ScalarTransform, VolumeBounds


@dataclass
class RenderOptions:
    """api::RenderOptions (VolumeRenderer/VolumeRendererApi.hpp:28-44)."""
    width: int = 512
    height: int = 512
    box_transparency: float = 0.0
    antialiasing: int = 1
    visibility_graph: bool = True
    write_visibility_graph: bool = False
    min_level: int = 0
    max_level: int = -1
    log_scale_input: bool = False
    component: int = 0
    output_filename: str = "volume-renderer.ppm"
    up_vector: Optional[Tuple[float, float, float]] = None
    scalar_range: Optional[Tuple[float, float]] = None
    camera: Optional[CameraParameters] = None
    color_map: Optional[List[ColorMapControlPoint]] = None
    # "volume" (the reference's image) or "max_intensity": per pixel the colour-map entry of the
    # largest value along the ray (FrameRenderer.render_max_intensity; antialiasing must be 1)
    mode: str = "volume"


RENDER_MODES = ("volume", "max_intensity")


@dataclass
class SceneGeometry:
    """VolumeRenderer::SceneGeometry (VolumeRenderer/VolumeRenderer.hpp:74-89), hot-path fields."""
    all_boxes: List[AmrBox]            # metadata of every box (replicated), .owner set
    local_boxes: List[AmrBox]          # this rank's boxes, cell data in HBM
    scalar_transform: ScalarTransform
    bounds: VolumeBounds
    scalar_range: Tuple[float, float] = (0.0, 1.0)
    processed_scalar_range: Optional[Tuple[float, float]] = None   # after log scaling, if any
    # scene units per physical unit: plotfiles are rescaled so that their shortest edge is 1
    world_scale: float = 1.0


@dataclass
class AmrData:
    """api::AmrData (VolumeRenderer/VolumeRendererApi.hpp:22-26) without AMReX objects: per level
    the grids' index boxes and cell arrays instead of a MultiFab, the problem's lower corner and
    cell sizes instead of an amrex::Geometry.
    level_boxes[l] = [((ilo, jlo, klo), (ihi, jhi, khi)), ...]   inclusive, cell-centred
    level_data[l][g] = float64 array [nz, ny, nx] or [ncomp, nz, ny, nx] (numpy or torch)"""
    level_boxes: List[list]
    level_data: List[list]
    prob_lo: Tuple[float, float, float]
    cell_sizes: List[Tuple[float, float, float]]
    refinement_ratios: List[int]


def load_amr_data_geometry(ctx, data: AmrData, requested_min_level: int = 0,
                           requested_max_level: int = -1, component: int = 0,
                           log_scale_input: bool = False, normalize_to_data_range: bool = True,
                           rank: int = 0, n_ranks: int = 1, process_group=None) -> "SceneGeometry":
    """loadMultiFabGeometry (VolumeRendererApi.cpp:44-131)."""
    from . import plotfile as pf
    if not data.level_boxes or len(data.level_boxes) != len(data.level_data) or \
            len(data.cell_sizes) != len(data.level_boxes):
        raise ValueError("levelData and levelGeometry must be non-empty and of matching sizes")
    finest = len(data.level_boxes) - 1
    min_level, max_level = pf.clamp_levels(requested_min_level, requested_max_level, finest)
    if min_level > max_level:
        raise RuntimeError("minLevel must not exceed maxLevel")
    if max_level > 0 and len(data.refinement_ratios) < max_level:
        raise ValueError("refinementRatios must provide ratios for each level transition")
    if component < 0:
        raise ValueError("component index out of range")

    def fetch(level, grid_ids):
        out = {}
        for g in grid_ids:
            cells = data.level_data[level][g]
            if cells is None:
                raise ValueError("levelData contains a null MultiFab pointer")
            if cells.ndim == 4:
                if component >= cells.shape[0]:
                    raise ValueError("component index out of range")
                cells = cells[component]
            elif component != 0:
                raise ValueError("component index out of range")
            out[g] = cells
        return out

    return pf.build_scene_from_levels(
        ctx, [list(b) for b in data.level_boxes], data.cell_sizes, data.prob_lo,
        data.refinement_ratios, fetch, min_level, max_level, log_scale_input,
        normalize_to_data_range, rank, n_ranks, process_group,
        "Failed to locate any volumetric data in the provided MultiFabs.")


def build_scene_geometry(ctx, all_boxes: Sequence[AmrBox], local_boxes: Sequence[AmrBox],
                         bounds: VolumeBounds, log_scale_input: bool = False,
                         normalize_to_data_range: bool = True, process_group=None,
                         n_ranks: int = 1) -> "SceneGeometry":
    """The scalar part of detail::BuildSceneGeometry (VolumeRenderer/SceneBuilder.cpp:315-443):
    one streaming pass over the local cells (min, max, min positive, finite count), the
    MIN / MAX / SUM reductions over ranks (:327-344, :368-385) and the scalar transform.
    The geometric part (world corners, global rescale, padded bounds) needs amrex::Geometry and
    is plotfile.load_plotfile_geometry's: boxes arrive here with their corners."""
    import torch
    import torch.distributed as dist
    from . import runtime
    scene = ctx.create_scene(local_boxes, ScalarTransform())
    lo, hi, lo_pos, finite = scene.scalar_stats()
    if n_ranks > 1:
        device = ctx.device if dist.get_backend(process_group) == "nccl" else "cpu"
        mins = torch.tensor([lo, lo_pos], dtype=torch.float64, device=device)
        maxs = torch.tensor([hi], dtype=torch.float64, device=device)
        count = torch.tensor([finite], dtype=torch.int64, device=device)
        dist.all_reduce(mins, op=dist.ReduceOp.MIN, group=process_group)
        dist.all_reduce(maxs, op=dist.ReduceOp.MAX, group=process_group)
        dist.all_reduce(count, op=dist.ReduceOp.SUM, group=process_group)
        lo, lo_pos, hi, finite = mins[0].item(), mins[1].item(), maxs[0].item(), int(count.item())
    transform, processed_range, scalar_range = runtime.scene_transform_from_stats(
        (lo, hi, lo_pos), finite, log_scale_input, normalize_to_data_range)
    return SceneGeometry(list(all_boxes), list(local_boxes), transform, bounds, scalar_range,
                         processed_range)


# ---- what the products below share ---------------------------------------------------------------

def _require_plotfile(plotfile: str) -> None:
    if not plotfile:
        raise RuntimeError("plotfile path is required")
    if not os.path.exists(plotfile):
        raise RuntimeError(f"plotfile path '{plotfile}' does not exist")


def _header_levels(header, n_levels: int):
    """(cell_size, prob_lo, ref_ratio) of a plotfile's first n_levels levels, as the *_scene
    functions take them."""
    return header.cell_size[:n_levels], header.prob_lo, header.ref_ratio[:n_levels - 1]


def _checked_cell_sizes(scene: "SceneGeometry", cell_sizes) -> List[Tuple[float, ...]]:
    """cell_sizes as float triples: one per level up to the scene's finest at least, 16 at most."""
    sizes = [tuple(float(v) for v in c) for c in cell_sizes]
    finest = max((int(b.level) for b in scene.all_boxes), default=0)
    if not (finest < len(sizes) <= 16) or any(len(c) != 3 for c in sizes):
        raise ValueError("cell_sizes must hold (dx, dy, dz) per level up to the finest loaded one "
                         "(at most 16)")
    return sizes


def _require_one_rank(scene: "SceneGeometry", n_ranks: int, message: str) -> None:
    if n_ranks > 1 or len(scene.local_boxes) != len(scene.all_boxes):
        raise NotImplementedError(message)


@contextlib.contextmanager
def _native_scenes(ctx, geometries):
    """The runtime.Scene of every entry's local boxes (None stays None), in order; all of them
    are closed on the way out, also those made before a later one failed."""
    made = []
    try:
        for geometry in geometries:
            made.append(None if geometry is None else
                        ctx.create_scene(geometry.local_boxes, geometry.scalar_transform))
        yield made
    finally:
        for scene in made:
            if scene is not None:
                scene.close()


def _blank_like(ctx, geometry: "SceneGeometry", rank: int) -> "SceneGeometry":
    """geometry's boxes with new cells for a kernel to write (_allocate_like), no transform."""
    return SceneGeometry(geometry.all_boxes, _allocate_like(ctx, geometry.local_boxes, rank),
                         ScalarTransform(), geometry.bounds, world_scale=geometry.world_scale)


def _computed_scene(ctx, written: "SceneGeometry", log_scale_input: bool,
                    normalize_to_data_range: bool, process_group, n_ranks: int) -> "SceneGeometry":
    """The scene of cells a kernel has written into _blank_like's boxes: statistics and the
    scalar transform from build_scene_geometry, the world scale of the scene they came from."""
    result = build_scene_geometry(ctx, written.all_boxes, written.local_boxes, written.bounds,
                                  log_scale_input, normalize_to_data_range, process_group, n_ranks)
    result.world_scale = written.world_scale
    return result


def _sum_over_ranks(ctx, tensors, process_group, root: Optional[int] = None) -> list:
    """Every tensor (None stays None) summed over the group's ranks, through the host if the
    group's backend is not NCCL -- the results are then host tensors.  Without root every rank
    gets the sums (all-reduce); with it only that global rank does (reduce)."""
    import torch.distributed as dist
    stage = dist.get_backend(process_group) != "nccl"
    ctx.synchronize()
    summed = []
    for t in tensors:
        if t is not None:
            t = t.cpu() if stage else t
            if root is None:
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=process_group)
            else:
                dist.reduce(t, root, op=dist.ReduceOp.SUM, group=process_group)
        summed.append(t)
    return summed


def _copied(a):
    return a.copy() if hasattr(a, "copy") else a.clone()


def _write_picture(rgb8, output: str) -> None:
    """rgb8 [height, width, 3] on the device -> `output`: a PNG for .png, else a PPM."""
    writer = save_png if os.path.splitext(output)[1].lower() == ".png" else save_ppm
    if not writer(rgb8.cpu().numpy(), output):
        raise RuntimeError(f"could not write '{output}'")


# ---- derived fields ("Derived fields") ----------------------------------------------

def _allocate_like(ctx, local: Sequence[AmrBox], rank: int) -> List[AmrBox]:
    """New cells for the boxes `local`: one device allocation, every box its own contiguous
    [nz, ny, nx] block on a 16-byte boundary."""
    import torch
    offsets, total = [], 0
    for b in local:
        nx, ny, nz = b.cell_dimensions
        offsets.append(total)
        total += (nx * ny * nz + 1) // 2 * 2        # every block starts on a 16-byte boundary
    cells = torch.empty(total, dtype=torch.float64, device=ctx.device)
    out_boxes = []
    for b, begin in zip(local, offsets):
        nx, ny, nz = b.cell_dimensions
        out_boxes.append(AmrBox(b.min_corner, b.max_corner,
                                cells[begin:begin + nx * ny * nz].view(nz, ny, nx), b.level,
                                owner=rank))
    return out_boxes


def derive_scene(ctx, program: DerivedProgram, scenes: Sequence["SceneGeometry"],
                 geometry: "SceneGeometry", cell_sizes, rank: int = 0, n_ranks: int = 1,
                 process_group=None, log_scale_input: bool = False,
                 normalize_to_data_range: bool = True) -> "SceneGeometry":
    """The derived field of a compiled program as a scene ("Derived fields"): scenes
    are the loaded scenes of program.fields, in that order, and geometry any loaded scene of the
    same plotfile, levels, rank and world size (it supplies all_boxes, bounds and world_scale, so
    that a program without fields still has boxes).  cell_sizes[l] = (dx, dy, dz) of level l in the
    plotfile's physical units, one entry per level up to the finest loaded one.  One kernel writes
    program(cell) for every cell of every local box into one new device allocation, every box its
    own contiguous [nz, ny, nx] block on a 16-byte boundary; statistics, their reduction over ranks
    and the scalar transform come from build_scene_geometry, to which log_scale_input and
    normalize_to_data_range go as load_plotfile_geometry's do (the defaults are a loaded scene's).
    The result is accepted wherever a loaded scene is."""
    scenes = list(scenes)
    if len(scenes) != len(program.fields):
        raise ValueError("scenes must hold one loaded scene per field of the program")
    local = list(geometry.local_boxes)
    for scene in scenes:
        if len(scene.local_boxes) != len(local):
            raise ValueError("the scenes must hold the same boxes as geometry")
    sizes = _checked_cell_sizes(geometry, cell_sizes)
    written = _blank_like(ctx, geometry, rank)
    to_physical = float(geometry.world_scale)
    origin = [[float(b.min_corner[a]) / to_physical for a in range(3)] for b in local]
    with _native_scenes(ctx, scenes + [written]) as (*inputs, out):
        import numpy as np
        out.derive(inputs, program.instructions, program.constants,
                   np.array(origin, dtype=np.float64).reshape(len(local), 3), sizes)
    return _computed_scene(ctx, written, log_scale_input, normalize_to_data_range, process_group,
                           n_ranks)


# ---- the level setup of the products that cross levels -------------------------------------------

def _level_setup(scene: "SceneGeometry", local, cell_sizes, prob_lo, ref_ratio):
    """(sizes, ratios, box_index_lo) as the native calls of the gradient fields, clumps,
    isosurfaces and streamlines take them: cell_sizes as float triples per level up to the finest
    loaded one, one ref_ratio per level transition, and the index of every local box's first cell
    recovered from its corner (gradient.box_index_lo)."""
    from . import gradient
    sizes = _checked_cell_sizes(scene, cell_sizes)
    ratios = [int(r) for r in ref_ratio][:len(sizes) - 1]
    if len(ratios) != len(sizes) - 1:
        raise ValueError("ref_ratio must hold one ratio per level transition")
    index = gradient.box_index_lo([b.min_corner for b in local], [b.level for b in local],
                                  scene.world_scale, prob_lo, sizes)
    return sizes, ratios, index


# ---- gradient fields ("Gradient fields") --------------------------------------------

def gradient_scene(ctx, scene: "SceneGeometry", axis: int, cell_sizes, prob_lo, ref_ratio,
                   rank: int = 0, n_ranks: int = 1, process_group=None,
                   log_scale_input: bool = False,
                   normalize_to_data_range: bool = True) -> "SceneGeometry":
    """The difference of a scene's field along axis (0 = x, 1 = y, 2 = z) as a scene (DESIGN.md 7,
    "Gradient fields"): central where a cell has both neighbours, one-sided where it has one, 0.0
    where it has none; past a box's face the neighbour is the cell of the same or a coarser level
    that holds it, or the mean of its children one level finer.  scene is a loaded (or derived)
    scene of a plotfile whose header gives cell_sizes[l] = (dx, dy, dz) per level up to the finest
    loaded one, prob_lo and ref_ratio; the boxes' integer indices are recovered from their corners
    (ValueError if one is not an integer to 1e-6).  The output is allocated as derive_scene's is,
    and statistics and the scalar transform come from build_scene_geometry with the caller's flags.
    Every box of the scene must be on this rank: with n_ranks > 1, or fewer local boxes than
    boxes, NotImplementedError is raised before any device work."""
    axis = int(axis)
    if axis not in (0, 1, 2):
        raise ValueError("axis must be 0 (x), 1 (y) or 2 (z)")
    _require_one_rank(scene, n_ranks, "a gradient field needs every box of the scene on one rank: "
                      "ghost cells are not exchanged between ranks")
    sizes, ratios, index = _level_setup(scene, scene.local_boxes, cell_sizes, prob_lo, ref_ratio)
    written = _blank_like(ctx, scene, rank)
    with _native_scenes(ctx, [scene, written]) as (field, out):
        out.gradient(field, axis, index, ratios, [c[axis] for c in sizes])
    return _computed_scene(ctx, written, log_scale_input, normalize_to_data_range, process_group,
                           n_ranks)


# ---- clumps ("Clumps") ---------------------------------------------------------------

def clump_scene(ctx, scene: "SceneGeometry", lower: float, upper: float, cell_sizes, prob_lo,
                ref_ratio, rank: int = 0, n_ranks: int = 1, process_group=None,
                log_scale_input: bool = False, normalize_to_data_range: bool = True):
    """The clumps of a scene's field as a label scene ("Clumps"): the connected
    components of the cells whose raw value v satisfies lower <= v <= upper (either bound may be
    infinite; a NaN is never selected), adjacent through the six faces inside a box and, past a
    box's face, through the cell of the same or a coarser level that holds the ghost.  Returns
    (SceneGeometry, n_clumps): the scene holds f64(label) in 1..n_clumps for a selected cell,
    numbered in ascending order of each clump's smallest cell ordinal (scene order of the boxes,
    then k, j, i), and 0.0 otherwise.  scene, cell_sizes, prob_lo and ref_ratio as gradient_scene
    takes them; the output is allocated as derive_scene's is, and statistics and the scalar
    transform come from build_scene_geometry with the caller's flags.  Every box of the scene must
    be on this rank: with n_ranks > 1, or fewer local boxes than boxes, NotImplementedError is
    raised before any device work."""
    from . import clumps as clump_rules
    lower, upper = clump_rules.check_bounds(lower, upper)
    _require_one_rank(scene, n_ranks, "clumps need every box of the scene on one rank: "
                      "labels are not merged between ranks")
    sizes, ratios, index = _level_setup(scene, scene.local_boxes, cell_sizes, prob_lo, ref_ratio)
    written = _blank_like(ctx, scene, rank)
    with _native_scenes(ctx, [scene, written]) as (field, out):
        count = out.clumps(field, lower, upper, index, ratios)
        ctx.synchronize()
        n_clumps = int(count.item())
    return _computed_scene(ctx, written, log_scale_input, normalize_to_data_range, process_group,
                           n_ranks), n_clumps


def clumps(plotfile: str, variable: str, lower: float = -math.inf, upper: float = math.inf,
           fields: Sequence[str] = (), min_level: int = 0, max_level: int = -1,
           mass: Optional[str] = None, velocity: Optional[Sequence[str]] = None,
           thermal: Optional[str] = None, G: float = 6.6743e-8, max_cells: int = 2 ** 18) -> dict:
    """The clumps of a plotfile's variable ("Clumps"), on cuda:0: the connected
    components of the uncovered cells of the loaded levels whose raw value lies in [lower, upper],
    with their sizes.  variable and every name of fields is a stored variable or a registered
    derived, gradient, clump or grid field.  Returns a dict: n (the number of clumps, numbered 1..n by
    smallest cell ordinal; entry c - 1 of every array belongs to clump c), cells_by_level int64
    [L, n], cells int64 [n], volume float64 [n] = sum_l vol[l] * f64(cells[l]) (level ascending
    from +0.0), integrals {name: float64 [n]} = sum_l vol[l] * sums[l], the volume integral of
    each requested field over each clump, taken over the cells where that field is finite,
    outside (labels that are no clump's; 0) and nonfinite (cells of clumps where a requested
    field is not finite, over all fields).  n == 0 gives empty arrays.  With mass (the name of a
    mass density; velocity: three names, thermal: a thermal energy density, both optional) every
    clump of 2 to max_cells cells is also tested for gravitational binding with the constant G
    (cgs by default), and the dict gains mass, self_energy, kinetic, thermal, bound, evaluated
    and excluded as clump_binding_scene makes them; the members whose thermal energy is not
    finite are added to nonfinite.  Without mass nothing of that is loaded or run."""
    import numpy as np
    from . import clumps as clump_rules
    from . import plotfile as pf
    lower, upper = clump_rules.check_bounds(lower, upper)
    names = [str(name) for name in fields]
    binding_names = _binding_names(mass, velocity, thermal)
    if mass is not None:
        clump_rules.check_max_cells(max_cells)
    ctx, rank, world, group, scenes, volumes = _load_fields(
        plotfile, [variable] + names + binding_names, min_level, max_level)
    header = pf.PlotFileData(plotfile)
    n_levels = len(volumes)
    labels, n = clump_scene(ctx, scenes[0], lower, upper, *_header_levels(header, n_levels), rank,
                            world, group)
    cells_by_level = np.zeros((n_levels, n), dtype=np.int64)
    sums = {name: np.zeros((n_levels, n), dtype=np.float64) for name in names}
    outside = nonfinite = 0
    if n > 0:
        if n * n_levels >= clump_rules.TABLE_MAX_ENTRIES:
            raise ValueError("too many clumps for one table: n * levels must stay below 2^28")
        with _native_scenes(ctx, [labels]) as (label_scene,):
            counted, _, totals = label_scene.clump_table(n, n_levels)
            ctx.synchronize()
            cells_by_level = counted.cpu().numpy()
            outside = int(totals[0].item())
            for name, scene in zip(names, scenes[1:]):
                with _native_scenes(ctx, [scene]) as (field,):
                    _, summed, totals = label_scene.clump_table(n, n_levels, field)
                    ctx.synchronize()
                sums[name] = summed.cpu().numpy()
                nonfinite += int(totals[1].item())
    found = {"n": n, "cells_by_level": cells_by_level, "cells": cells_by_level.sum(axis=0),
             "volume": clump_rules.clump_volumes(cells_by_level, volumes),
             "integrals": {name: clump_rules.clump_integrals(sums[name], volumes)
                           for name in names},
             "outside": outside, "nonfinite": nonfinite}
    if mass is not None:
        binding = clump_binding_scene(
            ctx, labels, n, found["cells"],
            *_binding_scenes(scenes, 1 + len(names), mass, velocity, thermal),
            *_header_levels(header, n_levels), G=G, max_cells=max_cells, n_ranks=world)
        found["nonfinite"] += binding.pop("nonfinite")
        found.update(binding)
    return found


# ---- clump binding ("Clump binding") --------------------------------------------------

def _clump_member_lists(ctx, label_scene, n: int, wanted, offsets, index, ratios, sizes, prob_lo,
                        fields):
    """The sorted member keys of the wanted clumps of a native label scene, with the members'
    levels, centres [3, m] and the raw value of every native scene of `fields`, all on the
    device.  RuntimeError if a cell carries a label that is no clump in 1..n."""
    keys, totals = label_scene.clump_members(n, wanted, int(offsets[-1]))
    if int(totals[0].item()) != 0:
        raise RuntimeError(f"{int(totals[0].item())} cells carry a label that is no clump in "
                           f"1..{n}")
    levels, centres, _ = label_scene.clump_member_data(keys, index, ratios, sizes, prob_lo)
    values = [label_scene.clump_member_data(keys, index, ratios, sizes, prob_lo, field=field,
                                            centres=False)[2] for field in fields]
    return keys, levels, centres, values


def clump_members_scene(ctx, labels: "SceneGeometry", n: int, cells, cell_sizes, prob_lo,
                        ref_ratio, fields: Sequence["SceneGeometry"] = (), min_cells: int = 1,
                        max_cells: int = 2 ** 18, n_ranks: int = 1) -> dict:
    """The cells of the clumps of a label scene, clump by clump ("Clump binding").
    labels and n: what clump_scene returned; cells: the cell count per clump (the clump table's,
    summed over levels); fields: scenes of the same boxes whose value is read at every member.  A
    clump is listed if min_cells <= cells <= max_cells (clumps.member_segments).  Returns a dict
    of numpy arrays: labels int64 (the listed clumps, ascending), offsets int64 (members of
    labels[s]: offsets[s] .. offsets[s + 1] - 1), ordinal int64 [m] (the cell ordinals of
    "Clumps", ascending per clump), level uint8 [m], centres float64 [m, 3] = prob_lo + (f64(I) +
    0.5) * dx_l, values: one float64 [m] per scene of fields.  Every box of the scene must be on
    this rank, as for clump_scene."""
    import numpy as np
    from . import clumps as clump_rules
    _require_one_rank(labels, n_ranks, "clumps need every box of the scene on one rank: "
                      "labels are not merged between ranks")
    sizes, ratios, index = _level_setup(labels, labels.local_boxes, cell_sizes, prob_lo, ref_ratio)
    wanted, offsets = clump_rules.member_segments(cells, min_cells, max_cells)
    if len(wanted) != int(n):
        raise ValueError("cells must hold one count per clump")
    fields = list(fields)
    found = {"labels": np.nonzero(wanted)[0].astype(np.int64) + 1, "offsets": offsets,
             "ordinal": np.zeros(0, dtype=np.int64), "level": np.zeros(0, dtype=np.uint8),
             "centres": np.zeros((0, 3), dtype=np.float64),
             "values": [np.zeros(0, dtype=np.float64) for _ in fields]}
    if int(offsets[-1]) == 0:
        return found
    with _native_scenes(ctx, [labels] + fields) as (label_scene, *native_fields):
        keys, levels, centres, values = _clump_member_lists(
            ctx, label_scene, int(n), wanted, offsets, index, ratios, sizes, prob_lo, native_fields)
        ctx.synchronize()
        found["ordinal"] = (keys & 0xffffffff).cpu().numpy()
        found["level"] = levels.cpu().numpy()
        found["centres"] = np.ascontiguousarray(centres.cpu().numpy().T)
        found["values"] = [v.cpu().numpy() for v in values]
    return found


def clump_members(plotfile: str, variable: str, lower: float = -math.inf, upper: float = math.inf,
                  fields: Sequence[str] = (), min_cells: int = 1, max_cells: int = 2 ** 18,
                  min_level: int = 0, max_level: int = -1, output: Optional[str] = None) -> dict:
    """The cells of the clumps of a plotfile's variable over [lower, upper] (yt's clump[field]),
    on cuda:0.  variable and every name of fields as api.clumps takes them.  Returns a dict: n
    (the number of clumps), and labels, offsets, ordinal, level, centres and values {name: float64
    [m]} as clump_members_scene makes them, for the clumps of min_cells to max_cells cells.  With
    output, the arrays are also written as one .npz (the values as value_<name>)."""
    import numpy as np
    from . import clumps as clump_rules
    from . import plotfile as pf
    lower, upper = clump_rules.check_bounds(lower, upper)
    names = [str(name) for name in fields]
    ctx, rank, world, group, scenes, volumes = _load_fields(plotfile, [variable] + names,
                                                            min_level, max_level)
    header = pf.PlotFileData(plotfile)
    n_levels = len(volumes)
    levels = _header_levels(header, n_levels)
    labels, n = clump_scene(ctx, scenes[0], lower, upper, *levels, rank, world, group)
    cells = np.zeros(0, dtype=np.int64)
    if n > 0:
        if n * n_levels >= clump_rules.TABLE_MAX_ENTRIES:
            raise ValueError("too many clumps for one table: n * levels must stay below 2^28")
        with _native_scenes(ctx, [labels]) as (label_scene,):
            counted, _, _ = label_scene.clump_table(n, n_levels)
            ctx.synchronize()
            cells = counted.cpu().numpy().sum(axis=0)
    found = clump_members_scene(ctx, labels, n, cells, *levels, fields=scenes[1:],
                                min_cells=min_cells, max_cells=max_cells, n_ranks=world)
    found["values"] = dict(zip(names, found["values"]))
    found["n"] = n
    if output:
        arrays = {key: np.asarray(value) for key, value in found.items() if key != "values"}
        arrays.update({f"value_{name}": values for name, values in found["values"].items()})
        np.savez(output, **arrays)
    return found


def clump_binding_scene(ctx, labels: "SceneGeometry", n: int, cells, mass: "SceneGeometry",
                        velocity: Optional[Sequence["SceneGeometry"]],
                        thermal: Optional["SceneGeometry"], cell_sizes, prob_lo, ref_ratio,
                        G: float = 6.6743e-8, min_cells: int = 1, max_cells: int = 2 ** 18,
                        n_ranks: int = 1) -> dict:
    """yt's gravitationally_bound for the clumps of a label scene ("Clump binding").
    labels, n and cells as clump_members_scene takes them; mass: the scene of a mass density rho;
    velocity: None or three scenes; thermal: None or the scene of a thermal energy density e.  A
    clump of max(min_cells, 2) to max_cells cells (at most 2^22) is evaluated: m = rho * vol_l per
    member (0, and counted in excluded, where rho is negative or not finite), M = sum m, W =
    sum_{i<j} m_i m_j / r_ij between the cell centres (Context.clump_pair_energy), vbar = sum m v
    / M, K = 0.5 sum m |v - vbar|^2 (0 without velocities or with M == 0; the velocity of a member
    with m == 0 is not looked at: it may be a NaN), T = sum e * vol_l over
    the members whose e is finite (the others counted in nonfinite); bound = G * W > K + T.  Any
    other clump has evaluated False, NaNs and bound True.  Returns a dict of numpy arrays per
    clump: mass, self_energy (= G * W), kinetic, thermal float64 [n], bound, evaluated bool [n],
    excluded int64 [n], and nonfinite (int)."""
    import numpy as np
    import torch
    from . import clumps as clump_rules
    _require_one_rank(labels, n_ranks, "clumps need every box of the scene on one rank: "
                      "labels are not merged between ranks")
    n = int(n)
    if velocity is not None and len(velocity) != 3:
        raise ValueError("velocity holds three scenes or is None")
    G = float(G)
    if not (math.isfinite(G) and G > 0.0):
        raise ValueError("G must be finite and positive")
    sizes, ratios, index = _level_setup(labels, labels.local_boxes, cell_sizes, prob_lo, ref_ratio)
    wanted, offsets = clump_rules.binding_segments(cells, min_cells, max_cells)
    if len(wanted) != n:
        raise ValueError("cells must hold one count per clump")
    nan = np.full(n, np.nan, dtype=np.float64)
    found = {"mass": nan.copy(), "self_energy": nan.copy(), "kinetic": nan.copy(),
             "thermal": nan.copy(), "bound": np.ones(n, dtype=bool), "evaluated": wanted.copy(),
             "excluded": np.zeros(n, dtype=np.int64), "nonfinite": 0}
    n_segments = int(wanted.sum())
    if n_segments == 0:
        return found
    fields = [mass] + (list(velocity) if velocity is not None else []) + \
        ([thermal] if thermal is not None else [])
    with _native_scenes(ctx, [labels] + fields) as (label_scene, *native_fields):
        _, levels, centres, values = _clump_member_lists(
            ctx, label_scene, n, wanted, offsets, index, ratios, sizes, prob_lo, native_fields)
        device = ctx.device
        volume = torch.tensor(level_cell_volumes(sizes), dtype=torch.float64,
                              device=device)[levels.long()]
        counts = torch.from_numpy(np.diff(offsets)).to(device)
        segment = torch.repeat_interleave(torch.arange(n_segments, device=device), counts)

        def per_segment(terms):
            return torch.zeros(n_segments, dtype=torch.float64,
                               device=device).index_add_(0, segment, terms)

        rho = values[0]
        usable = torch.isfinite(rho) & (rho >= 0.0)
        m = torch.where(usable, rho * volume, torch.zeros_like(rho))
        excluded = torch.zeros(n_segments, dtype=torch.int64,
                               device=device).index_add_(0, segment, (~usable).to(torch.int64))
        W, _ = ctx.clump_pair_energy(offsets, centres[0].contiguous(), centres[1].contiguous(),
                                     centres[2].contiguous(), m)
        M = per_segment(m)
        K = torch.zeros_like(M)
        if velocity is not None:
            heavy = M > 0.0
            safe = torch.where(heavy, M, torch.ones_like(M))
            for v in values[1:4]:
                # a member without mass has no velocity: whatever its cell holds, a NaN included
                v = torch.where(m > 0.0, v, torch.zeros_like(v))
                vbar = per_segment(m * v) / safe
                away = v - vbar[segment]
                K = K + per_segment(m * (away * away))
            K = torch.where(heavy, 0.5 * K, torch.zeros_like(K))
        T = torch.zeros_like(M)
        if thermal is not None:
            e = values[-1]
            known = torch.isfinite(e)
            T = per_segment(torch.where(known, e * volume, torch.zeros_like(e)))
            found["nonfinite"] = int((~known).sum().item())
        ctx.synchronize()
        W, M, K, T = (t.cpu().numpy() for t in (W, M, K, T))
        found["excluded"][wanted] = excluded.cpu().numpy()
    found["mass"][wanted] = M
    found["self_energy"][wanted] = np.float64(G) * W
    found["kinetic"][wanted] = K
    found["thermal"][wanted] = T
    found["bound"] = clump_rules.bound_mask(1.0, found["self_energy"], found["kinetic"],
                                            found["thermal"], found["evaluated"])
    return found


def _binding_scenes(scenes, n_plain: int, mass, velocity, thermal):
    """(mass scene, velocity scenes or None, thermal scene or None) from the scenes loaded behind
    the first n_plain."""
    at = n_plain
    mass_scene = scenes[at]
    at += 1
    velocity_scenes = None
    if velocity is not None:
        velocity_scenes = scenes[at:at + 3]
        at += 3
    return mass_scene, velocity_scenes, scenes[at] if thermal is not None else None


def _binding_names(mass, velocity, thermal) -> List[str]:
    """The field names a binding evaluation loads, in _binding_scenes' order; ValueError for
    velocity or thermal without mass and for a velocity that is not three names."""
    if mass is None:
        if velocity is not None or thermal is not None:
            raise ValueError("velocity and thermal need mass")
        return []
    names = [str(mass)]
    if velocity is not None:
        velocity = [str(v) for v in velocity]
        if len(velocity) != 3:
            raise ValueError("velocity holds three field names")
        names += velocity
    if thermal is not None:
        names.append(str(thermal))
    return names


# ---- clump trees ("Clump tree") ------------------------------------------------------

def clump_tree_scene(ctx, scene: "SceneGeometry", thresholds, upper, cell_sizes, prob_lo,
                     ref_ratio, tables: Sequence["SceneGeometry"] = (), rank: int = 0,
                     n_ranks: int = 1, binding: Optional[dict] = None) -> dict:
    """The clumps of a scene's field over a ladder of thresholds, linked into a tree (DESIGN.md 7,
    "Clump tree").  thresholds: 1 to 64 finite values, strictly ascending; upper: one closed upper
    bound for all of them (clumps.check_thresholds).  The clumps of thresholds[i] are clump_scene's
    over [thresholds[i], upper]; every one of them lies inside exactly one clump of thresholds[i -
    1], its parent.  One clump_scene call per threshold up to the first without a clump (no later
    one has any, and none is asked for), with at most two label scenes alive; per threshold one
    Scene.clump_links call against the labels of the threshold below, one Scene.clump_table call,
    and one more per scene of `tables` (scenes of the same boxes, summed per clump).  scene,
    cell_sizes, prob_lo and ref_ratio as clump_scene takes them; L = len(cell_sizes).  Returns a
    dict over the nodes -- ascending threshold, then label: counts (clumps per threshold, one per
    threshold), parent_labels (per threshold an int64 array, the parent's label per clump; empty
    for threshold 0), index_lo, index_hi int64 [n, 3] (the inclusive bounding box in level L - 1's
    index space), left_edge = prob_lo + f64(index_lo) * dx[L - 1], right_edge = prob_lo +
    f64(index_hi + 1) * dx[L - 1] float64 [n, 3], cells_by_level int64 [L, n], sums (per scene of
    tables float64 [L, n]) and nonfinite (cells of clumps where a summed field is not finite).
    RuntimeError, naming the threshold and the label, if a clump's cells carry two parent labels,
    if a label or parent label is none, or if a clump has no cell.  binding (None, or a dict of
    clump_binding_scene's arguments mass, velocity, thermal, G, min_cells and max_cells): every
    threshold's clumps are tested for binding while that threshold's label scene is alive, and
    the result gains binding, clump_binding_scene's arrays over the nodes, with nonfinite added
    up.  Every box of the scene must be on this rank, as for clump_scene."""
    import numpy as np
    from . import clumps as clump_rules
    thresholds, upper = clump_rules.check_thresholds(thresholds, upper)
    _require_one_rank(scene, n_ranks, "clumps need every box of the scene on one rank: "
                      "labels are not merged between ranks")
    sizes, ratios, index = _level_setup(scene, scene.local_boxes, cell_sizes, prob_lo, ref_ratio)
    n_levels = len(sizes)
    tables = list(tables)
    counts = [0] * len(thresholds)
    parent_labels = [np.zeros(0, dtype=np.int64) for _ in thresholds]
    extents, cells, nonfinite = [], [], 0
    bindings = []
    sums = [[] for _ in tables]
    below, n_below = None, 0
    with _native_scenes(ctx, tables) as fields:
        for step, threshold in enumerate(thresholds):
            labels, n = clump_scene(ctx, scene, threshold, upper, cell_sizes, prob_lo, ref_ratio,
                                    rank, n_ranks)
            if n == 0:
                break
            if n * n_levels >= clump_rules.TABLE_MAX_ENTRIES:
                raise ValueError("too many clumps for one table: n * levels must stay below 2^28")
            with _native_scenes(ctx, [labels, below]) as (label_scene, parent_scene):
                extent, parent_lo, parent_hi, link_totals = label_scene.clump_links(
                    n, index, ratios, parent_scene, n_below)
                counted, _, totals = label_scene.clump_table(n, n_levels)
                summed = []
                for field in fields:
                    _, field_sums, field_totals = label_scene.clump_table(n, n_levels, field)
                    summed.append((field_sums, field_totals))
                ctx.synchronize()
            where = f"threshold {threshold!r}"
            if int(totals[0].item()) != 0 or int(link_totals[0].item()) != 0:
                raise RuntimeError(f"{where}: {max(int(totals[0].item()), int(link_totals[0].item()))} "
                                   f"cells carry a label that is no clump in 1..{n}")
            if int(link_totals[1].item()) != 0:
                raise RuntimeError(f"{where}: {int(link_totals[1].item())} cells of clumps in "
                                   f"1..{n} lie in no clump of the threshold below")
            extent = extent.cpu().numpy().astype(np.int64)
            untouched = np.nonzero((extent[:3] == 2 ** 31 - 1).any(axis=0) |
                                   (extent[3:] == -2 ** 31).any(axis=0))[0]
            if untouched.size:
                raise RuntimeError(f"{where}: clump {int(untouched[0]) + 1} has no cell")
            if parent_scene is not None:
                held_lo = parent_lo.cpu().numpy().astype(np.int64)
                held_hi = parent_hi.cpu().numpy().astype(np.int64)
                split = np.nonzero(held_lo != held_hi)[0]
                if split.size:
                    c = int(split[0])
                    raise RuntimeError(f"{where}: clump {c + 1} lies in clumps {int(held_lo[c])} "
                                       f"to {int(held_hi[c])} of the threshold below")
                parent_labels[step] = held_lo
            counts[step] = n
            extents.append(extent)
            cells.append(counted.cpu().numpy())
            for held, (field_sums, field_totals) in zip(sums, summed):
                held.append(field_sums.cpu().numpy())
                nonfinite += int(field_totals[1].item())
            if binding is not None:
                bindings.append(clump_binding_scene(
                    ctx, labels, n, cells[-1].sum(axis=0), binding["mass"], binding["velocity"],
                    binding["thermal"], cell_sizes, prob_lo, ref_ratio, G=binding["G"],
                    min_cells=binding["min_cells"], max_cells=binding["max_cells"],
                    n_ranks=n_ranks))
            below, n_below = labels, n
    total = sum(counts)
    extent = np.concatenate(extents + [np.zeros((6, 0), dtype=np.int64)], axis=1)
    index_lo = np.ascontiguousarray(extent[:3].T)
    index_hi = np.ascontiguousarray(extent[3:].T)
    origin = np.array([float(v) for v in prob_lo], dtype=np.float64)
    finest = np.array(sizes[n_levels - 1], dtype=np.float64)
    empty_cells = np.zeros((n_levels, 0), dtype=np.int64)
    empty_sums = np.zeros((n_levels, 0), dtype=np.float64)
    found = {"n": total, "counts": counts, "parent_labels": parent_labels,
             "index_lo": index_lo, "index_hi": index_hi,
             "left_edge": origin + index_lo.astype(np.float64) * finest,
             "right_edge": origin + (index_hi + 1).astype(np.float64) * finest,
             "cells_by_level": np.concatenate(cells + [empty_cells], axis=1),
             "sums": [np.concatenate(held + [empty_sums], axis=1) for held in sums],
             "nonfinite": nonfinite}
    if binding is not None:
        kinds = {"mass": np.float64, "self_energy": np.float64, "kinetic": np.float64,
                 "thermal": np.float64, "bound": bool, "evaluated": bool, "excluded": np.int64}
        found["binding"] = {key: np.concatenate([b[key] for b in bindings] +
                                                [np.zeros(0, dtype=kind)])
                            for key, kind in kinds.items()}
        found["binding"]["nonfinite"] = sum(b["nonfinite"] for b in bindings)
    return found


def clump_tree(plotfile: str, variable: str, thresholds, upper: float = math.inf,
               fields: Sequence[str] = (), min_cells: int = 1, min_level: int = 0,
               max_level: int = -1, output: Optional[str] = None, mass: Optional[str] = None,
               velocity: Optional[Sequence[str]] = None, thermal: Optional[str] = None,
               G: float = 6.6743e-8, max_cells: int = 2 ** 18) -> dict:
    """The clump tree of a plotfile's variable over a ladder of thresholds ("Clump
    tree"; yt's find_clumps), on cuda:0.  thresholds and upper as clump_tree_scene takes them
    (clumps.threshold_ladder gives yt's ladder); variable and every name of fields as api.clumps
    takes them.  Returns a dict: thresholds, upper, n (nodes; node v is clump label[v] of threshold
    threshold_index[v], numbered by ascending threshold, then label), node_begin int64 [k + 1],
    threshold_index, label, parent (-1 at the first threshold) int64 [n], child_offsets int64 [n +
    1] and children (CSR, ascending), cells_by_level int64 [L, n], cells, volume and integrals
    {name: float64 [n]} as api.clumps makes them, index_lo, index_hi int64 [n, 3] (the inclusive
    bounding box in the finest loaded level's index space), left_edge, right_edge float64 [n, 3],
    kept, kept_parent and leaves (clumps.collapse_tree with min_cells: a clump that does not split
    is the same clump), and nonfinite.  n == 0 gives empty arrays.  With mass (velocity, thermal,
    G and max_cells as api.clumps takes them) every node of max(min_cells, 2) to max_cells cells
    is tested for gravitational binding, the dict gains mass, self_energy, kinetic, thermal,
    bound, evaluated and excluded per node, and collapse_tree takes bound as its passes: an
    unbound clump and everything below it are dropped, as yt's gravitationally_bound validator
    drops them.  With output, the dict is also written as one .npz (clumps.save_tree_npz)."""
    import numpy as np
    from . import clumps as clump_rules
    from . import plotfile as pf
    thresholds, upper = clump_rules.check_thresholds(thresholds, upper)
    min_cells = int(min_cells)
    if min_cells < 1:
        raise ValueError("min_cells must be at least 1")
    names = [str(name) for name in fields]
    binding_names = _binding_names(mass, velocity, thermal)
    if mass is not None:
        clump_rules.check_max_cells(max_cells)
    ctx, rank, world, group, scenes, volumes = _load_fields(
        plotfile, [variable] + names + binding_names, min_level, max_level)
    header = pf.PlotFileData(plotfile)
    n_levels = len(volumes)
    binding = None
    if mass is not None:
        mass_scene, velocity_scenes, thermal_scene = _binding_scenes(scenes, 1 + len(names), mass,
                                                                     velocity, thermal)
        binding = {"mass": mass_scene, "velocity": velocity_scenes, "thermal": thermal_scene,
                   "G": G, "min_cells": min_cells, "max_cells": max_cells}
    found = clump_tree_scene(ctx, scenes[0], thresholds, upper, *_header_levels(header, n_levels),
                             tables=scenes[1:1 + len(names)], rank=rank, n_ranks=world,
                             binding=binding)
    nodes = clump_rules.tree_nodes(found["counts"], found["parent_labels"])
    cells_by_level = found["cells_by_level"]
    cells = cells_by_level.sum(axis=0)
    tree = {"thresholds": np.array(thresholds, dtype=np.float64), "upper": upper, "n": found["n"]}
    tree.update(nodes)
    tree.update({"cells_by_level": cells_by_level, "cells": cells,
                 "volume": clump_rules.clump_volumes(cells_by_level, volumes),
                 "integrals": {name: clump_rules.clump_integrals(summed, volumes)
                               for name, summed in zip(names, found["sums"])},
                 "index_lo": found["index_lo"], "index_hi": found["index_hi"],
                 "left_edge": found["left_edge"], "right_edge": found["right_edge"]})
    if binding is None:
        tree.update(clump_rules.collapse_tree(nodes["parent"], cells, min_cells))
        tree["nonfinite"] = found["nonfinite"]
    else:
        tested = found["binding"]
        tree.update({key: tested[key] for key in ("mass", "self_energy", "kinetic", "thermal",
                                                  "bound", "evaluated", "excluded")})
        tree.update(clump_rules.collapse_tree(nodes["parent"], cells, min_cells, tested["bound"]))
        tree["nonfinite"] = found["nonfinite"] + tested["nonfinite"]
    if output:
        clump_rules.save_tree_npz(output, tree)
    return tree


# ---- isosurfaces ("Isosurface") -----------------------------------------------------

def isosurface_scene(ctx, scene: "SceneGeometry", value: float, cell_sizes, prob_lo, ref_ratio,
                     sample: Optional["SceneGeometry"] = None, rank: int = 0, n_ranks: int = 1):
    """The isosurface field == value of a scene's raw field by marching tetrahedra (DESIGN.md 7,
    "Isosurface"), as a triangle soup in a canonical order.  scene, cell_sizes, prob_lo and
    ref_ratio as gradient_scene takes them; sample: a scene with the same boxes whose field is
    interpolated at every vertex.  Returns (vertices float64 [n, 3, 3] in the plotfile's physical
    units, levels uint8 [n], samples float64 [n, 3] or None, skipped): numpy arrays and the number
    of surface cubes left out for a corner that is not finite.  One call counts, the arrays are
    allocated, a second call emits.  Every box of the scene must be on this rank: with n_ranks >
    1, or fewer local boxes than boxes, NotImplementedError is raised before any device work."""
    import numpy as np
    value = float(value)
    if not math.isfinite(value):
        raise ValueError("an isosurface's value must be finite")
    _require_one_rank(scene, n_ranks, "an isosurface needs every box of the scene on one rank: "
                      "ghost cells are not exchanged between ranks")
    if sample is not None and len(sample.local_boxes) != len(scene.local_boxes):
        raise ValueError("the sample scene must hold the same boxes as the scene")
    sizes, ratios, index = _level_setup(scene, scene.local_boxes, cell_sizes, prob_lo, ref_ratio)
    origin = [float(v) for v in prob_lo]
    with _native_scenes(ctx, [scene, sample]) as (field, other):
        counts, _, _, _ = field.isosurface(value, index, ratios, sizes, origin, other)
        ctx.synchronize()
        n, skipped = (int(v) for v in counts.cpu().tolist())
        vertices = np.zeros((0, 3, 3), dtype=np.float64)
        levels = np.zeros(0, dtype=np.uint8)
        samples = np.zeros((0, 3), dtype=np.float64) if sample is not None else None
        if n > 0:
            _, v, l, s = field.isosurface(value, index, ratios, sizes, origin, other, capacity=n)
            ctx.synchronize()
            vertices, levels = v.cpu().numpy(), l.cpu().numpy()
            if s is not None:
                samples = s.cpu().numpy()
    return vertices, levels, samples, skipped


def isosurface(plotfile: str, variable: str, value: float, fields: Sequence[str] = (),
               min_level: int = 0, max_level: int = -1, output: Optional[str] = None) -> dict:
    """The isosurface variable == value of a plotfile ("Isosurface"), on cuda:0, over
    the uncovered cells of the loaded levels.  variable and every name of fields is a stored
    variable or a registered derived, gradient, clump or grid field.  Returns a dict: n (triangles),
    vertices float64 [n, 3, 3] in the plotfile's physical units, the normal (v1 - v0) x (v2 - v0)
    pointing to the variable < value side, level uint8 [n] (the level of the cube a triangle came
    from), area float64 [n] = 0.5 |cross|, total_area (math.fsum), samples {name: float64 [n, 3]}
    (each requested field interpolated at every vertex) and skipped (surface cubes left out for a
    corner that is not finite).  n == 0 gives empty arrays.  With output the surface is written
    as a binary PLY file, the samples as vertex properties (surfaces.save_ply).  At a coarse-fine
    interface the surface has a crack of half the difference of the two cell sizes."""
    import numpy as np
    from . import plotfile as pf
    from . import surfaces
    names = [str(name) for name in fields]
    ctx, rank, world, group, scenes, volumes = _load_fields(plotfile, [variable] + names,
                                                            min_level, max_level)
    header = pf.PlotFileData(plotfile)
    n_levels = len(volumes)
    arguments = (float(value), *_header_levels(header, n_levels))
    samples = {}
    if names:
        for name, scene in zip(names, scenes[1:]):
            vertices, levels, sampled, skipped = isosurface_scene(ctx, scenes[0], *arguments,
                                                                  scene, rank, world)
            samples[name] = sampled
    else:
        vertices, levels, _, skipped = isosurface_scene(ctx, scenes[0], *arguments, None, rank,
                                                        world)
    area = surfaces.triangle_areas(vertices)
    result = {"n": int(vertices.shape[0]), "vertices": vertices, "level": levels, "area": area,
              "total_area": math.fsum(area.tolist()), "samples": samples, "skipped": skipped}
    if output:
        surfaces.save_ply(vertices, output, samples)
    return result


# ---- streamlines ("Streamlines") ------------------------------------------------------

def streamline_scene(ctx, vx: "SceneGeometry", vy: "SceneGeometry", vz: "SceneGeometry", seeds,
                     cell_sizes, prob_lo, ref_ratio, step: float = 0.5, max_steps: int = 1000,
                     direction: int = 1, sample: Optional["SceneGeometry"] = None, rank: int = 0,
                     n_ranks: int = 1):
    """RK4 field lines of the vector field (vx, vy, vz) -- three scenes with the same boxes --
    from seeds [n, 3] in the plotfile's physical units ("Streamlines"): steps of step
    times the leaf's smallest cell size along the unit vector, direction +1 or -1, at most
    max_steps steps.  cell_sizes, prob_lo and ref_ratio as gradient_scene takes them; sample: a
    scene with the same boxes whose field is interpolated at every point.  Returns numpy arrays
    (points float64 [n, max_steps + 1, 3], NaN past a line's count; counts int64 [n]; status uint8
    [n]: 0 max_steps reached, 1 outside, 2 stagnant, 3 not finite; samples float64 [n, max_steps +
    1] or None).  Every box of the scene must be on this rank: with n_ranks > 1, or fewer local
    boxes than boxes, NotImplementedError is raised before any device work."""
    import numpy as np
    step, direction, max_steps = float(step), int(direction), int(max_steps)
    if not (math.isfinite(step) and 0.0 < step <= 1.0):
        raise ValueError("step must be finite and lie in (0, 1]")
    if direction not in (1, -1):
        raise ValueError("direction must be +1 or -1")
    if not 0 <= max_steps <= 2 ** 20:
        raise ValueError("max_steps must lie in [0, 2^20]")
    _require_one_rank(vx, n_ranks, "streamlines need every box of the scene on one rank: "
                      "lines are not handed over between ranks")
    if any(scene is not None and len(scene.local_boxes) != len(vx.local_boxes)
           for scene in (vy, vz, sample)):
        raise ValueError("the scenes must hold the same boxes")
    start = np.ascontiguousarray(seeds, dtype=np.float64)
    if start.ndim != 2 or start.shape[1] != 3:
        raise ValueError("seeds must be an array [n, 3]")
    if start.shape[0] * (max_steps + 1) >= 2 ** 32:
        raise ValueError("n_seeds * (max_steps + 1) must stay below 2^32")
    sizes, ratios, index = _level_setup(vx, vx.local_boxes, cell_sizes, prob_lo, ref_ratio)
    origin = [float(v) for v in prob_lo]
    with _native_scenes(ctx, [vx, vy, vz, sample]) as fields:
        points, samples, counts, status = fields[0].streamlines(
            fields[1], fields[2], start, step, direction, max_steps, index, ratios, sizes, origin,
            fields[3])
        ctx.synchronize()
        points, counts, status = points.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy()
        if samples is not None:
            samples = samples.cpu().numpy()
    return points, counts.astype(np.int64), status, samples


_DIRECTIONS = {"forward": (1,), "backward": (-1,), "both": (-1, 1)}


def streamlines(plotfile: str,
                variables: Sequence[str] = ("x-velocity", "y-velocity", "z-velocity"),
                seeds=(), step: float = 0.5, max_steps: int = 1000, direction: str = "forward",
                fields: Sequence[str] = (), min_level: int = 0, max_level: int = -1,
                output: Optional[str] = None) -> dict:
    """Field lines of a plotfile's vector field ("Streamlines"), on cuda:0, through
    the uncovered cells of the loaded levels: classical RK4 along the unit vector of the three
    variables, trilinear between cell centres and piecewise constant in the one-cell layer next to
    a domain face, a hole or a finer region.  variables and every name of fields is a stored
    variable or a registered derived, gradient, clump or grid field; seeds: [n, 3] in the plotfile's
    physical units; direction "forward", "backward" or "both" (a backward and a forward call,
    joined as the backward line reversed, then the forward line, the seed kept once).  Returns a
    dict: n (lines), lines (a list of float64 [count_i, 3]; empty for a seed outside the loaded
    cells), status uint8 [n] (0 max_steps reached, 1 outside, 2 stagnant, 3 not finite; [n, 2] =
    (backward, forward) with "both"), length float64 [n] (math.fsum of a line's segment lengths)
    and samples {name: list of float64 [count_i]} (each requested field at every point, NaN at a
    final point that is outside).  With output the lines are written as a legacy-VTK ASCII file,
    the samples as point scalars (lines.save_vtk_lines)."""
    import numpy as np
    from . import lines as line_rules
    from . import plotfile as pf
    if direction not in _DIRECTIONS:
        raise ValueError('direction must be "forward", "backward" or "both"')
    components = [str(name) for name in variables]
    if len(components) != 3:
        raise ValueError("variables must name the three components")
    names = [str(name) for name in fields]
    start = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 3)
    ctx, rank, world, group, scenes, volumes = _load_fields(plotfile, components + names,
                                                            min_level, max_level)
    header = pf.PlotFileData(plotfile)
    n_levels = len(volumes)
    arguments = (*_header_levels(header, n_levels), float(step), int(max_steps))
    passes = []        # per direction (lines, status, {name: values per line})
    for sign in _DIRECTIONS[direction]:
        sampled = {}
        for name, scene in zip(names or [None], scenes[3:] or [None]):
            points, counts, status, values = streamline_scene(ctx, *scenes[:3], start, *arguments,
                                                              sign, scene, rank, world)
            if name is not None:
                sampled[name] = [values[i, :int(c)].copy() for i, c in enumerate(counts.tolist())]
        passes.append((line_rules.split_lines(points, counts), status, sampled))
    if len(passes) == 2:
        (back, back_status, back_values), (ahead, ahead_status, ahead_values) = passes
        found = line_rules.join_both(back, ahead)
        status = np.stack([back_status, ahead_status], axis=1)
        samples = {name: line_rules.join_both(back_values[name], ahead_values[name])
                   for name in names}
    else:
        found, status, samples = passes[0]
    result = {"n": len(found), "lines": found, "status": status,
              "length": line_rules.line_lengths(found), "samples": samples}
    if output:
        line_rules.save_vtk_lines(found, output, samples)
    return result


def sample_points(plotfile: str, points, fields: Sequence[str], min_level: int = 0,
                  max_level: int = -1):
    """The value of every field of fields at every point of points [n, 3] (the plotfile's physical
    units), on cuda:0, by the streamlines' rule ("Streamlines"): trilinear between the
    eight cell centres around the point if all are present (the same level as the point's leaf, or
    coarser) and finite, else the value of the leaf cell itself.  Returns ({name: float64 [n]},
    inside bool [n]): a point outside the loaded cells has NaN and inside False.  A thin wrapper:
    lines of no steps, the field itself as the three components and as the sample."""
    import numpy as np
    from . import plotfile as pf
    names = [str(name) for name in fields]
    if not names:
        raise ValueError("sample_points needs at least one field")
    at = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    ctx, rank, world, group, scenes, volumes = _load_fields(plotfile, names, min_level, max_level)
    header = pf.PlotFileData(plotfile)
    n_levels = len(volumes)
    values, inside = {}, np.zeros(at.shape[0], dtype=bool)
    for name, scene in zip(names, scenes):
        _, counts, _, sampled = streamline_scene(
            ctx, scene, scene, scene, at, *_header_levels(header, n_levels), 1.0, 0, 1, scene,
            rank, world)
        values[name] = sampled[:, 0].copy()
        inside = counts == 1
    return values, inside


# ---- what the grid products share: covering grids, power spectra, the Helmholtz split, potentials --

def _plotfile_grid(plotfile: str, level, region, left_edge, right_edge, min_level: int,
                   max_level: int, check_dims):
    """(header, level, lo, dims) of a plotfile-level function over a grid of one level: region
    and level as api.covering_grid has them and the product's rule on dims -- check_dims, which
    returns them or raises -- before anything is loaded."""
    from . import grids
    from . import plotfile as pf
    if region is not None and (left_edge is not None or right_edge is not None):
        raise ValueError("give region or left_edge / right_edge, not both")
    if (left_edge is None) != (right_edge is None):
        raise ValueError("left_edge and right_edge go together")
    _require_plotfile(plotfile)
    header = pf.PlotFileData(plotfile)
    _, finest_loaded = pf.clamp_levels(int(min_level), int(max_level), header.finest_level)
    level = finest_loaded if level is None else int(level)
    if not 0 <= level <= header.finest_level:
        raise ValueError(f"level must lie in [0, {header.finest_level}], the plotfile's levels")
    size = header.cell_size[level]
    if region is not None:
        first, last = (tuple(int(v) for v in corner) for corner in region)
        if len(first) != 3 or len(last) != 3:
            raise ValueError("region must be ((ilo, jlo, klo), (ihi, jhi, khi))")
        lo, dims = first, tuple(last[a] - first[a] + 1 for a in range(3))
        if min(dims) < 1:
            raise ValueError("region must hold at least one cell along every axis")
    elif left_edge is not None:
        lo, dims = grids.index_region(header.prob_lo, size, left_edge, right_edge)
    else:
        refine = math.prod(header.ref_ratio[:level])
        domain_lo, domain_hi = header.prob_domain[0]
        lo = tuple(v * refine for v in domain_lo)
        dims = tuple((domain_hi[a] + 1) * refine - lo[a] for a in range(3))
    return header, level, lo, check_dims(dims)


def _grid_arguments(header, scene: "SceneGeometry", level: int, lo, dims):
    """(level, lo, dims, cell_sizes, prob_lo, ref_ratio) as the *_scene functions of the grid
    products take them: the levels run up to the finer of `level` and the finest loaded one."""
    n_levels = max(level, max(int(b.level) for b in scene.all_boxes)) + 1
    return (level, lo, dims, *_header_levels(header, n_levels))


def _grid_head(header, level: int, lo, dims, **between) -> dict:
    """How the result of a plotfile-level grid product begins: level, lo, dims, the entries the
    product puts there (`between`) and the level's cell size."""
    return {"level": level, "lo": lo, "dims": dims, **between,
            "cell_size": tuple(float(v) for v in header.cell_size[level])}


def _scene_grid_arguments(scene: "SceneGeometry", level, lo, dims, cell_sizes, n_ranks: int,
                          what: str, check_dims):
    """(level, lo, dims, the level's cell size) of a *_scene function over a grid whose dims
    check_dims admits (spectra.check_dims: a periodic power-of-two grid), checked before any
    device work."""
    level = int(level)
    lo = tuple(int(v) for v in lo)
    if len(lo) != 3:
        raise ValueError("lo and dims must hold three values")
    dims = check_dims(dims)
    _require_one_rank(scene, n_ranks, f"{what} needs every box of the scene on one rank: cells "
                      "are not gathered between ranks")
    sizes = [tuple(float(v) for v in c) for c in cell_sizes]
    if not 0 <= level < len(sizes):
        raise ValueError("level must lie in [0, the number of cell_sizes)")
    return level, lo, dims, sizes[level]


def _covered_grid(field, level, lo, dims, index, ratios, fill):
    """(values, absent) of one native scene's covering grid; absent cells without a fill value
    raise ValueError."""
    import torch
    values, coverage, _ = field.covering_grid(level, lo, dims, index, ratios,
                                              math.nan if fill is None else float(fill), True)
    absent = int(torch.count_nonzero(coverage == 0.0).item())
    if absent and fill is None:
        raise ValueError(f"{absent} cells of the region hold no data: pass a fill value, or a "
                         "region the loaded levels cover")
    return values, absent


def _edge_arguments(edges, bins, k_range, k_log, grid=None):
    """The edges of api.power_spectrum and api.helmholtz, in two calls.  Without grid, on the
    arguments alone, before anything is loaded: edges exclude bins, k_range and k_log and are
    checked; returns them, or None.  With grid = (dims, cell size), once these are known: the
    edges spectra.make_edges makes where none were given, checked for their squares."""
    from . import spectra
    if grid is None:        # the first call: what the arguments alone can be refused for
        if edges is not None and (bins is not None or k_range is not None or k_log):
            raise ValueError("give edges or bins / k_range / k_log, not both")
        if edges is not None:
            edges = spectra.check_edges(edges)
    elif edges is None:     # the second call without explicit edges: made for this grid
        edges = spectra.make_edges(*grid, bins, k_range, bool(k_log))
    if edges is not None:   # either call, whenever there are edges: their squares must differ
        spectra.squared_edges(edges)
    return edges


def _shell_sums(binned, dims, k_edges):
    """(power, spectrum, k, outside, nonfinite) of what Context.spectrum_bins returned, binned =
    (modes, sums, totals) as numpy arrays, over a grid of dims (spectra.normalise)."""
    from . import spectra
    _, sums, totals = binned
    power, spectrum, k = spectra.normalise(sums, dims[0] * dims[1] * dims[2], k_edges)
    return power, spectrum, k, int(totals[0]), int(totals[1])


# ---- covering grids ("Covering grid") ------------------------------------------------

def covering_grid_scene(ctx, scene: "SceneGeometry", level: int, lo, dims, cell_sizes, prob_lo,
                        ref_ratio, fill: float = math.nan, with_coverage: bool = True,
                        rank: int = 0, n_ranks: int = 1):
    """A scene's raw field resampled to the cells [lo, lo + dims) of level `level` (DESIGN.md 7,
    "Covering grid"): where a leaf of the same or a coarser level holds the cell, that leaf's
    value with its bits kept; where finer leaves lie in it, their volume-weighted mean; where
    nothing does, fill.  lo and dims = (nx, ny, nz) are level-`level` indices; the region may
    leave the domain.  scene, prob_lo as gradient_scene takes them; cell_sizes and ref_ratio run
    up to the finer of `level` and the finest loaded level at least (every entry of cell_sizes
    counts as a level, 16 at the most).  Returns numpy arrays (values float64 [nz, ny, nx], coverage float64
    [nz, ny, nx]: the fraction of the cell's volume that loaded leaves fill, cell level int8
    [nz, ny, nx]: the level of the finest leaf used, -1 for none); the last two are None without
    with_coverage -- they depend on the boxes alone.  Every box of the scene must be on this rank:
    with n_ranks > 1, or fewer local boxes than boxes, NotImplementedError is raised before any
    device work."""
    level = int(level)
    lo, dims = tuple(int(v) for v in lo), tuple(int(v) for v in dims)
    if len(lo) != 3 or len(dims) != 3:
        raise ValueError("lo and dims must hold three values")
    if min(dims) < 1:
        raise ValueError("dims must be at least 1")
    _require_one_rank(scene, n_ranks, "a covering grid needs every box of the scene on one rank: "
                      "cells are not gathered between ranks")
    if not 0 <= level < len(list(cell_sizes)):
        raise ValueError("level must lie in [0, the number of cell_sizes)")
    sizes, ratios, index = _level_setup(scene, scene.local_boxes, cell_sizes, prob_lo, ref_ratio)
    with _native_scenes(ctx, [scene]) as (field,):
        values, coverage, cell_level = field.covering_grid(level, lo, dims, index, ratios,
                                                           float(fill), bool(with_coverage))
        ctx.synchronize()
        values = values.cpu().numpy()
        if coverage is not None:
            coverage, cell_level = coverage.cpu().numpy(), cell_level.cpu().numpy()
    return values, coverage, cell_level


def covering_grid(plotfile: str, level: Optional[int] = None, fields: Sequence[str] = (),
                  region=None, left_edge=None, right_edge=None, min_level: int = 0,
                  max_level: int = -1, fill: float = math.nan,
                  output: Optional[str] = None) -> dict:
    """Fields of a plotfile as plain arrays at one level (yt's covering_grid; DESIGN.md 7, "Covering
    grid"), on cuda:0: piecewise constant where the loaded data is coarser than `level`, the
    volume-weighted mean of the leaves where it is finer, fill where no loaded level has a cell.
    level: 0 .. the plotfile's finest level, by default the finest loaded one.  fields: stored
    variables or registered derived, gradient, clump or grid fields; by default the plotfile's first
    variable.  region = ((ilo, jlo, klo), (ihi, jhi, khi)), inclusive level-`level` indices, or
    left_edge / right_edge in the plotfile's physical units (the cells whose centres lie in
    [left_edge, right_edge); grids.index_region), not both; by default the whole domain.  Either
    may leave the domain.  Returns a dict: level, lo (the index of the first cell), dims (nx, ny,
    nz), left_edge, right_edge and cell_size (physical), fields {name: float64 [nz, ny, nx]},
    coverage float64 [nz, ny, nx] (the fraction of a cell's volume that loaded leaves fill),
    cell_level int8 [nz, ny, nx] (the finest level used, -1 for none), absent (cells of coverage
    0) and partial (cells of a coverage strictly between 0 and 1).  With output the dict is
    written as one .npz file (grids.save_npz)."""
    import numpy as np
    from . import grids
    header, level, lo, dims = _plotfile_grid(plotfile, level, region, left_edge, right_edge,
                                             min_level, max_level,
                                             lambda dims: dims)   # a region of any size
    names = [str(name) for name in fields] or [header.var_names[0]]
    ctx, rank, world, group, scenes, _ = _load_fields(plotfile, names, min_level, max_level)
    arguments = (*_grid_arguments(header, scenes[0], level, lo, dims), float(fill))
    found, coverage, cell_level = {}, None, None
    for name, scene in zip(names, scenes):
        # coverage and cell level are the same for every field of one plotfile: once
        values, c, l = covering_grid_scene(ctx, scene, *arguments, coverage is None, rank, world)
        found[name] = values
        if coverage is None:
            coverage, cell_level = c, l
    left, right = grids.grid_edges(header.prob_lo, header.cell_size[level], lo, dims)
    result = {**_grid_head(header, level, lo, dims, left_edge=left, right_edge=right),
              "fields": found, "coverage": coverage, "cell_level": cell_level,
              "absent": int(np.count_nonzero(coverage == 0.0)),
              "partial": int(np.count_nonzero((coverage > 0.0) & (coverage < 1.0)))}
    if output:
        grids.save_npz(result, output)
    return result


# ---- grid fields ("Grid fields") -----------------------------------------------------

def grid_scene(ctx, geometry: "SceneGeometry", grid, level: int, lo, cell_sizes, prob_lo,
               ref_ratio, interpolation: str = "constant", periodic: bool = False,
               fill: float = math.nan, rank: int = 0, n_ranks: int = 1, process_group=None,
               log_scale_input: bool = False, normalize_to_data_range: bool = True):
    """A uniform grid written back onto the cells of a scene ("Grid fields"), the
    inverse of covering_grid_scene: grid is a numpy or torch float64 [nz, ny, nx] array of the
    level-`level` cells from the index lo on (what covering_grid_scene, a potential or a Helmholtz
    component is); geometry is any loaded scene, whose boxes the result has.  A cell of `level`
    gets the grid's value with its bits kept; a finer cell the value of the grid cell that holds
    it ("constant") or the trilinear interpolation between the grid's cell centres ("linear";
    past the region's faces the grid is wrapped with periodic and clamped without); a coarser
    cell the mean of the grid cells inside it; a cell the grid does not reach gets fill.
    cell_sizes, prob_lo and ref_ratio as covering_grid_scene takes them.  Returns (SceneGeometry,
    outside, partial): the cells that got fill, and the coarser cells only part of which the grid
    covers.  The output is allocated as derive_scene's is, and statistics and the scalar transform
    come from build_scene_geometry with the caller's flags.  Every box of the scene must be on
    this rank: with n_ranks > 1, or fewer local boxes than boxes, NotImplementedError is raised
    before any device work."""
    import numpy as np
    import torch
    from . import gridfields
    if interpolation not in gridfields.INTERPOLATIONS:
        raise ValueError('interpolation must be "constant" or "linear"')
    level = int(level)
    lo = tuple(int(v) for v in lo)
    if len(lo) != 3:
        raise ValueError("lo must hold three values")
    if not isinstance(grid, torch.Tensor):
        grid = torch.from_numpy(np.ascontiguousarray(grid, dtype=np.float64))
    if grid.ndim != 3 or grid.numel() == 0 or grid.dtype != torch.float64:
        raise ValueError("grid must be a float64 [nz, ny, nx] array with at least one cell")
    _require_one_rank(geometry, n_ranks, "a grid field needs every box of the scene on one rank: "
                      "the grid is not shared between ranks")
    if not 0 <= level < len(list(cell_sizes)):
        raise ValueError("level must lie in [0, the number of cell_sizes)")
    sizes, ratios, index = _level_setup(geometry, geometry.local_boxes, cell_sizes, prob_lo,
                                        ref_ratio)
    grid = grid.to(ctx.device).contiguous()
    written = _blank_like(ctx, geometry, rank)
    with _native_scenes(ctx, [written]) as (out,):
        totals = out.grid_field(grid, level, lo, index, ratios,
                                gridfields.INTERPOLATIONS.index(interpolation), bool(periodic),
                                float(fill))
        ctx.synchronize()
        outside, partial = (int(v) for v in totals.cpu().tolist())
    return _computed_scene(ctx, written, log_scale_input, normalize_to_data_range, process_group,
                           n_ranks), outside, partial


def _grid_product_device(ctx, entry: dict, inputs, level: int, lo, dims, cell_sizes, prob_lo,
                         ref_ratio, shared: dict, n_ranks: int):
    """The grid of a registered potential or Helmholtz field (gridfields.py) on the device, from
    the loaded scenes of its inputs.  shared: what the grid fields of one call have computed so
    far, by product -- a potential; the projected spectra of a velocity field, and every component
    transformed back from them (a transformed spectrum is used up, so each is transformed once)."""
    from . import spectra
    isolated = entry["kind"] == "potential" and entry["boundary"] == "isolated"
    first = inputs[0]
    level, lo, dims, size = _scene_grid_arguments(
        first, level, lo, dims, cell_sizes, n_ranks, "a grid field",
        spectra.check_isolated_dims if isolated else spectra.check_dims)
    for other in inputs[1:]:
        if len(other.local_boxes) != len(first.local_boxes):
            raise ValueError("the velocity components must be scenes over the same boxes")
    sizes, ratios, index = _level_setup(first, first.local_boxes, cell_sizes, prob_lo, ref_ratio)
    where, fill = (level, lo, dims), entry["fill"]
    if entry["kind"] == "potential":
        key = ("potential", entry["of"], entry["boundary"], entry["constant"],
               entry["self_term"], where, repr(fill))       # repr: a NaN equals itself
        if key not in shared:
            with _native_scenes(ctx, [first]) as (field,):
                if isolated:
                    scale, self_value = _isolated_scale(entry["constant"], entry["self_term"], size)
                    shared[key], _, _ = _isolated_potential_device(
                        ctx, field, level, lo, dims, index, ratios, size, scale, self_value, fill)
                else:
                    scale = -(entry["constant"] / (4.0 * math.pi * math.pi))
                    shared[key], _, _ = _potential_device(
                        ctx, field, level, lo, dims, index, ratios,
                        spectra.inverse_length_sq(dims, size), scale, fill)
                ctx.synchronize()
        return shared[key]
    split = ("helmholtz", entry["velocity"], where, repr(fill))
    if split not in shared:
        with _native_scenes(ctx, inputs) as fields:
            shared[split], _ = _helmholtz_spectra_device(
                ctx, fields, level, lo, dims, index, ratios, spectra.inverse_length(dims, size),
                fill)
            ctx.synchronize()
    wanted = (entry["part"], entry["component"])
    if split + wanted not in shared:
        shared[split + wanted] = _helmholtz_grids_device(ctx, shared[split], [wanted])[0][wanted]
    return shared[split + wanted]


def _grid_field_scene(ctx, plotfile: str, entry: dict, inputs, geometry: "SceneGeometry",
                      shared: dict, min_level: int, max_level: int, rank: int, n_ranks: int,
                      process_group, log_scale_input: bool, normalize_to_data_range: bool):
    """The scene of a registered grid field (gridfields.py): its grid -- the caller's array, or
    the product computed from the loaded scenes `inputs`, which stays on the device -- written
    onto the boxes of `geometry` by grid_scene.  The region and the level follow _plotfile_grid's
    rules (level None: the call's finest loaded level) with the product's own rule on dims."""
    from . import plotfile as pf
    from . import spectra
    if entry["kind"] == "array":
        header = pf.PlotFileData(plotfile)
        level, lo, grid = entry["level"], entry["lo"], entry["array"]
        if level > header.finest_level:
            raise ValueError(f"level must lie in [0, {header.finest_level}], the plotfile's levels")
        arguments = _grid_arguments(header, geometry, level, lo, None)
    else:
        isolated = entry["kind"] == "potential" and entry["boundary"] == "isolated"
        header, level, lo, dims = _plotfile_grid(
            plotfile, entry["level"], entry["region"], entry["left_edge"], entry["right_edge"],
            min_level, max_level, spectra.check_isolated_dims if isolated else spectra.check_dims)
        arguments = _grid_arguments(header, geometry, level, lo, dims)
        grid = _grid_product_device(ctx, entry, inputs, *arguments, shared, n_ranks)
    _, _, _, cell_sizes, prob_lo, ref_ratio = arguments
    scene, _, _ = grid_scene(ctx, geometry, grid, level, lo, cell_sizes, prob_lo, ref_ratio,
                             entry["interpolation"], entry["periodic"], entry["outside"], rank,
                             n_ranks, process_group, log_scale_input, normalize_to_data_range)
    return scene


# ---- particle fields ("Particle fields") ---------------------------------------------

def deposit_scene(ctx, geometry: "SceneGeometry", positions, values, cell_sizes, prob_lo,
                  ref_ratio, method: str = "cic", quantity: str = "density", rank: int = 0,
                  n_ranks: int = 1, process_group=None, log_scale_input: bool = False,
                  normalize_to_data_range: bool = True):
    """Particles deposited onto the cells of a scene ("Particle fields"): positions
    is a numpy or torch [n, 3] array in the plotfile's physical units, values an [n] array or None
    (1.0 each); geometry is any loaded scene, whose boxes the result has.  With method "ngp" a
    particle's value goes to the leaf cell that holds it; with "cic" it is shared among the eight
    cell centres around it at the leaf's level, under the same-or-coarser rule of the
    streamlines' corners, and the share of a corner that rule does not find (a domain face, a
    hole, a region that finer cells cover) stays with the particle's own cell.  A cell's value is
    the sum of its shares in particle order (quantity "sum"), or that sum over the cell's volume
    ("density").  cell_sizes, prob_lo and ref_ratio as streamline_scene takes them.  Returns
    (SceneGeometry, outside, rerouted): the particles without a leaf, which deposit nothing, and
    the corner shares that stayed with their own cell.  The output is allocated as derive_scene's
    is, and statistics and the scalar transform come from build_scene_geometry with the caller's
    flags.  Every box of the scene must be on this rank: with n_ranks > 1, or fewer local boxes
    than boxes, NotImplementedError is raised before any device work."""
    from . import particles
    particles.check_method(method)
    particles.check_quantity(quantity)
    positions, values = particles.check_arrays(positions, values)
    _require_one_rank(geometry, n_ranks, "a particle field needs every box of the scene on one "
                      "rank: a particle's cloud is not shared between ranks")
    sizes, ratios, index = _level_setup(geometry, geometry.local_boxes, cell_sizes, prob_lo,
                                        ref_ratio)
    written = _blank_like(ctx, geometry, rank)
    with _native_scenes(ctx, [written]) as (out,):
        cells, shares, _, totals = out.particle_cells(
            positions, values, particles.METHODS.index(method), index, ratios, sizes, prob_lo)
        out.particle_deposit(cells, shares, particles.QUANTITIES.index(quantity), sizes)
        ctx.synchronize()
        outside, rerouted = (int(v) for v in totals.cpu().tolist())
    return _computed_scene(ctx, written, log_scale_input, normalize_to_data_range, process_group,
                           n_ranks), outside, rerouted


def particle_cells(plotfile: str, positions, min_level: int = 0, max_level: int = -1) -> dict:
    """The leaf cell of every particle of positions [n, 3] (the plotfile's physical units) among
    the loaded levels, on cuda:0.  Returns a dict of numpy arrays: level uint8 [n] (255 for a
    particle outside the loaded cells), ordinal int64 [n] (the cell ordinal of "Clumps", -1
    outside) and centres float64 [n, 3] = prob_lo + (f64(I) + 0.5) * dx_l (NaN outside)."""
    import numpy as np
    import torch
    from . import particles
    from . import plotfile as pf
    positions, _ = particles.check_arrays(positions, None)
    ctx, rank, world, group, scenes, volumes = _load_fields(plotfile, [""], min_level, max_level)
    scene = scenes[0]
    _require_one_rank(scene, world, "a particle field needs every box of the scene on one rank: "
                      "a particle's cloud is not shared between ranks")
    header = pf.PlotFileData(plotfile)
    levels = _header_levels(header, len(volumes))
    sizes, ratios, index = _level_setup(scene, scene.local_boxes, *levels)
    with _native_scenes(ctx, [scene]) as (native,):
        cells, _, level_of, _ = native.particle_cells(positions, None, 0, index, ratios, sizes,
                                                      levels[1], levels=True)
        cells = cells.reshape(-1)
        inside = level_of != 255
        # the centres of the cells that were found, through the clump members' lookup
        found = cells[inside].contiguous()
        _, centres, _ = native.clump_member_data(found, index, ratios, sizes, levels[1])
        ctx.synchronize()
        inside = inside.cpu().numpy()
        where = np.full((inside.size, 3), np.nan)
        where[inside] = centres.cpu().numpy().T
        ordinal = torch.where(level_of != 255, cells, torch.full_like(cells, -1)).cpu().numpy()
    return {"level": level_of.cpu().numpy(), "ordinal": ordinal, "centres": where}


# ---- particle groups ("Particle groups") ----------------------------------------------

def particle_groups(positions, linking_length, masses=None, velocities=None,
                    min_members: int = 20, domain=None, periodic=False, max_pair_tests=None,
                    output: Optional[str] = None, ctx=None) -> dict:
    """Friends-of-friends groups of particles ("Particle groups"): positions is a
    numpy or torch [n, 3] array; two particles are linked iff they are at most linking_length
    apart (api.linking_length gives the conventional 0.2 mean separations), a group is a connected
    set of linked particles, and the groups of at least min_members members are numbered 1..count
    by their smallest particle index.  domain is (lo, hi) or a plotfile, whose prob_lo and prob_hi
    are taken; without one the box is the bounding box of the finite positions and periodic must
    be false.  periodic is a flag or three: on a periodic axis distances are minimum-image ones
    over the domain's extent, which must be more than three linking lengths, and a particle not in
    [lo, hi) there is outside.  A particle with a coordinate that is not finite is outside too;
    outside particles link to nothing and have label 0.

    The grouping runs on the device (ctx, or the runtime's context): the particles are binned into
    a uniform grid of cells at least a linking length wide and every pair in the same or adjacent
    cells is tested, so the cost is quadratic in a cell's occupancy.  The number of pair tests is
    counted exactly beforehand, and above max_pair_tests (None: groups.DEFAULT_MAX_PAIR_TESTS)
    ValueError names it before the link kernel is launched.  The result does not depend on the grid.

    Returns a dict: n; labels int32 [n] (0: none); count; first int64 [count] (each group's
    smallest member); offsets int64 [count + 1] and members int64 (particle indices by label, then
    ascending: group g + 1 has members[offsets[g]:offsets[g + 1]]); mass [count] (masses, or 1.0
    each) and centre [count, 3] (mass-weighted; on a periodic axis the first member's coordinate
    plus the mean minimum-image offset from it, wrapped into the domain -- meaningless for a group
    wider than half the period); with velocities also velocity [count, 3] (mass-weighted mean) and
    dispersion [count] (1-D rms about it); outside; pair_tests; dims (the grid that was used).
    The float sums are numpy's on the host.  output: an .npz file that gets the dict.
    ValueError, before any device work, for wrong shapes, dtypes that are not real, a
    linking_length that is not finite and positive, min_members below 1, and periodic without a
    domain."""
    import numpy as np
    import torch
    from . import groups
    positions, masses, velocities, b, min_members, box, flags, cap = groups.check_arguments(
        positions, linking_length, masses, velocities, min_members, domain, periodic,
        max_pair_tests)
    if cap is None:
        cap = groups.DEFAULT_MAX_PAIR_TESTS
    if ctx is None:
        ctx = _runtime_scope()[0]
    n = int(positions.shape[0])
    if isinstance(positions, torch.Tensor):
        points = positions.to(device=ctx.device, dtype=torch.float64).contiguous()
    else:
        points = torch.from_numpy(np.array(positions, dtype=np.float64, order="C")).to(ctx.device)
    if box is None:
        finite = torch.isfinite(points)
        finite_lo, finite_hi = [None] * 3, [None] * 3
        if n:
            low = torch.where(finite, points, torch.full_like(points, math.inf)).amin(0).tolist()
            high = torch.where(finite, points, torch.full_like(points, -math.inf)).amax(0).tolist()
            for d in range(3):
                if low[d] <= high[d]:
                    finite_lo[d], finite_hi[d] = low[d], high[d]
        box = groups.bounding_box(finite_lo, finite_hi, b)
    lo, hi = box
    dims = groups.choose_dims(n, b, lo, hi, flags)
    points, cells, parent, totals = ctx.particle_group_cells(points, lo, hi, dims, flags)
    labels, _, _, n_groups, pair_tests = ctx.particle_groups(
        points, cells, parent, b, lo, hi, dims, flags, min_members, max_pair_tests=cap)
    ctx.synchronize()
    labels = labels.cpu().numpy()
    count = int(n_groups.item())
    offsets, members, first = groups.member_lists(labels, count)
    host = points.cpu().numpy()
    result = {"n": n, "labels": labels, "count": count, "first": first, "offsets": offsets,
              "members": members}
    result.update(groups.catalogue(
        host, None if masses is None else groups._as_numpy(masses),
        None if velocities is None else groups._as_numpy(velocities), offsets, members, lo, hi,
        flags))
    result.update({"outside": int(totals.item()), "pair_tests": int(pair_tests),
                   "dims": tuple(int(v) for v in dims)})
    if output:
        np.savez(output, **{key: np.asarray(value) for key, value in result.items()})
    return result


# ---- power spectra ("Power spectrum") ------------------------------------------------

def power_spectrum_scene(ctx, scene: "SceneGeometry", level: int, lo, dims, cell_sizes, prob_lo,
                         ref_ratio, edges=None, fill: Optional[float] = None, rank: int = 0,
                         n_ranks: int = 1) -> dict:
    """The power spectrum of a scene's raw field over the cells [lo, lo + dims) of level `level`
    ("Power spectrum"): the covering grid of covering_grid_scene, its 3-D transform
    and the shell sums of |F|^2, all on the device; only the bins come back.  dims = (nx, ny, nz),
    every one a power of two in [1, 1024]; edges: n + 1 wave numbers (2 pi over a length), by
    default spectra.default_edges; fill: what a cell without data counts as -- with None such a
    cell (absent > 0) raises ValueError.  The other arguments are covering_grid_scene's.  Returns
    a dict: k_edges and k float64, power and spectrum float64 [n] (spectra.normalise), modes int64
    [n], outside and nonfinite (modes beyond the edges; modes whose |F|^2 is not finite) and
    absent.  With n_ranks > 1, or fewer local boxes than boxes, NotImplementedError is raised
    before any device work."""
    import numpy as np
    from . import spectra
    level, lo, dims, size = _scene_grid_arguments(scene, level, lo, dims, cell_sizes, n_ranks,
                                                  "a power spectrum", spectra.check_dims)
    k_edges = spectra.default_edges(dims, size) if edges is None else spectra.check_edges(edges)
    edges_sq = spectra.squared_edges(k_edges)
    g = spectra.inverse_length_sq(dims, size)
    sizes, ratios, index = _level_setup(scene, scene.local_boxes, cell_sizes, prob_lo, ref_ratio)
    with _native_scenes(ctx, [scene]) as (field,):
        values, absent = _covered_grid(field, level, lo, dims, index, ratios, fill)
        binned = ctx.spectrum_bins(ctx.fft3d(values), g, edges_sq)
        ctx.synchronize()
        binned = tuple(t.cpu().numpy() for t in binned)
    power, spectrum, k, outside, nonfinite = _shell_sums(binned, dims, k_edges)
    return {"k_edges": np.array(k_edges), "k": k, "power": power, "spectrum": spectrum,
            "modes": binned[0], "outside": outside, "nonfinite": nonfinite, "absent": absent}


def power_spectrum(plotfile: str, fields: Sequence[str] = (), level: Optional[int] = None,
                   region=None, left_edge=None, right_edge=None, bins: Optional[int] = None,
                   k_range=None, k_log: bool = False, edges=None, min_level: int = 0,
                   max_level: int = -1, fill: Optional[float] = None,
                   output: Optional[str] = None) -> dict:
    """Power spectra of fields of a plotfile ("Power spectrum"), on cuda:0: each
    field's covering grid at `level` over a region, its forward 3-D transform and |F|^2 summed
    over shells of the wave number k = 2 pi |m / L|.  fields, level, region, left_edge /
    right_edge, min_level and max_level as api.covering_grid takes them; the region must hold a
    power of two of cells, 1024 at most, along every axis.  edges: n + 1 wave numbers, or bins
    and / or k_range = (k_min, k_max) with k_log for equal ratios (spectra.make_edges); by
    default spectra.default_edges, one bin per fundamental up to the smallest Nyquist wave
    number.  fill: what a cell without data counts as; with None such cells raise ValueError.
    Returns a dict: level, lo, dims (nx, ny, nz), cell_size, k_edges [n + 1], k [n] (the bins'
    centres), fields {name: {"power", "spectrum", "modes"}} -- power [n]: sum |F|^2 / N^2 per bin,
    which over all modes adds up to the field's mean square; spectrum [n]: power per unit k;
    modes int64 [n] -- total [n] (the fields' power added in the order given: three velocity
    components give a kinetic-energy spectrum), outside and nonfinite (modes beyond the edges and
    modes whose |F|^2 is not finite, summed over the fields) and absent (cells without data).
    With output the dict is written as one .npz file (spectra.save_npz)."""
    import numpy as np
    from . import spectra
    edges = _edge_arguments(edges, bins, k_range, k_log)
    header, level, lo, dims = _plotfile_grid(plotfile, level, region, left_edge, right_edge,
                                             min_level, max_level, spectra.check_dims)
    edges = _edge_arguments(edges, bins, k_range, k_log, (dims, header.cell_size[level]))
    names = [str(name) for name in fields] or [header.var_names[0]]
    ctx, rank, world, group, scenes, _ = _load_fields(plotfile, names, min_level, max_level)
    arguments = (*_grid_arguments(header, scenes[0], level, lo, dims), edges, fill)
    found, total, outside, nonfinite, absent, k = {}, None, 0, 0, 0, None
    for name, scene in zip(names, scenes):
        one = power_spectrum_scene(ctx, scene, *arguments, rank, world)
        found[name] = {key: one[key] for key in ("power", "spectrum", "modes")}
        total = one["power"].copy() if total is None else total + one["power"]
        outside += one["outside"]
        nonfinite += one["nonfinite"]
        absent, k = one["absent"], one["k"]
    result = {**_grid_head(header, level, lo, dims),
              "k_edges": np.array(edges, dtype=np.float64), "k": k, "fields": found,
              "total": total, "outside": outside, "nonfinite": nonfinite, "absent": absent}
    if output:
        spectra.save_npz(result, output)
    return result


# ---- structure functions ("Structure functions") -------------------------------------

def _structure_arguments(n_fields: int, max_order, edges, bins, r_range, r_log):
    """What api.structure_functions and structure_function_scene can be refused for on the
    arguments alone: one field or three, the order, edges that exclude bins, r_range and r_log.
    Returns (max_order, the checked edges or None)."""
    from . import structure
    structure.kinds(n_fields)
    order = structure.check_order(max_order)
    if edges is not None and (bins is not None or r_range is not None or r_log):
        raise ValueError("give edges or bins / r_range / r_log, not both")
    return order, None if edges is None else structure.check_edges(edges)


def structure_function_scene(ctx, scenes, level: int, lo, dims, cell_sizes, prob_lo, ref_ratio,
                             lags=None, max_order: int = 6, periodic: bool = False, edges=None,
                             fill: Optional[float] = None, rank: int = 0,
                             n_ranks: int = 1) -> dict:
    """The structure functions S_p(r) = <|v(x + r) - v(x)|^p>, p = 1 .. max_order, of one scene's
    raw field or of the vector field of three scenes over the same boxes, over the cells [lo, lo +
    dims) of level `level` ("Structure functions"): the covering grids of
    covering_grid_scene and every pair of cells a lag apart, all on the device; only the per-lag
    sums come back.  dims = (nx, ny, nz), any values >= 1.  lags: integers [M, 3], rows (lx, ly,
    lz), M <= 4096, every |l_d| < N_d, one of each +/- pair; by default structure.default_lags.
    periodic: the region wraps; without it pairs that leave it count as outside.  edges: n + 1
    lengths to bin the lags by; by default one bin per distinct lag length.  fill: what a cell
    without data counts as -- with None such a cell (absent > 0) raises ValueError; with nan its
    pairs are left out and counted as nonfinite.  The other arguments are covering_grid_scene's.
    Returns a dict: lags int32 [M, 3], r_lag float64 [M], pairs_lag int64 [M], sums_lag float64
    [M, K, max_order]; r [n], r_edges (with edges), pairs int64 [n] and S {kind: float64
    [max_order, n]} with the kinds "scalar", or "longitudinal", "transverse" and "magnitude"
    (structure.bin_lags); outside, nonfinite and absent.  With n_ranks > 1, or fewer local boxes
    than boxes, NotImplementedError is raised before any device work."""
    import numpy as np
    from . import structure
    scenes = [scenes] if isinstance(scenes, SceneGeometry) else list(scenes)
    max_order, edges = _structure_arguments(len(scenes), max_order, edges, None, None, False)
    first = scenes[0]
    level, lo, dims, size = _scene_grid_arguments(first, level, lo, dims, cell_sizes, n_ranks,
                                                  "a structure function", structure.check_dims)
    for other in scenes[1:]:
        _require_one_rank(other, n_ranks, "a structure function needs every box of the scene on "
                          "one rank: cells are not gathered between ranks")
        if len(other.local_boxes) != len(first.local_boxes):
            raise ValueError("the three components must be scenes over the same boxes")
    lags = structure.check_lags(structure.default_lags(dims) if lags is None else lags, dims)
    r_lag = structure.lag_lengths(lags, size)
    directions = structure.unit_directions(lags, size) if len(scenes) == 3 else None
    sizes, ratios, index = _level_setup(first, first.local_boxes, cell_sizes, prob_lo, ref_ratio)
    with _native_scenes(ctx, scenes) as fields:
        grids, absent = [], 0
        for field in fields:
            values, absent = _covered_grid(field, level, lo, dims, index, ratios, fill)
            grids.append(values)
        found = ctx.structure_functions(grids, lags, directions, max_order, bool(periodic))
        ctx.synchronize()
        pairs_lag, sums_lag, totals = (t.cpu().numpy() for t in found)
    binned = structure.bin_lags(r_lag, pairs_lag, sums_lag, edges)
    result = {"lags": lags, "r_lag": r_lag, "pairs_lag": pairs_lag, "sums_lag": sums_lag,
              "r": binned["r"]}
    if edges is not None:
        result["r_edges"] = np.array(edges)
    result.update({"pairs": binned["pairs"],
                   "S": dict(zip(structure.kinds(len(scenes)), binned["S"])),
                   "outside": int(totals[0]), "nonfinite": int(totals[1]), "absent": absent})
    return result


def structure_functions(plotfile: str, fields, level: Optional[int] = None, region=None,
                        left_edge=None, right_edge=None, lags=None, max_order: int = 6,
                        periodic: bool = False, bins: Optional[int] = None, r_range=None,
                        r_log: bool = False, edges=None, min_level: int = 0, max_level: int = -1,
                        fill: Optional[float] = None, output: Optional[str] = None) -> dict:
    """Structure functions of a plotfile ("Structure functions"), on cuda:0: S_p(r) =
    <|v(x + r) - v(x)|^p> for p = 1 .. max_order (8 at the most) over every pair of cells of a
    region's covering grid that lies one of the lags apart.  fields: one name -- the moments of
    |dv| of that field, "scalar" -- or the three components (x, y, z) of a vector field -- the
    moments of the longitudinal increment |dv . r / r|, of the transverse one |dv - (dv . r) r /
    r^2| and of the magnitude |dv|; stored, derived, gradient, clump or grid fields.  level,
    region, left_edge / right_edge, min_level and max_level as api.covering_grid takes them; the
    region may have any size -- no power of two -- below 2^31 cells.  lags: integers [M, 3] in
    cells of `level`, by default structure.default_lags (13 directions times 1, 2, 3, 4, 6, 8,
    12, ... cells).  periodic: the region wraps around.  edges: n + 1 lengths, or bins and / or
    r_range = (r_min, r_max) with r_log for equal ratios (structure.make_edges); by default one
    bin per distinct lag length.  fill: what a cell without data counts as; with None such cells
    raise ValueError, with nan their pairs are left out and counted as nonfinite.  Returns a dict:
    level, lo, dims (nx, ny, nz), cell_size, fields, max_order, periodic; per lag lags int32 [M,
    3], r_lag [M] (physical length), pairs_lag int64 [M] and sums_lag float64 [M, K, max_order];
    per bin r [n], r_edges [n + 1] (with edges), pairs int64 [n] and S {kind: float64 [max_order,
    n]}, row p - 1 the moment of order p; outside and nonfinite (pairs that leave the region;
    pairs with a difference that is not finite) and absent (cells without data).  With output the
    dict is written as one .npz file (structure.save_npz)."""
    from . import structure
    names = [fields] if isinstance(fields, str) else [str(name) for name in fields]
    max_order, edges = _structure_arguments(len(names), max_order, edges, bins, r_range, r_log)
    if bins is None and r_range is None and r_log:
        raise ValueError("r_log needs bins or r_range")
    header, level, lo, dims = _plotfile_grid(plotfile, level, region, left_edge, right_edge,
                                             min_level, max_level, structure.check_dims)
    size = header.cell_size[level]
    lags = structure.check_lags(structure.default_lags(dims) if lags is None else lags, dims)
    if edges is None:
        edges = structure.make_edges(structure.lag_lengths(lags, size), bins, r_range,
                                     bool(r_log))
    ctx, rank, world, group, scenes, _ = _load_fields(plotfile, names, min_level, max_level)
    found = structure_function_scene(ctx, scenes,
                                     *_grid_arguments(header, scenes[0], level, lo, dims), lags,
                                     max_order, periodic, edges, fill, rank, world)
    result = {**_grid_head(header, level, lo, dims), "fields": tuple(names),
              "max_order": max_order, "periodic": bool(periodic), **found}
    if output:
        structure.save_npz(result, output)
    return result


# ---- inverse transform, Helmholtz split, potential -----------------------------------

# The device parts of the grid products whose results are grids: they return device tensors, so
# that helmholtz_scene, potential_scene and isolated_potential_scene (which copy them to the host)
# and the grid fields (which hand them to grid_scene) run the same steps.

def _helmholtz_spectra_device(ctx, fields, level, lo, dims, index, ratios, inverse_length, fill):
    """({part: three spectra}, absent): the covering grids of three native scenes, their
    transforms and the split into the solenoidal and the compressive part."""
    from . import spectra
    transformed, absent = [], 0
    for field in fields:
        values, absent = _covered_grid(field, level, lo, dims, index, ratios, fill)
        transformed.append(ctx.fft3d(values))
    return dict(zip(spectra.PARTS, ctx.helmholtz_split(*transformed, inverse_length))), absent


def _helmholtz_grids_device(ctx, parts, wanted):
    """({(part, component): grid}, the largest |imaginary part| as a 0-d tensor): the inverse
    transforms of the spectra `wanted` names, in that order, and of no other; a transformed
    spectrum is used up."""
    import torch
    worst = torch.zeros((), dtype=torch.float64, device=ctx.device)
    found = {}
    for part, component in wanted:
        real, imag = ctx.ifft3d(parts[part][component], with_imag=True)
        # torch.maximum lets a NaN through, as the largest |imag| of such a grid is
        worst = torch.maximum(worst, imag.abs().max())
        found[(part, component)] = real
    return found, worst


def _potential_device(ctx, field, level, lo, dims, index, ratios, inverse_length_sq, scale, fill):
    """(potential, the largest |imaginary part| as a 0-d tensor, absent) of a native scene."""
    values, absent = _covered_grid(field, level, lo, dims, index, ratios, fill)
    spectrum = ctx.inverse_laplacian(ctx.fft3d(values), inverse_length_sq, scale)
    real, imag = ctx.ifft3d(spectrum, with_imag=True)
    return real, imag.abs().max(), absent


def _isolated_potential_device(ctx, field, level, lo, dims, index, ratios, size, scale,
                               self_value, fill):
    """(potential, the largest |imaginary part| in the region as a 0-d tensor, absent) of a
    native scene, by the zero-padded convolution."""
    import torch
    from . import spectra
    padded, (nx, ny, nz) = spectra.padded_dims(dims), dims
    values, absent = _covered_grid(field, level, lo, dims, index, ratios, fill)
    # every tensor is dropped as soon as the next step has read it: at 512^3 the padded grids
    # would otherwise add up to some 70 GB
    grid = torch.zeros(padded[::-1], dtype=torch.float64, device=ctx.device)
    grid[:nz, :ny, :nx] = values
    del values
    spectrum = ctx.fft3d(grid)
    del grid
    green = ctx.isolated_green(padded, size, scale, self_value)
    kernel = ctx.fft3d(green)
    del green
    ctx.spectrum_multiply(spectrum, kernel)
    del kernel
    real, imag = ctx.ifft3d(spectrum, with_imag=True)
    del spectrum
    worst = imag[:nz, :ny, :nx].abs().max()
    del imag
    potential = real[:nz, :ny, :nx].contiguous()
    del real
    return potential, worst, absent


def helmholtz_scene(ctx, vx: "SceneGeometry", vy: "SceneGeometry", vz: "SceneGeometry",
                    level: int, lo, dims, cell_sizes, prob_lo, ref_ratio, edges=None,
                    fill: Optional[float] = None, grids: bool = True, rank: int = 0,
                    n_ranks: int = 1) -> dict:
    """The Helmholtz split of the velocity field (vx, vy, vz) -- three scenes over the same boxes
    -- on the periodic grid of the cells [lo, lo + dims) of level `level` ("Inverse
    transform, Helmholtz split, potential"): three covering grids, their transforms, the split
    into a solenoidal (divergence-free) and a compressive (curl-free) part per mode, the shell
    sums of the three solenoidal and of the three compressive spectra into two sets of bins and,
    with grids, the six inverse transforms, all on the device.  dims, edges and fill as
    power_spectrum_scene takes them, the other arguments as covering_grid_scene does.  Returns a
    dict: k_edges and k float64; power, spectrum and modes, dicts with "solenoidal" and
    "compressive" (spectra.normalise of the sums over the three components; modes int64 [n] counts
    a mode once per component) and, power and spectrum, "total", their sum; outside and nonfinite
    (summed over the six spectra); absent; with grids also solenoidal and compressive (three
    float64 [nz, ny, nx] numpy arrays each) and imag_max, the largest |imaginary part| the six
    inverses left.  With n_ranks > 1, or fewer local boxes than boxes, NotImplementedError is
    raised before any device work."""
    import numpy as np
    import torch
    from . import spectra
    level, lo, dims, size = _scene_grid_arguments(vx, level, lo, dims, cell_sizes, n_ranks,
                                                  "a Helmholtz split", spectra.check_dims)
    for other in (vy, vz):
        _require_one_rank(other, n_ranks, "a Helmholtz split needs every box of the scene on one "
                          "rank: cells are not gathered between ranks")
        if len(other.local_boxes) != len(vx.local_boxes):
            raise ValueError("vx, vy and vz must be scenes over the same boxes")
    k_edges = spectra.default_edges(dims, size) if edges is None else spectra.check_edges(edges)
    edges_sq = spectra.squared_edges(k_edges)
    g = spectra.inverse_length_sq(dims, size)
    h = spectra.inverse_length(dims, size)
    sizes, ratios, index = _level_setup(vx, vx.local_boxes, cell_sizes, prob_lo, ref_ratio)
    found = {}
    with _native_scenes(ctx, [vx, vy, vz]) as fields:
        parts, absent = _helmholtz_spectra_device(ctx, fields, level, lo, dims, index, ratios, h,
                                                  fill)
        binned = {}
        for part, three in parts.items():
            out = None
            for spectrum in three:
                out = ctx.spectrum_bins(spectrum, g, edges_sq, out)
            binned[part] = out
        if grids:
            wanted = [(part, c) for part in parts for c in range(3)]
            real, worst = _helmholtz_grids_device(ctx, parts, wanted)
            found = {part: [real[(part, c)] for c in range(3)] for part in parts}
        ctx.synchronize()
        binned = {part: tuple(t.cpu().numpy() for t in out) for part, out in binned.items()}
        if grids:
            found = {part: tuple(t.cpu().numpy() for t in three) for part, three in found.items()}
            found["imag_max"] = float(worst.item())
    result = {"k_edges": np.array(k_edges), "power": {}, "spectrum": {}, "modes": {}}
    outside = nonfinite = 0
    for part, out in binned.items():
        power, spectrum, result["k"], out_outside, out_nonfinite = \
            _shell_sums(out, dims, k_edges)
        result["power"][part], result["spectrum"][part], result["modes"][part] = \
            power, spectrum, out[0]
        outside, nonfinite = outside + out_outside, nonfinite + out_nonfinite
    for key in ("power", "spectrum"):
        result[key]["total"] = result[key]["solenoidal"] + result[key]["compressive"]
    result["compressive_fraction"] = spectra.compressive_fraction(
        result["power"]["solenoidal"], result["power"]["compressive"], k_edges)
    result["outside"], result["nonfinite"] = outside, nonfinite
    result["absent"] = absent
    result.update(found)
    return result


def helmholtz(plotfile: str, velocity: Sequence[str], level: Optional[int] = None, region=None,
              left_edge=None, right_edge=None, bins: Optional[int] = None, k_range=None,
              k_log: bool = False, edges=None, grids: bool = True, min_level: int = 0,
              max_level: int = -1, fill: Optional[float] = None,
              output: Optional[str] = None) -> dict:
    """The Helmholtz split of a plotfile's velocity field into its solenoidal and compressive
    parts ("Inverse transform, Helmholtz split, potential"), on cuda:0, over a
    periodic grid.  velocity: the names of the three components (x, y, z), stored, derived or
    gradient fields; every other argument as api.power_spectrum takes it.  Returns a dict: level,
    lo, dims (nx, ny, nz), cell_size, k_edges [n + 1], k [n]; power, spectrum and modes, dicts
    with "solenoidal" and "compressive" -- the kinetic-energy spectra of the two parts, the three
    components added, normalised as api.power_spectrum's -- and "total" (power and spectrum);
    compressive_fraction, sum(P_c) / (sum(P_c) + sum(P_s)) over the bins with a lower edge above
    0 (spectra.compressive_fraction); outside, nonfinite and absent; and with grids solenoidal
    and compressive, {name: float64 [nz, ny, nx]} with the components' names, and imag_max, the
    largest |imaginary part| the six inverse transforms left (rounding alone, unless cells are not
    finite).  With output the dict is written as one .npz file (spectra.save_helmholtz_npz)."""
    from . import spectra
    names = [velocity] if isinstance(velocity, str) else [str(name) for name in velocity]
    if len(names) != 3:
        raise ValueError("velocity must name three components")
    edges = _edge_arguments(edges, bins, k_range, k_log)
    header, level, lo, dims = _plotfile_grid(plotfile, level, region, left_edge, right_edge,
                                             min_level, max_level, spectra.check_dims)
    edges = _edge_arguments(edges, bins, k_range, k_log, (dims, header.cell_size[level]))
    ctx, rank, world, group, scenes, _ = _load_fields(plotfile, names, min_level, max_level)
    found = helmholtz_scene(ctx, *scenes, *_grid_arguments(header, scenes[0], level, lo, dims),
                            edges, fill, bool(grids), rank, world)
    result = _grid_head(header, level, lo, dims)
    result.update(found)
    for part in ("solenoidal", "compressive"):
        if part in found:
            result[part] = dict(zip(names, found[part]))
    if output:
        spectra.save_helmholtz_npz(result, output)
    return result


def potential_scene(ctx, scene: "SceneGeometry", level: int, lo, dims, cell_sizes, prob_lo,
                    ref_ratio, constant: float = 1.0, fill: Optional[float] = None,
                    rank: int = 0, n_ranks: int = 1) -> dict:
    """The periodic solution of laplace(phi) = constant (rho - mean rho) for a scene's raw field
    rho over the cells [lo, lo + dims) of level `level` ("Inverse transform,
    Helmholtz split, potential"): the covering grid, its transform, every mode times scale / q
    with scale = -(constant / (4 pi^2)) and q = sum_d m_d^2 / L_d^2 (the mean mode becomes 0) and
    the inverse transform, all on the device.  dims and fill as power_spectrum_scene takes them,
    the other arguments as covering_grid_scene does.  Returns a dict: potential float64
    [nz, ny, nx] (numpy), imag_max (the largest |imaginary part| the inverse left) and absent.
    With n_ranks > 1, or fewer local boxes than boxes, NotImplementedError is raised before any
    device work."""
    from . import spectra
    constant = float(constant)
    if not math.isfinite(constant):
        raise ValueError("constant must be finite")
    level, lo, dims, size = _scene_grid_arguments(scene, level, lo, dims, cell_sizes, n_ranks,
                                                  "a potential", spectra.check_dims)
    g = spectra.inverse_length_sq(dims, size)
    scale = -(constant / (4.0 * math.pi * math.pi))
    sizes, ratios, index = _level_setup(scene, scene.local_boxes, cell_sizes, prob_lo, ref_ratio)
    with _native_scenes(ctx, [scene]) as (field,):
        real, worst, absent = _potential_device(ctx, field, level, lo, dims, index, ratios, g,
                                                scale, fill)
        ctx.synchronize()
        return {"potential": real.cpu().numpy(), "imag_max": float(worst.item()),
                "absent": absent}


def potential(plotfile: str, variable: str = "", constant: float = 1.0,
              level: Optional[int] = None, region=None, left_edge=None, right_edge=None,
              min_level: int = 0, max_level: int = -1, fill: Optional[float] = None,
              output: Optional[str] = None) -> dict:
    """The periodic potential of a field of a plotfile ("Inverse transform,
    Helmholtz split, potential"), on cuda:0: phi with laplace(phi) = constant (rho - mean rho) on
    the covering grid of `variable` (by default the first variable) at `level` over a region with
    periodic boundaries -- constant = 4 pi G gives the gravitational potential of a density.
    level, region, left_edge / right_edge, min_level, max_level and fill as api.power_spectrum
    takes them.  Returns a dict: level, lo, dims (nx, ny, nz), cell_size, constant, potential
    float64 [nz, ny, nx], imag_max and absent.  With output the dict is written as one .npz file
    (spectra.save_potential_npz)."""
    from . import spectra
    constant = float(constant)
    if not math.isfinite(constant):
        raise ValueError("constant must be finite")
    header, level, lo, dims = _plotfile_grid(plotfile, level, region, left_edge, right_edge,
                                             min_level, max_level, spectra.check_dims)
    name = str(variable) or header.var_names[0]
    ctx, rank, world, group, scenes, _ = _load_fields(plotfile, [name], min_level, max_level)
    found = potential_scene(ctx, scenes[0], *_grid_arguments(header, scenes[0], level, lo, dims),
                            constant, fill, rank, world)
    result = {**_grid_head(header, level, lo, dims), "constant": constant}
    result.update(found)
    if output:
        spectra.save_potential_npz(result, output)
    return result


# ---- isolated potential ("Isolated potential") ---------------------------------------

def _isolated_constants(constant, self_term) -> Tuple[float, float]:
    constant, self_term = float(constant), float(self_term)
    if not math.isfinite(constant):
        raise ValueError("constant must be finite")
    if not (math.isfinite(self_term) and self_term >= 0.0):
        raise ValueError("self_term must be finite and not negative")
    return constant, self_term


def _isolated_scale(constant: float, self_term: float, size) -> Tuple[float, float]:
    """(scale, G(0)) of the isolated Green's function on cells of `size`."""
    volume = (size[0] * size[1]) * size[2]
    scale = -((constant * volume) / (4.0 * math.pi))
    return scale, scale * self_term


def isolated_potential_scene(ctx, scene: "SceneGeometry", level: int, lo, dims, cell_sizes,
                             prob_lo, ref_ratio, constant: float = 1.0, self_term: float = 0.0,
                             fill: Optional[float] = None, rank: int = 0,
                             n_ranks: int = 1) -> dict:
    """The free-space solution of laplace(phi) = constant rho for a scene's raw field rho over the
    cells [lo, lo + dims) of level `level`, nothing outside them ("Isolated
    potential"): phi_i = sum_j G(x_i - x_j) rho_j with G = scale / r, scale = -(constant dx dy dz
    / (4 pi)), and G(0) = scale * self_term, by Hockney and Eastwood's zero-padded convolution --
    the covering grid, padded with zeros to spectra.padded_dims(dims), its transform, the
    transform of the Green's grid, their product, the inverse transform and the region's corner
    of it, all on the device.  dims: between 1 and 512 cells per axis, powers of two or not; fill
    as power_spectrum_scene takes it, the other arguments as covering_grid_scene does.  Returns a
    dict: potential float64 [nz, ny, nx] (numpy), imag_max (the largest |imaginary part| the
    inverse left in the region), absent and padded_dims.  With n_ranks > 1, or fewer local boxes
    than boxes, NotImplementedError is raised before any device work."""
    import torch
    from . import spectra
    constant, self_term = _isolated_constants(constant, self_term)
    level, lo, dims, size = _scene_grid_arguments(scene, level, lo, dims, cell_sizes, n_ranks,
                                                  "an isolated potential",
                                                  spectra.check_isolated_dims)
    padded = spectra.padded_dims(dims)
    scale, self_value = _isolated_scale(constant, self_term, size)
    sizes, ratios, index = _level_setup(scene, scene.local_boxes, cell_sizes, prob_lo, ref_ratio)
    with _native_scenes(ctx, [scene]) as (field,):
        potential, worst, absent = _isolated_potential_device(
            ctx, field, level, lo, dims, index, ratios, size, scale, self_value, fill)
        ctx.synchronize()
        return {"potential": potential.cpu().numpy(), "imag_max": float(worst.item()),
                "absent": absent, "padded_dims": padded}


def isolated_potential(plotfile: str, variable: str = "", constant: float = 1.0,
                       level: Optional[int] = None, region=None, left_edge=None, right_edge=None,
                       self_term: float = 0.0, min_level: int = 0, max_level: int = -1,
                       fill: Optional[float] = None, output: Optional[str] = None) -> dict:
    """The potential of a field of a plotfile with isolated (open) boundaries (DESIGN.md 7,
    "Isolated potential"), on cuda:0: phi with laplace(phi) = constant rho for the covering grid
    rho of `variable` (by default the first variable) at `level` over a region, with nothing
    outside the region and phi -> 0 far from it -- constant = 4 pi G gives the gravitational
    potential of a density.  phi_i = sum_j G_ij rho_j with G_ij = -(constant dx dy dz / (4 pi)) /
    |x_i - x_j| between cell centres; self_term (1 / length, >= 0, by default 0) stands for
    1 / |x_i - x_i|, a cell's share in its own potential: with 0 every cell is a point mass that
    does not act on itself, and 0.5 sum_i m_i phi_i is clump binding's pairwise sum.  The region
    holds between 1 and 512 cells along every axis, powers of two or not; level, region,
    left_edge / right_edge, min_level, max_level and fill as api.potential takes them.  Returns a
    dict: level, lo, dims (nx, ny, nz), padded_dims, cell_size, constant, self_term, potential
    float64 [nz, ny, nx], imag_max and absent.  With output the dict is written as one .npz file
    (spectra.save_isolated_potential_npz)."""
    from . import spectra
    constant, self_term = _isolated_constants(constant, self_term)
    header, level, lo, dims = _plotfile_grid(plotfile, level, region, left_edge, right_edge,
                                             min_level, max_level, spectra.check_isolated_dims)
    name = str(variable) or header.var_names[0]
    ctx, rank, world, group, scenes, _ = _load_fields(plotfile, [name], min_level, max_level)
    found = isolated_potential_scene(ctx, scenes[0],
                                     *_grid_arguments(header, scenes[0], level, lo, dims),
                                     constant, self_term, fill, rank, world)
    result = {**_grid_head(header, level, lo, dims, padded_dims=found["padded_dims"]),
              "constant": constant, "self_term": self_term}
    result.update(found)
    if output:
        spectra.save_isolated_potential_npz(result, output)
    return result


# ---- rays ("Rays") ---------------------------------------------------------------------

def ray_scene(ctx, scene: "SceneGeometry", start, end, cell_sizes, prob_lo, ref_ratio,
              max_trips: Optional[int] = None, rank: int = 0, n_ranks: int = 1) -> dict:
    """The leaf cells of a scene's raw field that the segments start[s] -> end[s] cross, in order
    ("Rays"; yt's ds.ray).  start, end: [n, 3] in the plotfile's physical units;
    scene, cell_sizes, prob_lo and ref_ratio as gradient_scene takes them.  max_trips bounds the
    cells one ray walks; by default 8 + 2 sum_d (Bhi[d] - Blo[d] + 1) (r_0 ... r_(L - 2)), twice the
    planes of the finest level across the scene's level-0 bounding box, 2^30 at the most.  Returns
    a dict of numpy arrays: per ray offsets int64 [n + 1], status uint8 [n] (0 complete, 1 the
    ray misses, 2 max_trips reached, 3 an end point is not finite or start == end), t_enter and
    t_leave float64 [n] (NaN for status 1 and 3), integral and covered float64 [n] (sum value ds
    over the leaf segments with a finite value, sum ds over the leaf segments); per segment,
    packed by ray at offsets[s], t0, t1 float64, level int8 (-1 where no loaded leaf holds the
    stretch) and value float64 (the leaf's raw value, NaN at level -1).  One call counts,
    torch.cumsum gives the offsets, a second call emits.  Every box of the scene must be on this
    rank: with n_ranks > 1, or fewer local boxes than boxes, NotImplementedError is raised before
    any device work."""
    import numpy as np
    import torch
    from . import rays as ray_rules
    local = list(scene.local_boxes)
    _require_one_rank(scene, n_ranks, "rays need every box of the scene on one rank: "
                      "rays are not handed over between ranks")
    first, last = ray_rules.end_points(start, end)
    if first.shape[0] >= 2 ** 32:
        raise ValueError("the number of rays must stay below 2^32")
    sizes, ratios, index = _level_setup(scene, local, cell_sizes, prob_lo, ref_ratio)
    if max_trips is None:
        bounds = ray_rules.level0_bounds(index, [b.cell_dimensions for b in local],
                                         [b.level for b in local], ratios)
        max_trips = ray_rules.default_max_trips(bounds, ratios, len(sizes))
    max_trips = int(max_trips)
    if not 1 <= max_trips <= ray_rules.MAX_TRIPS:
        raise ValueError("max_trips must lie in [1, 2^30]")
    origin = [float(v) for v in prob_lo]
    n = first.shape[0]
    with _native_scenes(ctx, [scene]) as (field,):
        a = torch.from_numpy(first).to(ctx.device)
        b = torch.from_numpy(last).to(ctx.device)
        arguments = (a, b, max_trips, index, ratios, sizes, origin)
        counts, status, span = field.rays(*arguments)
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=ctx.device)
        torch.cumsum(counts.to(torch.int64), 0, out=offsets[1:])
        ctx.synchronize()
        total = int(offsets[-1].item())
        segments = [np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.float64),
                    np.zeros(0, dtype=np.int8), np.zeros(0, dtype=np.float64)]
        integral, covered = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        if total > 0:
            emitted = field.rays(*arguments, offsets=offsets, n_segments=total)
            ctx.synchronize()
            *segments, integral, covered = (t.cpu().numpy() for t in emitted)
        status, span = status.cpu().numpy(), span.cpu().numpy()
        offsets = offsets.cpu().numpy()
    t0, t1, level, value = segments
    return {"offsets": offsets, "status": status, "t_enter": span[:, 0].copy(),
            "t_leave": span[:, 1].copy(), "integral": integral, "covered": covered,
            "t0": t0, "t1": t1, "level": level, "value": value}


def rays(plotfile: str, start, end, fields: Sequence[str] = (), min_level: int = 0,
         max_level: int = -1, max_trips: Optional[int] = None,
         output: Optional[str] = None) -> dict:
    """Line-outs of a plotfile (yt's ds.ray / LinePlot; DESIGN.md 7, "Rays"), on cuda:0: for every
    segment start[s] -> end[s] ([n, 3] each, or a single [3] each; the plotfile's physical units)
    the uncovered cells of the loaded levels that it crosses, in order, and the exact column
    integral sum value ds of every field along it.  fields: stored variables or registered
    derived, gradient, clump or grid fields; by default the plotfile's first variable.  Returns a dict:
    per ray n, start and end float64 [n, 3], offsets int64 [n + 1], status uint8 [n] (0 complete,
    1 the ray misses the data's bounding box, 2 max_trips reached, 3 an end point is not finite or
    start == end), t_enter and t_leave float64 [n] (the part of the segment inside the bounding
    box as parameters in [0, 1]; NaN for status 1 and 3), length float64 [n] (|end - start|) and
    covered_length float64 [n] (the length inside loaded leaves); per segment, packed by ray at
    offsets[s], t0, t1 float64 and level int8 (-1 for a stretch no loaded leaf holds, as min_level
    or a missing grid leaves them); per field fields {name: float64 [total]} (the leaf's raw
    value, NaN at level -1) and integrals {name: float64 [n]} (over the segments whose value is
    finite).  max_trips as ray_scene takes it.  With output the dict is written as one .npz file
    (rays.save_npz)."""
    import numpy as np
    from . import plotfile as pf
    from . import rays as ray_rules
    first, last = ray_rules.end_points(start, end)
    _require_plotfile(plotfile)
    header = pf.PlotFileData(plotfile)
    names = [str(name) for name in fields] or [header.var_names[0]]
    ctx, rank, world, group, scenes, volumes = _load_fields(plotfile, names, min_level, max_level)
    n_levels = len(volumes)
    arguments = (first, last, *_header_levels(header, n_levels), max_trips, rank, world)
    geometry, values, integrals = None, {}, {}
    for name, scene in zip(names, scenes):
        found = ray_scene(ctx, scene, *arguments)
        values[name], integrals[name] = found.pop("value"), found.pop("integral")
        if geometry is None:
            geometry = found
        else:
            # the cells crossed depend on the boxes alone, not on the field's values
            for key, array in geometry.items():
                if array.shape != found[key].shape or array.tobytes() != found[key].tobytes():
                    raise RuntimeError(f"rays: field '{name}' was walked through other cells "
                                       f"({key} differs)")
    with np.errstate(all="ignore"):
        d = last - first
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    result = {"n": int(first.shape[0]), "start": first, "end": last,
              "offsets": geometry["offsets"], "status": geometry["status"],
              "t_enter": geometry["t_enter"], "t_leave": geometry["t_leave"], "length": length,
              "covered_length": geometry["covered"], "t0": geometry["t0"], "t1": geometry["t1"],
              "level": geometry["level"], "fields": values, "integrals": integrals}
    if output:
        ray_rules.save_npz(result, output)
    return result


def ray_sums_scene(ctx, scene: "SceneGeometry", start, end, cell_sizes, prob_lo, ref_ratio,
                   weight_scene: Optional["SceneGeometry"] = None,
                   max_trips: Optional[int] = None, rank: int = 0, n_ranks: int = 1) -> dict:
    """The exact column of every segment start[s] -> end[s] through a scene's raw field, in one
    walk and with nothing stored per segment ("Off-axis projection").  The arguments
    are ray_scene's; weight_scene: a scene with the same boxes (another variable of the plotfile
    at the same levels, or a computed field of it), or None.  Returns a dict of numpy arrays per
    ray: count uint32 (the segments ray_scene would list), status uint8, t_enter and t_leave
    float64 as ray_scene gives them, and float64 sums over the leaf segments in walk order, w
    being a segment's length: covered = sum w; without weight_scene integral = sum v w and
    counted = sum w over the finite values v, weight is None; with it integral = sum (v q) w,
    weight = sum q w and counted = sum w where v and the weight's value q are both finite.  Every
    box of the scene must be on this rank, as for ray_scene."""
    import numpy as np
    import torch
    from . import rays as ray_rules
    local = list(scene.local_boxes)
    _require_one_rank(scene, n_ranks, "rays need every box of the scene on one rank: "
                      "rays are not handed over between ranks")
    first, last = ray_rules.end_points(start, end)
    if first.shape[0] >= 2 ** 32:
        raise ValueError("the number of rays must stay below 2^32")
    sizes, ratios, index = _level_setup(scene, local, cell_sizes, prob_lo, ref_ratio)
    if max_trips is None:
        bounds = ray_rules.level0_bounds(index, [b.cell_dimensions for b in local],
                                         [b.level for b in local], ratios)
        max_trips = ray_rules.default_max_trips(bounds, ratios, len(sizes))
    max_trips = int(max_trips)
    if not 1 <= max_trips <= ray_rules.MAX_TRIPS:
        raise ValueError("max_trips must lie in [1, 2^30]")
    origin = [float(v) for v in prob_lo]
    with _native_scenes(ctx, [scene, weight_scene]) as (field, weight):
        a = torch.from_numpy(first).to(ctx.device)
        b = torch.from_numpy(last).to(ctx.device)
        found = field.ray_sums(a, b, max_trips, index, ratios, sizes, origin, weight)
        ctx.synchronize()
        counts, status, span, integral, weight_sum, counted, covered = (
            t if t is None else t.cpu().numpy() for t in found)
    return {"count": counts.view(np.uint32), "status": status, "t_enter": span[:, 0].copy(),
            "t_leave": span[:, 1].copy(), "integral": integral, "weight": weight_sum,
            "counted": counted, "covered": covered}


def _load_variable_scenes(ctx, plotfile: str, names, min_level: int, max_level: int,
                          log_scale_input: bool, normalize_to_data_range: bool, rank: int,
                          n_ranks: int, process_group) -> list:
    """One scene per variable name, for every plotfile-level function.  A registered clump field
    is resolved like a gradient field (its input raw, clump_scene applies the caller's flags).  A
    name that is neither a registered derived field nor a registered gradient field goes to
    plotfile.load_plotfile_geometry as it always did.  A derived field is compiled, its fields are
    resolved raw (the plotfile's first variable if it reads none) and derive_scene applies the
    caller's flags.  A gradient field's input is resolved raw and gradient_scene applies the
    caller's flags.  A registered grid field's inputs (gridfields.py: a potential's source, a
    Helmholtz field's three components, nothing for an array) are resolved raw, its grid is
    computed on the device and grid_scene writes it onto their boxes with the caller's flags; the
    grid fields of one call share what they have in common (_grid_product_device).  A registered
    particle field (particles.py) has no inputs: its positions and values go to the device once
    per call and deposit_scene puts them onto the boxes of the plotfile's first variable with the
    caller's flags.  Resolution is
    recursive -- a derived field may read gradient or grid fields, a gradient field may take a
    derived or another gradient field, a potential a derived density -- and every name is loaded
    or computed once per call and pair of flags, however many names need it."""
    from . import clumps as clump_rules
    from . import derive, gradient, gridfields, particles
    from . import plotfile as pf
    registered = derive.derived_fields()
    gradients = gradient.gradient_fields()
    clump_names = clump_rules.clump_fields()
    grid_names = gridfields.grid_fields()
    particle_names = particles.particle_fields()
    particle_arrays = {}   # name -> (positions, values) on the device
    resolved = {}
    shared_grids = {}      # what the grid fields of this call share: spectra and grids by product
    header = []

    def plotfile_header():
        if not header:
            header.append(pf.PlotFileData(plotfile))
        return header[0]

    def resolve(name, log, normalize):
        key = (name, bool(log), bool(normalize))
        if key in resolved:
            return resolved[key]
        if name in gradients:
            of, axis = gradients[name]
            _check_variable(plotfile, plotfile_header(), of, f"gradient field '{name}'")
            inner = resolve(of, False, True)
            finest = max(int(b.level) for b in inner.all_boxes)
            scene = gradient_scene(ctx, inner, axis, *_header_levels(plotfile_header(), finest + 1),
                                   rank, n_ranks, process_group, log, normalize)
        elif name in clump_names:
            of, lower, upper = clump_names[name]
            _check_variable(plotfile, plotfile_header(), of, f"clump field '{name}'")
            inner = resolve(of, False, True)
            finest = max(int(b.level) for b in inner.all_boxes)
            scene, _ = clump_scene(ctx, inner, lower, upper,
                                   *_header_levels(plotfile_header(), finest + 1), rank, n_ranks,
                                   process_group, log, normalize)
        elif name in grid_names:
            entry = grid_names[name]
            for of in gridfields.inputs_of(name):
                _check_variable(plotfile, plotfile_header(), of, f"grid field '{name}'")
            # the first input, or the plotfile's first variable, gives the boxes
            inputs = [resolve(of, False, True) for of in gridfields.inputs_of(name)]
            geometry = inputs[0] if inputs else resolve("", False, True)
            scene = _grid_field_scene(ctx, plotfile, entry, inputs, geometry, shared_grids,
                                      min_level, max_level, rank, n_ranks, process_group, log,
                                      normalize)
        elif name in particle_names:
            # the plotfile's first variable gives the boxes, as for an array grid field; the
            # positions and values go to the device once per call
            entry = particle_names[name]
            geometry = resolve("", False, True)
            if name not in particle_arrays:
                import torch
                particle_arrays[name] = tuple(
                    None if a is None else torch.from_numpy(a).to(ctx.device)
                    for a in (entry["positions"], entry["values"]))
            finest = max(int(b.level) for b in geometry.all_boxes)
            scene, _, _ = deposit_scene(ctx, geometry, *particle_arrays[name],
                                        *_header_levels(plotfile_header(), finest + 1),
                                        entry["method"], entry["quantity"], rank, n_ranks,
                                        process_group, log, normalize)
        elif name in registered:
            program = derive.compile_field(name)
            _check_derived_inputs(plotfile, plotfile_header(), name, program)
            inputs = [resolve(field, False, True) for field in program.fields]
            geometry = inputs[0] if inputs else resolve("", False, True)
            finest = max(int(b.level) for b in geometry.all_boxes)
            scene = derive_scene(ctx, program, inputs, geometry,
                                 plotfile_header().cell_size[:finest + 1], rank, n_ranks,
                                 process_group, log, normalize)
        else:
            scene = pf.load_plotfile_geometry(ctx, plotfile, name, min_level, max_level, log,
                                              normalize, rank, n_ranks, process_group)
        resolved[key] = scene
        return scene

    return [resolve(name, log_scale_input, normalize_to_data_range) for name in names]


def _check_variable(plotfile: str, header, name: str, needed_by: str = "") -> None:
    """RuntimeError unless `name` is a stored variable of the plotfile or a registered derived,
    gradient, clump or grid field whose own inputs are."""
    from . import clumps as clump_rules
    from . import derive, gradient, gridfields, particles
    gradients = gradient.gradient_fields()
    clump_names = clump_rules.clump_fields()
    if name in particles.particle_fields():
        return                         # made of the caller's arrays: nothing of the plotfile's
    if name in gridfields.grid_fields():
        for of in gridfields.inputs_of(name):
            _check_variable(plotfile, header, of, f"grid field '{name}'")
    elif name in gradients:
        _check_variable(plotfile, header, gradients[name][0], f"gradient field '{name}'")
    elif name in clump_names:
        _check_variable(plotfile, header, clump_names[name][0], f"clump field '{name}'")
    elif name in derive.derived_fields():
        _check_derived_inputs(plotfile, header, name, derive.compile_field(name))
    elif name not in header.var_names:
        why = f" (needed by {needed_by})" if needed_by else ""
        raise RuntimeError(f"Variable '{name}'{why} not found in plotfile '{plotfile}'.")


def _check_derived_inputs(plotfile: str, header, name: str, program: DerivedProgram) -> None:
    for field in program.fields:
        _check_variable(plotfile, header, field, f"derived field '{name}'")


def compute_histogram(plotfile: str, variable: Optional[str] = None, min_level: int = 0,
                      max_level: int = -1, log_scale: bool = False, bins: int = 256, ctx=None,
                      rank: int = 0, n_ranks: int = 1, process_group=None) -> dict:
    """The reference python module's compute_histogram (module.cpp:304-356, same keyword names
    and defaults; VolumeRenderer::computeScalarHistogram, VolumeRenderer.cpp:880-897): load the
    plotfile with normalisation to the data range, then bin every uncovered cell."""
    from . import plotfile as pf
    from . import runtime
    if bins <= 0:
        raise ValueError("binCount must be positive")
    if ctx is None:
        ctx, rank, n_ranks, process_group = _runtime_scope()
    scene = _load_variable_scenes(ctx, plotfile, [variable or ""], min_level, max_level,
                                  log_scale, True, rank, n_ranks, process_group)[0]
    return compute_scene_histogram(ctx, scene.all_boxes, scene.local_boxes, log_scale, bins,
                                   process_group, n_ranks)


def compute_scene_histogram(ctx, all_boxes: Sequence[AmrBox], local_boxes: Sequence[AmrBox],
                            log_scale: bool = False, bins: int = 256, process_group=None,
                            n_ranks: int = 1) -> dict:
    """api::ComputeHistogram (VolumeRendererApi.cpp:397-413) for boxes already in HBM: scene statistics with
    normalisation to the data range, then the 64-bit bin counts of every cell
    (ComputeSceneHistogram, SceneBuilder.cpp:445-577).  Returns the module's dict keys."""
    import torch
    import torch.distributed as dist
    from . import runtime
    if bins <= 0:
        raise ValueError("binCount must be positive")
    scene = ctx.create_scene(local_boxes, ScalarTransform())
    lo, hi, lo_pos, finite = scene.scalar_stats()
    stage = n_ranks > 1 and dist.get_backend(process_group) != "nccl"
    if n_ranks > 1:
        device = "cpu" if stage else ctx.device
        mins = torch.tensor([lo, lo_pos], dtype=torch.float64, device=device)
        maxs = torch.tensor([hi], dtype=torch.float64, device=device)
        count = torch.tensor([finite], dtype=torch.int64, device=device)
        dist.all_reduce(mins, op=dist.ReduceOp.MIN, group=process_group)
        dist.all_reduce(maxs, op=dist.ReduceOp.MAX, group=process_group)
        dist.all_reduce(count, op=dist.ReduceOp.SUM, group=process_group)
        lo, lo_pos, hi, finite = mins[0].item(), mins[1].item(), maxs[0].item(), int(count.item())
    transform, processed_range, scalar_range = runtime.scene_transform_from_stats(
        (lo, hi, lo_pos), finite, log_scale, True)
    original = (lo, hi if hi != lo else lo + 1.0)
    counts = scene.histogram(transform, scalar_range[0], scalar_range[1], bins)
    if n_ranks > 1:
        if stage:
            host = counts.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=process_group)
            counts = host
        else:
            dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=process_group)
    ctx.synchronize()
    host_counts = counts.cpu().numpy().astype("uint64")
    samples = int(host_counts.sum())
    if samples == 0:
        host_counts[:] = 0
    return {"counts": host_counts, "normalized_range": scalar_range,
            "processed_range": processed_range,
            "original_range": (float(__import__("numpy").float32(original[0])),
                               float(__import__("numpy").float32(original[1]))),
            "samples": samples}


def _finite(values) -> bool:
    return all(math.isfinite(float(v)) for v in values)


def validate_mode(options: RenderOptions) -> None:
    """RenderOptions.mode: one of RENDER_MODES; a max_intensity frame has no antialiasing."""
    if options.mode not in RENDER_MODES:
        raise ValueError(f"mode must be one of {', '.join(RENDER_MODES)}, not {options.mode!r}")
    if options.mode == "max_intensity" and options.antialiasing != 1:
        raise ValueError("max_intensity frames have no antialiasing (antialiasing must be 1)")


def validate_options(options: RenderOptions) -> None:
    """The argument checks of api::Render (VolumeRendererApi.cpp:150-255, 257-274), and of the
    render mode."""
    validate_mode(options)
    if not options.output_filename:
        raise ValueError("output filename must not be empty")
    if options.min_level < 0:
        raise ValueError("min level must be non-negative")
    if options.max_level < -1:
        raise ValueError("max level must be non-negative or -1 for all levels")
    if options.max_level >= 0 and options.min_level > options.max_level:
        raise RuntimeError("min level must not exceed max level")
    if options.up_vector is not None:
        if len(options.up_vector) != 3 or not _finite(options.up_vector) or \
                math.sqrt(sum(float(v) ** 2 for v in options.up_vector)) <= 0.0:
            raise ValueError("up_vector must be a finite, non-zero 3-vector")
    if options.scalar_range is not None:
        lo, hi = options.scalar_range
        if not _finite((lo, hi)) or not (lo < hi):
            raise ValueError("scalar_range must contain two values with min < max.")
    if options.color_map is not None:  # validateColorMap (VolumeRendererApi.cpp:163-196)
        if len(options.color_map) < 2:
            raise ValueError("color map must provide at least two control points")
        previous = -math.inf
        for p in options.color_map:
            vals = (p.value, p.red, p.green, p.blue, p.alpha) if isinstance(
                p, ColorMapControlPoint) else tuple(p)
            if len(vals) != 5:
                raise ValueError("color_map entries are (value, red, green, blue, alpha)")
            if not math.isfinite(float(vals[0])):
                raise ValueError("color map control point values must be finite")
            if float(vals[0]) <= previous:
                raise ValueError("color map control point values must be strictly increasing")
            previous = float(vals[0])
            for name, component in zip(("red", "green", "blue", "alpha"), vals[1:]):
                if not math.isfinite(float(component)) or not (0.0 <= float(component) <= 1.0):
                    raise ValueError(f"color map {name} components must be finite and within "
                                     "[0, 1]")
    if options.camera is not None:
        cam = options.camera
        if not _finite(cam.eye) or not _finite(cam.look_at) or not _finite(cam.up):
            raise ValueError("camera vectors must be finite")
        forward = [float(cam.look_at[a]) - float(cam.eye[a]) for a in range(3)]
        if not math.sqrt(sum(v * v for v in forward)) > 0.0:
            raise ValueError("camera eye and look-at must be distinct")
        up = [float(v) for v in cam.up]
        if not math.sqrt(sum(v * v for v in up)) > 0.0:
            raise ValueError("camera up vector must be non-zero")
        cross = (forward[1] * up[2] - forward[2] * up[1], forward[2] * up[0] - forward[0] * up[2],
                 forward[0] * up[1] - forward[1] * up[0])
        if not math.sqrt(sum(v * v for v in cross)) > 1e-6:
            raise ValueError("camera up vector must not be parallel to the view direction")
        if not (0.0 < cam.fov_y_degrees < 180.0):
            raise ValueError("camera_fov_y must be in (0, 180) degrees")
        if not (cam.near_plane > 0.0 and cam.far_plane > cam.near_plane):
            raise ValueError("camera near/far planes must satisfy 0 < near < far")


def save_ppm(rgb8, filename: str) -> bool:
    """SavePPM (Common/SavePPM.cpp:17-36): binary P6, rows already top-down in `rgb8`."""
    height, width = int(rgb8.shape[0]), int(rgb8.shape[1])
    data = rgb8.cpu().numpy().tobytes() if hasattr(rgb8, "cpu") else bytes(rgb8)
    with open(filename, "wb") as fh:
        fh.write(f"P6\n{width} {height}\n255\n".encode("ascii"))
        fh.write(data)
    return True


def save_png(rgb8, filename: str) -> bool:
    """SavePNG (Common/SavePNG.cpp:24-81): 8-bit RGB, non-interlaced, rows top-down -- the same
    pixel bytes as the PPM.  The reference hands the rows to libpng; the compressed stream
    depends on libpng's filter heuristics and zlib's settings, so parity is on the decoded
    pixels, not the file bytes.  Rows are stored with filter type 0 (None)."""
    import struct
    import zlib
    height, width = int(rgb8.shape[0]), int(rgb8.shape[1])
    rows = rgb8.cpu().numpy() if hasattr(rgb8, "cpu") else rgb8
    raw = b"".join(b"\x00" + rows[y].tobytes() for y in range(height))

    def chunk(tag: bytes, payload: bytes) -> bytes:
        return (struct.pack(">I", len(payload)) + tag + payload
                + struct.pack(">I", zlib.crc32(tag + payload) & 0xFFFFFFFF))

    try:
        with open(filename, "wb") as fh:
            fh.write(b"\x89PNG\r\n\x1a\n")
            fh.write(chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)))
            fh.write(chunk(b"IDAT", zlib.compress(raw, 6)))
            fh.write(chunk(b"IEND", b""))
    except OSError:
        return False
    return True


def _libm_float(name: str):
    """float f(float) of the host libm (std::sin / cos / tan / log on a float argument)."""
    import ctypes
    import ctypes.util
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    fn = getattr(lib, name)
    fn.restype = ctypes.c_float
    fn.argtypes = [ctypes.c_float]
    return lambda x: fn(float(x))


_runtime = {"refs": 0, "ctx": None, "owns_group": False}


def _ensure_runtime() -> None:
    """ensure_runtime_initialized (module.cpp:35-66): the rendering context on the local GPU and,
    when launched with one process per GPU (WORLD_SIZE > 1), the RCCL process group."""
    from . import runtime
    import torch
    if _runtime["ctx"] is None:
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        world = int(os.environ.get("WORLD_SIZE", "1"))
        torch.cuda.set_device(local_rank)
        if world > 1:
            import torch.distributed as dist
            if not dist.is_initialized():
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
                _runtime["owns_group"] = True
        _runtime["ctx"] = runtime.Context(local_rank)


def initialize_runtime() -> None:
    """amrVolumeRenderer.initialize_runtime (module.cpp:103-107): set the process up once ahead
    of several render() / compute_histogram() calls (reference counted)."""
    _ensure_runtime()
    _runtime["refs"] += 1


def finalize_runtime() -> None:
    """amrVolumeRenderer.finalize_runtime (module.cpp:109-119)."""
    if _runtime["refs"] == 0:
        raise RuntimeError("amrVolumeRenderer.finalize_runtime requires a matching "
                           "initialize_runtime call")
    _runtime["refs"] -= 1
    if _runtime["refs"] == 0:
        if _runtime["ctx"] is not None:
            _runtime["ctx"].close()
            _runtime["ctx"] = None
        if _runtime["owns_group"]:
            import torch.distributed as dist
            dist.destroy_process_group()
            _runtime["owns_group"] = False


def _runtime_scope():
    """(context, rank, world size, process group) of the runtime.  Like the reference's
    RuntimeScope (module.cpp:86-101) a call without a prior initialize_runtime() initialises on
    demand -- honouring LOCAL_RANK / RANK / WORLD_SIZE, so that under a one-process-per-GPU
    launcher every process renders its own share on its own GPU.  Unlike the reference's scope
    (which finalises MPI on exit when no manual reference is held, after which nothing can be
    initialised again) the on-demand runtime stays until finalize_runtime drops the last manual
    reference or the process ends."""
    _ensure_runtime()
    rank, world, group = 0, 1, None
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        rank, world, group = dist.get_rank(), dist.get_world_size(), dist.group.WORLD
    elif int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError("WORLD_SIZE > 1 but no process group could be initialised")
    return _runtime["ctx"], rank, world, group


class _Mt19937:
    """std::mt19937 (the 32-bit Mersenne Twister of the C++ standard, [rand.predef])."""

    def __init__(self, seed: int):
        self.state = [0] * 624
        self.state[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            prev = self.state[i - 1]
            self.state[i] = (1812433253 * (prev ^ (prev >> 30)) + i) & 0xFFFFFFFF
        self.index = 624

    def __call__(self) -> int:
        if self.index >= 624:
            st = self.state
            for i in range(624):
                y = (st[i] & 0x80000000) | (st[(i + 1) % 624] & 0x7FFFFFFF)
                st[i] = st[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.index = 0
        y = self.state[self.index]
        self.index += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


def _uniform_float(rng: _Mt19937, a, b):
    """libstdc++'s std::uniform_real_distribution<float>(a, b)(mt19937): generate_canonical
    takes one 32-bit draw, converts it to float, divides by 2^32 and steps a result of 1.0 down
    to the float below; then canonical * (b - a) + a, all in float."""
    import numpy as np
    f32 = np.float32
    canonical = f32(f32(rng()) / f32(4294967296.0))
    if canonical >= f32(1.0):
        canonical = np.nextafter(f32(1.0), f32(0.0))
    return f32(f32(canonical * f32(f32(b) - f32(a))) + f32(a))


def automatic_camera(bounds: VolumeBounds, camera_seed: int = 91021,
                     up_vector: Optional[Sequence[float]] = None) -> CameraParameters:
    """The camera renderScene places when none is given (VolumeRenderer.cpp:974-1023): on a
    sphere around the bounds' centre, azimuth and altitude drawn from std::mt19937(cameraSeed).
    Float arithmetic and the host libm's sin / cos / tan as in the reference's host code."""
    import numpy as np
    f32 = np.float32
    k_pi = f32(3.14159265358979323846)
    k_two_pi = f32(f32(2.0) * k_pi)
    # amrex::RealVect is double: 0.5f * (min + max) promotes to double
    center = [0.5 * (bounds.min_corner[a] + bounds.max_corner[a]) for a in range(3)]
    half = [0.5 * (bounds.max_corner[a] - bounds.min_corner[a]) for a in range(3)]
    radius = f32(math.sqrt(half[0] * half[0] + half[1] * half[1] + half[2] * half[2]))
    if radius <= f32(0.0):
        radius = f32(1.0)
    fov_y = f32(k_pi * f32(0.25))
    max_altitude = f32(k_pi * f32(0.25))
    half_fov = f32(fov_y * f32(0.5))
    sinf, cosf, tanf = _libm_float("sinf"), _libm_float("cosf"), _libm_float("tanf")
    min_distance = f32(radius / f32(tanf(half_fov))) if half_fov > 0 else radius
    safety = max(f32(f32(0.25) * radius), f32(0.5))
    distance = f32(min_distance + safety)
    rng = _Mt19937(camera_seed)
    azimuth = _uniform_float(rng, f32(0.0), k_two_pi)
    altitude = _uniform_float(rng, -max_altitude, max_altitude)
    cos_altitude, sin_altitude = f32(cosf(altitude)), f32(sinf(altitude))
    sin_azimuth, cos_azimuth = f32(sinf(azimuth)), f32(cosf(azimuth))
    eye = (center[0] + float(f32(f32(distance * cos_altitude) * sin_azimuth)),
           center[1] + float(f32(distance * sin_altitude)),
           center[2] + float(f32(f32(distance * cos_altitude) * cos_azimuth)))

    def normalize(v):
        length = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        if length > 0.0 and math.isfinite(length):
            return (v[0] / length, v[1] / length, v[2] / length)
        return (0.0, 0.0, -1.0)

    def cross_length(a, b):
        c = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
        return math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])

    up = tuple(float(v) for v in up_vector) if up_vector is not None else (0.0, 1.0, 0.0)
    view_dir = normalize(tuple(center[a] - eye[a] for a in range(3)))
    if cross_length(view_dir, up) <= float(f32(1e-4)):
        up = (0.0, 0.0, 1.0)
        if cross_length(view_dir, up) <= float(f32(1e-4)):
            up = (1.0, 0.0, 0.0)
    up = normalize(up)
    return CameraParameters(eye, tuple(center), up,
                            float(f32(f32(fov_y * f32(180.0)) / k_pi)), float(f32(0.1)),
                            float(f32(distance * f32(4.0))))


def render_scene(ctx, scene: SceneGeometry, options: RenderOptions, rank: int = 0,
                 n_ranks: int = 1, process_group=None, stage_through_host: bool = False) -> int:
    """renderScene (VolumeRenderer.cpp:947-1101 -> renderSingleTrial) with an explicit camera or
    the automatic one: paints, composites, gathers and writes the image on rank 0.  Returns 0 on
    success like the reference."""
    from .renderer import FrameRenderer, RenderParameters
    validate_options(options)
    camera = options.camera
    if camera is None:
        camera = automatic_camera(scene.bounds, up_vector=options.up_vector)
    extension = os.path.splitext(options.output_filename)[1].lower()
    renderer = FrameRenderer(ctx, scene.all_boxes, scene.local_boxes, scene.scalar_transform,
                             scene.bounds, scene.scalar_range, rank, n_ranks, process_group,
                             color_map=options.color_map, stage_through_host=stage_through_host)
    if options.mode == "max_intensity":
        rgb8, _ = renderer.render_max_intensity(
            RenderParameters(options.width, options.height, options.box_transparency,
                             options.antialiasing, options.visibility_graph, draw_bounds=False,
                             write_visibility_graph=options.write_visibility_graph), camera)
    else:
        _, rgb8 = renderer.render(
            RenderParameters(options.width, options.height, options.box_transparency,
                             options.antialiasing, options.visibility_graph,
                             write_visibility_graph=options.write_visibility_graph), camera)
    renderer.synchronize()
    if rank == 0:
        # any other extension falls back to PPM (VolumeRenderer.cpp:1316-1327)
        writer = save_png if extension == ".png" else save_ppm
        if not writer(rgb8, options.output_filename):
            return 1
    return 0


def render(plotfile: str, width: int = 512, height: int = 512, box_transparency: float = 0.0,
           antialiasing: int = 1, visibility_graph: bool = True,
           write_visibility_graph: bool = False, variable: Optional[str] = None,
           min_level: int = 0, max_level: int = -1, log_scale: bool = False,
           up_vector: Optional[Sequence[float]] = None, output: Optional[str] = None,
           scalar_range: Optional[Sequence[float]] = None,
           camera_eye: Optional[Sequence[float]] = None,
           camera_look_at: Optional[Sequence[float]] = None,
           camera_up: Optional[Sequence[float]] = None, camera_fov_y: Optional[float] = None,
           camera_near: Optional[float] = None, camera_far: Optional[float] = None,
           color_map: Optional[Sequence[Sequence[float]]] = None, mode: str = "volume") -> int:
    """The reference's python entry (python/amrVolumeRenderer/module.cpp:275-303), same keyword
    names and defaults: validates the arguments as the reference does, reads the plotfile
    (plotfile.py), renders on cuda:0 and writes the image.  Multi-rank use: call run() with the
    rank, world size and process group.  mode: "volume" (default) or "max_intensity" (a
    maximum-intensity projection, RenderOptions.mode)."""
    camera = None
    if camera_eye is not None or camera_look_at is not None:
        if camera_eye is None or camera_look_at is None:
            raise ValueError("camera_eye and camera_look_at must be given together")
        camera = CameraParameters(tuple(camera_eye), tuple(camera_look_at),
                                  tuple(camera_up) if camera_up is not None else (0.0, 1.0, 0.0),
                                  45.0 if camera_fov_y is None else float(camera_fov_y),
                                  0.1 if camera_near is None else float(camera_near),
                                  1000.0 if camera_far is None else float(camera_far))
    cmap = None
    if color_map is not None:
        cmap = []
        for entry in color_map:
            if len(tuple(entry)) != 5:
                raise ValueError("color_map entries are (value, red, green, blue, alpha)")
            cmap.append(ColorMapControlPoint(*[float(v) for v in entry]))
    options = RenderOptions(
        width=width, height=height, box_transparency=box_transparency, antialiasing=antialiasing,
        visibility_graph=visibility_graph, write_visibility_graph=write_visibility_graph,
        min_level=min_level, max_level=max_level, log_scale_input=log_scale,
        output_filename=output if output is not None else "volume-renderer.ppm",
        up_vector=tuple(up_vector) if up_vector is not None else None,
        scalar_range=tuple(scalar_range) if scalar_range is not None else None,
        camera=camera, color_map=cmap, mode=mode)
    validate_options(options)
    from .renderer import validate_render_parameters, RenderParameters
    validate_render_parameters(RenderParameters(width, height, box_transparency, antialiasing))
    if not plotfile:
        raise RuntimeError("plotfile path is required")
    if not os.path.exists(plotfile):
        raise RuntimeError(f"plotfile path '{plotfile}' does not exist")
    ctx, rank, world, group = _runtime_scope()
    return run(plotfile, options, variable or "", ctx, rank, world, group)


def run(plotfile: str, options: RenderOptions, variable_name: str = "", ctx=None, rank: int = 0,
        n_ranks: int = 1, process_group=None, stage_through_host: bool = False) -> int:
    """VolumeRenderer::run(RunOptions) after its argument checks (VolumeRenderer.cpp:1469-1576):
    load the plotfile, apply a scalar-range override and convert the colour map's physical
    values to normalised ones, then renderScene."""
    from . import plotfile as pf
    from . import runtime
    validate_mode(options)
    if ctx is None:
        ctx = runtime.Context(0)
    has_override = options.scalar_range is not None
    scene = _load_variable_scenes(ctx, plotfile, [variable_name], options.min_level,
                                  options.max_level, options.log_scale_input,
                                  not has_override, rank, n_ranks, process_group)[0]
    return _render_loaded_scene(ctx, scene, options, rank, n_ranks, process_group,
                                stage_through_host)


def render_amr_data(data: AmrData, options: RenderOptions, ctx=None, rank: int = 0,
                    n_ranks: int = 1, process_group=None) -> int:
    """api::Render(const AmrData&, const RenderOptions&) (VolumeRendererApi.cpp:257-395)."""
    from . import runtime
    validate_options(options)
    if ctx is None:
        ctx = runtime.Context(0)
    scene = load_amr_data_geometry(ctx, data, options.min_level, options.max_level,
                                   options.component, options.log_scale_input,
                                   options.scalar_range is None, rank, n_ranks, process_group)
    return _render_loaded_scene(ctx, scene, options, rank, n_ranks, process_group)


def _render_loaded_scene(ctx, scene: SceneGeometry, options: RenderOptions, rank: int,
                         n_ranks: int, process_group, stage_through_host: bool = False) -> int:
    """The common tail of VolumeRenderer::run and api::Render: scalar-range override, colour-map
    values from physical to normalised, camera-up normalisation, renderScene."""
    import numpy as np
    f32 = np.float32
    has_override = options.scalar_range is not None
    if scene.processed_scalar_range is None:
        raise RuntimeError("Internal error: processed scalar range unavailable for color mapping.")
    processed_min, processed_max = (f32(v) for v in scene.processed_scalar_range)
    span = f32(processed_max - processed_min)
    if not (span > 0.0) or not np.isfinite(span):
        raise RuntimeError("Failed to establish a finite scalar range for color mapping.")
    logf = _libm_float("logf")

    def to_processed(physical) -> np.float32:
        physical = f32(physical)
        if not np.isfinite(physical):
            raise ValueError("color_map scalar values must be finite.")
        if options.log_scale_input:
            if not (physical > 0.0):
                raise ValueError("color_map scalar values must be positive when log scaling is "
                                 "enabled.")
            return f32(logf(physical))
        return physical

    norm_min, norm_max = processed_min, processed_max
    if has_override:
        norm_min = to_processed(options.scalar_range[0])
        norm_max = to_processed(options.scalar_range[1])
        if not (norm_min < norm_max):
            raise ValueError("scalar_range must contain two values with min < max.")
    norm_span = f32(norm_max - norm_min)
    if not (norm_span > 0.0) or not np.isfinite(norm_span):
        raise RuntimeError("Failed to establish a finite scalar range for color mapping.")
    if has_override:
        # SetSceneNormalizationRange (SceneBuilder.cpp:427-443), amrex::Real arithmetic
        lo, hi = float(norm_min), float(norm_max)
        transform = scene.scalar_transform
        transform.normalize_to_unit_range = True
        transform.normalization_min = lo
        transform.inverse_normalization_span = 1.0 / (hi - lo)
        scene.scalar_range = (0.0, 1.0)
    if options.color_map is not None:
        converted = []
        for point in options.color_map:
            value = f32(f32(to_processed(point.value) - norm_min) / norm_span)
            if not np.isfinite(value):
                raise ValueError("color_map produced a non-finite normalized scalar value.")
            value = min(max(value, f32(0.0)), f32(1.0))
            converted.append(ColorMapControlPoint(float(value), point.red, point.green,
                                                  point.blue, point.alpha))
        options = _replace(options, color_map=converted)
    if options.camera is not None:
        cam = options.camera
        length = math.sqrt(sum(float(v) ** 2 for v in cam.up))
        up = tuple(float(v) / length for v in cam.up) if (length > 0.0 and math.isfinite(length)) \
            else (0.0, 0.0, -1.0)
        options = _replace(options, camera=CameraParameters(cam.eye, cam.look_at, up,
                                                            cam.fov_y_degrees, cam.near_plane,
                                                            cam.far_plane))
    return render_scene(ctx, scene, options, rank, n_ranks, process_group, stage_through_host)


def _replace(options: RenderOptions, **changes) -> RenderOptions:
    import dataclasses
    return dataclasses.replace(options, **changes)


def validate_projection_arguments(width: int, height: int, quantity: str, log_scale: bool,
                                  value_range: Optional[Sequence[float]]) -> Optional[Tuple[float, float]]:
    """The argument checks of project(), before any GPU work: returns value_range as floats."""
    from .renderer import validate_render_parameters, RenderParameters
    from .runtime import PROJECTION_QUANTITIES
    if quantity not in PROJECTION_QUANTITIES:
        raise ValueError(f"quantity must be one of {', '.join(PROJECTION_QUANTITIES)}, not {quantity!r}")
    validate_render_parameters(RenderParameters(width, height))
    if value_range is None:
        return None
    values = tuple(value_range)
    if len(values) != 2:
        raise ValueError("value_range must hold two values (lo, hi)")
    lo, hi = (float(v) for v in values)
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("value_range must be finite")
    if not (lo < hi):
        raise ValueError("value_range must satisfy lo < hi")
    if log_scale and not (lo > 0.0):
        raise ValueError("value_range must be positive when log_scale is enabled")
    return lo, hi


def projection_rgb_table(color_map: Optional[Sequence[Sequence[float]]] = None):
    """The 256 RGB8 entries of a projection picture: buildColorTable's colours of the colour map
    over [0, 1] (entries (value, red, green, blue, alpha); alpha has no effect), each component as
    Color::GetComponentAsByte makes it a byte -> [256, 3] uint8."""
    import numpy as np
    from .runtime import build_color_table
    cmap = None
    if color_map is not None:
        cmap = []
        for entry in color_map:
            if len(tuple(entry)) != 5:
                raise ValueError("color_map entries are (value, red, green, blue, alpha)")
            cmap.append(ColorMapControlPoint(*[float(v) for v in entry]))
    table = build_color_table(1.0, 1.0, (0.0, 1.0), cmap)[:, :3]
    scaled = (table * np.float32(256.0)).astype(np.float32)
    return np.clip(np.trunc(scaled), 0, 255).astype(np.uint8)


def project(plotfile: str, width: int = 512, height: int = 512, variable: Optional[str] = None,
            min_level: int = 0, max_level: int = -1,
            camera_eye: Optional[Sequence[float]] = None,
            camera_look_at: Optional[Sequence[float]] = None,
            camera_up: Optional[Sequence[float]] = None, camera_fov_y: Optional[float] = None,
            camera_near: Optional[float] = None, camera_far: Optional[float] = None,
            quantity: str = "column", log_scale: bool = False,
            value_range: Optional[Sequence[float]] = None,
            color_map: Optional[Sequence[Sequence[float]]] = None, output: Optional[str] = None,
            up_vector: Optional[Sequence[float]] = None):
    """Line-integral projection of a plotfile's raw field (yt's ProjectionPlot; DESIGN.md, "Column
    projection"), on cuda:0.  Per pixel, over the samples of the maximum-intensity march, column =
    sum over boxes of step * (sum of the finite cell values) and length = sum of step * (their
    number), with lengths in the plotfile's physical units (the geometry loader's rescale undone).
    quantity "column" returns column (for a density, the surface density), "mean" column / length
    (0 where length is 0).  Returns that array on rank 0 -- numpy float64 [height, width], row 0 at
    the bottom like the image's origin -- and None on other ranks.  With output (.png, else PPM) rank
    0 also writes the picture: q = the quantity (log10 of it with log_scale) -> colour-map entry
    clamp(floor((q - lo) / (hi - lo) * 255), 0, 255) over value_range = (lo, hi) (log_scale: lo and
    hi are quantities, not logarithms), or over the min and max of q when value_range is None;
    pixels with length 0 (and, with log_scale, q <= 0) are black.  The camera arguments are
    those of render(); without camera_eye / camera_look_at the automatic camera is used."""
    rng = validate_projection_arguments(width, height, quantity, log_scale, value_range)
    camera = None
    if camera_eye is not None or camera_look_at is not None:
        if camera_eye is None or camera_look_at is None:
            raise ValueError("camera_eye and camera_look_at must be given together")
        up = tuple(camera_up) if camera_up is not None else (0.0, 1.0, 0.0)
        length = math.sqrt(sum(float(v) ** 2 for v in up))
        up = tuple(float(v) / length for v in up) if (length > 0.0 and math.isfinite(length)) \
            else (0.0, 0.0, -1.0)
        camera = CameraParameters(tuple(camera_eye), tuple(camera_look_at), up,
                                  45.0 if camera_fov_y is None else float(camera_fov_y),
                                  0.1 if camera_near is None else float(camera_near),
                                  1000.0 if camera_far is None else float(camera_far))
    table = projection_rgb_table(color_map)
    _require_plotfile(plotfile)
    from .renderer import FrameRenderer, RenderParameters
    import torch
    ctx, rank, world, group = _runtime_scope()
    scene = _load_variable_scenes(ctx, plotfile, [variable or ""], min_level, max_level, False,
                                  True, rank, world, group)[0]
    if camera is None:
        camera = automatic_camera(scene.bounds,
                                  up_vector=tuple(up_vector) if up_vector is not None else None)
    renderer = FrameRenderer(ctx, scene.all_boxes, scene.local_boxes, scene.scalar_transform,
                             scene.bounds, scene.scalar_range, rank, world, group)
    column, length = renderer.render_projection(RenderParameters(width, height, draw_bounds=False),
                                                camera)
    renderer.synchronize()
    if rank != 0:
        return None
    # scene lengths -> physical lengths
    to_physical = 1.0 / float(scene.world_scale)
    column = column * to_physical
    length = length * to_physical
    if quantity == "mean":
        q = torch.where(length > 0.0, column / torch.where(length > 0.0, length, 1.0),
                        torch.zeros_like(column))
    else:
        q = column
    if output is not None:
        rgb8, _ = ctx.projection_colorize(
            column, length, torch.from_numpy(table).to(column.device), quantity, log_scale,
            None if rng is None else ((math.log10(rng[0]), math.log10(rng[1])) if log_scale else rng))
        _write_picture(rgb8, output)
    return q.cpu().numpy()


# ---- slices ("Slice") ---------------------------------------------------------------

SLICE_QUANTITIES = ("value", "level")
# axis -> (normal, north): (U, V) = (y, z), (z, x), (x, y), yt's convention
SLICE_AXES = {"x": ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0)),
              "y": ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0)),
              "z": ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0))}


@dataclass
class SlicePlane:
    """A slice's plane in the plotfile's physical units: pixel (x, y) of a W x H image, row 0 at
    the bottom, shows the point center + ((x + 0.5) / W - 0.5) width[0] U + ((y + 0.5) / H - 0.5)
    width[1] V with (U, V) = slice_basis(normal, north)."""
    center: Tuple[float, float, float]
    normal: Tuple[float, float, float]
    north: Tuple[float, float, float]
    width: Tuple[float, float]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _unit(v, what: str):
    values = tuple(float(c) for c in v)
    if len(values) != 3:
        raise ValueError(f"{what} must hold three values")
    length = math.sqrt(values[0] * values[0] + values[1] * values[1] + values[2] * values[2])
    if not (math.isfinite(length) and length > 0.0):
        raise ValueError(f"{what} must be a finite, non-zero vector")
    return tuple(c / length for c in values)


def slice_basis(normal: Sequence[float], north: Sequence[float]):
    """(n, U, V) of a slice plane, float64: n = normal / |normal|, U = normalize(north x n),
    V = n x U -- with n pointing at the viewer U points right and V up.  ValueError if north is
    parallel to the normal (|north x n| <= 1e-6 for unit vectors), zero or not finite."""
    n = _unit(normal, "normal")
    right = _cross(_unit(north, "north"), n)
    length = math.sqrt(right[0] * right[0] + right[1] * right[1] + right[2] * right[2])
    if not (length > 1e-6):
        raise ValueError("north must not be parallel to the normal")
    u = tuple(c / length for c in right)
    return n, u, _cross(n, u)


def validate_slice_arguments(width: int, height: int, axis: str = "z",
                             normal: Optional[Sequence[float]] = None,
                             north: Optional[Sequence[float]] = None,
                             plane_width: Optional[Sequence[float]] = None,
                             quantity: str = "value", log_scale: bool = False,
                             value_range: Optional[Sequence[float]] = None):
    """The argument checks of slice(), before any GPU work.  Returns (normal, north, plane_width
    or None, value_range or None): normal / north as given (they override axis) or the axis's."""
    if quantity not in SLICE_QUANTITIES:
        raise ValueError(f"quantity must be one of {', '.join(SLICE_QUANTITIES)}, not {quantity!r}")
    if normal is None and north is None:
        if axis not in SLICE_AXES:
            raise ValueError(f"axis must be one of x, y, z, not {axis!r}")
        normal, north = SLICE_AXES[axis]
    elif normal is None:
        if axis not in SLICE_AXES:
            raise ValueError(f"axis must be one of x, y, z, not {axis!r}")
        normal = SLICE_AXES[axis][0]
    elif north is None:
        raise ValueError("north must be given with normal")
    slice_basis(normal, north)
    widths = None
    if plane_width is not None:
        widths = tuple(float(v) for v in plane_width)
        if len(widths) != 2:
            raise ValueError("plane_width must hold two values (wu, wv)")
        if not all(math.isfinite(v) and v > 0.0 for v in widths):
            raise ValueError("plane_width must be finite and positive")
    rng = validate_projection_arguments(width, height, "column", log_scale, value_range)
    return tuple(float(c) for c in normal), tuple(float(c) for c in north), widths, rng


def combine_slices(parts):
    """The slices of several owners -> the slice of them all; parts: (value, level, box) triples
    as slice_scene returns them (torch tensors or numpy arrays of one shape).  The owners' boxes
    are disjoint, so at most one part hits a pixel and the others hold (0.0, -1, -1) there: the
    combination is the SUM of value and the MAX of level and of box.  The sum runs over the
    values' 64-bit patterns (a miss is all zero bits), which keeps the hit's bits -- -0.0 and a
    NaN's payload included -- where a floating-point sum would not."""
    import numpy as np
    import torch
    parts = list(parts)
    if not parts:
        raise ValueError("combine_slices needs at least one part")
    as_tensor = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    value, level, box = (as_tensor(a) for a in parts[0])
    if value.dtype != torch.float64 or level.dtype != torch.int8 or box.dtype != torch.int32:
        raise ValueError("parts are (float64 value, int8 level, int32 box)")
    bits = value.contiguous().view(torch.int64).clone()
    level, box = level.clone(), box.clone()
    for part in parts[1:]:
        v, l, b = (as_tensor(a) for a in part)
        if v.shape != value.shape or l.shape != value.shape or b.shape != value.shape or \
                (v.dtype, l.dtype, b.dtype) != (torch.float64, torch.int8, torch.int32):
            raise ValueError("parts must agree in shape and type")
        bits += v.contiguous().view(torch.int64)
        level = torch.maximum(level, l)
        box = torch.maximum(box, b)
    out = (bits.view(torch.float64), level, box)
    if not isinstance(parts[0][0], torch.Tensor):
        return tuple(t.numpy() for t in out)
    return out


def slice_scene(ctx, scene: SceneGeometry, plane: SlicePlane, width: int, height: int,
                rank: int = 0, n_ranks: int = 1, process_group=None):
    """The slice of a loaded scene: (value float64, level int8, box int32), [height, width]
    tensors on ctx.device, row 0 at the bottom ("Slice"): the raw value of the cell
    that contains the pixel's point, its box's AMR level and its index in scene.all_boxes;
    (0.0, -1, -1) where no box does.  Every rank slices its local_boxes; for n_ranks > 1 the parts
    are combined on rank 0 as combine_slices states (other ranks get (None, None, None)), through
    the host if the group's backend is not NCCL.  Every box of scene.local_boxes must be among
    scene.all_boxes with the same corners and level (ValueError otherwise): that is where its
    index comes from.  Each call stages the box table anew; for many slices of one scene keep a
    runtime.Scene and call its slice()."""
    import torch
    _, u, v = slice_basis(plane.normal, plane.north)
    wu, wv = (float(w) for w in plane.width)
    if not (math.isfinite(wu) and wu > 0.0 and math.isfinite(wv) and wv > 0.0):
        raise ValueError("plane_width must be finite and positive")
    if int(width) <= 0 or int(height) <= 0:
        raise ValueError("image dimensions must be positive")
    scale = float(scene.world_scale)
    center = tuple(float(c) for c in plane.center)
    origin = tuple((center[a] - 0.5 * wu * u[a] - 0.5 * wv * v[a]) * scale for a in range(3))
    du = tuple(u[a] * wu * scale / float(width) for a in range(3))
    dv = tuple(v[a] * wv * scale / float(height) for a in range(3))
    where = {(tuple(b.min_corner), tuple(b.max_corner), int(b.level)): i
             for i, b in enumerate(scene.all_boxes)}
    try:
        index = [where[(tuple(b.min_corner), tuple(b.max_corner), int(b.level))]
                 for b in scene.local_boxes]
    except KeyError:
        raise ValueError("a local box is not among the scene's all_boxes") from None
    with _native_scenes(ctx, [scene]) as (local,):
        value, level, box = local.slice(origin, du, dv, width, height, index)
        if n_ranks > 1:
            import torch.distributed as dist
            stage = dist.get_backend(process_group) != "nccl"
            root = dist.get_global_rank(process_group, 0) if process_group is not None else 0
            ctx.synchronize()
            parts = [value.view(torch.int64), level.to(torch.int32), box]
            if stage:
                parts = [t.cpu() for t in parts]
            dist.reduce(parts[0], root, op=dist.ReduceOp.SUM, group=process_group)
            dist.reduce(parts[1], root, op=dist.ReduceOp.MAX, group=process_group)
            dist.reduce(parts[2], root, op=dist.ReduceOp.MAX, group=process_group)
            if rank != 0:
                return None, None, None
            value = parts[0].to(ctx.device).view(torch.float64)
            level = parts[1].to(ctx.device).to(torch.int8)
            box = parts[2].to(ctx.device)
        ctx.synchronize()
    return value, level, box


def slice(plotfile: str, width: int = 512, height: int = 512, variable: Optional[str] = None,
          min_level: int = 0, max_level: int = -1, axis: str = "z",
          center: Optional[Sequence[float]] = None, normal: Optional[Sequence[float]] = None,
          north: Optional[Sequence[float]] = None, plane_width: Optional[Sequence[float]] = None,
          quantity: str = "value", log_scale: bool = False,
          value_range: Optional[Sequence[float]] = None,
          color_map: Optional[Sequence[Sequence[float]]] = None, annotate_grids: bool = False,
          output: Optional[str] = None):
    """Slice of a plotfile's raw field (yt's SlicePlot; DESIGN.md 7, "Slice"), on cuda:0: the plane
    through `center` with the given normal; per pixel the value of the finest loaded cell that
    contains the pixel's point (quantity "value", no interpolation, no transform) or that cell's
    AMR level (quantity "level").  axis "x" | "y" | "z" puts (right, up) = (y, z), (z, x), (x, y);
    normal with north (the direction that is up in the picture) override it.  center defaults to
    the centre of the data's bounding box, plane_width = (wu, wv) to the data's extent along right
    and up; all three are in the plotfile's physical units.  Returns the numpy float64 [height,
    width] image on rank 0, row 0 at the bottom, NaN where no loaded cell contains the point
    (outside the data, or in a hole left by min_level > 0), and None on other ranks.  With output
    (.png, else PPM) rank 0 also writes the picture, coloured as project() colours a column: entry
    clamp(floor((q - lo) / (hi - lo) * 255), 0, 255) of the colour map over value_range (or the
    min and max of q), log10 of q with log_scale; misses and non-finite values are black;
    annotate_grids draws the boxes' boundaries in white."""
    normal, north, widths, rng = validate_slice_arguments(width, height, axis, normal, north,
                                                          plane_width, quantity, log_scale,
                                                          value_range)
    if center is not None:
        center = tuple(float(c) for c in center)
        if len(center) != 3 or not _finite(center):
            raise ValueError("center must hold three finite values")
    table = projection_rgb_table(color_map)
    _require_plotfile(plotfile)
    import torch
    ctx, rank, world, group = _runtime_scope()
    scene = _load_variable_scenes(ctx, plotfile, [variable or ""], min_level, max_level, False,
                                  True, rank, world, group)[0]
    to_physical = 1.0 / float(scene.world_scale)
    lo = [min(b.min_corner[a] for b in scene.all_boxes) * to_physical for a in range(3)]
    hi = [max(b.max_corner[a] for b in scene.all_boxes) * to_physical for a in range(3)]
    if center is None:
        center = tuple(0.5 * (lo[a] + hi[a]) for a in range(3))
    if widths is None:
        _, u, v = slice_basis(normal, north)
        widths = tuple(sum(abs(e[a]) * (hi[a] - lo[a]) for a in range(3)) for e in (u, v))
    value, level, box = slice_scene(ctx, scene, SlicePlane(center, normal, north, widths), width,
                                    height, rank, world, group)
    if rank != 0:
        return None
    hit = level >= 0
    shown = value if quantity == "value" else level.to(torch.float64)
    if output is not None:
        rgb8, _ = ctx.projection_colorize(
            torch.where(hit, shown, torch.zeros_like(shown)), hit.to(torch.float64),
            torch.from_numpy(table).to(value.device), "column", log_scale,
            None if rng is None else ((math.log10(rng[0]), math.log10(rng[1])) if log_scale else rng))
        if annotate_grids:
            ctx.slice_outline(box, rgb8)
        _write_picture(rgb8, output)
    nan = torch.full_like(shown, float("nan"))
    return torch.where(hit, shown, nan).cpu().numpy()


# ---- phase plots and profiles ("Phase plot and profile") ----------------------------

JOINT_HISTOGRAM_MAX_BINS = 1024        # per axis
JOINT_HISTOGRAM_MAX_CELLS = 1 << 20    # nx * ny
JOINT_HISTOGRAM_MAX_LEVELS = 16
HISTOGRAM_WEIGHTS = ("cell_volume", "cells")


def _bin_count(n, what: str) -> int:
    import operator
    try:
        n = operator.index(n)
    except TypeError:
        n = 0
    if isinstance(n, bool) or not (1 <= n <= JOINT_HISTOGRAM_MAX_BINS):
        raise ValueError(f"{what} must be an integer in [1, {JOINT_HISTOGRAM_MAX_BINS}]")
    return n


def _bin_range(values, log: bool, what: str) -> Tuple[float, float]:
    values = tuple(values)
    if len(values) != 2:
        raise ValueError(f"{what} must hold two values (lo, hi)")
    lo, hi = (float(v) for v in values)
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"{what} must be finite")
    if not (lo < hi):
        raise ValueError(f"{what} must satisfy lo < hi")
    if log and not (lo > 0.0):
        raise ValueError(f"{what} must be positive for logarithmic bins")
    return lo, hi


def _checked_edges(edges, what: str):
    import numpy as np
    e = np.array(edges, dtype=np.float64)
    if e.ndim != 1 or not (2 <= e.size <= JOINT_HISTOGRAM_MAX_BINS + 1):
        raise ValueError(f"{what} must hold between 2 and {JOINT_HISTOGRAM_MAX_BINS + 1} values")
    if not np.isfinite(e).all():
        raise ValueError(f"{what} must be finite")
    if not (e[1:] > e[:-1]).all():
        raise ValueError(f"{what} must be strictly increasing")
    return e


def bin_edges(lo: float, hi: float, n: int, log: bool = False):
    """The n + 1 float64 edges of n bins over [lo, hi], numpy float64 arithmetic throughout:
    linear e[i] = lo + (hi - lo) * (i / n); log (lo > 0) e[i] = 10 ** (log10(lo) + (log10(hi) -
    log10(lo)) * (i / n)); e[0] = lo and e[n] = hi exactly in both.  ValueError if the result is
    not finite and strictly increasing (a range too narrow for n bins)."""
    import numpy as np
    n = _bin_count(n, "the bin count")
    lo, hi = _bin_range((lo, hi), log, "the bin range")
    fraction = np.arange(n + 1, dtype=np.float64) / np.float64(n)
    with np.errstate(over="ignore", invalid="ignore"):
        if log:
            a, b = np.log10(np.float64(lo)), np.log10(np.float64(hi))
            e = np.float64(10.0) ** (a + (b - a) * fraction)
        else:
            e = np.float64(lo) + (np.float64(hi) - np.float64(lo)) * fraction
    e[0], e[n] = lo, hi
    return _checked_edges(e, "the bin edges")


def _histogram_axis(bins, rng, log: bool, edges, name: str):
    """(n, range or None, edges or None) of one axis; explicit edges override the rest."""
    if edges is not None:
        e = _checked_edges(edges, f"{name}_edges")
        return e.size - 1, None, e
    n = _bin_count(bins, f"{name} bins")
    return n, (None if rng is None else _bin_range(rng, bool(log), f"{name}_range")), None


def validate_phase_arguments(z="cell_volume", bins=(128, 128), x_range=None, y_range=None,
                             x_log: bool = False, y_log: bool = False, x_edges=None, y_edges=None,
                             log_scale: bool = False, value_range=None):
    """The argument checks of phase(), before any GPU work and before the plotfile is opened.
    Returns ((nx, x_range, x_edges), (ny, y_range, y_edges), value_range): a range / edges entry
    is None where it was not given, edges are float64 arrays."""
    if not isinstance(z, str) or not z:
        raise ValueError(f"z must be one of {', '.join(HISTOGRAM_WEIGHTS)} or a variable name, "
                         f"not {z!r}")
    try:
        pair = tuple(bins)
    except TypeError:
        raise ValueError("bins must hold two values (nx, ny)") from None
    if len(pair) != 2:
        raise ValueError("bins must hold two values (nx, ny)")
    x = _histogram_axis(pair[0], x_range, x_log, x_edges, "x")
    y = _histogram_axis(pair[1], y_range, y_log, y_edges, "y")
    if x[0] * y[0] > JOINT_HISTOGRAM_MAX_CELLS:
        raise ValueError(f"the histogram must not have more than {JOINT_HISTOGRAM_MAX_CELLS} bins")
    rng = validate_projection_arguments(1, 1, "column", log_scale, value_range)
    return x, y, rng


def validate_profile_arguments(weight="cell_volume", bins=128, x_range=None, x_log: bool = False,
                               x_edges=None):
    """The argument checks of profile(), before any GPU work and before the plotfile is opened.
    Returns (nx, x_range or None, x_edges or None)."""
    if weight not in HISTOGRAM_WEIGHTS:
        raise ValueError(f"weight must be one of {', '.join(HISTOGRAM_WEIGHTS)}, not {weight!r}")
    return _histogram_axis(bins, x_range, x_log, x_edges, "x")


def joint_histogram_values(cells_by_level, sums_by_level, cell_volumes, z: str = "cell_volume"):
    """values of a joint histogram from its per-level arrays, float64, level ascending from +0.0:
    "cell_volume": sum_l vol[l] * f64(cells[l]); "cells": sum_l f64(cells[l]); anything else (a
    summed variable): sum_l vol[l] * sums[l], the volume integral of that variable per bin."""
    import numpy as np
    cells = np.asarray(cells_by_level)
    values = np.zeros(cells.shape[1:], dtype=np.float64)
    if z not in HISTOGRAM_WEIGHTS and sums_by_level is None:
        raise ValueError("a summed variable needs sums_by_level")
    for level in range(cells.shape[0]):
        vol = np.float64(cell_volumes[level])
        if z == "cell_volume":
            values = values + vol * cells[level].astype(np.float64)
        elif z == "cells":
            values = values + cells[level].astype(np.float64)
        else:
            values = values + vol * np.asarray(sums_by_level[level], dtype=np.float64)
    return values


def profile_mean(cells_by_level, sums_by_level, cell_volumes, weight: str = "cell_volume"):
    """(mean, weight_sum) of a profile from its per-level arrays: mean = sum_l w[l] sums[l] /
    sum_l w[l] f64(cells[l]) with w = vol ("cell_volume") or 1 ("cells"), level ascending from
    +0.0; NaN where the denominator (weight_sum) is 0."""
    import numpy as np
    if weight not in HISTOGRAM_WEIGHTS:
        raise ValueError(f"weight must be one of {', '.join(HISTOGRAM_WEIGHTS)}, not {weight!r}")
    cells = np.asarray(cells_by_level)
    numerator = np.zeros(cells.shape[1:], dtype=np.float64)
    weight_sum = np.zeros(cells.shape[1:], dtype=np.float64)
    for level in range(cells.shape[0]):
        w = np.float64(cell_volumes[level]) if weight == "cell_volume" else np.float64(1.0)
        numerator = numerator + w * np.asarray(sums_by_level[level], dtype=np.float64)
        weight_sum = weight_sum + w * cells[level].astype(np.float64)
    filled = weight_sum != 0.0
    mean = np.full(weight_sum.shape, np.nan, dtype=np.float64)
    mean[filled] = numerator[filled] / weight_sum[filled]
    return mean, weight_sum


def combine_joint_histograms(parts):
    """The joint histograms of several owners -> that of them all: the plain sum, in the order
    given.  parts: (cells, sums or None, totals) triples as Scene.joint_histogram returns them
    (torch tensors or numpy arrays of one shape); sums is None if it is None in every part."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_joint_histograms needs at least one part")
    cells, sums, totals = parts[0]
    cells, totals = _copied(cells), _copied(totals)
    if sums is not None:
        sums = _copied(sums)
    for c, s, t in parts[1:]:
        if tuple(c.shape) != tuple(cells.shape) or (s is None) != (sums is None):
            raise ValueError("parts must agree in shape and in having sums")
        cells += c
        totals += t
        if s is not None:
            sums += s
    return cells, sums, totals


def level_cell_volumes(cell_sizes) -> List[float]:
    """vol[l] = dx * dy * dz (float64, multiplied in this order) of each level's cell_size."""
    return [float(c[0]) * float(c[1]) * float(c[2]) for c in cell_sizes]


def phase_scene(ctx, scene_x: SceneGeometry, scene_y: Optional[SceneGeometry], x_edges, y_edges,
                cell_volumes: Sequence[float], z: str = "cell_volume",
                scene_z: Optional[SceneGeometry] = None, rank: int = 0, n_ranks: int = 1,
                process_group=None) -> dict:
    """Joint histogram of loaded scenes ("Phase plot and profile"): scene_x, scene_y
    and scene_z are the scenes load_plotfile_geometry returns for different variables of one
    plotfile with the same levels, rank and world size.  scene_y None: one y bin (a profile's
    input; y_edges is then None).  z "cell_volume" | "cells", or anything else with scene_z: that
    field is summed per bin.  cell_volumes[l] = the physical cell volume of level l, one entry per
    level up to the finest loaded one.  Every rank bins its local_boxes; cells, sums and totals are
    all-reduced with SUM (through the host if the group's backend is not NCCL).  Returns, on every
    rank, a dict of numpy arrays: values float64 [ny, nx] (joint_histogram_values), cells int64
    [ny, nx] and sums float64 [ny, nx] (None without scene_z) summed over levels, cells_by_level
    / sums_by_level [L, ny, nx], outside and nonfinite (int), x_edges, y_edges."""
    import numpy as np
    if (z not in HISTOGRAM_WEIGHTS) != (scene_z is not None):
        raise ValueError("scene_z is given exactly when z names a variable")
    ex = _checked_edges(x_edges, "x_edges")
    ey = None
    if scene_y is not None:
        ey = _checked_edges(y_edges, "y_edges")
    elif y_edges is not None:
        raise ValueError("y_edges must be given with scene_y")
    if (ex.size - 1) * (1 if ey is None else ey.size - 1) > JOINT_HISTOGRAM_MAX_CELLS:
        raise ValueError(f"the histogram must not have more than {JOINT_HISTOGRAM_MAX_CELLS} bins")
    volumes = [float(v) for v in cell_volumes]
    n_levels = len(volumes)
    finest = max((int(b.level) for b in scene_x.all_boxes), default=0)
    if not (finest < n_levels <= JOINT_HISTOGRAM_MAX_LEVELS):
        raise ValueError("cell_volumes must hold one entry per level up to the finest loaded one "
                         f"(at most {JOINT_HISTOGRAM_MAX_LEVELS})")
    with _native_scenes(ctx, [scene_x, scene_y, scene_z]) as (x, y, s):
        cells, sums, totals = x.joint_histogram(ex, y, ey, s, n_levels)
        if n_ranks > 1:
            cells, sums, totals = _sum_over_ranks(ctx, (cells, sums, totals), process_group)
        ctx.synchronize()
        cells_by_level = cells.cpu().numpy()
        sums_by_level = None if sums is None else sums.cpu().numpy()
        totals = totals.cpu().numpy()
    total_sums = None
    if sums_by_level is not None:
        total_sums = np.zeros(sums_by_level.shape[1:], dtype=np.float64)
        for level in range(n_levels):
            total_sums = total_sums + sums_by_level[level]
    return {"values": joint_histogram_values(cells_by_level, sums_by_level, volumes, z),
            "cells": cells_by_level.sum(axis=0), "sums": total_sums,
            "cells_by_level": cells_by_level, "sums_by_level": sums_by_level,
            "outside": int(totals[0]), "nonfinite": int(totals[1]),
            "x_edges": ex, "y_edges": ey}


def _field_range(ctx, scene: SceneGeometry, log: bool, what: str, n_ranks: int, process_group):
    """(lo, hi) of a field's finite cells over all ranks ((min positive, max) with log), hi moved
    off lo if they are equal."""
    import torch
    with _native_scenes(ctx, [scene]) as (local,):
        lo, hi, lo_pos, finite = local.scalar_stats()
    if n_ranks > 1:
        import torch.distributed as dist
        device = ctx.device if dist.get_backend(process_group) == "nccl" else "cpu"
        mins = torch.tensor([lo, lo_pos], dtype=torch.float64, device=device)
        maxs = torch.tensor([hi], dtype=torch.float64, device=device)
        dist.all_reduce(mins, op=dist.ReduceOp.MIN, group=process_group)
        dist.all_reduce(maxs, op=dist.ReduceOp.MAX, group=process_group)
        lo, lo_pos, hi = mins[0].item(), mins[1].item(), maxs[0].item()
    if log:
        lo = lo_pos
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise RuntimeError(f"{what} has no {'positive ' if log else ''}finite cells to take a bin "
                           "range from")
    if lo == hi:
        hi = lo * 10.0 if log else lo + 1.0
    return lo, hi


def _load_fields(plotfile: str, variables, min_level: int, max_level: int):
    """(ctx, rank, world, group, scenes, cell volumes): one scene per variable name."""
    _require_plotfile(plotfile)
    from . import plotfile as pf
    header = pf.PlotFileData(plotfile)
    for name in variables:
        if name:
            _check_variable(plotfile, header, name)
    ctx, rank, world, group = _runtime_scope()
    scenes = _load_variable_scenes(ctx, plotfile, [name or "" for name in variables], min_level,
                                   max_level, False, True, rank, world, group)
    finest = max(int(b.level) for b in scenes[0].all_boxes)
    return ctx, rank, world, group, scenes, level_cell_volumes(header.cell_size[:finest + 1])


def _axis_edges(ctx, scene, axis, log: bool, what: str, world: int, group):
    n, rng, edges = axis
    if edges is not None:
        return edges
    if rng is None:
        rng = _field_range(ctx, scene, bool(log), what, world, group)
    return bin_edges(rng[0], rng[1], n, bool(log))


def phase(plotfile: str, x_variable: str, y_variable: str, z: str = "cell_volume",
          bins: Sequence[int] = (128, 128), x_range: Optional[Sequence[float]] = None,
          y_range: Optional[Sequence[float]] = None, x_log: bool = False, y_log: bool = False,
          x_edges=None, y_edges=None, min_level: int = 0, max_level: int = -1,
          log_scale: bool = False, value_range: Optional[Sequence[float]] = None,
          color_map: Optional[Sequence[Sequence[float]]] = None, output: Optional[str] = None):
    """Phase plot of a plotfile (yt's PhasePlot; DESIGN.md 7, "Phase plot and profile"), on cuda:0:
    the joint histogram of the raw cells of x_variable and y_variable over bins = (nx, ny) bins,
    every uncovered cell of the loaded levels counted once.  z "cell_volume": the physical volume
    per bin, "cells": the number of cells, a variable's name: the volume integral of that variable
    over the bin's cells (mass, for a density).  A range defaults to the field's (min, max) over
    its finite cells, (min positive, max) with x_log / y_log, which make the bins logarithmic; equal
    ends become (lo, lo + 1) ((lo, 10 lo) with log).  x_edges / y_edges (strictly increasing) override
    range, bins and log.  A value v lies in bin i when e[i] <= v < e[i + 1], the last bin closed at
    the top.  Returns, on every rank, phase_scene's dict: values [ny, nx] float64 (row = y bin),
    cells, sums, cells_by_level, sums_by_level, outside, nonfinite, x_edges, y_edges.  With output
    (.png, else PPM) rank 0 also writes the picture, coloured as project() colours a column: x to
    the right, the lowest y bin at the bottom, values over value_range (or their min and max),
    log10 of them with log_scale; bins without cells are black."""
    x, y, rng = validate_phase_arguments(z, bins, x_range, y_range, x_log, y_log, x_edges, y_edges,
                                         log_scale, value_range)
    table = projection_rgb_table(color_map)
    summed = z not in HISTOGRAM_WEIGHTS
    variables = [x_variable, y_variable] + ([z] if summed else [])
    ctx, rank, world, group, scenes, volumes = _load_fields(plotfile, variables, min_level,
                                                            max_level)
    ex = _axis_edges(ctx, scenes[0], x, x_log, "x_variable", world, group)
    ey = _axis_edges(ctx, scenes[1], y, y_log, "y_variable", world, group)
    result = phase_scene(ctx, scenes[0], scenes[1], ex, ey, volumes, z,
                         scenes[2] if summed else None, rank, world, group)
    if output is not None and rank == 0:
        import torch
        column = torch.from_numpy(result["values"]).to(ctx.device)
        length = torch.from_numpy((result["cells"] > 0).astype("float64")).to(ctx.device)
        rgb8, _ = ctx.projection_colorize(
            column, length, torch.from_numpy(table).to(ctx.device), "column", log_scale,
            None if rng is None else ((math.log10(rng[0]), math.log10(rng[1])) if log_scale else rng))
        _write_picture(rgb8, output)
    return result


def profile(plotfile: str, x_variable: str, y_variable: str, weight: str = "cell_volume",
            bins: int = 128, x_range: Optional[Sequence[float]] = None, x_log: bool = False,
            x_edges=None, min_level: int = 0, max_level: int = -1) -> dict:
    """Profile of a plotfile (yt's ProfilePlot; DESIGN.md 7, "Phase plot and profile"), on cuda:0:
    the mean of y_variable over the cells whose x_variable lies in each of `bins` bins, weighted by
    the cells' physical volume (weight "cell_volume") or equally ("cells").  Range, log and edges
    as in phase().  Returns, on every rank, a dict: x_edges, mean float64 [nx] (NaN for a bin
    without cells), weight_sum float64 [nx] (the mean's denominator), cells int64 [nx], outside,
    nonfinite."""
    x = validate_profile_arguments(weight, bins, x_range, x_log, x_edges)
    ctx, rank, world, group, scenes, volumes = _load_fields(plotfile, [x_variable, y_variable],
                                                            min_level, max_level)
    ex = _axis_edges(ctx, scenes[0], x, x_log, "x_variable", world, group)
    result = phase_scene(ctx, scenes[0], None, ex, None, volumes, y_variable or "field",
                         scenes[1], rank, world, group)
    mean, weight_sum = profile_mean(result["cells_by_level"][:, 0, :],
                                    result["sums_by_level"][:, 0, :], volumes, weight)
    return {"x_edges": result["x_edges"], "mean": mean, "weight_sum": weight_sum,
            "cells": result["cells"][0], "outside": result["outside"],
            "nonfinite": result["nonfinite"]}


# ---- on-axis projections ("On-axis projection") -------------------------------------

AXIS_PROJECTION_QUANTITIES = ("column", "mean")
_AXIS_INDEX = {"x": 0, "y": 1, "z": 2}


def validate_axis_projection_arguments(width: int, height: int, axis: str = "z",
                                       quantity: str = "column",
                                       center: Optional[Sequence[float]] = None,
                                       plane_width: Optional[Sequence[float]] = None,
                                       log_scale: bool = False,
                                       value_range: Optional[Sequence[float]] = None,
                                       weight: Optional[str] = None):
    """The argument checks of project_axis(), before any GPU work and before the plotfile is
    opened.  Returns (center or None, plane_width or None, value_range or None) as floats."""
    if axis not in _AXIS_INDEX:
        raise ValueError(f"axis must be one of x, y, z, not {axis!r}")
    if quantity not in AXIS_PROJECTION_QUANTITIES:
        raise ValueError(f"quantity must be one of {', '.join(AXIS_PROJECTION_QUANTITIES)}, "
                         f"not {quantity!r}")
    rng = validate_projection_arguments(width, height, "column", log_scale, value_range)
    if center is not None:
        center = tuple(float(c) for c in center)
        if len(center) != 3 or not _finite(center):
            raise ValueError("center must hold three finite values")
    widths = None
    if plane_width is not None:
        widths = tuple(float(v) for v in plane_width)
        if len(widths) != 2:
            raise ValueError("plane_width must hold two values (wu, wv)")
        if not all(math.isfinite(v) and v > 0.0 for v in widths):
            raise ValueError("plane_width must be finite and positive")
    if weight is not None:
        if not isinstance(weight, str) or not weight:
            raise ValueError(f"weight must be a variable name or None, not {weight!r}")
        if quantity == "column":
            raise ValueError('a weighted projection is a mean: quantity="column" takes no weight')
    return center, widths, rng


def combine_axis_projections(parts):
    """The on-axis projections of several owners -> that of them all: the plain sum, in the order
    given.  parts: (integral, weight or None, length) triples as Scene.axis_projection returns
    them (torch tensors or numpy arrays of one shape); weight is None if it is None in every
    part."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_axis_projections needs at least one part")
    integral, weight, length = parts[0]
    integral, length = _copied(integral), _copied(length)
    if weight is not None:
        weight = _copied(weight)
    for i, w, l in parts[1:]:
        if tuple(i.shape) != tuple(integral.shape) or tuple(l.shape) != tuple(integral.shape) or \
                (w is None) != (weight is None):
            raise ValueError("parts must agree in shape and in having a weight")
        integral += i
        length += l
        if w is not None:
            weight += w
    return integral, weight, length


def project_axis_scene(ctx, scene_f: SceneGeometry, scene_w: Optional[SceneGeometry], axis: str,
                       center: Sequence[float], plane_width: Sequence[float], width: int,
                       height: int, level_dl: Sequence[float], rank: int = 0, n_ranks: int = 1,
                       process_group=None):
    """The on-axis projection of loaded scenes ("On-axis projection"): (integral,
    weight or None without scene_w, length), float64 [height, width] tensors on ctx.device, row 0
    at the bottom.  scene_f and scene_w are the scenes load_plotfile_geometry returns for two
    variables of one plotfile with the same levels, rank and world size.  Pixel (x, y) owns the
    line center + ((x + 0.5) / W - 0.5) wu U + ((y + 0.5) / H - 0.5) wv V along axis "x" | "y" |
    "z", (U, V) as in SLICE_AXES; center and plane_width = (wu, wv) are in the plotfile's physical
    units (center's component along the axis is ignored), level_dl[l] = the path length of a cell
    of level l, one entry per level up to the finest loaded one.  Every rank projects its
    local_boxes; for n_ranks > 1 the images are SUM-reduced onto rank 0 (other ranks get (None,
    None, None)), through the host if the group's backend is not NCCL."""
    if axis not in _AXIS_INDEX:
        raise ValueError(f"axis must be one of x, y, z, not {axis!r}")
    a = _AXIS_INDEX[axis]
    axis_u, axis_v = (a + 1) % 3, (a + 2) % 3
    wu, wv = (float(w) for w in plane_width)
    if not (math.isfinite(wu) and wu > 0.0 and math.isfinite(wv) and wv > 0.0):
        raise ValueError("plane_width must be finite and positive")
    if int(width) <= 0 or int(height) <= 0:
        raise ValueError("image dimensions must be positive")
    center = tuple(float(c) for c in center)
    if len(center) != 3 or not _finite((center[axis_u], center[axis_v])):
        raise ValueError("center must hold three finite values")
    dl = [float(v) for v in level_dl]
    finest = max((int(b.level) for b in scene_f.all_boxes), default=0)
    if not (finest < len(dl) <= 16):
        raise ValueError("level_dl must hold one entry per level up to the finest loaded one "
                         "(at most 16)")
    scale = float(scene_f.world_scale)
    origin = ((center[axis_u] - 0.5 * wu) * scale, (center[axis_v] - 0.5 * wv) * scale)
    du = wu * scale / float(width)
    dv = wv * scale / float(height)
    with _native_scenes(ctx, [scene_f, scene_w]) as (field, weight):
        images = field.axis_projection(a, origin, du, dv, width, height, dl, weight)
        if n_ranks > 1:
            import torch.distributed as dist
            root = dist.get_global_rank(process_group, 0) if process_group is not None else 0
            images = _sum_over_ranks(ctx, images, process_group, root)
            images = (None, None, None) if rank != 0 else \
                tuple(t if t is None else t.to(ctx.device) for t in images)
        ctx.synchronize()
    return images


def project_axis(plotfile: str, axis: str = "z", variable: Optional[str] = None,
                 weight: Optional[str] = None, width: int = 512, height: int = 512,
                 min_level: int = 0, max_level: int = -1,
                 center: Optional[Sequence[float]] = None,
                 plane_width: Optional[Sequence[float]] = None, quantity: str = "column",
                 log_scale: bool = False, value_range: Optional[Sequence[float]] = None,
                 color_map: Optional[Sequence[Sequence[float]]] = None,
                 output: Optional[str] = None):
    """On-axis projection of a plotfile's raw field (yt's ProjectionPlot; DESIGN.md 7, "On-axis
    projection"), on cuda:0: per pixel the line integral along axis "x" | "y" | "z" through every
    uncovered cell of the loaded levels on the pixel's line, a cell's path length being its level's
    cell size along the axis in the plotfile's physical units -- exact, with no step and no camera.
    (right, up) = (y, z), (z, x), (x, y) as in slice(); center defaults to the centre of the data's
    bounding box and plane_width = (wu, wv) to the data's extent along right and up.  quantity
    "column": integral = sum dl * f over the finite cells (for a density, the surface density);
    "mean": integral / length, length = sum dl over those cells.  With weight (a variable's name)
    the result is the weighted mean sum dl * f * w / sum dl * w over the cells where both are
    finite; pass quantity="mean" with it, "column" is refused.  Returns the numpy float64 [height, width] image on
    rank 0, row 0 at the bottom, NaN where the denominator is 0, and None on other ranks.  With
    output (.png, else PPM) rank 0 also writes the picture, coloured as project() colours a column
    over value_range (or the min and max shown), log10 with log_scale; pixels whose line meets no
    counted cell and non-finite values are black."""
    center, widths, rng = validate_axis_projection_arguments(
        width, height, axis, quantity, center, plane_width, log_scale, value_range, weight)
    table = projection_rgb_table(color_map)
    variables = [variable or ""] + ([weight] if weight is not None else [])
    ctx, rank, world, group, scenes, _ = _load_fields(plotfile, variables, min_level, max_level)
    from . import plotfile as pf
    import torch
    a = _AXIS_INDEX[axis]
    axis_u, axis_v = (a + 1) % 3, (a + 2) % 3
    scene = scenes[0]
    finest = max(int(b.level) for b in scene.all_boxes)
    level_dl = [float(c[a]) for c in pf.PlotFileData(plotfile).cell_size[:finest + 1]]
    to_physical = 1.0 / float(scene.world_scale)
    lo = [min(b.min_corner[i] for b in scene.all_boxes) * to_physical for i in range(3)]
    hi = [max(b.max_corner[i] for b in scene.all_boxes) * to_physical for i in range(3)]
    if center is None:
        center = tuple(0.5 * (lo[i] + hi[i]) for i in range(3))
    if widths is None:
        widths = (hi[axis_u] - lo[axis_u], hi[axis_v] - lo[axis_v])
    integral, weight_image, length = project_axis_scene(
        ctx, scene, scenes[1] if weight is not None else None, axis, center, widths, width, height,
        level_dl, rank, world, group)
    if rank != 0:
        return None
    denominator = weight_image if weight is not None else length
    if weight is None and quantity == "column":
        shown = integral
        nan = torch.zeros_like(integral)
    else:
        filled = denominator != 0.0
        nan = torch.full_like(integral, float("nan"))
        shown = torch.where(filled, integral / torch.where(filled, denominator, 1.0), nan)
    if output is not None:
        hit = length > 0.0
        rgb8, _ = ctx.projection_colorize(
            torch.where(hit, shown, torch.zeros_like(shown)), hit.to(torch.float64),
            torch.from_numpy(table).to(integral.device), "column", log_scale,
            None if rng is None else ((math.log10(rng[0]), math.log10(rng[1])) if log_scale else rng))
        _write_picture(rgb8, output)
    return shown.cpu().numpy()


# ---- velocity cubes ("Velocity cubes") ------------------------------------------------

def velocity_cube_scene(ctx, scene_e: SceneGeometry, scene_g: SceneGeometry,
                        scene_s: Optional[SceneGeometry], axis: str, center: Sequence[float],
                        plane_width: Sequence[float], width: int, height: int,
                        level_dl: Sequence[float], edges, rank: int = 0, n_ranks: int = 1,
                        process_group=None):
    """The velocity cube of loaded scenes ("Velocity cubes"): (cube [nc, height,
    width], under, over, length [height, width]), float64 tensors on ctx.device, row 0 at the
    bottom.  scene_e (emission), scene_g (the field the channels bin: a line-of-sight velocity, or
    any other) and scene_s (a 1-sigma width in the units of scene_g, or None) are scenes
    load_plotfile_geometry returns for variables of one plotfile with the same levels, rank and
    world size.  Axis, center, plane_width, level_dl, the pixel lines and the reduction over ranks
    are project_axis_scene's; edges are the nc + 1 channel edges (bin_edges, or any finite,
    strictly increasing array, nc <= 1024)."""
    if axis not in _AXIS_INDEX:
        raise ValueError(f"axis must be one of x, y, z, not {axis!r}")
    a = _AXIS_INDEX[axis]
    axis_u, axis_v = (a + 1) % 3, (a + 2) % 3
    wu, wv = (float(w) for w in plane_width)
    if not (math.isfinite(wu) and wu > 0.0 and math.isfinite(wv) and wv > 0.0):
        raise ValueError("plane_width must be finite and positive")
    if int(width) <= 0 or int(height) <= 0:
        raise ValueError("image dimensions must be positive")
    center = tuple(float(c) for c in center)
    if len(center) != 3 or not _finite((center[axis_u], center[axis_v])):
        raise ValueError("center must hold three finite values")
    dl = [float(v) for v in level_dl]
    finest = max((int(b.level) for b in scene_e.all_boxes), default=0)
    if not (finest < len(dl) <= 16):
        raise ValueError("level_dl must hold one entry per level up to the finest loaded one "
                         "(at most 16)")
    from . import cubes
    edges = cubes.checked_edges(edges)
    scale = float(scene_e.world_scale)
    origin = ((center[axis_u] - 0.5 * wu) * scale, (center[axis_v] - 0.5 * wv) * scale)
    du = wu * scale / float(width)
    dv = wv * scale / float(height)
    with _native_scenes(ctx, [scene_e, scene_g, scene_s]) as (emission, velocity, sigma):
        images = emission.velocity_cube(velocity, edges, a, origin, du, dv, width, height, dl,
                                        sigma)
        if n_ranks > 1:
            import torch.distributed as dist
            root = dist.get_global_rank(process_group, 0) if process_group is not None else 0
            images = _sum_over_ranks(ctx, images, process_group, root)
            images = (None, None, None, None) if rank != 0 else \
                tuple(t.to(ctx.device) for t in images)
        ctx.synchronize()
    return tuple(images)


def velocity_cube(plotfile: str, axis: str = "z", emission: Optional[str] = None,
                  velocity: Optional[str] = None, width_field: Optional[str] = None,
                  channels: int = 64, v_range: Optional[Sequence[float]] = None, edges=None,
                  width: int = 256, height: int = 256, min_level: int = 0, max_level: int = -1,
                  center: Optional[Sequence[float]] = None,
                  plane_width: Optional[Sequence[float]] = None, output: Optional[str] = None):
    """Position-position-velocity cube of a plotfile ("Velocity cubes"), on cuda:0:
    per pixel the on-axis column of `emission` along axis "x" | "y" | "z" (project_axis's lines,
    window and path lengths) split into `channels` channels of `velocity` over v_range -- by
    default the velocity field's finite (min, max) -- or into the channels of explicit `edges`.
    emission, velocity and width_field are variable names: stored, derived (add_field), gradient or
    grid fields.  Without width_field a cell's whole emission goes to the channel that holds its
    velocity; with it the cell's share is spread as a Gaussian of that 1-sigma width (in the units
    of velocity; 0 is sharp, cells with a negative or non-finite width are dropped).  Binning by
    the derived field "z" gives depth-limited slabs, by a temperature an emission-measure
    distribution.  Returns, on rank 0 (None on other ranks), a dict of numpy float64 arrays: cube
    [nc, height, width], under, over (what fell below edges[0] / above edges[nc]), length
    [height, width], edges [nc + 1], centers [nc], moments (moment 0, 1, 2 as cubes.moments
    defines them).  With output ending in .npz or .fits rank 0 also writes the file."""
    from . import cubes
    center, widths, rng, edges = cubes.validate_cube_arguments(
        axis, emission, velocity, width_field, channels, v_range, edges, width, height, center,
        plane_width, output)
    variables = [emission, velocity] + ([width_field] if width_field is not None else [])
    ctx, rank, world, group, scenes, _ = _load_fields(plotfile, variables, min_level, max_level)
    from . import plotfile as pf
    a = _AXIS_INDEX[axis]
    axis_u, axis_v = (a + 1) % 3, (a + 2) % 3
    scene = scenes[0]
    finest = max(int(b.level) for b in scene.all_boxes)
    level_dl = [float(c[a]) for c in pf.PlotFileData(plotfile).cell_size[:finest + 1]]
    to_physical = 1.0 / float(scene.world_scale)
    lo = [min(b.min_corner[i] for b in scene.all_boxes) * to_physical for i in range(3)]
    hi = [max(b.max_corner[i] for b in scene.all_boxes) * to_physical for i in range(3)]
    if center is None:
        center = tuple(0.5 * (lo[i] + hi[i]) for i in range(3))
    if widths is None:
        widths = (hi[axis_u] - lo[axis_u], hi[axis_v] - lo[axis_v])
    if edges is None:
        if rng is None:
            rng = _field_range(ctx, scenes[1], False, "velocity", world, group)
        edges = cubes.channel_edges(rng, channels)
    images = velocity_cube_scene(ctx, scene, scenes[1],
                                 scenes[2] if width_field is not None else None, axis, center,
                                 widths, width, height, level_dl, edges, rank, world, group)
    if rank != 0:
        return None
    cube, under, over, length = (t.cpu().numpy() for t in images)
    result = {"cube": cube, "under": under, "over": over, "length": length, "edges": edges,
              "centers": cubes.channel_centers(edges), "moments": cubes.moments(cube, edges)}
    if output is not None:
        if output.lower().endswith(".npz"):
            cubes.write_npz(output, result)
        else:
            origin = (center[axis_u] - 0.5 * widths[0], center[axis_v] - 0.5 * widths[1])
            cubes.write_fits(output, cube, edges, origin,
                             (widths[0] / float(width), widths[1] / float(height)), axis)
    return result


# ---- off-axis projection ("Off-axis projection") --------------------------------------

def validate_off_axis_projection_arguments(width: int, height: int, normal: Sequence[float],
                                           quantity: str = "column",
                                           center: Optional[Sequence[float]] = None,
                                           plane_width: Optional[Sequence[float]] = None,
                                           depth: Optional[float] = None,
                                           north: Optional[Sequence[float]] = None,
                                           log_scale: bool = False,
                                           value_range: Optional[Sequence[float]] = None,
                                           weight: Optional[str] = None):
    """The argument checks of project_off_axis(), before any GPU work and before the plotfile is
    opened: project_axis' rules for the image, the quantity, the center, plane_width, value_range
    and the weight, slice_basis' for the directions, and a finite, positive depth.  Returns
    (normal, north, center or None, plane_width or None, depth or None, value_range or None) as
    floats; north defaults to z, and to y where the normal is within slice_basis' 1e-6 of +-z."""
    center, widths, rng = validate_axis_projection_arguments(
        width, height, "z", quantity, center, plane_width, log_scale, value_range, weight)
    n = _unit(normal, "normal")
    if north is None:
        across = _cross((0.0, 0.0, 1.0), n)
        along_z = not math.sqrt(across[0] * across[0] + across[1] * across[1] +
                                across[2] * across[2]) > 1e-6
        north = (0.0, 1.0, 0.0) if along_z else (0.0, 0.0, 1.0)
    slice_basis(normal, north)
    if depth is not None:
        depth = float(depth)
        if not (math.isfinite(depth) and depth > 0.0):
            raise ValueError("depth must be finite and positive")
    return (tuple(float(c) for c in normal), tuple(float(c) for c in north), center, widths, depth,
            rng)


def project_off_axis_scene(ctx, scene_f: SceneGeometry, scene_w: Optional[SceneGeometry],
                           center: Sequence[float], normal: Sequence[float],
                           north: Sequence[float], plane_width: Sequence[float], depth: float,
                           width: int, height: int, cell_sizes, prob_lo, ref_ratio,
                           rank: int = 0, n_ranks: int = 1, tile_order: bool = False) -> dict:
    """The exact off-axis projection of loaded scenes ("Off-axis projection"): one
    ray per pixel (rays.pixel_rays over (n, U, V) = slice_basis(normal, north); center,
    plane_width = (wu, wv) and depth in the plotfile's physical units), every ray summed by
    ray_sums_scene, whose other arguments these are.  The rays go to the device in row-major pixel
    order; with tile_order tile by tile (rays.pixel_order; measured not to be faster),
    and either way the images come back in pixel order with the same bits.  Returns a dict of [height, width]
    images, row 0 at the bottom: integral, weight (None without scene_w), counted and covered
    float64, status uint8 and count uint32, as ray_sums_scene defines them per ray."""
    import numpy as np
    from . import rays as ray_rules
    _require_one_rank(scene_f, n_ranks, "rays need every box of the scene on one rank: "
                      "rays are not handed over between ranks")
    width, height = int(width), int(height)
    if width <= 0 or height <= 0:
        raise ValueError("image dimensions must be positive")
    center = tuple(float(c) for c in center)
    if len(center) != 3 or not _finite(center):
        raise ValueError("center must hold three finite values")
    widths = tuple(float(w) for w in plane_width)
    if len(widths) != 2 or not all(math.isfinite(w) and w > 0.0 for w in widths):
        raise ValueError("plane_width must be finite and positive")
    depth = float(depth)
    if not (math.isfinite(depth) and depth > 0.0):
        raise ValueError("depth must be finite and positive")
    n, u, v = slice_basis(normal, north)
    start, end = ray_rules.pixel_rays(center, n, u, v, widths, depth, width, height)
    order = ray_rules.pixel_order(width, height) if tile_order else \
        np.arange(width * height, dtype=np.int64)
    found = ray_sums_scene(ctx, scene_f, start[order], end[order], cell_sizes, prob_lo, ref_ratio,
                           scene_w, None, rank, n_ranks)
    images = {}
    for key in ("integral", "weight", "counted", "covered", "status", "count"):
        values = found[key]
        if values is not None:
            image = np.empty(width * height, dtype=values.dtype)
            image[order] = values
            values = image.reshape(height, width)
        images[key] = values
    return images


def project_off_axis(plotfile: str, normal: Sequence[float], variable: Optional[str] = None,
                     weight: Optional[str] = None, width: int = 512, height: int = 512,
                     min_level: int = 0, max_level: int = -1,
                     center: Optional[Sequence[float]] = None,
                     plane_width: Optional[Sequence[float]] = None,
                     depth: Optional[float] = None, north: Optional[Sequence[float]] = None,
                     quantity: str = "column", log_scale: bool = False,
                     value_range: Optional[Sequence[float]] = None,
                     color_map: Optional[Sequence[Sequence[float]]] = None,
                     output: Optional[str] = None):
    """Exact off-axis projection of a plotfile (yt's OffAxisProjectionPlot; DESIGN.md 7, "Off-axis
    projection"), on cuda:0: per pixel the line integral sum f ds along the pixel's ray through
    every uncovered cell of the loaded levels that the ray crosses, ds being the length of the ray
    inside the cell -- no step and no sampling.  The image plane passes through center with
    (n, right, up) = slice_basis(normal, north), n pointing at the viewer; the rays are depth long,
    half of it on either side of the plane.  variable and weight: stored variables or registered
    derived, gradient, clump or grid fields.  center defaults to the centre of the data's bounding box,
    plane_width = (wu, wv) and depth to the box's diagonal, so that the whole box is seen from any
    direction, and north to z (to y for a normal along z).  quantity "column": integral = sum f ds
    over the finite cells; "mean": integral / counted, counted = sum ds over those cells.  With
    weight the result is the weighted mean sum f w ds / sum w ds over the cells where both are
    finite; pass quantity="mean" with it, "column" is refused.  Returns the numpy float64 [height,
    width] image on rank 0, row 0 at the bottom, NaN where the denominator is 0.  With output
    (.png, else PPM) the picture is written, coloured as project_axis() colours its own; pixels
    whose ray meets no counted cell are black.  Several ranks raise NotImplementedError before
    any device work; a ray that ran out of trips raises RuntimeError."""
    normal, north, center, widths, depth, rng = validate_off_axis_projection_arguments(
        width, height, normal, quantity, center, plane_width, depth, north, log_scale, value_range,
        weight)
    table = projection_rgb_table(color_map)
    import numpy as np
    import torch
    import torch.distributed as dist
    from . import plotfile as pf
    from . import rays as ray_rules
    several = "an off-axis projection needs every box of the scene on one rank: rays are not " \
              "handed over between ranks"
    # known before the runtime is set up and anything is loaded
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or \
            (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        raise NotImplementedError(several)
    variables = [variable or ""] + ([weight] if weight is not None else [])
    ctx, rank, world, group, scenes, volumes = _load_fields(plotfile, variables, min_level,
                                                            max_level)
    scene = scenes[0]
    _require_one_rank(scene, world, several)
    to_physical = 1.0 / float(scene.world_scale)
    lo = [min(b.min_corner[i] for b in scene.all_boxes) * to_physical for i in range(3)]
    hi = [max(b.max_corner[i] for b in scene.all_boxes) * to_physical for i in range(3)]
    extent = [hi[i] - lo[i] for i in range(3)]
    diagonal = math.sqrt((extent[0] * extent[0] + extent[1] * extent[1]) + extent[2] * extent[2])
    if center is None:
        center = tuple(0.5 * (lo[i] + hi[i]) for i in range(3))
    if widths is None:
        widths = (diagonal, diagonal)
    if depth is None:
        depth = diagonal
    images = project_off_axis_scene(
        ctx, scene, scenes[1] if weight is not None else None, center, normal, north, widths,
        depth, width, height, *_header_levels(pf.PlotFileData(plotfile), len(volumes)), rank,
        world)
    cut = np.argwhere(images["status"] == ray_rules.TRUNCATED)
    if cut.size:
        y, x = (int(v) for v in cut[0])
        raise RuntimeError(f"project_off_axis: the ray of pixel (x={x}, y={y}) ran out of trips; "
                           f"its column would be short")
    integral, counted = images["integral"], images["counted"]
    if weight is None and quantity == "column":
        shown = integral
    else:
        denominator = images["weight"] if weight is not None else counted
        filled = denominator != 0.0
        shown = np.full_like(integral, math.nan)
        np.divide(integral, denominator, out=shown, where=filled)
    if output is not None:
        hit = torch.from_numpy(counted > 0.0).to(ctx.device)
        values = torch.from_numpy(shown).to(ctx.device)
        rgb8, _ = ctx.projection_colorize(
            torch.where(hit, values, torch.zeros_like(values)), hit.to(torch.float64),
            torch.from_numpy(table).to(ctx.device), "column", log_scale,
            None if rng is None else ((math.log10(rng[0]), math.log10(rng[1])) if log_scale else rng))
        _write_picture(rgb8, output)
    return shown


# ---- ray transfer ("Ray transfer") ----------------------------------------------------

def ray_transfer_scene(ctx, source: "SceneGeometry", opacity: "SceneGeometry", start, end,
                       cell_sizes, prob_lo, ref_ratio,
                       bin_scene: Optional["SceneGeometry"] = None,
                       width_scene: Optional["SceneGeometry"] = None, edges=None,
                       max_trips: Optional[int] = None, rank: int = 0, n_ranks: int = 1) -> dict:
    """Emission and absorption along every segment start[s] -> end[s], the cell nearest the start
    first ("Ray transfer").  source (the source function S), opacity (the absorption
    coefficient a per unit length; with channels integrated over the line), bin_scene (the field
    the channels bin, a line-of-sight velocity; None: grey) and width_scene (a 1-sigma width in the
    bin field's units, or None): scenes with the same boxes.  edges: the nc + 1 channel edges,
    given exactly with bin_scene (cubes.checked_edges).  The other arguments are ray_sums_scene's.
    Returns a dict of numpy arrays: per ray count uint32, status uint8, t_enter, t_leave, counted
    and covered float64 as ray_sums_scene gives them (a segment counts where S and a are finite
    and a >= 0, g is finite, s is finite and >= 0); intensity and tau float64 [nc, n] (nc = 1 for
    grey); outside float64 [2, n], the velocity-integrated optical depth below edges[0] and above
    edges[nc] (None for grey)."""
    import numpy as np
    import torch
    from . import cubes
    from . import rays as ray_rules
    local = list(source.local_boxes)
    _require_one_rank(source, n_ranks, "rays need every box of the scene on one rank: "
                      "rays are not handed over between ranks")
    if opacity is None:
        raise ValueError("ray transfer needs an opacity scene")
    if width_scene is not None and bin_scene is None:
        raise ValueError("a width scene needs a bin scene")
    if (bin_scene is None) != (edges is None):
        raise ValueError("edges are given exactly with a bin scene")
    if edges is not None:
        edges = cubes.checked_edges(edges)
    first, last = ray_rules.end_points(start, end)
    channels = 1 if edges is None else edges.size - 1
    if channels * first.shape[0] >= 2 ** 31:
        raise ValueError("the channels of all rays are 2^31 entries or more")
    sizes, ratios, index = _level_setup(source, local, cell_sizes, prob_lo, ref_ratio)
    if max_trips is None:
        bounds = ray_rules.level0_bounds(index, [b.cell_dimensions for b in local],
                                         [b.level for b in local], ratios)
        max_trips = ray_rules.default_max_trips(bounds, ratios, len(sizes))
    max_trips = int(max_trips)
    if not 1 <= max_trips <= ray_rules.MAX_TRIPS:
        raise ValueError("max_trips must lie in [1, 2^30]")
    origin = [float(v) for v in prob_lo]
    with _native_scenes(ctx, [source, opacity, bin_scene, width_scene]) as (s, a, g, w):
        found = s.ray_transfer(a, torch.from_numpy(first).to(ctx.device),
                               torch.from_numpy(last).to(ctx.device), max_trips, index, ratios,
                               sizes, origin, g, w, edges)
        ctx.synchronize()
        counts, status, span, intensity, tau, outside, counted, covered = (
            t if t is None else t.cpu().numpy() for t in found)
    return {"count": counts.view(np.uint32), "status": status, "t_enter": span[:, 0].copy(),
            "t_leave": span[:, 1].copy(), "intensity": intensity, "tau": tau, "outside": outside,
            "counted": counted, "covered": covered}


def transfer_off_axis_scene(ctx, source: SceneGeometry, opacity: SceneGeometry,
                            center: Sequence[float], normal: Sequence[float],
                            north: Sequence[float], plane_width: Sequence[float], depth: float,
                            width: int, height: int, cell_sizes, prob_lo, ref_ratio,
                            bin_scene: Optional[SceneGeometry] = None,
                            width_scene: Optional[SceneGeometry] = None, edges=None,
                            max_trips: Optional[int] = None, rank: int = 0,
                            n_ranks: int = 1) -> dict:
    """ray_transfer_scene on the pixel rays of project_off_axis_scene, whose view arguments these
    are: every ray runs from center + (depth / 2) n to center - (depth / 2) n, so the cell nearest
    the viewer comes first.  Returns a dict of images, row 0 at the bottom: intensity and tau
    float64 [nc, height, width], outside float64 [2, height, width] (None for grey), counted and
    covered float64, status uint8 and count uint32 [height, width]."""
    from . import rays as ray_rules
    _require_one_rank(source, n_ranks, "rays need every box of the scene on one rank: "
                      "rays are not handed over between ranks")
    width, height = int(width), int(height)
    if width <= 0 or height <= 0:
        raise ValueError("image dimensions must be positive")
    center = tuple(float(c) for c in center)
    if len(center) != 3 or not _finite(center):
        raise ValueError("center must hold three finite values")
    widths = tuple(float(w) for w in plane_width)
    if len(widths) != 2 or not all(math.isfinite(w) and w > 0.0 for w in widths):
        raise ValueError("plane_width must be finite and positive")
    depth = float(depth)
    if not (math.isfinite(depth) and depth > 0.0):
        raise ValueError("depth must be finite and positive")
    n, u, v = slice_basis(normal, north)
    start, end = ray_rules.pixel_rays(center, n, u, v, widths, depth, width, height)
    found = ray_transfer_scene(ctx, source, opacity, start, end, cell_sizes, prob_lo, ref_ratio,
                               bin_scene, width_scene, edges, max_trips, rank, n_ranks)
    images = {}
    for key in ("intensity", "tau", "outside"):
        values = found[key]
        images[key] = None if values is None else values.reshape(values.shape[0], height, width)
    for key in ("counted", "covered", "status", "count"):
        images[key] = found[key].reshape(height, width)
    return images


_SEVERAL_RANKS = "ray transfer needs every box of the scene on one rank: rays are not handed " \
                 "over between ranks"


def _one_rank_before_loading() -> None:
    """NotImplementedError for several ranks: known before the runtime is set up."""
    import torch.distributed as dist
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or \
            (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        raise NotImplementedError(_SEVERAL_RANKS)


def _off_axis_defaults(scene: SceneGeometry, center, widths, depth):
    """project_off_axis' defaults: the centre of the loaded boxes' bounding box and its diagonal."""
    to_physical = 1.0 / float(scene.world_scale)
    lo = [min(b.min_corner[i] for b in scene.all_boxes) * to_physical for i in range(3)]
    hi = [max(b.max_corner[i] for b in scene.all_boxes) * to_physical for i in range(3)]
    extent = [hi[i] - lo[i] for i in range(3)]
    diagonal = math.sqrt((extent[0] * extent[0] + extent[1] * extent[1]) + extent[2] * extent[2])
    if center is None:
        center = tuple(0.5 * (lo[i] + hi[i]) for i in range(3))
    return center, widths or (diagonal, diagonal), depth or diagonal


def _refuse_truncated(images: dict, what: str) -> None:
    import numpy as np
    from . import rays as ray_rules
    cut = np.argwhere(images["status"] == ray_rules.TRUNCATED)
    if cut.size:
        y, x = (int(v) for v in cut[0])
        raise RuntimeError(f"{what}: the ray of pixel (x={x}, y={y}) ran out of trips; its "
                           f"optical depth would be short")


def emission_absorption(plotfile: str, normal: Sequence[float], source: str, opacity: str,
                        background: float = 0.0, width: int = 512, height: int = 512,
                        min_level: int = 0, max_level: int = -1,
                        center: Optional[Sequence[float]] = None,
                        plane_width: Optional[Sequence[float]] = None,
                        depth: Optional[float] = None, north: Optional[Sequence[float]] = None,
                        log_scale: bool = False, value_range: Optional[Sequence[float]] = None,
                        color_map: Optional[Sequence[Sequence[float]]] = None,
                        output: Optional[str] = None) -> dict:
    """Grey emission and absorption through a plotfile along any line of sight ("Ray
    transfer"), on cuda:0: per pixel the formal solution I = sum S (1 - exp(-dtau)) exp(-tau in
    front) over the cells of project_off_axis' ray, nearest the viewer first, dtau = a ds -- dust
    continuum with a source function, X-ray absorption with a background.  source and opacity:
    stored variables or registered derived, gradient, clump or grid fields.  The view arguments
    are project_off_axis'.  background: the intensity behind the far end, added as background *
    exp(-tau).  Returns a dict of numpy float64 [height, width] images, row 0 at the bottom:
    intensity, tau, counted and covered (the lengths of the ray inside cells that count -- S and a
    finite, a >= 0 -- and inside loaded leaves).  With output (.png, else PPM) the intensity is
    written as a picture, coloured as project_off_axis colours its own; pixels whose ray meets no
    counted cell are black.  Several ranks raise NotImplementedError before any device work; a ray
    that ran out of trips raises RuntimeError."""
    from . import transfer
    normal, north, center, widths, depth, rng = validate_off_axis_projection_arguments(
        width, height, normal, "column", center, plane_width, depth, north, log_scale, value_range,
        None)
    background = transfer.validate_emission_absorption_arguments(source, opacity, background,
                                                                 width, height, output)
    table = projection_rgb_table(color_map)
    import torch
    from . import plotfile as pf
    _one_rank_before_loading()
    ctx, rank, world, group, scenes, volumes = _load_fields(plotfile, [source, opacity], min_level,
                                                            max_level)
    _require_one_rank(scenes[0], world, _SEVERAL_RANKS)
    center, widths, depth = _off_axis_defaults(scenes[0], center, widths, depth)
    images = transfer_off_axis_scene(
        ctx, scenes[0], scenes[1], center, normal, north, widths, depth, width, height,
        *_header_levels(pf.PlotFileData(plotfile), len(volumes)), None, None, None, None, rank,
        world)
    _refuse_truncated(images, "emission_absorption")
    tau = images["tau"][0]
    intensity = transfer.apply_background(images["intensity"], images["tau"], background)[0]
    result = {"intensity": intensity, "tau": tau, "counted": images["counted"],
              "covered": images["covered"]}
    if output is not None:
        hit = torch.from_numpy(images["counted"] > 0.0).to(ctx.device)
        values = torch.from_numpy(intensity).to(ctx.device)
        rgb8, _ = ctx.projection_colorize(
            torch.where(hit, values, torch.zeros_like(values)), hit.to(torch.float64),
            torch.from_numpy(table).to(ctx.device), "column", log_scale,
            None if rng is None else ((math.log10(rng[0]), math.log10(rng[1])) if log_scale else rng))
        _write_picture(rgb8, output)
    return result


_LINE_OF_SIGHT_FIELD = "_line_of_sight_velocity"


def line_cube(plotfile: str, normal: Sequence[float], source: str, opacity: str, velocity,
              width_field: Optional[str] = None, channels: int = 64,
              v_range: Optional[Sequence[float]] = None, edges=None, background=0.0,
              width: int = 256, height: int = 256, min_level: int = 0, max_level: int = -1,
              center: Optional[Sequence[float]] = None,
              plane_width: Optional[Sequence[float]] = None, depth: Optional[float] = None,
              north: Optional[Sequence[float]] = None, output: Optional[str] = None) -> dict:
    """Optically thick position-position-velocity cube of a plotfile along any line of sight
    ("Ray transfer"), on cuda:0: per pixel and channel the formal solution of emission
    and absorption along project_off_axis' ray, nearest the viewer first.  source: the source
    function; opacity: the absorption coefficient per unit length integrated over the line (a
    channel of width dv that holds a whole cell has dtau = a ds / dv).  velocity: one variable
    name, used as the line-of-sight velocity as it is, or three, the components of a velocity, of
    which -(n . v) is taken (receding gas is positive; n points at the viewer).  width_field: a
    1-sigma width in the units of velocity, or None (sharp).  channels, v_range (by default the
    velocity's finite (min, max)) and edges as api.velocity_cube takes them; the view arguments
    are project_off_axis'; background: one value or one per channel, added as background[c] *
    exp(-tau[c]).  Returns a dict of numpy float64 arrays: cube and tau [nc, height, width], outside
    [2, height, width] (the velocity-integrated optical depth below edges[0] and above edges[nc]),
    counted and covered [height, width], edges [nc + 1], centers [nc] and moments (cubes.moments of
    cube * channel width).  With output ending in .npz or .fits the file is written.  Several ranks
    raise NotImplementedError before any device work; a ray that ran out of trips raises
    RuntimeError."""
    from . import cubes
    from . import transfer
    normal, north, center, widths, depth, _ = validate_off_axis_projection_arguments(
        width, height, normal, "column", center, plane_width, depth, north, False, None, None)
    names, rng, edges, background = transfer.validate_line_cube_arguments(
        source, opacity, velocity, width_field, channels, v_range, edges, background, width,
        height, output)
    import numpy as np
    from . import plotfile as pf
    _one_rank_before_loading()
    temporary = len(names) == 3
    if temporary:
        if _LINE_OF_SIGHT_FIELD in derived_fields():
            raise ValueError(f"{_LINE_OF_SIGHT_FIELD!r} is line_cube's own field name")
        unit = slice_basis(normal, north)[0]
        add_field(_LINE_OF_SIGHT_FIELD, transfer.line_of_sight_expression(unit, names))
    try:
        variables = [source, opacity, _LINE_OF_SIGHT_FIELD if temporary else names[0]]
        if width_field is not None:
            variables.append(width_field)
        ctx, rank, world, group, scenes, volumes = _load_fields(plotfile, variables, min_level,
                                                                max_level)
    finally:
        if temporary:
            remove_field(_LINE_OF_SIGHT_FIELD)
    _require_one_rank(scenes[0], world, _SEVERAL_RANKS)
    center, widths, depth = _off_axis_defaults(scenes[0], center, widths, depth)
    if edges is None:
        if rng is None:
            rng = _field_range(ctx, scenes[2], False, "velocity", world, group)
        edges = cubes.channel_edges(rng, channels)
    images = transfer_off_axis_scene(
        ctx, scenes[0], scenes[1], center, normal, north, widths, depth, width, height,
        *_header_levels(pf.PlotFileData(plotfile), len(volumes)), scenes[2],
        scenes[3] if width_field is not None else None, edges, None, rank, world)
    _refuse_truncated(images, "line_cube")
    cube = transfer.apply_background(images["intensity"], images["tau"], background)
    edges = np.asarray(edges, dtype=np.float64)
    dv = (edges[1:] - edges[:-1])[:, None, None]
    result = {"cube": cube, "tau": images["tau"], "outside": images["outside"],
              "counted": images["counted"], "covered": images["covered"], "edges": edges,
              "centers": cubes.channel_centers(edges), "moments": cubes.moments(cube * dv, edges)}
    if output is not None:
        if output.lower().endswith(".npz"):
            cubes.write_npz(output, result, ("cube", "tau", "outside", "counted", "covered",
                                             "edges", "centers"))
        else:
            # the image plane's own (right, up) coordinates about the centre
            cubes.write_fits(output, cube, edges, (-0.5 * widths[0], -0.5 * widths[1]),
                             (widths[0] / float(width), widths[1] / float(height)), "z")
    return result
