"""The oracle's march against exact ray-cell geometry (tests/continuum.py): lengths, columns,
maximum intensity, homogeneous alpha and depth must lie inside brackets derived from the geometry
alone -- and the brackets must be tight enough to tell a different reading of the camera, the
steps, the hierarchy or the axes apart (the mutants at the end).  The coloured frame likewise:
the oracle's RGBA inside the float64 emission-absorption brackets under two colour maps, and seven
other readings of the coloured picture outside them.  No GPU.

What the oracle computed is read out of its volume march with the indicator and step-map devices
kept in tests/helpers.py."""
import numpy as np
import pytest

import continuum as K
from amrvolumerenderer_amd import plotfile, runtime, scenes
from amrvolumerenderer_amd.types import AmrBox, CameraParameters, ScalarTransform, make_params
from helpers import (SAMPLING_BOUNDS, check_step_table, count_samples, oracle_camera,
                     oracle_params, oracle_transform, step_map)

NORM = ScalarTransform(normalize_to_unit_range=True)
MAX_EXCLUDED = 0.01          # share of the hitting pixels a case may leave out
MIP_LEVELS = (20, 80, 140, 200)


# ---- fields: different along x, y and z -----------------------------------------------------------

def ramp(x, y, z):
    """Integers 0..15, steep along x, gentler along y, gentlest along z."""
    return np.floor(11.0 * x + 3.0 * y + z + 1e-9).clip(0, 15)


def smooth(x, y, z):
    return 0.2 + x * x + 0.5 * np.sin(3.0 * y) ** 2 + 0.25 * z


def box_of(field, lo, hi, shape, ghost=0, unit=None, level=0):
    """A continuum Box whose cells are field(cell centre / unit); with ghost > 0 the cells are a
    strided view into a larger array."""
    nz, ny, nx = shape
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    unit = np.asarray(unit if unit is not None else (1.0, 1.0, 1.0), float)
    c = [lo[a] + (hi[a] - lo[a]) * (np.arange(n) + 0.5) / n for a, n in ((0, nx), (1, ny), (2, nz))]
    cells = field(c[0][None, None, :] / unit[0], c[1][None, :, None] / unit[1],
                  c[2][:, None, None] / unit[2]) + np.zeros(shape)
    if ghost:
        big = np.full((nz + 2 * ghost, ny + 2 * ghost, nx + 2 * ghost), 1e30)
        big[ghost:-ghost, ghost:-ghost, ghost:-ghost] = cells
        cells = big[ghost:-ghost, ghost:-ghost, ghost:-ghost]
    else:
        cells = np.ascontiguousarray(cells)
    return K.Box(tuple(lo), tuple(hi), cells, level=level)


def mip_index(cells):
    """Integer cells 0..15 -> four colour-table entries."""
    return (60 * (cells.astype(np.int64) // 4) + 20).astype(np.int64)


def amr_boxes(spec, field):
    return [box_of(field, m.min_corner, m.max_corner, m.dims[::-1], level=m.level)
            for m in spec.boxes]


# ---- what the oracle computed --------------------------------------------------------------------

def meta(box):
    return AmrBox(tuple(box.min_corner), tuple(box.max_corner), None,
                  dims=tuple(int(n) for n in box.dims), level=box.level)


def f32_step(O, box):
    ob = O.make_box(np.ascontiguousarray(box.cells), box.min_corner, box.max_corner)
    return np.float64(np.float32(O.box_sampling(ob, oracle_params(O, 8, 8, (0.0, 1.0), 0.0, 0.0,
                                                                  SAMPLING_BOUNDS))[0]))


def oracle_length_column(O, boxes, cam, W, H, integer):
    """(length, column): f64(step) x the oracle's sample counts, summed over the boxes.  Integer
    cells through their bit planes, others through one indicator per distinct value."""
    length, column = np.zeros((H, W)), np.zeros((H, W))
    for box in boxes:
        step = f32_step(O, box)
        finite = np.isfinite(box.cells) & (np.abs(box.cells) < 1e29)
        count = lambda ind: count_samples(O, ind.astype(np.float64), box.min_corner,  # noqa: E731
                                          box.max_corner, cam, W, H, 0.0, meta(box))[0]
        n = count(finite)
        if not n.any():
            continue
        length += step * n
        if integer:
            ci = np.where(finite, box.cells, 0).astype(np.int64)
            for t in range(int(ci.max()).bit_length()):
                column += step * (count((ci >> t) & 1) << t)
        else:
            for v in np.unique(box.cells[finite]):
                column += step * v * count(finite & (box.cells == v))
    return length, column


def oracle_mip(O, boxes, cam, W, H):
    """The largest colour-table entry among the oracle's samples per pixel (-1: none)."""
    out = np.full((H, W), -1, np.int64)
    ocam, otr = oracle_camera(O, cam), oracle_transform(O, NORM)
    for box in boxes:
        cells = np.ascontiguousarray((box.index + 0.5) / 255.0)
        ob = O.make_box(cells, box.min_corner, box.max_corner)
        for t in (0,) + MIP_LEVELS:
            if t > box.index.max():
                break
            check_step_table(O, t, (0.0, 1.0))
            op = oracle_params(O, W, H, (0.0, 1.0), 0.0, 0.0, SAMPLING_BOUNDS, step_map(t))
            lit = O.paint_box(ob, otr, op, ocam, threads=16)[0][..., 3] > 0.0
            if not lit.any():
                break
            # entries present are 20, 80, ...: lit at threshold t means a sample with entry >= t
            reached = 20 if t == 0 else t
            out[lit] = np.maximum(out[lit], reached)
    return out


HOMOGENEOUS_ALPHA = 0.02
HOMOGENEOUS_MAP = [(0.0, 0.5, 0.5, 0.5, HOMOGENEOUS_ALPHA), (1.0, 0.5, 0.5, 0.5, HOMOGENEOUS_ALPHA)]


def homogeneous_tables(O, boxes, transparency, ref_dist):
    """Per box the opacity of one sample, from the oracle's colour table at the box's step; and
    the table's opacity at the reference step."""
    per_box = []
    for box in boxes:
        ob = O.make_box(np.ascontiguousarray(box.cells), box.min_corner, box.max_corner)
        op = oracle_params(O, 8, 8, (0.0, 1.0), transparency, ref_dist, SAMPLING_BOUNDS,
                           HOMOGENEOUS_MAP)
        _, factor, alpha_scale = O.box_sampling(ob, op)
        per_box.append(float(O.build_color_table(alpha_scale, factor, (0.0, 1.0),
                                                 HOMOGENEOUS_MAP)[127, 3]))
    a_ref = float(O.build_color_table(1.0 - transparency, 1.0, (0.0, 1.0), HOMOGENEOUS_MAP)[127, 3])
    return per_box, a_ref


def oracle_homogeneous_alpha(O, boxes, cam, W, H, transparency, ref_dist):
    keep = np.ones((H, W))
    ocam, otr = oracle_camera(O, cam), oracle_transform(O, NORM)
    for box in boxes:
        ob = O.make_box(np.full(box.cells.shape, 0.5), box.min_corner, box.max_corner)
        op = oracle_params(O, W, H, (0.0, 1.0), transparency, ref_dist, SAMPLING_BOUNDS,
                           HOMOGENEOUS_MAP)
        keep *= 1.0 - O.paint_box(ob, otr, op, ocam, threads=16)[0][..., 3].astype(np.float64)
    return 1.0 - keep


# ---- the brackets --------------------------------------------------------------------------------

def report(name, what, value):
    print(f"\ncontinuum {name}: {what} = {value}")


def check_length_column(name, e, length, column):
    ok = ~e.excluded
    share = e.excluded_share()
    report(name, "excluded share of hitting pixels", f"{share:.4f}")
    assert share <= MAX_EXCLUDED
    assert e.hit.sum() > 200
    # not excluded, but their brackets carry the near-an-edge term (continuum.py): kept in view
    report(name, "share of hitting pixels with a near-an-edge term", f"{e.lateral_share():.4f}")
    for what, got in (("length", length), ("column", column)):
        exact, under, over = (getattr(e, what + k) for k in ("", "_under", "_over"))
        err = got - exact
        used = np.where(err > 0, err / np.maximum(over, 1e-300), -err / np.maximum(under, 1e-300))
        report(name, f"{what}: largest error / margin", f"{float(used[ok].max()):.3f}; mean bracket "
               f"width / mean value {(under + over)[e.hit].mean() / exact[e.hit].mean():.3f}")
        bad = ok & e.outside(what, got)
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3])
    # a pixel no box is near gets nothing at all
    assert not length[~e.hit & ok].any()


def check_mip(name, e, mip):
    ok = ~e.excluded
    assert (mip[ok] >= e.mip_lo[ok]).all(), np.argwhere(ok & (mip < e.mip_lo))[:3]
    assert (mip[ok] <= e.mip_hi[ok]).all(), np.argwhere(ok & (mip > e.mip_hi))[:3]
    report(name, "MIP pixels pinned exactly (lower = upper)",
           f"{float((e.mip_lo == e.mip_hi)[e.hit].mean()):.3f}")


def check_alpha(name, e, alpha, a_ref, ref_step):
    """alpha inside the bracket of the sample counts, widened by the float32 recurrence's rounding
    (a <- a + a_b (1 - a): the product and the sum, <= 2^-24 each on values <= 1, so 2^-23 per
    sample) plus 2^-23 once for what is rounded outside the recurrence: the table entry a_b as a
    float32 (<= 2^-24 relative, on a total opacity <= 1) and the stored float32 alpha (2^-24);
    and the continuum's own transmittance inside the phase-free bracket."""
    ok = ~e.excluded
    widen = e.samples_hi * 2.0 ** -23 + 2.0 ** -23
    assert (alpha[ok] >= (e.alpha_lo - widen)[ok]).all()
    assert (alpha[ok] <= (e.alpha_hi + widen)[ok]).all()
    physical = -np.expm1(e.length / ref_step * np.log1p(-a_ref))
    assert (physical[ok] >= (e.physical_lo - widen)[ok]).all()
    assert (physical[ok] <= (e.physical_hi + widen)[ok]).all()
    report(name, "alpha bracket: mean width / mean alpha",
           f"{(e.alpha_hi - e.alpha_lo)[e.hit].mean() / e.alpha_hi[e.hit].mean():.3f}")


# ---- colour: maps, tables, what the oracle painted -------------------------------------------------

def plateau_map(bands):
    """Control points of a colour map that is constant (r, g, b, opacity) on each of the entry
    ranges [0, 20], [21, 80], [81, 140], [141, 200], [201, 255]: the four MIP_LEVELS entries are
    the last of their plateaus, so entry k + 1 is another colour than entry k.  The values are
    those at which build_color_table evaluates the entries, float32(i) / float32(255)."""
    edges = (0, 20, 21, 80, 81, 140, 141, 200, 201, 255)
    return [(float(np.float32(e) / np.float32(255.0)),) + tuple(bands[n // 2])
            for n, e in enumerate(edges)]


COLOUR_MAPS = {
    # colours well apart, red against blue too; opacities times (1 - 0.25) in [0.03, 0.3]
    "contrast": plateau_map([(0.9, 0.1, 0.1, 0.04), (0.1, 0.8, 0.2, 0.12), (0.1, 0.2, 0.9, 0.25),
                             (0.9, 0.8, 0.1, 0.4), (0.5, 0.5, 0.5, 0.3)]),
    # the same with a bright band of no opacity: colour without opacity must add nothing
    "gap": plateau_map([(0.9, 0.1, 0.1, 0.04), (0.1, 0.8, 0.2, 0.12), (1.0, 1.0, 0.95, 0.0),
                        (0.9, 0.8, 0.1, 0.4), (0.5, 0.5, 0.5, 0.3)]),
}
TRANSPARENCIES = (0.25, 0.85)


def level_tables(boxes, color_map, transparency, ref_dist, scalar_range=(0.0, 1.0),
                 bounds=SAMPLING_BOUNDS):
    """Per box the colour table of its level as float64 [256, 4], from the product's own host
    functions (pinned by test_host_parity.py): input data of the march, not a result of it.
    Opaque entries are out of the colour brackets' scope: every opacity <= 0.6 here."""
    params = make_params(8, 8, scalar_range, transparency, ref_dist, bounds, color_map)
    tables = []
    for box in boxes:
        _, factor, alpha_scale = runtime.box_sampling(meta(box), params)
        table = runtime.build_color_table(alpha_scale, factor, scalar_range,
                                          color_map).astype(np.float64)
        assert table.shape == (256, 4)
        assert (table[:, :3] >= 0.0).all() and (table[:, :3] <= 1.0).all()
        assert (table[:, 3] >= 0.0).all() and (table[:, 3] <= 0.6).all()
        tables.append(table)
    return tables


def index_cells(box):
    """What is uploaded for a box with .index: the entry is unambiguous under (0, 1) scaling."""
    return np.ascontiguousarray((box.index + 0.5) / 255.0)


def oracle_colour_layers(O, boxes, cam, W, H, color_map, transparency, ref_dist):
    ocam, otr = oracle_camera(O, cam), oracle_transform(O, NORM)
    op = oracle_params(O, W, H, (0.0, 1.0), transparency, ref_dist, SAMPLING_BOUNDS, color_map)
    return [O.paint_box(O.make_box(index_cells(box), box.min_corner, box.max_corner), otr, op, ocam,
                        threads=16)[0] for box in boxes]


def oracle_colour_frame(O, boxes, cam, W, H, color_map, transparency, ref_dist):
    """[H, W, 5]: the boxes' layers through the oracle's layered compose of one rank, which takes
    them in the order of their depth hints."""
    layers = oracle_colour_layers(O, boxes, cam, W, H, color_map, transparency, ref_dist)
    ocam = oracle_camera(O, cam)
    hints = [O.box_depth_hint(O.make_box(index_cells(b), b.min_corner, b.max_corner), ocam)
             for b in boxes]
    frame, _, _ = O.compose_layered(layers, hints, [0] * len(boxes), list(range(len(boxes))), 1)
    return frame.reshape(H, W, 5)


def check_colour(name, e, rgba):
    """rgba [H, W, >= 4] (premultiplied colour, alpha) inside the colour and alpha brackets on
    every pixel not excluded.  Returns the largest error / margin of (colour, alpha)."""
    ok = ~e.excluded
    assert e.excluded_share() <= MAX_EXCLUDED
    assert e.hit.sum() > 200
    rgba = np.asarray(rgba, np.float64)
    worst = []
    for what, got in (("colour", rgba[..., :3]), ("alpha", rgba[..., 3])):
        exact, under, over = (getattr(e, what + k) for k in ("", "_under", "_over"))
        err = got - exact
        used = np.where(err > 0, err / np.maximum(over, 1e-300), -err / np.maximum(under, 1e-300))
        width = (under + over)[e.hit].mean(axis=0) / exact[e.hit].mean(axis=0)
        worst.append(float(used[ok].max()))
        report(name, f"{what}: largest error / margin", f"{worst[-1]:.3f}; mean bracket width / "
               f"mean value {np.array2string(np.atleast_1d(width), precision=3)}")
        bad = ok & e.outside(what, got)
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3])
    assert not rgba[~e.hit & ok][:, :4].any()
    return tuple(worst)


# ---- single boxes --------------------------------------------------------------------------------

DEFAULT = scenes.default_camera()
SINGLE = {
    # name: (lo, hi, shape [nz, ny, nx], ghost, camera, W, H)
    "power_of_two": ((0, 0, 0), (1, 1, 1), (32, 32, 32), 0, DEFAULT, 96, 64),
    "reciprocal_noncubic_cells": ((0.1, 0.2, -0.3), (0.8, 0.65, 0.8), (36, 20, 24), 0, DEFAULT, 64, 80),
    "general_division": ((0.05, 0.1, 0.15), (0.42, 0.47, 0.52), (20, 20, 20), 0,
                         CameraParameters((1.4, 0.9, 1.7), (0.23, 0.28, 0.33), (0, 1, 0), 35.0), 72, 56),
    "ghost_cells_view": ((0, 0, 0), (1, 1, 1), (16, 24, 20), 2, DEFAULT, 80, 64),
    # (the eye off the cell lattice: on a cell corner every ray would start near an edge)
    "eye_inside": ((0, 0, 0), (1, 1, 1), (24, 24, 24), 0,
                   CameraParameters((0.52, 0.47, 0.51), (0.9, 0.6, 0.1), (0, 1, 0), 60.0), 72, 56),
    "partly_off_screen": ((0, 0, 0), (1, 1, 1), (24, 24, 24), 0,
                          CameraParameters((1.6, 0.5, 2.0), (0.9, 0.5, 0.5), (0, 1, 0), 40.0), 72, 56),
    "rolled_up": ((0, 0, 0), (1, 1, 1), (24, 24, 24), 0,
                  CameraParameters((2.2, 1.6, 2.9), (0.5, 0.5, 0.5), (0.5, 1.0, 0.3), 45.0), 56, 72),
}


def single_box(name):
    lo, hi, shape, ghost, cam, W, H = SINGLE[name]
    box = box_of(ramp, lo, hi, shape, ghost)
    box.index = mip_index(box.cells)
    return box, cam, W, H


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_single_box(O, avr_lib, name):
    box, cam, W, H = single_box(name)
    e = K.expected(cam, W, H, [box])
    length, column = oracle_length_column(O, [box], cam, W, H, integer=True)
    check_length_column(name, e, length, column)
    check_mip(name, e, oracle_mip(O, [box], cam, W, H))
    # depth of the volume layer
    d = K.rays(cam, W, H).reshape(-1, 3)
    bt = K.box_terms(cam, d, box)
    ob = O.make_box(np.ascontiguousarray(box.cells / 15.0), box.min_corner, box.max_corner)
    img = O.paint_box(ob, oracle_transform(O, NORM), oracle_params(O, W, H, (0.0, 1.0), 0.0, 0.0,
                      SAMPLING_BOUNDS, HOMOGENEOUS_MAP), oracle_camera(O, cam), threads=16)[0]
    depth = img[..., 4].reshape(-1)[bt.ch.rays].astype(np.float64)
    seen = (img[..., 3].reshape(-1)[bt.ch.rays] > 0) & ~e.excluded.reshape(-1)[bt.ch.rays]
    assert seen.sum() > 200
    assert (np.abs(depth - bt.depth)[seen] <= bt.depth_margin[seen]).all()
    missed = np.ones(W * H, bool)
    missed[bt.ch.rays] = False
    assert np.isinf(img[..., 4].reshape(-1)[missed & ~e.excluded.reshape(-1)]).all()


def test_single_box_smooth_cells_and_special_values(O, avr_lib):
    lo, hi, shape, _, cam, W, H = SINGLE["power_of_two"]
    box = box_of(lambda x, y, z: np.round(smooth(x, y, z) * 4.0) / 4.0 + 1.0 / 3.0, lo, hi,
                 (16, 16, 16))
    flat = box.cells.reshape(-1)
    flat[np.random.default_rng(3).choice(flat.size, 200, replace=False)] = np.nan
    e = K.expected(cam, W, H, [box])
    length, column = oracle_length_column(O, [box], cam, W, H, integer=False)
    check_length_column("smooth_with_nan", e, length, column)


# ---- AMR scenes: boxes summed ---------------------------------------------------------------------

AMR = {"two_levels": (scenes.make_amr_scene(32, 2, 8), scenes.orbit_camera(3), 96, 64),
       "three_levels": (scenes.make_amr_scene(32, 3, 8), DEFAULT, 80, 64)}
TEETH = (scenes.make_amr_scene(64, 3, 16), DEFAULT, 90, 60)


@pytest.mark.parametrize("name", sorted(AMR))
def test_amr_scene(O, avr_lib, name):
    spec, cam, W, H = AMR[name]
    boxes = amr_boxes(spec, ramp)
    for b in boxes:
        b.index = mip_index(b.cells)
    transparency = 0.25
    ref_step = max(b.step for b in boxes)
    per_box, a_ref = homogeneous_tables(O, boxes, transparency, ref_step)
    e = K.expected(cam, W, H, boxes, sample_alpha=per_box)
    assert e.boxes_crossed.max() >= 2 * spec.levels
    length, column = oracle_length_column(O, boxes, cam, W, H, integer=True)
    check_length_column(name, e, length, column)
    check_mip(name, e, oracle_mip(O, boxes, cam, W, H))
    check_alpha(name, e, oracle_homogeneous_alpha(O, boxes, cam, W, H, transparency, ref_step),
                a_ref, ref_step)
    smooth_boxes = amr_boxes(spec, lambda x, y, z: np.round(smooth(x, y, z) * 3.0) / 3.0)
    es = K.expected(cam, W, H, smooth_boxes)
    check_length_column(name + "_smooth", es,
                        *oracle_length_column(O, smooth_boxes, cam, W, H, integer=False))


# ---- coloured frames ---------------------------------------------------------------------------------

_COLOUR_CASES = {}


def colour_case(name, map_name, transparency=0.0):
    """(boxes, camera, W, H, reference step, tables, expectation) of a SINGLE or AMR case under
    a colour map: built once per process and shared, read-only, with the GPU tests.  A single
    box is painted the way test_single_box paints it: no transparency, its own step the
    reference."""
    key = (name, map_name, transparency)
    if key not in _COLOUR_CASES:
        if name in SINGLE:
            box, cam, W, H = single_box(name)
            boxes, bounds, ref_step = [box], SAMPLING_BOUNDS, 0.0
        else:
            spec, cam, W, H = AMR[name]
            boxes, bounds = amr_boxes(spec, ramp), spec.bounds
            for b in boxes:
                b.index = mip_index(b.cells)
            ref_step = runtime.reference_sample_distance([meta(b) for b in boxes],
                                                         bounds.min_corner, bounds.max_corner)
        tables = level_tables(boxes, COLOUR_MAPS[map_name], transparency, ref_step, bounds=bounds)
        _COLOUR_CASES[key] = (boxes, cam, W, H, ref_step, tables,
                              K.expected(cam, W, H, boxes, tables=tables))
    return _COLOUR_CASES[key]


@pytest.mark.parametrize("map_name", sorted(COLOUR_MAPS))
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_single_box_colour(O, avr_lib, name, map_name):
    boxes, cam, W, H, ref_step, _, e = colour_case(name, map_name)
    img = oracle_colour_layers(O, boxes, cam, W, H, COLOUR_MAPS[map_name], 0.0, ref_step)[0]
    check_colour(f"{name}/{map_name}", e, img)


@pytest.mark.parametrize("transparency", TRANSPARENCIES)
@pytest.mark.parametrize("map_name", sorted(COLOUR_MAPS))
@pytest.mark.parametrize("name", sorted(AMR))
def test_amr_scene_colour(O, avr_lib, name, map_name, transparency):
    boxes, cam, W, H, ref_step, tables, e = colour_case(name, map_name, transparency)
    assert e.boxes_crossed.max() >= 2 * AMR[name][0].levels
    # the levels' tables differ (the finer, the less opaque per sample), the colours do not
    coarse, fine = tables[0], tables[-1]
    assert boxes[0].level == 0 and boxes[-1].level > 0
    assert (fine[list(MIP_LEVELS), 3] <= 0.75 * coarse[list(MIP_LEVELS), 3]).all()
    frame = oracle_colour_frame(O, boxes, cam, W, H, COLOUR_MAPS[map_name], transparency, ref_step)
    check_colour(f"{name}/{map_name}/{transparency}", e, frame)


# ---- a written plotfile: levels with overlap, physical extent ------------------------------------

PROB_LO, PROB_HI = (0.0, 0.0, 0.0), (3.0, 4.5, 2.4)


def plotfile_levels(value=lambda r: r + 1.0):
    """Three levels over a 12 x 12 x 12 base grid, ratio 2, each finer level over a part of the one
    below (two grids on level 1); cells = ramp at the cell centre in domain-normalised units."""
    def lev(n, boxes):
        data = []
        for lo, hi in boxes:
            c = [(np.arange(lo[a], hi[a] + 1) + 0.5) / n for a in range(3)]
            data.append(value(ramp(c[0][None, None, :], c[1][None, :, None], c[2][:, None, None]))
                        + np.zeros((hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)))
        return {"domain": ((0, 0, 0), (n - 1,) * 3), "boxes": boxes, "data": data}
    return [lev(12, [((0, 0, 0), (11, 11, 11))]),
            lev(24, [((4, 6, 2), (13, 17, 11)), ((14, 6, 2), (19, 13, 15))]),
            lev(48, [((12, 16, 8), (23, 31, 19))])]


def write_levels(path, value=lambda r: r + 1.0):
    """value(ramp) is what the cells hold: ramp + 1 by default."""
    levels = plotfile_levels(value)
    plotfile.write_plotfile(str(path), ["density"],
                            [{**l, "data": [d[None] for d in l["data"]]} for l in levels],
                            PROB_LO, PROB_HI, [2, 2])
    return levels


def world_boxes(pf, scale=1.0):
    """World-space continuum boxes of the convexified hierarchy of a PlotFileData, read on the
    host: prob_lo + index * cell size, times `scale`."""
    n_levels = pf.finest_level + 1
    convex = plotfile.convexify([pf.boxes(l) for l in range(n_levels)], pf.ref_ratio)
    out, index_boxes = [], []
    for level in range(n_levels):
        grids = pf.get(level, "density")
        dx = pf.cell_size[level]
        index_boxes.append([part for _, part in convex[level]])
        for parent, (lo, hi) in convex[level]:
            glo = pf.boxes(level)[parent][0]
            view = grids[parent][lo[2] - glo[2]:hi[2] - glo[2] + 1, lo[1] - glo[1]:hi[1] - glo[1] + 1,
                                 lo[0] - glo[0]:hi[0] - glo[0] + 1]
            out.append(K.Box(tuple(scale * (pf.prob_lo[a] + lo[a] * dx[a]) for a in range(3)),
                             tuple(scale * (pf.prob_lo[a] + (hi[a] + 1) * dx[a]) for a in range(3)),
                             view, level=level))
    return out, index_boxes


PLOTFILE_CAMERA = CameraParameters((6.5, 7.0, 6.0), (1.5, 2.25, 1.2), (0, 1, 0), 40.0)


def test_plotfile_convexify_against_the_finest_value(tmp_path):
    levels = write_levels(tmp_path / "pf")
    pf = plotfile.PlotFileData(str(tmp_path / "pf"))
    boxes, index_boxes = world_boxes(pf)
    count = K.coverage_count(index_boxes, pf.ref_ratio, (11, 11, 11))
    assert (count == 1).all()            # disjoint, and their union is the domain
    grid = K.finest_value_grid(levels, [2, 2])
    assert np.isfinite(grid).all()
    whole = K.Box(PROB_LO, PROB_HI, grid)
    W, H = 64, 48
    a = K.expected(PLOTFILE_CAMERA, W, H, boxes)
    b = K.expected(PLOTFILE_CAMERA, W, H, [whole])
    assert a.hit.sum() > 500 and np.array_equal(a.hit, b.hit)
    assert np.allclose(a.column, b.column, rtol=1e-12, atol=0.0)
    assert np.allclose(a.length, b.length, rtol=1e-12, atol=0.0)


# ---- teeth: a different reading must leave the brackets ------------------------------------------

def outside(e, length, column, mip=None):
    """Share of the hitting, not excluded pixels at which (length, column, mip) is outside e's
    brackets."""
    ok = e.hit & ~e.excluded
    bad = e.outside("length", length) | e.outside("column", column)
    if mip is not None:
        bad |= (mip[0] > e.mip_hi) | (mip[1] < e.mip_lo)
    return float((bad & ok).sum()) / max(int(ok.sum()), 1)


def test_mutants_of_the_reference_leave_its_brackets(tmp_path):
    spec, cam, W, H = TEETH
    boxes = amr_boxes(spec, ramp)
    for b in boxes:
        b.index = mip_index(b.cells)
    ref_step = max(b.step for b in boxes)
    a = HOMOGENEOUS_ALPHA
    per_box = [-np.expm1(b.step / ref_step * np.log1p(-a)) for b in boxes]
    e = K.expected(cam, W, H, boxes, sample_alpha=per_box)
    excluded = e.excluded_share()
    assert excluded <= MAX_EXCLUDED
    shares = {}

    def geometric(name, mutant):
        shares[name] = outside(e, mutant.length, mutant.column, (mutant.mip_lo, mutant.mip_hi))

    geometric("half_pixel_shift", K.expected(cam, W, H, boxes,
                                             conventions=K.Conventions(pixel_centre=0.0)))
    geometric("y_flipped", K.expected(cam, W, H, boxes,
                                      conventions=K.Conventions(row0_at_bottom=False)))
    geometric("fov_as_half_angle", K.expected(cam, W, H, boxes,
                                              conventions=K.Conventions(fov_is_full_angle=False)))
    geometric("aspect_on_y", K.expected(cam, W, H, boxes,
                                        conventions=K.Conventions(aspect_on_x=False)))
    # one covered coarse box kept: the first level-0 box under level 1
    h0 = 1.0 / spec.n0
    lo = tuple((spec.n0 // 4) * h0 for _ in range(3))
    kept = box_of(ramp, lo, tuple(v + spec.box_cells * h0 for v in lo), (spec.box_cells,) * 3)
    kept.index = mip_index(kept.cells)
    geometric("covered_coarse_box_kept", K.expected(cam, W, H, boxes + [kept]))
    # x and z transposed: every box reads the field with its axes swapped
    swapped = amr_boxes(spec, lambda x, y, z: ramp(z, y, x))
    for b in swapped:
        b.index = mip_index(b.cells)
    geometric("x_and_z_transposed", K.expected(cam, W, H, swapped))
    # the step doubled on one level, the table's opacity kept: the alpha brackets must part
    steps = [b.step * (2.0 if b.level == 1 else 1.0) for b in boxes]
    m = K.expected(cam, W, H, boxes, steps=steps, sample_alpha=per_box)
    widen = e.samples_hi * 2.0 ** -23 + 2.0 ** -23
    apart = (m.alpha_hi < e.alpha_lo - widen) | (m.alpha_lo > e.alpha_hi + widen)
    ok = e.hit & ~e.excluded
    shares["step_doubled_on_level_1"] = float((apart & ok).sum()) / int(ok.sum())

    # world scale dropped: the plotfile's boxes in scene units (shortest edge 1) against physical
    write_levels(tmp_path / "pf")
    pf = plotfile.PlotFileData(str(tmp_path / "pf"))
    scale = 1.0 / min(PROB_HI)
    physical, _ = world_boxes(pf)
    scene, _ = world_boxes(pf, scale)
    cam_scene = CameraParameters(tuple(scale * v for v in PLOTFILE_CAMERA.eye),
                                 tuple(scale * v for v in PLOTFILE_CAMERA.look_at), (0, 1, 0), 40.0)
    ep = K.expected(PLOTFILE_CAMERA, W, H, physical)
    es = K.expected(cam_scene, W, H, scene)
    # (the same rays: the rescaled picture's lengths are the physical ones times the scale)
    assert np.allclose(es.length / scale, ep.length, rtol=1e-9, atol=1e-12)
    assert ep.excluded_share() <= MAX_EXCLUDED
    shares["world_scale_dropped"] = outside(ep, es.length, es.column)

    for name, share in shares.items():
        report("mutant " + name, "share of pixels outside the brackets", f"{share:.4f}")
    report("mutants", "excluded share", f"{excluded:.4f}")
    assert len(shares) == 8
    for name, share in shares.items():
        assert share > max(excluded, ep.excluded_share()), name


def test_mutants_of_the_coloured_reference_leave_its_brackets(avr_lib):
    """Another reading of the coloured picture (K.Reading, or other tables), evaluated exactly in
    float64, must leave the colour brackets of the stated one on more pixels than are excluded."""
    spec, cam, W, H = TEETH
    boxes = amr_boxes(spec, ramp)
    for b in boxes:
        b.index = mip_index(b.cells)
    ref_step = runtime.reference_sample_distance([meta(b) for b in boxes], spec.bounds.min_corner,
                                                 spec.bounds.max_corner)
    # (at transparency 0.25 the coarse boxes in front are all but opaque and the finer levels
    # behind them hardly show: their tables would not matter)
    tables = {m: level_tables(boxes, COLOUR_MAPS[m], 0.85, ref_step, bounds=spec.bounds)
              for m in COLOUR_MAPS}
    e = {m: K.expected(cam, W, H, boxes, tables=tables[m]) for m in COLOUR_MAPS}
    excluded = e["contrast"].excluded_share()
    assert excluded <= MAX_EXCLUDED
    assert boxes[0].level == 0
    mutants = {
        "boxes_back_to_front": ("contrast", {"reading": K.Reading(boxes_front_to_back=False)}),
        "segments_back_to_front": ("contrast", {"reading": K.Reading(segments_front_to_back=False)}),
        "colour_taken_as_premultiplied": ("contrast", {"reading": K.Reading(colour_times_opacity=False)}),
        "coarsest_table_on_every_level": ("contrast", {"tables": [tables["contrast"][0]] * len(boxes)}),
        "entry_k_plus_1": ("contrast", {"reading": K.Reading(entry_offset=1)}),
        "red_and_blue_exchanged": ("contrast", {"reading": K.Reading(swap_red_blue=True)}),
        "layers_summed_without_shadow": ("contrast", {"reading": K.Reading(boxes_shadow=False)}),
        # colour without opacity must add nothing: the gap map's bright band shows if it does
        "gap_colour_taken_as_premultiplied": ("gap", {"reading": K.Reading(colour_times_opacity=False)}),
    }
    shares = {}
    for name, (m, change) in mutants.items():
        mutant = K.expected(cam, W, H, boxes, **{"tables": tables[m], **change})
        ok = e[m].hit & ~e[m].excluded
        bad = e[m].outside("colour", mutant.colour) | e[m].outside("alpha", mutant.alpha)
        shares[name] = float((bad & ok).sum()) / int(ok.sum())
        report("mutant " + name, "share of pixels outside the colour brackets", f"{shares[name]:.4f}")
    report("coloured mutants", "excluded share", f"{excluded:.4f}")
    for m in COLOUR_MAPS:
        width = (e[m].colour_under + e[m].colour_over)[e[m].hit].mean(axis=0) / \
            e[m].colour[e[m].hit].mean(axis=0)
        report("coloured mutants", f"{m}: mean bracket width / mean value per channel",
               np.array2string(width, precision=3))
    assert len(shares) == 8
    for name, share in shares.items():
        assert share > excluded, name
