"""Holds tests/wide_view_cases.py to its claims, in plain Python integers and numpy: the spans and
parities of the wide views, that no two cells share an element, the poison around every view, the
byte offsets reached, and the ends and nesting of the translated hierarchies.  For the inputs of
the newer products the numpy references say, without a GPU, that they reach what the GPU tests are
about: the cells the fixed particles land in, the leaf counts per level, the cloud corners on the
index limits, the fill and partial cells of the partial grid, the clump threshold."""
import numpy as np
import pytest

import clump_reference
import grid_field_reference as gf
import particle_reference as pr
import wide_view_cases as cases
from gradient_reference import same_bits

CASES = cases.wide_cases()
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]


def test_the_seven_cases_are_the_ones_the_kernels_need():
    assert IDS == ["end_pair", "odd_row_end", "row_stride_at_cap", "row_stride_below_cap",
                   "unpaired_at_limit", "chunk_crossing_paired", "chunk_crossing_unpaired"]
    assert cases.STORAGE == 2 ** 28 + 2 ** 20 and cases.BASE == 2 ** 19
    assert cases.SPAN_LIMIT == 2 ** 28 - 1


def test_spans_strides_and_parities_are_as_stated():
    want = {   # name: (offset, dims, jstride, kstride, span)
        "end_pair": (2 ** 19, (6, 2, 2), 2 ** 26, 2 ** 28 - 2 ** 26 - 6, 2 ** 28 - 1),
        "odd_row_end": (2 ** 19, (5, 2, 2), 2 ** 26, 2 ** 28 - 2 ** 26 - 6, 2 ** 28 - 2),
        "row_stride_at_cap": (2 ** 19, (7, 2, 2), 2 ** 27, 2 ** 27 - 8, 2 ** 28 - 2),
        "row_stride_below_cap": (2 ** 19, (2, 2, 2), 2 ** 27 - 2, 2 ** 27, 2 ** 28 - 1),
    }
    for name, (offset, dims, js, ks, s) in want.items():
        view = BY_NAME[name].view
        assert view == cases.View(offset, dims, js, ks), name
        assert cases.span(view) == s, name
    # 1, 2, the twin of 3 and the paired 5: the pair path of every kernel
    for name in ("end_pair", "odd_row_end", "row_stride_below_cap", "chunk_crossing_paired"):
        c = BY_NAME[name]
        assert c.view.offset % 2 == 0 and c.view.jstride % 2 == 0 and c.view.kstride % 2 == 0
        assert c.classify_pairs and c.others_pair
    assert BY_NAME["end_pair"].view.dims[0] % 2 == 0        # whole pairs only
    assert BY_NAME["odd_row_end"].view.dims[0] % 2 == 1     # a single-cell tail in every row
    # 3: at the cap only classify_tile leaves the pair path
    cap = BY_NAME["row_stride_at_cap"]
    assert cap.view.jstride == 2 ** 27 and cap.view.kstride < cap.view.jstride
    assert not cap.classify_pairs and cap.others_pair
    assert BY_NAME["row_stride_below_cap"].view.jstride + 2 == 2 ** 27
    # 4: nothing pairs; kstride is the largest odd one the span rule admits
    odd = BY_NAME["unpaired_at_limit"]
    assert odd.view.offset % 2 == 1 and odd.view.jstride % 2 == 1 and odd.view.kstride % 2 == 1
    assert not odd.classify_pairs and not odd.others_pair
    assert cases.span(odd.view) == cases.SPAN_LIMIT
    assert cases.span(odd.view._replace(kstride=odd.view.kstride + 2)) > cases.SPAN_LIMIT
    # 5: a row crosses the chunk, the second brick of rows holds one row, one plane of two
    for name, paired in (("chunk_crossing_paired", True), ("chunk_crossing_unpaired", False)):
        c = BY_NAME[name]
        nx, ny, nz = c.view.dims
        assert (nx, ny, nz) == (130, 5, 2) and c.view.jstride == 132
        assert cases.CHUNK < nx < 2 * cases.CHUNK and ny % cases.BRICK == 1 and nz < cases.BRICK
        assert c.classify_pairs == c.others_pair == paired
        assert c.view.kstride * (nz - 1) > cases.span(c.view) - 1024     # nearly all of the span
        assert cases.SPAN_LIMIT - 1 <= cases.span(c.view) <= cases.SPAN_LIMIT


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_span_rule_accepts_every_field_and_the_limit_cases_sit_on_it(case):
    for f in range(cases.MAX_FIELDS):
        view = cases.field_view(case, f)
        assert view.jstride >= 0 and view.kstride >= 0 and cases.span(view) <= cases.SPAN_LIMIT
        assert cases.is_paired(view) == case.others_pair     # the shifts keep the parity
        assert cases.classify_is_paired(view) == case.classify_pairs
    largest_byte_offset = 8 * cases.span(case.view)
    assert largest_byte_offset >= 2 ** 30                    # bit 30 of the offset is in use
    assert case.at_limit == (largest_byte_offset == 2 ** 31 - 8)
    assert case.at_limit == (case.name in ("end_pair", "row_stride_below_cap", "unpaired_at_limit",
                                           "chunk_crossing_paired"))
    if case.name == "end_pair":     # the last 16-byte pair ends at byte 2^31 exactly
        assert largest_byte_offset - 8 + 16 == 2 ** 31


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_two_cells_share_an_element_and_poison_surrounds_every_view(case):
    nx, ny, nz = case.view.dims
    seen = set()
    for f in range(cases.MAX_FIELDS):
        view = cases.field_view(case, f)
        cells = cases.elements(view)
        assert len(cells) == nx * ny * nz                    # no two cells of a view coincide
        assert not (cells & seen)                            # nor of two views in one storage
        seen |= cells
        before = min(cells)
        after = cases.STORAGE - 1 - max(cells)
        # the first field keeps 2^19 - 1 elements of poison on each side, the shifted ones all
        # but their shift of it
        slack = f * case.field_shift
        assert before >= 2 ** 19 - 1 and after >= 2 ** 19 - 1 - slack >= 2 ** 18, (f, before, after)
        assert max(cells) == view.offset + cases.span(view)


def test_the_brick_row_past_ny_of_case_3_does_not_fit_32_bits_of_bytes():
    """A tile is a brick of four rows, and these boxes have two: rows 2 and 3 are masked.  For row 3
    of case 3 the byte offset jstride * 3 * 8 alone is 2^31 or more, past num_records of
    classify_tile's buffer resource and, one doubling on, past 32 bits, so a kernel must not form
    an address from it.  That relies on the masks of classify_tile (`valid` before lane_cell, and
    the j < ny test of its unpaired path), for_each_cell in avr_scene_stats.hip, derive_tile's
    valid##p, for_each_cell of avr_cell_tiles.h (clumps, joint histogram, gradient), and the
    per-cell lookups of the other products, which only address cells they have located."""
    for name in ("row_stride_at_cap", "row_stride_below_cap"):
        view = BY_NAME[name].view
        assert view.dims[1] == 2 < cases.BRICK
    assert BY_NAME["row_stride_at_cap"].view.jstride * 3 * 8 >= 2 ** 31
    assert BY_NAME["row_stride_at_cap"].view.jstride * 3 * 8 < 2 ** 32
    assert BY_NAME["row_stride_below_cap"].view.jstride * 3 * 8 >= 2 ** 31


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cells_are_distinct_finite_and_no_poison(case):
    every = np.concatenate([cases.field_cells(case, f).reshape(-1)
                            for f in range(cases.MAX_FIELDS)] +
                           [cases.small_cells((cases.PLAIN_NX,) + case.view.dims[1:], f).reshape(-1)
                            for f in range(cases.MAX_FIELDS)] +
                           [cases.small_cells(cases.FINE_DIMS, 10 + f).reshape(-1)
                            for f in range(cases.MAX_FIELDS)])
    assert np.isfinite(every).all() and np.unique(every).size == every.size
    assert cases.POISON < 0 and np.isfinite(cases.POISON) and (every > 1.0).all()
    assert np.array([cases.POISON]).view(np.int64)[0] == cases.POISON_BITS
    first = cases.field_cells(case, 0)
    assert first[-1, -1, -1] == first.max()
    assert first[-1, -1, -2] == np.sort(first.reshape(-1))[-2]
    odd = cases.field_cells(case, 0, odd=True)
    assert np.isnan(odd.flat[1]) and odd.flat[2] == np.inf and odd.flat[3] == -np.inf
    assert (~np.isfinite(odd)).sum() == 3 and np.isfinite(odd[-1, -1, -2:]).all()
    keep = np.isfinite(odd)
    assert np.array_equal(odd[keep], first[keep])
    for whole in (cases.field_cells(case, cases.WHOLE),
                  cases.small_cells(cases.FINE_DIMS, 10 + cases.WHOLE)):
        assert np.array_equal(whole, np.rint(whole)) and whole.sum() < 2.0 ** 53


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("wide_first", [True, False])
def test_the_scene_around_a_wide_box_nests_and_keeps_its_last_cell_a_leaf(case, wide_first):
    boxes = cases.hierarchy(case, wide_first)
    assert [b.kind for b in boxes] == (["wide", "plain", "fine"] if wide_first
                                       else ["plain", "wide", "fine"])
    by_kind = {b.kind: b for b in boxes}
    wide, plain, fine = by_kind["wide"], by_kind["plain"], by_kind["fine"]
    assert wide.dims == case.view.dims and wide.index_lo == (0, 0, 0)
    nx, ny, nz = wide.dims
    assert plain.index_lo == (nx, 0, 0) and plain.dims == (cases.PLAIN_NX, ny, nz)
    # the fine box, coarsened, covers one cell of each coarse box and lies inside their union
    lo = tuple(v // cases.RATIO[0] for v in fine.index_lo)
    hi = tuple((v + n - 1) // cases.RATIO[0] for v, n in zip(fine.index_lo, fine.dims))
    assert lo == (nx - 1, 0, 0) and hi == (nx, 0, 0)
    assert (nx - 1, ny - 1, nz - 1) != hi and ny > 1
    assert cases.corners(wide)[1][0] == cases.corners(plain)[0][0]
    assert cases.corners(plain)[1] == cases.extent(case)
    assert cases.corners(fine)[0][0] == (nx - 1) * cases.CELL


# ---- part A: the inputs of the newer products --------------------------------------------------

def wide_hierarchy(case):
    """particle_reference's hierarchy of a case's scene as the runtime sees it.  The scene is made
    of boxes, not of a plotfile's leaves: the two level-0 cells under the fine box are cells of
    their boxes like any other, so a level-0 cloud corner finds them present and a share lands in
    them, while a point inside the fine box is still located there, finest level first."""
    h = pr.hierarchy(cases.scene_levels(case), cases.RATIO, cases.level_sizes(), (0.0, 0.0, 0.0))
    assert (~h.mask[0]).sum() == 2 and h.mask[1].sum() == 16
    h.mask[0][...] = True
    return h


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_channel_edges_put_wide_cells_under_inside_and_over(case):
    nx, ny, nz = case.view.dims
    velocity = cases.field_cells(case, 1)
    edges = cases.CUBE_EDGES
    assert edges.size == 6 and (np.diff(edges) > 0.0).all()
    assert (velocity < edges[0]).any() and (velocity > edges[-1]).sum() == 0
    assert edges[-2] <= velocity[-1, -1, -1] < edges[-1]            # the last cell: the last channel
    assert all(cases.small_cells(dims, tag + 1).min() > edges[-1]
               for dims, tag in (((cases.PLAIN_NX, ny, nz), 0), (cases.FINE_DIMS, 10)))
    binned = cases.field_cells(case, 3)
    edges = cases.TRANSFER_EDGES
    assert edges.size == 4 and (np.diff(edges) > 0.0).all()
    assert (binned < edges[0]).any() and edges[-2] <= binned[-1, -1, -1] < edges[-1]
    # the opacity's scale is a power of two, and the longest row has an optical depth of order 1
    assert np.frexp(cases.OPACITY_SCALE)[0] == 0.5
    row = cases.field_cells(case, 2)[-1, -1, :] * cases.OPACITY_SCALE * cases.CELL
    assert 0.04 < row.sum() < 8.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_fixed_particles_land_in_the_cells_claimed(case):
    nx, ny, nz = case.view.dims
    points, values = cases.wide_particles(case)
    assert 256 < len(points) <= 365 and values.shape == (len(points),)
    assert np.isfinite(points).all() and np.isfinite(values).all() and (values[:5] != 0.0).all()
    h = wide_hierarchy(case)
    level, q, index = h.locate(points)
    assert level[:5].tolist() == [0, 0, 0, 1, 1]
    assert index[0].tolist() == [0, 0, 0]
    assert index[1].tolist() == [nx - 1, ny - 1, nz - 1]            # the wide box's last cell
    assert (q[1] - index[1]).tolist() == [0.75] * 3
    assert index[2].tolist() == [nx, ny - 1, nz - 1] and q[2][0] == nx      # on the face: plain
    fine = cases.hierarchy(case)[2]
    for row in (3, 4):
        assert all(fine.index_lo[a] <= index[row][a] < fine.index_lo[a] + fine.dims[a]
                   for a in range(3))
    assert (level == -1).sum() > 50 and (level == 0).sum() > 100
    for method in (0, 1):
        found = pr.contributions(h, points, values, method)
        assert found["outside"] == (level == -1).sum()
        assert (found["rerouted"] > 0) == (method == 1)
        named = {(int(l), tuple(int(v) for v in i))
                 for l, i in zip(found["level"].reshape(-1), found["index"].reshape(-1, 3)) if l >= 0}
        assert (0, cases.empty_cell(case)) not in named             # the clear pass alone writes it
        assert (0, (nx - 1, ny - 1, nz - 1)) in named
        dense = pr.deposit(h, found, 0)[0]
        assert dense[nz - 1, ny - 1, nx - 1] != 0.0
        e = cases.empty_cell(case)
        assert dense[e[2], e[1], e[0]] == 0.0 and not np.signbit(dense[e[2], e[1], e[0]])
    # cloud in cell: the last-cell particle's corners past the domain in y and z come back to it,
    # the one in +x alone lands in the plain box
    found = pr.contributions(h, points, values, 1)
    corners = [(int(l), tuple(int(v) for v in i)) for l, i in zip(found["level"][1], found["index"][1])]
    assert corners.count((0, (nx - 1, ny - 1, nz - 1))) == 7 and corners[1] == (0, (nx, ny - 1, nz - 1))
    assert (0, (nx - 1, ny - 1, nz - 1)) in [
        (int(l), tuple(int(v) for v in i)) for l, i in zip(found["level"][2], found["index"][2])]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_partial_grid_leaves_fill_and_partial_cells_in_the_wide_box(case):
    nx, ny, nz = case.view.dims
    grids = {g.name: g for g in cases.wide_grids(case)}
    assert sorted(grids) == ["margin", "partial", "refined"]
    for g in grids.values():
        finite = g.grid[np.isfinite(g.grid)]
        assert np.isnan(g.grid).sum() == 1 and np.unique(finite).size == finite.size == g.grid.size - 1
    assert grids["margin"].level == 0 and grids["margin"].lo == (-1, 0, 0)
    assert grids["margin"].grid.shape == (nz, ny, nx + cases.PLAIN_NX + 1)
    assert grids["margin"].modes == [(0, False), (1, False), (1, True)]
    assert grids["refined"].grid.shape == (2 * nz, 2 * ny, 2 * (nx + cases.PLAIN_NX))
    k, j, i = np.indices((nz, ny, nx))
    index = np.stack([i.reshape(-1), j.reshape(-1), k.reshape(-1)])
    g = grids["partial"]
    values, filled, partial = gf.grid_cells(g.grid, g.level, g.lo, 0, index, cases.RATIO)
    filled, partial = filled.reshape(nz, ny, nx), partial.reshape(nz, ny, nx)
    assert filled[:, :, 0].all() and not filled[:, :, 1:].any() and partial[:, :, 1:].all()
    assert partial[-1, -1, -1] and np.isnan(values.reshape(nz, ny, nx)[filled]).all()
    # the whole grids leave nothing out, and the fine box is finer than the margin grid
    for name in ("margin", "refined"):
        g = grids[name]
        _, filled, partial = gf.grid_cells(g.grid, g.level, g.lo, 0, index, cases.RATIO)
        assert not filled.any() and not partial.any()
    assert cases.hierarchy(case)[2].level > grids["margin"].level


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_clump_threshold_makes_the_wide_boxs_last_cell_a_member(case):
    first = cases.field_cells(case, 0, odd=True)
    assert cases.CLUMP_LOWER <= first[-1, -1, -1] <= cases.CLUMP_UPPER
    assert (first < cases.CLUMP_LOWER).any()                        # and not every cell is one
    levels = cases.scene_levels(case)
    assert same_bits(levels[0]["data"][0][0], first)
    boxes = [(b.level, b.index_lo, tuple(lo + n - 1 for lo, n in zip(b.index_lo, b.dims)))
             for b in cases.hierarchy(case)]
    labels, n = clump_reference.clump_levels(levels, cases.RATIO, 0, cases.CLUMP_LOWER,
                                             cases.CLUMP_UPPER, boxes)
    nx, ny, nz = case.view.dims
    assert n >= 1 and labels[0][nz - 1, ny - 1, nx - 1] >= 1.0


# ---- part B ---------------------------------------------------------------------------------------

HIERARCHIES = cases.far_hierarchies()


@pytest.mark.parametrize("h", HIERARCHIES, ids=[h.name for h in HIERARCHIES])
def test_translated_hierarchies_end_on_the_index_limits_and_keep_their_nesting(h):
    assert [h.name for h in HIERARCHIES] == ["ratios_2_2", "ratios_4_2"]
    assert h.ratio == ([2, 2] if h.name == "ratios_2_2" else [4, 2]) and len(h.domains) == 3
    refine = h.ratio[0] * h.ratio[1]
    plain = cases.far_levels(h)
    moved = cases.translations(h)
    assert sorted(moved) == ["bottom", "top"]
    for name, t in moved.items():
        for l in range(2):
            assert t[l + 1] == tuple(v * h.ratio[l] for v in t[l])
        levels = cases.far_levels(h, t)
        lo, hi = levels[0]["domain"]
        if name == "top":
            assert all((hi[a] + 1) * refine - 1 == 2 ** 30 - 1 for a in range(3))
        else:
            assert all(lo[a] * refine == -2 ** 30 for a in range(3))
        for l, lev in enumerate(levels):
            to_finest = refine if l == 0 else (h.ratio[1] if l == 1 else 1)
            for (blo, bhi), data, was in zip(lev["boxes"], lev["data"], plain[l]["data"]):
                assert data is not was and np.array_equal(data, was, equal_nan=True)
                for a in range(3):      # the index rule, in the box's level and refined
                    assert -2 ** 30 <= blo[a] * to_finest and (bhi[a] + 1) * to_finest <= 2 ** 30
                    assert lev["domain"][0][a] <= blo[a] <= bhi[a] <= lev["domain"][1][a]
                if l == 0:
                    continue
                # floor division through the ratio maps the box into one box of the level below,
                # the same one as before the translation
                r = h.ratio[l - 1]
                # whole coarse cells: a coarse cell under the box is covered by it entirely
                assert all(blo[a] % r == 0 and (bhi[a] + 1) % r == 0 for a in range(3))
                parents = [p for p, (plo, phi) in enumerate(levels[l - 1]["boxes"])
                           if all(plo[a] <= blo[a] // r and bhi[a] // r <= phi[a] for a in range(3))]
                b = lev["boxes"].index((blo, bhi))
                olo, ohi = plain[l]["boxes"][b]
                before = [p for p, (plo, phi) in enumerate(plain[l - 1]["boxes"])
                          if all(plo[a] <= olo[a] // r and ohi[a] // r <= phi[a] for a in range(3))]
                assert parents == before and len(parents) == 1


PLACES = [(h, where) for h in HIERARCHIES for where in (None, "top", "bottom")]


def far_conditions(h, where, hier, found, points):
    """What the far particles must reach, from the reference's own output: shared with the GPU
    test, which asserts it again on the run it compares with."""
    leaves = np.bincount(found["leaf_level"][found["leaf_level"] >= 0], minlength=3)
    assert (leaves >= 32).all(), leaves
    assert found["outside"] > 0 and found["rerouted"] > 0
    corners = cases.rerouted_corners(hier, points)
    assert len(corners) == found["rerouted"]
    if where == "top":      # a corner cell whose first finest-level index is 2^30
        assert any(cases.finest_range(h, level, index[a])[0] == 2 ** 30
                   for level, index in corners for a in range(3))
    if where == "bottom":   # a corner cell whose last finest-level index is -2^30 - 1
        assert any(cases.finest_range(h, level, index[a])[1] == -2 ** 30 - 1
                   for level, index in corners for a in range(3))
    return leaves


@pytest.mark.parametrize("h,where", PLACES, ids=[f"{h.name}-{w}" for h, w in PLACES])
def test_the_far_particles_reach_every_level_and_the_corners_on_the_index_limits(h, where):
    translation = cases.translations(h)[where] if where else None
    sizes, prob_lo = cases.far_geometry(h, translation)
    hier = pr.hierarchy(cases.far_levels(h, translation), h.ratio, sizes, prob_lo)
    p = cases.far_particles(h)
    assert 256 < len(p.points) < 600 and p.values.shape == (len(p.points),)
    found = pr.contributions(hier, p.points, p.values, 1)
    far_conditions(h, where, hier, found, p.points)
    # the lattice batch: q is exact, so it is the untranslated q moved by the translation
    at = (p.points[p.lattice] - np.array(prob_lo)) / sizes[2][0]
    near = (p.points[p.lattice] - np.array(cases.FAR_PROB_LO)) / sizes[2][0]
    shift = np.array(translation[2] if where else (0, 0, 0), dtype=np.float64)
    assert np.array_equal(at, near + shift) and np.array_equal(at * 16.0, np.rint(at * 16.0))
    # the corners themselves: prob_lo is inside (cell 0 of level 0), prob_hi is not
    corner = len(p.points) - 12
    assert found["leaf_level"][corner] == 0 and found["leaf_level"][corner + 1] == -1
    base = pr.contributions(pr.hierarchy(cases.far_levels(h), h.ratio, *cases.far_geometry(h)),
                            p.points, p.values, 1)
    assert (found["outside"], found["rerouted"]) == (base["outside"], base["rerouted"])
    assert same_bits(found["shares"][p.lattice], base["shares"][p.lattice])


@pytest.mark.parametrize("h", HIERARCHIES, ids=[h.name for h in HIERARCHIES])
def test_the_far_transfer_fields_and_edges(h):
    levels = cases.far_levels(h)
    assert sorted(cases.FAR_FIELDS) == ["bin", "opacity", "source", "width"]
    for name in cases.FAR_FIELDS:
        mapped = cases.far_field_levels(levels, name)
        for lev, was in zip(mapped, levels):
            assert lev["boxes"] == was["boxes"] and lev["domain"] == was["domain"]
            for data, stored in zip(lev["data"], was["data"]):
                assert data.shape == (1,) + stored.shape[1:] and data.dtype == np.float64
                if name == "source":
                    assert same_bits(data[0], stored[0])
                if name == "opacity":
                    assert same_bits(data[0], np.abs(stored[2]) / 1024.0) and (data >= 0.0).all()
                if name == "bin":
                    assert same_bits(data[0], stored[2] / 2.0)
                if name == "width":
                    assert (data > 0.0).all() and (data <= 30.0 * 31.25).all()
    for edges in (cases.FAR_SHARP_EDGES, cases.FAR_BROAD_EDGES):
        assert edges.size == 4 and (np.diff(edges) > 0.0).all()
    binned = np.concatenate([d[0].reshape(-1) for lev in cases.far_field_levels(levels, "bin")
                             for d in lev["data"]])
    binned = binned[np.abs(binned) < 1e20]                  # without the cells under a finer grid
    assert (binned < cases.FAR_SHARP_EDGES[0]).any() and (binned > cases.FAR_SHARP_EDGES[-1]).any()
    assert np.all(np.diff(cases.FAR_BROAD_EDGES) == 31.25)
