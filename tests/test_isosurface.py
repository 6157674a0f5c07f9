"""Isosurfaces without a GPU: the numpy reference (isosurface_reference) against things that are
not its twin -- planes with closed-form areas, a closed sphere's topology, a brute-force
enumeration of the surface cubes -- and the host side of the API: surfaces.py, the declared ABI
entry, api.isosurface with the device work patched out."""
import math
import os
import types

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, plotfile, surfaces
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import gradient_reference as ref
import isosurface_reference as iso

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_level(shape, grids, sizes, prob_lo, field):
    """levels of one level over a domain of shape (nx, ny, nz): field(x, y, z) at the cell
    centres.  Returns (levels, scene boxes)."""
    nx, ny, nz = shape
    k, j, i = np.indices((nz, ny, nx)).astype(np.float64)
    x = prob_lo[0] + (i + 0.5) * sizes[0]
    y = prob_lo[1] + (j + 0.5) * sizes[1]
    z = prob_lo[2] + (k + 0.5) * sizes[2]
    dense = field(x, y, z)
    data = [dense[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1][None] for lo, hi in grids]
    levels = [{"domain": ((0, 0, 0), (nx - 1, ny - 1, nz - 1)), "boxes": list(grids),
               "data": data}]
    return levels, [(0, lo, hi) for lo, hi in grids], dense


def normals(vertices):
    return np.cross(vertices[:, 1] - vertices[:, 0], vertices[:, 2] - vertices[:, 0])


# ---- planes ----------------------------------------------------------------------------------------

SIZES = (0.5, 0.25, 1.0)
PROB_LO = (-1.0, 2.0, 0.5)
SHAPE = (8, 7, 6)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_an_axis_plane_has_its_vertices_on_the_plane_and_the_area_of_the_domains_section(axis, sign):
    grids = [((0, 0, 0), (3, 6, 5)), ((4, 0, 0), (7, 6, 5))]
    levels, boxes, _ = one_level(SHAPE, grids, SIZES, PROB_LO,
                                 lambda x, y, z: sign * (x, y, z)[axis])
    # 0.3 of the way through the cell-centre range, which no centre is at
    first = PROB_LO[axis] + 0.5 * SIZES[axis]
    at = first + 0.3 * (SHAPE[axis] - 1) * SIZES[axis]
    got = iso.isosurface(levels, [], 0, sign * at, boxes, [SIZES], PROB_LO)
    v = got["vertices"]
    n = v.shape[0]
    assert n > 0 and got["skipped"] == 0 and (got["level"] == 0).all()
    assert np.abs(v[:, :, axis] - at).max() <= 2.0 ** -51 * abs(at)
    u, w = (axis + 1) % 3, (axis + 2) % 3
    area = (SHAPE[u] - 1) * SIZES[u] * (SHAPE[w] - 1) * SIZES[w]
    total = math.fsum(surfaces.triangle_areas(v).tolist())
    assert abs(total - area) <= n * 2.0 ** -50 * area
    gradient = np.zeros(3)
    gradient[axis] = sign
    assert (normals(v) @ gradient < 0.0).all()


def test_an_oblique_plane_cuts_a_triangle_of_known_area_off_the_corner():
    levels, boxes, _ = one_level((8, 8, 8), [((0, 0, 0), (7, 7, 7))], (1.0, 1.0, 1.0),
                                 (0.0, 0.0, 0.0), lambda x, y, z: x + y + z)
    value = 4.8                                    # the centres start at (0.5, 0.5, 0.5)
    got = iso.isosurface(levels, [], 0, value, boxes, [(1.0, 1.0, 1.0)], (0.0, 0.0, 0.0))
    v = got["vertices"]
    n = v.shape[0]
    assert n > 10
    assert np.abs(v.sum(axis=2) - value).max() <= 4 * 2.0 ** -52 * value
    side = value - 1.5                             # x' + y' + z' = side cuts legs of that length
    area = math.sqrt(3.0) / 2.0 * side * side
    total = math.fsum(surfaces.triangle_areas(v).tolist())
    assert abs(total - area) <= n * 2.0 ** -50 * area
    assert (normals(v) @ np.ones(3) < 0.0).all()
    # the other side: the same surface, the normals reversed
    levels, boxes, _ = one_level((8, 8, 8), [((0, 0, 0), (7, 7, 7))], (1.0, 1.0, 1.0),
                                 (0.0, 0.0, 0.0), lambda x, y, z: -(x + y + z))
    other = iso.isosurface(levels, [], 0, -value, boxes, [(1.0, 1.0, 1.0)], (0.0, 0.0, 0.0))
    assert other["vertices"].shape[0] == n
    assert (normals(other["vertices"]) @ np.ones(3) > 0.0).all()


# ---- a closed sphere -------------------------------------------------------------------------------

SPHERE_GRIDS = [((8 * a, 8 * b, 8 * c), (8 * a + 7, 8 * b + 7, 8 * c + 7))
                for c in range(2) for b in range(2) for a in range(2)]
CENTRE = (7.9 + 1 / 3, 8.1 - 1 / 7, 7.7 + 1 / 11)


def sphere():
    field = lambda x, y, z: 30.0 - ((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2 +
                                    (z - CENTRE[2]) ** 2)
    levels, boxes, dense = one_level((16, 16, 16), SPHERE_GRIDS, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0),
                                     field)
    value = 1.0
    assert not (dense == value).any()              # no corner lies on the surface
    return iso.isosurface(levels, [], 0, value, boxes, [(1.0, 1.0, 1.0)], (0.0, 0.0, 0.0))


def test_a_sphere_across_eight_boxes_is_closed_oriented_and_of_genus_zero():
    got = sphere()
    v = got["vertices"]
    n = v.shape[0]
    assert n > 500 and got["skipped"] == 0
    keys = np.ascontiguousarray(v).view(np.uint64).reshape(n, 3, 3)
    names = {}
    welded = np.zeros((n, 3), dtype=np.int64)
    for t in range(n):
        for c in range(3):
            welded[t, c] = names.setdefault(tuple(keys[t, c].tolist()), len(names))
    directed = {}
    for t in range(n):
        for c in range(3):
            edge = (int(welded[t, c]), int(welded[t, (c + 1) % 3]))
            assert edge[0] != edge[1]
            directed[edge] = directed.get(edge, 0) + 1
    assert set(directed.values()) == {1}           # every directed edge once ...
    assert all((b, a) in directed for a, b in directed)        # ... and its reverse once
    assert len(names) - len(directed) // 2 + n == 2            # V - E + F
    # outward: the field falls away from the centre
    centroid = v.mean(axis=1)
    assert ((normals(v) * (centroid - np.array(CENTRE))).sum(axis=1) > 0.0).all()


def test_the_flux_of_a_constant_field_through_a_closed_surface_vanishes():
    got = sphere()
    area = math.fsum(surfaces.triangle_areas(got["vertices"]).tolist())
    n = got["vertices"].shape[0]
    assert abs(surfaces.surface_flux(got, 1.0, -2.0, 0.5)) <= n * 2.0 ** -50 * area * 3.5
    along = np.full((n, 3), 0.25)
    assert abs(surfaces.surface_flux(got["vertices"], along, 0.0, 0.0)) <= n * 2.0 ** -50 * area
    # F = x: the divergence theorem gives the volume, which lies near the ball's
    volume = surfaces.surface_flux(got, got["vertices"][:, :, 0], 0.0, 0.0)
    assert abs(volume / (4.0 / 3.0 * math.pi * 29.0 ** 1.5) - 1.0) < 0.05


# ---- the cubes of a hierarchy ----------------------------------------------------------------------

THREE_DOMAINS = [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (47, 23, 31))]
THREE_BOXES = [[((0, 0, 0), (6, 5, 7)), ((7, 0, 0), (11, 5, 7))],
               [((4, 2, 2), (11, 7, 9)), ((12, 2, 2), (17, 9, 9))],
               [((12, 6, 6), (21, 13, 15))]]


def scene_boxes(levels, ratio, min_level=0, max_level=-1):
    if max_level < 0:
        max_level = len(levels) - 1
    convex = plotfile.convexify([lev["boxes"] for lev in levels[:max_level + 1]], ratio[:max_level])
    return [(l, lo, hi) for l in range(min_level, max_level + 1) for _, (lo, hi) in convex[l]]


@pytest.mark.parametrize("loaded", [(0, -1), (1, -1), (0, 1)])
def test_the_surface_cubes_and_their_owners_equal_a_brute_force_enumeration(loaded):
    ratio = [2, 2]
    levels = ref.make_levels(THREE_DOMAINS, THREE_BOXES, ratio, 51)
    min_level, max_level = loaded
    boxes = scene_boxes(levels, ratio, min_level, max_level)
    sizes = ref.cell_sizes(levels, (0.0, 0.0, 0.0), (1.5, 0.75, 1.0))
    got = iso.isosurface(levels, ratio, 0, 0.1, boxes, sizes, (0.0, 0.0, 0.0), min_level, max_level)
    top = len(levels) - 1 if max_level < 0 else max_level
    leaves = [set() for _ in levels]
    for l in range(min_level, top + 1):
        for lo, hi in levels[l]["boxes"]:
            leaves[l].update((i, j, k) for k in range(lo[2], hi[2] + 1)
                             for j in range(lo[1], hi[1] + 1) for i in range(lo[0], hi[0] + 1))
        if l < top:
            for lo, hi in levels[l + 1]["boxes"]:
                leaves[l].difference_update(
                    (i, j, k) for k in range(lo[2] // 2, hi[2] // 2 + 1)
                    for j in range(lo[1] // 2, hi[1] // 2 + 1)
                    for i in range(lo[0] // 2, hi[0] // 2 + 1))
    holder = [dict() for _ in levels]
    for b, (l, lo, hi) in enumerate(boxes):
        for k in range(lo[2], hi[2] + 1):
            for j in range(lo[1], hi[1] + 1):
                for i in range(lo[0], hi[0] + 1):
                    holder[l][(i, j, k)] = b
    assert all(set(holder[l]) == leaves[l] for l in range(len(levels)))

    def present(l, g):
        for m in range(l, -1, -1):
            if g in leaves[m]:
                return True
            if m > 0:
                g = tuple(v // ratio[m - 1] for v in g)
        return False

    want = []
    for l in range(len(levels)):
        (dlo, dhi) = levels[l]["domain"]
        for k in range(dlo[2] - 1, dhi[2] + 1):
            for j in range(dlo[1] - 1, dhi[1] + 1):
                for i in range(dlo[0] - 1, dhi[0] + 1):
                    corners = [(i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)) for c in range(8)]
                    own = [g for g in corners if g in leaves[l]]
                    if own and all(present(l, g) for g in corners):
                        want.append((holder[l][own[0]], l, (i, j, k)))
    assert len(want) > 1000
    assert sorted(want) == sorted(got["cubes"])
    # the output order: by box, then k, j, i
    assert got["cubes"] == sorted(got["cubes"], key=lambda c: (c[0], c[2][2], c[2][1], c[2][0]))
    if loaded == (0, -1):
        # cubes of fine boxes reach into the coarse region, and none has a covered corner
        assert any(l == 2 and i == 11 for _, l, (i, _, _) in want)
        assert not any(l == 1 and (i, j, k) == (6, 3, 3) for _, l, (i, j, k) in want)


def test_the_tables_follow_the_rules():
    for mask in range(16):
        inside = [n for n in range(4) if mask >> n & 1]
        outside = [n for n in range(4) if not mask >> n & 1]
        if len(inside) in (0, 4):
            want = ()
        elif len(inside) == 1:
            want = tuple((inside[0], p) for p in outside)
        elif len(inside) == 3:
            want = tuple((outside[0], p) for p in inside)
        else:
            (a, b), (p, q) = inside, outside
            want = ((a, p), (a, q), (b, q), (b, p))
        assert iso.EDGES[mask] == want
    # every tetrahedron is a path from corner 0 to corner 7 that changes one axis a step; the six
    # paths are the six orders of the axes, and an order's parity is the tetrahedron's
    orders = set()
    for tet, odd in zip(iso.TETS, iso.TET_ODD):
        steps = [tet[n + 1] - tet[n] for n in range(3)]
        assert tet[0] == 0 and tet[3] == 7 and sorted(steps) == [1, 2, 4]
        order = [int(math.log2(s)) for s in steps]
        orders.add(tuple(order))
        inversions = sum(order[a] > order[b] for a in range(3) for b in range(a + 1, 3))
        assert inversions % 2 == odd
    assert len(orders) == 6


# ---- the host side of the API ----------------------------------------------------------------------

def test_a_ply_file_round_trips(tmp_path):
    rng = np.random.default_rng(52)
    v = rng.standard_normal((7, 3, 3))
    samples = {"density": rng.standard_normal((7, 3)), "t_2": rng.standard_normal((7, 3))}
    path = str(tmp_path / "surface.ply")
    surfaces.save_ply(v, path, samples)
    with open(path, "rb") as fh:
        head = fh.read(64)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 21\n")
    back, back_samples = surfaces.load_ply(path)
    assert ref.same_bits(back, v) and list(back_samples) == ["density", "t_2"]
    assert all(ref.same_bits(back_samples[k], samples[k]) for k in samples)
    assert os.path.getsize(path) == len(open(path, "rb").read().split(b"end_header\n")[0]) + 11 + \
        21 * 5 * 8 + 7 * 13
    surfaces.save_ply(np.zeros((0, 3, 3)), path)
    back, back_samples = surfaces.load_ply(path)
    assert back.shape == (0, 3, 3) and back_samples == {}
    with pytest.raises(ValueError):
        surfaces.save_ply(v, path, {"two words": samples["density"]})
    with pytest.raises(ValueError):
        surfaces.save_ply(v, path, {"short": samples["density"][:3]})
    with pytest.raises(ValueError):
        surfaces.save_ply(v[:, :2], path)


def test_the_entry_is_declared_and_the_abi_version_stays(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    assert "int avr_scene_isosurface(avr_context *ctx, const avr_scene *field" in header
    assert len(_capi.SIGNATURES["avr_scene_isosurface"][1]) == 14
    assert getattr(avr_lib, "avr_scene_isosurface") is not None
    assert avr_lib.avr_abi_version() == 2


def _tiny_plotfile(path):
    levels = ref.make_levels([((0, 0, 0), (3, 3, 3)), ((0, 0, 0), (7, 7, 7))],
                             [[((0, 0, 0), (3, 3, 3))], [((2, 2, 2), (5, 5, 5))]], [2], 53)
    plotfile.write_plotfile(str(path), list(ref.VARIABLES), levels, (0.0, 0.0, 0.0),
                            (1.0, 1.0, 1.0), [2])
    return str(path)


def _patched(monkeypatch, triangles):
    """api.isosurface without a device: _load_fields and isosurface_scene answer from `triangles`."""
    asked = []
    scene = lambda what: types.SimpleNamespace(local_boxes=what, scalar_transform=None)

    def fake_load_fields(plotfile_path, variables, min_level, max_level):
        return "ctx", 0, 1, None, [scene(name) for name in variables], [0.015625, 0.001953125]

    def fake_scene(ctx, inner, value, cell_sizes, prob_lo, ref_ratio, sample=None, rank=0,
                   n_ranks=1):
        assert ctx == "ctx" and inner.local_boxes == "u" and len(cell_sizes) == 2
        assert list(ref_ratio) == [2] and list(prob_lo) == [0.0, 0.0, 0.0]
        asked.append((value, None if sample is None else sample.local_boxes))
        n = triangles.shape[0]
        sampled = None if sample is None else np.full((n, 3), float(len(sample.local_boxes)))
        return triangles, np.ones(n, dtype=np.uint8), sampled, 4

    monkeypatch.setattr(api, "_load_fields", fake_load_fields)
    monkeypatch.setattr(api, "isosurface_scene", fake_scene)
    return asked


def test_api_isosurface_assembles_areas_samples_and_the_file(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    triangles = np.array([[[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 4.0, 0.0]],
                          [[1.0, 1.0, 1.0], [1.0, 1.0, 3.0], [1.0, 2.0, 1.0]]])
    asked = _patched(monkeypatch, triangles)
    out = str(tmp_path / "out.ply")
    got = api.isosurface(path, "u", 0.25, fields=["odd", "whole"], output=out)
    assert asked == [(0.25, "odd"), (0.25, "whole")]           # one emit call per field
    assert got["n"] == 2 and got["skipped"] == 4 and got["level"].tolist() == [1, 1]
    assert got["area"].tolist() == [6.0, 1.0] and got["total_area"] == 7.0
    assert got["samples"]["odd"].tolist() == [[3.0] * 3] * 2
    assert got["samples"]["whole"].tolist() == [[5.0] * 3] * 2
    back, back_samples = surfaces.load_ply(out)
    assert ref.same_bits(back, triangles) and list(back_samples) == ["odd", "whole"]
    bare = api.isosurface(path, "u", 0.25)
    assert asked[-1] == (0.25, None) and bare["samples"] == {} and bare["n"] == 2


def test_no_triangles_give_empty_arrays(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    _patched(monkeypatch, np.zeros((0, 3, 3)))
    got = api.isosurface(path, "u", 1e9, fields=["odd"], output=str(tmp_path / "none.ply"))
    assert got["n"] == 0 and got["vertices"].shape == (0, 3, 3) and got["area"].shape == (0,)
    assert got["total_area"] == 0.0 and got["level"].shape == (0,)
    assert got["samples"]["odd"].shape == (0, 3)
    assert surfaces.load_ply(str(tmp_path / "none.ply"))[0].shape == (0, 3, 3)


def test_boxes_on_other_ranks_and_values_that_are_not_finite_are_refused_before_device_work():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the context was used ({name})")

    box = AmrBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), level=0, dims=(4, 4, 4))
    bounds = VolumeBounds((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    whole = api.SceneGeometry([box, box], [box, box], ScalarTransform(), bounds)
    part = api.SceneGeometry([box, box], [box], ScalarTransform(), bounds)
    arguments = ([(0.25, 0.25, 0.25)], (0.0, 0.0, 0.0), [])
    with pytest.raises(NotImplementedError):
        api.isosurface_scene(NoDevice(), whole, 0.5, *arguments, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        api.isosurface_scene(NoDevice(), part, 0.5, *arguments)
    for value in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="finite"):
            api.isosurface_scene(NoDevice(), whole, value, *arguments)
