"""Particle groups on the GPU: the kernels of avr_particle_groups.hip through
avr_particle_group_cells and avr_particle_groups, Context.particle_group_cells / particle_groups and
api.particle_groups, against the all-pairs numpy reference (particle_group_reference), which has no
grid.  Labels, counts, roots, sizes, members, first, outside, cells and pair_tests are equal; there
is no tolerance on the grouping.  The catalogue's float sums are held to math.fsum of the same
terms within the a-priori bound of DESIGN.md 7, "Particle groups" (quotient_bound)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, groups, plotfile

import gradient_reference as ref
import particle_group_reference as pg

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
B = 0.02
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4096]


def clear_registries():
    for name in list(api.particle_fields()):
        api.remove_particle_field(name)


@pytest.fixture(autouse=True)
def _empty_registries():
    clear_registries()
    yield
    clear_registries()


@functools.lru_cache(maxsize=None)
def blobs(n):
    """A few Gaussian blobs on a uniform background in the unit box, 2 % of the particles with a
    NaN or an infinite coordinate; masses and velocities to go with them."""
    rng = np.random.default_rng(1000 + n)
    centres = rng.random((4, 3)) * 0.8 + 0.1
    which = rng.integers(0, 8, size=n)                       # 0..3: a blob; else the background
    points = rng.random((n, 3))
    in_blob = which < 4
    points[in_blob] = centres[which[in_blob]] + 0.012 * rng.standard_normal((int(in_blob.sum()), 3))
    bad = rng.random(n) < 0.02
    points[bad, rng.integers(0, 3, size=int(bad.sum()))] = \
        rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
    masses = rng.integers(1, 9, size=n).astype(np.float64) * 0.37
    velocities = rng.standard_normal((n, 3)) * 3.0 + 10.0
    for array in (points, masses, velocities):
        array.setflags(write=False)
    return points, masses, velocities


@functools.lru_cache(maxsize=None)
def blob_groups(n, min_members=1):
    return pg.groups(blobs(n)[0], B, *UNIT, min_members=min_members)


def flat_cells(points, lo, hi, dims, periodic=False):
    """The reference's cell of every particle as the kernel numbers it, all ones outside."""
    lo_, hi_, flags = pg.box_of(lo, hi, periodic)
    inside = pg.inside_of(points, lo_, hi_, flags)
    cells = np.full(len(points), NONE, dtype=np.uint32)
    at = pg.cell_of(np.asarray(points, dtype=np.float64)[inside], lo, hi, dims)
    cells[inside] = (at[:, 2] * dims[1] + at[:, 1]) * dims[0] + at[:, 0]
    return cells


def native(ctx, points, b, lo, hi, dims, periodic=False, min_members=1, totals=None):
    """Both native calls through the Context's wrappers, everything back on the host."""
    pts, cells, parent, totals = ctx.particle_group_cells(np.array(points), lo, hi, dims, periodic,
                                                          totals)
    labels, parent, sizes, n_groups, pair_tests = ctx.particle_groups(
        pts, cells, parent, b, lo, hi, dims, periodic, min_members)
    ctx.synchronize()
    return {"cells": cells.cpu().numpy().view(np.uint32),
            "parent": parent.cpu().numpy().view(np.uint32),
            "labels": labels.cpu().numpy(), "sizes": sizes.cpu().numpy().view(np.uint32),
            "count": int(n_groups.item()), "outside": int(totals.item()),
            "pair_tests": pair_tests}


def check(got, want, points, lo, hi, dims, periodic=False, min_members=1):
    """A native result against the reference's grouping and the definition's cells."""
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], want["labels"])
    assert got["count"] == want["count"] and got["outside"] == want["outside"]
    root = np.where(want["root"] < 0, NONE, want["root"]).astype(np.uint32)
    assert np.array_equal(got["parent"], root)
    sizes = np.zeros(len(points), dtype=np.uint32)
    inside = want["root"] >= 0
    if inside.any():
        sizes += np.bincount(want["root"][inside], minlength=len(points)).astype(np.uint32)
    assert np.array_equal(got["sizes"], sizes)
    assert np.array_equal(got["cells"], flat_cells(points, lo, hi, dims, periodic))
    assert got["pair_tests"] == pg.pair_tests(points, lo, hi, dims, periodic)


# ---- random particles --------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_blobs_on_a_background_with_bad_coordinates(ctx, n):
    points = blobs(n)[0]
    dims = groups.choose_dims(n, B, np.zeros(3), np.ones(3), (False,) * 3)
    got = native(ctx, points, B, *UNIT, dims)
    want = blob_groups(n)
    check(got, want, points, *UNIT, dims)
    if n == 4096:
        assert want["count"] > 100 and want["sizes"].max() > 200 and want["outside"] > 40


@pytest.mark.parametrize("grid", ["least", "double", "one"])
def test_the_groups_do_not_depend_on_the_grid(ctx, grid):
    points = blobs(4096)[0]
    slack = 1.0 + 2.0 ** -10
    dims = {"least": (int(1.0 / (B * slack)),) * 3, "double": (int(1.0 / (2.0 * B)),) * 3,
            "one": (1, 1, 1)}[grid]
    assert dims == {"least": (49, 49, 49), "double": (25, 25, 25), "one": (1, 1, 1)}[grid]
    got = native(ctx, points, B, *UNIT, dims)
    check(got, blob_groups(4096), points, *UNIT, dims)
    if grid == "one":                                         # every particle against every other
        inside = 4096 - got["outside"]
        assert got["pair_tests"] == inside * (inside - 1) // 2


@pytest.mark.parametrize("min_members", [1, 2, 20])
@pytest.mark.parametrize("n", [257, 4096])
def test_min_members(ctx, n, min_members):
    points = blobs(n)[0]
    dims = groups.choose_dims(n, B, np.zeros(3), np.ones(3), (False,) * 3)
    got = native(ctx, points, B, *UNIT, dims, min_members=min_members)
    want = blob_groups(n, min_members)
    check(got, want, points, *UNIT, dims, min_members=min_members)
    assert want["count"] < blob_groups(n)["count"] or min_members == 1


# ---- placed particles --------------------------------------------------------------------------------

def test_pairs_at_exactly_one_linking_length_and_an_ulp_either_side_across_a_cell_boundary(ctx):
    # cells of width 1 in a box of 4: the pairs straddle the boundary at 1.0 of their axis
    lo, hi, dims, b = (0.0, 0.0, 0.0), (4.0, 4.0, 4.0), (4, 4, 4), 0.5
    points, linked = [], []
    for axis in range(3):
        for variant, far in enumerate((1.25, np.nextafter(1.25, 0.0), np.nextafter(1.25, 2.0))):
            p = np.array([2.5, 2.5, 2.5])
            p[(axis + 1) % 3] = 0.25 + variant              # the pairs are far from each other
            p[(axis + 2) % 3] = 3.5
            q = p.copy()
            p[axis], q[axis] = 0.75, far
            points += [p, q]
            linked.append(variant < 2)
    points = np.array(points)
    got = native(ctx, points, b, lo, hi, dims)
    want = pg.groups(points, b, lo, hi)
    check(got, want, points, lo, hi, dims)
    for pair, together in enumerate(linked):
        assert (got["labels"][2 * pair] == got["labels"][2 * pair + 1]) == together
        assert got["cells"][2 * pair] != got["cells"][2 * pair + 1]
    assert got["count"] == 18 - sum(linked)


def test_a_shuffled_filament_through_many_cells_is_one_group(ctx):
    n, b = 3000, 5e-4
    rng = np.random.default_rng(31)
    step = 0.9 * b / math.sqrt(3.0)
    along = 0.1 + step * rng.permutation(n).astype(np.float64)
    points = np.stack([along, along, along], axis=1)
    dims = groups.choose_dims(n, b, np.zeros(3), np.ones(3), (False,) * 3)
    got = native(ctx, points, b, *UNIT, dims)
    assert got["count"] == 1 and bool((got["labels"] == 1).all())
    assert bool((got["parent"] == 0).all()) and got["sizes"][0] == n and got["sizes"][1:].sum() == 0
    assert len(np.unique(got["cells"])) >= 15
    # one link missing splits it: the reference agrees on both
    want = pg.groups(points, b, *UNIT)
    check(got, want, points, *UNIT, dims)
    broken = points[along != 0.1 + step * 1500]
    got = native(ctx, broken, b, *UNIT, dims)
    check(got, pg.groups(broken, b, *UNIT), broken, *UNIT, dims)
    assert got["count"] == 2 and sorted(got["sizes"][got["sizes"] > 0].tolist()) == [1499, 1500]


def test_coincident_points_in_one_cell(ctx):
    points = np.tile([[0.3, 0.6, 0.9]], (512, 1))
    got = native(ctx, points, 1e-3, *UNIT, (7, 7, 7), min_members=512)
    assert got["count"] == 1 and bool((got["labels"] == 1).all()) and got["sizes"][0] == 512
    assert got["pair_tests"] == 512 * 511 // 2 and len(np.unique(got["cells"])) == 1
    got = native(ctx, points, 1e-3, *UNIT, (7, 7, 7), min_members=513)
    assert got["count"] == 0 and not got["labels"].any() and got["sizes"][0] == 512


@pytest.mark.parametrize("axes", [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)])
def test_periodic_wraps_through_faces_edges_and_the_corner(ctx, axes):
    flags = tuple(d in axes for d in range(3))
    dims = tuple(3 if f else 5 for f in flags)
    b = 0.0625
    rng = np.random.default_rng(41 + sum(axes))
    p, q = np.full(3, 0.5), np.full(3, 0.5)
    for d in axes:
        p[d], q[d] = 0.015625, 1.0 - 0.015625
    # near the faces on both sides, at and past the period's ends, and a background
    near = rng.random((300, 3))
    depth = 0.03 * rng.random(300)
    near[:, axes[0]] = np.where(rng.random(300) < 0.5, depth, 1.0 - depth)
    ends = np.array([[0.0, 0.5, 0.5], [1.0, 0.5, 0.5], [0.5, 1.0, 0.5], [0.5, 0.5, -0.001],
                     [np.nextafter(1.0, 0.0)] * 3, [0.0, 0.0, 0.0], [1.2, -0.2, 0.5]])
    points = np.concatenate([[p, q], near, ends, rng.random((200, 3))])
    got = native(ctx, points, b, *UNIT, dims, flags)
    want = pg.groups(points, b, *UNIT, flags)
    check(got, want, points, *UNIT, dims, flags)
    assert got["labels"][0] == got["labels"][1] != 0
    open_box = native(ctx, points, b, *UNIT, dims)
    check(open_box, pg.groups(points, b, *UNIT), points, *UNIT, dims)
    assert open_box["labels"][0] != open_box["labels"][1]


def test_particles_beyond_a_plain_face_are_clamped_into_the_edge_cells(ctx):
    b, dims = 0.05, (8, 8, 8)
    rng = np.random.default_rng(47)
    placed = np.array([[-0.30, 0.5, 0.5], [-0.28, 0.5, 0.5], [-0.03, 0.5, 0.5], [0.01, 0.5, 0.5],
                       [1.7, 0.5, 0.5], [1.74, 0.5, 0.5], [0.99, 0.5, 0.5], [1.03, 0.5, 0.5],
                       [0.5, -3.0, 9.0], [0.5, -3.02, 9.03], [1e300, 0.5, 0.5], [-1e300, 0.5, 0.5]])
    points = np.concatenate([placed, rng.random((400, 3)) * 1.6 - 0.3])
    got = native(ctx, points, b, *UNIT, dims)
    want = pg.groups(points, b, *UNIT)
    check(got, want, points, *UNIT, dims)
    assert got["outside"] == 0
    for first in (0, 2, 4, 6, 8):
        assert got["labels"][first] == got["labels"][first + 1]
    assert got["cells"][0] == got["cells"][3] and got["cells"][10] != got["cells"][11]


# ---- the native contract -----------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_the_outputs_untouched(ctx):
    n, device = 300, ctx.device
    points_host = blobs(4096)[0][:n]
    points = torch.from_numpy(np.array(points_host)).to(device)
    dims = (6, 5, 4)
    _, cells_ok, parent_ok, _ = ctx.particle_group_cells(points, *UNIT, dims, False)
    keys, order = torch.sort(cells_ok.to(torch.int64) & NONE, stable=True)
    cell_begin = torch.searchsorted(
        keys, torch.arange(121, dtype=torch.int64, device=device)).contiguous()
    ordered = points[order].contiguous()
    n_inside = int(cell_begin[-1].item())
    cells = torch.full((n,), 7, dtype=torch.int32, device=device)
    parent = torch.full((n,), 8, dtype=torch.int32, device=device)
    labels = torch.full((n,), 9, dtype=torch.int32, device=device)
    sizes = torch.full((n,), 10, dtype=torch.int32, device=device)
    totals = torch.tensor([11], dtype=torch.int64, device=device)
    n_groups = torch.tensor([12], dtype=torch.int64, device=device)

    def untouched():
        ctx.synchronize()
        return bool((cells == 7).all()) and bool((parent == 8).all()) and \
            bool((labels == 9).all()) and bool((sizes == 10).all()) and \
            totals.tolist() == [11] and n_groups.tolist() == [12]

    ints = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    doubles = lambda a: None if a is None else \
        np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    pointer = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def locate(points=points, n=n, lo=UNIT[0], hi=UNIT[1], dims=dims, periodic=(0, 0, 0),
               cells=cells, parent=parent, totals=totals):
        return _capi.lib().avr_particle_group_cells(
            ctx._handle, pointer(points), n, doubles(lo), doubles(hi), ints(dims), ints(periodic),
            pointer(cells), pointer(parent), pointer(totals))

    def link(points=ordered, order=order, cell_begin=cell_begin, n=n, n_inside=n_inside, b=B,
             lo=UNIT[0], hi=UNIT[1], dims=dims, periodic=(0, 0, 0), min_members=1, parent=parent,
             labels=labels, sizes=sizes, n_groups=n_groups):
        return _capi.lib().avr_particle_groups(
            ctx._handle, pointer(points), pointer(order), pointer(cell_begin), n, n_inside, b,
            doubles(lo), doubles(hi), ints(dims), ints(periodic), min_members, pointer(parent),
            pointer(labels), pointer(sizes), pointer(n_groups))

    box = "lo and hi must be finite with lo < hi"
    wrong = [
        (locate, dict(points=None), "null argument"),
        (locate, dict(cells=None), "null argument"),
        (locate, dict(parent=None), "null argument"),
        (locate, dict(totals=None), "null argument"),
        (locate, dict(lo=None), "null argument"),
        (locate, dict(n=2 ** 31), "n must stay below 2^31"),
        (locate, dict(lo=(0.0, math.nan, 0.0)), box),
        (locate, dict(hi=(1.0, 1.0, 0.0)), box),
        (locate, dict(dims=(6, 0, 4)), "dims must lie in [1, 1024]"),
        (locate, dict(dims=(6, 5, 1025)), "dims must lie in [1, 1024]"),
        (locate, dict(dims=(1024, 1024, 128)), "the grid must hold fewer than 2^27 cells"),
        (locate, dict(dims=(6, 2, 4), periodic=(0, 1, 0)), "a periodic axis needs at least 3 cells"),
        (locate, dict(parent=cells), "two output arrays overlap"),
        (locate, dict(totals=parent.view(torch.int64)), "two output arrays overlap"),
        (locate, dict(points=cells.view(torch.float64)), "an output array overlaps the points"),
        (link, dict(points=None), "null argument"),
        (link, dict(order=None), "null argument"),
        (link, dict(cell_begin=None), "null argument"),
        (link, dict(labels=None), "null argument"),
        (link, dict(n_groups=None), "null argument"),
        (link, dict(n=0, n_inside=0, n_groups=None), "null argument"),
        (link, dict(n=2 ** 31), "n must stay below 2^31"),
        (link, dict(n_inside=n + 1), "n_inside must not exceed n"),
        (link, dict(b=0.0), "the linking length must be finite and positive"),
        (link, dict(b=math.inf), "the linking length must be finite and positive"),
        (link, dict(hi=(1.0, math.inf, 1.0)), box),
        (link, dict(dims=(0, 5, 4)), "dims must lie in [1, 1024]"),
        (link, dict(dims=(6, 5, 2), periodic=(0, 0, 1)), "a periodic axis needs at least 3 cells"),
        (link, dict(b=0.2), "a cell must be at least (1 + 2^-10) linking lengths wide"),
        (link, dict(b=1.0 / 6.0), "a cell must be at least (1 + 2^-10) linking lengths wide"),
        (link, dict(min_members=0), "min_members must lie in [1, 2^31)"),
        (link, dict(min_members=2 ** 31), "min_members must lie in [1, 2^31)"),
        (link, dict(labels=parent), "two output arrays overlap"),
        (link, dict(n_groups=sizes.view(torch.int64)), "two output arrays overlap"),
        (link, dict(labels=order.view(torch.int32)),
         "an output array overlaps the points, the order or the cell ranges"),
        (link, dict(sizes=ordered.view(torch.int32)),
         "an output array overlaps the points, the order or the cell ranges"),
    ]
    for call, arguments, message in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert _capi.lib().avr_last_error().decode() == message, arguments
        assert untouched(), arguments
    # n == 0 launches nothing; the groups' call still sets n_groups to 0
    assert locate(n=0, points=None, cells=None, parent=None, totals=None) == 0
    assert untouched()
    assert link(n=0, n_inside=0, points=None, order=None, cell_begin=None, parent=None,
                labels=None, sizes=None) == 0
    ctx.synchronize()
    assert n_groups.tolist() == [0]
    n_groups.fill_(12)
    assert untouched()
    # the calls that are in order write everything, and the prefilled totals are added to
    assert locate() == 0
    ctx.synchronize()
    want = pg.groups(points_host, B, *UNIT)
    assert totals.tolist() == [11 + want["outside"]]
    assert torch.equal(cells, cells_ok) and torch.equal(parent, parent_ok)
    assert link() == 0
    ctx.synchronize()
    assert np.array_equal(labels.cpu().numpy(), want["labels"])
    assert n_groups.tolist() == [want["count"]]


def test_two_runs_of_one_call_are_equal_by_bits(ctx):
    points = blobs(4096)[0]
    dims = (25, 25, 25)
    totals = torch.tensor([1000], dtype=torch.int64, device=ctx.device)
    runs = [native(ctx, points, B, *UNIT, dims, min_members=2, totals=totals) for _ in range(2)]
    for key in ("cells", "parent", "labels", "sizes"):
        assert runs[0][key].tobytes() == runs[1][key].tobytes()
    assert runs[0]["count"] == runs[1]["count"] and runs[0]["pair_tests"] == runs[1]["pair_tests"]
    outside = blob_groups(4096)["outside"]
    assert runs[0]["outside"] == 1000 + outside and runs[1]["outside"] == 1000 + 2 * outside


# ---- through api.particle_groups ---------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 257, 4096])
def test_the_member_lists_and_the_catalogue(ctx, n, tmp_path):
    points, masses, velocities = blobs(n)
    least = 3
    output = str(tmp_path / "groups.npz")
    got = api.particle_groups(points, B, masses=masses, velocities=velocities, min_members=least,
                              domain=UNIT, output=output, ctx=ctx)
    want = blob_groups(n, least)
    assert got["n"] == n and got["count"] == want["count"] and got["outside"] == want["outside"]
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], want["labels"])
    for key in ("first", "offsets", "members"):
        assert got[key].dtype == np.int64 and np.array_equal(got[key], want[key]), key
    assert got["dims"] == groups.choose_dims(n, B, np.zeros(3), np.ones(3), (False,) * 3)
    assert got["pair_tests"] == pg.pair_tests(points, *UNIT, got["dims"])
    # the float sums against fsum of the same terms
    exact = pg.fsum_catalogue(points, want["labels"], want["count"], masses, velocities,
                              got["velocity"])
    worst = 0.0
    for g in range(want["count"]):
        size, mass = exact["size"][g], exact["mass"][g]
        bound = size * pg.U * exact["mass_abs"][g]
        worst = max(worst, abs(got["mass"][g] - mass) / bound)
        assert abs(got["mass"][g] - mass) <= bound
        for d in range(3):
            for key, top, top_abs in (("centre", "moment", "moment_abs"),
                                      ("velocity", "momentum", "momentum_abs")):
                bound = pg.quotient_bound(size, exact[top][g][d], exact[top_abs][g][d], mass,
                                          exact["mass_abs"][g])
                error = abs(got[key][g, d] - exact[top][g][d] / mass)
                worst = max(worst, error / bound)
                assert error <= bound, (key, g, d, error, bound)
        # the dispersion: the quotient's bound through 3 mass, then the square root's rounding
        variance = exact["spread"][g] / (3.0 * mass)
        bound = pg.quotient_bound(size, exact["spread"][g], exact["spread_abs"][g], 3.0 * mass,
                                  3.0 * exact["mass_abs"][g]) + 2.0 * pg.U * variance
        sigma = math.sqrt(variance)
        if variance > 0.0:
            # |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= |a - b| / sqrt(b)
            bound = bound / sigma + 2.0 * pg.U * sigma
            error = abs(got["dispersion"][g] - sigma)
            worst = max(worst, error / bound)
            assert error <= bound, ("dispersion", g, error, bound)
        else:
            assert got["dispersion"][g] == 0.0
    print("worst fraction of the bound", n, worst)
    # the file holds the dict
    with np.load(output) as held:
        assert sorted(held.files) == sorted(got)
        for key, value in got.items():
            assert np.array_equal(held[key], np.asarray(value), equal_nan=True), key
    # without masses and velocities: unit masses, no velocity entries; without a domain: the
    # bounding box, and the same groups
    plain = api.particle_groups(points, B, min_members=least, ctx=ctx)
    assert "velocity" not in plain and "dispersion" not in plain
    assert np.array_equal(plain["labels"], want["labels"])
    assert np.array_equal(plain["mass"], np.diff(want["offsets"]).astype(np.float64))
    as_tensor = api.particle_groups(torch.from_numpy(np.array(points)), B, min_members=least,
                                    domain=UNIT, ctx=ctx)
    assert np.array_equal(as_tensor["labels"], want["labels"])


def test_a_periodic_domain_through_the_api(ctx):
    rng = np.random.default_rng(53)
    lo, hi = (-1.0, 0.0, 2.0), (1.0, 4.0, 3.0)
    blob = np.array([-0.98, 3.97, 2.5]) + 0.03 * rng.standard_normal((60, 3))
    points = np.concatenate([blob, np.array(lo) + rng.random((500, 3)) * (np.array(hi) - lo)])
    masses = rng.integers(1, 5, size=len(points)).astype(np.float64)
    b = 0.06
    got = api.particle_groups(points, b, masses=masses, min_members=5, domain=(lo, hi),
                              periodic=True, ctx=ctx)
    want = pg.groups(points, b, lo, hi, True, 5)
    assert np.array_equal(got["labels"], want["labels"]) and got["count"] == want["count"] >= 1
    assert got["outside"] == want["outside"] > 0
    assert np.array_equal(got["members"], want["members"])
    assert got["pair_tests"] == pg.pair_tests(points, lo, hi, got["dims"], True)
    # the blob straddles the x and y faces: its centre lies in the domain, near the corner
    g = int(np.argmax(np.diff(got["offsets"])))
    centre = got["centre"][g]
    assert all(lo[d] <= centre[d] < hi[d] for d in range(3))
    wrapped = np.array([-0.98, 3.97, 2.5])
    gap = np.abs(centre - wrapped)
    gap = np.minimum(gap, np.array(hi) - lo - gap)
    assert float(gap.max()) < 0.03
    mixed = api.particle_groups(points, b, min_members=5, domain=(lo, hi),
                                periodic=(True, False, False), ctx=ctx)
    assert np.array_equal(mixed["labels"], pg.groups(points, b, lo, hi, (True, False, False),
                                                     5)["labels"])


def test_max_pair_tests_refuses_the_coincident_case_before_the_link(ctx, monkeypatch):
    points = np.tile([[0.3, 0.6, 0.9]], (512, 1))
    launched = []
    from amrvolumerenderer_amd import runtime

    def spy(ctx_, entry, *arguments):
        launched.append(entry)
        return real_native(ctx_, entry, *arguments)

    real_native = runtime._native
    monkeypatch.setattr(runtime, "_native", spy)
    with pytest.raises(ValueError, match=r"130816 pairs.*max_pair_tests = 1000.*smaller linking"):
        api.particle_groups(points, 1e-3, min_members=1, domain=UNIT, max_pair_tests=1000, ctx=ctx)
    assert launched == ["avr_particle_group_cells"]
    got = api.particle_groups(points, 1e-3, min_members=1, domain=UNIT, max_pair_tests=130816,
                              ctx=ctx)
    assert launched == ["avr_particle_group_cells"] * 2 + ["avr_particle_groups"]
    assert got["count"] == 1 and got["pair_tests"] == 130816


def test_the_largest_group_deposited_as_a_particle_field(ctx, tmp_path):
    """The README's example on one level of 16 x 8 x 8 cells: the largest group's members go
    through add_particle_field, and the projection's sum times the pixel area is that group's
    mass."""
    lo, hi = (0.0, 0.0, 0.0), (2.0, 1.0, 1.0)
    levels = ref.make_levels([((0, 0, 0), (15, 7, 7))], [[((0, 0, 0), (15, 7, 7))]], [], 74)
    path = str(tmp_path / "flat")
    plotfile.write_plotfile(path, list(ref.VARIABLES), levels, lo, hi, [])
    rng = np.random.default_rng(59)
    quarter = 0.125 / 4.0                                     # a quarter of a cell: dyadic
    halo = np.array([1.25, 0.5, 0.5]) + quarter * rng.integers(-3, 4, size=(80, 3))
    small = np.array([0.5, 0.25, 0.75]) + quarter * rng.integers(-1, 2, size=(30, 3))
    field = np.array(lo) + quarter * np.stack([rng.integers(0, 64, size=200),
                                               rng.integers(0, 32, size=200),
                                               rng.integers(0, 32, size=200)], axis=1)
    positions = np.concatenate([field[:100], halo, field[100:], small])
    masses = rng.integers(1, 60, size=len(positions)).astype(np.float64)
    b = 2.5 * quarter
    found = api.particle_groups(positions, b, masses=masses, min_members=20, domain=path, ctx=ctx)
    want = pg.groups(positions, b, lo, hi, False, 20)
    assert np.array_equal(found["labels"], want["labels"]) and found["count"] >= 2
    g = int(np.argmax(np.diff(found["offsets"])))
    members = found["members"][found["offsets"][g]:found["offsets"][g + 1]]
    assert len(members) >= 80 and set(range(100, 180)) <= set(members.tolist())
    api.add_particle_field("halo", positions[members], masses[members])
    image = api.project_axis(path, "z", "halo", width=16, height=8)
    assert float(image.sum()) * (0.125 * 0.125) == float(masses[members].sum()) == found["mass"][g]
