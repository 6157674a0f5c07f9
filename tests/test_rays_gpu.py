"""Rays on the GPU: the kernel of avr_rays.hip through avr_scene_rays, api.ray_scene and api.rays,
against the reference on the plotfile's own level arrays (ray_reference).  Counts, status, spans,
t0, t1, levels, values, integrals and covered lengths are equal by bits.  Cell sizes are powers of
two, and every coarse cell that a finer grid covers holds 1e30: a read of a parent grid past a
leaf box's view would show as a wrong value."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, plotfile
from amrvolumerenderer_amd import rays as ray_rules

import derive_reference
import gradient_reference as ref
import ray_reference as rr

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)


@pytest.fixture(autouse=True)
def _empty_registries():
    def clear():
        for name in list(api.clump_fields()):
            api.remove_clump_field(name)
        for name in list(api.gradient_fields()):
            api.remove_gradient_field(name)
        for name in list(api.derived_fields()):
            api.remove_field(name)
    clear()
    yield
    clear()


@dataclasses.dataclass(eq=False)
class Case:
    path: str
    levels: list
    lo: tuple
    hi: tuple
    ratio: list
    cache: dict = dataclasses.field(default_factory=dict)

    def sizes(self):
        return ref.cell_sizes(self.levels, self.lo, self.hi)

    def scene_boxes(self, min_level=0, max_level=-1):
        """(level, lo, hi) of every scene box, in the loader's order."""
        if max_level < 0:
            max_level = len(self.levels) - 1
        convex = plotfile.convexify([lev["boxes"] for lev in self.levels[:max_level + 1]],
                                    self.ratio[:max_level])
        return [(l, lo, hi) for l in range(min_level, max_level + 1) for _, (lo, hi) in convex[l]]

    def reference(self, name, min_level=0, max_level=-1):
        """The reference's hierarchy of one field, made once."""
        key = (name, min_level, max_level)
        if key not in self.cache:
            self.cache[key] = rr.Hierarchy(self.levels, self.ratio, VARIABLES.index(name),
                                           self.sizes(), self.lo, min_level, max_level)
        return self.cache[key]

    def wanted(self, name, n, max_trips=None, min_level=0, max_level=-1):
        """The reference's answer for the first n rays of the pool, computed once."""
        key = ("rays", name, n, max_trips, min_level, max_level)
        if key not in self.cache:
            hierarchy = self.reference(name, min_level, max_level)
            start, end = self.rays(n)
            self.cache[key] = hierarchy.rays(
                start, end, hierarchy.default_max_trips() if max_trips is None else max_trips)
        return self.cache[key]

    def rays(self, n):
        """The first n rays of a pool of 256: one of every status, rays that start or end outside,
        the domain's diagonals, rays on faces and edges of boxes (which are also coarse-fine
        interfaces) and through their corners, axis rays through cell centres, generic rays."""
        if "pool" not in self.cache:
            lo, hi = np.array(self.lo), np.array(self.hi)
            size = hi - lo
            at = lambda *f: lo + np.array(f) * size
            inside, other = at(0.2, 0.3, 0.3), at(0.8, 0.65, 0.9)
            pairs = [(inside, other),                                        # in order
                     (at(-0.6, -1.0, 0.5), at(-0.3, 2.0, 0.5)),              # passes beside
                     (at(1.3, 0.5, 0.5), at(2.0, 0.6, 0.6)),                 # wholly outside
                     (inside, inside),                                       # A == B
                     ([math.nan, inside[1], inside[2]], other),
                     (inside, [other[0], math.inf, other[2]]),
                     (at(-0.3, 0.3, 0.3), inside), (inside, at(-0.3, 0.3, 0.3)),
                     (lo, hi), (hi, lo), (at(0, 1, 0), at(1, 0, 1)), (at(1, 1, 0), at(0, 0, 1)),
                     (lo - size, hi + size),
                     (at(-0.5, 1.0, 0.5), at(1.5, 1.0, 0.5)),                # on the high face: a miss
                     (at(-0.5, 0.0, 0.0), at(1.5, 0.0, 0.0))]                # on the low edge: inside
            sizes = self.sizes()
            for level, blo, bhi in self.scene_boxes():
                dx = np.array(sizes[level])
                low, high = lo + np.array(blo) * dx, lo + (np.array(bhi) + 1) * dx
                middle = 0.5 * (low + high)
                # along x in the box's low y face, and along its low (y, z) edge
                pairs.append(([lo[0] - 0.25, low[1], middle[2] + 0.3 * dx[2]],
                              [hi[0] + 0.25, low[1], middle[2] + 0.3 * dx[2]]))
                pairs.append(([hi[0] + 0.25, low[1], low[2]], [lo[0] - 0.25, low[1], low[2]]))
                # along z in the box's high x face; along y through its high corner
                pairs.append(([high[0], middle[1] + 0.3 * dx[1], lo[2] - 0.5],
                              [high[0], middle[1] + 0.3 * dx[1], hi[2] + 0.5]))
                pairs.append(([high[0], hi[1] + 0.5, high[2]], [high[0], lo[1] - 0.5, high[2]]))
                # through the low and the high corner along the cell diagonal, and generically
                pairs.append((low - 3.0 * dx, low + 3.0 * dx))
                pairs.append((high + 2.0 * dx, high - 5.0 * dx))
                pairs.append((low - dx * np.array([0.7, 1.3, 0.4]), low + dx * np.array([1.4, 2.6, 0.8])))
                # through the centres of a row of cells
                pairs.append(([lo[0], middle[1] + 0.5 * dx[1], middle[2] + 0.5 * dx[2]],
                              [hi[0], middle[1] + 0.5 * dx[1], middle[2] + 0.5 * dx[2]]))
            s = np.arange(1, 257, dtype=np.float64)[:, None]
            fa = np.mod(s * np.array([math.sqrt(2.0), math.sqrt(3.0), math.sqrt(5.0)]), 1.0)
            fb = np.mod(s * np.array([math.sqrt(7.0), math.sqrt(11.0), math.sqrt(13.0)]) + 0.37, 1.0)
            grow = lambda f: lo + (f * 1.4 - 0.2) * size
            start = np.concatenate([np.array([p[0] for p in pairs], dtype=np.float64), grow(fa)])
            end = np.concatenate([np.array([p[1] for p in pairs], dtype=np.float64), grow(fb)])
            self.cache["pool"] = (np.ascontiguousarray(start[:256]), np.ascontiguousarray(end[:256]))
        start, end = self.cache["pool"]
        assert n <= start.shape[0]
        return start[:n], end[:n]


def _write(path, domains, boxes, lo, hi, ratio, seed):
    levels = ref.make_levels(domains, boxes, ratio, seed)
    case = Case(str(path), levels, lo, hi, list(ratio))
    for size in case.sizes():
        assert all(np.frexp(s)[0] == 0.5 for s in size)             # powers of two
    plotfile.write_plotfile(str(path), VARIABLES, levels, lo, hi, ratio)
    return case


THREE_DOMAINS = [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (47, 23, 31))]
# two fine boxes that touch at i = 11 | 12; the finest grid lies inside the first
THREE_BOXES = [[((0, 0, 0), (6, 5, 7)), ((7, 0, 0), (11, 5, 7))],
               [((4, 2, 2), (11, 7, 9)), ((12, 2, 2), (17, 9, 9))],
               [((12, 6, 6), (21, 13, 15))]]


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("rays") / "three", THREE_DOMAINS, THREE_BOXES,
                  (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2], 91)


@pytest.fixture(scope="module")
def ratio_four(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("rays") / "four",
                  [((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (23, 15, 15))],
                  [[((0, 0, 0), (5, 3, 3))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (3.0, 2.0, 2.0), [4], 93)


def load(ctx, case, name, min_level=0, max_level=-1):
    return plotfile.load_plotfile_geometry(ctx, case.path, name, min_level, max_level, False, True)


KEYS = ("offsets", "status", "t_enter", "t_leave", "t0", "t1", "level", "value", "integral",
        "covered")


def same_rays(got, want):
    counts = np.diff(want["offsets"])
    print("rays:", counts.size, "segments:", int(got["offsets"][-1]), "reference:",
          int(want["offsets"][-1]), "status:", np.bincount(got["status"], minlength=4).tolist(),
          "reference:", np.bincount(want["status"], minlength=4).tolist())
    assert np.array_equal(got["offsets"], want["offsets"]) and got["offsets"].dtype == np.int64
    assert got["status"].dtype == np.uint8 and np.array_equal(got["status"], want["status"])
    assert got["level"].dtype == np.int8 and np.array_equal(got["level"], want["level"])
    for key in ("t_enter", "t_leave", "t0", "t1", "value", "integral", "covered"):
        assert ref.same_bits(got[key], want[key]), key


def check(ctx, case, name, n, max_trips=None, min_level=0, max_level=-1):
    scene = load(ctx, case, name, min_level, max_level)
    finest = max(b.level for b in scene.all_boxes)
    start, end = case.rays(n)
    got = api.ray_scene(ctx, scene, start, end, case.sizes()[:finest + 1], case.lo,
                        case.ratio[:finest], max_trips)
    want = case.wanted(name, n, max_trips, min_level, max_level)
    same_rays(got, want)
    return got, scene


# ---- hierarchy -----------------------------------------------------------------------------------

def test_three_levels_with_fine_boxes_that_touch(ctx, three):
    got, scene = check(ctx, three, "u", 256)
    assert {b.level for b in scene.local_boxes} == {0, 1, 2}
    assert got["status"][:6].tolist() == [0, 1, 1, 3, 3, 3] and got["status"][13] == 1
    assert set(got["level"].tolist()) == {0, 1, 2} and (got["status"] == 2).sum() == 0
    assert (got["status"] == 0).sum() > 150 and got["offsets"][-1] > 2000


def test_nan_and_infinite_cells_are_values_but_not_integrated(ctx, three):
    got, _ = check(ctx, three, "odd", 256)
    assert (~np.isfinite(got["value"])).sum() > 10 and np.isfinite(got["integral"]).all()


def test_ratio_four(ctx, ratio_four):
    got, _ = check(ctx, ratio_four, "u", 120)
    assert set(got["level"].tolist()) == {0, 1}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_the_one_wave_workgroup_edge(ctx, three, n):
    check(ctx, three, "whole", n)


@pytest.mark.parametrize("levels", [(1, -1), (0, 1), (1, 1)])
def test_level_cuts_leave_holes_and_whole_coarse_grids(ctx, three, levels):
    got, scene = check(ctx, three, "u", 256, None, *levels)
    if levels[0] == 1:
        assert 0 not in {b.level for b in scene.local_boxes}
        absent = got["level"] < 0
        assert absent.sum() > 10 and np.isnan(got["value"][absent]).all()
    else:
        assert (got["level"] >= 0).all()


def test_max_trips_truncates_and_the_passes_agree(ctx, three):
    got, _ = check(ctx, three, "u", 256, 3)
    counts = np.diff(got["offsets"])
    assert (got["status"] == 2).sum() > 150 and counts.max() <= 3
    assert ((got["status"] == 2) | (counts <= 3)).all()
    got, _ = check(ctx, three, "u", 65, 1)
    assert np.diff(got["offsets"]).max() == 1


def test_a_repeat_gives_equal_bits(ctx, three):
    scene = load(ctx, three, "odd")
    start, end = three.rays(256)
    runs = [api.ray_scene(ctx, scene, start, end, three.sizes(), three.lo, three.ratio)
            for _ in range(2)]
    for key in KEYS:
        assert runs[0][key].tobytes() == runs[1][key].tobytes(), key


# ---- the C ABI -------------------------------------------------------------------------------------

def test_wrong_arguments_leave_the_outputs_untouched_and_a_ray_keeps_to_its_range(ctx, three):
    u = load(ctx, three, "u")
    su = ctx.create_scene(u.local_boxes, u.scalar_transform)
    n, max_trips = 65, 5
    start_host, end_host = three.rays(n)
    want = three.wanted("u", n, max_trips)
    counts_want = np.diff(want["offsets"])
    # every ray's range one slot longer than its count: the slot after a ray's last segment
    room = np.concatenate([[0], np.cumsum(counts_want + 1)]).astype(np.int64)
    total = int(room[-1])
    device = ctx.device
    start = torch.from_numpy(start_host).to(device)
    end = torch.from_numpy(end_host).to(device)
    offsets = torch.from_numpy(room).to(device)
    counts = torch.full((n,), -7, dtype=torch.int32, device=device)
    status = torch.full((n,), 9, dtype=torch.uint8, device=device)
    span = torch.full((n, 2), 0.5, dtype=torch.float64, device=device)
    pad = 16                                    # slots past n_segments
    t0 = torch.full((total + pad,), 0.25, dtype=torch.float64, device=device)
    t1 = torch.full((total + pad,), 0.25, dtype=torch.float64, device=device)
    level = torch.full((total + pad,), 77, dtype=torch.int8, device=device)
    value = torch.full((total + pad,), 0.25, dtype=torch.float64, device=device)
    integral = torch.full((n,), 0.125, dtype=torch.float64, device=device)
    covered = torch.full((n,), 0.125, dtype=torch.float64, device=device)
    index = np.array([lo for _, lo, _ in three.scene_boxes()], dtype=np.int32)

    def untouched():
        ctx.synchronize()
        return bool((counts == -7).all()) and bool((status == 9).all()) and \
            bool((span == 0.5).all()) and bool((t0 == 0.25).all()) and bool((t1 == 0.25).all()) \
            and bool((level == 77).all()) and bool((value == 0.25).all()) and \
            bool((integral == 0.125).all()) and bool((covered == 0.125).all())

    def call(field=su, start=start, end=end, n_rays=n, max_trips=max_trips, index=index,
             ratio=(2, 2), sizes=None, prob_lo=None, n_levels=3, offsets=None, n_segments=0,
             counts=counts, status=status, span=span, t0=t0, t1=t1, level=level, value=value,
             integral=integral, covered=covered):
        index = np.ascontiguousarray(index, np.int32)
        ratio = np.ascontiguousarray(ratio, np.int32)
        sizes = np.ascontiguousarray(three.sizes() if sizes is None else sizes, np.float64)
        prob_lo = np.ascontiguousarray(three.lo if prob_lo is None else prob_lo, np.float64)
        pointer = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        return _capi.lib().avr_scene_rays(
            ctx._handle, field._handle, pointer(start), pointer(end), n_rays, max_trips,
            index.ctypes.data_as(C.POINTER(C.c_int32)), ratio.ctypes.data_as(C.POINTER(C.c_int32)),
            sizes.ctypes.data_as(C.POINTER(C.c_double)),
            prob_lo.ctypes.data_as(C.POINTER(C.c_double)), n_levels, pointer(offsets), n_segments,
            pointer(counts), pointer(status), pointer(span), pointer(t0), pointer(t1),
            pointer(level), pointer(value), pointer(integral), pointer(covered))

    def message():
        return _capi.lib().avr_last_error().decode()

    inside = u.local_boxes[1].values          # an output array that is an input box's cells
    bad_sizes = np.array(three.sizes())
    bad_sizes[1, 2] = 0.0
    far = index.copy()
    far[0, 0] = 2 ** 30
    emit = dict(offsets=offsets, n_segments=total)
    wrong = [
        (dict(max_trips=0), "max_trips must lie in [1, 2^30]"),
        (dict(max_trips=2 ** 30 + 1), "max_trips must lie in [1, 2^30]"),
        (dict(n_rays=2 ** 32), "n_rays must stay below 2^32"),
        (dict(n_segments=2 ** 40 + 1, offsets=offsets), "n_segments must not exceed 2^40"),
        (dict(n_levels=0), "n_levels must lie in [1, 16]"),
        (dict(n_levels=2), "a box's level is not below n_levels"),
        (dict(start=None), "null argument"),
        (dict(counts=None), "null argument"),
        (dict(span=None), "null argument"),
        (dict(t0=None, **emit), "null argument"),
        (dict(covered=None, **emit), "null argument"),
        (dict(sizes=bad_sizes), "level_cell_size must be finite and positive"),
        (dict(prob_lo=(0.0, math.nan, 0.0)), "prob_lo must be finite"),
        (dict(ratio=(2, 1)), "a level ratio is below 2"),
        (dict(index=far), "a box's index range leaves [-2^30, 2^30)"),
        (dict(span=inside), "an output array or the rays overlap an input box's cells"),
        (dict(end=inside), "an output array or the rays overlap an input box's cells"),
        (dict(value=inside, **emit), "an output array or the rays overlap an input box's cells"),
    ]
    for arguments, text in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert text in message(), (arguments, message())
        assert untouched(), arguments
    assert call(n_rays=0) == 0 and call(n_rays=0, **emit) == 0 and untouched()   # no launch
    # the count pass writes its three arrays and nothing else
    assert call() == 0
    ctx.synchronize()
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), counts_want)
    assert np.array_equal(status.cpu().numpy(), want["status"])
    assert ref.same_bits(span.cpu().numpy()[:, 0], want["t_enter"])
    assert ref.same_bits(span.cpu().numpy()[:, 1], want["t_leave"])
    assert bool((t0 == 0.25).all()) and bool((value == 0.25).all()) and \
        bool((level == 77).all()) and bool((integral == 0.125).all())
    # the emit pass writes a ray's segments at its offset, and neither the slot after them nor
    # the slots past n_segments
    counts.fill_(-7)
    status.fill_(9)
    assert call(**emit) == 0
    ctx.synchronize()
    assert bool((counts == -7).all()) and bool((status == 9).all())
    got = {"t0": t0.cpu().numpy(), "t1": t1.cpu().numpy(), "level": level.cpu().numpy(),
           "value": value.cpu().numpy()}
    written = np.zeros(total + pad, dtype=bool)
    for s in range(n):
        written[room[s]:room[s] + counts_want[s]] = True
    assert written.sum() == want["offsets"][-1] > 100
    for key in ("t0", "t1", "value"):
        assert ref.same_bits(got[key][written], want[key]), key
        assert (got[key][~written] == 0.25).all(), key
    assert np.array_equal(got["level"][written], want["level"]) and (got["level"][~written] == 77).all()
    assert ref.same_bits(integral.cpu().numpy(), want["integral"])
    assert ref.same_bits(covered.cpu().numpy(), want["covered"])
    # offsets that leave no room: a ray writes what fits its range and nothing else
    for array in (t0, t1, value):
        array.fill_(0.25)
    level.fill_(77)
    tight = torch.from_numpy(np.minimum(want["offsets"], 40)).to(device)
    assert call(offsets=tight, n_segments=40) == 0
    ctx.synchronize()
    assert ref.same_bits(t0.cpu().numpy()[:40], want["t0"][:40])
    assert bool((t0[40:] == 0.25).all()) and bool((level[40:] == 77).all())
    su.close()


# ---- composition -----------------------------------------------------------------------------------

def regridded(case, dense):
    dlo = [lev["domain"][0] for lev in case.levels]
    cut = lambda l, lo, hi: dense[l][lo[2] - dlo[l][2]:hi[2] - dlo[l][2] + 1,
                                     lo[1] - dlo[l][1]:hi[1] - dlo[l][1] + 1,
                                     lo[0] - dlo[l][0]:hi[0] - dlo[l][0] + 1]
    return [{"domain": lev["domain"], "boxes": lev["boxes"],
             "data": [cut(l, *box)[None] for box in lev["boxes"]]}
            for l, lev in enumerate(case.levels)]


def test_api_rays_of_two_stored_fields_a_derived_and_a_gradient_field(ctx, three, tmp_path):
    start, end = three.rays(256)
    out = str(tmp_path / "rays.npz")
    got = api.rays(three.path, start, end, fields=["u", "odd"], output=out)
    want = {name: three.wanted(name, 256) for name in ("u", "odd")}
    geometry = want["u"]
    assert got["n"] == 256 and np.array_equal(got["offsets"], geometry["offsets"])
    assert np.array_equal(got["status"], geometry["status"])
    assert np.array_equal(got["level"], geometry["level"]) and got["level"].dtype == np.int8
    for key, other in (("t_enter", "t_enter"), ("t_leave", "t_leave"), ("t0", "t0"), ("t1", "t1"),
                       ("covered_length", "covered")):
        assert ref.same_bits(got[key], geometry[other]), key
    d = end - start
    with np.errstate(all="ignore"):
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert ref.same_bits(got["length"], length)
    for name in ("u", "odd"):
        assert ref.same_bits(got["fields"][name], want[name]["value"])
        assert ref.same_bits(got["integrals"][name], want[name]["integral"])
    back = ray_rules.load_npz(out)
    assert back["n"] == 256 and list(back["fields"]) == ["u", "odd"]
    assert ref.same_bits(back["fields"]["odd"], got["fields"]["odd"])
    assert back["t0"].tobytes() == got["t0"].tobytes()
    # one ray as two points, the first variable, a level cut
    one = api.rays(three.path, start[0], end[0], min_level=1)
    cut = three.reference("u", 1, -1).rays(start[:1], end[:1],
                                           three.reference("u", 1, -1).default_max_trips())
    assert one["n"] == 1 and list(one["fields"]) == ["u"]
    assert ref.same_bits(one["fields"]["u"], cut["value"]) and ref.same_bits(one["t1"], cut["t1"])
    assert api.rays(three.path, np.zeros((0, 3)), np.zeros((0, 3)))["n"] == 0

    api.add_field("uu", "u * u")
    squared = derive_reference.evaluate_levels("u * u", three.levels, VARIABLES, three.lo, three.hi)
    levels = [{"domain": lev["domain"], "boxes": lev["boxes"], "data": [g[None] for g in grids]}
              for lev, grids in zip(three.levels, squared)]
    api.add_gradient_field("du_dx", "u", "x")
    gradient = ref.gradient_levels(three.levels, three.ratio, three.sizes(), 0, 0)[0]
    got = api.rays(three.path, start, end, fields=["uu", "du_dx"])
    for name, data in (("uu", levels), ("du_dx", regridded(three, gradient))):
        hierarchy = rr.Hierarchy(data, three.ratio, 0, three.sizes(), three.lo)
        other = hierarchy.rays(start, end, hierarchy.default_max_trips())
        assert np.array_equal(got["offsets"], other["offsets"])
        assert ref.same_bits(got["fields"][name], other["value"]), name
        assert ref.same_bits(got["integrals"][name], other["integral"]), name


def test_a_slice_of_a_stored_variable_is_unchanged_around_rays(ctx, three):
    before = api.slice(three.path, 40, 30, "u", axis="y")
    start, end = three.rays(64)
    assert api.rays(three.path, start, end)["n"] == 64
    after = api.slice(three.path, 40, 30, "u", axis="y")
    assert ref.same_bits(before, after)
