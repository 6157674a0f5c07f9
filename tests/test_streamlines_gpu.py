"""Streamlines on the GPU: the kernel of avr_streamlines.hip through avr_scene_streamlines,
api.streamline_scene, api.streamlines and api.sample_points, against the numpy reference on the
plotfile's own level arrays (streamline_reference).  Points, samples, counts and status are equal
by bits; slots past a line's count are NaN.  Cell sizes are powers of two, and every coarse cell
that a finer grid covers holds 1e30: a read of a parent grid past a leaf box's view would show as
a wrong point."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, lines, plotfile

import derive_reference
import gradient_reference as ref
import streamline_reference as sl

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

    def reference(self, names, sample=None, min_level=0, max_level=-1):
        """The reference's hierarchy of three components and a sample, made once."""
        key = (tuple(names), sample, min_level, max_level)
        if key not in self.cache:
            self.cache[key] = sl.Hierarchy(
                self.levels, self.ratio, [VARIABLES.index(n) for n in names], self.sizes(),
                self.lo, min_level, max_level,
                None if sample is None else VARIABLES.index(sample))
        return self.cache[key]

    def seeds(self, n, min_level=0, max_level=-1):
        """n seeds: a lattice point, a NaN seed, seeds outside, an infinite one, points exactly on
        box faces (corners of boxes, which are also coarse-fine interfaces, and face centres), on
        domain faces, then the rest of a 7 x 7 x 6 lattice."""
        lo, hi = np.array(self.lo), np.array(self.hi)
        f = (np.stack(np.meshgrid(np.arange(6), np.arange(7), np.arange(7), indexing="ij"), -1)
             .reshape(-1, 3)[:, ::-1] + 0.37) / np.array([7.0, 7.0, 6.0])
        lattice = lo + f * (hi - lo)
        special = [lattice[0], [math.nan, lattice[1][1], lattice[1][2]], lo - 1.0, hi + 5.0,
                   [lattice[2][0], math.inf, lattice[2][2]], lo, hi,
                   [lo[0], lattice[3][1], lattice[3][2]], [lattice[4][0], hi[1], lattice[4][2]]]
        sizes = self.sizes()
        boxes = self.scene_boxes(min_level, max_level)
        for level, blo, bhi in boxes[::max(1, len(boxes) // 12)]:
            dx = np.array(sizes[level])
            special.append(lo + np.array(blo) * dx)
            special.append(lo + (np.array(bhi) + 1) * dx)
            special.append(lo + (np.array(blo) + np.array([0.0, 0.5, 0.5])) * dx)
            special.append(lo + (np.array(bhi) + np.array([0.5, 1.0, 0.5])) * dx)
        pool = np.concatenate([np.array(special, dtype=np.float64), lattice[5:]])
        assert pool.shape[0] >= n
        return np.ascontiguousarray(pool[:n])


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
    return _write(tmp_path_factory.mktemp("lines") / "three", THREE_DOMAINS, THREE_BOXES,
                  (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2], 71)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    grids = [((0, 0, 0), (130, 4, 2)), ((131, 0, 0), (386, 3, 3)), ((387, 0, 0), (387, 3, 3)),
             ((388, 0, 0), (390, 3, 3)), ((395, 7, 7), (395, 7, 7))]
    return _write(tmp_path_factory.mktemp("lines") / "shapes", [((0, 0, 0), (399, 7, 7))],
                  [grids], (0.0, 0.0, 0.0), (100.0, 2.0, 2.0), [], 72)


@pytest.fixture(scope="module")
def ratio_four(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("lines") / "four",
                  [((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (23, 15, 15))],
                  [[((0, 0, 0), (5, 3, 3))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (3.0, 2.0, 2.0), [4], 73)


@pytest.fixture(scope="module")
def skipped_level(tmp_path_factory):
    """The finest grid covers the low-x half of the middle one: a level-0 leaf lies face to face
    with level-2 cells."""
    return _write(tmp_path_factory.mktemp("lines") / "skipped",
                  [((0, 0, 0), (7, 3, 3)), ((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))],
                  [[((0, 0, 0), (7, 3, 3))], [((4, 2, 2), (11, 5, 5))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2, 2], 74)


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    grids = [((4 * a, 4 * b, 4 * c), (4 * a + 3, 4 * b + 3, 4 * c + 3))
             for c in range(5) for b in range(4) for a in range(4)]
    return _write(tmp_path_factory.mktemp("lines") / "many", [((0, 0, 0), (15, 15, 19))],
                  [grids], (0.0, 0.0, 0.0), (2.0, 2.0, 2.5), [], 75)


def load(ctx, case, name, min_level=0, max_level=-1):
    return plotfile.load_plotfile_geometry(ctx, case.path, name, min_level, max_level, False, True)


def same_lines(got, want, max_steps):
    points, counts, status, samples = got
    n = want["counts"].shape[0]
    print("lines:", n, "points:", int(counts.sum()), "reference:", int(want["counts"].sum()),
          "status:", np.bincount(status, minlength=4).tolist(),
          "reference:", np.bincount(want["status"], minlength=4).tolist())
    assert points.shape == (n, max_steps + 1, 3) and counts.shape == (n,)
    assert status.dtype == np.uint8 and np.array_equal(status, want["status"])
    assert np.array_equal(counts, want["counts"])
    past = np.arange(max_steps + 1)[None, :] >= counts[:, None]
    assert np.isnan(points[past]).all()
    assert ref.same_bits(points, want["points"])          # the reference is NaN past the count too
    if want["samples"] is None:
        assert samples is None
    else:
        assert np.isnan(samples[past]).all() and ref.same_bits(samples, want["samples"])


def check(ctx, case, names, n_seeds, step, direction, max_steps, sample=None, min_level=0,
          max_level=-1):
    loaded = {name: load(ctx, case, name, min_level, max_level)
              for name in set(names) | ({sample} if sample else set())}
    finest = max(b.level for b in loaded[names[0]].all_boxes)
    seeds = case.seeds(n_seeds, min_level, max_level)
    got = api.streamline_scene(ctx, *[loaded[name] for name in names], seeds,
                               case.sizes()[:finest + 1], case.lo, case.ratio[:finest], step,
                               max_steps, direction, loaded[sample] if sample else None)
    want = case.reference(names, sample, min_level, max_level).trace(seeds, step, direction,
                                                                     max_steps)
    same_lines(got, want, max_steps)
    return got, loaded[names[0]]


RANDOM = ("u", "whole", "u")
ODD = ("u", "odd", "whole")


# ---- hierarchy -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_seeds,max_steps,step,direction,sample", [
    (257, 64, 0.5, 1, "whole"), (65, 64, 1.0, -1, None), (64, 1, 0.03125, 1, "u"),
    (63, 0, 0.5, -1, "whole"), (1, 64, 0.03125, 1, None), (65, 64, 0.03125, -1, "odd")])
def test_three_levels_with_fine_boxes_that_touch(ctx, three, n_seeds, max_steps, step, direction,
                                                 sample):
    (points, counts, status, _), scene = check(ctx, three, RANDOM, n_seeds, step, direction,
                                               max_steps, sample)
    assert {b.level for b in scene.local_boxes} == {0, 1, 2}
    if n_seeds >= 63:
        assert counts[1] == 0 and status[1] == 1                     # the NaN seed
        assert (counts[2:5] == 0).all() and (status[2:5] == 1).all()  # outside, infinite
    if n_seeds == 257 and max_steps == 64:
        # lines that cross levels, leave the domain, and run all their steps
        levels = three.reference(RANDOM, sample).locate(points[:, 0][counts > 0])[0]
        assert set(levels.tolist()) == {0, 1, 2}
        assert (status == 0).any() and ((status == 1) & (counts > 1)).any()
        assert (counts == max_steps + 1).sum() == (status == 0).sum()


def test_ratio_four(ctx, ratio_four):
    check(ctx, ratio_four, RANDOM, 257, 0.5, 1, 64, "whole")
    check(ctx, ratio_four, RANDOM, 65, 1.0, -1, 64)


def test_a_coarse_leaf_face_to_face_with_cells_two_levels_finer(ctx, skipped_level):
    check(ctx, skipped_level, RANDOM, 257, 0.5, 1, 64, "u")
    check(ctx, skipped_level, RANDOM, 64, 1.0, -1, 64)


@pytest.mark.parametrize("levels", [(1, -1), (0, 0)])
def test_level_ranges_leave_holes_and_whole_coarse_grids(ctx, three, levels):
    (_, counts, status, _), scene = check(ctx, three, RANDOM, 257, 0.5, 1, 64, "whole", *levels)
    if levels[0] == 1:
        assert {b.level for b in scene.local_boxes} == {1, 2}
        assert ((status == 1) & (counts > 1)).any()                  # into the hole
        assert (counts == 0).sum() > 5                               # seeds in the hole


def test_eighty_boxes(ctx, many):
    _, scene = check(ctx, many, RANDOM, 257, 0.5, 1, 64, "whole")
    assert len(scene.local_boxes) == 80
    check(ctx, many, RANDOM, 65, 1.0, -1, 64)


def test_rows_of_131_and_256_cells_a_thin_box_and_a_lone_cell(ctx, shapes):
    _, scene = check(ctx, shapes, RANDOM, 257, 0.5, 1, 64, "u")
    assert [b.cell_dimensions for b in scene.local_boxes] == [(131, 5, 3), (256, 4, 4), (1, 4, 4),
                                                              (3, 4, 4), (1, 1, 1)]
    # a seed in the lone cell: every corner but its own is absent
    lone = np.array([[(395 + 0.25) * 0.25, (7 + 0.5) * 0.25, (7 + 0.75) * 0.25]])
    u = load(ctx, shapes, "u")
    got = api.streamline_scene(ctx, u, u, u, lone, shapes.sizes(), shapes.lo, [], 0.5, 4, 1, u)
    want = shapes.reference(("u", "u", "u"), "u").trace(lone, 0.5, 1, 4)
    same_lines(got, want, 4)
    assert got[1][0] >= 1


# ---- values --------------------------------------------------------------------------------------

def test_nan_and_infinite_cells_fall_back_to_the_leaf_or_end_the_line(ctx, three):
    (_, counts, status, samples), _ = check(ctx, three, ODD, 257, 0.5, 1, 64, "odd")
    assert (status == 3).any() and (status == 1).any()
    check(ctx, three, ODD, 65, 1.0, -1, 64, "odd")
    check(ctx, three, ODD, 64, 0.03125, 1, 64)


def test_a_repeat_gives_equal_bits(ctx, three):
    scenes = [load(ctx, three, name) for name in ("u", "odd", "whole")]
    seeds = three.seeds(257)
    runs = [api.streamline_scene(ctx, *scenes, seeds, three.sizes(), three.lo, three.ratio, 0.5,
                                 64, 1, scenes[1]) for _ in range(2)]
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    assert ref.same_bits(runs[0][0], runs[1][0]) and ref.same_bits(runs[0][3], runs[1][3])


# ---- the C ABI -------------------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_leave_the_outputs_untouched(ctx, three):
    u = load(ctx, three, "u")
    w = load(ctx, three, "whole")
    coarse = load(ctx, three, "u", 0, 0)
    su = ctx.create_scene(u.local_boxes, u.scalar_transform)
    sw = ctx.create_scene(w.local_boxes, w.scalar_transform)
    other = ctx.create_scene(coarse.local_boxes, coarse.scalar_transform)
    narrow = ctx.create_scene([dataclasses.replace(u.local_boxes[0],
                                                   values=u.local_boxes[0].values[:, :, :-1])]
                              + u.local_boxes[1:], u.scalar_transform)
    relevelled = ctx.create_scene(u.local_boxes[:-1] + [dataclasses.replace(u.local_boxes[-1],
                                                                             level=0)],
                                  u.scalar_transform)
    n, max_steps = 65, 8
    seeds_host = three.seeds(n)
    seeds = torch.from_numpy(seeds_host).to(ctx.device)
    points = torch.full((n, max_steps + 1, 3), 0.5, dtype=torch.float64, device=ctx.device)
    samples = torch.full((n, max_steps + 1), 0.25, dtype=torch.float64, device=ctx.device)
    counts = torch.full((n,), -7, dtype=torch.int32, device=ctx.device)
    status = torch.full((n,), 9, dtype=torch.uint8, device=ctx.device)
    index = np.array([lo for _, lo, _ in three.scene_boxes()], dtype=np.int32)

    def untouched():
        ctx.synchronize()
        return bool((points == 0.5).all()) and bool((samples == 0.25).all()) and \
            bool((counts == -7).all()) and bool((status == 9).all())

    def call(vx=su, vy=sw, vz=su, sample=sw, seeds=seeds, n_seeds=n, step=0.5, direction=1,
             max_steps=max_steps, index=index, ratio=(2, 2), sizes=None, prob_lo=None, n_levels=3,
             points=points, samples=samples, counts=counts, status=status):
        index = np.ascontiguousarray(index, np.int32)
        ratio = np.ascontiguousarray(ratio, np.int32)
        sizes = np.ascontiguousarray(three.sizes() if sizes is None else sizes, np.float64)
        prob_lo = np.ascontiguousarray(three.lo if prob_lo is None else prob_lo, np.float64)
        pointer = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        return _capi.lib().avr_scene_streamlines(
            ctx._handle, vx._handle, vy._handle, vz._handle,
            sample._handle if sample is not None else None, pointer(seeds), n_seeds, step,
            direction, max_steps, index.ctypes.data_as(C.POINTER(C.c_int32)),
            ratio.ctypes.data_as(C.POINTER(C.c_int32)), sizes.ctypes.data_as(C.POINTER(C.c_double)),
            prob_lo.ctypes.data_as(C.POINTER(C.c_double)), n_levels, pointer(points),
            pointer(samples), pointer(counts), pointer(status))

    def message():
        return _capi.lib().avr_last_error().decode()

    inside = u.local_boxes[1].values          # an output array that is an input box's cells
    bad_sizes = np.array(three.sizes())
    bad_sizes[1, 2] = 0.0
    far = index.copy()
    far[0, 0] = 2 ** 30
    wrong = [
        (dict(vy=other), "hold the same number of boxes"),                    # not congruent
        (dict(sample=other), "hold the same number of boxes"),
        (dict(vz=narrow), "the scenes' boxes differ in dims or level"),
        (dict(vy=relevelled), "the scenes' boxes differ in dims or level"),
        (dict(sample=narrow), "the scenes' boxes differ in dims or level"),
        (dict(step=0.0), "step must be finite and lie in (0, 1]"),
        (dict(step=math.nan), "step must be finite and lie in (0, 1]"),
        (dict(step=2.0), "step must be finite and lie in (0, 1]"),
        (dict(direction=0), "direction must be +1 or -1"),
        (dict(sample=None), "samples_dev is given exactly when sample is"),
        (dict(samples=None), "samples_dev is given exactly when sample is"),
        (dict(points=inside), "an output array or the seeds overlap an input box's cells"),
        (dict(seeds=inside), "an output array or the seeds overlap an input box's cells"),
        (dict(max_steps=2 ** 20 + 1, n_seeds=1), "max_steps must not exceed 2^20"),
        (dict(n_seeds=2 ** 32), "n_seeds * (max_steps + 1) must stay below 2^32"),
        (dict(n_levels=2), "a box's level is not below n_levels"),
        (dict(sizes=bad_sizes), "level_cell_size must be finite and positive"),
        (dict(prob_lo=(0.0, math.nan, 0.0)), "prob_lo must be finite"),
        (dict(ratio=(2, 1)), "a level ratio is below 2"),
        (dict(index=far), "a box's index range leaves [-2^30, 2^30)"),
        (dict(counts=None), "null argument"),
    ]
    for arguments, text in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert text in message(), (arguments, message())
        assert untouched(), arguments
    assert call(n_seeds=0) == 0 and untouched()           # no seeds: no launch
    # ... and the call that is in order writes every line, and nothing past a line's count
    assert call() == 0
    ctx.synchronize()
    want = three.reference(("u", "whole", "u"), "whole").trace(seeds_host, 0.5, 1, max_steps)
    got_counts = counts.cpu().numpy().astype(np.int64)
    assert np.array_equal(got_counts, want["counts"])
    assert np.array_equal(status.cpu().numpy(), want["status"])
    past = np.arange(max_steps + 1)[None, :] >= got_counts[:, None]
    got_points, got_samples = points.cpu().numpy(), samples.cpu().numpy()
    assert (got_points[past] == 0.5).all() and (got_samples[past] == 0.25).all()
    assert ref.same_bits(got_points[~past], want["points"][~past])
    assert ref.same_bits(got_samples[~past], want["samples"][~past])
    for scene in (su, sw, other, narrow, relevelled):
        scene.close()


# ---- composition -----------------------------------------------------------------------------------

def derived_levels(case, texts):
    grids = [derive_reference.evaluate_levels(text, case.levels, VARIABLES, case.lo, case.hi)
             for text in texts]
    return [{"domain": lev["domain"], "boxes": lev["boxes"],
             "data": [np.stack([g[l][b] for g in grids]) for b in range(len(lev["boxes"]))]}
            for l, lev in enumerate(case.levels)]


SMOOTH = {"swirl_x": "0.0 - (y + 0.25)", "swirl_y": "x - 0.75", "lift": "0.0625 * (z - 1.5)",
          "radius": "sqrt((x - 0.75)**2 + (y + 0.25)**2)", "zero": "0.0 * u"}


def test_smooth_derived_fields_as_components_and_as_the_sample(ctx, three, tmp_path):
    for name, text in SMOOTH.items():
        api.add_field(name, text)
    names = list(SMOOTH)
    levels = derived_levels(three, [SMOOTH[name] for name in names])
    seeds = three.seeds(65)
    hierarchy = sl.Hierarchy(levels, three.ratio, (0, 1, 2), three.sizes(), three.lo, sample=3)
    ahead = hierarchy.trace(seeds, 0.5, 1, 64)
    back = hierarchy.trace(seeds, 0.5, -1, 64)
    out = str(tmp_path / "swirl.vtk")
    got = api.streamlines(three.path, ("swirl_x", "swirl_y", "lift"), seeds, step=0.5,
                          max_steps=64, direction="both", fields=["radius"], output=out)
    assert got["n"] == 65 and got["status"].shape == (65, 2)
    assert np.array_equal(got["status"][:, 0], back["status"])
    assert np.array_equal(got["status"][:, 1], ahead["status"])
    want = lines.join_both(lines.split_lines(back["points"], back["counts"]),
                           lines.split_lines(ahead["points"], ahead["counts"]))
    want_radius = lines.join_both(
        [back["samples"][i, :c] for i, c in enumerate(back["counts"])],
        [ahead["samples"][i, :c] for i, c in enumerate(ahead["counts"])])
    assert max(line.shape[0] for line in want) > 64
    for line, radius, w, wr in zip(got["lines"], got["samples"]["radius"], want, want_radius):
        assert ref.same_bits(line, w) and ref.same_bits(radius, wr)
    assert ref.same_bits(got["length"], lines.line_lengths(want))
    stored, stored_samples = lines.load_vtk_lines(out)
    assert all(ref.same_bits(a, b) for a, b in zip(stored, want)) and list(stored_samples) == ["radius"]
    # a field of zeros is stagnant at every seed that has a leaf
    still = api.streamlines(three.path, ("zero", "zero", "zero"), seeds, max_steps=4)
    zero = sl.Hierarchy(levels, three.ratio, (4, 4, 4), three.sizes(), three.lo).trace(seeds, 0.5, 1, 4)
    assert np.array_equal(still["status"], zero["status"]) and (zero["status"] == 2).sum() > 40
    assert [line.shape[0] for line in still["lines"]] == zero["counts"].tolist()
    assert set(zero["counts"].tolist()) == {0, 1}


def test_api_streamlines_and_sample_points_on_stored_variables(ctx, three):
    seeds = three.seeds(64)
    got = api.streamlines(three.path, ODD, seeds, step=1.0, max_steps=16, direction="backward",
                          fields=["whole", "odd"], min_level=1)
    for sample in ("whole", "odd"):
        want = three.reference(ODD, sample, 1, -1).trace(seeds, 1.0, -1, 16)
        assert np.array_equal(got["status"], want["status"])
        for i, (line, values) in enumerate(zip(got["lines"], got["samples"][sample])):
            c = want["counts"][i]
            assert ref.same_bits(line, want["points"][i, :c])
            assert ref.same_bits(values, want["samples"][i, :c])
    assert api.streamlines(three.path, RANDOM, np.zeros((0, 3)))["n"] == 0
    values, inside = api.sample_points(three.path, seeds, ["u", "odd"])
    for name in ("u", "odd"):
        want, want_inside = sl.sample_points(three.levels, three.ratio, VARIABLES.index(name),
                                             three.sizes(), three.lo, seeds)
        assert np.array_equal(inside, want_inside) and ref.same_bits(values[name], want)
    assert inside.sum() > 40 and not inside[1:5].any()


def test_a_slice_of_a_stored_variable_is_unchanged_around_streamlines(ctx, three):
    before = api.slice(three.path, 40, 30, "u", axis="y")
    assert api.streamlines(three.path, RANDOM, three.seeds(64), max_steps=8)["n"] == 64
    after = api.slice(three.path, 40, 30, "u", axis="y")
    assert ref.same_bits(before, after)
