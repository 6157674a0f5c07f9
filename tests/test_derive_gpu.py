"""Derived fields on the GPU: derive_kernel through avr_scene_derive, api.derive_scene and the
registry against the eval reference on the plotfile's own level arrays (derive_reference).
Equality is by bits, NaN equal to NaN, with no tolerance anywhere: every operation is correctly
rounded and the order is fixed, so any difference is a bug.  Every geometry keeps its cell sizes
and world_scale powers of two, so the kernel's centres (origin + (i + 0.5) dx per box) and the
reference's (prob_lo + (I + 0.5) dx per level) are both exact and equal (asserted below)."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, derive, plotfile
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform

import derive_reference as ref
from helpers import spawn_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIABLES = list(ref.VARIABLES)
TWINS = {"ke_stored": ref.TEXTS["kinetic_energy"], "radius_stored": ref.TEXTS["radius"],
         "clamp_stored": ref.TEXTS["clamp"]}


@pytest.fixture(autouse=True)
def _empty_registry():
    for name in list(api.derived_fields()):
        api.remove_field(name)
    yield
    for name in list(api.derived_fields()):
        api.remove_field(name)


def _integers(rng, box):
    """[6, nz, ny, nx]: integers in [-1000, 1000]; about 2 % of density and of other NaN / +Inf /
    -Inf; pressure positive."""
    lo, hi = box
    shape = (len(VARIABLES), hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
    data = rng.integers(-1000, 1001, size=shape).astype(np.float64)
    data[4] = np.abs(data[4]) + 1.0
    for comp in (0, 5):
        flat = data[comp].reshape(-1)
        odd = rng.choice(flat.size, min(max(flat.size // 50, 3), flat.size), replace=False)
        flat[odd] = np.array([np.nan, np.inf, -np.inf])[np.arange(odd.size) % 3]
    return data


@dataclasses.dataclass
class Case:
    path: str
    levels: list
    lo: tuple
    hi: tuple
    variables: list

    def sizes(self):
        return ref.cell_sizes(self.levels, self.lo, self.hi)

    def dense(self, text):
        """Per level the reference over the level's domain, NaN where no grid is."""
        out = []
        grids = ref.evaluate_levels(text, self.levels, VARIABLES, self.lo, self.hi)
        for lev, values in zip(self.levels, grids):
            dlo, dhi = lev["domain"]
            full = np.full(tuple(dhi[a] - dlo[a] + 1 for a in (2, 1, 0)), np.nan)
            for (lo, hi), v in zip(lev["boxes"], values):
                full[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = v
            out.append(full)
        return out


def _write(path, boxes, domains, lo, hi, seed, twins=False):
    rng = np.random.default_rng(seed)
    levels = [{"domain": d, "boxes": b, "data": [_integers(rng, box) for box in b]}
              for d, b in zip(domains, boxes)]
    case = Case(str(path), levels, lo, hi, list(VARIABLES))
    for size in case.sizes():
        assert all(ref.is_power_of_two(s) for s in size)
    written = levels
    if twins:
        extra = [ref.evaluate_levels(text, levels, VARIABLES, lo, hi) for text in TWINS.values()]
        written = [{"domain": lev["domain"], "boxes": lev["boxes"],
                    "data": [np.concatenate([data] + [e[l][g][None] for e in extra])
                             for g, data in enumerate(lev["data"])]}
                   for l, lev in enumerate(levels)]
        case.variables = VARIABLES + list(TWINS)
    plotfile.write_plotfile(str(path), case.variables, written, lo, hi, [2] * (len(levels) - 1))
    return case


THREE_BOXES = [
    [((0, 0, 0), (6, 9, 7)), ((7, 0, 0), (11, 9, 7))],
    [((4, 4, 2), (13, 11, 9)), ((14, 6, 4), (19, 15, 11))],
    [((12, 10, 6), (23, 19, 13)), ((30, 14, 10), (37, 25, 19))],
]
THREE_DOMAINS = [((0, 0, 0), (11, 9, 7)), ((0, 0, 0), (23, 19, 15)), ((0, 0, 0), (47, 39, 31))]
THREE_LO, THREE_HI = (0.0, -1.0, 2.0), (1.5, 0.25, 3.0)        # coarse cells of 1/8


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    """The slice tests' three_levels (non-cubic, grids 7 and 5 cells wide) with the stored twins of
    three expressions as extra variables."""
    return _write(tmp_path_factory.mktemp("derive") / "three", THREE_BOXES, THREE_DOMAINS, THREE_LO,
                  THREE_HI, 2026, twins=True)


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    fine = [((8 * a + 2, 8 * b + 2, 8 * c + 2), (8 * a + 5, 8 * b + 5, 8 * c + 5))
            for c in range(4) for b in range(4) for a in range(4)]
    return _write(tmp_path_factory.mktemp("derive") / "many", [[((0, 0, 0), (15, 15, 15))], fine],
                  [((0, 0, 0), (15, 15, 15)), ((0, 0, 0), (31, 31, 31))],
                  (0.0, -1.0, 2.0), (1.0, 0.0, 3.0), 78)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """One level, three grids: 131 x 5 x 3 (a second 128-cell segment with an odd tail, odd
    strides), 256 x 4 x 4 (even and aligned: the pair path) and 1 x 1 x 1."""
    grids = [((0, 0, 0), (130, 4, 2)), ((0, 0, 4), (255, 3, 7)), ((200, 7, 0), (200, 7, 0))]
    return _write(tmp_path_factory.mktemp("derive") / "shapes", [grids],
                  [((0, 0, 0), (255, 7, 7))], (0.0, -1.0, 2.0), (4.0, 0.0, 4.0), 5)


@pytest.fixture(scope="module")
def holes(tmp_path_factory):
    """Two levels whose fine boxes span 16 x 20 x 16 fine cells of 1/32: loaded with min_level=1
    the shortest edge is 1/2, so world_scale is 2 -- a power of two other than 1."""
    fine = [((8, 8, 8), (23, 23, 15)), ((8, 8, 16), (23, 27, 23))]
    return _write(tmp_path_factory.mktemp("derive") / "holes", [[((0, 0, 0), (15, 15, 15))], fine],
                  [((0, 0, 0), (15, 15, 15)), ((0, 0, 0), (31, 31, 31))],
                  (0.0, -1.0, 2.0), (1.0, 0.0, 3.0), 79)


def load(ctx, case, name, min_level=0, max_level=-1, **kw):
    return plotfile.load_plotfile_geometry(ctx, case.path, name, min_level, max_level, False, True,
                                           **kw)


def derive_text(ctx, case, text, min_level=0, max_level=-1, select=None):
    program = api.compile_expression(text)
    scenes = [load(ctx, case, name, min_level, max_level) for name in program.fields]
    geometry = scenes[0] if scenes else load(ctx, case, "", min_level, max_level)
    if select is not None:
        scenes = [dataclasses.replace(s, local_boxes=select(s.local_boxes)) for s in scenes]
        geometry = dataclasses.replace(geometry, local_boxes=select(geometry.local_boxes))
    assert ref.is_power_of_two(geometry.world_scale)
    finest = max(b.level for b in geometry.all_boxes)
    out = api.derive_scene(ctx, program, scenes, geometry, case.sizes()[:finest + 1])
    ctx.synchronize()
    return out, scenes


def box_cells(case, scene, box, dense):
    """The reference's cells of a scene box, cut from the level's dense array."""
    size = case.sizes()[box.level]
    nx, ny, nz = box.cell_dimensions
    lo = [(box.min_corner[a] / scene.world_scale - case.lo[a]) / size[a] for a in range(3)]
    assert all(v == round(v) for v in lo)
    i, j, k = (int(v) for v in lo)
    return dense[box.level][k:k + nz, j:j + ny, i:i + nx]


def pair_path(scene, inputs):
    """Per local box whether the kernel reads and writes it as f64 pairs: the host's rule, every
    input and the output 16-byte aligned with even strides."""
    even = lambda b: (b.values.data_ptr() % 16 == 0 and b.values.stride(1) % 2 == 0 and
                      b.values.stride(0) % 2 == 0)
    return [all(even(s.local_boxes[i]) for s in [scene] + list(inputs))
            for i in range(len(scene.local_boxes))]


def check(ctx, case, text, min_level=0, max_level=-1):
    scene, inputs = derive_text(ctx, case, text, min_level, max_level)
    dense = case.dense(text)
    assert len(scene.local_boxes) == len(scene.all_boxes) > 0
    for box in scene.local_boxes:
        want = box_cells(case, scene, box, dense)
        got = box.values.cpu().numpy()
        assert box.values.is_contiguous() and box.values.data_ptr() % 16 == 0
        assert ref.same_bits(got, want), (text, box.level, box.cell_dimensions)
    return scene, inputs


# ---- the kernel against the reference --------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ref.TEXTS))
def test_every_text_equals_the_reference_on_three_levels(ctx, three, name):
    scene, inputs = check(ctx, three, ref.TEXTS[name])
    # odd-strided views into the parent grids and odd-width outputs: the 8-byte path
    assert not all(pair_path(scene, inputs))
    values = np.concatenate([b.values.cpu().numpy().ravel() for b in scene.local_boxes])
    finite = values[np.isfinite(values)]
    assert scene.scalar_range is not None and finite.size > 0
    if name == "full":
        program = api.compile_expression(ref.TEXTS[name])
        assert (len(program.fields), len(program.instructions), len(program.constants)) == (6, 64, 16)
    if name == "denormal":
        assert set(np.unique(finite)) == {5e-324, 1e-323}
    if name == "constant":
        assert (values == 1.0).all()


def test_segments_tails_pairs_and_a_single_cell(ctx, shapes):
    for name in ("kinetic_energy", "radius", "geometry", "full", "compare"):
        scene, inputs = check(ctx, shapes, ref.TEXTS[name])
        dims = [b.cell_dimensions for b in scene.local_boxes]
        assert sorted(dims) == [(1, 1, 1), (131, 5, 3), (256, 4, 4)]
        paired = dict(zip(dims, pair_path(scene, inputs)))       # over every input and the output
        assert paired[(256, 4, 4)] and not paired[(131, 5, 3)]   # both paths occurred


def test_the_pair_path_on_rows_of_odd_width(ctx):
    """Even-strided, aligned views of a box 131 cells wide: the pair path, whose last cell of every
    row is read and written alone.  Reachable through the C ABI only (api.derive_scene's output of
    an odd width has odd strides); the padding column must keep its sentinel."""
    nx, ny, nz, sentinel = 131, 5, 3, -7.0
    rng = np.random.default_rng(3)
    host = [rng.integers(-1000, 1001, size=(nz, ny, nx + 1)).astype(np.float64) for _ in range(2)]
    host[0][1, 2, 130] = np.nan
    padded = [torch.from_numpy(h).to(ctx.device) for h in host]
    padded.append(torch.full((nz, ny, nx + 1), sentinel, dtype=torch.float64, device=ctx.device))
    corner = ((0.25, 0.0, 0.0), (0.25 + nx * 0.125, ny * 0.125, nz * 0.125))
    boxes = [AmrBox(corner[0], corner[1], t[:, :, :nx], 0) for t in padded]
    for b in boxes:
        assert b.values.data_ptr() % 16 == 0 and b.values.stride(1) % 2 == 0 and \
            b.values.stride(0) % 2 == 0 and b.cell_dimensions == (nx, ny, nz)
    scenes = [ctx.create_scene([b], ScalarTransform()) for b in boxes]
    text = "field('a') * field('b') + x"
    program = api.compile_expression(text)
    scenes[2].derive(scenes[:2], program.instructions, program.constants, [corner[0]],
                     [(0.125, 0.125, 0.125)])
    ctx.synchronize()
    got = padded[2].cpu().numpy()
    x = 0.25 + (np.arange(nx, dtype=np.float64) + 0.5) * 0.125
    want = ref.evaluate(text, {"a": host[0][:, :, :nx], "b": host[1][:, :, :nx]},
                        {"x": x[None, None, :]}, (nz, ny, nx))
    assert ref.same_bits(got[:, :, :nx], want) and np.isnan(want[1, 2, 130])
    assert (got[:, :, nx] == sentinel).all()


def test_more_than_sixty_four_boxes(ctx, many):
    scene, _ = check(ctx, many, ref.TEXTS["mach"])
    assert len(scene.local_boxes) > 64
    check(ctx, many, ref.TEXTS["radius"])


def test_min_level_and_max_level(ctx, three, holes):
    scene, _ = check(ctx, holes, ref.TEXTS["kinetic_energy"], min_level=1)
    assert {b.level for b in scene.local_boxes} == {1} and scene.world_scale == 2.0
    scene, _ = check(ctx, holes, ref.TEXTS["radius"], min_level=1)
    scene, _ = check(ctx, holes, ref.TEXTS["geometry"], min_level=1)
    assert {b.level for b in scene.local_boxes} == {1} and len(scene.local_boxes) == 2
    scene, _ = check(ctx, three, ref.TEXTS["geometry"], max_level=0)
    assert {b.level for b in scene.local_boxes} == {0}
    check(ctx, three, ref.TEXTS["kinetic_energy"], max_level=0)


@pytest.mark.parametrize("owners", [2, 3])
def test_owners_derive_the_same_cells_as_one_owner(ctx, three, owners):
    text = ref.TEXTS["mach"]
    whole, _ = derive_text(ctx, three, text)
    for owner in range(owners):
        part, _ = derive_text(ctx, three, text, select=lambda boxes, o=owner: boxes[o::owners])
        assert len(part.local_boxes) == len(whole.local_boxes[owner::owners]) > 0
        for got, want in zip(part.local_boxes, whole.local_boxes[owner::owners]):
            assert got.min_corner == want.min_corner
            assert ref.same_bits(got.values.cpu().numpy(), want.values.cpu().numpy())


# ---- the C ABI's checks ----------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_the_output_untouched(ctx, three):
    f = load(ctx, three, "density")
    g = load(ctx, three, "u")
    coarse = load(ctx, three, "u", 0, 0)
    sf = ctx.create_scene(f.local_boxes, f.scalar_transform)
    sg = ctx.create_scene(g.local_boxes, g.scalar_transform)
    other = ctx.create_scene(coarse.local_boxes, coarse.scalar_transform)
    # the same number of boxes, but one box narrower / on another level
    narrow = ctx.create_scene([dataclasses.replace(g.local_boxes[0],
                                                   values=g.local_boxes[0].values[:, :, :-1])]
                              + g.local_boxes[1:], g.scalar_transform)
    relevelled = ctx.create_scene(g.local_boxes[:-1] + [dataclasses.replace(g.local_boxes[-1],
                                                                             level=0)],
                                  g.scalar_transform)
    assert len(narrow.boxes) == len(relevelled.boxes) == len(sf.boxes) and g.local_boxes[-1].level
    sentinel = 0.5
    outs = [AmrBox(b.min_corner, b.max_corner,
                   torch.full(b.values.shape, sentinel, dtype=torch.float64, device=ctx.device),
                   b.level) for b in f.local_boxes]
    out = ctx.create_scene(outs, ScalarTransform())
    origin = np.zeros((len(outs), 3))
    sizes = np.array(three.sizes())
    word = lambda op, operand=0: op | (operand << 8)
    good_code = [word(derive.OP_FIELD, 0), word(derive.OP_FIELD, 1), word(derive.OP_ADD)]

    def untouched():
        ctx.synchronize()
        return all(bool((b.values == sentinel).all()) for b in outs)

    def call(inputs=(sf, sg), code=good_code, constants=(1.0,), origin=origin, sizes=sizes,
             n_inputs=None, n_code=None, n_constants=None, n_levels=None, target=out):
        handles = (C.c_void_p * 8)(*[s._handle.value for s in inputs])
        code = np.ascontiguousarray(code, np.uint32)
        constants = np.ascontiguousarray(constants, np.float64)
        origin = np.ascontiguousarray(origin, np.float64)
        sizes = np.ascontiguousarray(sizes, np.float64)
        doubles = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        return _capi.lib().avr_scene_derive(
            ctx._handle, handles, len(inputs) if n_inputs is None else n_inputs, target._handle,
            code.ctypes.data_as(C.POINTER(C.c_uint32)), code.size if n_code is None else n_code,
            doubles(constants), constants.size if n_constants is None else n_constants,
            doubles(origin), doubles(sizes), sizes.shape[0] if n_levels is None else n_levels)

    push = word(derive.OP_FIELD, 0)
    deep = [push] * 9 + [word(derive.OP_ADD)] * 8
    bad_origin = origin.copy()
    bad_origin[1, 2] = np.nan
    bad_sizes = sizes.copy()
    bad_sizes[0, 0] = np.inf
    wrong = [
        dict(n_inputs=7), dict(n_inputs=-1), dict(n_code=65, code=[push] * 65), dict(n_code=0),
        dict(n_constants=17, constants=[1.0] * 17),
        dict(code=[word(20)]), dict(code=[word(255)]),                        # unknown opcodes
        dict(code=[word(derive.OP_FIELD, 2)]), dict(code=[word(derive.OP_CONST, 1)]),
        dict(code=[word(derive.OP_BUILTIN, 8)]),
        dict(code=[push, word(derive.OP_ADD)]), dict(code=[word(derive.OP_NEG)]),   # underflow
        dict(code=[push, push, word(derive.OP_WHERE)]),
        dict(code=deep),                                                      # depth 9
        dict(code=[push, push]),                                              # two values left
        dict(inputs=(sf, other)),                                             # another box list
        dict(inputs=(sf, narrow)), dict(inputs=(sf, relevelled)),             # ... of the same length
        dict(n_levels=2), dict(n_levels=17, sizes=np.ones((17, 3))),
        dict(origin=bad_origin), dict(sizes=bad_sizes),
        dict(inputs=(sf, out)),                                               # reads what it writes
    ]
    for arguments in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert untouched(), arguments
    with pytest.raises(ValueError, match="same number of boxes"):
        out.derive([sf, other], good_code, [], origin, sizes)
    assert untouched()
    # ... and the call that is in order overwrites the cells; depth 8 is in order too
    assert call(code=[push] * 8 + [word(derive.OP_ADD)] * 7) == 0
    assert call() == 0
    ctx.synchronize()
    for o, a, b in zip(outs, f.local_boxes, g.local_boxes):
        with np.errstate(invalid="ignore"):
            want = a.values.cpu().numpy() + b.values.cpu().numpy()
        assert ref.same_bits(o.values.cpu().numpy(), want)


# ---- derived equals stored -------------------------------------------------------------------------

def _register_twins():
    api.add_field("ke", TWINS["ke_stored"])
    api.add_field("radius", TWINS["radius_stored"])
    api.add_field("clamp", TWINS["clamp_stored"])


def same(a, b):
    if isinstance(a, dict):
        return all(same(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return ref.same_bits(a, b)
    return bool(np.array_equal(a, b))


def test_slices_projections_and_histograms_of_a_derived_field_equal_its_stored_twin(three):
    _register_twins()
    ctx = api._runtime_scope()[0]
    path = three.path
    for name in ("ke", "radius", "clamp"):
        derived = api.slice_scene(ctx, api._load_variable_scenes(
            ctx, path, [name], 0, -1, False, True, 0, 1, None)[0],
            api.SlicePlane((0.7, -0.4, 2.45), (0.2, 0.3, 1.0), (0.0, 1.0, 0.0), (1.4, 1.2)), 61, 47)
        stored = api.slice_scene(ctx, load(ctx, three, name + "_stored"),
            api.SlicePlane((0.7, -0.4, 2.45), (0.2, 0.3, 1.0), (0.0, 1.0, 0.0), (1.4, 1.2)), 61, 47)
        for got, want in zip(derived, stored):
            assert same(got.cpu().numpy(), want.cpu().numpy())
        assert (stored[1].cpu().numpy() >= 0).sum() > 1000
        assert same(api.slice(path, 40, 30, name, axis="y"),
                    api.slice(path, 40, 30, name + "_stored", axis="y"))
        assert same(api.compute_histogram(path, name, bins=32),
                    api.compute_histogram(path, name + "_stored", bins=32))
        assert same(api.project(path, 48, 32, name), api.project(path, 48, 32, name + "_stored"))
    weighted = api.project_axis(path, "z", "u", "clamp", 53, 41, quantity="mean")
    assert same(weighted, api.project_axis(path, "z", "u", "clamp_stored", 53, 41, quantity="mean"))
    assert np.isfinite(weighted).sum() > 1000
    assert same(api.project_axis(path, "x", "ke", None, 33, 29),
                api.project_axis(path, "x", "ke_stored", None, 33, 29))


def test_phase_and_profile_of_derived_fields_equal_their_stored_twins(three):
    _register_twins()
    path = three.path
    # the summed field is integer valued (clamp: integers in [1, 100] and -|other|), so the sums
    # are exact in any order
    got = api.phase(path, "radius", "ke", "clamp", bins=(16, 12))
    want = api.phase(path, "radius_stored", "ke_stored", "clamp_stored", bins=(16, 12))
    assert same(got, want) and got["cells"].sum() > 1000 and got["nonfinite"] > 0
    got = api.phase(path, "radius", "u", "cells", bins=(16, 12), x_range=(0.2, 0.9))
    want = api.phase(path, "radius_stored", "u", "cells", bins=(16, 12), x_range=(0.2, 0.9))
    assert same(got, want) and got["outside"] > 0
    got = api.profile(path, "radius", "clamp", bins=24)
    assert same(got, api.profile(path, "radius_stored", "clamp_stored", bins=24))


def test_frames_of_a_derived_field_equal_its_stored_twin(three, tmp_path):
    _register_twins()
    ctx = api._runtime_scope()[0]
    for mode in ("max_intensity", "volume"):
        pictures = []
        for name in ("ke", "ke_stored"):
            out = str(tmp_path / f"{mode}_{name}.ppm")
            options = api.RenderOptions(width=96, height=64, output_filename=out, mode=mode)
            assert api.run(three.path, options, name, ctx) == 0
            with open(out, "rb") as fh:
                pictures.append(fh.read())
        assert pictures[0] == pictures[1] and len(set(pictures[0][20:])) > 8
    derived = api._load_variable_scenes(ctx, three.path, ["ke"], 0, -1, False, True, 0, 1, None)[0]
    stored = load(ctx, three, "ke_stored")
    assert derived.scalar_range == stored.scalar_range
    assert derived.processed_scalar_range == stored.processed_scalar_range
    assert derived.scalar_transform == stored.scalar_transform
    logged = api._load_variable_scenes(ctx, three.path, ["ke"], 0, -1, True, True, 0, 1, None)[0]
    assert logged.scalar_transform == plotfile.load_plotfile_geometry(
        ctx, three.path, "ke_stored", 0, -1, True, True).scalar_transform


def test_a_radial_profile_through_the_registry_equals_the_reference(three):
    api.add_field("r", ref.TEXTS["radius"])
    edges = np.linspace(0.0, 1.25, 11)
    got = api.profile(three.path, "r", "u", weight="cells", x_edges=edges)
    radius, u = three.dense(ref.TEXTS["radius"]), three.dense("u")
    ctx = api._runtime_scope()[0]
    scene = load(ctx, three, "u")
    cells = np.zeros(10, dtype=np.int64)
    sums = np.zeros(10)
    for box in scene.local_boxes:
        r = box_cells(three, scene, box, radius).ravel()
        v = box_cells(three, scene, box, u).ravel()
        keep = (r >= edges[0]) & (r <= edges[-1])
        bins = np.minimum(np.searchsorted(edges, r[keep], side="right") - 1, 9)
        cells += np.bincount(bins, minlength=10)
        sums += np.bincount(bins, weights=v[keep], minlength=10)     # integers: exact
    assert np.array_equal(got["cells"], cells) and cells.sum() > 1000 and (cells > 0).sum() > 5
    with np.errstate(invalid="ignore"):
        assert ref.same_bits(got["mean"], sums / cells)
    with pytest.raises(RuntimeError, match="'nothing' .needed by derived field 'bad'. not found"):
        api.add_field("bad", "nothing + 1")
        api.profile(three.path, "bad", "u")


# ---- ranks -----------------------------------------------------------------------------------------

def _rank_worker(rank, world, port, path, out_path, text):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from amrvolumerenderer_amd import api, runtime
        ctx = runtime.Context(0)
        api.add_field("ke", text)
        scene = api._load_variable_scenes(ctx, path, ["ke"], 0, -1, False, True, rank, world,
                                          dist.group.WORLD)[0]
        assert 0 < len(scene.local_boxes) < len(scene.all_boxes)
        cut = api.slice_scene(ctx, scene, api.SlicePlane((0.7, -0.4, 2.45), (0.0, 0.0, 1.0),
                                                         (0.0, 1.0, 0.0), (1.4, 1.2)), 61, 47,
                              rank, world, dist.group.WORLD)
        if rank == 0:
            np.savez(out_path, value=cut[0].cpu().numpy(), level=cut[1].cpu().numpy(),
                     box=cut[2].cpu().numpy(), scalar_range=np.array(scene.scalar_range),
                     processed=np.array(scene.processed_scalar_range))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_give_the_one_rank_range_and_slice(tmp_path, ctx, three):
    out = tmp_path / "ranks.npz"
    spawn_ranks(_rank_worker, 2, lambda port: (2, port, three.path, str(out), TWINS["ke_stored"]))
    got = np.load(out)
    api.add_field("ke", TWINS["ke_stored"])
    scene = api._load_variable_scenes(ctx, three.path, ["ke"], 0, -1, False, True, 0, 1, None)[0]
    cut = api.slice_scene(ctx, scene, api.SlicePlane((0.7, -0.4, 2.45), (0.0, 0.0, 1.0),
                                                     (0.0, 1.0, 0.0), (1.4, 1.2)), 61, 47)
    assert same(got["value"], cut[0].cpu().numpy()) and same(got["level"], cut[1].cpu().numpy())
    assert same(got["box"], cut[2].cpu().numpy())
    assert tuple(got["scalar_range"]) == tuple(scene.scalar_range)
    assert tuple(got["processed"]) == tuple(scene.processed_scalar_range)


# ---- nothing else moves ----------------------------------------------------------------------------

def test_products_of_stored_variables_are_unchanged_around_a_derive(three, tmp_path):
    ctx = api._runtime_scope()[0]

    def products():
        out = str(tmp_path / "frame.ppm")
        assert api.run(three.path, api.RenderOptions(width=96, height=64, output_filename=out),
                       "u", ctx) == 0
        with open(out, "rb") as fh:
            frame = fh.read()
        return (api.slice(three.path, 40, 30, "u", axis="y"),
                api.project_axis(three.path, "z", "u", None, 53, 41), frame,
                api.phase(three.path, "u", "v", "pressure", bins=(16, 12)))

    before = products()
    api.add_field("speed", ref.TEXTS["velocity_magnitude"])
    during = products()                    # registered but unused
    assert np.isfinite(api.slice(three.path, 40, 30, "speed", axis="y")).sum() > 500
    after = products()
    for a, b, c in zip(before, during, after):
        if isinstance(a, bytes):
            assert a == b == c
        else:
            assert same(a, b) and same(a, c)
