"""Joint histograms on the GPU: avr_scene_joint_histogram, Scene.joint_histogram, api.phase_scene,
api.phase and api.profile.

The reference answer is independent float64 numpy on the plotfile's own level arrays
(tests/phase_reference.py), not on the convexified boxes: per loaded level the cells that no grid
of the next finer loaded level covers, then the per-cell rule with numpy.searchsorted.  That pins
convexify, box ownership, the strided views into the parent grids and the kernel together.  Counts
(per level and bin, outside, nonfinite) must match exactly in every case.  Sums must match bit for
bit on the field of small integers, and on the random field within the a-priori bound for
recursive summation in any order, (n - 1) 2^-53 sum |v| plus the rounding of the reference sum
(phase_reference.check_sums; a textbook bound, not a measured tolerance)."""
import os
import sys

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import api, plotfile
from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters

import phase_reference as ref
from helpers import colorize as _colorize
from helpers import read_png as _read_png
from helpers import spawn_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = {name: i for i, name in enumerate(ref.VARIABLES)}

LINEAR = (-300.0, 300.0)      # the fixtures plant cells on edges of these two ranges
LOG = (1e-3, 1e3)


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    levels = ref.three_levels()
    return ref.write(tmp_path_factory.mktemp("phase") / "three", levels), levels


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    levels = ref.many_boxes()
    return ref.write(tmp_path_factory.mktemp("phase") / "many", levels), levels


def load(ctx, path, name, min_level=0, max_level=-1):
    return plotfile.load_plotfile_geometry(ctx, path, name, min_level, max_level, False, True)


def on_edges(levels, comp, edges, min_level=0, max_level=-1):
    """How many uncovered, loaded cells of component comp lie exactly on e[0], an interior edge,
    e[n]."""
    min_level, max_level = ref.clamp(levels, min_level, max_level)
    v = np.concatenate([d[comp][m] for l in range(min_level, max_level + 1)
                        for d, m in zip(levels[l]["data"], ref.uncovered(levels, l, max_level))])
    return (int((v == edges[0]).sum()), int(np.isin(v, edges[1:-1]).sum()),
            int((v == edges[-1]).sum()))


def check(ctx, path, levels, x, y, s, x_edges, y_edges, min_level=0, max_level=-1, exact=None):
    """phase_scene against the reference: counts exactly, sums by check_sums, values by the host
    formula on the returned per-level arrays.  Returns (result, reference)."""
    want = ref.reference(levels, COMP[x], None if y is None else COMP[y],
                         None if s is None else COMP[s], x_edges, y_edges, min_level, max_level)
    scenes = [None if name is None else load(ctx, path, name, min_level, max_level)
              for name in (x, y, s)]
    _, finest = ref.clamp(levels, min_level, max_level)
    vol = ref.volumes(levels)[:finest + 1]
    z = "cell_volume" if s is None else s
    got = api.phase_scene(ctx, scenes[0], scenes[1], x_edges, y_edges, vol, z, scenes[2])
    ny = 1 if y is None else len(y_edges) - 1
    assert got["cells_by_level"].shape == (finest + 1, ny, len(x_edges) - 1)
    assert got["cells_by_level"].dtype == np.int64
    assert np.array_equal(got["cells_by_level"], want["cells"])
    assert got["outside"] == want["outside"] and got["nonfinite"] == want["nonfinite"]
    assert got["cells"].sum() + got["outside"] + got["nonfinite"] == want["uncovered"]
    assert np.array_equal(got["cells"], want["cells"].sum(axis=0))
    assert np.array_equal(got["x_edges"], x_edges)
    assert got["y_edges"] is None if y is None else np.array_equal(got["y_edges"], y_edges)
    if s is None:
        assert got["sums"] is None and got["sums_by_level"] is None
    else:
        worst = ref.check_sums(got["sums_by_level"], want, s == "count" if exact is None else exact)
        print(f"sums[{s}]: largest error / bound = {worst:.3g}")
    # values: the host formula on the returned arrays, bit for bit, for all three kinds
    for kind in ("cell_volume", "cells") + (() if s is None else (s,)):
        values = np.zeros(got["cells"].shape, np.float64)
        for level in range(finest + 1):
            if kind == "cell_volume":
                values = values + vol[level] * got["cells_by_level"][level].astype(np.float64)
            elif kind == "cells":
                values = values + got["cells_by_level"][level].astype(np.float64)
            else:
                values = values + vol[level] * got["sums_by_level"][level]
        formula = api.joint_histogram_values(got["cells_by_level"], got["sums_by_level"], vol, kind)
        assert np.array_equal(formula.view(np.uint64), values.view(np.uint64))
        if kind == z:
            assert np.array_equal(got["values"].view(np.uint64), values.view(np.uint64))
    return got, want


# ---- against the reference ---------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [(1, 1), (7, 5), (128, 128), (1024, 1024)])
@pytest.mark.parametrize("s", [None, "energy", "count"])
def test_linear_by_log_bins_of_every_size(ctx, three, bins, s):
    """1 x 1 and 7 x 5 keep their bins in LDS, 128 x 128 and 1024 x 1024 do not fit the budget and
    take the global path; cells lie exactly on e[0], on interior edges and on e[n] of both axes."""
    path, levels = three
    x_edges = api.bin_edges(*LINEAR, bins[0])
    y_edges = api.bin_edges(*LOG, bins[1], log=True)
    for comp, edges in ((0, x_edges), (1, y_edges)):
        first, interior, last = on_edges(levels, comp, edges)
        assert first >= 1 and last >= 1 and (interior >= 5 or len(edges) == 2)
    got, want = check(ctx, path, levels, "density", "temperature", s, x_edges, y_edges)
    assert {l for l in range(3) if want["cells"][l].sum() > 100} == {0, 1, 2}
    assert want["outside"] > 0 and want["nonfinite"] > 100


@pytest.mark.parametrize("s", [None, "energy", "count"])
def test_explicit_edges_with_cells_on_every_edge(ctx, three, s):
    path, levels = three
    for comp, edges in ((0, ref.X_EDGES), (1, ref.Y_EDGES)):
        first, interior, last = on_edges(levels, comp, edges)
        assert first >= 1 and last >= 1 and interior >= len(edges) - 2
    got, want = check(ctx, path, levels, "density", "temperature", s, ref.X_EDGES, ref.Y_EDGES)
    assert want["outside"] > 100            # the explicit ranges cut both fields
    # the axes the other way round
    check(ctx, path, levels, "temperature", "density", s, ref.Y_EDGES, ref.X_EDGES)


@pytest.mark.parametrize("s", [None, "energy", "count"])
@pytest.mark.parametrize("n", [1, 9, 1024])
def test_one_y_bin(ctx, three, n, s):
    path, levels = three
    check(ctx, path, levels, "density", None, s, api.bin_edges(*LINEAR, n), None)
    check(ctx, path, levels, "temperature", None, s, api.bin_edges(*LOG, n, log=True), None)


def test_a_range_that_excludes_part_of_the_data(ctx, three):
    path, levels = three
    got, want = check(ctx, path, levels, "density", "temperature", "energy",
                      api.bin_edges(-20.0, 60.0, 16), api.bin_edges(0.5, 2.0, 4, log=True))
    assert want["outside"] > want["cells"].sum() > 50


@pytest.mark.parametrize("min_level,max_level", [(1, -1), (0, 0), (1, 1), (0, 1)])
def test_level_ranges(ctx, three, min_level, max_level):
    """min_level = 1 leaves holes (and empty level-0 arrays), max_level = 0 uncovers the coarse
    cells under the refined grids."""
    path, levels = three
    for s in (None, "count", "energy"):
        got, want = check(ctx, path, levels, "density", "temperature", s,
                          api.bin_edges(*LINEAR, 7), api.bin_edges(*LOG, 5, log=True),
                          min_level, max_level)
    lo, hi = ref.clamp(levels, min_level, max_level)
    filled = {l for l in range(hi + 1) if got["cells_by_level"][l].any()}
    assert filled == set(range(lo, hi + 1))
    if max_level == 0:
        assert want["uncovered"] == 12 * 10 * 8


def test_many_boxes(ctx, many):
    path, levels = many
    scene = load(ctx, path, "density")
    assert len(scene.all_boxes) >= 169
    for s in (None, "count", "energy"):
        check(ctx, path, levels, "density", "temperature", s, api.bin_edges(*LINEAR, 128),
              api.bin_edges(*LOG, 5, log=True))
    check(ctx, path, levels, "density", None, "count", ref.X_EDGES, None)


def test_both_read_paths_are_taken(ctx, three, many):
    """Boxes whose rows start on a 16-byte boundary with even strides are read as f64 pairs, the
    others cell by cell: both kinds are in the scenes the tests above bin."""
    for path, _ in (three, many):
        boxes = load(ctx, path, "density").local_boxes
        paired = [b.values.data_ptr() % 16 == 0 and b.values.stride(1) % 2 == 0 and
                  b.values.stride(0) % 2 == 0 for b in boxes]
        assert any(paired) and not all(paired)
    odd_rows = [b for b in load(ctx, three[0], "density").local_boxes if b.values.stride(1) % 2]
    unaligned = [b for b in load(ctx, three[0], "density").local_boxes
                 if b.values.data_ptr() % 16]
    assert odd_rows and unaligned


# ---- the C ABI's checks ----------------------------------------------------------------------------------

def test_incongruent_scenes_are_refused_and_the_outputs_untouched(ctx, three):
    path, _ = three
    x = load(ctx, path, "density")
    y = load(ctx, path, "temperature", 0, 0)          # another box list
    sx = ctx.create_scene(x.local_boxes, x.scalar_transform)
    sy = ctx.create_scene(y.local_boxes, y.scalar_transform)
    same = ctx.create_scene(load(ctx, path, "temperature").local_boxes, x.scalar_transform)
    assert len(sx.boxes) != len(sy.boxes)
    cells = torch.full((3, 5, 7), 7, dtype=torch.int64, device=ctx.device)
    sums = torch.full((3, 5, 7), 0.5, dtype=torch.float64, device=ctx.device)
    totals = torch.full((2,), 9, dtype=torch.int64, device=ctx.device)
    xe, ye = api.bin_edges(*LINEAR, 7), api.bin_edges(*LOG, 5, log=True)

    def untouched():
        ctx.synchronize()
        return bool((cells == 7).all()) and bool((sums == 0.5).all()) and bool((totals == 9).all())

    with pytest.raises(ValueError, match="same number of boxes"):
        sx.joint_histogram(xe, sy, ye, same, 3, cells, sums, totals)
    assert untouched()
    with pytest.raises(ValueError, match="same number of boxes"):
        sx.joint_histogram(xe, same, ye, sy, 3, cells, sums, totals)
    assert untouched()
    # the same number of boxes, other dims: the coarse boxes of a max_level = 0 scene, reversed
    coarse = list(y.local_boxes)
    if len(coarse) > 1 and tuple(coarse[0].values.shape) != tuple(coarse[-1].values.shape):
        swapped = ctx.create_scene(coarse[::-1], y.scalar_transform)
        with pytest.raises(ValueError, match="differ in dims or level"):
            sy.joint_histogram(xe, swapped, ye, None, 3, cells, None, totals)
        assert untouched()
    # levels the arrays do not cover, edges that do not increase, too many bins
    with pytest.raises(ValueError, match="n_levels"):
        sx.joint_histogram(xe, same, ye, None, 2, cells[:2].contiguous(), None, totals)
    bad = xe.copy()
    bad[3] = bad[2]
    with pytest.raises(ValueError, match="strictly increasing"):
        sx.joint_histogram(bad, same, ye, None, 3, cells, None, totals)
    bad[3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        sx.joint_histogram(bad, same, ye, None, 3, cells, None, totals)
    assert untouched()
    # ... and the call that is in order ADDS to what the arrays hold
    sx.joint_histogram(xe, same, ye, same, 3, cells, sums, totals)
    fresh = sx.joint_histogram(xe, same, ye, same)
    ctx.synchronize()
    assert torch.equal(cells, fresh[0] + 7) and torch.equal(totals, fresh[2] + 9)
    assert fresh[0].sum() > 1000


# ---- owners and ranks --------------------------------------------------------------------------------------

@pytest.mark.parametrize("owners", [2, 3])
def test_owners_sum_to_the_one_owner_histogram(ctx, three, owners):
    path, levels = three
    fields = [load(ctx, path, name) for name in ("density", "temperature", "count")]
    xe, ye = api.bin_edges(*LINEAR, 7), api.bin_edges(*LOG, 5, log=True)

    def histogram(select):
        scenes = [ctx.create_scene(select(f.local_boxes), f.scalar_transform) for f in fields]
        out = scenes[0].joint_histogram(xe, scenes[1], ye, scenes[2], 3)
        ctx.synchronize()
        return out

    whole = histogram(lambda boxes: boxes)
    parts = [histogram(lambda boxes, o=owner: boxes[o::owners]) for owner in range(owners)]
    assert all(int(p[0].sum()) > 0 for p in parts)
    cells, sums, totals = api.combine_joint_histograms(parts)
    assert torch.equal(cells, whole[0]) and torch.equal(totals, whole[2])
    assert torch.equal(sums.view(torch.int64), whole[1].view(torch.int64))     # integers: exact
    want = ref.reference(levels, 0, 1, 3, xe, ye)
    assert np.array_equal(cells.cpu().numpy(), want["cells"])
    # accumulating into one set of arrays is the same sum
    scenes = [[ctx.create_scene(f.local_boxes[o::owners], f.scalar_transform) for f in fields]
              for o in range(owners)]
    out = None
    for sx, sy, ss in scenes:
        out = sx.joint_histogram(xe, sy, ye, ss, 3, *(out or (None, None, None)))
    ctx.synchronize()
    assert torch.equal(out[0], whole[0]) and torch.equal(out[2], whole[2])
    assert torch.equal(out[1].view(torch.int64), whole[1].view(torch.int64))


def _phase_worker(rank, world, port, path, out_path, xe, ye, vol):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from amrvolumerenderer_amd import api, plotfile, runtime
        ctx = runtime.Context(0)
        scenes = [plotfile.load_plotfile_geometry(ctx, path, name, 0, -1, False, True, rank, world,
                                                  dist.group.WORLD)
                  for name in ("density", "temperature", "count")]
        assert 0 < len(scenes[0].local_boxes) < len(scenes[0].all_boxes)
        got = api.phase_scene(ctx, scenes[0], scenes[1], xe, ye, vol, "count", scenes[2], rank,
                              world, dist.group.WORLD)
        np.savez(f"{out_path}.{rank}.npz", cells=got["cells_by_level"], sums=got["sums_by_level"],
                 values=got["values"], totals=np.array([got["outside"], got["nonfinite"]]))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_get_the_one_rank_counts(tmp_path, ctx, three):
    """phase_scene's own reduction: every rank bins its boxes, a non-NCCL group stages the
    all-reduce through the host, and every rank holds the whole histogram."""
    path, levels = three
    xe, ye = api.bin_edges(*LINEAR, 7), api.bin_edges(*LOG, 5, log=True)
    vol = ref.volumes(levels)
    out = str(tmp_path / "phase")
    spawn_ranks(_phase_worker, 2, lambda port: (2, port, path, out, xe, ye, vol))
    one, want = check(ctx, path, levels, "density", "temperature", "count", xe, ye)
    for rank in range(2):
        got = np.load(f"{out}.{rank}.npz")
        assert np.array_equal(got["cells"], want["cells"])
        assert got["totals"].tolist() == [want["outside"], want["nonfinite"]]
        assert np.array_equal(got["sums"].view(np.uint64), one["sums_by_level"].view(np.uint64))
        assert np.array_equal(got["values"].view(np.uint64), one["values"].view(np.uint64))


# ---- api.phase and api.profile --------------------------------------------------------------------------------

CMAP = [(0.0, 0.0, 0.0, 0.3, 1.0), (0.5, 0.9, 0.2, 0.1, 1.0), (1.0, 1.0, 1.0, 0.6, 1.0)]


def finite_range(levels, comp, positive=False):
    v = np.concatenate([d[comp][m] for l in range(len(levels))
                        for d, m in zip(levels[l]["data"], ref.uncovered(levels, l, len(levels) - 1))])
    v = v[np.isfinite(v) & ((v > 0.0) | (not positive))]
    return float(v.min()), float(v.max())


def test_api_phase_returns_the_histogram_and_writes_the_picture(three, tmp_path):
    path, levels = three
    vol = ref.volumes(levels)
    table = api.projection_rgb_table(CMAP)

    # default ranges: (min, max) of the finite cells, (min positive, max) with log
    got = api.phase(path, "density", "temperature", bins=(24, 16), y_log=True,
                    output=str(tmp_path / "auto.ppm"))
    xe = ref.linear_edges(*finite_range(levels, 0), 24)
    ye = ref.log_edges(*finite_range(levels, 1, True), 16)
    assert np.array_equal(got["x_edges"], xe) and np.array_equal(got["y_edges"], ye)
    want = ref.reference(levels, 0, 1, None, xe, ye)
    assert np.array_equal(got["cells_by_level"], want["cells"])
    assert got["outside"] == 0 and got["nonfinite"] == want["nonfinite"]
    values = api.joint_histogram_values(want["cells"], None, vol)
    assert np.array_equal(got["values"].view(np.uint64), values.view(np.uint64))
    filled = want["cells"].sum(axis=0) > 0
    assert filled.sum() > 50 and (~filled).sum() > 20
    q = np.where(filled, values, 0.0)
    raw = open(tmp_path / "auto.ppm", "rb").read()
    head = b"P6\n24 16\n255\n"
    assert raw.startswith(head)
    picture = np.frombuffer(raw[len(head):], np.uint8).reshape(16, 24, 3)
    assert np.array_equal(picture, _colorize(q, q[filled].min(), q[filled].max(),
                                             api.projection_rgb_table(None), filled))
    assert not picture[::-1][~filled].any()            # empty bins are black, row 0 at the bottom

    # explicit edges, a summed variable, a fixed range, a colour map, a PNG
    got = api.phase(path, "density", "temperature", z="count", x_edges=ref.X_EDGES,
                    y_edges=ref.Y_EDGES, bins=(3, 3), x_range=(0.0, 1.0), value_range=(-2e4, 3e4),
                    color_map=CMAP, output=str(tmp_path / "fixed.png"))
    want = ref.reference(levels, 0, 1, 3, ref.X_EDGES, ref.Y_EDGES)
    assert np.array_equal(got["cells_by_level"], want["cells"])
    assert ref.check_sums(got["sums_by_level"], want, True) == 0.0
    values = api.joint_histogram_values(got["cells_by_level"], got["sums_by_level"], vol, "count")
    assert np.array_equal(got["values"].view(np.uint64), values.view(np.uint64))
    filled = got["cells"] > 0
    picture = _read_png(tmp_path / "fixed.png")
    assert picture.shape == (len(ref.Y_EDGES) - 1, len(ref.X_EDGES) - 1, 3)
    assert np.array_equal(picture, _colorize(values, -2e4, 3e4, table, filled))
    # ... and the bytes of the picture before the file: colorize of the same arrays on the device
    ctx = api._runtime_scope()[0]
    rgb8, _ = ctx.projection_colorize(torch.from_numpy(values).to(ctx.device),
                                      torch.from_numpy(filled.astype(np.float64)).to(ctx.device),
                                      torch.from_numpy(table).to(ctx.device), "column", False,
                                      (-2e4, 3e4))
    assert np.array_equal(rgb8.cpu().numpy(), picture)

    # min_level / max_level reach the loader
    got = api.phase(path, "density", "temperature", z="cells", x_edges=ref.X_EDGES,
                    y_edges=ref.Y_EDGES, min_level=1, max_level=1)
    want = ref.reference(levels, 0, 1, None, ref.X_EDGES, ref.Y_EDGES, 1, 1)
    assert np.array_equal(got["cells_by_level"], want["cells"])
    assert np.array_equal(got["values"], want["cells"].sum(axis=0).astype(np.float64))


@pytest.mark.parametrize("weight", ["cell_volume", "cells"])
def test_api_profile(three, weight):
    path, levels = three
    vol = ref.volumes(levels)
    for field, exact in (("count", True), ("energy", False)):
        got = api.profile(path, "temperature", field, weight=weight, bins=12, x_log=True)
        xe = ref.log_edges(*finite_range(levels, 1, True), 12)
        assert np.array_equal(got["x_edges"], xe)
        want = ref.reference(levels, 1, None, COMP[field], xe, None)
        assert np.array_equal(got["cells"], want["cells"].sum(axis=0)[0])
        assert got["outside"] == 0 and got["nonfinite"] == want["nonfinite"]
        if exact:
            # integer sums are exact, so the whole profile follows from the reference
            sums = np.array([[float(sum(want["terms"][l].get(b, []))) for b in range(12)]
                             for l in range(3)])
            mean, weight_sum = api.profile_mean(want["cells"][:, 0, :], sums, vol, weight)
            assert np.array_equal(got["mean"].view(np.uint64), mean.view(np.uint64))
            assert np.array_equal(got["weight_sum"].view(np.uint64), weight_sum.view(np.uint64))
    # explicit edges with empty bins: NaN there
    edges = np.array([-4e6, -3e6, -5e5, 0.0, 5e5, 3e6])
    got = api.profile(path, "count", "density", weight=weight, x_edges=edges)
    assert got["cells"][0] == 0 and np.isnan(got["mean"][0]) and got["weight_sum"][0] == 0.0
    assert np.isfinite(got["mean"][1:]).all() and got["outside"] == 0


def test_profile_mean_and_weight_sum_follow_the_returned_arrays(ctx, three):
    path, levels = three
    vol = ref.volumes(levels)
    xe = api.bin_edges(*LINEAR, 9)
    scenes = [load(ctx, path, name) for name in ("density", "energy")]
    got = api.phase_scene(ctx, scenes[0], None, xe, None, vol, "energy", scenes[1])
    for weight in ("cell_volume", "cells"):
        numerator = np.zeros(9)
        denominator = np.zeros(9)
        for level in range(3):
            w = vol[level] if weight == "cell_volume" else 1.0
            numerator = numerator + w * got["sums_by_level"][level, 0]
            denominator = denominator + w * got["cells_by_level"][level, 0].astype(np.float64)
        mean, weight_sum = api.profile_mean(got["cells_by_level"][:, 0], got["sums_by_level"][:, 0],
                                            vol, weight)
        assert np.array_equal(weight_sum.view(np.uint64), denominator.view(np.uint64))
        assert (denominator > 0).all()
        assert np.array_equal(mean.view(np.uint64), (numerator / denominator).view(np.uint64))


def test_histogram_project_and_volume_frames_are_unchanged_around_a_phase(three, tmp_path):
    path, _ = three
    ctx = api._runtime_scope()[0]
    scene = load(ctx, path, "")
    camera = api.automatic_camera(scene.bounds)
    params = RenderParameters(120, 72, 0.85, 1, draw_bounds=False)

    def frames():
        histogram = api.compute_histogram(path, bins=64)
        column = api.project(path, width=96, height=64, output=str(tmp_path / "p.png"))
        picture = _read_png(tmp_path / "p.png")
        renderer = FrameRenderer(ctx, scene.all_boxes, scene.local_boxes, scene.scalar_transform,
                                 scene.bounds, scene.scalar_range)
        image, rgb8 = renderer.render(params, camera, want_image=True)
        renderer.synchronize()
        out = (column, picture, image.cpu().numpy().copy(), rgb8.cpu().numpy().copy(), histogram)
        if renderer.native is not None:
            renderer.native.close()
        return out

    before = frames()
    got = api.phase(path, "density", "temperature", z="energy", bins=(128, 128), y_log=True,
                    output=str(tmp_path / "phase.png"))
    assert got["cells"].sum() > 1000
    profile = api.profile(path, "density", "energy")
    assert profile["cells"].sum() > 1000
    after = frames()
    assert (before[0] != 0).sum() > 500 and before[3].any() and before[4]["samples"] > 1000
    assert np.array_equal(before[0].view(np.uint64), after[0].view(np.uint64))
    assert np.array_equal(before[1], after[1])
    assert np.array_equal(before[2].view(np.uint32), after[2].view(np.uint32))
    assert np.array_equal(before[3], after[3])
    assert np.array_equal(before[4]["counts"], after[4]["counts"])
    assert {k: v for k, v in before[4].items() if k != "counts"} == \
        {k: v for k, v in after[4].items() if k != "counts"}
