"""Clump trees on the GPU: clump_link_kernel through avr_scene_clump_links, api.clump_tree_scene
and api.clump_tree, against the reference on the plotfile's own level arrays
(clump_tree_reference).  Integers are equal; a sum lies within (n - 1) 2^-53 sum |vs| of the
correctly rounded one (plus that one's own rounding), the a-priori bound of n f64 additions in any
order, as test_clumps_gpu.py holds its tables to; edges are equal by bits.  Cell sizes are powers
of two.  The hand-made label scenes are the smallest shapes at which a wave's carried record can
go wrong: 17 tiles (two workgroups), labels that change per plane, at a tile's edge, in the middle
of a row and lane by lane, on both access widths."""
import ctypes as C
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, plotfile
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform

import clump_tree_reference as tr
import gradient_reference as ref

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)
INF = math.inf
U = 2.0 ** -53
I32_MAX, I32_MIN, U32_MAX = 2 ** 31 - 1, -2 ** 31, 2 ** 32 - 1
LADDER = (-0.5, 0.0, 0.5, 1.0, 1.5, 2.5)


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

    def sizes(self):
        return ref.cell_sizes(self.levels, self.lo, self.hi)

    def scene_boxes(self, min_level=0, max_level=-1):
        if max_level < 0:
            max_level = len(self.levels) - 1
        convex = plotfile.convexify([lev["boxes"] for lev in self.levels[:max_level + 1]],
                                    self.ratio[:max_level])
        return [(l, lo, hi) for l in range(min_level, max_level + 1) for _, (lo, hi) in convex[l]]

    @functools.lru_cache(maxsize=None)
    def tree(self, variable, thresholds, upper, fields=(), min_level=0, max_level=-1):
        """The reference, made once per set of arguments and shared."""
        return tr.clump_tree(self.levels, self.ratio, VARIABLES.index(variable), thresholds, upper,
                             self.scene_boxes(min_level, max_level), min_level, max_level,
                             tuple(VARIABLES.index(f) for f in fields))


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
    return _write(tmp_path_factory.mktemp("tree") / "three", THREE_DOMAINS, THREE_BOXES,
                  (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2], 41)


@pytest.fixture(scope="module")
def ratio_four(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("tree") / "four",
                  [((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (23, 15, 15))],
                  [[((0, 0, 0), (5, 3, 3))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (3.0, 2.0, 2.0), [4], 43)


@pytest.fixture(scope="module")
def skipped_level(tmp_path_factory):
    """The finest grid covers the low-x half of the middle one: a level-0 leaf lies face to face
    with level-2 cells; R = 4, 2, 1."""
    return _write(tmp_path_factory.mktemp("tree") / "skipped",
                  [((0, 0, 0), (7, 3, 3)), ((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))],
                  [[((0, 0, 0), (7, 3, 3))], [((4, 2, 2), (11, 5, 5))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2, 2], 44)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    grids = [((0, 0, 0), (130, 4, 2)), ((131, 0, 0), (386, 3, 3)), ((387, 0, 0), (387, 3, 3)),
             ((388, 0, 0), (390, 3, 3)), ((395, 7, 7), (395, 7, 7))]
    return _write(tmp_path_factory.mktemp("tree") / "shapes", [((0, 0, 0), (399, 7, 7))],
                  [grids], (0.0, 0.0, 0.0), (100.0, 2.0, 2.0), [], 42)


def literal_collapse(parent, cells, min_cells):
    """The collapse rule, node by node."""
    n = len(parent)
    valid = [cells[v] >= min_cells for v in range(n)]
    valid_children = [sum(1 for w in range(n) if parent[w] == v and valid[w]) for v in range(n)]
    kept = [valid[v] and (parent[v] == -1 or valid_children[parent[v]] >= 2) for v in range(n)]
    kept_parent = []
    for v in range(n):
        up = parent[v] if kept[v] else -1
        while up >= 0 and not kept[up]:
            up = parent[up]
        kept_parent.append(up)
    leaves = [v for v in range(n) if kept[v] and v not in set(kept_parent)]
    return kept, kept_parent, leaves


def integral_and_bound(case, want, name):
    """The reference's integral of field `name` per node and how far a device integral may lie
    from it: per level the sum's bound, (n - 1) u sum |vs| and the reference's own rounding, scaled
    by the (power of two) volume, and the additions over the levels.  A cell whose value is not
    finite is in neither sum, so the cell count only overstates n."""
    f, n_levels = VARIABLES.index(name), want["n_levels"]
    volumes = api.level_cell_volumes(case.sizes()[:n_levels])
    cells, sums, abs_sums = want["cells_by_level"], want["sums"][f], want["abs_sums"][f]
    integral = sum(np.float64(volumes[l]) * sums[l] for l in range(n_levels))
    bound = sum(volumes[l] * (np.maximum(cells[l] - 1, 0) * U * abs_sums[l] + U * abs(sums[l]))
                for l in range(n_levels)) + \
        n_levels * U * sum(volumes[l] * abs_sums[l] for l in range(n_levels))
    return integral, bound


def check_tree(case, variable, thresholds, upper=INF, fields=(), min_cells=1, min_level=0,
               max_level=-1):
    got = api.clump_tree(case.path, variable, thresholds, upper, fields=list(fields),
                         min_cells=min_cells, min_level=min_level, max_level=max_level)
    want = case.tree(variable, tuple(thresholds), upper, tuple(fields), min_level, max_level)
    n_levels = want["n_levels"]
    n = sum(want["counts"])
    assert got["n"] == n and got["thresholds"].tolist() == list(thresholds) and got["upper"] == upper
    assert np.array_equal(got["node_begin"], want["node_begin"])
    assert np.array_equal(got["parent"], want["parent"])
    assert np.array_equal(np.diff(got["node_begin"]), want["counts"])
    for step, count in enumerate(want["counts"]):
        nodes = slice(got["node_begin"][step], got["node_begin"][step + 1])
        assert (got["threshold_index"][nodes] == step).all()
        assert got["label"][nodes].tolist() == list(range(1, count + 1))
    for v in range(n):
        mine = got["children"][got["child_offsets"][v]:got["child_offsets"][v + 1]].tolist()
        assert mine == np.nonzero(want["parent"] == v)[0].tolist()
    assert np.array_equal(got["index_lo"], want["index_lo"])
    assert np.array_equal(got["index_hi"], want["index_hi"])
    assert got["index_lo"].dtype == got["index_hi"].dtype == np.int64
    assert np.array_equal(got["cells_by_level"], want["cells_by_level"])
    assert np.array_equal(got["cells"], want["cells_by_level"].sum(axis=0))
    # edges: one multiply and one add, equal by bits
    finest = np.array(case.sizes()[n_levels - 1], dtype=np.float64)
    origin = np.array(case.lo, dtype=np.float64)
    assert ref.same_bits(got["left_edge"], origin + want["index_lo"].astype(np.float64) * finest)
    assert ref.same_bits(got["right_edge"],
                         origin + (want["index_hi"] + 1).astype(np.float64) * finest)
    volumes = api.level_cell_volumes(case.sizes()[:n_levels])
    volume = sum(np.float64(volumes[l]) * want["cells_by_level"][l].astype(np.float64)
                 for l in range(n_levels))
    assert ref.same_bits(got["volume"], 0.0 + volume)
    for name in fields:
        integral, bound = integral_and_bound(case, want, name)
        error = np.abs(got["integrals"][name] - integral)
        print(name, "largest integral error / bound:",
              float((error / np.maximum(bound, 1e-300)).max()) if n else 0.0)
        assert (error <= bound).all()
    assert got["nonfinite"] == want["nonfinite"]
    kept, kept_parent, leaves = literal_collapse(want["parent"].tolist(), got["cells"].tolist(),
                                                 min_cells)
    assert got["kept"].tolist() == kept and got["kept_parent"].tolist() == kept_parent
    assert got["leaves"].tolist() == leaves
    return got, want


# ---- hierarchies through api.clump_tree ----------------------------------------------------------

def test_three_levels_six_thresholds(three):
    got, want = check_tree(three, "u", LADDER, fields=("u", "odd"))
    assert want["counts"] == [4, 27, 122, 166, 107, 10]
    children = np.diff(got["child_offsets"])
    assert (children >= 2).any() and (children == 1).any()         # splits and sole children
    assert (children[:got["node_begin"][5]] == 0).any()            # clumps that vanish
    assert not got["kept"].all() and got["kept"].any() and got["nonfinite"] > 0
    # a clump through all three levels: its box is wider than any one level's cells
    assert (got["cells_by_level"] > 0).all(axis=0).any()


def test_min_cells_prunes_siblings(three):
    got, _ = check_tree(three, "u", LADDER, min_cells=3)
    loose, _ = check_tree(three, "u", LADDER)
    assert got["kept"].sum() < loose["kept"].sum() and (got["cells"][got["kept"]] >= 3).all()
    # at 5 cells some kept clumps hang under an ancestor beyond their parent: a chain folded
    more, want = check_tree(three, "u", LADDER, min_cells=5)
    assert (more["kept_parent"][more["kept"]] != want["parent"][more["kept"]]).any()


def test_a_finite_upper_bound(three):
    got, want = check_tree(three, "u", LADDER[:4], upper=1.75)
    assert got["n"] > 50


@pytest.mark.parametrize("levels", [(1, -1), (0, 0)])
def test_level_ranges(three, levels):
    got, want = check_tree(three, "u", LADDER, min_level=levels[0], max_level=levels[1])
    assert want["n_levels"] == (3 if levels[1] < 0 else 1) and got["n"] > 20
    assert got["cells_by_level"].shape[0] == want["n_levels"]


def test_ratio_four(ratio_four):
    got, _ = check_tree(ratio_four, "u", (-0.5, 0.3, 1.0), fields=("whole",))
    coarse = got["cells_by_level"][0] > 0                          # a level-0 cell is 4 wide
    assert coarse.any() and ((got["index_hi"] - got["index_lo"] + 1)[coarse] >= 4).all()


def test_a_coarse_leaf_face_to_face_with_cells_two_levels_finer(skipped_level):
    got, _ = check_tree(skipped_level, "u", (-0.5, 0.2, 0.9))
    spans = (got["cells_by_level"][0] > 0) & (got["cells_by_level"][2] > 0)
    assert spans.any()                                             # R = 4 and R = 1 in one clump
    whole, _ = check_tree(skipped_level, "u", (-1e3,))             # one clump: the whole domain
    assert whole["n"] == 1 and whole["index_lo"].tolist() == [[0, 0, 0]]
    assert whole["index_hi"].tolist() == [[31, 15, 15]]


def test_rows_of_131_and_256_cells_a_thin_box_and_a_lone_cell(shapes):
    got, _ = check_tree(shapes, "u", (-0.5, 0.3, 1.2), fields=("u",))
    whole, _ = check_tree(shapes, "u", (-1e3,))
    assert whole["index_lo"].tolist() == [[0, 0, 0], [395, 7, 7]]
    assert whole["index_hi"].tolist() == [[390, 4, 3], [395, 7, 7]]


def test_no_clump_at_all_and_an_output_file(three, tmp_path):
    got = api.clump_tree(three.path, "u", [50.0, 60.0], fields=["u"])
    assert got["n"] == 0 and got["index_lo"].shape == (0, 3) and got["cells_by_level"].shape == (3, 0)
    assert got["node_begin"].tolist() == [0, 0, 0] and got["integrals"]["u"].shape == (0,)
    out = str(tmp_path / "tree.npz")
    got = api.clump_tree(three.path, "u", LADDER[3:], output=out)
    saved = np.load(out)
    assert np.array_equal(saved["parent"], got["parent"]) and int(saved["n"]) == got["n"] > 100
    assert np.array_equal(saved["left_edge"], got["left_edge"])


# ---- avr_scene_clump_links on hand-made label scenes -------------------------------------------------

def label_scene(ctx, boxes, aligned=True):
    """A scene over boxes of hand-made cells: (cells [nz, ny, nx], level).  Not aligned: every box
    starts 8 bytes off a 16-byte boundary, so the kernel reads single cells."""
    made = []
    for cells, level in boxes:
        flat = torch.empty(cells.size + 3, dtype=torch.float64, device=ctx.device)
        offset = (flat.data_ptr() // 8 + (0 if aligned else 1)) % 2
        view = flat[offset:offset + cells.size].view(cells.shape)
        view.copy_(torch.from_numpy(np.ascontiguousarray(cells, dtype=np.float64)))
        assert view.data_ptr() % 16 == (0 if aligned else 8)
        nz, ny, nx = cells.shape
        made.append(AmrBox((0.0, 0.0, 0.0), (float(nx), float(ny), float(nz)), view, level))
    return ctx.create_scene(made, ScalarTransform())


def links_by_hand(boxes, parents, n, n_parents, index_lo, scales, start=None):
    """The rules of avr_scene_clump_links, cell by cell in numpy: (extent [6, n], parent_lo,
    parent_hi, totals)."""
    extent = np.empty((6, n), dtype=np.int64)
    extent[:3], extent[3:] = I32_MAX, I32_MIN
    low = np.full(n, U32_MAX, dtype=np.int64)
    high = np.zeros(n, dtype=np.int64)
    if start is not None:
        extent, low, high = (np.array(v, dtype=np.int64) for v in start)
    totals = [0, 0]
    for b, (cells, _) in enumerate(boxes):
        k, j, i = np.indices(cells.shape)
        active = cells.view(np.int64) != 0                              # not +0.0
        with np.errstate(invalid="ignore"):
            integer = (cells >= 1.0) & (cells <= n) & (cells == np.floor(cells))
            totals[0] += int((active & ~integer).sum())
            counted = active & integer
            if parents is not None:
                under = parents[b][0]
                linked = (under >= 1.0) & (under <= n_parents) & (under == np.floor(under))
                totals[1] += int((counted & ~linked).sum())
                counted &= linked
        for c in np.unique(cells[counted]).astype(np.int64):
            mine = counted & (cells == c)
            for axis, position in enumerate((i, j, k)):
                ends = (index_lo[b][axis] + position[mine]) * scales[b]
                extent[axis, c - 1] = min(extent[axis, c - 1], ends.min())
                extent[3 + axis, c - 1] = max(extent[3 + axis, c - 1], ends.max() + scales[b] - 1)
            if parents is not None:
                low[c - 1] = min(low[c - 1], int(parents[b][0][mine].min()))
                high[c - 1] = max(high[c - 1], int(parents[b][0][mine].max()))
    return extent, low, high, totals


def run_links(ctx, boxes, parents, n, n_parents, index_lo, ratios, aligned=True, **outputs):
    labels = label_scene(ctx, boxes, aligned)
    under = label_scene(ctx, parents, aligned) if parents is not None else None
    got = labels.clump_links(n, np.array(index_lo, dtype=np.int32), ratios, under, n_parents,
                             **outputs)
    ctx.synchronize()
    labels.close()
    if under is not None:
        under.close()
    extent, low, high, totals = got
    return (extent.cpu().numpy().astype(np.int64),
            None if low is None else low.cpu().numpy().astype(np.int64),
            None if high is None else high.cpu().numpy().astype(np.int64),
            totals.cpu().numpy().tolist())


def assert_links(got, want, has_parents=True):
    assert np.array_equal(got[0], want[0])
    if has_parents:
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    else:
        assert got[1] is None and got[2] is None
    assert got[3] == want[3]


SHAPE = (68, 4, 128)        # 17 tiles of 4 planes: two workgroups, the second with one tile


def carried_patterns():
    k, j, i = np.indices(SHAPE)
    return {
        "one label": np.full(SHAPE, 2.0),                           # flushed at a workgroup's end only
        "per plane": (1 + k).astype(np.float64),                    # changes inside every tile
        "at a tile edge": np.where(k < 8, 1.0, np.where(k < 64, 2.0, 3.0)),   # and a workgroup's
        "at lane 37": np.where(i < 37, 1.0, 2.0),                   # the middle of a row
        "lane by lane": (1 + i % 2).astype(np.float64),             # every single-cell visit mixed
        "pair by pair": (1 + (i // 2) % 3).astype(np.float64),      # every visit mixed
        "rows": (1 + (j + 4 * k) % 7).astype(np.float64),           # one label per row
    }


@pytest.mark.parametrize("aligned", [True, False])                  # 16-byte pairs, single cells
@pytest.mark.parametrize("pattern", list(carried_patterns()))
def test_a_wave_carries_its_record_across_visits_tiles_and_workgroups(ctx, pattern, aligned):
    labels = carried_patterns()[pattern]
    n = int(labels.max()) + 1                                       # the last clump has no cell
    k, j, i = np.indices(SHAPE)
    parents = (1 + k // 16 + (i >= 100)).astype(np.float64)         # clumps under several parents
    index_lo = [(-40, 7, -2 ** 20)]
    got = run_links(ctx, [(labels, 0)], [(parents, 0)], n, 6, index_lo, [], aligned)
    assert_links(got, links_by_hand([(labels, 0)], [(parents, 0)], n, 6, index_lo, [1]))
    assert got[0][0, n - 1] == I32_MAX and got[1][n - 1] == U32_MAX and got[3] == [0, 0]
    bare = run_links(ctx, [(labels, 0)], None, n, 0, index_lo, [], aligned)
    assert_links(bare, links_by_hand([(labels, 0)], None, n, 0, index_lo, [1]), False)
    assert np.array_equal(bare[0], got[0])


@pytest.mark.parametrize("aligned", [True, False])
def test_one_label_through_boxes_of_two_levels_in_one_workgroup(ctx, aligned):
    # 2 + 4 + 1 tiles; ratio 4: a level-0 cell covers 4 cells of the finest level
    boxes = [(np.full((8, 4, 6), 1.0), 0), (np.full((6, 8, 10), 1.0), 1), (np.full((2, 2, 2), 1.0), 0)]
    boxes[1][0][3, :, 4:] = 2.0
    index_lo = [(-3, 1, -2), (-20, 9, 40), (5, -9, 0)]
    got = run_links(ctx, boxes, None, 2, 0, index_lo, [4], aligned)
    want = links_by_hand(boxes, None, 2, 0, index_lo, [4, 1, 4])
    assert_links(got, want, False)
    assert got[0][:, 0].tolist() == [-20, -36, -8, 27, 19, 45]       # the union over both levels
    # three levels at ratios (2, 4): R = 8, 4, 1
    boxes = [(np.full((4, 4, 4), 1.0), 0), (np.full((4, 4, 4), 1.0), 1), (np.full((4, 4, 6), 1.0), 2)]
    index_lo = [(-2, 0, 0), (-9, 3, 1), (17, -31, 5)]
    got = run_links(ctx, boxes, None, 1, 0, index_lo, [2, 4], aligned)
    assert_links(got, links_by_hand(boxes, None, 1, 0, index_lo, [8, 4, 1]), False)
    assert got[0][:, 0].tolist() == [-36, -31, 0, 22, 31, 31]


@pytest.mark.parametrize("aligned", [True, False])
def test_labels_and_parents_that_are_none(ctx, aligned):
    rng = np.random.default_rng(47)
    shape = (5, 6, 131) if not aligned else (5, 6, 132)
    labels = (1 + np.indices(shape)[2] // 33).astype(np.float64)     # 1 .. 4, runs of 33 cells
    flat = labels.reshape(-1)
    strays = rng.choice(flat.size, 70, replace=False)
    flat[strays] = np.array([2.5, 6.0, -1.0, np.nan, 0.0, -0.0, np.inf])[np.arange(70) % 7]
    parents = np.full(shape, 2.0)
    bad = rng.choice(flat.size, 90, replace=False)
    parents.reshape(-1)[bad] = np.array([0.0, np.nan, 3.0, 1.5, -0.0, -2.0])[np.arange(90) % 6]
    parents[labels == 4.0] = np.where(np.indices(shape)[0] % 2 == 0, 0.0, np.nan)[labels == 4.0]
    index_lo = [(0, 0, 0)]
    got = run_links(ctx, [(labels, 0)], [(parents, 0)], 5, 2, index_lo, [], aligned)
    want = links_by_hand([(labels, 0)], [(parents, 0)], 5, 2, index_lo, [1])
    assert_links(got, want)
    # 2.5, 6.0 (= n + 1), -1, NaN, -0.0 and Inf are counted, +0.0 is skipped
    assert got[3][0] == 60 and got[3][1] > 90
    # clump 4 lies under +0.0 and NaN only: nothing contributed; clump 5 has no cell
    for c in (4, 5):
        assert got[0][:, c - 1].tolist() == [I32_MAX] * 3 + [I32_MIN] * 3
        assert (got[1][c - 1], got[2][c - 1]) == (U32_MAX, 0)
    assert (got[1][:3] == 2).all() and (got[2][:3] == 2).all()
    bare = run_links(ctx, [(labels, 0)], None, 5, 0, index_lo, [], aligned)
    assert_links(bare, links_by_hand([(labels, 0)], None, 5, 0, index_lo, [1]), False)
    assert bare[3] == [60, 0] and bare[0][0, 3] < I32_MAX


def test_a_child_across_two_parents_reports_both(ctx):
    labels = np.full((4, 4, 200), 1.0)
    labels[:, :, 150:] = 2.0
    parents = np.full((4, 4, 200), 3.0)
    parents[2, 1, 77] = 1.0
    parents[:, :, 170:] = 5.0
    got = run_links(ctx, [(labels, 0)], [(parents, 0)], 2, 5, [(0, 0, 0)], [])
    assert got[1].tolist() == [1, 3] and got[2].tolist() == [3, 5] and got[3] == [0, 0]


def test_outputs_handed_in_are_combined_into_and_a_repeat_gives_equal_bits(ctx):
    rng = np.random.default_rng(48)
    labels = (1 + rng.integers(0, 3, SHAPE)).astype(np.float64)
    labels[:, :, :5] = 0.0
    labels[labels == 2.0] = np.where(np.indices(SHAPE)[0] < 30, 2.0, 0.0)[labels == 2.0]
    parents = (1 + np.indices(SHAPE)[1]).astype(np.float64)
    index_lo = [(10, 20, 30)]
    fresh = run_links(ctx, [(labels, 0)], [(parents, 0)], 3, 4, index_lo, [])
    assert_links(fresh, links_by_hand([(labels, 0)], [(parents, 0)], 3, 4, index_lo, [1]))
    assert_links(run_links(ctx, [(labels, 0)], [(parents, 0)], 3, 4, index_lo, []), fresh)
    # pre-set ends tighter and looser than the data: the true minimum and maximum come out
    start = (np.array([[0, 500, I32_MAX], [25, 0, 21], [999, 30, 30],
                       [1000, 11, I32_MIN], [22, 500, 21], [0, 97, 35]]),
             np.array([1, 4, U32_MAX]), np.array([2, 0, 9]))
    extent = torch.tensor(start[0], dtype=torch.int32, device=ctx.device)
    low = torch.tensor(start[1], dtype=torch.int64).to(torch.uint32).to(ctx.device)
    high = torch.tensor(start[2], dtype=torch.int64).to(torch.uint32).to(ctx.device)
    totals = torch.tensor([5, 6], dtype=torch.int64, device=ctx.device)
    got = run_links(ctx, [(labels, 0)], [(parents, 0)], 3, 4, index_lo, [], extent=extent,
                    parent_lo=low, parent_hi=high, totals=totals)
    want = links_by_hand([(labels, 0)], [(parents, 0)], 3, 4, index_lo, [1], start)
    assert_links(got, (want[0], want[1], want[2], [5, 6]))
    assert (got[0] != fresh[0]).any() and (got[0] != start[0]).any()
    assert got[0][0, 0] == 0 and got[0][3, 0] == 1000 and got[0][0, 1] == fresh[0][0, 1]


def test_wrong_arguments_are_refused_and_the_outputs_untouched(ctx):
    cells = np.full((4, 4, 8), 1.0)
    labels = label_scene(ctx, [(cells, 0), (cells, 1)])
    parents = label_scene(ctx, [(cells, 0), (cells, 1)])
    short = label_scene(ctx, [(cells, 0)])
    narrow = label_scene(ctx, [(cells, 0), (cells[:, :, :-1], 1)])
    relevelled = label_scene(ctx, [(cells, 0), (cells, 0)])
    extent = torch.full((6, 3), 77, dtype=torch.int32, device=ctx.device)
    low = torch.full((3,), 55, dtype=torch.int32, device=ctx.device)
    high = torch.full((3,), 44, dtype=torch.int32, device=ctx.device)
    totals = torch.full((2,), 9, dtype=torch.int64, device=ctx.device)
    index = np.array([(0, 0, 0), (32, 0, 0)], dtype=np.int32)

    def untouched():
        ctx.synchronize()
        return bool((extent == 77).all() and (low == 55).all() and (high == 44).all() and
                    (totals == 9).all())

    def call(under=parents, n=3, n_parents=2, index=index, ratio=(2,), n_levels=2, with_low=True,
             with_high=True, with_extent=True):
        index = np.ascontiguousarray(index, np.int32)
        ratio = np.ascontiguousarray(ratio, np.int32)
        pointer = lambda t, given: C.c_void_p(t.data_ptr()) if given else None
        return _capi.lib().avr_scene_clump_links(
            ctx._handle, labels._handle, under._handle if under is not None else None, n, n_parents,
            index.ctypes.data_as(C.POINTER(C.c_int32)), ratio.ctypes.data_as(C.POINTER(C.c_int32)),
            n_levels, pointer(extent, with_extent), pointer(low, with_low), pointer(high, with_high),
            C.c_void_p(totals.data_ptr()))

    far = index.copy()
    far[1, 0] = 2 ** 30 - 7
    refined_far = index.copy()
    refined_far[0, 1] = -2 ** 29 - 1
    wrong = [
        dict(n=0), dict(n=2 ** 28), dict(n_parents=0), dict(n_parents=2 ** 28),
        dict(under=None, with_low=False, with_high=False),           # n_parents without a scene
        dict(under=None, n_parents=0),                                # parent arrays without one
        dict(with_low=False), dict(with_high=False), dict(with_extent=False),
        dict(n_levels=0), dict(n_levels=17, ratio=[2] * 16),
        dict(n_levels=1, ratio=()),                                   # a level >= n_levels
        dict(ratio=(1,)), dict(ratio=(-2,)),
        dict(index=far), dict(index=refined_far),
        dict(under=short), dict(under=narrow), dict(under=relevelled),   # incongruent
    ]
    for arguments in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert untouched(), arguments
    with pytest.raises(ValueError):
        labels.clump_links(3, index, [2], parents, 0)
    with pytest.raises(ValueError):
        labels.clump_links(3, index, [2], None, 2)
    with pytest.raises(ValueError):
        labels.clump_links(0, index, [2])
    with pytest.raises(ValueError):
        labels.clump_links(3, index, [2], extent=torch.zeros((3, 6), dtype=torch.int32,
                                                             device=ctx.device))
    assert untouched()
    assert call() == 0                                # in order: combined into what the arrays held
    ctx.synchronize()
    assert extent.cpu().numpy().tolist() == [[0, 77, 77], [0, 77, 77], [0, 77, 77],
                                             [77, 77, 77], [77, 77, 77], [77, 77, 77]]
    assert low.tolist() == [1, 55, 55] and high.tolist() == [44, 44, 44] and totals.tolist() == [9, 9]
    for scene in (labels, parents, short, narrow, relevelled):
        scene.close()


# ---- composition -----------------------------------------------------------------------------------

def test_a_covering_grid_over_a_nodes_box_holds_the_node_on_every_face(three):
    tree = api.clump_tree(three.path, "u", LADDER)
    scale = np.array([4, 2, 1], dtype=np.int64)
    step = 2                                                       # 122 clumps above 0.5
    api.add_clump_field("node", "u", LADDER[step], INF)
    nodes = np.arange(tree["node_begin"][step], tree["node_begin"][step + 1])
    biggest = nodes[np.argsort(tree["cells"][nodes])[-3:]]
    across = nodes[(tree["cells_by_level"][:, nodes] > 0).sum(axis=0) >= 2][:2]
    chosen = sorted(set(biggest.tolist()) | set(across.tolist()) | {int(nodes[0])})
    assert len(chosen) >= 4
    for v in chosen:
        lo, hi = tree["index_lo"][v].tolist(), tree["index_hi"][v].tolist()
        grid = api.covering_grid(three.path, 2, ["node"], region=(lo, hi))["fields"]["node"]
        mine = grid == float(tree["label"][v])
        for face in (mine[0], mine[-1], mine[:, 0], mine[:, -1], mine[:, :, 0], mine[:, :, -1]):
            assert face.any(), (v, lo, hi)                          # the box is tight
        assert np.count_nonzero(mine) == int((tree["cells_by_level"][:, v] * scale ** 3).sum())


def same(a, b):
    if isinstance(a, dict):
        return all(same(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return ref.same_bits(a, b) if a.dtype.kind == "f" else bool(np.array_equal(a, b))


def test_api_clumps_at_a_threshold_equals_that_slice_of_the_tree(three):
    tree = api.clump_tree(three.path, "u", LADDER, fields=["odd"])
    integral, bound = integral_and_bound(three, three.tree("u", LADDER, INF, ("odd",)), "odd")
    for step in (0, 3, 5):
        flat = api.clumps(three.path, "u", LADDER[step], INF, fields=["odd"])
        nodes = slice(tree["node_begin"][step], tree["node_begin"][step + 1])
        assert flat["n"] == nodes.stop - nodes.start and flat["outside"] == 0
        assert np.array_equal(flat["cells_by_level"], tree["cells_by_level"][:, nodes])
        assert np.array_equal(flat["cells"], tree["cells"][nodes])
        assert ref.same_bits(flat["volume"], tree["volume"][nodes])
        # two sums of the same values in no fixed order: each within the bound of the reference
        assert (np.abs(flat["integrals"]["odd"] - integral[nodes]) <= bound[nodes]).all()
        assert (np.abs(tree["integrals"]["odd"][nodes] - integral[nodes]) <= bound[nodes]).all()


def test_products_of_stored_variables_are_unchanged_around_a_tree(ctx, three, tmp_path):
    def products():
        out = str(tmp_path / "frame.ppm")
        assert api.run(three.path, api.RenderOptions(width=96, height=64, output_filename=out),
                       "u", ctx) == 0
        with open(out, "rb") as fh:
            frame = fh.read()
        return (api.slice(three.path, 40, 30, "u", axis="y"),
                api.project_axis(three.path, "z", "u", None, 53, 41), frame)

    before = products()
    assert api.clump_tree(three.path, "u", LADDER, fields=["u"])["n"] == 436
    after = products()
    for a, b in zip(before, after):
        if isinstance(a, bytes):
            assert a == b
        else:
            assert same(a, b)


def test_clump_tree_scene_keeps_two_label_scenes_and_makes_one_call_per_threshold(ctx, three,
                                                                                  monkeypatch):
    scene = plotfile.load_plotfile_geometry(ctx, three.path, "u", 0, -1, False, True)
    asked, real = [], api.clump_scene

    def counting(ctx_, inner, lower, upper, *rest):
        asked.append(lower)
        return real(ctx_, inner, lower, upper, *rest)

    monkeypatch.setattr(api, "clump_scene", counting)
    got = api.clump_tree_scene(ctx, scene, [1.5, 2.5, 50.0, 60.0], INF, three.sizes(), three.lo,
                               three.ratio)
    assert asked == [1.5, 2.5, 50.0]                               # none for the fourth
    want = three.tree("u", (1.5, 2.5, 50.0, 60.0), INF)
    assert got["counts"] == want["counts"] == [107, 10, 0, 0]
    assert np.array_equal(got["parent_labels"][1], want["parent_labels"][1])
    assert np.array_equal(got["index_lo"], want["index_lo"])
    assert np.array_equal(got["cells_by_level"], want["cells_by_level"])
