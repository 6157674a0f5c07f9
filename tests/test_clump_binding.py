"""Clump binding, what needs no GPU: the reference's self-energy against an independent arrangement
(W = 0.5 sum_i m_i phi_i from a full distance matrix), hand cases, the numpy twin, binding_segments
at its limits, collapse_tree with a validator's verdict on hand-written trees, and api.clumps and
api.clump_tree with the device work patched out -- the dicts without mass unchanged, with mass
assembled per node, and every refusal."""
import math
import os
import types

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, clumps
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import binding_reference as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
INF = math.inf


def test_the_entries_are_declared_and_the_abi_version_stays(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    for name, count in (("avr_scene_clump_members", 8), ("avr_scene_clump_member_data", 13),
                        ("avr_clump_pair_energy", 9)):
        at = header.index(f"int {name}(avr_context *ctx")
        declared = header[at:header.index(";", at)]
        assert len(_capi.SIGNATURES[name][1]) == declared.count(",") + 1 == count
        assert getattr(avr_lib, name) is not None
    assert avr_lib.avr_abi_version() == 2
    assert callable(api.clump_members) and callable(api.clump_binding_scene)


# ---- the self-energy ---------------------------------------------------------------------------------

def cloud(n, seed, zero_masses=0):
    """n members at distinct points of a lattice of spacing 2^-6, masses in [0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    sites = rng.choice(64 ** 3, n, replace=False)
    x, y, z = ((sites // 64 ** a % 64).astype(np.float64) / 64.0 for a in range(3))
    m = rng.random(n) + 0.5
    m[rng.choice(n, zero_masses, replace=False)] = 0.0
    return x, y, z, m


@pytest.mark.parametrize("n, zeros", [(2, 0), (3, 1), (17, 0), (64, 5), (300, 20)])
def test_the_reference_agrees_with_half_the_sum_of_mass_times_potential(n, zeros):
    x, y, z, m = cloud(n, 100 + n, zeros)
    want = br.self_energy(x, y, z, m)
    literal = br.self_energy_literal(x.tolist(), y.tolist(), z.tolist(), m.tolist())
    assert abs(want - literal) <= 2 * U * literal          # the same terms, rounded twice or once
    # independently: every pair twice, through a potential per member
    dx, dy, dz = (a[:, None] - a[None, :] for a in (x, y, z))
    distance = np.sqrt(dx * dx + dy * dy + dz * dz)
    np.fill_diagonal(distance, INF)
    potential = (m[None, :] / distance).sum(axis=1)
    other = 0.5 * float((m * potential).sum())
    print(n, "relative difference / (4 N u):", abs(other - want) / (4 * n * U * want))
    assert abs(other - want) <= 4 * n * U * want
    assert want > 0.0


def test_hand_cases_by_bits():
    # two cells: one term, m1 m2 / d, with d = sqrt((9 + 16) + 144) = 13
    two = ([0.0, 3.0], [1.0, 5.0], [2.0, 14.0], [0.7, 1.9])
    want = 0.7 * 1.9 / 13.0
    assert br.self_energy(*two) == br.self_energy_literal(*two) == want
    assert clumps.pair_energy(*two, [0, 2]).tolist() == [want]
    # N = 0 and N = 1: +0.0
    for n in (0, 1):
        one = ([1.0] * n, [2.0] * n, [3.0] * n, [5.0] * n)
        assert br.self_energy(*one) == br.self_energy_literal(*one) == 0.0
        got = clumps.pair_energy(*one, [0, n])
        assert got.tolist() == [0.0] and not np.signbit(got[0])
    # a member without mass adds nothing, whichever place it holds
    x, y, z, m = cloud(9, 7)
    base = br.self_energy(x, y, z, m)
    for at in (0, 4, 9):
        more = [np.insert(a, at, v) for a, v in zip((x, y, z, m), (0.3, 0.1, 0.2, 0.0))]
        assert br.self_energy(*more) == base
    # the twin: segment by segment the reference's bits, empty segments between full ones
    x, y, z, m = cloud(40, 8, 3)
    offsets = [0, 0, 7, 7, 8, 30, 40, 40]
    assert np.array_equal(clumps.pair_energy(x, y, z, m, offsets),
                          br.segment_energies(x, y, z, m, offsets))
    assert clumps.pair_energy(x, y, z, m, [0]).shape == (0,)


# ---- which clumps are evaluated -------------------------------------------------------------------------

def test_binding_segments_at_min_cells_two_max_cells_and_one_past_each():
    cells = [1, 2, 3, 4, 5, 6, 7]
    wanted, offsets = clumps.binding_segments(cells, min_cells=4, max_cells=6)
    assert wanted.tolist() == [False, False, False, True, True, True, False]
    assert offsets.tolist() == [0, 4, 9, 15] and offsets.dtype == np.int64 and wanted.dtype == bool
    # min_cells below 2: a clump of one cell has no pair
    for low in (0, 1, 2):
        wanted, offsets = clumps.binding_segments(cells, min_cells=low, max_cells=3)
        assert wanted.tolist() == [False, True, True, False, False, False, False]
        assert offsets.tolist() == [0, 2, 5]
    wanted, offsets = clumps.binding_segments(cells, 1, 1)
    assert not wanted.any() and offsets.tolist() == [0]
    wanted, offsets = clumps.binding_segments([], 1, 8)
    assert wanted.shape == (0,) and offsets.tolist() == [0]
    # the members' list takes clumps of one cell
    wanted, offsets = clumps.member_segments(cells, 1, 2)
    assert wanted.tolist() == [True, True] + [False] * 5 and offsets.tolist() == [0, 1, 3]
    # the hard limits
    most = 2 ** 22
    assert clumps.binding_segments([most, most + 1], 1, most)[0].tolist() == [True, False]
    with pytest.raises(ValueError, match="2\\^22"):
        clumps.binding_segments([5], 1, most + 1)
    assert clumps.binding_segments([most] * 511 + [most - 1], 1, most)[1][-1] == 2 ** 31 - 1
    with pytest.raises(ValueError, match="2\\^31"):
        clumps.binding_segments([most] * 512, 1, most)
    assert clumps.BINDING_DEFAULT_MAX_CELLS == 2 ** 18
    assert clumps.check_max_cells(most) == most
    with pytest.raises(ValueError, match="2\\^22"):
        clumps.check_max_cells(most + 1)


def test_bound_mask():
    got = clumps.bound_mask(2.0, [1.0, 1.0, math.nan, 0.0, 3.0], [1.0, 1.5, math.nan, 0.0, 1.0],
                            [0.5, 0.5, math.nan, 0.0, math.nan], [True, True, False, True, True])
    # 2 > 1.5; 2 > 2 is not; unevaluated; 0 > 0 is not; a NaN energy never binds
    assert got.tolist() == [True, False, True, False, False] and got.dtype == bool


# ---- collapse_tree with a validator's verdict -----------------------------------------------------------

HAND_TREES = [([-1, 0, 1, 2], [9, 7, 5, 2], 1), ([-1, 0, 0], [9, 4, 3], 1),
              ([-1, 0, 1, 1, 2], [9, 8, 4, 3, 1], 1), ([-1, 0, 0, 1], [9, 6, 2, 5], 3),
              ([-1, 0, 0, 1], [9, 6, 2, 5], 2), ([-1, -1, 0, 0, 1, 1], [2, 9, 1, 1, 4, 4], 3),
              ([-1, 0, 0, 1, 1, 2], [6, 3, 3, 1, 1, 1], 1), ([], [], 1)]


def fold(parent, cells, min_cells, passes=None):
    return {k: v.tolist() for k, v in clumps.collapse_tree(parent, cells, min_cells, passes).items()}


def literal_collapse(parent, cells, min_cells, passes):
    """The issue's rule, node by node: validity is inherited from the top down."""
    n = len(parent)
    valid = []
    for v in range(n):
        valid.append(cells[v] >= min_cells and bool(passes[v]) and
                     (parent[v] == -1 or valid[parent[v]]))
    valid_children = [sum(1 for w in range(n) if parent[w] == v and valid[w]) for v in range(n)]
    kept = [valid[v] and (parent[v] == -1 or valid_children[parent[v]] >= 2) for v in range(n)]
    kept_parent = []
    for v in range(n):
        up = parent[v] if kept[v] else -1
        while up >= 0 and not kept[up]:
            up = parent[up]
        kept_parent.append(up)
    leaves = [v for v in range(n) if kept[v] and v not in set(kept_parent)]
    return {"kept": kept, "kept_parent": kept_parent, "leaves": leaves}


@pytest.mark.parametrize("parent, cells, min_cells", HAND_TREES)
def test_without_passes_and_with_all_passing_the_collapse_is_todays(parent, cells, min_cells):
    """The hand-written trees of test_clump_tree.py, whose counts fall from parent to child: the
    inherited rule, all nodes passing, gives what the count alone gives."""
    today = fold(parent, cells, min_cells)
    assert fold(parent, cells, min_cells, None) == today
    assert fold(parent, cells, min_cells, [True] * len(parent)) == today
    assert literal_collapse(parent, cells, min_cells, [True] * len(parent)) == today


def test_collapse_tree_with_passes_on_hand_written_trees():
    # a bound child under an unbound parent is dropped with it; the root's other child stays, a
    # sole child now
    parent, cells = [-1, 0, 0, 1, 1], [20, 9, 8, 4, 3]
    assert fold(parent, cells, 1, [True, False, True, True, True]) == {
        "kept": [True, False, False, False, False], "kept_parent": [-1] * 5, "leaves": [0]}
    assert fold(parent, cells, 1)["kept"] == [True] * 5
    # an unbound sibling: the other one is a sole child and folds into the parent
    assert fold([-1, 0, 0], [9, 4, 3], 1, [True, True, False]) == {
        "kept": [True, False, False], "kept_parent": [-1, -1, -1], "leaves": [0]}
    # an unbound sole child takes the chain below it along
    assert fold([-1, 0, 1, 1], [9, 8, 4, 3], 1, [True, False, True, True]) == {
        "kept": [True, False, False, False], "kept_parent": [-1] * 4, "leaves": [0]}
    assert fold([-1, 0, 1, 1], [9, 8, 4, 3], 1)["kept"] == [True, False, True, True]
    # unevaluated roots pass (bound_mask gives True), an unbound root goes with its subtree
    passes = clumps.bound_mask(1.0, [math.nan, 1.0, 5.0, 5.0, 5.0, 5.0], [math.nan, 2.0, 1, 1, 1, 1],
                               [math.nan, 0.0, 0, 0, 0, 0], [False, True, True, True, True, True])
    assert passes.tolist() == [True, False, True, True, True, True]
    assert fold([-1, -1, 0, 0, 1, 1], [50, 40, 9, 8, 7, 6], 1, passes) == {
        "kept": [True, False, True, True, False, False], "kept_parent": [-1, -1, 0, 0, -1, -1],
        "leaves": [2, 3]}
    # min_cells and passes together, against the rule written out node by node
    rng = np.random.default_rng(3)
    for _ in range(50):
        n = int(rng.integers(1, 12))
        parent = [-1] + [int(rng.integers(-1, v)) for v in range(1, n)]
        cells = [int(c) for c in rng.integers(1, 9, n)]
        passes = [bool(p) for p in rng.integers(0, 4, n)]
        assert fold(parent, cells, 3, passes) == literal_collapse(parent, cells, 3, passes)
    with pytest.raises(ValueError, match="passes"):
        clumps.collapse_tree([-1, 0], [3, 2], 1, [True])


# ---- api.clumps and api.clump_tree with the device work patched out -------------------------------------

class FakeScene:
    def __init__(self, ctx, what):
        self.ctx, self.what = ctx, what

    def clump_table(self, n, n_levels, field=None):
        import torch
        self.ctx.asked.append(("table", self.what, None if field is None else field.what))
        cells = self.ctx.cells[self.what]
        return (torch.tensor(cells, dtype=torch.int64),
                None if field is None else torch.zeros((n_levels, n), dtype=torch.float64),
                torch.zeros(2, dtype=torch.int64))

    def clump_links(self, n, index, ratios, parents=None, n_parents=0):
        import torch
        extent = torch.zeros((6, n), dtype=torch.int32)
        held = None if parents is None else torch.from_numpy(
            np.array(self.ctx.parents[self.what], dtype=np.uint32))
        return extent, held, held, torch.zeros(2, dtype=torch.int64)

    def close(self):
        pass


class FakeContext:
    """Scenes that answer the table and the links from prepared arrays, on the host."""

    def __init__(self, cells, parents):
        self.cells, self.parents, self.asked = cells, parents, []

    def synchronize(self):
        pass

    def create_scene(self, boxes, transform):
        return FakeScene(self, boxes[0])


@pytest.fixture
def patched(monkeypatch, tmp_path):
    """Threshold 1.0: two clumps of 11 and 16 cells; 2.0: three of 1, 8 and 2 under clumps 2, 1, 2;
    nothing at 3.0.  Binding answers come from `verdicts`, per label scene."""
    from amrvolumerenderer_amd import plotfile
    import gradient_reference as ref
    levels = ref.make_levels([((0, 0, 0), (3, 3, 3)), ((0, 0, 0), (7, 7, 7))],
                             [[((0, 0, 0), (3, 3, 3))], [((2, 2, 2), (5, 5, 5))]], [2], 5)
    path = str(tmp_path / "plt")
    plotfile.write_plotfile(path, list(ref.VARIABLES), levels, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), [2])
    ctx = FakeContext({1.0: [[3, 0], [8, 16]], 2.0: [[1, 0, 0], [0, 8, 2]]}, {2.0: [2, 1, 2]})
    counts = {1.0: 2, 2.0: 3, 3.0: 0}
    scene = lambda what: types.SimpleNamespace(local_boxes=[what], all_boxes=[what],
                                               scalar_transform=None)
    state = types.SimpleNamespace(ctx=ctx, path=path, loaded=[], binding_calls=[], verdicts={})

    def fake_load_fields(plotfile_path, variables, min_level, max_level):
        state.loaded.append(list(variables))
        return ctx, 0, 1, None, [scene(name) for name in variables], [0.5, 0.0625]

    def fake_clump_scene(ctx_, inner, lower, upper, cell_sizes, prob_lo, ref_ratio, rank=0,
                         n_ranks=1, process_group=None):
        return scene(lower), counts[lower]

    def fake_binding(ctx_, labels, n, cells, mass, velocity, thermal, cell_sizes, prob_lo,
                     ref_ratio, G=6.6743e-8, min_cells=1, max_cells=2 ** 18, n_ranks=1):
        what = labels.local_boxes[0]
        state.binding_calls.append((what, n, list(cells), mass.local_boxes[0],
                                    None if velocity is None else [v.local_boxes[0] for v in velocity],
                                    None if thermal is None else thermal.local_boxes[0],
                                    G, min_cells, max_cells))
        evaluated = np.array([max(min_cells, 2) <= c <= max_cells for c in cells])
        bound = np.where(evaluated, np.array(state.verdicts[what]), True)
        number = np.where(evaluated, np.arange(n) + 10.0 * what, np.nan)
        return {"mass": number, "self_energy": number * 2, "kinetic": number * 3,
                "thermal": number * 4, "bound": bound, "evaluated": evaluated,
                "excluded": np.arange(n, dtype=np.int64), "nonfinite": 5}

    monkeypatch.setattr(api, "_load_fields", fake_load_fields)
    monkeypatch.setattr(api, "clump_scene", fake_clump_scene)
    monkeypatch.setattr(api, "_level_setup",
                        lambda geometry, local, sizes, lo, ratio: ([tuple(c) for c in sizes], [2], "index"))
    monkeypatch.setattr(api, "clump_binding_scene", fake_binding)
    return state


PLAIN_KEYS = ["n", "cells_by_level", "cells", "volume", "integrals", "outside", "nonfinite"]
BINDING_KEYS = ["mass", "self_energy", "kinetic", "thermal", "bound", "evaluated", "excluded"]


def same_dict(a, b):
    assert list(a) == list(b)
    for key in a:
        if isinstance(a[key], dict):
            same_dict(a[key], b[key])
        elif isinstance(a[key], np.ndarray):
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
        else:
            assert type(a[key]) is type(b[key]) and a[key] == b[key], key


def test_api_clumps_without_mass_is_unchanged_and_with_mass_gains_the_binding(patched):
    plain = api.clumps(patched.path, "u", 1.0, fields=["odd"])
    assert list(plain) == PLAIN_KEYS and patched.binding_calls == []
    assert patched.loaded == [["u", "odd"]]                      # nothing else is loaded
    asked = list(patched.ctx.asked)
    assert asked == [("table", 1.0, None), ("table", 1.0, "odd")]
    assert plain["cells"].tolist() == [11, 16] and plain["nonfinite"] == 0
    patched.verdicts[1.0] = [False, True]
    got = api.clumps(patched.path, "u", 1.0, fields=["odd"], mass="whole",
                     velocity=("u", "odd", "whole"), thermal="u", G=2.5, max_cells=12)
    assert list(got) == PLAIN_KEYS + BINDING_KEYS
    same_dict({key: got[key] for key in PLAIN_KEYS if key != "nonfinite"},
              {key: plain[key] for key in PLAIN_KEYS if key != "nonfinite"})
    assert patched.loaded[-1] == ["u", "odd", "whole", "u", "odd", "whole", "u"]
    assert patched.binding_calls == [(1.0, 2, [11, 16], "whole", ["u", "odd", "whole"], "u", 2.5,
                                      1, 12)]
    assert got["evaluated"].tolist() == [True, False] and got["bound"].tolist() == [False, True]
    assert got["mass"][0] == 10.0 and np.isnan(got["mass"][1]) and got["nonfinite"] == 5
    assert got["excluded"].tolist() == [0, 1]
    # the same device work around it, and the same dict after it
    assert patched.ctx.asked[len(asked):] == asked
    same_dict(api.clumps(patched.path, "u", 1.0, fields=["odd"]), plain)
    only_mass = api.clumps(patched.path, "u", 1.0, mass="whole")
    assert patched.loaded[-1] == ["u", "whole"]
    assert patched.binding_calls[-1][3:] == ("whole", None, None, 6.6743e-8, 1, 2 ** 18)
    assert only_mass["evaluated"].tolist() == [True, True]


def test_api_clump_tree_evaluates_per_threshold_and_collapses_with_the_verdicts(patched, tmp_path):
    plain = api.clump_tree(patched.path, "u", [1.0, 2.0, 3.0], fields=["odd"])
    assert patched.binding_calls == [] and not set(BINDING_KEYS) & set(plain)
    assert plain["kept"].tolist() == [True, True, True, False, True]
    patched.verdicts.update({1.0: [True, False], 2.0: [True, True, True]})
    out = str(tmp_path / "tree.npz")
    got = api.clump_tree(patched.path, "u", [1.0, 2.0, 3.0], fields=["odd"], mass="whole",
                         thermal="odd", G=3.0, max_cells=12, output=out)
    assert patched.loaded[-1] == ["u", "odd", "whole", "odd"]
    assert [call[:3] for call in patched.binding_calls] == [(1.0, 2, [11, 16]), (2.0, 3, [1, 8, 2])]
    assert all(call[3:] == ("whole", None, "odd", 3.0, 1, 12) for call in patched.binding_calls)
    # node 1 (16 cells) is past max_cells: unevaluated, and kept whatever its verdict
    assert got["evaluated"].tolist() == [True, False, False, True, True]
    assert got["bound"].tolist() == [True, True, True, True, True]
    assert got["kept"].tolist() == plain["kept"].tolist()
    assert got["mass"][[0, 3, 4]].tolist() == [10.0, 21.0, 22.0] and np.isnan(got["mass"][[1, 2]]).all()
    assert got["self_energy"][3] == 42.0 and got["kinetic"][3] == 63.0 and got["thermal"][3] == 84.0
    assert got["excluded"].tolist() == [0, 1, 0, 1, 2] and got["nonfinite"] == plain["nonfinite"] + 10
    for key in set(plain) - {"nonfinite"}:
        same_dict({key: got[key]}, {key: plain[key]})
    saved = np.load(out)
    assert np.array_equal(saved["bound"], got["bound"]) and saved["mass"].dtype == np.float64
    # node 0 unbound: its child, node 3, goes with it; nodes 2 and 4 stay under node 1
    patched.verdicts.update({1.0: [False, True]})
    got = api.clump_tree(patched.path, "u", [1.0, 2.0, 3.0], mass="whole", max_cells=12)
    assert got["bound"].tolist() == [False, True, True, True, True]
    assert got["kept"].tolist() == [False, True, True, False, True]
    assert got["leaves"].tolist() == [2, 4]
    # min_cells reaches the evaluation: clumps below it are not summed
    got = api.clump_tree(patched.path, "u", [1.0, 2.0], mass="whole", min_cells=8)
    assert got["evaluated"].tolist() == [True, True, False, True, False]
    assert patched.binding_calls[-1][7:] == (8, 2 ** 18)
    same_dict(api.clump_tree(patched.path, "u", [1.0, 2.0, 3.0], fields=["odd"]), plain)


def test_every_refusal_comes_before_any_device_work(patched):
    calls = lambda: (len(patched.loaded), len(patched.binding_calls))
    before = calls()
    for function, arguments in ((api.clumps, (1.0,)), (api.clump_tree, ([1.0, 2.0],))):
        for bad in (dict(velocity=("u", "u", "u")), dict(thermal="u"),
                    dict(mass="u", velocity=("u", "u")), dict(mass="u", max_cells=2 ** 22 + 1)):
            with pytest.raises(ValueError):
                function(patched.path, "u", *arguments, **bad)
    assert calls() == before


def test_boxes_on_other_ranks_and_wrong_arguments_are_refused_before_any_device_work():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the context was used ({name})")

    box = AmrBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), level=0, dims=(4, 4, 4))
    bounds = VolumeBounds((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    whole = api.SceneGeometry([box, box], [box, box], ScalarTransform(), bounds)
    part = api.SceneGeometry([box, box], [box], ScalarTransform(), bounds)
    levels = ([(0.25, 0.25, 0.25)], (0.0, 0.0, 0.0), [])
    for labels, ranks in ((whole, 2), (part, 1)):
        with pytest.raises(NotImplementedError):
            api.clump_members_scene(NoDevice(), labels, 2, [5, 6], *levels, n_ranks=ranks)
        with pytest.raises(NotImplementedError):
            api.clump_binding_scene(NoDevice(), labels, 2, [5, 6], whole, None, None, *levels,
                                    n_ranks=ranks)
    with pytest.raises(ValueError, match="three"):
        api.clump_binding_scene(NoDevice(), whole, 2, [5, 6], whole, [whole, whole], None, *levels)
    for G in (0.0, -1.0, INF, math.nan):
        with pytest.raises(ValueError, match="G"):
            api.clump_binding_scene(NoDevice(), whole, 2, [5, 6], whole, None, None, *levels, G=G)
    with pytest.raises(ValueError, match="2\\^22"):
        api.clump_binding_scene(NoDevice(), whole, 2, [5, 6], whole, None, None, *levels,
                                max_cells=2 ** 22 + 1)
    with pytest.raises(ValueError, match="one count per clump"):
        api.clump_binding_scene(NoDevice(), whole, 3, [5, 6], whole, None, None, *levels)
    with pytest.raises(ValueError, match="one count per clump"):
        api.clump_members_scene(NoDevice(), whole, 3, [5, 6], *levels)
    # nothing to evaluate: no device work, every clump unevaluated and kept
    got = api.clump_binding_scene(NoDevice(), whole, 2, [1, 9], whole, None, None, *levels,
                                  max_cells=8)
    assert got["evaluated"].tolist() == [False, False] and got["bound"].tolist() == [True, True]
    assert np.isnan(got["self_energy"]).all() and got["excluded"].tolist() == [0, 0]
    none = api.clump_members_scene(NoDevice(), whole, 2, [1, 9], *levels, min_cells=2, max_cells=8)
    assert none["labels"].shape == (0,) and none["offsets"].tolist() == [0]
    assert none["centres"].shape == (0, 3)
