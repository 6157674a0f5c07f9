"""Clump binding on the GPU: clump_members_kernel and clump_member_data_kernel through
avr_scene_clump_members / _member_data and api.clump_members, clump_pair_kernel and its reduction
through avr_clump_pair_energy, and api.clumps / api.clump_tree with a mass field, against the
reference on the plotfile's own level arrays (binding_reference).  Keys, offsets and levels are
equal; centres and values are equal by bits (cell sizes are powers of two).  A self-energy lies
within (depth + 8) 2^-53 W of the reference -- depth as the call returns it, asserted <= N + 64:
that many rounded additions and the 8 * 2^-53 of a term -- plus the reference's own 8 * 2^-53 W.
M and T lie within (n - 1) 2^-53 sum |terms| of the reference and its one rounding, the a-priori
bound of n additions in any order as the clump tables are held to it (the terms themselves are
equal: volumes are powers of two); K also within what the shift of vbar allows.  The hand-made
label scenes are the smallest at which the slots a wave reserves can go wrong: 17 tiles (two
workgroups), a label change in the middle of a row, lane by lane, and a wanted mask that
alternates, on both access widths and on odd rows at even strides."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, clumps, plotfile
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform

import binding_reference as br
import clump_reference as cr
import clump_tree_reference as tr
import gradient_reference as ref

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)
INF = math.inf
U = 2.0 ** -53
INVALID = _capi.AVR_ERR_INVALID_ARGUMENT


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

    def scene_boxes(self):
        convex = plotfile.convexify([lev["boxes"] for lev in self.levels], self.ratio)
        return [(l, lo, hi) for l in range(len(self.levels)) for _, (lo, hi) in convex[l]]

    def volumes(self):
        return api.level_cell_volumes(self.sizes())


def _write(path, domains, boxes, lo, hi, ratio, seed):
    levels = ref.make_levels(domains, boxes, ratio, seed)
    case = Case(str(path), levels, lo, hi, list(ratio))
    for size in case.sizes():
        assert all(np.frexp(s)[0] == 0.5 for s in size)             # powers of two
    plotfile.write_plotfile(str(path), VARIABLES, levels, lo, hi, ratio)
    return case


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    """Three levels at ratio 2: two fine boxes that touch, the finest grid inside the first."""
    return _write(tmp_path_factory.mktemp("binding") / "three",
                  [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (47, 23, 31))],
                  [[((0, 0, 0), (6, 5, 7)), ((7, 0, 0), (11, 5, 7))],
                   [((4, 2, 2), (11, 7, 9)), ((12, 2, 2), (17, 9, 9))],
                   [((12, 6, 6), (21, 13, 15))]],
                  (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2], 41)


@pytest.fixture(scope="module")
def ratio_four(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("binding") / "four",
                  [((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (23, 15, 15))],
                  [[((0, 0, 0), (5, 3, 3))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (3.0, 2.0, 2.0), [4], 43)


@pytest.fixture(scope="module")
def skipped_level(tmp_path_factory):
    """The finest grid covers the low-x half of the middle one: a level-0 leaf lies face to face
    with level-2 cells."""
    return _write(tmp_path_factory.mktemp("binding") / "skipped",
                  [((0, 0, 0), (7, 3, 3)), ((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))],
                  [[((0, 0, 0), (7, 3, 3))], [((4, 2, 2), (11, 5, 5))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2, 2], 44)


def reference_clumps(case, variable, lower, upper=INF):
    """(per-level label arrays, n, cells per clump) of the reference."""
    labels, n = cr.clump_levels(case.levels, case.ratio, VARIABLES.index(variable), lower, upper,
                                case.scene_boxes())
    cells = np.zeros(n, dtype=np.int64)
    for level in labels:
        found = level[level > 0.0].astype(np.int64)
        cells += np.bincount(found - 1, minlength=n)
    return labels, n, cells


# ---- members through api.clump_members ------------------------------------------------------------------

def check_members(case, lower, min_cells, max_cells):
    labels, n, cells = reference_clumps(case, "u", lower)
    wanted, offsets = clumps.member_segments(cells, min_cells, max_cells)
    want = br.members(labels, n, wanted, case.levels, case.ratio, case.scene_boxes(), case.lo,
                      case.sizes(), (VARIABLES.index("odd"), VARIABLES.index("whole")))
    got = api.clump_members(case.path, "u", lower, fields=["odd", "whole"], min_cells=min_cells,
                            max_cells=max_cells)
    assert got["n"] == n and 0 < wanted.sum() < n
    assert np.array_equal(got["labels"], want["labels"]) and got["labels"].dtype == np.int64
    assert np.array_equal(got["offsets"], want["offsets"]) and np.array_equal(offsets, want["offsets"])
    assert np.array_equal(got["ordinal"], want["ordinal"]) and got["ordinal"].dtype == np.int64
    assert np.array_equal(got["level"], want["level"]) and got["level"].dtype == np.uint8
    assert got["centres"].shape == (int(offsets[-1]), 3)
    assert ref.same_bits(got["centres"], want["centres"])
    assert ref.same_bits(got["values"]["odd"], want["values"][VARIABLES.index("odd")])
    assert ref.same_bits(got["values"]["whole"], want["values"][VARIABLES.index("whole")])
    return got


def test_members_of_three_levels(three, tmp_path):
    got = check_members(three, 0.4, 2, 200)
    assert len(set(got["level"].tolist())) == 3 and not np.isfinite(got["values"]["odd"]).all()
    # clumps of one cell are listed too, and the file holds the arrays
    single = check_members(three, 1.5, 1, 1)
    assert (np.diff(single["offsets"]) == 1).all() and single["labels"].size > 3
    out = str(tmp_path / "members.npz")
    saved = api.clump_members(three.path, "u", 1.5, fields=["whole"], max_cells=1, output=out)
    held = np.load(out)
    assert np.array_equal(held["ordinal"], saved["ordinal"]) and int(held["n"]) == saved["n"]
    assert np.array_equal(held["value_whole"], saved["values"]["whole"])
    assert np.array_equal(held["centres"], single["centres"])
    none = api.clump_members(three.path, "u", 50.0, fields=["whole"])
    assert none["n"] == 0 and none["ordinal"].shape == (0,) and none["offsets"].tolist() == [0]


def test_members_at_ratio_four(ratio_four):
    got = check_members(ratio_four, 0.3, 2, 10 ** 6)
    assert set(got["level"].tolist()) == {0, 1}


def test_members_next_to_a_skipped_level(skipped_level):
    got = check_members(skipped_level, 0.2, 3, 10 ** 6)
    assert set(got["level"].tolist()) == {0, 1, 2}


# ---- avr_scene_clump_members on hand-made label scenes ----------------------------------------------------

SHAPE = (68, 4, 128)        # 17 tiles of 4 planes: two workgroups, the second with one tile


def label_scene(ctx, boxes, aligned=True, padded=False):
    """A scene over boxes of hand-made cells: (cells [nz, ny, nx], level).  Not aligned: every box
    starts 8 bytes off a 16-byte boundary, so the kernel reads single cells.  Padded: rows of nx +
    nx % 2 + 2 elements and two rows more per plane (poisoned), so that a box of odd nx still has
    even strides and is read in pairs, its last cell alone."""
    made = []
    for cells, level in boxes:
        nz, ny, nx = cells.shape
        row, rows = (nx + nx % 2 + 2, ny + 2) if padded else (nx, ny)
        flat = torch.full((nz * rows * row + 3,), 1e30, dtype=torch.float64, device=ctx.device)
        offset = (flat.data_ptr() // 8 + (0 if aligned else 1)) % 2
        view = flat[offset:offset + nz * rows * row].view(nz, rows, row)[:, :ny, :nx]
        view.copy_(torch.from_numpy(np.ascontiguousarray(cells, dtype=np.float64)))
        assert view.data_ptr() % 16 == (0 if aligned else 8)
        made.append(AmrBox((0.0, 0.0, 0.0), (float(nx), float(ny), float(nz)), view, level))
    return ctx.create_scene(made, ScalarTransform())


def members_by_hand(boxes, n, wanted):
    """The rules of avr_scene_clump_members, in numpy: (sorted keys, outside)."""
    keys, outside, begin = [], 0, 0
    for cells, _ in boxes:
        flat = cells.reshape(-1)
        active = flat.view(np.int64) != 0                               # not +0.0
        with np.errstate(invalid="ignore"):
            integer = (flat >= 1.0) & (flat <= n) & (flat == np.floor(flat))
        outside += int((active & ~integer).sum())
        at = np.nonzero(active & integer)[0]
        c = flat[at].astype(np.int64) - 1
        keep = np.asarray(wanted, dtype=bool)[c]
        keys.append((c[keep] << 32) | (begin + at[keep]))
        begin += flat.size
    return np.sort(np.concatenate(keys)), outside


def member_patterns():
    k, j, i = np.indices(SHAPE)
    return {
        "one label": (np.full(SHAPE, 2.0), [0, 1, 0]),
        "per plane": ((1 + k).astype(np.float64), [p % 3 != 1 for p in range(69)]),
        "at lane 37": (np.where(i < 37, 1.0, 2.0), [0, 1]),
        "lane by lane": ((1 + i % 2).astype(np.float64), [1, 0, 0]),
        "alternating mask": ((1 + (i + 128 * j) % 64).astype(np.float64), [c % 2 for c in range(64)]),
        "every lane": ((1 + (i + j + k) % 5).astype(np.float64), [1] * 5),
    }


@pytest.mark.parametrize("aligned", [True, False])                  # 16-byte pairs, single cells
@pytest.mark.parametrize("pattern", list(member_patterns()))
def test_every_member_takes_one_slot_across_visits_tiles_and_workgroups(ctx, pattern, aligned):
    labels, wanted = member_patterns()[pattern]
    n = len(wanted)
    want, _ = members_by_hand([(labels, 0)], n, wanted)
    scene = label_scene(ctx, [(labels, 0)], aligned)
    keys, totals = scene.clump_members(n, wanted, want.size)        # the capacity is exact
    assert keys.dtype == torch.int64 and np.array_equal(keys.cpu().numpy(), want)
    assert totals.tolist() == [0] and want.size > 1000
    with pytest.raises(ValueError, match="member cells"):
        scene.clump_members(n, wanted, want.size - 1)
    scene.close()


@pytest.mark.parametrize("aligned", [True, False])
def test_stray_labels_boxes_of_two_levels_and_a_capacity_one_short(ctx, aligned):
    rng = np.random.default_rng(51)
    first = (1 + np.indices((5, 6, 131 if not aligned else 132))[2] // 33).astype(np.float64)
    flat = first.reshape(-1)
    strays = rng.choice(flat.size, 70, replace=False)
    flat[strays] = np.array([2.5, 6.0, -1.0, np.nan, 0.0, -0.0, np.inf])[np.arange(70) % 7]
    second = (1 + np.indices((3, 2, 10))[0]).astype(np.float64) + 1.0        # labels 2 .. 4
    boxes = [(first, 0), (np.zeros((2, 2, 2)), 0), (second, 1)]
    wanted = [1, 0, 1, 1, 1]
    want, outside = members_by_hand(boxes, 5, wanted)
    assert outside == 60
    scene = label_scene(ctx, boxes, aligned)
    keys, totals = scene.clump_members(5, wanted, want.size,
                                       torch.full((1,), 7, dtype=torch.int64, device=ctx.device))
    assert np.array_equal(keys.cpu().numpy(), want) and totals.tolist() == [7 + 60]
    # odd rows at even strides: read in pairs, the last cell of a row alone; the padding is poison
    odd_rows = [(first[:, :, :131].copy(), 0), (second[:, :, :9].copy(), 1)]
    padded = label_scene(ctx, odd_rows, True, padded=True)
    assert padded.boxes[0].values.stride(1) % 2 == 0 and padded.boxes[0].values.stride(0) % 2 == 0
    by_hand, strays_outside = members_by_hand(odd_rows, 5, wanted)
    keys, totals = padded.clump_members(5, wanted, by_hand.size)
    assert np.array_equal(keys.cpu().numpy(), by_hand) and totals.tolist() == [strays_outside]
    padded.close()
    # one slot short: the count is reported, and nothing is written past the end
    capacity = want.size - 1
    buffer = torch.full((capacity + 64,), -7, dtype=torch.int64, device=ctx.device)
    count = torch.full((1,), 99, dtype=torch.int64, device=ctx.device)
    totals = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    mask = torch.tensor(wanted, dtype=torch.uint8, device=ctx.device)
    ctx.join()
    status = _capi.lib().avr_scene_clump_members(
        ctx._handle, scene._handle, 5, C.c_void_p(mask.data_ptr()), capacity,
        C.c_void_p(buffer.data_ptr()), C.c_void_p(count.data_ptr()), C.c_void_p(totals.data_ptr()))
    assert status == 0
    ctx.synchronize()
    assert count.item() == want.size and totals.item() == 60
    assert (buffer[capacity:] == -7).all()
    written = buffer[:capacity].cpu().numpy()
    assert len(set(written.tolist())) == capacity and set(written.tolist()) <= set(want.tolist())
    scene.close()


def test_member_data_on_two_levels_both_widths_and_a_key_that_names_no_cell(ctx):
    rng = np.random.default_rng(52)
    shapes = [((3, 5, 7), 0), ((2, 2, 2), 1), ((4, 3, 9), 1)]
    values = [(rng.standard_normal(shape), level) for shape, level in shapes]
    values[2][0][1, 2, 3] = np.nan
    index_lo = [(-3, 4, 0), (10, -6, 2), (-20, 0, 7)]
    sizes = [(0.5, 0.25, 1.0), (0.125, 0.0625, 0.25)]
    prob_lo = (-1.0, 2.0, 0.5)
    n_cells = sum(v.size for v, _ in values)
    ordinals = rng.permutation(n_cells)[:150]
    keys = np.sort((rng.integers(0, 9, ordinals.size).astype(np.int64) << 32) | ordinals)
    keys = np.concatenate([keys, [(3 << 32) | n_cells, (1 << 32) | (2 ** 32 - 1)]])
    want_level, want_centre, want_value = [], [], []
    begins = np.cumsum([0] + [v.size for v, _ in values])
    for key in keys.tolist():
        ordinal = key & 0xffffffff
        if ordinal >= n_cells:
            want_level.append(255), want_centre.append([np.nan] * 3), want_value.append(np.nan)
            continue
        b = int(np.searchsorted(begins, ordinal, side="right")) - 1
        cells, level = values[b]
        k, j, i = np.unravel_index(ordinal - begins[b], cells.shape)
        want_level.append(level)
        want_centre.append([prob_lo[a] + (float(index_lo[b][a] + at) + 0.5) * sizes[level][a]
                            for a, at in enumerate((i, j, k))])
        want_value.append(cells[k, j, i])
    for aligned in (True, False):
        scene = label_scene(ctx, [(np.zeros(shape), level) for shape, level in shapes])
        field = label_scene(ctx, values, aligned)
        device_keys = torch.from_numpy(keys).to(ctx.device)
        levels, centres, none = scene.clump_member_data(device_keys, index_lo, [2], sizes, prob_lo)
        assert none is None and levels.dtype == torch.uint8 and centres.shape == (3, keys.size)
        assert levels.cpu().tolist() == want_level
        assert ref.same_bits(centres.cpu().numpy().T, np.array(want_centre))
        no_levels, no_centres, read = scene.clump_member_data(device_keys, index_lo, [2], sizes,
                                                             prob_lo, field=field, centres=False)
        assert no_levels is None and no_centres is None
        assert ref.same_bits(read.cpu().numpy(), np.array(want_value))
        with pytest.raises(ValueError):
            scene.clump_member_data(device_keys, index_lo, [2], sizes, prob_lo, centres=False)
        empty = scene.clump_member_data(device_keys[:0], index_lo, [2], sizes, prob_lo, field=field)
        assert [tuple(t.shape) for t in empty] == [(0,), (3, 0), (0,)]
        scene.close()
        field.close()


def test_wrong_member_arguments_are_refused_and_the_outputs_untouched(ctx):
    cells = np.full((4, 4, 8), 1.0)
    labels = label_scene(ctx, [(cells, 0), (cells, 1)])
    field = label_scene(ctx, [(cells, 0), (cells, 1)])
    short = label_scene(ctx, [(cells, 0)])
    narrow = label_scene(ctx, [(cells, 0), (cells[:, :, :-1], 1)])
    deep = label_scene(ctx, [(cells, 0), (cells, 16)])
    device = ctx.device
    keys = torch.full((300,), 77, dtype=torch.int64, device=device)
    count = torch.full((1,), 55, dtype=torch.int64, device=device)
    totals = torch.full((1,), 9, dtype=torch.int64, device=device)
    wanted = torch.ones(3, dtype=torch.uint8, device=device)
    values = torch.full((300,), 7.0, dtype=torch.float64, device=device)
    centres = torch.full((3, 300), 6.0, dtype=torch.float64, device=device)
    levels = torch.full((300,), 5, dtype=torch.uint8, device=device)
    pointer = lambda t, given=True: C.c_void_p(t.data_ptr()) if given else None

    def untouched():
        ctx.synchronize()
        return bool((keys == 77).all() and (count == 55).all() and (totals == 9).all() and
                    (values == 7.0).all() and (centres == 6.0).all() and (levels == 5).all())

    def members(scene=labels, n=3, capacity=300, with_wanted=True, with_keys=True, with_count=True,
                with_totals=True):
        return _capi.lib().avr_scene_clump_members(
            ctx._handle, scene._handle if scene is not None else None, n, pointer(wanted, with_wanted),
            capacity, pointer(keys, with_keys), pointer(count, with_count),
            pointer(totals, with_totals))

    for arguments in (dict(n=0), dict(n=2 ** 28), dict(capacity=0), dict(capacity=2 ** 31),
                      dict(scene=None), dict(with_wanted=False), dict(with_keys=False),
                      dict(with_count=False), dict(with_totals=False), dict(scene=deep)):
        assert members(**arguments) == INVALID, arguments
        assert untouched(), arguments

    index = np.array([(0, 0, 0), (32, 0, 0)], dtype=np.int32)
    sizes = np.array([(0.5, 0.5, 0.5), (0.25, 0.25, 0.25)])
    origin = np.zeros(3)

    def data(scene=labels, under=field, n=200, index=index, ratio=(2,), sizes=sizes, origin=origin,
             n_levels=2, with_keys=True, with_values=True, with_centres=True, with_levels=True):
        index = np.ascontiguousarray(index, np.int32)
        ratio = np.ascontiguousarray(ratio, np.int32)
        sizes = np.ascontiguousarray(sizes, np.float64)
        origin = np.ascontiguousarray(origin, np.float64)
        doubles = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        return _capi.lib().avr_scene_clump_member_data(
            ctx._handle, scene._handle if scene is not None else None, pointer(keys, with_keys), n,
            under._handle if under is not None else None, pointer(values, with_values),
            index.ctypes.data_as(C.POINTER(C.c_int32)), ratio.ctypes.data_as(C.POINTER(C.c_int32)),
            doubles(sizes), doubles(origin), n_levels, pointer(centres, with_centres),
            pointer(levels, with_levels))

    far = index.copy()
    far[1, 0] = 2 ** 30 - 7
    flat = sizes.copy()
    flat[1, 2] = 0.0
    nowhere = origin.copy()
    nowhere[1] = np.nan
    for arguments in (dict(scene=None), dict(with_keys=False), dict(n=2 ** 31),
                      dict(under=None), dict(with_values=False),               # half a group
                      dict(with_centres=False), dict(with_levels=False),
                      dict(under=None, with_values=False, with_centres=False, with_levels=False),
                      dict(n_levels=0), dict(n_levels=17), dict(n_levels=1, ratio=()),
                      dict(ratio=(1,)), dict(index=far), dict(sizes=flat), dict(origin=nowhere),
                      dict(under=short), dict(under=narrow)):
        assert data(**arguments) == INVALID, arguments
        assert untouched(), arguments
    with pytest.raises(ValueError):
        labels.clump_members(0, [], 5)
    with pytest.raises(ValueError):
        labels.clump_members(3, [1, 1], 5)
    assert untouched()
    # in order: the count is cleared and the members arrive; key 77 is cell 77 of the first box
    assert data() == 0 and members() == 0
    ctx.synchronize()
    assert count.item() == 256 and totals.item() == 9 and (keys[256:] == 77).all()
    assert sorted(keys[:256].tolist()) == list(range(256))
    assert levels[:200].tolist() == [0] * 200 and (levels[200:] == 5).all()
    written = centres.view(-1)[:600].view(3, 200)                   # [3][n_members], packed
    assert written.tolist() == [[5.5 * 0.5] * 200, [1.5 * 0.5] * 200, [2.5 * 0.5] * 200]
    assert (centres.view(-1)[600:] == 6.0).all()
    assert (values[:200] == 1.0).all() and (values[200:] == 7.0).all()
    for scene in (labels, field, short, narrow, deep):
        scene.close()


# ---- avr_clump_pair_energy ------------------------------------------------------------------------------

def cloud(counts, seed, zero_masses=0.0):
    """Segments of distinct cell centres of two levels -- spacing 2^-7 where x < 1/2, 2^-6 beyond
    -- with masses in [0.5, 1.5), some of them zero.  Returns (offsets, x, y, z, m)."""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    xs = []
    for count in counts:
        fine = rng.choice(64 * 128 * 128, count // 2, replace=False)
        coarse = rng.choice(32 * 64 * 64, count - count // 2, replace=False)
        at = np.concatenate([
            (np.stack([fine % 64, fine // 64 % 128, fine // (64 * 128)]) + 0.5) / 128.0,
            (np.stack([coarse % 32 + 32, coarse // 32 % 64, coarse // (32 * 64)]) + 0.5) / 64.0],
            axis=1)
        xs.append(at[:, rng.permutation(count)])
    x, y, z = np.concatenate(xs + [np.zeros((3, 0))], axis=1)
    m = rng.random(x.size) + 0.5
    m[rng.random(x.size) < zero_masses] = 0.0
    return offsets, x, y, z, m


def run_pairs(ctx, offsets, x, y, z, m):
    device = [torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device) for a in (x, y, z, m)]
    w, depth = ctx.clump_pair_energy(offsets, *device)
    ctx.synchronize()
    return w.cpu().numpy(), depth


def check_pairs(ctx, counts, seed, zero_masses=0.0):
    offsets, x, y, z, m = cloud(counts, seed, zero_masses)
    got, depth = run_pairs(ctx, offsets, x, y, z, m)
    want = br.segment_energies(x, y, z, m, offsets)
    n = np.diff(offsets)
    assert depth.dtype == np.int64 and (depth <= n + 64).all() and (depth[n < 2] == 0).all()
    assert (depth[n >= 2] >= 2).all()
    bound = (depth + 8) * U * want + 8 * U * want
    worst = np.abs(got - want)[n >= 2] / bound[n >= 2]
    print("segments", len(counts), "largest error / bound:", float(worst.max()) if worst.size else 0.0)
    assert (np.abs(got - want) <= bound).all()
    assert (got[n < 2] == 0.0).all() and not np.signbit(got[n < 2]).any()
    again, _ = run_pairs(ctx, offsets, x, y, z, m)
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))      # equal bits
    return got, want


def test_segments_around_a_tile_with_empty_ones_between(ctx):
    got, want = check_pairs(ctx, [0, 1, 2, 255, 0, 0, 256, 257, 513, 1, 0], 61)
    assert (want[[2, 3, 6, 7, 8]] > 0.0).all()
    check_pairs(ctx, [2], 62)
    check_pairs(ctx, [1], 63)
    check_pairs(ctx, [0, 0], 64)


def test_one_segment_of_seventeen_tiles(ctx):
    check_pairs(ctx, [4099], 65)


def test_three_hundred_small_segments_and_zero_masses(ctx):
    rng = np.random.default_rng(66)
    check_pairs(ctx, rng.integers(1, 71, 300).tolist(), 67)
    got, want = check_pairs(ctx, [5, 300, 64], 68, zero_masses=0.3)
    offsets, x, y, z, m = cloud([40], 69)
    none, _ = run_pairs(ctx, offsets, x, y, z, np.zeros_like(m))
    assert none.tolist() == [0.0]


def test_two_cells_by_bits_and_the_numpy_twin(ctx):
    two = ([0.0, 3.0], [1.0, 5.0], [2.0, 14.0], [0.7, 1.9])
    got, depth = run_pairs(ctx, [0, 2], *(np.array(a) for a in two))
    assert got.tolist() == [0.7 * 1.9 / 13.0] and depth.tolist() == [2 + 8 + 3 + 1 + 6]
    offsets, x, y, z, m = cloud([3, 0, 130], 70)
    got, _ = run_pairs(ctx, offsets, x, y, z, m)
    twin = clumps.pair_energy(x, y, z, m, offsets)
    assert (np.abs(got - twin) <= (np.diff(offsets) + 64 + 16) * U * twin).all()


def test_wrong_pair_arguments_are_refused_and_the_outputs_untouched(ctx):
    device = ctx.device
    x = torch.rand(64, dtype=torch.float64, device=device)
    w = torch.full((4,), 7.0, dtype=torch.float64, device=device)
    depth = np.full(4, 33, dtype=np.int64)
    pointer = lambda t, given=True: C.c_void_p(t.data_ptr()) if given else None

    def call(offsets, n_segments=None, with_offsets=True, with_x=True, with_m=True, with_w=True):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n_segments = offsets.size - 1 if n_segments is None else n_segments
        return _capi.lib().avr_clump_pair_energy(
            ctx._handle, offsets.ctypes.data_as(C.POINTER(C.c_int64)) if with_offsets else None,
            n_segments, pointer(x, with_x), pointer(x), pointer(x), pointer(x, with_m),
            pointer(w, with_w), depth.ctypes.data_as(C.POINTER(C.c_int64)))

    def untouched():
        ctx.synchronize()
        return bool((w == 7.0).all()) and (depth == 33).all()

    most = 2 ** 22
    wrong = [dict(offsets=[1, 5]), dict(offsets=[0, 9, 8]), dict(offsets=[0, -1]),
             dict(offsets=[0, most + 1]),                      # a segment past 2^22: no cell is read
             dict(offsets=np.arange(513) * most),             # 2^31 members, from offsets alone
             dict(offsets=np.arange(33) * most),              # 2^26 items, from offsets alone
             dict(offsets=[0, 8], with_offsets=False), dict(offsets=[0, 8], with_x=False),
             dict(offsets=[0, 8], with_m=False), dict(offsets=[0, 8], with_w=False)]
    for arguments in wrong:
        assert call(**arguments) == INVALID, arguments
        assert untouched(), arguments
    for bad in ([1, 2], [0, 3, 2]):
        with pytest.raises(ValueError, match="ascend"):
            ctx.clump_pair_energy(bad, x[:2], x[:2], x[:2], x[:2])
    with pytest.raises(ValueError):
        ctx.clump_pair_energy([0, 9], x[:8], x[:8], x[:8], x[:8])
    assert untouched()
    # no segment: nothing is launched, and no array is needed
    assert call([0]) == 0 and untouched()
    none, no_depth = ctx.clump_pair_energy([0], x[:0], x[:0], x[:0], x[:0])
    assert none.shape == (0,) and no_depth.shape == (0,)
    # in order: W and depth are written for the segments the call names
    assert call([0, 0, 20, 21]) == 0
    ctx.synchronize()
    assert w[0].item() == 0.0 and w[1].item() > 0.0 and w[2].item() == 0.0 and w[3].item() == 7.0
    assert depth.tolist() == [0, 20 + 18, 0, 33]


# ---- end to end: api.clumps and api.clump_tree with a mass field -----------------------------------------

def reference_binding(case, labels, n, cells, min_cells, max_cells, mass, velocity, thermal):
    """Per clump of a reference label field what clump_binding_scene returns, with G left out: W,
    M, K, T, excluded, evaluated, nonfinite, and per clump how far a device value may lie from
    each (w_tol per unit of G)."""
    wanted, offsets = clumps.binding_segments(cells, min_cells, max_cells)
    names = [mass] + list(velocity or []) + ([thermal] if thermal else [])
    components = tuple(sorted({VARIABLES.index(name) for name in names}))
    found = br.members(labels, n, wanted, case.levels, case.ratio, case.scene_boxes(), case.lo,
                       case.sizes(), components)
    out = {key: np.full(n, np.nan) for key in ("W", "M", "K", "T", "w_tol", "m_tol", "k_tol", "t_tol")}
    out.update(evaluated=wanted, excluded=np.zeros(n, dtype=np.int64), nonfinite=0)
    value = lambda name, cut: found["values"][VARIABLES.index(name)][cut]
    for s, c in enumerate(np.nonzero(wanted)[0]):
        cut = slice(int(offsets[s]), int(offsets[s + 1]))
        one = br.binding(found["level"][cut], value(mass, cut), case.volumes(),
                         None if velocity is None else [value(v, cut) for v in velocity],
                         value(thermal, cut) if thermal else None)
        x, y, z = found["centres"][cut].T
        count = cut.stop - cut.start
        out["W"][c] = br.self_energy(x, y, z, one["m"])
        out["w_tol"][c] = (count + 64 + 8 + 8) * U * out["W"][c]
        out["M"][c], out["K"][c], out["T"][c] = one["M"], one["K"], one["T"]
        out["m_tol"][c] = (count - 1) * U * one["abs_M"]
        out["k_tol"][c] = one["k_tolerance"]
        out["t_tol"][c] = (count - 1) * U * one["abs_T"]
        out["excluded"][c] = one["excluded"]
        out["nonfinite"] += one["nonfinite"]
    return out


def choose_G(wants):
    """A constant for which no evaluated clump's G W lies within its tolerance of K + T, from the
    reference alone: the middle of the widest gap between the clumps' (K + T) / W, so that some
    are bound and some are not.  The margin is asserted."""
    with np.errstate(all="ignore"):                                 # NaNs where nothing was evaluated
        ratio = np.concatenate([((w["K"] + w["T"]) / w["W"])[w["evaluated"] & (w["W"] > 0.0)]
                                for w in wants])
    ratio = np.sort(ratio[ratio > 0.0])
    assert ratio.size > 6
    inner = ratio[ratio.size // 4: -(ratio.size // 4)]
    at = int(np.argmax(inner[1:] / inner[:-1]))
    G = float(math.sqrt(inner[at] * inner[at + 1]))
    for w in wants:
        e = w["evaluated"]
        margin = np.abs(G * w["W"][e] - (w["K"][e] + w["T"][e]))
        allowed = G * w["w_tol"][e] + w["k_tol"][e] + w["t_tol"][e] + \
            4 * U * (G * w["W"][e] + np.abs(w["K"][e]) + np.abs(w["T"][e]))
        # a clump without mass has W = K = T = 0 on both sides, exactly: not bound
        massless = (w["W"][e] == 0.0) & (w["K"][e] + w["T"][e] == 0.0)
        assert ((margin > 4 * allowed) | massless).all()
    return G


def assert_binding(got, want, G, nodes=slice(None)):
    e = want["evaluated"]
    assert np.array_equal(got["evaluated"][nodes], e)
    assert np.array_equal(got["excluded"][nodes], want["excluded"])
    # besides the tolerance: the reference's own rounding (M, T: one, as the tables'), the product
    # with G on both sides (W: two); K's tolerance holds its own
    for key, ours, tolerance, scale, own in (
            ("mass", "M", "m_tol", 1.0, 1), ("self_energy", "W", "w_tol", G, 2),
            ("kinetic", "K", "k_tol", 1.0, 0), ("thermal", "T", "t_tol", 1.0, 1)):
        mine = got[key][nodes]
        assert np.isnan(mine[~e]).all() and np.isfinite(mine[e]).all(), key
        error = np.abs(mine[e] - scale * want[ours][e])
        allowed = scale * want[tolerance][e] + own * U * np.abs(scale * want[ours][e])
        print(key, "largest error / bound:",
              float((error / np.maximum(allowed, 1e-300)).max()) if error.size else 0.0)
        assert (error <= allowed).all(), (key, float((error / np.maximum(allowed, 1e-300)).max()))
    bound = np.where(e, G * want["W"] > want["K"] + want["T"], True)
    assert np.array_equal(got["bound"][nodes], bound)
    return bound


def test_api_clumps_with_mass_velocity_and_thermal(three):
    labels, n, cells = reference_clumps(three, "u", 0.5)
    # the third velocity is not finite exactly where the mass is not: such members are excluded,
    # and their velocity must not reach K
    velocity = ("u", "whole", "odd")
    want = reference_binding(three, labels, n, cells, 1, 100, "odd", velocity, "odd")
    assert np.isfinite(want["K"][want["evaluated"]]).all()
    assert 5 < want["evaluated"].sum() < n and want["excluded"].sum() > 0 and want["nonfinite"] > 0
    assert (cells > 100).any()                                      # an envelope goes unevaluated
    G = choose_G([want])
    plain = api.clumps(three.path, "u", 0.5, fields=["odd"])
    got = api.clumps(three.path, "u", 0.5, fields=["odd"], mass="odd", velocity=velocity,
                     thermal="odd", G=G, max_cells=100)
    bound = assert_binding(got, want, G)
    assert bound[want["evaluated"]].any() and not bound[want["evaluated"]].all()
    assert got["nonfinite"] == plain["nonfinite"] + want["nonfinite"]
    for key in ("n", "cells_by_level", "cells", "volume", "outside"):
        assert np.array_equal(got[key], plain[key])
    # a derived mass, no velocities, no thermal energy: K = T = 0 and every evaluated clump binds
    api.add_field("heavy", "abs(u)")
    bare = api.clumps(three.path, "u", 0.5, mass="heavy", max_cells=100)
    e = want["evaluated"]
    assert np.array_equal(bare["evaluated"], e) and bare["bound"].all()
    assert (bare["kinetic"][e] == 0.0).all() and (bare["thermal"][e] == 0.0).all()
    assert (bare["excluded"] == 0).all() and (bare["mass"][e] > 0.0).all()
    assert (bare["self_energy"][e] > 0.0).all() and np.isnan(bare["self_energy"][~e]).all()


def literal_collapse(parent, cells, min_cells, passes):
    n = len(parent)
    valid = []
    for v in range(n):
        valid.append(bool(cells[v] >= min_cells and passes[v] and
                          (parent[v] == -1 or valid[parent[v]])))
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


def same(a, b):
    if isinstance(a, dict):
        return list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and any(isinstance(v, (np.ndarray, dict)) for v in a):
        return len(a) == len(b) and all(same(v, w) for v, w in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return ref.same_bits(a, b) if a.dtype.kind == "f" else bool(np.array_equal(a, b))


def test_api_clump_tree_with_mass_collapses_with_the_verdicts(ctx, three, tmp_path):
    thresholds, min_cells, max_cells = (0.4, 0.6, 0.75), 2, 100
    tree = tr.clump_tree(three.levels, three.ratio, VARIABLES.index("u"), thresholds, INF,
                         three.scene_boxes())
    velocity = ("whole", "u", "whole")
    wants, at = [], 0
    for step, count in enumerate(tree["counts"]):
        cells = tree["cells_by_level"][:, at:at + count].sum(axis=0)
        wants.append(reference_binding(three, tree["labels"][step], count, cells, min_cells,
                                       max_cells, "odd", velocity, None))
        at += count
    roots = slice(0, tree["counts"][0])
    assert not wants[0]["evaluated"][np.argmax(tree["cells_by_level"].sum(axis=0)[roots])]
    G = choose_G(wants)

    def products():
        out = str(tmp_path / "frame.ppm")
        assert api.run(three.path, api.RenderOptions(width=96, height=64, output_filename=out),
                       "u", ctx) == 0
        with open(out, "rb") as fh:
            frame = fh.read()
        plain = api.clump_tree(three.path, "u", thresholds, min_cells=min_cells)
        return frame, api.project_axis(three.path, "z", "u", None, 53, 41), plain

    before = products()
    got = api.clump_tree(three.path, "u", thresholds, min_cells=min_cells, mass="odd",
                         velocity=velocity, G=G, max_cells=max_cells)
    after = products()
    assert before[0] == after[0]
    assert same(before[1], after[1]) and same(before[2], after[2])
    assert not {"bound", "evaluated", "mass"} & set(before[2])
    assert np.array_equal(got["parent"], tree["parent"]) and got["n"] == sum(tree["counts"])
    bound, at = [], 0
    for want, count in zip(wants, tree["counts"]):
        bound.append(assert_binding(got, want, G, slice(at, at + count)))
        at += count
    bound = np.concatenate(bound)
    assert not bound.all() and bound[~got["evaluated"]].all()
    assert (got["thermal"][got["evaluated"]] == 0.0).all()
    kept, kept_parent, leaves = literal_collapse(tree["parent"].tolist(), got["cells"].tolist(),
                                                 min_cells, bound.tolist())
    assert got["kept"].tolist() == kept and got["kept_parent"].tolist() == kept_parent
    assert got["leaves"].tolist() == leaves
    unbound = ~bound & (got["cells"] >= min_cells)
    assert unbound.any() and not got["kept"][unbound].any()         # the verdicts reach the tree
