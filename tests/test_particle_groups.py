"""Particle groups without a GPU: the numpy reference (particle_group_reference) against groupings
that are known by hand -- a chain spaced exactly one linking length on dyadic coordinates, the same
chain with one gap an ulp wider, blobs around min_members, the numbering under a permutation, pairs
linked only across a periodic face, edge and corner, what is outside, coincident points --, the
refusals of api.particle_groups that come before any device work, the host-side helpers (the grid
that is chosen, the member lists, the catalogue), api.linking_length, and the declarations of the
two native entries."""
import math
import os

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, groups

import particle_group_reference as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 0.125


def chain(gap_after=None):
    """Five points spaced exactly B along x from 1.0 on (all dyadic: the differences are exact and
    d2 == b2); with gap_after = i the points from i + 1 on lie one ulp further."""
    x = 1.0 + B * np.arange(5)
    if gap_after is not None:
        x[gap_after + 1:] = np.nextafter(x[gap_after + 1:], np.inf)
    return np.stack([x, np.full(5, 0.5), np.full(5, 0.25)], axis=1)


# ---- the reference ---------------------------------------------------------------------------------

def test_a_chain_spaced_exactly_one_linking_length_is_one_group():
    got = pg.groups(chain(), B, (0, 0, 0), (2, 1, 1))
    assert got["count"] == 1 and got["labels"].tolist() == [1] * 5
    assert got["first"].tolist() == [0] and got["offsets"].tolist() == [0, 5]
    assert got["members"].tolist() == [0, 1, 2, 3, 4] and got["outside"] == 0


def test_a_gap_one_ulp_wider_splits_the_chain_there():
    points = chain(gap_after=2)
    # the gap 2 -> 3 is B + ulp(1.375) > B, every other gap is still exactly B
    assert points[3, 0] - points[2, 0] > B and points[4, 0] - points[3, 0] == B
    got = pg.groups(points, B, (0, 0, 0), (2, 1, 1))
    assert got["count"] == 2 and got["labels"].tolist() == [1, 1, 1, 2, 2]
    assert got["first"].tolist() == [0, 3] and got["offsets"].tolist() == [0, 3, 5]


def test_min_members_just_above_and_below_the_blobs():
    rng = np.random.default_rng(5)
    small = 0.25 + 0.01 * rng.random((7, 3))
    large = 0.75 + 0.01 * rng.random((12, 3))
    points = np.concatenate([small, large])
    for least, want in ((7, [1] * 7 + [2] * 12), (8, [0] * 7 + [1] * 12), (12, [0] * 7 + [1] * 12),
                        (13, [0] * 19)):
        got = pg.groups(points, 0.05, min_members=least)
        assert got["labels"].tolist() == want and got["count"] == max(want)


def test_numbering_follows_the_smallest_index_under_a_permutation():
    rng = np.random.default_rng(6)
    centres = np.array([[0.2, 0.2, 0.2], [0.5, 0.5, 0.5], [0.8, 0.8, 0.8]])
    points = np.concatenate([c + 0.01 * rng.random((5, 3)) for c in centres])
    plain = pg.groups(points, 0.05)
    assert plain["labels"].tolist() == [1] * 5 + [2] * 5 + [3] * 5
    order = rng.permutation(15)
    shuffled = pg.groups(points[order], 0.05)
    blob = order // 5                               # the blob of each shuffled particle
    ranks = {b: r + 1 for r, b in enumerate(sorted(range(3), key=lambda b: np.nonzero(blob == b)[0][0]))}
    assert shuffled["labels"].tolist() == [ranks[b] for b in blob]
    assert shuffled["first"].tolist() == sorted(int(np.nonzero(blob == b)[0][0]) for b in range(3))
    for g in range(3):
        part = shuffled["members"][shuffled["offsets"][g]:shuffled["offsets"][g + 1]]
        assert part.tolist() == sorted(part.tolist()) and part[0] == shuffled["first"][g]


@pytest.mark.parametrize("axes", [(0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2)])
def test_a_pair_linked_only_through_the_periodic_wrap(axes):
    p, q = np.full(3, 0.5), np.full(3, 0.5)
    for d in axes:
        p[d], q[d] = 0.015625, 1.0 - 0.015625       # 1/32 apart through the face
    points = np.stack([p, q])
    flags = [d in axes for d in range(3)]
    b = 0.0625
    assert pg.groups(points, b, periodic=flags)["labels"].tolist() == [1, 1]
    assert pg.groups(points, b, periodic=False)["labels"].tolist() == [1, 2]
    for d in axes:                                  # every wrapped axis is needed
        fewer = [f and e != d for e, f in enumerate(flags)]
        assert pg.groups(points, b, periodic=fewer)["labels"].tolist() == [1, 2]


def test_nan_infinite_and_out_of_period_positions_are_outside():
    points = np.array([[0.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf],
                       [0.51, 0.5, 0.5], [1.0, 0.5, 0.5], [-0.01, 0.5, 0.5], [0.5, 1.5, 0.5]])
    got = pg.groups(points, 0.05, periodic=(True, False, False))
    # x = hi and x < lo are outside on the periodic axis; y = 1.5 is beyond a plain face: inside
    assert got["labels"].tolist() == [1, 0, 0, 0, 1, 0, 0, 2] and got["outside"] == 5
    assert got["root"].tolist() == [0, -1, -1, -1, 0, -1, -1, 7]
    got = pg.groups(points, 0.05)
    assert got["labels"].tolist() == [1, 0, 0, 0, 1, 2, 3, 4] and got["outside"] == 3


def test_coincident_points_are_linked():
    points = np.tile([[0.3, 0.6, 0.9]], (6, 1))
    got = pg.groups(points, 1e-300)
    assert got["count"] == 1 and got["labels"].tolist() == [1] * 6


def test_pair_tests_counts_the_pairs_of_the_same_and_adjacent_cells():
    points = np.array([[0.1, 0.1, 0.1], [0.15, 0.1, 0.1], [0.4, 0.1, 0.1], [0.9, 0.1, 0.1],
                       [np.nan, 0.0, 0.0]])
    # cells along x with dims 4: 0, 0, 1, 3
    assert pg.pair_tests(points, (0, 0, 0), (1, 1, 1), (4, 1, 1)) == 3
    assert pg.pair_tests(points, (0, 0, 0), (1, 1, 1), (4, 3, 3), (True, True, True)) == 5
    assert pg.pair_tests(points, (0, 0, 0), (1, 1, 1), (1, 1, 1)) == 6


# ---- the host side of the api ------------------------------------------------------------------------

def test_group_pair_tests_equals_the_pair_by_pair_count():
    import torch
    from amrvolumerenderer_amd import runtime
    rng = np.random.default_rng(11)
    points = rng.random((300, 3))
    for dims, flags in (((5, 4, 3), (False, False, False)), ((5, 4, 3), (True, False, True)),
                        ((3, 3, 3), (True, True, True)), ((1, 7, 1), (False, False, False)),
                        ((2, 2, 2), (False, False, False)), ((1, 1, 1), (False, False, False))):
        cells = pg.cell_of(points, (0, 0, 0), (1, 1, 1), dims)
        flat = (cells[:, 2] * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]
        counts = np.bincount(flat, minlength=int(np.prod(dims))).reshape(dims[2], dims[1], dims[0])
        got = runtime.group_pair_tests(torch.from_numpy(counts), flags)
        assert got == pg.pair_tests(points, (0, 0, 0), (1, 1, 1), dims, flags), (dims, flags)


def test_the_chosen_grid_keeps_the_rule_and_about_four_cells_a_particle():
    slack = 1.0 + 2.0 ** -10
    for n, b, lo, hi, flags in ((1000, 0.01, (0, 0, 0), (1, 1, 1), (False,) * 3),
                                (10, 1e-6, (0, 0, 0), (1, 2, 3), (True,) * 3),
                                (10 ** 8, 1e-4, (-1, -1, -1), (1, 1, 1), (False, True, False)),
                                (0, 0.3, (0, 0, 0), (1, 1, 1), (True, False, False)),
                                (5, 2.0, (0, 0, 0), (1, 1, 1), (False,) * 3)):
        dims = groups.choose_dims(n, b, np.array(lo, float), np.array(hi, float), flags)
        cells = dims[0] * dims[1] * dims[2]
        assert cells < 2 ** 27 and all(1 <= m <= 1024 for m in dims)
        assert cells <= max(4 * n, 27)
        for d in range(3):
            assert dims[d] == 1 or (hi[d] - lo[d]) / dims[d] >= b * slack
            assert not flags[d] or dims[d] >= 3
    assert groups.choose_dims(1000, 0.01, np.zeros(3), np.ones(3), (False,) * 3) == (15, 15, 15)
    with pytest.raises(ValueError, match="a third of the period"):
        groups.choose_dims(10, 0.34, np.zeros(3), np.ones(3), (True, False, False))


def test_member_lists_and_the_catalogue_by_hand():
    labels = np.array([2, 0, 1, 2, 1, 0, 2], dtype=np.int32)
    offsets, members, first = groups.member_lists(labels, 2)
    assert offsets.tolist() == [0, 2, 5] and members.tolist() == [2, 4, 0, 3, 6]
    assert first.tolist() == [2, 0]
    offsets0, members0, first0 = groups.member_lists(np.zeros(4, dtype=np.int32), 0)
    assert offsets0.tolist() == [0] and members0.size == 0 and first0.size == 0
    x = np.array([[1.0, 0.0, 0.0], [9.0, 9.0, 9.0], [0.25, 2.0, 4.0], [3.0, 0.0, 0.0],
                  [7.75, 4.0, 8.0], [9.0, 9.0, 9.0], [5.0, 0.0, 0.0]])
    m = np.array([1.0, 5.0, 3.0, 1.0, 1.0, 5.0, 2.0])
    v = np.array([[1.0, 0, 0], [0, 0, 0], [2.0, 0, 0], [1.0, 0, 0], [-2.0, 0, 0], [0, 0, 0],
                  [1.0, 0, 0]])
    lo, hi = np.zeros(3), np.full(3, 8.0)
    plain = groups.catalogue(x, m, v, offsets, members, lo, hi, (False,) * 3)
    assert plain["mass"].tolist() == [4.0, 4.0]
    assert plain["centre"].tolist() == [[(0.75 + 7.75) / 4, 2.5, 5.0], [3.5, 0.0, 0.0]]
    assert plain["velocity"].tolist() == [[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    assert plain["dispersion"].tolist() == [math.sqrt((3.0 + 9.0) / 12.0), 0.0]
    # group 1 across the periodic x face: offsets from x0 = 0.25 are 0 and -0.5
    wrapped = groups.catalogue(x, m, None, offsets, members, lo, hi, (True, False, False))
    assert wrapped["centre"][0].tolist() == [0.25 - 0.5 / 4, 2.5, 5.0]
    assert wrapped["centre"][1].tolist() == [3.5, 0.0, 0.0] and "velocity" not in wrapped
    # a centre below lo is wrapped into [lo, hi)
    members2 = np.array([2, 4])
    x2 = x.copy()
    x2[2, 0], x2[4, 0] = 0.0, 7.0
    got = groups.catalogue(x2, None, None, np.array([0, 2]), members2, lo, hi, (True,) * 3)
    assert got["centre"][0, 0] == 7.5 and got["mass"].tolist() == [2.0]


def test_linking_length():
    assert api.linking_length(8, 1.0) == 0.2 * 0.125 ** (1.0 / 3.0)
    assert api.linking_length(1000, 8.0, b=0.5) == 0.5 * (8.0 / 1000) ** (1.0 / 3.0)
    for bad in ((0, 1.0, 0.2), (10, 0.0, 0.2), (10, math.inf, 0.2), (10, 1.0, -1.0),
                (10, 1.0, math.nan)):
        with pytest.raises(ValueError):
            api.linking_length(*bad)


def test_the_refusals_come_before_any_device_work(monkeypatch, tmp_path):
    def untouched(*args, **kwargs):
        raise AssertionError("the runtime was touched")

    monkeypatch.setattr(api, "_runtime_scope", untouched)
    monkeypatch.setattr(api, "_ensure_runtime", untouched)
    points = np.zeros((4, 3))
    for arguments, message in (
            ((np.zeros((4, 2)), 0.1), r"positions must be \[n, 3\]"),
            ((np.zeros(12), 0.1), r"positions must be \[n, 3\]"),
            ((np.zeros((4, 3), dtype=complex), 0.1), "real numbers"),
            ((np.array([["a"] * 3]), 0.1), "real numbers"),
            ((points, 0.0), "finite positive"),
            ((points, -1.0), "finite positive"),
            ((points, math.nan), "finite positive"),
            ((points, math.inf), "finite positive"),
            ((points, "wide"), "finite positive")):
        with pytest.raises(ValueError, match=message):
            api.particle_groups(*arguments)
    for keywords, message in (
            ({"masses": np.ones(3)}, "one value per particle"),
            ({"masses": np.ones(4, dtype=complex)}, "real numbers"),
            ({"velocities": np.ones((4, 2))}, r"velocities must be \[n, 3\]"),
            ({"min_members": 0}, "min_members"),
            ({"min_members": 2.5}, "min_members"),
            ({"min_members": 2 ** 31}, "min_members"),
            ({"periodic": True}, "periodic needs a domain"),
            ({"periodic": (False, True, False)}, "periodic needs a domain"),
            ({"periodic": (True, True)}, "a flag or three"),
            ({"domain": ((0, 0), (1, 1))}, "domain must be"),
            ({"domain": ((0, 0, 0), (1, 0, 1))}, "finite with lo < hi"),
            ({"domain": ((0, 0, 0), (1, math.inf, 1))}, "finite with lo < hi"),
            ({"domain": ((0, 0, 0), (1, 1, 1)), "periodic": True}, "a third of the period"),
            ({"max_pair_tests": -1}, "max_pair_tests")):
        with pytest.raises(ValueError, match=message):
            api.particle_groups(points, 0.4, **keywords)
    # a plotfile's prob_lo and prob_hi are the domain: read, and then the runtime is asked for
    from amrvolumerenderer_amd import plotfile
    import gradient_reference as ref
    levels = ref.make_levels([((0, 0, 0), (3, 3, 3))], [[((0, 0, 0), (3, 3, 3))]], [], 5)
    path = str(tmp_path / "plt")
    plotfile.write_plotfile(path, list(ref.VARIABLES), levels, (0.0, 0.0, 0.0), (4.0, 4.0, 4.0), [])
    with pytest.raises(ValueError, match="a third of the period"):
        api.particle_groups(points, 1.4, domain=path, periodic=True)
    with pytest.raises(AssertionError, match="the runtime was touched"):
        api.particle_groups(points, 0.4, domain=path, periodic=True)
    with pytest.raises(AssertionError, match="the runtime was touched"):
        api.particle_groups(points, 0.4)


# ---- declarations ------------------------------------------------------------------------------------

def test_the_entries_are_declared_and_exported(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    assert "int avr_particle_group_cells(avr_context *ctx, const double *points_dev, " \
           "uint64_t n," in header
    assert "int avr_particle_groups(avr_context *ctx, const double *points_sorted_dev, " \
           "const int64_t *order_dev," in header
    for entry, count in (("avr_particle_group_cells", 10), ("avr_particle_groups", 16)):
        declared = header.split(f"int {entry}(")[1].split(");")[0]
        assert len(_capi.SIGNATURES[entry][1]) == declared.count(",") + 1 == count
        assert getattr(avr_lib, entry) is not None
    assert avr_lib.avr_abi_version() == 2
