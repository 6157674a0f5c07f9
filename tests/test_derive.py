"""Derived fields without a GPU: the compiler (api.compile_expression), its numpy twin
(api.evaluate_program) against the eval reference (derive_reference) bit for bit, the registry and
the plotfile-level loader."""
import types

import numpy as np
import pytest

from amrvolumerenderer_amd import api, derive
from amrvolumerenderer_amd import plotfile as pf

import derive_reference as ref


@pytest.fixture(autouse=True)
def _empty_registry():
    for name in list(api.derived_fields()):
        api.remove_field(name)
    yield
    for name in list(api.derived_fields()):
        api.remove_field(name)


# ---- compiler --------------------------------------------------------------------------------------

def test_postfix_order_field_order_and_constant_sharing():
    p = api.compile_expression("0.5 * density * (u**2 + field('z-vel')**2) - 0.5 + 2 + 2.0")
    assert p.fields == ("density", "u", "z-vel")
    assert p.listing() == [
        ("CONST", 0), ("FIELD", 0), ("MUL", 0), ("FIELD", 1), ("SQUARE", 0), ("FIELD", 2),
        ("SQUARE", 0), ("ADD", 0), ("MUL", 0), ("CONST", 0), ("SUB", 0), ("CONST", 1), ("ADD", 0),
        ("CONST", 1), ("ADD", 0)]
    assert p.instructions.dtype == np.uint32 and p.constants.dtype == np.float64
    assert p.constants.tolist() == [0.5, 2.0]
    # 0.0 and -0.0 differ in bits; unary minus is an instruction, unary plus is none
    q = api.compile_expression("0.0 + -0.0 + +x")
    assert q.listing() == [("CONST", 0), ("CONST", 0), ("NEG", 0), ("ADD", 0), ("BUILTIN", 0),
                           ("ADD", 0)]
    assert q.fields == ()
    w = api.compile_expression("where(a <= b, minimum(a, b), maximum(sqrt(a), abs(level)))")
    assert [n for n, _ in w.listing()] == ["FIELD", "FIELD", "LE", "FIELD", "FIELD", "MIN", "FIELD",
                                           "SQRT", "BUILTIN", "ABS", "MAX", "WHERE"]
    assert [k for n, k in w.listing() if n == "BUILTIN"] == [7]


@pytest.mark.parametrize("text, piece", [
    ("a.real", "a.real"), ("a[0]", "a[0]"), ("lambda: 1", "lambda"), ("log(a)", "log(a)"),
    ("a ** 3", "a ** 3"), ("a ** b", "a ** b"), ("a ** 2.0", "a ** 2.0"), ("a < b < c", "a < b < c"),
    ("a if b else c", "a if b else c"), ("a and b", "a and b"), ("not a", "not a"),
    ("a % b", "a % b"), ("a // b", "a // b"), ("'text'", "'text'"), ("True", "True"),
    ("sqrt", "sqrt"), ("sqrt(a, b)", "sqrt(a, b)"), ("where(a, b)", "where(a, b)"),
    ("field(a)", "field(a)"), ("abs(a=1)", "abs(a=1)"), ("a is b", "a is b"), ("[a]", "[a]"),
    ("__import__('os')", "__import__"),
])
def test_everything_else_is_refused_by_name(text, piece):
    with pytest.raises(ValueError, match=None) as error:
        api.compile_expression(text)
    assert piece in str(error.value)


def test_not_an_expression():
    for text in ("", "   ", "a = 1", "a +", None, 3):
        with pytest.raises(ValueError):
            api.compile_expression(text)


def _sum(names):
    return " + ".join(names)


def test_each_limit_passes_and_one_more_is_refused():
    fields = [f"f{i}" for i in range(7)]
    assert len(api.compile_expression(_sum(fields[:6])).fields) == 6
    with pytest.raises(ValueError, match="more than 6 fields"):
        api.compile_expression(_sum(fields))
    # a + a + ... : n operands are 2 n - 1 instructions; -(...) makes the count even
    assert len(api.compile_expression("-(" + _sum(["a"] * 32) + ")").instructions) == 64
    with pytest.raises(ValueError, match="more than 64 instructions"):
        api.compile_expression("-(" + _sum(["a"] * 32) + ") + a")
    constants = [f"{i}.5" for i in range(17)]
    assert len(api.compile_expression(_sum(constants[:16])).constants) == 16
    assert len(api.compile_expression(_sum(constants[:16] + ["3.5", "0.5"])).constants) == 16
    with pytest.raises(ValueError, match="more than 16 constants"):
        api.compile_expression(_sum(constants))

    def nest(depth):
        return "a" if depth == 1 else f"a + ({nest(depth - 1)})"
    assert len(api.compile_expression(nest(8)).instructions) == 15
    with pytest.raises(ValueError, match="deeper than 8"):
        api.compile_expression(nest(9))
    assert len(api.compile_expression(ref.TEXTS["full"]).instructions) == 64
    full = api.compile_expression(ref.TEXTS["full"])
    assert len(full.fields) == 6 and len(full.constants) == 16


def test_registry_names_cycles_and_inlining():
    for name in ("x", "level", "cell_volume", "cells", "sqrt", "where", "field", "", None):
        with pytest.raises(ValueError):
            api.add_field(name, "density")
    with pytest.raises(ValueError):
        api.add_field("speed", "u +")
    assert api.derived_fields() == {}
    api.add_field("speed2", "u**2 + v**2")
    api.add_field("speed", "sqrt(speed2)")
    program = api.add_field("ke", "0.5 * density * speed ** 2")
    assert api.derived_fields() == {"speed2": "u**2 + v**2", "speed": "sqrt(speed2)",
                                    "ke": "0.5 * density * speed ** 2"}
    direct = api.compile_expression("0.5 * density * sqrt(u**2 + v**2) ** 2")
    assert program.fields == direct.fields == ("density", "u", "v")
    assert program.instructions.tolist() == direct.instructions.tolist()
    # compile_expression alone knows no registered names: speed is a stored field there
    assert api.compile_expression("speed").fields == ("speed",)
    with pytest.raises(ValueError, match="cycle"):
        api.add_field("speed2", "ke + 1")
    with pytest.raises(ValueError, match="cycle"):
        api.add_field("self", "self + 1")
    assert "self" not in api.derived_fields() and api.derived_fields()["speed2"] == "u**2 + v**2"
    # the limits apply to the inlined program
    api.add_field("six", _sum([f"f{i}" for i in range(6)]))
    with pytest.raises(ValueError, match="more than 6 fields"):
        api.add_field("seven", "six + g")
    api.add_field("minus-one", "0 - 1")           # not an identifier: reachable through field()
    assert api.add_field("uses", "field('minus-one') * u").fields == ("u",)
    api.remove_field("uses")
    with pytest.raises(KeyError):
        api.remove_field("uses")


# ---- evaluator -------------------------------------------------------------------------------------

def _arrays():
    rng = np.random.default_rng(11)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308,
                        1.0, -1.0, 1e308, -1e308, 3.0, -4.0, 0.1, 1e-200])
    n = special.size
    fields = {}
    for i, name in enumerate(ref.VARIABLES):
        column = np.roll(special, 3 * i + 1)
        grid = np.concatenate([np.repeat(special, n), np.tile(column, n),
                               rng.standard_normal(500) * 10.0 ** rng.integers(-3, 4, 500)])
        fields[name] = rng.permutation(grid) if i > 1 else grid
    fields["u"][: n * n] = np.repeat(special, n)      # every pair of specials in (u, v)
    fields["v"][: n * n] = np.tile(special, n)
    size = fields["u"].size
    builtins = {"x": rng.standard_normal(size), "y": rng.standard_normal(size),
                "z": rng.standard_normal(size), "dx": 0.125, "dy": 0.25, "dz": 0.5,
                "cell_volume": (0.125 * 0.25) * 0.5, "level": 2.0}
    return fields, builtins, size


def test_the_texts_use_every_opcode_and_reach_depth_eight():
    used, deepest = set(), 0
    for text in ref.TEXTS.values():
        program = api.compile_expression(text)
        depth = 0
        for name, _ in program.listing():
            used.add(name)
            depth += 1 - {"CONST": 0, "FIELD": 0, "BUILTIN": 0, "NEG": 1, "SQUARE": 1, "SQRT": 1,
                          "ABS": 1, "WHERE": 3}.get(name, 2)
            deepest = max(deepest, depth)
        assert depth == 1
    assert used == set(derive.OP_NAMES) and deepest == 8


@pytest.mark.parametrize("name", sorted(ref.TEXTS))
def test_the_interpreter_equals_the_eval_reference_bit_for_bit(name):
    fields, builtins, size = _arrays()
    text = ref.TEXTS[name]
    program = api.compile_expression(text)
    got = api.evaluate_program(program, [fields[f] for f in program.fields], builtins)
    want = ref.evaluate(text, fields, builtins, (size,))
    assert got.shape == want.shape == (size,) and got.dtype == np.float64
    assert ref.same_bits(got, want)
    if name in ("velocity_magnitude", "mach", "nan_condition"):
        assert np.isnan(want).any() and np.isfinite(want).any()
    if name == "denormal":
        assert (want[np.isfinite(fields["u"]) & ~np.isnan(fields["density"])] == 1e-323).all()
    if name == "compare":      # NaN: only != holds
        both = np.isnan(fields["u"]) | np.isnan(fields["v"])
        assert (want[both] == 32.0).all() and set(np.unique(want)) == {32.0 + 1 + 2, 32.0 + 4 + 8,
                                                                        2.0 + 8 + 16, 32.0}


def test_negative_sqrt_signed_zero_and_nan_selection():
    a = np.array([-1.0, -0.0, 0.0, 4.0, np.nan])
    b = np.array([1.0, 0.0, -0.0, np.nan, 2.0])
    run = lambda t: api.evaluate_program(api.compile_expression(t), [a, b][:len(
        api.compile_expression(t).fields)], {})
    root = run("sqrt(a)")
    assert np.isnan(root[0]) and np.signbit(root[1]) and root[3] == 2.0
    low, high = run("minimum(a, b)"), run("maximum(a, b)")
    assert low.tolist()[:3] == [-1.0, 0.0, -0.0] and np.signbit(low[2]) and not np.signbit(low[1])
    assert np.isnan(low[3]) and np.isnan(low[4])       # b NaN: b; a NaN: a
    assert np.isnan(high[3]) and np.isnan(high[4]) and high[0] == 1.0
    assert run("where(a, 1, 2)").tolist() == [1.0, 2.0, 2.0, 1.0, 1.0]


# ---- loader ----------------------------------------------------------------------------------------

def test_stored_names_reach_the_plotfile_loader_unchanged(monkeypatch, tmp_path):
    calls = []

    class Stop(Exception):
        pass

    def loader(*args, **kwargs):
        calls.append((args, kwargs))
        raise Stop

    monkeypatch.setattr(pf, "load_plotfile_geometry", loader)
    ctx, group = object(), object()
    path = str(tmp_path / "plt")
    with pytest.raises(Stop):
        api.compute_histogram(path, "density", 1, 2, True, 16, ctx, 3, 4, group)
    with pytest.raises(Stop):
        api.run(path, api.RenderOptions(min_level=1, max_level=2, log_scale_input=True,
                                        scalar_range=(1.0, 2.0)), "u", ctx, 3, 4, group)
    with pytest.raises(Stop):
        api.run(path, api.RenderOptions(), "", ctx)
    assert calls == [((ctx, path, "density", 1, 2, True, True, 3, 4, group), {}),
                     ((ctx, path, "u", 1, 2, True, False, 3, 4, group), {}),
                     ((ctx, path, "", 0, -1, False, True, 0, 1, None), {})]
    # a registered field that the call does not name changes nothing
    api.add_field("speed", "sqrt(u**2 + v**2)")
    with pytest.raises(Stop):
        api.compute_histogram(path, "density", 1, 2, True, 16, ctx, 3, 4, group)
    assert calls[3] == calls[0]
    # ... and one that it names loads the stored fields raw, each once
    del calls[:]
    scenes = {}

    def stored(ctx_, path_, name, *rest):
        calls.append((name,) + rest)
        scenes[name] = types.SimpleNamespace(all_boxes=[types.SimpleNamespace(level=0)])
        return scenes[name]

    monkeypatch.setattr(pf, "load_plotfile_geometry", stored)
    monkeypatch.setattr(pf, "PlotFileData", lambda p: type("H", (), {
        "var_names": ["density", "u", "v"], "cell_size": [(1.0, 1.0, 1.0)]})())
    derived = []
    monkeypatch.setattr(api, "derive_scene", lambda *a: derived.append(a) or "derived")
    api.add_field("ke", "density * speed ** 2 + u")
    got = api._load_variable_scenes(ctx, path, ["speed", "u", "ke"], 1, 2, True, False, 3, 4, group)
    assert got == ["derived", scenes["u"], "derived"]
    assert calls == [("u", 1, 2, False, True, 3, 4, group), ("v", 1, 2, False, True, 3, 4, group),
                     ("u", 1, 2, True, False, 3, 4, group),
                     ("density", 1, 2, False, True, 3, 4, group)]
    assert [d[1].fields for d in derived] == [("u", "v"), ("density", "u", "v")]
    assert derived[0][8:] == (True, False) and derived[0][5:8] == (3, 4, group)
    api.add_field("needs", "density * missing")
    with pytest.raises(RuntimeError, match="'missing' .needed by derived field 'needs'. not found"):
        api._load_variable_scenes(ctx, path, ["needs"], 0, -1, False, True, 0, 1, None)
