"""The numpy reference of derived fields ("Derived fields"), independent of the
product's compiler: an expression text is evaluated with Python's eval in a namespace of numpy
arrays and numpy-backed sqrt, abs, where, minimum and maximum with the stated definitions
  where(c, a, b) = (c != 0) ? a : b       minimum(a, b) = (a < b || a != a) ? a : b
  comparisons give 1.0 or 0.0             maximum(a, b) = (a > b || a != a) ? a : b
It works on a plotfile's own level arrays; cell centres are prob_lo + (I + 0.5) * dx_l with I the
cell's global index at its level."""
import numpy as np

BUILTINS = ("x", "y", "z", "dx", "dy", "dz", "cell_volume", "level")


class Value:
    """A float64 array whose comparisons give 1.0 / 0.0 and whose arithmetic stays a Value."""

    def __init__(self, a):
        self.a = np.asarray(a.a if isinstance(a, Value) else a, dtype=np.float64)

    @staticmethod
    def of(v):
        return v.a if isinstance(v, Value) else np.float64(v)

    def _bin(self, other, f, swap=False):
        with np.errstate(all="ignore"):
            a, b = self.a, Value.of(other)
            return Value(f(b, a) if swap else f(a, b))

    def _cmp(self, other, f):
        return Value(np.where(f(self.a, Value.of(other)), np.float64(1.0), np.float64(0.0)))

    __add__ = lambda s, o: s._bin(o, np.add)
    __radd__ = lambda s, o: s._bin(o, np.add, True)
    __sub__ = lambda s, o: s._bin(o, np.subtract)
    __rsub__ = lambda s, o: s._bin(o, np.subtract, True)
    __mul__ = lambda s, o: s._bin(o, np.multiply)
    __rmul__ = lambda s, o: s._bin(o, np.multiply, True)
    __truediv__ = lambda s, o: s._bin(o, np.divide)
    __rtruediv__ = lambda s, o: s._bin(o, np.divide, True)
    __neg__ = lambda s: Value(-s.a)
    __pos__ = lambda s: s
    __lt__ = lambda s, o: s._cmp(o, np.less)
    __le__ = lambda s, o: s._cmp(o, np.less_equal)
    __gt__ = lambda s, o: s._cmp(o, np.greater)
    __ge__ = lambda s, o: s._cmp(o, np.greater_equal)
    __eq__ = lambda s, o: s._cmp(o, np.equal)
    __ne__ = lambda s, o: s._cmp(o, np.not_equal)
    __hash__ = None

    def __pow__(self, e):
        assert type(e) is int and e == 2
        with np.errstate(all="ignore"):
            return Value(self.a * self.a)


def _lift(v):
    return v if isinstance(v, Value) else Value(np.float64(v))


def _sqrt(a):
    with np.errstate(all="ignore"):
        return Value(np.sqrt(_lift(a).a))


def _abs(a):
    return Value(np.abs(_lift(a).a))


def _where(c, a, b):
    return Value(np.where(_lift(c).a != 0.0, _lift(a).a, _lift(b).a))


def _minimum(a, b):
    a, b = _lift(a).a, _lift(b).a
    return Value(np.where((a < b) | (a != a), a, b))


def _maximum(a, b):
    a, b = _lift(a).a, _lift(b).a
    return Value(np.where((a > b) | (a != a), a, b))


def evaluate(text, fields, builtins, shape):
    """text over fields (name -> array) and builtins (name -> array or scalar) -> float64 array
    of `shape`.  Numbers in the text are lifted, so that 1 < 2 is 1.0 here too."""
    namespace = {"__builtins__": {}, "sqrt": _sqrt, "abs": _abs, "where": _where,
                 "minimum": _minimum, "maximum": _maximum}
    names = {name: Value(a) for name, a in fields.items()}
    namespace["field"] = lambda name: names[name]
    namespace.update({k: v for k, v in names.items() if k.isidentifier()})
    namespace.update({k: Value(v) for k, v in builtins.items()})
    import ast

    class Lift(ast.NodeTransformer):          # every number literal becomes a Value
        def visit_Constant(self, node):
            if isinstance(node.value, (int, float)) and not isinstance(node.value, bool):
                return ast.copy_location(ast.Call(ast.Name("_num", ast.Load()), [node], []), node)
            return node

        def visit_BinOp(self, node):
            if isinstance(node.op, ast.Pow):  # the exponent stays an int
                node.left = self.visit(node.left)
                return node
            return self.generic_visit(node)

        def visit_Call(self, node):
            if isinstance(node.func, ast.Name) and node.func.id == "field":
                return node
            return self.generic_visit(node)

    namespace["_num"] = lambda v: Value(np.float64(v))
    tree = ast.fix_missing_locations(Lift().visit(ast.parse(text.strip(), mode="eval")))
    result = eval(compile(tree, "<expression>", "eval"), namespace)
    return np.array(np.broadcast_to(_lift(result).a, shape))


def cell_sizes(levels, prob_lo, prob_hi):
    """[(dx, dy, dz)] per level from the level domains, as write_plotfile derives them."""
    out = []
    for lev in levels:
        lo, hi = lev["domain"]
        out.append(tuple((prob_hi[a] - prob_lo[a]) / (hi[a] - lo[a] + 1) for a in range(3)))
    return out


def is_power_of_two(v):
    m, _ = np.frexp(abs(float(v)))
    return float(v) != 0.0 and m == 0.5


def grid_builtins(box, level, size, prob_lo):
    """The built-ins over one grid of a level: box = ((ilo, jlo, klo), (ihi, jhi, khi))."""
    lo, hi = box
    centre = [np.float64(prob_lo[a]) + (np.arange(lo[a], hi[a] + 1, dtype=np.float64) + 0.5)
              * np.float64(size[a]) for a in range(3)]
    dx, dy, dz = (np.float64(s) for s in size)
    return {"x": centre[0][None, None, :], "y": centre[1][None, :, None],
            "z": centre[2][:, None, None], "dx": dx, "dy": dy, "dz": dz,
            "cell_volume": (dx * dy) * dz, "level": np.float64(level)}


def evaluate_levels(text, levels, variables, prob_lo, prob_hi):
    """The expression over a plotfile's own level arrays: [[array per grid] per level]; levels as
    plotfile.write_plotfile takes them (data [ncomp, nz, ny, nx] per grid)."""
    sizes = cell_sizes(levels, prob_lo, prob_hi)
    out = []
    for level, lev in enumerate(levels):
        grids = []
        for box, data in zip(lev["boxes"], lev["data"]):
            data = np.asarray(data, dtype=np.float64)
            fields = {name: data[c] for c, name in enumerate(variables)}
            grids.append(evaluate(text, fields, grid_builtins(box, level, sizes[level], prob_lo),
                                  data.shape[1:]))
        out.append(grids)
    return out


def same_bits(a, b):
    """Equal by bits, NaN equal to NaN."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | both_nan).all())


# ---- the expressions both test files use -----------------------------------------------------------
# over the variables density, u, v, w, pressure, other: every opcode, and a stack of 8
def full_program_text():
    """6 fields, 64 instructions, 16 constants, depth 8."""
    text = "-(density + (u + (v + (w + (pressure + (other + (1.5 + 2.5)))))))"
    names = ("density", "u", "v", "w", "pressure", "other")
    for k in range(10):
        text = f"({text}) + {k + 3}.25 * {names[k % 6]}"
    for k in range(4):
        text = f"({text}) + {k + 20}.125"
    return text


TEXTS = {
    "velocity_magnitude": "sqrt(u**2 + v**2 + w**2)",
    "kinetic_energy": "0.5 * density * (u**2 + v**2 + w**2)",
    "mach": "sqrt(u**2 + v**2 + w**2) / sqrt(1.4 * pressure / density)",
    "radius": "sqrt((x - 0.75)**2 + (y + 0.375)**2 + (z - 2.5)**2)",
    "clamp": "where(density > 0, minimum(maximum(density, 1), 100), -abs(other))",
    "compare": "(u < v) + 2 * (u <= v) + 4 * (u > v) + 8 * (u >= v) + 16 * (u == v) + 32 * (u != v)",
    "subtract_divide": "+(density - other) / (u - w)",
    "nan_condition": "where(other, 1.0, 2.0) + minimum(other, u) - maximum(v, other)",
    "deep": "u + (v + (w + (density + (u * (v * (w * density))))))",
    "geometry": "cell_volume * density + level + dx + dy * 2 + dz * 4 + x + y + z",
    "denormal": "5e-324 * (density == density) + 5e-324 + 0.0 * u",
    "quoted": 'field("density") * field("other") - density',
    "constant": "1.0",
    "full": full_program_text(),
}
VARIABLES = ("density", "u", "v", "w", "pressure", "other")
