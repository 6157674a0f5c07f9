"""Derived fields ("Derived fields"): per-cell expressions of stored fields, compiled
to the postfix program that derive_kernel (csrc/avr_derive.hip) interprets.  numpy only.

The program is the expression tree in postfix, left operand first: no constant folding, no
reassociation, no common-subexpression elimination, so that a plain numpy evaluation of the same
text computes the same values bit for bit.
"""
from __future__ import annotations

import ast
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

# opcodes (csrc/avr_internal.h, DeriveOp): word = opcode | operand << 8
OP_CONST, OP_FIELD, OP_BUILTIN = 0, 1, 2
OP_ADD, OP_SUB, OP_MUL, OP_DIV = 3, 4, 5, 6
OP_NEG, OP_SQUARE, OP_SQRT, OP_ABS = 7, 8, 9, 10
OP_MIN, OP_MAX = 11, 12
OP_LT, OP_LE, OP_GT, OP_GE, OP_EQ, OP_NE = 13, 14, 15, 16, 17, 18
OP_WHERE = 19
OP_NAMES = ("CONST", "FIELD", "BUILTIN", "ADD", "SUB", "MUL", "DIV", "NEG", "SQUARE", "SQRT", "ABS",
            "MIN", "MAX", "LT", "LE", "GT", "GE", "EQ", "NE", "WHERE")

BUILTINS = ("x", "y", "z", "dx", "dy", "dz", "cell_volume", "level")
FUNCTIONS = {"sqrt": (OP_SQRT, 1), "abs": (OP_ABS, 1), "minimum": (OP_MIN, 2),
             "maximum": (OP_MAX, 2), "where": (OP_WHERE, 3)}
FIELD_FUNCTION = "field"
# names a derived field cannot take besides the built-ins and the functions (api.HISTOGRAM_WEIGHTS)
RESERVED_NAMES = ("cell_volume", "cells")

MAX_FIELDS = 6
MAX_INSTRUCTIONS = 64
MAX_CONSTANTS = 16
MAX_DEPTH = 8

_BINARY = {ast.Add: OP_ADD, ast.Sub: OP_SUB, ast.Mult: OP_MUL, ast.Div: OP_DIV}
_COMPARE = {ast.Lt: OP_LT, ast.LtE: OP_LE, ast.Gt: OP_GT, ast.GtE: OP_GE, ast.Eq: OP_EQ,
            ast.NotEq: OP_NE}
_POPS = {OP_CONST: 0, OP_FIELD: 0, OP_BUILTIN: 0, OP_NEG: 1, OP_SQUARE: 1, OP_SQRT: 1, OP_ABS: 1,
         OP_WHERE: 3}


@dataclass
class DerivedProgram:
    """A compiled expression: `fields` are the stored fields it reads, in order of first use (the
    operand of a FIELD instruction indexes them), `instructions` one uint32 word per instruction
    (opcode | operand << 8), `constants` the float64 constants (the operand of CONST)."""
    fields: Tuple[str, ...]
    instructions: np.ndarray
    constants: np.ndarray
    text: str

    def listing(self) -> List[Tuple[str, int]]:
        """[(opcode name, operand)] -- for tests and for reading."""
        return [(OP_NAMES[int(w) & 0xFF], int(w) >> 8) for w in self.instructions]


def _piece(text: str, node) -> str:
    try:
        found = ast.get_source_segment(text, node)
    except Exception:
        found = None
    return found if found else type(node).__name__


class _Compiler:
    def __init__(self, text: str, registry: Dict[str, str]):
        self.text = text
        self.registry = registry
        self.fields: List[str] = []
        self.code: List[int] = []
        self.constants: List[float] = []
        self.constant_bits: List[bytes] = []
        self.depth = 0
        self.active: List[str] = []     # registered fields being inlined (cycle check)

    def fail(self, text, node, why):
        raise ValueError(f"{why}: {_piece(text, node)!r}")

    def emit(self, op: int, operand: int = 0):
        self.code.append(op | (operand << 8))
        if len(self.code) > MAX_INSTRUCTIONS:
            raise ValueError(f"the expression needs more than {MAX_INSTRUCTIONS} instructions: "
                             f"{self.text!r}")
        pops = _POPS.get(op, 2)
        self.depth += 1 - pops
        if self.depth > MAX_DEPTH:
            raise ValueError(f"the expression needs a stack deeper than {MAX_DEPTH}: {self.text!r}")

    def constant(self, value: float):
        bits = struct.pack("<d", value)
        if bits in self.constant_bits:
            index = self.constant_bits.index(bits)
        else:
            if len(self.constants) == MAX_CONSTANTS:
                raise ValueError(f"the expression has more than {MAX_CONSTANTS} constants: "
                                 f"{self.text!r}")
            index = len(self.constants)
            self.constants.append(value)
            self.constant_bits.append(bits)
        self.emit(OP_CONST, index)

    def field(self, name: str, text, node):
        if name in self.registry:
            if name in self.active:
                raise ValueError("derived fields refer to each other in a cycle: "
                                 + " -> ".join(self.active + [name]))
            self.active.append(name)
            inner = self.registry[name]
            self.visit(inner, _parse(inner).body)
            self.active.pop()
            return
        if not name:
            self.fail(text, node, "a field name must not be empty")
        if name not in self.fields:
            if len(self.fields) == MAX_FIELDS:
                raise ValueError(f"the expression reads more than {MAX_FIELDS} fields: "
                                 f"{self.text!r}")
            self.fields.append(name)
        self.emit(OP_FIELD, self.fields.index(name))

    def visit(self, text: str, node):
        if isinstance(node, ast.Constant):
            if isinstance(node.value, bool) or not isinstance(node.value, (int, float)):
                self.fail(text, node, "only int and float literals are numbers")
            try:
                self.constant(float(node.value))
            except OverflowError:
                self.fail(text, node, "the literal does not fit a float64")
        elif isinstance(node, ast.Name):
            if node.id in BUILTINS:
                self.emit(OP_BUILTIN, BUILTINS.index(node.id))
            elif node.id in FUNCTIONS or node.id == FIELD_FUNCTION:
                self.fail(text, node, "a function name is not a value")
            else:
                self.field(node.id, text, node)
        elif isinstance(node, ast.UnaryOp):
            if isinstance(node.op, ast.USub):
                self.visit(text, node.operand)
                self.emit(OP_NEG)
            elif isinstance(node.op, ast.UAdd):
                self.visit(text, node.operand)
            else:
                self.fail(text, node, "operator not allowed")
        elif isinstance(node, ast.BinOp):
            if isinstance(node.op, ast.Pow):
                exponent = node.right
                if not (isinstance(exponent, ast.Constant) and type(exponent.value) is int
                        and exponent.value == 2):
                    self.fail(text, node, "** takes the literal exponent 2 only")
                self.visit(text, node.left)
                self.emit(OP_SQUARE)
            elif type(node.op) in _BINARY:
                self.visit(text, node.left)
                self.visit(text, node.right)
                self.emit(_BINARY[type(node.op)])
            else:
                self.fail(text, node, "operator not allowed")
        elif isinstance(node, ast.Compare):
            if len(node.ops) != 1:
                self.fail(text, node, "chained comparisons are not allowed")
            if type(node.ops[0]) not in _COMPARE:
                self.fail(text, node, "comparison not allowed")
            self.visit(text, node.left)
            self.visit(text, node.comparators[0])
            self.emit(_COMPARE[type(node.ops[0])])
        elif isinstance(node, ast.Call):
            if not isinstance(node.func, ast.Name) or node.keywords:
                self.fail(text, node, "call not allowed")
            name = node.func.id
            if name == FIELD_FUNCTION:
                if len(node.args) != 1 or not (isinstance(node.args[0], ast.Constant)
                                               and isinstance(node.args[0].value, str)):
                    self.fail(text, node, "field() takes one string literal")
                self.field(node.args[0].value, text, node)
            elif name in FUNCTIONS:
                op, count = FUNCTIONS[name]
                if len(node.args) != count or any(isinstance(a, ast.Starred) for a in node.args):
                    self.fail(text, node, f"{name}() takes {count} argument{'s' if count > 1 else ''}")
                for argument in node.args:
                    self.visit(text, argument)
                self.emit(op)
            else:
                self.fail(text, node, "unknown function")
        else:
            self.fail(text, node, "not allowed in a derived field")


def _parse(text: str):
    if not isinstance(text, str) or not text.strip():
        raise ValueError("a derived field's expression must be a non-empty string")
    try:
        return ast.parse(text.strip(), mode="eval")
    except SyntaxError as error:
        raise ValueError(f"not an expression: {text!r} ({error.msg})") from None


def compile_expression(text: str, registry: Optional[Dict[str, str]] = None) -> DerivedProgram:
    """text -> DerivedProgram.  Parsed with ast in "eval" mode, only whitelisted nodes are walked
    and nothing is ever evaluated; anything else is a ValueError that names the offending piece.
    Numbers: int and float literals (f64 constants).  A bare identifier that is not a built-in
    (x, y, z, dx, dy, dz, cell_volume, level) or a function name is a field; field("x-velocity")
    covers names that are not identifiers.  Operators: + - * /, unary - and +, e ** 2 (= e * e),
    and one of < <= > >= == != between two operands (1.0 or 0.0).  Functions: sqrt(a), abs(a),
    minimum(a, b), maximum(a, b), where(c, a, b).  Names in `registry` (name -> expression) are
    inlined.  At most 6 fields, 64 instructions, 16 constants (equal bit patterns share one) and a
    stack of 8."""
    compiler = _Compiler(text, dict(registry or {}))
    compiler.visit(text.strip() if isinstance(text, str) else text, _parse(text).body)
    return DerivedProgram(tuple(compiler.fields), np.array(compiler.code, dtype=np.uint32),
                          np.array(compiler.constants, dtype=np.float64), text)


def evaluate_program(program: DerivedProgram, field_arrays: Sequence, builtins: Dict[str, object]):
    """The numpy twin of derive_kernel: interprets program.instructions over field_arrays (one
    float64 array per program.fields entry, all of one shape) and builtins (name -> float64 array
    or scalar for every built-in the program uses).  Returns a float64 array."""
    fields = [np.asarray(a, dtype=np.float64) for a in field_arrays]
    if len(fields) != len(program.fields):
        raise ValueError("field_arrays must hold one array per field of the program")
    shape = np.broadcast_shapes(*[f.shape for f in fields],
                                *[np.shape(v) for v in builtins.values()])
    one, zero = np.float64(1.0), np.float64(0.0)
    stack = []
    with np.errstate(all="ignore"):
        for word in program.instructions:
            op, operand = int(word) & 0xFF, int(word) >> 8
            if op == OP_CONST:
                stack.append(np.float64(program.constants[operand]))
            elif op == OP_FIELD:
                stack.append(fields[operand])
            elif op == OP_BUILTIN:
                stack.append(np.asarray(builtins[BUILTINS[operand]], dtype=np.float64))
            elif op in (OP_NEG, OP_SQUARE, OP_SQRT, OP_ABS):
                a = stack.pop()
                stack.append(-a if op == OP_NEG else a * a if op == OP_SQUARE
                             else np.sqrt(a) if op == OP_SQRT else np.abs(a))
            elif op == OP_WHERE:
                b, a, c = stack.pop(), stack.pop(), stack.pop()
                stack.append(np.where(c != zero, a, b))
            elif OP_ADD <= op <= OP_NE:
                b, a = stack.pop(), stack.pop()
                if op == OP_ADD:
                    r = a + b
                elif op == OP_SUB:
                    r = a - b
                elif op == OP_MUL:
                    r = a * b
                elif op == OP_DIV:
                    r = np.divide(a, b)
                elif op == OP_MIN:
                    r = np.where((a < b) | (a != a), a, b)
                elif op == OP_MAX:
                    r = np.where((a > b) | (a != a), a, b)
                else:
                    compare = {OP_LT: np.less, OP_LE: np.less_equal, OP_GT: np.greater,
                               OP_GE: np.greater_equal, OP_EQ: np.equal, OP_NE: np.not_equal}[op]
                    r = np.where(compare(a, b), one, zero)
                stack.append(r)
            else:
                raise ValueError(f"unknown opcode {op}")
    if len(stack) != 1:
        raise ValueError("the program does not end with exactly one value")
    return np.array(np.broadcast_to(np.asarray(stack[0], dtype=np.float64), shape))


# ---- registry ------------------------------------------------------------------------------------

_registry: Dict[str, str] = {}


def is_reserved_name(name: str) -> bool:
    """Whether no registered field may take the name: a built-in, a function or a histogram weight."""
    return name in BUILTINS or name in FUNCTIONS or name == FIELD_FUNCTION or name in RESERVED_NAMES


def add_field(name: str, expression: str) -> DerivedProgram:
    """Registers the derived field `name` = expression for every plotfile-level function of the
    api (render, run, project, project_axis, slice, phase, profile, compute_histogram): wherever
    they take a variable name, `name` now means the expression.  The expression may name other
    registered fields, which are inlined when it is compiled (the limits apply to the inlined
    program); a cycle is refused here.  A name equal to a built-in, a function or a histogram
    weight ("cell_volume", "cells") is refused.  A registered name SHADOWS a plotfile variable of
    the same name: the stored variable is no longer reachable under it until remove_field, neither
    by the api's functions nor by an expression -- field("density") resolves through the registry
    too, so a field called "density" cannot read the stored density (that is refused as a cycle);
    give a field that rescales a stored variable a name of its own.  A name that is not registered
    here stays a field of the program; where it is a registered gradient field (gradient.py) the
    loader supplies that, and a name registered there is refused here, as is a cycle through both.
    Returns the compiled program."""
    if not isinstance(name, str) or not name:
        raise ValueError("a derived field's name must be a non-empty string")
    if is_reserved_name(name):
        raise ValueError(f"{name!r} is a built-in, a function or a histogram weight and cannot "
                         "name a derived field")
    from . import gradient
    gradients = gradient.gradient_fields()
    if name in gradients:
        raise ValueError(f"{name!r} is a registered gradient field")
    from . import clumps
    clump_fields = clumps.clump_fields()
    if name in clump_fields:
        raise ValueError(f"{name!r} is a registered clump field")
    from . import gridfields
    grid_fields = gridfields.grid_fields()
    if name in grid_fields:
        raise ValueError(f"{name!r} is a registered grid field")
    from . import particles
    if name in particles.particle_fields():
        raise ValueError(f"{name!r} is a registered particle field")
    trial = dict(_registry)
    trial[name] = expression
    program = compile_expression(name if name.isidentifier() else f"field({name!r})", trial)
    if gradients or clump_fields or grid_fields:
        # a gradient, clump or grid field it reads may read it
        gradient.check_no_cycle(name, trial, gradients, clump_fields)
    _registry[name] = expression
    return DerivedProgram(program.fields, program.instructions, program.constants, expression)


def remove_field(name: str) -> None:
    """Forgets a registered derived field (KeyError if there is none of that name)."""
    del _registry[name]


def derived_fields() -> Dict[str, str]:
    """name -> expression of every registered derived field (a copy)."""
    return dict(_registry)


def compile_field(name: str) -> DerivedProgram:
    """The inlined program of the registered field `name`."""
    return compile_expression(name if name.isidentifier() else f"field({name!r})", _registry)
