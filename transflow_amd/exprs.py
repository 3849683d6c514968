"""Compiler from the `polar` flow filter's user expressions to the postfix programs the GPU runs.

The reference evaluates two Python expressions of (t, r, a) with r, a float32 arrays [H, W]
(transflow/flow/filters.py:75-87, utils.parse_lambda_expression utils.py:409-414).  Here every
subtree that does not touch r or a stays Python: it is evaluated on the host for each frame (so
`math`, `random`, anything of t works as in the reference) and becomes a constant of the program;
the array part must be built from arithmetic, comparisons and the numpy functions in FUNCS, which is
what runs per pixel in `k_pp_polar`.  numpy's typing is kept: float32 arithmetic unless a
numpy.float64 scalar takes part (NEP 50: Python scalars are weak).  Transcendental functions differ
from numpy's by a few units in the last place.
"""
from __future__ import annotations

import ast
import math
import os
import random
import re

import numpy

# opcodes shared with flowops.hip (enum PolarOp)
OPS = ["push_r", "push_a", "push_const", "add", "sub", "mul", "div", "pow", "mod", "floordiv", "neg", "sin", "cos",
       "tan", "arcsin", "arccos", "arctan", "arctan2", "sqrt", "abs", "exp", "log", "log2", "log10", "minimum",
       "maximum", "floor", "ceil", "rint", "sign", "square", "hypot", "lt", "le", "gt", "ge", "eq", "ne", "where",
       "clip", "reciprocal", "not"]
OP = {name: i for i, name in enumerate(OPS)}
MAX_INSTR = 48
MAX_STACK = 12

BINOPS = {ast.Add: "add", ast.Sub: "sub", ast.Mult: "mul", ast.Div: "div", ast.Pow: "pow", ast.Mod: "mod",
          ast.FloorDiv: "floordiv"}
CMPOPS = {ast.Lt: "lt", ast.LtE: "le", ast.Gt: "gt", ast.GtE: "ge", ast.Eq: "eq", ast.NotEq: "ne"}
# numpy function name -> (opcode, number of arguments)
FUNCS = {"sin": ("sin", 1), "cos": ("cos", 1), "tan": ("tan", 1), "arcsin": ("arcsin", 1), "arccos": ("arccos", 1),
         "arctan": ("arctan", 1), "arctan2": ("arctan2", 2), "atan2": ("arctan2", 2), "asin": ("arcsin", 1),
         "acos": ("arccos", 1), "atan": ("arctan", 1), "sqrt": ("sqrt", 1), "abs": ("abs", 1),
         "absolute": ("abs", 1), "fabs": ("abs", 1), "exp": ("exp", 1), "log": ("log", 1), "log2": ("log2", 1),
         "log10": ("log10", 1), "minimum": ("minimum", 2), "maximum": ("maximum", 2), "floor": ("floor", 1),
         "ceil": ("ceil", 1), "rint": ("rint", 1), "round": ("rint", 1), "sign": ("sign", 1), "square": ("square", 1),
         "hypot": ("hypot", 2), "where": ("where", 3), "clip": ("clip", 3), "power": ("pow", 2),
         "reciprocal": ("reciprocal", 1), "add": ("add", 2), "subtract": ("sub", 2), "multiply": ("mul", 2),
         "divide": ("div", 2), "negative": ("neg", 1), "mod": ("mod", 2), "floor_divide": ("floordiv", 2),
         "less": ("lt", 2), "greater": ("gt", 2)}
SCOPE = {"math": math, "numpy": numpy, "random": random, "re": re, "os": os}   # the reference's utils module scope
F32, F64, BOOL = 0, 1, 2


class Unsupported(NotImplementedError):
    pass


def _uses_arrays(node) -> bool:
    return any(isinstance(n, ast.Name) and n.id in ("r", "a") for n in ast.walk(node))


CMP = ("lt", "le", "gt", "ge", "eq", "ne")
FLOAT_UFUNCS = ("sin", "cos", "tan", "arcsin", "arccos", "arctan", "sqrt", "exp", "log", "log2", "log10", "rint")
FAST_POWERS = (2.0, 0.5, -1.0, 1.0)
I64 = "i64"     # an integer array (numpy's int64): carried as float64 on the device, reported as F64


def _static_kind(op, kinds):
    """The static kind of op's result (see Program._const), or Unsupported where numpy would leave float32 /
    float64 arithmetic for good or may do so for some host value."""
    if op in CMP:
        return "b"
    if op == "not":
        if kinds[0] != "b":
            raise Unsupported("~ on a non-boolean array")
        return "b"
    if op == "where":
        kinds = kinds[1:]                                 # the condition does not take part in the promotion
    if "f" in kinds:
        return "f"
    boolean = all(k in ("b", "cb") for k in kinds)
    unknown = any(k in ("x", "cx") for k in kinds)
    if op in FLOAT_UFUNCS or op in ("arctan2", "hypot"):
        if any(k in ("i", "ci", "cf") for k in kinds):
            return "f"
        raise Unsupported(f"numpy.{op} of a boolean array is float16")
    if op in ("neg", "sign"):
        if kinds[0] == "i":
            return "i"
        raise Unsupported(f"numpy.{'negative' if op == 'neg' else op} of a boolean array raises TypeError")
    if op in ("abs", "floor", "ceil"):
        return kinds[0]
    if op == "div":
        return "f"
    if op in ("pow", "mod", "floordiv") and "cf" in kinds:
        return "f"
    if op in ("square", "reciprocal", "pow", "mod", "floordiv"):
        raise Unsupported(f"integer {op} of a boolean or integer array")
    if op == "sub" and boolean:
        raise Unsupported("numpy cannot subtract boolean arrays (TypeError)")
    # add, sub, mul, minimum, maximum, clip, where
    if "cf" in kinds:
        return "f"
    if unknown:
        return "x"
    return "b" if boolean else "i"


def _boolean_form(node) -> bool:
    """A host subtree whose value is a bool by its form: a comparison, `not`, bool(...)."""
    return isinstance(node, ast.Compare) or (isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.Not)) or (
        isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "bool")


def _maybe_boolean(node) -> bool:
    """A host subtree that may evaluate to a bool: of boolean form or literal, or an and / or / if-else one of
    whose operands may."""
    if isinstance(node, ast.BoolOp):
        return any(_maybe_boolean(v) for v in node.values)
    if isinstance(node, ast.IfExp):
        return _maybe_boolean(node.body) or _maybe_boolean(node.orelse)
    return _literal_kind(node) == "cb"


def _literal_kind(node):
    """'cb' / 'ci' / 'cf' for a literal bool / int / float (a comparison, `not` or bool(...) is a bool too),
    'cx' for a host value whose type shows per frame."""
    if _boolean_form(node):
        return "cb"
    try:
        v = ast.literal_eval(node)
    except (ValueError, TypeError, SyntaxError, MemoryError, RecursionError):
        return "cx"
    return "cb" if isinstance(v, bool) else "ci" if isinstance(v, int) else "cf" if isinstance(v, float) else "cx"


def _promote(kinds):
    """numpy's result type (NEP 50) of arrays / strong scalars F32, F64, BOOL, I64 and weak Python scalars
    'wb' / 'wi' / 'wf' (bool / int / float)."""
    if F64 in kinds:
        return F64
    if F32 in kinds:
        return F64 if I64 in kinds else F32
    if "wf" in kinds:
        return F64
    if I64 in kinds or "wi" in kinds:
        return I64
    return BOOL


def _integer_result(op, k):
    """The kind of op on boolean (k == BOOL) or integer (k == I64) operands, as numpy computes it."""
    if op == "div" or (k == I64 and (op in FLOAT_UFUNCS or op in ("arctan2", "hypot"))):
        return F64                                       # true division / float ufuncs of integers: float64
    if op in ("pow", "mod", "floordiv", "reciprocal"):
        raise Unsupported(f"integer {op} of a boolean or integer array")
    if k == BOOL and (op in FLOAT_UFUNCS or op in ("arctan2", "hypot", "square", "sign", "neg", "sub")):
        raise Unsupported(f"numpy's {op} of a boolean array is not bool or float arithmetic")
    return k


def _const_kind(v):
    if isinstance(v, numpy.ndarray):
        raise Unsupported("array-valued sub-expression that does not come from r or a")
    if isinstance(v, (bool, numpy.bool_)):
        return "wb"
    if isinstance(v, numpy.floating) and v.dtype in (numpy.float32, numpy.float64):
        return F64 if v.dtype == numpy.float64 else F32
    if isinstance(v, numpy.integer) and numpy.result_type(numpy.float32, v.dtype) == numpy.float64:
        return I64
    if isinstance(v, (int, float)) and not isinstance(v, numpy.generic):
        return "wi" if isinstance(v, int) else "wf"
    raise Unsupported(f"polar sub-expression of type {type(v).__name__}")


class Program:
    """One compiled expression: `code` is a list of (opcode, f64 flag, host-constant index or -1);
    `consts` the Python code objects of the host subtrees (evaluated per frame with t)."""

    def __init__(self, text: str):
        self.text = text
        tree = ast.parse(text.strip(), mode="eval").body
        self.code: list = []
        self.consts: list = []
        self.static: list = []
        self.scalar_only = not _uses_arrays(tree)
        self.maybe_boolean = self.scalar_only and _maybe_boolean(tree)
        self._whole = compile(ast.Expression(tree), "<polar>", "eval")
        if not self.scalar_only:
            self._emit(tree)
            if len(self.code) > MAX_INSTR:
                raise Unsupported(f"polar expression too long for the device ({len(self.code)} > {MAX_INSTR} steps)")
            self._check_stack()

    # ---- compilation ------------------------------------------------------------------------
    # Every instruction also gets a static kind, known before any frame: "f" a float array, "b" a boolean array,
    # "i" an integer array, "x" an array that is boolean, integer or float depending on a host value's type; host
    # values "cb" / "ci" / "cf" for a literal bool / int / float (or a comparison), "cx" for anything else.  numpy runs boolean and
    # integer arrays through loops the device does not model (float16 results, logic for arithmetic, integer
    # division); those expressions raise Unsupported here, while the Program is built, so that dropin can hand the
    # request to the reference instead.
    def _const(self, node):
        """A host subtree: dtype is known only per frame; recorded as 'weak unless numpy says otherwise'."""
        self.consts.append(compile(ast.Expression(node), "<polar>", "eval"))
        self.code.append(["push_const", None, len(self.consts) - 1])
        self.static.append(_literal_kind(node))
        return len(self.code) - 1

    def _emit(self, node):
        if not _uses_arrays(node):
            return self._const(node)
        if isinstance(node, ast.Name):
            self.code.append(["push_r" if node.id == "r" else "push_a", F32, -1])
            self.static.append("f")
            return len(self.code) - 1
        if isinstance(node, ast.BinOp) and type(node.op) in BINOPS:
            lt = self._emit(node.left)
            rt = self._emit(node.right)
            i = self._push_op(BINOPS[type(node.op)], lt, rt)
            if isinstance(node.op, ast.Pow):
                self.code[i][1] = ("args", (lt, rt), "**")     # the operator: numpy's scalar fast paths apply
            return i
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
            t = self._emit(node.operand)
            if isinstance(node.op, ast.USub):
                return self._push_op("neg", t)
            if self.static[t] != "f":
                raise Unsupported("unary + of a boolean or integer array")
            return t
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.Invert):
            return self._push_op("not", self._emit(node.operand))
        if isinstance(node, ast.Compare) and len(node.ops) == 1 and type(node.ops[0]) in CMPOPS:
            lt = self._emit(node.left)
            rt = self._emit(node.comparators[0])
            return self._push_op(CMPOPS[type(node.ops[0])], lt, rt)
        if isinstance(node, ast.Call) and not node.keywords:
            fn = node.func
            name = None
            if isinstance(fn, ast.Attribute) and isinstance(fn.value, ast.Name) and fn.value.id == "numpy":
                name = fn.attr
            elif isinstance(fn, ast.Name) and fn.id == "abs":
                name = "abs"
            if name in FUNCS and FUNCS[name][1] == len(node.args):
                args = [self._emit(arg) for arg in node.args]
                return self._push_op(FUNCS[name][0], *args)
        raise Unsupported(f"polar expression not supported on the device: {ast.unparse(node)!r}")

    def _push_op(self, op, *args):
        # the result's dtype is settled per frame in resolve(): constants' types are known only then
        self.static.append(_static_kind(op, [self.static[i] for i in args]))
        self.code.append([op, ("args", args), -1])
        return len(self.code) - 1

    def _check_stack(self):
        depth = peak = 0
        arity = {"where": 3, "clip": 3}
        for op, _, _ in self.code:
            if op.startswith("push"):
                depth += 1
            else:
                n = arity.get(op, 2 if op in ("add", "sub", "mul", "div", "pow", "mod", "floordiv", "arctan2", "minimum",
                                              "maximum", "hypot", "lt", "le", "gt", "ge", "eq", "ne") else 1)
                depth -= n - 1
            peak = max(peak, depth)
        if peak > MAX_STACK:
            raise Unsupported(f"polar expression needs a deeper stack than the device has ({peak} > {MAX_STACK})")

    # ---- per frame ------------------------------------------------------------------------------
    def host_value(self, t):
        """The whole expression on the host (only valid when it does not use r or a)."""
        return eval(self._whole, SCOPE, {"t": t})

    def resolve(self, t):
        """[(opcode, f64 flag, immediate)] for this frame: host constants evaluated, types propagated
        the way numpy does (weak Python scalars, strong numpy scalars)."""
        vals = [eval(c, SCOPE, {"t": t}) for c in self.consts]
        kinds = {}      # instruction index -> F32 / F64 / BOOL / I64, or 'wb' / 'wi' / 'wf' for a Python scalar
        out = []
        for i, (op, info, ci) in enumerate(self.code):
            if op == "push_const":
                v = vals[ci]
                kinds[i] = _const_kind(v)
                out.append((OP[op], 1, float(v)))       # immediates travel as double; rounded at use
                continue
            if op in ("push_r", "push_a"):
                kinds[i] = F32
                out.append((OP[op], 0, 0.0))
                continue
            ks = [kinds[j] for j in info[1]]
            k = _promote(ks[1:] if op == "where" else ks)
            if op == "pow" and info[2:] == ("**",) and ks[0] in (F32, F64) and \
                    self.code[info[1][1]][0] == "push_const" and float(vals[self.code[info[1][1]][2]]) in FAST_POWERS:
                # float array ** scalar: numpy's fast path, a ufunc of the array alone whatever the scalar's type
                # (2 -> square, 0.5 -> sqrt, -1 -> reciprocal, 1 -> the array itself); numpy.power promotes as usual
                kinds[i] = ks[0]
                e = out.pop()[2]                         # the exponent, pushed just before
                if e != 1.0:
                    out.append((OP[{2.0: "square", 0.5: "sqrt", -1.0: "reciprocal"}[e]], int(ks[0] != F32), 0.0))
                continue
            if op in CMP:
                kinds[i] = BOOL
                out.append((OP[op], int(k != F32), 0.0))
                continue
            if op == "not" and ks[0] != BOOL:
                raise Unsupported("~ on a non-boolean array")
            if k in (BOOL, I64):
                # boolean / integer operands: numpy's own loops, modelled where they are exact, refused otherwise
                # (float16 results for a boolean, integer division and powers, TypeError)
                k = _integer_result(op, k)
            kinds[i] = k
            if op == "add" and k == BOOL:
                op = "maximum"                           # bool + bool is a logical or
            out.append((OP[op], int(k != F32), 0.0))
        kind = kinds[len(self.code) - 1] if self.code else "wf"
        return out, (F64 if kind == I64 else kind)


class PolarFilter:
    """filters.py:75-87 with its two expressions compiled for the device."""

    def __init__(self, expr_radius: str, expr_theta: str):
        self.radius, self.theta = Program(expr_radius), Program(expr_theta)
        th = self.theta
        if th.maybe_boolean if th.scalar_only else th.static[-1] in ("b", "x", "cb"):
            raise Unsupported("numpy.sin of a boolean angle is float16")

    @staticmethod
    def _steps(prog: Program, t):
        if prog.scalar_only:
            v = prog.host_value(t)
            kind = _const_kind(v)
            return [(OP["push_const"], 1, float(v))], (F64 if kind == I64 else kind)
        return prog.resolve(t)

    def programs(self, t):
        """(radius steps, theta steps, wide_trig, wide_product) for frame time t."""
        sr, kr = self._steps(self.radius, t)
        st, kt = self._steps(self.theta, t)
        if kt in (BOOL, "wb"):
            raise Unsupported("numpy.sin of a boolean angle is float16")
        wide_trig = kt != F32            # numpy.sin of a float64 -- or of a bare Python scalar -- is a float64
        wide_product = wide_trig or kr == F64
        return sr, st, wide_trig, wide_product
