"""The polar filter's expression compiler (transflow_amd/exprs.py) without a GPU: its programs are run
by a numpy stack machine that mirrors k_pp_polar step for step, and compared with what the reference
computed (tests/golden/flow_polar.npz).  Also pins the oracle's polar() on the same vectors."""
import os

import numpy as np
import pytest

from oracle import flow_ops_ref as F
from tests.helpers import GOLDEN
from transflow_amd.exprs import FUNCS, OPS, PolarFilter, Program, Unsupported

Z = np.load(os.path.join(GOLDEN, "flow_polar.npz"))
T = float(Z["t"])


def run_program(steps, r, a):
    """numpy twin of polar_eval in flowops.hip: a stack of float64 arrays, float32 steps round-trip."""
    st = []
    f32 = lambda x: np.asarray(x, np.float64).astype(np.float32)   # noqa: E731
    un = {"neg": np.negative, "sin": np.sin, "cos": np.cos, "tan": np.tan, "arcsin": np.arcsin, "arccos": np.arccos,
          "arctan": np.arctan, "sqrt": np.sqrt, "abs": np.abs, "exp": np.exp, "log": np.log, "log2": np.log2,
          "log10": np.log10, "floor": np.floor, "ceil": np.ceil, "rint": np.rint, "sign": np.sign,
          "square": np.square, "reciprocal": lambda x: 1 / x}
    bi = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "pow": np.power, "mod": np.mod,
          "floordiv": np.floor_divide, "arctan2": np.arctan2, "minimum": np.minimum, "maximum": np.maximum,
          "hypot": np.hypot, "lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal,
          "eq": np.equal, "ne": np.not_equal}
    with np.errstate(all="ignore"):
        for op, wide, imm in steps:
            name = OPS[op]
            cast = (lambda x: np.asarray(x, np.float64)) if wide else f32
            if name == "push_r":
                st.append(np.asarray(r, np.float64))
            elif name == "push_a":
                st.append(np.asarray(a, np.float64))
            elif name == "push_const":
                st.append(np.float64(imm))
            elif name == "where":
                y, x, c = st.pop(), st.pop(), st.pop()
                st.append(np.where(c != 0, cast(x), cast(y)).astype(np.float64))
            elif name == "clip":
                hi, lo, x = st.pop(), st.pop(), st.pop()
                st.append(np.clip(cast(x), cast(lo), cast(hi)).astype(np.float64))
            elif name == "not":
                st.append((st.pop() == 0).astype(np.float64))
            elif name in bi:
                b, x = st.pop(), st.pop()
                st.append(np.asarray(bi[name](cast(x), cast(b)), np.float64))
            else:
                st.append(np.asarray(un[name](cast(st.pop())), np.float64))
    assert len(st) == 1
    return st[0]


def apply_polar(flow, er, ea, t):
    pf = PolarFilter(er, ea)
    sr, sa, wide_trig, wide_product = pf.programs(t)
    x, y = flow[:, :, 0], flow[:, :, 1]
    r = np.sqrt(x * x + y * y)
    a = np.arctan2(y, x)
    R, A = run_program(sr, r, a), run_program(sa, r, a)
    s, c = (np.sin(A), np.cos(A)) if wide_trig else (np.sin(A.astype(np.float32)), np.cos(A.astype(np.float32)))
    if wide_product:
        oy, ox = (R * s).astype(np.float32), (R * c).astype(np.float32)
    else:
        oy, ox = R.astype(np.float32) * s.astype(np.float32), R.astype(np.float32) * c.astype(np.float32)
    out = np.empty_like(flow)           # assigned, not added to zeros: -0.0 stays -0.0
    out[:, :, 1], out[:, :, 0] = oy, ox
    return out


@pytest.mark.parametrize("i", range(int(Z["cases"])))
def test_compiled_programs_reproduce_the_reference(i):
    er, ea = str(Z[f"er_{i}"]), str(Z[f"ea_{i}"])
    out = apply_polar(Z[f"in_{i}"].copy(), er, ea, T)
    exp = Z[f"out_{i}"]
    # same numpy functions on the same float32 values, in the type numpy would have used: exact
    np.testing.assert_array_equal(out, exp, err_msg=f"{er!r} : {ea!r}")


@pytest.mark.parametrize("i", range(int(Z["cases"])))
def test_oracle_polar_golden(i):
    out = F.polar(Z[f"in_{i}"].copy(), str(Z[f"er_{i}"]), str(Z[f"ea_{i}"]), T)
    np.testing.assert_array_equal(out, Z[f"out_{i}"])


def test_compiler_limits_and_errors():
    assert Program("2*t+1").scalar_only and Program("2*t+1").host_value(0.5) == 2.0
    steps, kind = Program("r + numpy.float64(1)").resolve(0.0)
    assert kind == 1 and steps[-1][1] == 1                      # a numpy.float64 scalar is strong: float64 add
    steps, kind = Program("r + 1.5").resolve(0.0)
    assert kind == 0 and steps[-1][1] == 0                      # a Python float is weak: float32 add
    assert [OPS[s[0]] for s in Program("r**2").resolve(0.0)[0]] == ["push_r", "square"]
    assert [OPS[s[0]] for s in Program("r**0.5").resolve(0.0)[0]] == ["push_r", "sqrt"]
    assert [OPS[s[0]] for s in Program("r**t").resolve(3.0)[0]] == ["push_r", "push_const", "pow"]
    for bad in ("r.sum()", "numpy.cumsum(r)", "[r, a][0]", "r if t else a", "numpy.fft.fft(r)"):
        with pytest.raises(Unsupported):
            Program(bad)
    with pytest.raises(Unsupported):
        Program("+".join(["r"] * 40))                           # longer than the device's program
    with pytest.raises(Unsupported):
        Program("r + numpy.ones(3)").resolve(0.0)               # host subtree that is an array
    with pytest.raises(SyntaxError):
        Program("r +")


# ---- typing corpus ---------------------------------------------------------------------------------------------
# (radius, theta) pairs.  What numpy makes of each on float32 r, a decides what the compiler must do: the same
# result types (F32 <-> float32, F64 <-> float64 or int64, BOOL <-> bool) and sin / product widths, or, where
# numpy leaves float32 / float64 / bool (float16, int8, logic, TypeError, ValueError), Unsupported raised as
# the PolarFilter is built, so that dropin hands the request to the reference.
CORPUS = [
    # every opcode, weak Python scalars (float32 arithmetic)
    ("r", "a"), ("r + 1.5", "a"), ("r - 0.1", "a - 1"), ("r * 0.3", "a * 2"), ("r / 7", "a / 3"),
    ("r % 1.5", "a"), ("(r - 7) % 1.5", "a"), ("r // 0.1", "a"), ("(r - 32) // 0.3", "a"), ("-r", "-a"),
    ("numpy.sin(r)", "numpy.cos(a)"), ("numpy.tan(r)", "a"), ("numpy.arcsin(r / 64)", "numpy.arccos(r / 64)"),
    ("numpy.arctan(r)", "numpy.arctan2(a, r)"), ("numpy.sqrt(r)", "a"), ("numpy.abs(r - 3)", "a"),
    ("numpy.exp(r / 16)", "a"), ("numpy.log(r)", "a"), ("numpy.log2(r)", "numpy.log10(r)"),
    ("numpy.minimum(r, 3)", "numpy.maximum(a, 1)"), ("numpy.floor(r * 0.3)", "numpy.ceil(a)"),
    ("numpy.rint(r - 0.5)", "a"), ("numpy.sign(r - 2)", "a"), ("numpy.square(r)", "a"),
    ("numpy.hypot(r, 3)", "a"), ("numpy.where(r < 2, r, 0)", "a"), ("numpy.where(r <= 2, 1.5, r)", "a"),
    ("numpy.where(r > 2, r, 2)", "a"), ("numpy.where(r >= 2, r, -r)", "a"), ("numpy.where(r == 2, 0, r)", "a"),
    ("numpy.where(r != 2, r, 0)", "a"), ("numpy.where(~(r > 2), r, 0)", "a"), ("numpy.clip(r, 1, 4)", "a"),
    ("numpy.clip(r - 32, -0.0, 3.5)", "a"),
    ("numpy.reciprocal(r)", "a"), ("r ** 1.7", "a"),
    # the other spellings of FUNCS
    ("numpy.atan2(r, 2)", "numpy.asin(a / 4)"), ("numpy.acos(r / 64)", "numpy.atan(a)"),
    ("numpy.absolute(r - 3)", "numpy.fabs(a)"), ("abs(r - 3)", "a"), ("numpy.round(r)", "a"),
    ("numpy.power(r, 1.5)", "a"), ("numpy.add(r, 1)", "numpy.subtract(a, 1)"),
    ("numpy.multiply(r, 2)", "numpy.divide(a, 2)"), ("numpy.negative(r)", "a"), ("numpy.mod(r, 0.7)", "a"),
    ("numpy.floor_divide(r, 0.7)", "a"), ("numpy.where(numpy.less(r, 2), 0, r)", "a"),
    ("numpy.where(numpy.greater(r, 2), 0, r)", "a"), ("np.sqrt(r)", "a"),
    # strong numpy scalars and host subtrees of t
    ("r + numpy.float64(1)", "a"), ("r * numpy.float32(0.1)", "a"), ("r", "a * numpy.float64(2)"),
    ("r", "a + numpy.float32(1)"), ("r * (1 + t)", "a + math.sin(t)"), ("r + numpy.float64(t)", "a"),
    ("r // numpy.float64(0.1)", "a"), ("(r - 7) % numpy.float64(1.5)", "a"), ("r + numpy.int64(2)", "a"),
    ("r * t", "t * 3"), ("2 * t", "a"), ("numpy.float64(2)", "a"), ("numpy.float32(2)", "a + t"),
    ("r", "numpy.float32(t)"), ("r", "0"), ("1", "a"),
    # numpy's scalar-exponent fast paths
    ("r ** 2", "a"), ("r ** 0.5", "a"), ("r ** -1", "a"), ("r ** 1", "a"), ("r ** 3", "a"), ("r ** t", "a"),
    ("r ** numpy.float64(2)", "a"), ("r ** 2.0", "a ** 2"),
    # numpy.power is the plain ufunc: no fast path, normal promotion
    ("numpy.power(r, numpy.float64(2))", "a + 0.3"), ("numpy.power(r, numpy.float64(0.5))", "a + 0.3"),
    ("numpy.power(-r, 0.5)", "a"), ("numpy.power(r, 2)", "a"), ("numpy.power(r - 32, -1)", "a"),
    ("(-r) ** 0.5", "a"), ("(r - 32) ** numpy.float64(-1)", "a + 0.3"),
    # comparisons feeding where, * and +
    ("r * (r > 2)", "a"), ("r + (a > 1)", "a"), ("(r > 2) * r", "a"), ("(r > 2) * 1.5", "a"),
    ("(r > 2) + 1", "a"), ("(r > 2) * t", "a"), ("(r > 2) / 2", "a"), ("numpy.where(r > 2, 1, 0)", "a"),
    ("numpy.where(r > 2, 1, 0) * 2 - 1", "a"), ("numpy.where(r > 2, 1.5, 0)", "a"),
    ("r", "numpy.where(r > 2, 1, 0)"), ("numpy.where(r > 2, 1, 0) / 3", "numpy.sin(numpy.where(r > 2, 1, 0))"),
    # booleans among themselves: logic, not arithmetic
    ("(r > 2) + (r > 4)", "a"), ("(r > 2) * (r < 4)", "a"), ("numpy.maximum(r > 2, r > 4)", "a"),
    ("(r > 2) + True", "a"), ("numpy.where(r > 2, True, False)", "a"), ("numpy.abs(r > 2)", "a"),
    ("((r > 2) + (r > 4)) * r", "a"), ("(r > 2) / (r > 4)", "a"),
    ("(r > 2) + (t > 1)", "a"), ("(r > 2) * (t < 1)", "a"), ("(r > 2) - (t > 1)", "a"),
    # float ufuncs of booleans (float16), unary minus of a boolean (TypeError), integer loops: refused
    ("numpy.exp(r > 2)", "a"), ("numpy.sqrt(r > 2)", "a"), ("r", "r > 2"), ("r", "numpy.sin(r > 2)"),
    ("-(r > 2)", "a"), ("(r > 2) - (r > 4)", "a"), ("(r > 2) ** 2", "a"), ("(r > 2) // (r > 4)", "a"),
    ("numpy.arctan2(r > 2, r > 4)", "a"), ("numpy.sign(r > 2)", "a"), ("numpy.square(r > 2)", "a"),
    ("numpy.reciprocal(r > 2)", "a"), ("r", "True"),
    ("r", "t > 1"), ("r", "t > 1 and t"), ("r", "1.0 if t > 1 else (t < 2)"), ("r", "1.0 if t > 1 else 2.0"), ("numpy.where(r > 2, 3, 1) ** -1", "a"),
    ("numpy.where(r > 2, 3, 1) // 0", "a"),
]
# expressions numpy computes in its integer loops that the compiler refuses although numpy does not raise
REFUSED = {"numpy.where(r > 2, 3, 1) // 0"}
T_CORPUS = 0.7


def assert_same_bits(out, exp, msg=""):
    """Bit for bit, signed zeros included; NaN in the same places (a NaN's sign and payload are not numpy's to
    promise)."""
    nan = np.isnan(exp)
    np.testing.assert_array_equal(np.isnan(out), nan, err_msg=f"NaN positions: {msg}")
    bad = ~nan & (out.view(np.uint32) != exp.view(np.uint32))
    assert not bad.any(), f"{msg}: {int(bad.sum())} values differ, e.g. {out[bad][:4]} != {exp[bad][:4]}"


def _corpus_flow():
    from tests.helpers import polar_flow, polar_values
    f = polar_flow(polar_values())
    g = np.random.default_rng(23).normal(0, 4, (1, 64, 2)).astype(np.float32)
    return np.concatenate([f, g], axis=1)


def _numpy_types(er, ea, flow):
    """(radius dtype, theta dtype, sin dtype, product dtype) as numpy evaluates them, or None if numpy raises."""
    import math
    import random
    scope = {"math": math, "numpy": np, "random": random}         # the reference's scope: no `np`
    try:
        with np.errstate(all="ignore"):
            r = np.sqrt(flow[..., 0] * flow[..., 0] + flow[..., 1] * flow[..., 1])
            a = np.arctan2(flow[..., 1], flow[..., 0])
            R = eval("lambda t, r, a: " + er, scope)(T_CORPUS, r, a)
            A = eval("lambda t, r, a: " + ea, scope)(T_CORPUS, r, a)
            s = np.sin(A)
            p = R * s
    except (TypeError, ValueError, NameError):
        return None
    return tuple(np.result_type(x) for x in (R, A, s, p))


def _device_types(dt):
    return {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int64): 1, np.dtype(bool): 2}.get(dt)


@pytest.mark.parametrize("er,ea", CORPUS)
def test_corpus_types_follow_numpy(er, ea):
    flow = _corpus_flow()
    types = _numpy_types(er, ea, flow)
    representable = types is not None and all(_device_types(d) is not None for d in types[:2]) and \
        types[2] in (np.float32, np.float64) and types[3] in (np.float32, np.float64)
    if not representable or er in REFUSED:
        with pytest.raises(Unsupported):
            PolarFilter(er, ea)
        return
    pf = PolarFilter(er, ea)
    _, _, wide_trig, wide_product = pf.programs(T_CORPUS)
    assert wide_trig == (types[2] == np.float64), types
    assert wide_product == (types[3] == np.float64), types
    for prog, dt in ((pf.radius, types[0]), (pf.theta, types[1])):
        if not prog.scalar_only:
            assert prog.resolve(T_CORPUS)[1] == _device_types(dt), (prog.text, dt)


@pytest.mark.parametrize("er,ea", [c for c in CORPUS if c[0] not in REFUSED])
def test_corpus_twin_matches_oracle_bit_for_bit(er, ea):
    """The twin runs the compiled program through numpy's own ufuncs in the types the compiler chose: where those
    are numpy's types the results agree bit for bit, signed zeros and NaN positions included, on every value of
    the set -- transcendentals too, as both sides call the same numpy function."""
    flow = _corpus_flow()
    if _numpy_types(er, ea, flow) is None:          # the reference raises: so does the compiler
        with pytest.raises(Unsupported):
            PolarFilter(er, ea)
        return
    try:
        PolarFilter(er, ea)
    except Unsupported:                             # float16 and the like: test_corpus_types_follow_numpy
        return
    with np.errstate(all="ignore"):
        exp = F.polar(flow.copy(), er, ea, T_CORPUS)
        out = apply_polar(flow.copy(), er, ea, T_CORPUS)
    assert_same_bits(out, exp, f"{er!r} : {ea!r}")


def test_corpus_covers_every_opcode_and_spelling():
    seen = set()
    for er, ea in CORPUS:
        try:
            pf = PolarFilter(er, ea)
            sr, sa, _, _ = pf.programs(T_CORPUS)
        except Unsupported:
            continue
        seen |= {OPS[s[0]] for s in sr + sa}
        seen |= {op for op, _, _ in pf.radius.code + pf.theta.code}
    assert set(OPS) <= seen, set(OPS) - seen
    text = " ".join(er + " " + ea for er, ea in CORPUS)
    for name in FUNCS:
        assert f"numpy.{name}(" in text or (name == "abs" and "abs(" in text), name
    assert len(CORPUS) >= 60
