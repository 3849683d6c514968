"""The polar filter's interpreter (k_pp_polar / polar_eval in flowops.hip) opcode by opcode against the oracle's
numpy evaluation (oracle.flow_ops_ref.polar).

The flows are (x, 0): then r == |x| on both sides (the float32 square of x is exact in the norm's sqrt away from
under- and overflow) and a is 0 or pi.  With the angle expression "0" both sides multiply by cos 0 = 1 and
sin 0 = 0 exactly, so out[..., 0] is the radius program's result rounded to float32 and the two sides can be
compared bit for bit.

Exact operations (arithmetic, floor_divide, mod, rounding, comparisons, where, clip, ...) must agree bit for bit,
signed zeros and NaN positions included, in float32 (Python-scalar constants) and float64 (numpy.float64
constants).  Transcendental functions must put NaN and +-inf in the same places and be within a per-function
number of float32 ulps elsewhere; ULP_BOUND below records the largest distance observed on an MI355X and the
bound allowed (at most twice the observed value, never above 4).  Observed / allowed, float32 forms:
sin 1/2, cos 1/2, tan 2/4, arcsin 2/4, arccos 1/2, arctan 1/2, arctan2 2/4, exp 2/4, log 2/4, log2 1/2,
log10 3/4, pow 1/2, hypot 1/2; float64 forms 0 for all of them.  Denormal float32 results (r * 1e-39) are kept
on the device, so they sit in the exact class.
"""
import numpy as np
import pytest

from oracle import flow_ops_ref as F
from tests.helpers import polar_flow, polar_values

pytestmark = pytest.mark.gpu
T = 0.7


def _run(er, ea, flow):
    from transflow_amd.exprs import PolarFilter
    from transflow_amd.flowops import polar_filter
    with np.errstate(all="ignore"):
        exp = F.polar(flow.copy(), er, ea, T)
    out = polar_filter(flow.copy(), PolarFilter(er, ea), T)
    return out, exp


def _same_bits(out, exp, msg):
    nan = np.isnan(exp)
    np.testing.assert_array_equal(np.isnan(out), nan, err_msg=f"NaN positions: {msg}")
    bad = ~nan & (out.view(np.uint32) != exp.view(np.uint32))
    if bad.any():
        i = np.nonzero(bad.reshape(-1, 2).any(axis=1))[0][:6]
        raise AssertionError(f"{msg}: {int(bad.sum())} values differ; at pixels {i.tolist()}: "
                             f"device {out.reshape(-1, 2)[i].tolist()} numpy {exp.reshape(-1, 2)[i].tolist()}")


def _ordered(x):
    """float32 -> integers in the order of the floats, one apart per ulp (+0 and -0 both 0)."""
    u = x.astype(np.float32).view(np.int32).astype(np.int64)
    return np.where(u < 0, -(u & 0x7FFFFFFF), u)


def ulp_distance(out, exp):
    """Per element: the float32 ulp distance of finite values; NaN / inf positions are checked separately."""
    fin = np.isfinite(exp) & np.isfinite(out)
    d = np.zeros(exp.shape, np.int64)
    d[fin] = np.abs(_ordered(out[fin]) - _ordered(exp[fin]))
    return d


def _check_ulps(out, exp, bound, msg):
    np.testing.assert_array_equal(np.isnan(out), np.isnan(exp), err_msg=f"NaN positions: {msg}")
    np.testing.assert_array_equal(np.isposinf(out), np.isposinf(exp), err_msg=f"+inf positions: {msg}")
    np.testing.assert_array_equal(np.isneginf(out), np.isneginf(exp), err_msg=f"-inf positions: {msg}")
    d = ulp_distance(out, exp)
    worst = int(d.max(initial=0))
    if worst > bound:
        i = int(np.argmax(d.reshape(-1, 2).max(axis=1)))
        raise AssertionError(f"{msg}: {worst} ulp > {bound}; at pixel {i}: device {out.reshape(-1, 2)[i].tolist()} "
                             f"numpy {exp.reshape(-1, 2)[i].tolist()}")
    return worst


def _forms(template):
    """The float32 form (Python-scalar constants) and the float64 form (numpy.float64 constants) of a template
    whose constants are written {like this}."""
    import re
    f32 = re.sub(r"\{([^}]*)\}", r"\1", template)
    f64 = re.sub(r"\{([^}]*)\}", r"numpy.float64(\1)", template)
    return [f32, f64]


DIVISORS = ("0.1", "-0.1", "0.2", "0.3", "-0.3", "0.5", "1.5", "-1.5", "7", "-7", "0.0", "-0.0")
EXACT_TEMPLATES = [
    "(r - {32}) + {0.1}", "r - {7.5}", "(r - {32}) * {0.3}", "(r - {32}) / {0.3}", "(r - {32}) / {0.0}",
    "(r - {32}) / {-0.0}", "-(r - {32})", "numpy.abs(r - {32})", "numpy.sqrt(r - {2})",
    "numpy.floor(r - {32.5})", "numpy.ceil((r - {32}) * {0.3})", "numpy.rint(r - {32})",
    "numpy.rint((r - {32}) * {0.1})", "numpy.sign(r - {2})", "numpy.square(r - {32})",
    "numpy.reciprocal(r - {32})", "numpy.minimum(r - {32}, {0.0})", "numpy.maximum(r - {32}, {-0.0})",
    "numpy.minimum({-0.0}, r - {32})", "numpy.clip(r - {32}, {-0.0}, {3.5})", "numpy.clip(r - {32}, {-3}, {0.0})",
    "numpy.where(r > {2}, r - {32}, {-0.0})", "numpy.where(r < {2.1}, {1.5}, r)",
    "numpy.where(r <= {2.1}, {1.5}, r)", "numpy.where(r >= {2.1}, {1.5}, r)", "numpy.where(r == {0.3}, {1.5}, r)",
    "numpy.where(r != {0.3}, r * {0.1}, {1.5})", "numpy.where(~(r >= {2.1}), r, {0.5})",
    "r * {1e-39}", "(r - {32}) * {1e-39} / {3}", "r * {1e-20} * {1e-20}",
] + [f"r // {{{d}}}" for d in DIVISORS] + [f"(r - {{32}}) // {{{d}}}" for d in DIVISORS] \
  + [f"r % {{{d}}}" for d in DIVISORS] + [f"(r - {{7}}) % {{{d}}}" for d in DIVISORS]
EXACT = [e for tpl in EXACT_TEMPLATES for e in _forms(tpl)] + [
    "r ** 2", "(r - 32) ** 2", "r ** 0.5", "(r - 32) ** -1", "r ** 1", "(r - 32) ** numpy.float64(2)",
    "(-r) ** 0.5", "(r - 32) ** numpy.float64(-1)",
    "(r > 2) + (r > 4)", "(r > 2) * (r < 40)", "(r > 2) * 1.5", "numpy.where(r > 2, 1, 0) * 2 - 1",
    "numpy.where(r > 2, True, False) * r", "(r > 2) / (r > 4)", "numpy.abs(r > 2) + r",
]


@pytest.fixture(scope="module")
def values_flow():
    return polar_flow(polar_values())


@pytest.mark.parametrize("er", EXACT)
def test_exact_opcodes_bit_for_bit(er, values_flow):
    out, exp = _run(er, "0", values_flow)
    _same_bits(out, exp, er)


def test_exact_opcodes_on_a_1080p_frame():
    """Volume: one 1080p frame of rounded and unrounded normal(0, 3) values through the division-like opcodes."""
    rng = np.random.default_rng(31)
    x = rng.normal(0, 3, 1080 * 1920).astype(np.float32)
    x[::2] = np.rint(x[::2])
    flow = polar_flow(x).reshape(1080, 1920, 2)
    for er in ("r // 0.1", "(r - 4) // 0.2", "(r - 4) % 0.1", "(r - 4) % numpy.float64(0.3)",
               "r // numpy.float64(0.1)", "numpy.clip(r - 3, -0.0, 2)", "numpy.rint(r * 0.5)"):
        out, exp = _run(er, "0", flow)
        _same_bits(out, exp, er)


# function -> (templates, largest distance observed on an MI355X, bound); distances in float32 ulps of the output.
# The observed maxima are those of the float32 forms (device sinf, expf, ... against numpy's float32 loops); every
# float64 form rounded to the same float32 as numpy's on all values (0 ulp).
ULP_BOUND = {
    "sin": (["numpy.sin(r - {32})", "numpy.sin(r * {0.1})"], 1, 2),
    "cos": (["numpy.cos(r - {32})", "numpy.cos(r * {0.1})"], 1, 2),
    "tan": (["numpy.tan(r - {32})", "numpy.tan(r * {0.1})"], 2, 4),
    "arcsin": (["numpy.arcsin((r - {32}) / {32})"], 2, 4),
    "arccos": (["numpy.arccos((r - {32}) / {32})"], 1, 2),
    "arctan": (["numpy.arctan(r - {32})"], 1, 2),
    "arctan2": (["numpy.arctan2(r - {32}, {-1.5})", "numpy.arctan2({-0.0}, r - {32})",
                 "numpy.arctan2({1.0}, r - {32})"], 2, 4),
    "exp": (["numpy.exp(r - {32})", "numpy.exp({-1} * r)"], 2, 4),
    "log": (["numpy.log(r - {1})"], 2, 4),
    "log2": (["numpy.log2(r - {1})"], 1, 2),
    "log10": (["numpy.log10(r - {1})"], 3, 4),
    "pow": (["numpy.power(r, {1.7})", "numpy.power(r - {32}, {3})", "numpy.power({2.0}, r - {32})",
             "(r - {32}) ** t", "numpy.power(r - {32}, {2})", "numpy.power(-r, {0.5})",
             "numpy.power(r - {32}, {-1})"], 1, 2),
    "hypot": (["numpy.hypot(r - {32}, {3.0})", "numpy.hypot(r, r * {1})"], 1, 2),
}


@pytest.mark.parametrize("fn", sorted(ULP_BOUND))
def test_transcendentals_within_ulps(fn, values_flow):
    templates, _, bound = ULP_BOUND[fn]
    for tpl in templates:
        f32, f64 = _forms(tpl)
        for er, b in ((f32, bound), (f64, 0)):          # float64 forms: observed 0, so no tolerance
            out, exp = _run(er, "0", values_flow)
            _check_ulps(out, exp, b, er)


# angle programs of each kind with radius programs of each kind: (radius, theta, wide_trig, wide_product, bound)
THETA_CASES = [
    ("numpy.float32(1)", "r * 0.37 + a", False, False, 2),          # observed 1
    ("numpy.float64(1)", "r * 0.37 + a", False, True, 2),           # observed 1
    ("numpy.float32(1)", "r * numpy.float64(0.37) + a", True, True, 0),
    ("numpy.float64(1)", "r * numpy.float64(0.37) + a", True, True, 0),
    ("numpy.float32(1)", "t * 3", True, True, 0),
    ("numpy.float64(1)", "t * 3", True, True, 0),
    ("1", "r * 0.37 + a", False, False, 2),                         # observed 1
    ("r * 0.5", "numpy.float32(t)", False, False, 0),
    ("r * numpy.float64(0.5)", "a - r * 0.1", False, True, 4),      # observed 2
]


@pytest.mark.parametrize("er,ea,wide_trig,wide_product,bound", THETA_CASES)
def test_theta_side_and_output_flags(er, ea, wide_trig, wide_product, bound, values_flow):
    from transflow_amd.exprs import PolarFilter
    _, _, wt, wp = PolarFilter(er, ea).programs(T)
    assert (wt, wp) == (wide_trig, wide_product)
    flow = values_flow[:, np.abs(values_flow[0, :, 0]) < 1e6]       # finite angles: sin of +-inf is NaN on both sides
    out, exp = _run(er, ea, flow)
    _check_ulps(out, exp, bound, f"{er} : {ea}")
