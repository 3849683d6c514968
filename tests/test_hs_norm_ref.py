"""CPU checks of the float64 model of Horn-Schunck's staged convergence test (tests/hs_norm_ref.py) over the sweep that
the GPU tests run (tests/test_gpu_hs_norm.py): the model is sound against numpy.linalg.norm(m, 2), its longdouble form
agrees with it, and the sweep reaches every stage in every orientation."""
import numpy as np
import pytest

from tests import hs_norm_ref as N


@pytest.fixture(scope="module")
def cases():
    """[(family, (h, w), dtype, field, float64 values, sigma)] of the sweep, computed once; numpy's own sigma, in the
    field's dtype as the reference takes it, goes with the field."""
    out = []
    for family, shape, dtype, m in N.sweep():
        out.append((family, shape, dtype, (m, np.linalg.norm(m, 2)), N.values(m), float(np.linalg.norm(m.astype(np.float64), 2))))
    return out


def test_sweep_is_the_one_the_issue_lists(cases):
    assert len(cases) == len(N.SHAPES) * len(N.FAMILIES) * len(N.DTYPES) - 4      # zerosum of 1x1 and 300x1 is zero
    assert {N.orientation(*s) for s in N.SHAPES} == {"portrait", "landscape", "square"}


def test_bounds_are_sound(cases):
    for family, shape, dtype, m, v, sigma in cases:
        for x in v.lower():
            assert x <= sigma * (1 + 1e-12), (family, shape, dtype)
        for x in v.upper():
            assert x >= sigma * (1 - 1e-12), (family, shape, dtype)


def test_decision_is_numpys_or_undecided(cases):
    for family, shape, dtype, m, v, sigma in cases:
        for rel in N.RELS:
            delta = sigma / rel
            dec, stage = N.decide(v, delta)
            assert dec in (N.UNDECIDED, int(m[1] < delta)), (family, shape, dtype, rel)
            assert (stage == N.ST_HOST) == (dec == N.UNDECIDED)
            if rel in N.GUARD_BAND_RELS:
                assert (dec, stage) == (N.UNDECIDED, N.ST_HOST), (family, shape, dtype, rel)


def test_no_comparand_sits_on_its_threshold(cases):
    """The GPU test may leave a case out when a comparand is within 1e-9 of its threshold: none is."""
    closest = min(N.comparand_margin(v, sigma / rel) for _, _, _, _, v, sigma in cases for rel in N.RELS)
    assert closest > 1e-6, closest


def test_power_bounds_do_not_decrease(cases):
    for family, shape, dtype, m, v, sigma in cases:
        if family != "zerosum":        # there the start vector is orthogonal to du: amplified rounding noise
            assert (v.power[1:] >= v.power[:-1] * (1 - 1e-12)).all(), (family, shape, dtype)


def test_every_stage_decides_in_every_orientation(cases):
    seen = set()
    for family, shape, dtype, m, v, sigma in cases:
        for rel in N.RELS:
            seen.add((N.orientation(*shape),) + N.decide(v, sigma / rel))
    for o in ("portrait", "landscape", "square"):
        for outcome in ((N.CONVERGED, N.ST_BOUNDS), (N.NOT_CONVERGED, N.ST_BOUNDS), (N.NOT_CONVERGED, N.ST_POWER),
                        (N.CONVERGED, N.ST_GRAM), (N.UNDECIDED, N.ST_HOST)):
            assert (o,) + outcome in seen, (o, outcome)


def test_corner_needs_the_higher_gram_powers(cases):
    """q equal singular values: the Gram bound of k is sigma q^(1 / 4k) -- for q = 5, 1.495, 1.223 and 1.106 sigma.  So
    sigma = 0.9 delta is certified by k = 4 alone, and sigma = 0.8 delta by k = 2 (1.223 * 0.8 < 1 - GUARD), not by
    k = 1."""
    n = 0
    for family, shape, dtype, m, v, sigma in cases:
        if family == "corner" and min(shape) >= 5:
            n += 1
            np.testing.assert_allclose(v.gram / sigma, 5.0 ** (1 / np.array([4.0, 8.0, 16.0])), rtol=1e-6)
            assert N.decide(v, sigma / 0.9) == (N.CONVERGED, N.ST_GRAM) and N.gram_k(v, sigma / 0.9) == 4
            assert N.decide(v, sigma / 0.8) == (N.CONVERGED, N.ST_GRAM) and N.gram_k(v, sigma / 0.8) == 2
    assert n == 20


def test_longdouble_model_agrees(cases):
    """The yardstick of the GPU test: the same code in longdouble, here on the shapes that take no time."""
    worst = 0.0
    for family, shape, dtype, m, v, sigma in cases:
        if shape[0] * shape[1] > 129 * 257:
            continue
        y = N.values(m[0], np.longdouble)
        for a, b in zip([v.F, v.U, v.L] + list(v.gram), [y.F, y.U, y.L] + list(y.gram)):
            worst = max(worst, abs(float(a / b) - 1))
        if family != "zerosum":
            worst = max(worst, float(np.abs(v.power / y.power - 1).max()))
    assert worst < 1e-13, worst


def test_special_deltas_and_magnitudes():
    m = N.field("noise", 9, 200, np.float64)
    v = N.values(m)
    for delta in (0.0, -1.0, float("nan")):
        assert N.decide(v, delta) == (N.NOT_CONVERGED, N.ST_BOUNDS)
    assert N.decide(v, float("inf")) == (N.CONVERGED, N.ST_BOUNDS)
    big = N.values(m * 1e170)
    assert big.nonfinite and N.decide(big, 1.0) == (N.UNDECIDED, N.ST_HOST)
    for scale in (1e-170, 1e-300):
        t = N.values(m * scale)
        sigma = float(np.linalg.norm(m * scale, 2))
        assert t.tiny and t.U >= sigma
        for rel in (0.5, 2):
            assert N.decide(t, sigma / rel)[0] in (N.UNDECIDED, int(sigma < sigma / rel))
