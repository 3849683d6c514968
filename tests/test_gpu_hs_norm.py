"""The device's staged convergence test of Horn-Schunck (transflow_amd/csrc/hs_norm.hip and the fused partial sums of
k_hs_iterate) against the numpy model tests/hs_norm_ref.py: every value of every stage against the model in longdouble,
every decision and deciding stage against the model's rule, on shapes that reach one pixel, one row, one column, ragged
strips, column blocks, tiles and k-slices and both orientations of the Gram matrix, and on fields whose mass sits in the
last row, the last column or the bottom-right corner, where a lost tail shows.

Measured on an MI355X (worst |device - longdouble model| over the allowance 64 max(|float64 model - longdouble model|,
2^-53 value), over the sweep): power bounds 0.064, Gram bounds 0.095; F, U, L over H W 2^-53: 0.0056."""
import functools

import numpy as np
import pytest

from tests import hs_norm_ref as N
from tests import hs_ref
from tests.helpers import synth_pair

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
LD = np.longdouble


def _name(dtype):
    return np.dtype(dtype).name


@functools.lru_cache(maxsize=None)
def _field(family, h, w, dtype_name):
    return N.field(family, h, w, np.dtype(dtype_name).type)


@functools.lru_cache(maxsize=None)
def _model64(family, h, w, dtype_name):
    """(float64 model values, sigma in float64, numpy's own sigma in the field's dtype) -- computed once, shared."""
    m = _field(family, h, w, dtype_name)
    return N.values(m), float(np.linalg.norm(m.astype(np.float64), 2)), np.linalg.norm(m, 2)


CASES = [(f, h, w, _name(d)) for h, w in N.SHAPES for f in N.FAMILIES for d in N.DTYPES if N.field(f, h, w, d) is not None]
SHAPE_CASES = [(h, w, _name(d)) for h, w in N.SHAPES for d in N.DTYPES]


def _check_values(got, m, family, sigma):
    """The device's values of du = m against the model.  Prints the measured ratios, then asserts."""
    h, w = m.shape
    v64, vld = N.values(m), N.values(m, LD)
    ratios = {}
    # F, U, L: sums of H W non-negative doubles, in any order
    dev = np.array([got["F"], got["U"], got["L"]], LD)
    ref = np.array([vld.F, vld.U, vld.L], LD)
    ratios["bounds"] = float((np.abs(dev - ref) / (ref * (h * w * EPS))).max())

    def ratio(dev, m64, mld):
        allow = 64 * np.maximum(np.abs(m64.astype(LD) - mld), EPS * mld)
        return float((np.abs(dev.astype(LD) - mld) / allow).max())

    ratios["gram"] = ratio(got["gram"], v64.gram, vld.gram)
    if family != "zerosum":
        ratios["power"] = ratio(got["power"], v64.power, vld.power)
    print("HSNORM values %s %dx%d %s: " % (family, h, w, m.dtype.name) + " ".join("%s=%.3g" % kv for kv in sorted(ratios.items())))
    assert np.isfinite(got["power"]).all() and np.isfinite(got["gram"]).all()
    for stage, r in ratios.items():
        assert r <= 1, (stage, r)
    if family == "zerosum":   # the start vector is orthogonal to du: the power bounds are amplified rounding, but still sound
        assert (got["power"] <= sigma * (1 + 1e-12)).all()
        assert got["L"] <= sigma * (1 + 1e-12)


@pytest.mark.parametrize("family,h,w,dtype", CASES, ids=["%s-%dx%d-%s" % c for c in CASES])
def test_values_match_the_longdouble_model(family, h, w, dtype):
    from transflow_amd.hornschunck import stage_norm_values
    m = _field(family, h, w, dtype)
    _check_values(stage_norm_values(m, None), m, family, _model64(family, h, w, dtype)[1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=_name)
def test_values_of_a_difference_rounded_in_the_chains_dtype(dtype):
    """u_new = u_old + field, so that u_new - u_old rounds in float32: the model gets that difference."""
    from transflow_amd.hornschunck import stage_norm_values
    h, w = 65, 63
    u_old = (3.0 * np.random.default_rng(77).normal(size=(h, w))).astype(dtype)
    u_new = (u_old + N.field("edges", h, w, dtype)).astype(dtype)
    du = u_new - u_old
    assert du.dtype == dtype
    if dtype == np.float32:
        assert not np.array_equal(du, N.field("edges", h, w, dtype))      # (the difference did round)
    _check_values(stage_norm_values(u_new, u_old), du, "edges", float(np.linalg.norm(du.astype(np.float64), 2)))


@pytest.mark.parametrize("h,w,dtype", SHAPE_CASES, ids=["%dx%d-%s" % c for c in SHAPE_CASES])
def test_decisions_and_stages_are_the_models(h, w, dtype):
    from transflow_amd.hornschunck import stage_norm_test
    left_out = 0
    n = 0
    for family in N.FAMILIES:
        m = _field(family, h, w, dtype)
        if m is None:
            continue
        v, sigma, np_sigma = _model64(family, h, w, dtype)
        for rel in N.RELS:
            delta = sigma / rel
            if N.comparand_margin(v, delta) < 1e-9:
                left_out += 1
                continue
            n += 1
            got = stage_norm_test(m, delta)
            exp = N.decide(v, delta)
            if rel in N.GUARD_BAND_RELS:
                assert exp == (N.UNDECIDED, N.ST_HOST)
            if family == "zerosum" and rel not in N.GUARD_BAND_RELS:      # its power stage is rounding noise
                assert got[0] in (N.UNDECIDED, int(np_sigma < delta)), (family, rel, got)
                assert (got[1] == N.ST_HOST) == (got[0] == N.UNDECIDED)
            else:
                assert got == exp, (family, rel, got, exp)
    assert left_out == 0 and n >= 6 * len(N.RELS)


@pytest.mark.parametrize("h,w", [(9, 200), (200, 9), (65, 63)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=_name)
def test_special_deltas_follow_numpys_comparison(h, w, dtype):
    from transflow_amd.hornschunck import stage_norm_test
    m = _field("noise", h, w, _name(dtype))
    sigma = np.linalg.norm(m, 2)
    for delta in (0.0, -1.0, float("nan"), float("inf")):
        assert stage_norm_test(m, delta) == (int(sigma < delta), N.ST_BOUNDS), delta


@pytest.mark.parametrize("h,w", [(9, 200), (200, 9), (65, 63)])
@pytest.mark.parametrize("scale", [1e-170, 1e-300])
def test_tiny_float64_fields_are_numpys_or_the_hosts(h, w, scale):
    """|du|^2 underflows: F and the sums of squares are lost, and must not be taken for a small norm."""
    from transflow_amd.hornschunck import stage_norm_test, stage_norm_values
    for family in N.FAMILIES:
        m = _field(family, h, w, "float64") * scale
        sigma = float(np.linalg.norm(m, 2))
        assert sigma > 0
        got = stage_norm_values(m, None)
        assert got["U"] >= sigma * (1 - 1e-12)
        for rel in (0.5, 2):
            delta = sigma / rel
            dec, stage = stage_norm_test(m, delta)
            assert dec in (N.UNDECIDED, int(sigma < delta)), (family, rel, dec, stage)
            assert (stage == N.ST_HOST) == (dec == N.UNDECIDED)


@pytest.mark.parametrize("h,w", [(9, 200), (200, 9), (65, 63)])
def test_huge_float64_fields_go_to_the_host(h, w):
    from transflow_amd.hornschunck import stage_norm_test
    for family in N.FAMILIES:
        m = _field(family, h, w, "float64") * 1e170
        sigma = float(np.linalg.norm(m, 2))
        for rel in (0.5, 2):
            assert stage_norm_test(m, sigma / rel) == (N.UNDECIDED, N.ST_HOST), (family, rel)


# ---- the partial sums that k_hs_iterate fuses -------------------------------------------------------------------------
ALPHA, DECAY, TINY_DELTA = 1, 0.95, 1e-30
FUSED_SHAPES = [(1, 1), (1, 300), (300, 1), (32, 256), (33, 257), (65, 513)]


def _pair(h, w, seed):
    return synth_pair(h, w, seed=seed, shift=(2.5, 1.5), noise=5.0)


def _init_flow(h, w, seed):
    return np.random.default_rng(seed).normal(0, 1.0, (h, w, 2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _fused_case(h, w, chain, k, seed):
    """(prev, next, initial flow or None, iterations the reference runs, F, U, L of its last du in longdouble)."""
    a, b = _pair(h, w, seed)
    flow = _init_flow(h, w, seed + 1) if chain == "f32" else None
    n = hs_ref.horn_schunck(a, b, flow, ALPHA, k, DECAY, TINY_DELTA, return_iters=True)[1]
    du = hs_ref.delta_u_at(a, b, flow, ALPHA, n, DECAY)
    assert du.dtype == (np.float32 if chain == "f32" else np.float64)
    return a, b, flow, n, N.bounds(du, LD)


def _assert_bounds(got, exp, h, w):
    for g, e in zip(got, exp):
        assert abs(LD(g) - e) <= h * w * EPS * e, (got, exp)


@pytest.mark.parametrize("h,w", FUSED_SHAPES, ids=["%dx%d" % s for s in FUSED_SHAPES])
@pytest.mark.parametrize("chain", ["f64", "f32"])
@pytest.mark.parametrize("k", [1, 3])
def test_fused_partials_give_the_bounds_of_the_last_difference(h, w, chain, k):
    from transflow_amd.hornschunck import HornSchunck
    a, b, flow, n, exp = _fused_case(h, w, chain, k, 100 + h + w)
    hs = HornSchunck(w, h)
    hs.calc(a, b, None if flow is None else flow.copy(), alpha=ALPHA, max_iters=k, decay=DECAY, delta=TINY_DELTA)
    stats = hs.last_stats(0)
    assert stats["iterations"] == n and stats["bounds"] == n and stats["host"] == 0
    if exp[0] > 0:
        assert n == k           # a field that moves is NOT_CONVERGED against 1e-30 every time
    _assert_bounds(hs.last_bounds(0), exp, h, w)
    hs.calc(a, b, None, alpha=ALPHA, max_iters=k, decay=DECAY, delta=None)
    with pytest.raises(ValueError):
        hs.last_bounds(0)       # no delta: no check was made
    hs.close()


@pytest.mark.parametrize("h,w", [(1, 300), (33, 257), (65, 513)], ids=["1x300", "33x257", "65x513"])
def test_fused_partials_of_a_batch_are_each_pairs_own(h, w):
    """Three pairs, f64, f32, f64, in a handle of four: the pair-indexed strides of the partials and the blocks in both
    launch lists."""
    from transflow_amd.hornschunck import HornSchunck
    k = 3
    cases = [_fused_case(h, w, chain, k, 100 + h + w + 10 * i) for i, chain in enumerate(("f64", "f32", "f64"))]
    batch = HornSchunck(w, h, frame_slots=6, max_pairs=4)
    for i, (a, b, flow, n, exp) in enumerate(cases):
        batch.set_frame(2 * i, a)
        batch.set_frame(2 * i + 1, b)
        batch.set_initial_flow(i, None if flow is None else flow.copy())
    batch.calc_slots([0, 2, 4], [1, 3, 5], alpha=ALPHA, max_iters=k, decay=DECAY, delta=TINY_DELTA)
    single = HornSchunck(w, h)
    for i, (a, b, flow, n, exp) in enumerate(cases):
        assert batch.last_stats(i)["iterations"] == n
        got = batch.last_bounds(i)
        _assert_bounds(got, exp, h, w)
        single.calc(a, b, None if flow is None else flow.copy(), alpha=ALPHA, max_iters=k, decay=DECAY, delta=TINY_DELTA)
        assert np.array(got).tobytes() == np.array(single.last_bounds(0)).tobytes(), i
    with pytest.raises(ValueError):
        batch.last_bounds(3)    # not a pair of the call
    batch.close()
    single.close()


# ---- portrait frames end to end -------------------------------------------------------------------------------------
def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


@pytest.mark.parametrize("anchor", [0, 1], ids=["f64-at-delta", "f32-at-delta"])
@pytest.mark.parametrize("rel", [0.99, 1.01])
def test_portrait_pairs_stop_where_the_reference_stops(anchor, rel):
    """200 x 90 frames (H > W: the Gram matrix is built on the transposed side), three pairs f64, f32, f64 in one call,
    delta at sigma_4 / rel of pair `anchor`: bit-equal flows, equal iteration counts, and the stage that the model names
    for every check."""
    from transflow_amd.hornschunck import HornSchunck
    h, w, iters = 200, 90, 8
    pairs = []
    for i, chain in enumerate(("f64", "f32", "f64")):
        a, b = _pair(h, w, 300 + i)
        pairs.append((a, b, _init_flow(h, w, 310 + i) if chain == "f32" else None))
    a, b, flow = pairs[anchor]
    delta = hs_ref.sigma_max(hs_ref.delta_u_at(a, b, flow, ALPHA, 4, DECAY)) / rel
    hs = HornSchunck(w, h, frame_slots=6, max_pairs=3)
    for i, (a, b, flow) in enumerate(pairs):
        hs.set_frame(2 * i, a)
        hs.set_frame(2 * i + 1, b)
        hs.set_initial_flow(i, None if flow is None else flow.copy())
    hs.calc_slots([0, 2, 4], [1, 3, 5], alpha=ALPHA, max_iters=iters, decay=DECAY, delta=delta)
    for i, (a, b, flow) in enumerate(pairs):
        exp, n = hs_ref.horn_schunck(a, b, flow, ALPHA, iters, DECAY, delta, return_iters=True)
        stats = hs.last_stats(i)
        assert _bits_equal(hs.get_flow(i), exp), i
        assert stats["iterations"] == n, i
        model = {"bounds": 0, "power": 0, "gram": 0, "host": 0}
        for k in range(1, n + 1):
            v = N.values(hs_ref.delta_u_at(a, b, flow, ALPHA, k, DECAY))
            assert N.comparand_margin(v, delta) > 1e-9
            model[("bounds", "power", "gram", "host")[N.decide(v, delta)[1]]] += 1
        assert {s: stats[s] for s in model} == model, (i, stats, model)
        if i == anchor:
            assert n == 4 if rel < 1 else n > 4     # sigma_4 on either side of delta
    hs.close()
