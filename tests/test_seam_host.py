"""transflow_amd/seam.py on the CPU: the lazy magnitude chain answers exactly the pipeline's expression and gives
numpy's own values and types to every other use; and the restatements the GPU tests lean on (tests/seam_cases.py)
equal what the reference returned (tests/golden/seam.npz)."""
import os

import numpy as np
import pytest

from tests import flow_ops_cases as K
from tests import seam_cases as S
from tests.helpers import GOLDEN
from tests.test_flow_ops_cases import render_compared
from transflow_amd import deviceflow, seam
from transflow_amd.deviceflow import DeviceFlow

ZS = np.load(os.path.join(GOLDEN, "seam.npz"))


def _flow(h=5, w=7, seed=0, dtype=np.float32):
    a = np.random.default_rng(seed).normal(0, 2, (h, w, 2)).astype(dtype)
    f = DeviceFlow(a.shape, 0xdead0000, None, dtype=dtype)
    f._host = a.copy()          # as if it had been brought down
    return f, a


@pytest.fixture
def device_view(monkeypatch):
    monkeypatch.setattr(deviceflow, "DEVICE_VIEW", True)


def _same(got, want):
    assert type(got) is type(want) and got.dtype == want.dtype and got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def test_the_pipelines_chain_is_lazy_and_its_values_are_numpys(device_view):
    f, a = _flow()
    sq = np.power(f, 2)
    s = np.sum(sq, axis=2)
    m = np.sqrt(s)
    assert type(sq) is seam.FlowSquares and type(s) is seam.FlowSquareSum and type(m) is seam.FlowMagnitude
    assert m.flow is f and m.resident
    assert (sq.shape, s.shape, m.shape) == (a.shape, a.shape[:2], a.shape[:2]) and m.dtype == np.float32 and m.ndim == 2
    assert type(np.sum(np.power(f, 2), 2)) is seam.FlowSquareSum and type(np.power(f, 2.0)) is seam.FlowSquares
    assert type(np.power(f, np.float32(2))) is seam.FlowSquares
    _same(np.asarray(sq), np.power(a, 2))
    _same(np.asarray(s), np.sum(np.power(a, 2), axis=2))
    _same(np.asarray(m), np.sqrt(np.sum(np.power(a, 2), axis=2)))
    assert not m.resident                                    # its host values exist now: the view takes those


def test_every_other_use_gives_numpys_values_and_types(device_view):
    f, a = _flow(seed=1)
    _same(np.power(f, 3), np.power(a, 3))
    _same(np.power(f, np.float64(2)), np.power(a, np.float64(2)))          # a float64 result: not the pipeline's chain
    _same(np.power(2, f), np.power(2, a))
    _same(np.power(f, 2, dtype=np.float64), np.power(a, 2, dtype=np.float64))
    out = np.empty_like(a)
    assert np.power(f, 2, out=out) is out
    _same(out, np.power(a, 2))
    sq = np.power(f, 2)
    _same(np.sum(sq, axis=0), np.sum(np.power(a, 2), axis=0))
    _same(np.sum(np.power(f, 2), axis=2, keepdims=True), np.sum(np.power(a, 2), axis=2, keepdims=True))
    _same(np.sum(np.power(f, 2)), np.sum(np.power(a, 2)))
    _same(np.power(f, 2) + 1, np.power(a, 2) + 1)
    s = np.sum(np.power(f, 2), axis=2)
    _same(np.sqrt(s) + 1, np.sqrt(np.sum(np.power(a, 2), axis=2)) + 1)
    _same(s * 2, np.sum(np.power(a, 2), axis=2) * 2)
    _same(np.square(s), np.square(np.sum(np.power(a, 2), axis=2)))
    m = np.sqrt(np.sum(np.power(f, 2), axis=2))
    _same(m[1:3], np.sqrt(np.sum(np.power(a, 2), axis=2))[1:3])
    _same(np.clip(m, 0, 1), np.clip(np.sqrt(np.sum(np.power(a, 2), axis=2)), 0, 1))
    assert m.max() == np.sqrt(np.sum(np.power(a, 2), axis=2)).max() and len(m) == a.shape[0]


def test_flows_the_device_route_does_not_take_are_not_lazy(device_view):
    f, a = _flow(seed=2)
    f *= 2                                                   # modified on the host: the device copy is stale
    _same(np.power(f, 2), np.power(a * 2, 2))
    f64, a64 = _flow(seed=3, dtype=np.float64)
    _same(np.power(f64, 2), np.power(a64, 2))


def test_with_the_switch_off_nothing_lazy_appears():
    f, a = _flow(seed=4)
    assert deviceflow.DEVICE_VIEW is False
    _same(np.power(f, 2), np.power(a, 2))
    _same(np.sqrt(np.sum(np.power(f, 2), axis=2)), np.sqrt(np.sum(np.power(a, 2), axis=2)))


def test_what_the_device_route_serves():
    f, _ = _flow()
    g, _ = _flow(seed=1)
    assert seam.is_resident(f) and seam._served("sum", [f, g]) and seam._served("absmax", [f, g])
    assert seam.merge("first", [f, g]) is f                  # the reference's flows[0]
    assert not seam._served("absmax", [f, g, f]) and not seam._served("sum", [f] * 9) and not seam._served("sum", [])
    assert not seam._served("sum", [f, np.zeros(f.shape, np.float32)]) and not seam._served("median", [f, g])
    assert not seam._served("sum", [f, _flow(h=6)[0]]) and not seam._served("sum", [f, _flow(dtype=np.float64)[0]])
    g *= 2
    assert not seam.is_resident(g) and not seam._served("sum", [f, g])


def test_the_fixture_holds_one_output_per_case_and_nothing_else():
    assert sorted(ZS.files) == sorted(c["name"] for c in S.fused_cases() + S.magnitude_cases())
    assert os.path.getsize(os.path.join(GOLDEN, "seam.npz")) <= 1 << 20


def test_fused_restatement_equals_the_reference():
    with np.errstate(all="ignore"):
        for c in S.fused_cases():
            assert K.same_values(S.fused_form(c, S.fused_inputs(c)), ZS[c["name"]]), c["name"]
    shapes = {(c["h"], c["w"]) for c in S.fused_cases()}
    factors = {(c["wf"], c["hf"]) for c in S.fused_cases()}
    assert shapes == {(1, 1), (5, 3), (9, 31), (2, 129)} and factors == {(3, 2), (2, 3), (1, 5), (7, 1), (2, 1)}
    assert {(w * wf) % 2 for (h, w) in shapes for (wf, hf) in factors} == {0, 1} and max(w * wf for (h, w) in shapes for (wf, hf) in factors) > 2 * 256


@pytest.mark.filterwarnings("ignore:invalid value encountered in cast")
def test_magnitude_restatement_equals_the_reference():
    S.assert_magnitude_cases_reach_their_targets()
    with np.errstate(all="ignore"):
        for c in S.magnitude_cases():
            flow = S.magnitude_input(c["n"], c["scale"], c["nans"])
            assert K.same_bits(S.magnitude_form(flow), np.sqrt(np.sum(np.power(flow, 2), axis=2))), c["name"]
            keep = render_compared(c, c["n"])
            assert c["n"] - keep.sum() <= 3
            assert K.same_bits(S.magnitude_view_form(c, flow)[0, keep], ZS[c["name"]][0, keep]), c["name"]
    planted = [c for c in S.magnitude_cases() if c["nans"]]
    assert planted and all(np.isnan(S.magnitude_input(c["n"], c["scale"], True)[0, list(K.nan_pixels(c["n"]))]).any(axis=1).all() for c in planted)
