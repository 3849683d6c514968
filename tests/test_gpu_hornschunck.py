"""Horn-Schunck on the GPU against the reference's function (tests/golden/hs_*.npz, captured from it) and against the
numpy restatement (tests/hs_ref.py), bit for bit: flows are compared as int32 bit patterns, stopping iterations equal."""
import glob
import hashlib
import os

import numpy as np
import pytest

from oracle import remap_ref as R
from tests import hs_ref
from tests.helpers import GOLDEN, synth_pair

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


def _case_args(z):
    alpha = int(z["alpha"]) if bool(z["alpha_is_int"]) else float(z["alpha"])
    decay = int(z["decay"]) if bool(z["decay_is_int"]) else float(z["decay"])
    delta = float(z["delta"]) if bool(z["has_delta"]) else None
    return dict(alpha=alpha, max_iters=int(z["max_iters"]), decay=decay, delta=delta)


GOLDEN_CASES = sorted(glob.glob(os.path.join(GOLDEN, "hs_*.npz")))


@pytest.mark.parametrize("path", GOLDEN_CASES, ids=[os.path.basename(p)[3:-4] for p in GOLDEN_CASES])
def test_matches_reference_fixture(path):
    from transflow_amd.hornschunck import HornSchunck
    z = np.load(path)
    prev, nxt = z["prev"], z["next"]
    h, w = prev.shape
    hs = HornSchunck(w, h)
    flow_in = z["flow_in"] if "flow_in" in z.files else None
    out = hs.calc(prev, nxt, None if flow_in is None else flow_in.copy(), **_case_args(z))
    if "flow_out" in z.files:
        assert _bits_equal(out, z["flow_out"])
    else:
        assert hashlib.sha256(out.tobytes()).hexdigest() == z["flow_sha256"].item().decode()
        assert _bits_equal(out.reshape(-1, 2)[z["sample_index"]], z["flow_sample"])
    assert hs.last_stats(0)["iterations"] == int(z["iters_run"])
    hs.close()


def _pair(h, w, seed):
    return synth_pair(h, w, seed=seed, shift=(2.5, 1.5), noise=5.0)


def _init_flow(h, w, seed):
    return np.random.default_rng(seed).normal(0, 1.0, (h, w, 2)).astype(np.float32)


@pytest.mark.parametrize("chain", ["f64", "f32"])
@pytest.mark.parametrize("decay", [0, 0.95])
def test_matches_restatement_1080p(chain, decay):
    from transflow_amd.hornschunck import HornSchunck
    h, w = 1080, 1920
    a, b = _pair(h, w, 31)
    flow = _init_flow(h, w, 32) if chain == "f32" else None
    hs = HornSchunck(w, h)
    out = hs.calc(a, b, None if flow is None else flow.copy(), alpha=1, max_iters=3, decay=decay, delta=1)
    exp, n = hs_ref.horn_schunck(a, b, flow, 1, 3, decay, 1, return_iters=True)
    assert _bits_equal(out, exp)
    assert hs.last_stats(0)["iterations"] == n
    hs.close()


@pytest.mark.parametrize("chain,decay,delta", [("f64", 0, None), ("f32", 0, None), ("f32", 0.95, None), ("f64", 0.95, None),
                                               ("f32", 0.95, 1)])
def test_matches_restatement_4k(chain, decay, delta):
    from transflow_amd.hornschunck import HornSchunck
    h, w = 2160, 3840
    a, b = _pair(h, w, 41)
    flow = _init_flow(h, w, 42) if chain == "f32" else None
    hs = HornSchunck(w, h)
    out = hs.calc(a, b, None if flow is None else flow.copy(), alpha=1, max_iters=3, decay=decay, delta=delta)
    exp, n = hs_ref.horn_schunck(a, b, flow, 1, 3, decay, delta, return_iters=True)
    assert _bits_equal(out, exp)
    assert hs.last_stats(0)["iterations"] == n
    hs.close()


@pytest.mark.parametrize("alpha", [1, 0.5, 3])
def test_stage_derivatives(alpha):
    from transflow_amd.hornschunck import HornSchunck
    h, w = 123, 211
    a, b = _pair(h, w, 51)
    hs = HornSchunck(w, h)
    ex, ey, et, den = hs.stage_derivatives(a, b, alpha)
    rex, rey, ret = hs_ref.derivatives(a, b)
    for got, exp in ((ex, rex), (ey, rey), (et, ret), (den, hs_ref.denominator(rex, rey, alpha))):
        assert _bits_equal(got, exp)
    hs.close()


def _rank1_plus_noise(h, w, sigma, noise, dtype, seed):
    """A field whose spectral norm (as numpy computes it in `dtype`) is sigma, within numpy's rounding."""
    rng = np.random.default_rng(seed)
    x, y = rng.normal(size=h), rng.normal(size=w)
    m = np.outer(x / np.linalg.norm(x), y / np.linalg.norm(y)) + noise * rng.normal(size=(h, w)) / np.sqrt(h + w)
    m = m.astype(dtype)
    return (m * (sigma / np.linalg.norm(m, 2))).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("noise", [1e-3, 0.5])
@pytest.mark.parametrize("rel", [1 + 1e-2, 1 - 1e-2])
def test_norm_test_decides_on_the_device_away_from_delta(dtype, noise, rel):
    from transflow_amd.hornschunck import stage_norm_test
    delta = 2.5
    m = _rank1_plus_noise(300, 517, delta * rel, noise, dtype, seed=int(noise * 1000) + int(rel * 100))
    dec, stage = stage_norm_test(m, delta)
    assert stage in (0, 1, 2), (dec, stage)
    assert dec == int(np.linalg.norm(m, 2) < delta)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rel", [1 + 1e-4, 1 - 1e-4])
def test_norm_test_leaves_the_guard_band_to_the_host(dtype, rel):
    from transflow_amd.hornschunck import stage_norm_test
    delta = 2.5
    m = _rank1_plus_noise(300, 517, delta * rel, 0.5, dtype, seed=7)
    assert stage_norm_test(m, delta) == (-1, 3)


def test_norm_test_non_finite_goes_to_the_host():
    from transflow_amd.hornschunck import stage_norm_test
    m = np.zeros((40, 60))
    m[3, 4] = np.nan
    assert stage_norm_test(m, 1.0) == (-1, 3)
    m[3, 4] = np.inf
    assert stage_norm_test(m, 1.0) == (-1, 3)
    assert stage_norm_test(np.zeros((40, 60), np.float32), 1.0) == (1, 0)


def test_nan_delta_raises_linalgerror_as_the_reference():
    from transflow_amd.hornschunck import HornSchunck
    h, w = 37, 53
    a, b = _pair(h, w, 61)
    flow = _init_flow(h, w, 62)
    flow[10, 10, 0] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        hs_ref.horn_schunck(a, b, flow.copy(), 1, 3, 0.95, 1)
    hs = HornSchunck(w, h)
    with pytest.raises(np.linalg.LinAlgError):
        hs.calc(a, b, flow.copy(), alpha=1, max_iters=3, decay=0.95, delta=1)
    # delta None: no norm, the NaN just spreads -- to the same places (NaN payloads are not compared: x86 and the GPU
    # propagate different ones); every other value bit for bit
    out = hs.calc(a, b, flow.copy(), alpha=1, max_iters=3, decay=0.95, delta=None)
    exp = hs_ref.horn_schunck(a, b, flow.copy(), 1, 3, 0.95, None)
    nan = np.isnan(exp)
    assert nan.any() and np.array_equal(np.isnan(out), nan)
    assert _bits_equal(np.where(nan, 0, out), np.where(nan, 0, exp))
    hs.close()


def test_batch_equals_single_calls():
    from transflow_amd.hornschunck import HornSchunck
    h, w, n = 96, 128, 5
    frames = [_pair(h, w, 70 + i)[i % 2] for i in range(n + 1)]
    inits = [None if i % 2 == 0 else _init_flow(h, w, 80 + i) for i in range(n)]
    kw = dict(alpha=1, max_iters=40, decay=0.95, delta=0.05)
    batch = HornSchunck(w, h, frame_slots=n + 1, max_pairs=n)
    for s, f in enumerate(frames):
        batch.set_frame(s, f)
    for p in range(n):
        batch.set_initial_flow(p, inits[p])
    batch.calc_slots(list(range(n)), list(range(1, n + 1)), **kw)
    single = HornSchunck(w, h)
    iters = set()
    for p in range(n):
        exp = single.calc(frames[p], frames[p + 1], inits[p], **kw)
        assert _bits_equal(batch.get_flow(p), exp), p
        assert batch.last_stats(p) == single.last_stats(0)
        iters.add(single.last_stats(0)["iterations"])
        ref, k = hs_ref.horn_schunck(frames[p], frames[p + 1], inits[p], return_iters=True, **kw)
        assert _bits_equal(exp, ref) and k == single.last_stats(0)["iterations"]
    batch.close()
    single.close()


def test_bgr_ingest_equals_grey_ingest():
    from transflow_amd.flowops import bgr_to_grey
    from transflow_amd.hornschunck import HornSchunck
    h, w = 64, 80
    rng = np.random.default_rng(90)
    f0, f1 = (rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2))
    hs = HornSchunck(w, h)
    hs.set_frame_bgr(0, f0)
    hs.set_frame_bgr(1, f1)
    hs.set_initial_flow(0, None)
    hs.calc_slots([0], [1])
    got = hs.get_flow(0)
    exp = hs.calc(bgr_to_grey(f0), bgr_to_grey(f1))
    assert _bits_equal(got, exp)
    hs.close()


def _frames(h, w, n, seed=5):
    return [synth_pair(h, w, seed=seed, shift=(0.8 * i, 0.5 * i))[1] for i in range(n)]


@pytest.mark.parametrize("direction,decay,repeat,lock", [
    ("forward", 0, 1, None), ("backward", 0.95, 1, None), ("backward", 0.95, 2, None), ("forward", 0.95, 2, None),
    ("backward", 0.95, 1, "0.1,0.1")])
def test_flow_source_matches_host_loop(direction, decay, repeat, lock):
    """HipFlowSource with a HornSchunckConfig against the same source whose next() runs the restatement and whose
    post_process is the oracle's mirror: the reference's recurrence (each call starts from the post-processed previous
    flow; a rewind returns to flow=None) on both sides."""
    from transflow_amd.config import HornSchunckConfig
    from transflow_amd.flow import ArrayFrameProvider, FlowSource, HipFlowSource
    h, w = 60, 84
    frames = _frames(h, w, 5)
    cfg = HornSchunckConfig(hs_decay=decay, hs_iterations=6, hs_delta=0.5)
    d = R.FORWARD if direction == "forward" else R.BACKWARD

    class HostLoop(HipFlowSource):
        def next(self):
            frame = self.provider.read()
            if frame is None:
                raise StopIteration
            prev = self._prev_frame
            left, right = (prev, frame) if self.direction == FlowSource.Direction.FORWARD else (frame, prev)
            self._prev_frame = frame
            return hs_ref.horn_schunck(left, right, self.prev_flow.copy() if self.prev_flow is not None else None,
                                       **cfg.hs_kwargs())

        def post_process(self, raw):
            return R.post_process(raw, d)

    kw = dict(direction=direction, cv_config=cfg, repeat=repeat)
    if lock:
        kw.update(lock_expr=lock, lock_mode="stay")
    with HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), **kw) as source:
        got = [f.copy() for f in source]
    with HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), **kw) as oracle:
        oracle.__class__ = HostLoop
        exp = [f.copy() for f in oracle]
    assert len(got) == len(exp) >= 4 * repeat     # (a stay lock lengthens the output)
    for g, e in zip(got, exp):
        assert _bits_equal(g, e)
