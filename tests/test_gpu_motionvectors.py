"""The GPU motion-vector painter (tf_mv_*, transflow_amd/motionvectors.py) against flows the reference painted
(tests/golden/mv_*.npz) and against the numpy restatement (tests/mv_ref.py).  Every comparison is on bit patterns: a
painted 0 is -0.0, an unpainted pixel +0.0, and no pixel is exempt."""
import glob
import itertools
import os

import numpy as np
import pytest

from oracle import flow_ops_ref as F
from oracle import remap_ref as R
from tests import mv_ref
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "mv_*.npz")))


def _same_bits(got, exp):
    np.testing.assert_array_equal(mv_ref.bits(got), mv_ref.bits(exp))


def _into(mv, vectors, h, w):
    """rasterize_into a device buffer that held NaNs, then downloaded."""
    from transflow_amd.device import DevBuffer
    buf = DevBuffer.from_array(np.full((h, w, 2), np.float32(np.nan)))
    try:
        mv.rasterize_into(vectors, buf.ptr)
        return buf.download((h, w, 2), np.float32)
    finally:
        buf.close()


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_fixtures_bit_identical(path):
    from transflow_amd.motionvectors import MotionVectors
    z = np.load(path)
    vectors = z["vectors"] if bool(z["has_vectors"]) else None
    w, h, flow = int(z["width"]), int(z["height"]), z["flow"]
    mv = MotionVectors(w, h)
    try:
        _same_bits(mv.rasterize(vectors), flow)
        _same_bits(_into(mv, vectors, h, w), flow)
        _same_bits(mv.rasterize(vectors, out=np.full((h, w, 2), np.float32(7))), flow)
    finally:
        mv.close()


def test_fixture_set():
    assert len(FIXTURES) >= 6


SIZES = [(1920, 1080), (3840, 2160), (1, 1), (300, 1), (53, 37)]      # width, height


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{h}x{w}" for w, h in SIZES])
def test_generators_against_the_restatement(w, h):
    from transflow_amd.motionvectors import MotionVectors
    mv = MotionVectors(w, h)
    try:
        n_hostile = 4000 if w * h > 10 ** 6 else 600
        for k, table in enumerate((mv_ref.h264_like(w, h, seed=31), mv_ref.hostile(w, h, n_hostile, seed=32),
                                   mv_ref.h264_like(w, h, seed=33, intra=0.6))):
            exp = mv_ref.paint(table, w, h)
            _same_bits(mv.rasterize(table), exp)
            if k == 0:
                _same_bits(_into(mv, table, h, w), exp)
    finally:
        mv.close()


def test_the_winner_map_cleans_itself():
    """Dense, sparse, nothing, dense again on ONE handle: a winner left behind by an earlier frame would show as a
    painted pixel where the later frame has none (or as another vector's value)."""
    from transflow_amd.motionvectors import MotionVectors
    w, h = 854, 480
    dense = mv_ref.hostile(w, h, 1500, seed=41)
    sparse = mv_ref.h264_like(w, h, seed=42, intra=0.9)
    shorter = dense[:40]                                   # fewer vectors than a stale winner would index
    mv = MotionVectors(w, h)
    try:
        for table in (dense, sparse, None, dense, shorter, None, sparse):
            _same_bits(mv.rasterize(table), mv_ref.paint(table, w, h))
    finally:
        mv.close()


def test_a_rejected_table_raises_and_leaves_the_handle_usable():
    from transflow_amd.motionvectors import MotionVectors
    w, h = 160, 120
    good = mv_ref.h264_like(w, h, seed=43)
    mv = MotionVectors(w, h)
    try:
        _same_bits(mv.rasterize(good), mv_ref.paint(good, w, h))
        bad = good.copy()
        bad["motion_scale"][5] = 0
        with pytest.raises(ValueError, match="vector 5 has motion_scale 0"):
            mv.rasterize(bad)
        bad = good.copy()
        bad["source"][7] = 1
        with pytest.raises(ValueError, match="vector 7 has source 1"):
            mv.rasterize(bad)
        _same_bits(mv.rasterize(good), mv_ref.paint(good, w, h))
    finally:
        mv.close()


def test_same_table_twice_gives_the_same_bytes():
    from transflow_amd.motionvectors import MotionVectors
    w, h = 1920, 1080
    table = mv_ref.hostile(w, h, 5000, seed=44)
    mv = MotionVectors(w, h)
    try:
        first = mv.rasterize(table)
        for _ in range(3):
            assert mv.rasterize(table).tobytes() == first.tobytes()
    finally:
        mv.close()


# ---- the flow source ---------------------------------------------------------------------------------------------

def _tables(w, h, n):
    out = [mv_ref.h264_like(w, h, seed=50 + i, intra=0.3) for i in range(n)]
    out[2] = None                                           # a frame without side data
    out[4] = mv_ref.hostile(w, h, 60, seed=59)
    return out


FILTERS = {"none": None, "scale": "scale=1.5+t", "threshold": "threshold=2", "polar": "polar=r*2:a*0"}
# a STAY lock from t = 0.1 s for 0.1 s; the second pair is never reached, but must exist: past its last pair the lock
# schedule raises IndexError, as the reference's does (source.py:304-307)
LOCK = "(0.1,0.1),(100,0)"
SWEEP = list(itertools.product(("forward", "backward"), ("none", "scale", "threshold"), (False, True), (1, 2),
                               (None, LOCK)))
# a polar filter is what sends a source without locks down the host path
SWEEP += [("forward", "polar", False, 1, None), ("backward", "polar", True, 2, None)]


@pytest.mark.parametrize("direction,filt,masked,repeat,lock", SWEEP)
def test_flow_source_matches_host_loop(direction, filt, masked, repeat, lock):
    """MotionVectorFlowSource against the same source whose next() is the restatement and whose post_process is the
    oracle's mirror of source.py:337-363 (filters in place, mask into a new array, direction handling, clip).  Without
    a lock and without a polar filter the source takes the resident path, otherwise the base class's host path."""
    from transflow_amd.flow import FlowSource, HipFlowSource
    from transflow_amd.motionvectors import ArrayVectorProvider, MotionVectorFlowSource
    w, h = 84, 60
    tables = _tables(w, h, 6)
    d = R.FORWARD if direction == "forward" else R.BACKWARD
    mask = np.random.default_rng(6).choice([0.0, 0.5, 1.0], (h, w)).astype(np.float32)[..., np.newaxis] if masked else None

    class MaskedBuilder(MotionVectorFlowSource.Builder):
        def _load_inputs(self):
            super()._load_inputs()
            self.mask = mask                                # (a mask_path names an image file or a shape rule)

    class HostLoop(MotionVectorFlowSource):
        def next(self):
            return mv_ref.paint(self.provider.read(), w, h)

        def read_next_flow(self):
            return FlowSource.read_next_flow(self)

        def post_process(self, raw):
            for f in self.flow_filters:
                if f.name == "polar":
                    r_expr, a_expr = f.expr_string.split(":")
                    F.polar(raw, r_expr, a_expr, self.t)
                else:
                    R.FILTERS[f.name](raw, f.expr(self.t))
            return R.post_process(R.pre_steps(raw, (), self.mask), d)

    kw = dict(use_mvs=True, direction=direction, repeat=repeat, flow_filters=FILTERS[filt])
    if lock:
        kw.update(lock_expr=lock, lock_mode="stay")

    def run(cls):
        builder = HipFlowSource.from_args(ArrayVectorProvider(tables, w, h, 25.0), **kw)
        assert type(builder) is MotionVectorFlowSource.Builder
        builder.__class__ = MaskedBuilder
        with builder as source:
            resident = source._resident_ok()
            if cls is not None:
                source.__class__ = cls
            return [np.array(f, copy=True) for f in source], resident

    got, resident = run(None)
    exp, _ = run(HostLoop)
    assert resident == (lock is None and filt != "polar")
    assert len(got) == len(exp) >= 5 * repeat           # (a stay lock lengthens the output)
    for g, e in zip(got, exp):
        assert g.dtype == np.float32 and g.shape == (h, w, 2)
        _same_bits(g, e)


@pytest.mark.parametrize("direction,masked,dtype", [("backward", True, np.float64), ("forward", False, np.float64),
                                                    ("backward", False, np.float32)])
def test_flow_source_with_a_convolution_kernel(direction, masked, dtype):
    """The third condition that takes the source off the resident path: a convolution kernel (source.py:344-348).  The
    painted flow comes down, is filtered and masked, convolved into a NEW array of the convolution's type, and the
    direction handling and the clip work on that; against the oracle's post_process_with_kernel, bit for bit.  (A
    convolution sums from +0.0, so it hands the clip no -0.0: +0.0 + -0.0 is +0.0.)"""
    from transflow_amd.motionvectors import ArrayVectorProvider, MotionVectorFlowSource
    w, h = 84, 60
    tables = _tables(w, h, 6)
    d = R.FORWARD if direction == "forward" else R.BACKWARD
    mask = np.random.default_rng(6).choice([0.0, 0.5, 1.0], (h, w)).astype(np.float32)[..., np.newaxis] if masked else None
    kernel = np.random.default_rng(7).normal(0, 0.3, (3, 5)).astype(dtype)

    class Builder(MotionVectorFlowSource.Builder):
        def _load_inputs(self):
            super()._load_inputs()
            self.mask, self.kernel = mask, kernel

    class HostLoop(MotionVectorFlowSource):
        def next(self):
            return mv_ref.paint(self.provider.read(), w, h)

        def post_process(self, raw):
            for f in self.flow_filters:
                R.FILTERS[f.name](raw, f.expr(self.t))
            return F.post_process_with_kernel(R.pre_steps(raw, (), self.mask), kernel, d)

    def run(cls):
        with Builder(ArrayVectorProvider(tables, w, h, 25.0), direction=direction, flow_filters="scale=1.5+t") as source:
            assert not source._resident_ok()
            if cls is not None:
                source.__class__ = cls
            return [np.array(f, copy=True) for f in source]

    got, exp = run(None), run(HostLoop)
    assert len(got) == len(exp) == 5
    bits = np.uint64 if dtype is np.float64 else np.uint32
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype == np.dtype(dtype) and g.shape == (h, w, 2)
        np.testing.assert_array_equal(np.ascontiguousarray(g).view(bits), np.ascontiguousarray(e).view(bits))


@pytest.mark.parametrize("direction", ["backward", "forward"])
def test_device_flows_stay_on_the_device_and_give_the_same_frames(direction):
    """device_flows=True: the source yields DeviceFlows, a HipCompositor (moveref, random reset from the device's
    generator: the same frames for the same seed) reads them in HBM, and flows and frames are those of the same run
    fed host arrays."""
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    from transflow_amd.deviceflow import DeviceFlow
    from transflow_amd.motionvectors import ArrayVectorProvider, MotionVectorFlowSource
    w, h = 168, 120
    tables = _tables(w, h, 6)
    pix = np.random.default_rng(8).integers(0, 256, (h, w, 3), dtype=np.uint8)

    class Src:
        introduction_mask = np.ones((h, w), bool)

        def next(self, timeout=1):
            return pix

    def run(device_flows):
        comp = HipCompositor.from_args(h, w, [LayerConfig(0, reset_mode="random", reset_random_factor=0.05)], rng="device")
        comp.set_sources({0: [Src()]})
        flows, images = [], []
        builder = MotionVectorFlowSource.Builder(ArrayVectorProvider(tables, w, h, 25.0), device_flows=device_flows,
                                                 direction=direction, flow_filters="scale=2")
        with builder as source:
            for flow in source:
                if device_flows:
                    assert isinstance(flow, DeviceFlow) and flow.shape == (h, w, 2) and flow.dtype == np.float32
                else:
                    assert isinstance(flow, np.ndarray)
                comp.update(flow)
                images.append(comp.render().copy())
                flows.append(flow)
            if device_flows:
                assert not any(f._host is not None for f in flows)       # nothing came down: the compositor read HBM
            flows = [np.array(f, copy=True) for f in flows]
        return flows, images

    plain_flows, plain_images = run(False)
    dev_flows, dev_images = run(True)
    assert len(plain_flows) == len(dev_flows) == 5
    assert any(f.any() for f in plain_flows)
    for a, b in zip(plain_images, dev_images):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(plain_flows, dev_flows):
        _same_bits(a, b)
    assert len({img.tobytes() for img in plain_images}) > 1              # the flows moved something
