"""dropin.install(device_seam=True): the pipeline's merge, upscale and flow views keep a DeviceFlow on the device
(transflow_amd/seam.py) and give what the originals give; everything else goes to the originals.  The pipeline module
here is a stand-in with the names install() replaces, the oracle's functions standing where the reference's do: the
tests need no installed transflow."""
import sys
import types

import numpy as np
import pytest

from oracle import flow_ops_ref as F
from tests import flow_ops_cases as K

pytestmark = pytest.mark.gpu
KINDS = ("first", "sum", "average", "difference", "product", "maskbin", "masklin", "absmax")


def _device_flow(array, in_frame=False):
    from transflow_amd.device import DevBuffer
    from transflow_amd.deviceflow import DeviceFlow, _Event
    array = np.ascontiguousarray(array)
    buf = DevBuffer.from_array(array)
    ev = _Event()
    ev.record()
    flow = DeviceFlow(array.shape, buf.ptr, ev, owner=buf, dtype=array.dtype)
    flow.in_frame = in_frame
    return flow


def _field(h, w, seed):
    return np.random.default_rng(seed).normal(0, 1.5, (h, w, 2)).astype(np.float32)


@pytest.fixture
def pipeline(monkeypatch):
    package, module = types.ModuleType("transflow"), types.ModuleType("transflow.pipeline")
    package.pipeline, package.__path__ = module, []
    module.upscale_array = F.upscale
    module.render1d = lambda arr, scale=1, colors=None, binary=False: F.render1d(arr, scale, colors or K.R1_DEFAULT, binary)
    module.render2d = lambda arr, scale=1, colors=None: F.render2d(arr, scale, colors or K.R2_DEFAULT)

    class Pipeline:
        FLOW_MERGING_FUNCTIONS = {kind: (lambda flows, kind=kind: F.merge(kind, flows)) for kind in KINDS}

    class VideoOutput:                       # (install(jpeg_frames=...) wraps this factory too; no test here calls it)
        @classmethod
        def from_args(cls, path, width, height, **kwargs):
            raise NotImplementedError

    module.Pipeline = Pipeline
    output, video_output = types.ModuleType("transflow.output"), types.ModuleType("transflow.output.video_output")
    package.output, output.video_output, output.__path__, video_output.VideoOutput = output, video_output, [], VideoOutput
    for name, m in (("transflow", package), ("transflow.pipeline", module), ("transflow.output", output),
                    ("transflow.output.video_output", video_output)):
        monkeypatch.setitem(sys.modules, name, m)
    return module


@pytest.fixture
def installed(pipeline):
    from transflow_amd import dropin
    originals = types.SimpleNamespace(upscale_array=pipeline.upscale_array, render1d=pipeline.render1d,
                                      render2d=pipeline.render2d, merging=dict(pipeline.Pipeline.FLOW_MERGING_FUNCTIONS))

    def install(**options):
        dropin.install(flow=False, compositor=False, device_seam=True, **options)
        return originals
    try:
        yield install
    finally:
        dropin.uninstall()


def test_install_replaces_the_four_names_and_uninstall_restores_them(pipeline):
    from transflow_amd import deviceflow, dropin
    merging = pipeline.Pipeline.FLOW_MERGING_FUNCTIONS
    before = (pipeline.upscale_array, pipeline.render1d, pipeline.render2d, dict(merging))
    assert deviceflow.DEVICE_VIEW is False
    dropin.install(flow=False, compositor=False)
    assert (pipeline.upscale_array, pipeline.render1d, pipeline.render2d, dict(merging)) == before       # off by default
    dropin.install(flow=False, compositor=False, device_seam=True)
    try:
        assert deviceflow.DEVICE_VIEW is True and pipeline.Pipeline.FLOW_MERGING_FUNCTIONS is merging
        assert pipeline.upscale_array is not before[0] and pipeline.render1d is not before[1] and pipeline.render2d is not before[2]
        assert set(merging) == set(KINDS) and all(merging[k] is not before[3][k] for k in KINDS)
    finally:
        dropin.uninstall()
    assert pipeline.upscale_array is before[0] and pipeline.render1d is before[1] and pipeline.render2d is before[2]
    assert pipeline.Pipeline.FLOW_MERGING_FUNCTIONS is merging and all(merging[k] is before[3][k] for k in KINDS)
    assert deviceflow.DEVICE_VIEW is False


def test_device_flows_stay_on_the_device(pipeline, installed):
    """Fails without the feature: the originals bring the flows down and return arrays."""
    from transflow_amd.deviceflow import DeviceFlow
    orig = installed()
    a, b, c = _field(9, 31, 1), _field(9, 31, 2), _field(9, 31, 3)
    b[2, 3] = (0.2, -0.2)                                    # maskbin's threshold, and a tie for absmax
    a[2, 4], b[2, 4] = (1.5, -0.0), (-1.5, 0.0)
    merging = pipeline.Pipeline.FLOW_MERGING_FUNCTIONS
    for kind, hosts in (("sum", (a, b, c)), ("maskbin", (a, b, c)), ("absmax", (a, b)), ("average", (a, b, c)),
                        ("difference", (a, b)), ("product", (a, b)), ("masklin", (a, b))):
        flows = [_device_flow(h) for h in hosts]
        got = merging[kind](flows)
        assert isinstance(got, DeviceFlow) and got.shape == a.shape and got.dtype == np.float32, kind
        assert got._host is None and all(f._host is None for f in flows), kind
        assert K.merge_same(kind, np.asarray(got), orig.merging[kind](list(hosts))), kind
    flow = _device_flow(a)
    up = pipeline.upscale_array(flow, 3, 2)
    assert isinstance(up, DeviceFlow) and up.shape == (18, 93, 2) and up._host is None and flow._host is None
    assert K.same_values(np.asarray(up), orig.upscale_array(a, 3, 2))
    both = pipeline.upscale_array(merging["sum"]([_device_flow(a), _device_flow(b)]), 2, 2)    # pipeline.py:502-504
    assert isinstance(both, DeviceFlow) and K.same_values(np.asarray(both), orig.upscale_array(orig.merging["sum"]([a, b]), 2, 2))
    first = [_device_flow(a), _device_flow(b)]
    assert merging["first"](first) is first[0]


def test_every_other_operand_goes_to_the_original(pipeline, installed):
    from transflow_amd.deviceflow import DeviceFlow
    orig = installed()
    a, b = _field(5, 7, 4), _field(5, 7, 5)
    merging = pipeline.Pipeline.FLOW_MERGING_FUNCTIONS
    got = merging["sum"]([_device_flow(a), b])                                   # one ndarray operand
    assert type(got) is np.ndarray and K.same_values(got, orig.merging["sum"]([a, b]))
    flow = _device_flow(a)
    flow *= 2                                                                     # written on the host
    got = merging["sum"]([flow, _device_flow(b)])
    assert type(got) is np.ndarray and K.same_values(got, orig.merging["sum"]([a * 2, b]))
    got = pipeline.upscale_array(flow, 2, 3)
    assert type(got) is np.ndarray and K.same_values(got, orig.upscale_array(a * 2, 2, 3))
    wide = _device_flow(a.astype(np.float64))                                     # a float64 flow
    got = pipeline.upscale_array(wide, 2, 3)
    assert type(got) is np.ndarray and K.same_values(got, orig.upscale_array(a.astype(np.float64), 2, 3))
    got = merging["product"]([wide, _device_flow(b)])
    assert type(got) is np.ndarray and K.same_values(got, orig.merging["product"]([a.astype(np.float64), b]))
    nine = [_device_flow(_field(5, 7, 10 + i)) for i in range(9)]                 # more than the kernel takes
    got = merging["sum"](nine)
    assert type(got) is np.ndarray and K.same_values(got, orig.merging["sum"]([np.asarray(f) for f in nine]))
    with pytest.raises(ValueError):                                               # shapes that differ: the original's error
        merging["sum"]([_device_flow(a), _device_flow(_field(5, 8, 6))])
    assert type(pipeline.upscale_array(a, 2, 2)) is np.ndarray
    assert type(pipeline.render2d(a, 0.5)) is np.ndarray and type(pipeline.render1d(a[:, :, 0], 0.5)) is np.ndarray


class _HostSource:
    def __init__(self, array, introduction_mask):
        self.array, self.introduction_mask, self.counter = array, introduction_mask, -1

    def next(self, timeout=1):
        self.counter += 1
        return self.array

    @property
    def frame_number(self):
        return self.counter


def _compositor(h, w):
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    comp = HipCompositor.from_args(h, w, [LayerConfig(0)], background_color="#204060")
    pixmap = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
    comp.set_sources({0: [_HostSource(pixmap, np.ones((h, w), bool))]})
    return comp


def _small_in_frame_flows(count=3, h=6, w=8):
    from oracle import remap_ref as OR
    rng = np.random.default_rng(7)
    return [OR.post_process(rng.normal(0, 2.5, (h, w, 2)).astype(np.float32), OR.BACKWARD) for _ in range(count)]


def test_in_frame_is_kept_through_first_and_the_upscale_and_cleared_by_a_merge(pipeline, installed):
    orig = installed()
    merging = pipeline.Pipeline.FLOW_MERGING_FUNCTIONS
    small = _small_in_frame_flows()
    a, b = _device_flow(small[0], in_frame=True), _device_flow(small[1], in_frame=True)
    assert merging["first"]([a, b]).in_frame and pipeline.upscale_array(a, 3, 2).in_frame
    assert pipeline.upscale_array(merging["first"]([a, b]), 3, 2).in_frame
    assert merging["sum"]([a]).in_frame                                            # one flow: the flow itself
    assert not merging["sum"]([a, b]).in_frame and not pipeline.upscale_array(merging["sum"]([a, b]), 3, 2).in_frame
    assert not pipeline.upscale_array(_device_flow(small[0]), 3, 2).in_frame      # nothing promised, nothing gained
    # the upscaled in-frame flow drives a moveref layer without the check, and the frames are the host route's
    frames = {}
    for route in ("device", "host"):
        comp = _compositor(12, 24)
        try:
            out = []
            for f in small:
                flow = pipeline.upscale_array(_device_flow(f, in_frame=True), 3, 2) if route == "device" else orig.upscale_array(f, 3, 2)
                assert (route == "device") == hasattr(flow, "dev_ptr")
                comp.update(flow)
                out.append(np.array(comp.render()))
            frames[route] = out
        finally:
            comp.close()
    assert len(frames["device"]) == 3 and (frames["device"][0] != frames["device"][2]).any()
    for got, want in zip(frames["device"], frames["host"]):
        assert got.tobytes() == want.tobytes()
    # a merged flow that leaves the frame: update() says so, as it does for a host array
    far = np.full((12, 24, 2), 20, np.float32)
    merged = merging["sum"]([_device_flow(far, in_frame=True), _device_flow(far, in_frame=True)])
    comp = _compositor(12, 24)
    try:
        with pytest.raises(IndexError):
            comp.update(merged)
    finally:
        comp.close()


def test_views_return_the_originals_pixels(pipeline, installed):
    orig = installed()
    a = _field(17, 33, 8)
    a[0, :4] = [(0, 0), (2, 0), (0, -2), (1.2, 1.6)]
    for scale, colors in ((0.5, None), (-0.25, K.R2_COLORS)):
        flow = _device_flow(a)
        got = pipeline.render2d(flow, scale, colors)
        assert flow._host is None and type(got) is np.ndarray and got.dtype == np.uint8
        assert np.array(got).tobytes() == orig.render2d(a, scale, colors).tobytes()
    for scale, colors, binary in ((0.5, None, False), (0.5, K.R1_COLORS, True), (0.25, K.R1_COLORS, False)):
        flow = _device_flow(a)
        mag = np.sqrt(np.sum(np.power(flow, 2), axis=2))                          # pipeline.py:515
        got = pipeline.render1d(mag, scale, colors, binary)                       # :516
        assert flow._host is None and type(got) is np.ndarray
        assert np.array(got).tobytes() == orig.render1d(np.sqrt(np.sum(np.power(a, 2), axis=2)), scale, colors, binary).tobytes()
    flow = _device_flow(a)
    mag = np.sqrt(np.sum(np.power(flow, 2), axis=2))
    assert float(mag[0, 3]) == 2.0                                                 # read on the host: the original renders it
    assert np.array(pipeline.render1d(mag, 0.5)).tobytes() == orig.render1d(np.sqrt(np.sum(np.power(a, 2), axis=2)), 0.5).tobytes()


def test_views_leave_in_the_compositors_frame_form(pipeline, installed):
    from transflow_amd.device import DevBuffer
    from transflow_amd.jpeg import JpegEncoder, JpegFrame
    from transflow_amd.remap import CompImage
    orig = installed(jpeg_frames=90)
    a = _field(32, 48, 9) * np.float32(2)
    flow = _device_flow(a)
    frames = [pipeline.render2d(flow, 0.5), pipeline.render1d(np.sqrt(np.sum(np.power(flow, 2), axis=2)), 0.25)]
    pixels = [orig.render2d(a, 0.5), orig.render1d(np.sqrt(np.sum(np.power(a, 2), axis=2)), 0.25)]
    assert flow._host is None
    enc = JpegEncoder(32, 48, 90)
    try:
        for frame, px in zip(frames, pixels):
            assert isinstance(frame, JpegFrame) and frame.shape == (32, 48, 3) and frame.quality == 90
            buf = DevBuffer(px.nbytes)
            comp = CompImage(32, 48, image_dev=buf.ptr)      # (creating it paints the background)
            buf.upload(px)
            try:
                assert np.array_equal(comp.download(), px)
                assert frame.data == enc.frame(comp).data
            finally:
                comp.close()
                buf.close()
    finally:
        enc.close()


def test_an_upscaled_flow_reaches_the_archive_without_coming_down(pipeline, tmp_path):
    """With device_flow_export: numpy.round(flow).astype(int) of the upscaled DeviceFlow (pipeline.py:506) is computed
    on the device too."""
    from transflow_amd import archive, dropin
    from transflow_amd.flowzip import DeviceInt64Flow
    pipeline.NumpyOutput = archive.NumpyOutput
    a = _field(6, 8, 11) * np.float32(3)
    dropin.install(flow=False, compositor=False, device_seam=True, device_flow_export=True)
    try:
        flow = _device_flow(a)
        up = pipeline.upscale_array(flow, 2, 2)
        rounded = np.round(up).astype(int)
        assert isinstance(rounded, DeviceInt64Flow) and up._host is None and flow._host is None
        np.testing.assert_array_equal(np.asarray(rounded), np.round(F.upscale(a, 2, 2)).astype(int))
    finally:
        dropin.uninstall()
