"""With `resident_steps` a convolution kernel and polar filters ride the resident tail (FlowSource._post_process_steps): Farnebäck's own tail,
Horn-Schunck's out-of-place tail with its chain buffer (hip_resident), and MotionVectorFlowSource.  Every case is the
source as it is against a second source of the same configuration whose read_next_flow is the base class's: that one
takes the raw flows from the method handle as host arrays and hands them to FlowSource.post_process, the route from
before this path existed (pinned by the goldens of tests/test_gpu_flow_ops.py and test_gpu_postprocess.py, and the only
yardstick for `polar`, whose trigonometry is the device's).  Flows, their dtype and a chaining method's whole sequence
must agree bit for bit; with DeviceFlows nothing comes down and the compositor's frames are those of the host arrays."""
import numpy as np
import pytest

from tests import mv_ref
from tests.helpers import synth_pair

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (64, 96)]
N_FRAMES = 6
POLAR = "scale=1.5;polar=r*1.25+t:a+0.5;clip=4"


def _frames(h, w):
    return [synth_pair(h, w, seed=5, shift=(0.8 * i, 0.5 * i))[1] for i in range(N_FRAMES)]


def _mask(h, w):
    m = np.random.default_rng(6).choice([0.0, 0.5, 1.0], (h, w)).astype(np.float32)
    m[:, : w // 3] = 0
    return m[..., np.newaxis]


def _kernel(dtype):
    return np.random.default_rng(7).normal(0, 0.6, (3, 5)).astype(dtype)


# option -> (kernel, filters, masked)
OPTIONS = {"kernel f64": (_kernel(np.float64), None, False), "kernel f32": (_kernel(np.float32), None, False),
           "scale polar clip": (None, POLAR, False), "polar kernel mask": (_kernel(np.float64), POLAR, True)}
SOURCES = ("farneback", "horn-schunck", "horn-schunck masked", "motion vectors")


def _builder(kind, h, w, direction, option, device_flows=False, config_keys=None, **extra):
    """A builder whose mask and kernel are set as arrays (the paths name files)."""
    from transflow_amd.config import FlowConfig, HornSchunckConfig
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    from transflow_amd.motionvectors import ArrayVectorProvider
    kernel, filters, masked = OPTIONS[option]
    mask = _mask(h, w) if (masked or kind.endswith("masked")) else None
    kw = dict(direction=direction, flow_filters=filters, resident_steps=True)
    kw.update(extra)
    if kind == "motion vectors":
        tables = [mv_ref.h264_like(w, h, seed=50 + i, intra=0.3) for i in range(N_FRAMES)]
        builder = HipFlowSource.from_args(ArrayVectorProvider(tables, w, h, 25.0), use_mvs=True, **kw)
        builder.device_flows = device_flows
    else:
        keys = dict(hip_device_flows=device_flows, **(config_keys or {}))
        cfg = FlowConfig(**keys) if kind == "farneback" else HornSchunckConfig(
            hs_decay=0.95, hs_iterations=6, hs_delta=0.5, hip_resident=True, **keys)
        builder = HipFlowSource.from_args(ArrayFrameProvider(_frames(h, w), 25.0), cv_config=cfg, **kw)
    base = type(builder)

    class WithArrays(base):
        def _load_inputs(self):
            base._load_inputs(self)
            self.mask, self.kernel = mask, kernel
    builder.__class__ = WithArrays
    return builder


def _host_route(source):
    """The same source, taking the route FlowSource.__next__ has for a source that is not resident."""
    from transflow_amd.flow import FlowSource
    cls = type(source)
    source.__class__ = type("HostRoute", (cls,), {"read_next_flow": FlowSource.read_next_flow})


_EXPECTED = {}


def _expected(kind, h, w, direction, option):
    key = (kind, h, w, direction, option)
    if key not in _EXPECTED:
        with _builder(kind, h, w, direction, option) as source:
            _host_route(source)
            flows = [np.array(f, copy=True) for f in source]
        for f in flows:
            f.flags.writeable = False
        _EXPECTED[key] = flows
    return _EXPECTED[key]


def _same(got, exp, what):
    assert len(got) == len(exp) == N_FRAMES - 1, what
    for k, (g, e) in enumerate(zip(got, exp)):
        g = np.asarray(g)
        assert g.dtype == e.dtype and g.shape == e.shape, f"{what}, flow {k}: {g.dtype} for {e.dtype}"
        assert g.tobytes() == e.tobytes(), f"{what}, flow {k}: {int((g != e).sum())} values differ"


class _Pixmaps:
    def __init__(self, h, w):
        self.introduction_mask = np.ones((h, w), bool)
        self.pix = np.random.default_rng(8).integers(0, 256, (h, w, 3), dtype=np.uint8)

    def next(self, timeout=1):
        return self.pix


def _compositors(h, w):
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    comps = [HipCompositor.from_args(h, w, [LayerConfig(0)]), HipCompositor.from_args(h, w, [LayerConfig(0, classname="sum")])]
    for comp in comps:
        comp.set_sources({0: [_Pixmaps(h, w)]})
    return comps


def _render_all(flows, h, w, check=None):
    """The frames of a moveref and a sum compositor fed `flows`."""
    comps = _compositors(h, w)
    frames = []
    for flow in flows:
        for comp in comps:
            comp.update(flow)
            frames.append(comp.render().copy())
            if check is not None:
                check(flow)
    return frames


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("kind", SOURCES)
def test_resident_tail_equals_the_host_route(kind, h, w, direction, option):
    from transflow_amd.deviceflow import DeviceFlow
    exp = _expected(kind, h, w, direction, option)
    kernel = OPTIONS[option][0]
    want = np.dtype(np.float32) if kernel is None else np.result_type(np.float32, kernel.dtype)
    assert all(e.dtype == want for e in exp)

    with _builder(kind, h, w, direction, option) as source:
        assert source._resident_ok()
        got = [np.array(f, copy=True) for f in source]
        if kind.startswith("horn-schunck"):
            assert source.chain_valid
    _same(got, exp, "host arrays")

    def on_device(flow):
        assert flow._host is None, "the flow came down"

    with _builder(kind, h, w, direction, option, device_flows=True) as source:
        flows = []
        for flow in source:
            assert isinstance(flow, DeviceFlow) and flow.dtype == want and flow.in_frame and flow.nbytes == exp[0].nbytes
            flows.append(flow)
        dev_frames = _render_all(flows, h, w, on_device)
        assert all(f._host is None for f in flows)
        _same(flows, exp, "device flows")                        # (they come down here, once each)
    host_frames = _render_all(exp, h, w)
    assert len(dev_frames) == len(host_frames) == 2 * (N_FRAMES - 1)
    for k, (a, b) in enumerate(zip(dev_frames, host_frames)):
        np.testing.assert_array_equal(a, b, err_msg=f"frame {k // 2} of the {'sum' if k % 2 else 'moveref'} layer")


def test_sum_layer_floors_a_float64_device_flow():
    """The sum layer takes floor(flow) in double and the moving layers rint(flow): on a float64 DeviceFlow of halves the
    two differ, and each equals what the host branch makes of the same array."""
    from transflow_amd.device import DevBuffer
    from transflow_amd.deviceflow import DeviceFlow
    h, w = 37, 53
    flow = np.zeros((h, w, 2), np.float64)
    flow[5:20, 5:30, 0] = 1.4999999999          # rint 1, floor 1; as a float32 it is 1.5: rint 2
    flow[20:30, 5:30, 0] = -0.5                 # rint -0, floor -1
    flow[5:30, 30:40, 1] = 2.5                  # rint 2, floor 2
    buf = DevBuffer.from_array(flow)
    try:
        dev = DeviceFlow(flow.shape, buf.ptr, None, dtype=np.float64)
        dev.in_frame = True
        assert dev.nbytes == flow.nbytes and dev.dtype == np.float64
        got = _render_all([dev, dev], h, w)
        assert dev._host is None
        exp = _render_all([flow, flow], h, w)
        for a, b in zip(got, exp):
            np.testing.assert_array_equal(a, b)
        assert not np.array_equal(got[2], got[3])            # moveref and sum moved differently
        narrow = _render_all([flow.astype(np.float32)] * 2, h, w)
        assert not np.array_equal(narrow[2], exp[2])          # rounding the float32 cast is another frame
        assert np.asarray(dev).dtype == np.float64 and np.asarray(dev).tobytes() == flow.tobytes()
        assert np.round(dev).tobytes() == np.round(flow).tobytes()
    finally:
        buf.close()


@pytest.mark.parametrize("kind", ["farneback", "horn-schunck"])
def test_lock_expression_keeps_the_host_route(kind):
    h, w = 37, 53
    kw = dict(lock_expr="(0.08,0.08),(100,0)", lock_mode="stay")
    with _builder(kind, h, w, "backward", "kernel f64", **kw) as source:
        assert not source._resident_ok()
        got = [np.array(f, copy=True) for f in source]
    with _builder(kind, h, w, "backward", "kernel f64", **kw) as source:
        _host_route(source)
        exp = [np.array(f, copy=True) for f in source]
    assert len(got) == len(exp) >= N_FRAMES - 1
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype == np.float64 and g.tobytes() == e.tobytes()


@pytest.mark.parametrize("kind", SOURCES)
def test_without_resident_steps_the_host_route_stays(kind):
    """The argument is an opt-in: off, a kernel or a polar filter sends the source down the host route, with the same
    flows."""
    h, w = 37, 53
    for option in ("kernel f64", "scale polar clip"):
        with _builder(kind, h, w, "backward", option, resident_steps=False) as source:
            assert not source._resident_ok()
            got = [np.array(f, copy=True) for f in source]
        _same(got, _expected(kind, h, w, "backward", option), f"{option}, off")


def test_farneback_batch_with_a_kernel():
    """hip_batch: three pairs a call, each pair's flow convolved out of the handle's buffer of that pair."""
    h, w = 64, 96
    flows = {}
    for batch in (1, 3):
        with _builder("farneback", h, w, "forward", "kernel f64", config_keys={"hip_batch": batch}) as source:
            assert source._resident_ok() and source._batch_size() == batch
            flows[batch] = [np.array(f, copy=True) for f in source]
    _same(flows[3], flows[1], "a batch of three against one")
    assert flows[1][0].dtype == np.float64


ARCHIVE_FRAMES = 3


def _flow_archive(tmp_path, h, w):
    """An indexed archive of float32 flows, and the flows."""
    from transflow_amd.archive import DeviceFlowArchiveWriter
    rng = np.random.default_rng(21)
    flows = [rng.normal(0, 3, (h, w, 2)).astype(np.float32) for _ in range(ARCHIVE_FRAMES)]
    path = str(tmp_path / "clip.flow.zip")
    with DeviceFlowArchiveWriter(path, index=True) as out:
        out.write_meta({"path": "clip.mp4", "width": w, "height": h, "framerate": 25.0, "direction": 1, "seek_time": None})
        for f in flows:
            out.write_array(f)
    return path, flows


@pytest.mark.parametrize("device_flows", [False, True])
def test_archive_replay_with_a_kernel_and_a_polar_filter(tmp_path, device_flows):
    """ArchiveFlowSource(device_inflate=True): the member is inflated on the device and filtered, masked and convolved
    there; against the same archive read the host's way."""
    from transflow_amd.archive import ArchiveFlowSource
    from transflow_amd.flow import FlowFilter
    h, w = 37, 53
    path, _ = _flow_archive(tmp_path, h, w)
    kernel, mask = OPTIONS["kernel f64"][0], _mask(h, w)

    def run(**kw):
        builder = ArchiveFlowSource.Builder(path, **kw)
        builder.build()
        builder.mask, builder.kernel = mask, kernel
        builder.flow_filters = [FlowFilter.from_string(part) for part in POLAR.split(";")]
        source = builder.cls(*builder.args(), **builder.kwargs())
        try:
            out = []
            for _ in range(ARCHIVE_FRAMES):
                flow = next(source)
                out.append((source._resident_ok(), type(flow).__name__, np.array(flow, copy=True)))
            return out
        finally:
            source.close()
    exp = run()
    got = run(device_inflate=True, device_flows=device_flows, resident_steps=True)
    assert all(not r for r, _, _ in exp) and all(r for r, _, _ in got)
    assert all(name == ("DeviceFlow" if device_flows else "ndarray") for _, name, _ in got)
    for k, ((_, _, g), (_, _, e)) in enumerate(zip(got, exp)):
        assert g.dtype == e.dtype == np.float64 and g.tobytes() == e.tobytes(), f"flow {k}"


@pytest.mark.parametrize("rounded", [False, True])
def test_float64_device_flow_through_the_archive_writer(tmp_path, rounded):
    """The export of a float64 DeviceFlow: unrounded it is deflated where it is (the member is numpy's float64 array);
    rounded it comes down and numpy rounds it -- the device's rounding reads float32 flows only."""
    import zipfile

    from transflow_amd.archive import DeviceFlowArchiveWriter, read_archive_frame
    from transflow_amd.device import DevBuffer
    from transflow_amd.deviceflow import DeviceFlow
    from transflow_amd.flowzip import round_i64_dev
    h, w = 37, 53
    flow = np.random.default_rng(22).normal(0, 3, (h, w, 2))
    flow[0, :4, 0] = (0.5, 1.5, 2.5, 1.4999999999)
    flow[1, :2, 1] = (-0.5, -0.0)
    buf = DevBuffer.from_array(flow)
    path = str(tmp_path / "f64.flow.zip")
    try:
        dev = DeviceFlow(flow.shape, buf.ptr, None, dtype=np.float64)
        with DeviceFlowArchiveWriter(path) as out:
            out.write_array(dev, rounded=rounded)
        assert (dev._host is None) == (not rounded)
        with zipfile.ZipFile(path) as zf:
            got = read_archive_frame(zf, 0)
        exp = np.round(flow).astype(int) if rounded else flow
        assert got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()
        with pytest.raises(TypeError):
            round_i64_dev(dev)
    finally:
        buf.close()


def test_float64_device_flow_crosses_a_process_boundary_as_the_array():
    import pickle
    from multiprocessing.reduction import ForkingPickler
    h, w = 37, 53
    with _builder("motion vectors", h, w, "backward", "kernel f64", device_flows="ipc") as source:
        flow = next(source)
        assert flow.dtype == np.float64 and flow._cross is None
        back = pickle.loads(bytes(ForkingPickler.dumps(flow)))
        assert isinstance(back, np.ndarray) and back.dtype == np.float64
        assert back.tobytes() == _expected("motion vectors", h, w, "backward", "kernel f64")[0].tobytes()
        assert pickle.loads(pickle.dumps(flow)).tobytes() == back.tobytes()
