"""PostProcess (transflow_amd/flowops.py): FlowSource.post_process on the device without a flow method's handle.  It gives
what a Farnebäck handle's post_process entries give, bit for bit, and the sources that have no resident flow method --
a subclass yielding host arrays, the motion-vector source -- never make a Farnebäck handle."""
import ctypes as C

import numpy as np
import pytest

from oracle import flow_ops_ref as F
from oracle import remap_ref as R
from tests import mv_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (37, 23), (64, 2), (257, 3)]      # (257, 3): past one 256-thread block, a width that is no power of two
CHAINS = {"weak": [("scale", 1.5), ("threshold", 0.75), ("clip", 4.0)],
          "float64": [("scale", np.float64(1.5)), ("threshold", np.float64(0.75)), ("clip", np.float64(4.0))]}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _flow(h, w, seed=21):
    rng = np.random.default_rng(seed)
    f = rng.normal(0, 3, (h, w, 2)).astype(np.float32)
    f[rng.random((h, w)) < 0.2] = np.float32(-0.0)
    return f


def _masks(h, w):
    rng = np.random.default_rng(22)
    return {"none": None, "binary": rng.choice(np.array([0.0, 1.0], np.float32), (h, w)),
            "fractional": rng.random((h, w)).astype(np.float32)}


@pytest.mark.parametrize("w,h", SHAPES)
def test_equals_a_farneback_handle(w, h):
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer
    from transflow_amd.farneback import Farneback
    from transflow_amd.flowops import PostProcess
    lib = _lib.load()
    raw = _flow(h, w)
    fb, pp = Farneback(w, h, levels=0), PostProcess(w, h)

    def device_entry(obj, direction, ops, mask_dev):
        _lib.check(lib.tf_dev_upload(C.c_void_p(obj.flow_ptr(0)), C.c_void_p(raw.ctypes.data), raw.nbytes))
        obj.post_process_ex(0, direction, ops, mask_dev)
        out = np.empty_like(raw)
        _lib.check(lib.tf_dev_download(C.c_void_p(out.ctypes.data), C.c_void_p(obj.flow_ptr(0)), out.nbytes))
        return out

    try:
        for mask_name, mask in _masks(h, w).items():
            mdev = None if mask is None else DevBuffer.from_array(mask)
            for chain_name, ops in [("no filters", []), *CHAINS.items()]:
                what = f"{chain_name}, mask {mask_name}"
                for direction in (R.FORWARD, R.BACKWARD, None):
                    exp = fb.post_process_host_ex(raw.copy(), direction, ops, mask)
                    got = pp.post_process_host_ex(raw.copy(), direction, ops, mask)
                    np.testing.assert_array_equal(_bits(got), _bits(exp), err_msg=f"host entry, {what}, {direction}")
                    if direction is None:
                        continue
                    ptr = None if mdev is None else mdev.ptr
                    np.testing.assert_array_equal(_bits(device_entry(pp, direction, ops, ptr)), _bits(exp),
                                                  err_msg=f"device entry, {what}, {direction}")
                    np.testing.assert_array_equal(_bits(device_entry(fb, direction, ops, ptr)), _bits(exp),
                                                  err_msg=f"handle's device entry, {what}, {direction}")
            if mdev is not None:
                mdev.close()
        for obj in (fb, pp):
            with pytest.raises(NotImplementedError):
                obj.post_process_host_ex(raw.copy(), 0, [("scale", np.ones(3))])
            with pytest.raises(ValueError):
                obj.post_process_host_ex(raw.copy(), 0, [("scale", 1.0)] * 9)
            with pytest.raises(ValueError, match="C-contiguous float32 array of shape"):
                obj.post_process_host_ex(raw.astype(np.float64), 0)
    finally:
        fb.close()
        pp.close()


def test_a_float64_flow_takes_no_filters_or_mask():
    """tf_flow_post_process_ex_dev: the filters and the mask are float32's."""
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer
    from transflow_amd.flowops import flow_ops_array
    lib = _lib.load()
    w, h = 37, 23
    flow, other = DevBuffer(16 * w * h), DevBuffer(4 * w * h)
    arr, n = flow_ops_array([("scale", 2.0)])
    for n_ops, mask in ((n, None), (0, C.c_void_p(other.ptr))):
        with pytest.raises(ValueError):
            _lib.check(lib.tf_flow_post_process_ex_dev(C.c_void_p(flow.ptr), 1, w, h, 1, n_ops, arr, mask,
                                                       C.c_void_p(other.ptr)))
    flow.close()
    other.close()


@pytest.fixture
def no_farneback(monkeypatch):
    from transflow_amd import farneback

    def refuse(self, *args, **kwargs):
        raise AssertionError("a Farnebäck handle was made")
    monkeypatch.setattr(farneback.Farneback, "__init__", refuse)


FILTERS = "scale=1.5+t;threshold=0.75;clip=4"


def _ops(source_filters, t):
    """The filters' values at output time t; __next__ counts the frame before it post-processes it (source.py:319-321),
    so frame k of a 25 frames/s source is filtered at t = (k + 1) / 25."""
    return [(f.name, f.expr(t)) for f in source_filters]


@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("with_kernel", [False, True])
@pytest.mark.parametrize("w,h", SHAPES)
def test_host_array_source_needs_no_farneback_handle(no_farneback, direction, with_kernel, w, h):
    """A FlowSource subclass that yields host arrays, with filters, a mask and (with_kernel) a float64 convolution
    kernel, against the oracle's chain."""
    from transflow_amd.flow import FlowFilter, FlowSource
    flows = [_flow(h, w, seed=30 + i) for i in range(3)]
    mask = _masks(h, w)["fractional"][..., np.newaxis]
    kernel = np.random.default_rng(23).normal(0, 0.3, (3, 5)) if with_kernel else None
    d = R.FORWARD if direction == "forward" else R.BACKWARD

    class Arrays(FlowSource):
        def next(self):
            return flows[self.input_frame_index].copy()

    filters = [FlowFilter.from_string(p) for p in FILTERS.split(";")]
    source = Arrays(direction, w, h, 25.0, len(flows), 0, 0, len(flows), mask=mask, kernel=kernel, flow_filters=filters)
    try:
        got = [np.array(f, copy=True) for f in source]
    finally:
        source.close()
    assert len(got) == len(flows)
    for k, (g, raw) in enumerate(zip(got, flows)):
        pre = R.pre_steps(raw.copy(), _ops(filters, (k + 1) / 25.0), mask)
        exp = F.post_process_with_kernel(pre, kernel, d) if with_kernel else R.post_process(pre, d)
        assert g.dtype == exp.dtype == (np.float64 if with_kernel else np.float32)
        np.testing.assert_array_equal(_bits(g), _bits(exp), err_msg=f"frame {k}")


@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("device_flows", [False, True])
@pytest.mark.parametrize("w,h", SHAPES)
def test_motion_vector_source_needs_no_farneback_handle(no_farneback, direction, device_flows, w, h):
    """MotionVectorFlowSource on a list of vector tables, resident path, as host arrays and as DeviceFlows."""
    from transflow_amd.motionvectors import ArrayVectorProvider, MotionVectorFlowSource
    tables = [mv_ref.h264_like(w, h, seed=40 + i, intra=0.3) for i in range(4)]
    tables[2] = None                                        # a frame without side data
    mask = _masks(h, w)["fractional"][..., np.newaxis]
    d = R.FORWARD if direction == "forward" else R.BACKWARD

    class Builder(MotionVectorFlowSource.Builder):
        def _load_inputs(self):
            super()._load_inputs()
            self.mask = mask

    with Builder(ArrayVectorProvider(tables, w, h, 25.0), device_flows=device_flows, direction=direction,
                 flow_filters=FILTERS) as source:
        assert source._resident_ok()
        filters = source.flow_filters
        got = [np.array(f, copy=True) for f in source]
    assert len(got) == len(tables) - 1
    for k, g in enumerate(got):
        raw = mv_ref.paint(tables[k + 1], w, h)
        exp = R.post_process(R.pre_steps(raw, _ops(filters, (k + 1) / 25.0), mask), d)
        assert g.dtype == np.float32 and g.shape == (h, w, 2)
        np.testing.assert_array_equal(_bits(g), _bits(exp), err_msg=f"frame {k}")
