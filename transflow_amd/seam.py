"""The stretch of the reference's main loop between the flow sources and the compositor, for flows that stay in HBM.

    pipeline.py:502      flow = self.merge_flows(flows)                  -> merge(kind, flows)
    pipeline.py:503-504  flow = upscale_array(flow, wf, hf)              -> upscale(flow, wf, hf)
    pipeline.py:513      render2d(flow, ...)                             -> FlowView.view2d
    pipeline.py:515-516  render1d(sqrt(sum(power(flow, 2), axis=2)), ..) -> FlowMagnitude, FlowView.view_magnitude

`merge`, `upscale` and `merge_upscale` take the device route when every operand is a float32 `DeviceFlow` whose device
copy is current: one launch of tf_flow_seam_dev (csrc/flowseam.hip) from the operands' buffers into a slot of a ring
this module keeps per output shape, and the result is a `DeviceFlow` again -- nothing comes down, nothing goes up.
Any other operand (an ndarray, a flow modified on the host, a float64 flow, more than eight flows, shapes that
differ) goes to `fallback`, the function that stood there before, with its result and its exceptions; without a
fallback, to flowops.py's host-array function of the same step.

The magnitude is evaluated by the pipeline before render1d sees anything, so -- as flowzip.RoundedFlow does for
numpy.round -- exactly that chain is answered lazily while `deviceflow.DEVICE_VIEW` is on: numpy.power(flow, 2) is a
`FlowSquares`, numpy.sum of it over axis 2 a `FlowSquareSum`, numpy.sqrt of that a `FlowMagnitude` that remembers its
flow.  Every other use of any of the three computes numpy's own result on the host values.
dropin.install(device_seam=True) puts all of this where the pipeline finds the reference's names.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
from numpy.lib.mixins import NDArrayOperatorsMixin

from . import _lib
from ._lib import check
from .deviceflow import DeviceFlow, FlowRing
from .flowops import MAX_MERGE, MERGE_KINDS, _colors

_RINGS: dict = {}       # output shape -> the FlowRing the results of that shape live in


def is_resident(flow) -> bool:
    """A float32 (H, W, 2) DeviceFlow whose device copy is the current one."""
    return (isinstance(flow, DeviceFlow) and flow.dtype == np.float32 and not flow.on_host and len(flow.shape) == 3
            and flow.shape[2] == 2)


def _served(kind, flows) -> bool:
    if kind not in MERGE_KINDS or not isinstance(flows, (list, tuple)) or not 1 <= len(flows) <= MAX_MERGE:
        return False
    if kind == "absmax" and len(flows) != 2:      # (utils.py:378 fails in its reshape: the original says so)
        return False
    return all(is_resident(f) for f in flows) and all(f.shape == flows[0].shape for f in flows)


def _seam_dev(kind, flows, wf: int, hf: int) -> DeviceFlow:
    h, w, _ = flows[0].shape
    shape = (h * hf, w * wf, 2)
    ring = _RINGS.get(shape)
    if ring is None:
        ring = _RINGS[shape] = FlowRing(shape, slots=3)
    slot = ring.take()
    try:
        for f in flows:
            f.wait_on_stream()
        ptrs = (C.c_void_p * len(flows))(*[f.dev_ptr for f in flows])
        check(_lib.load().tf_flow_seam_dev(MERGE_KINDS[kind], len(flows), ptrs, w, h, wf, hf, C.c_void_p(slot.flow_ptr)))
        for f in flows:
            f.mark_used()
        slot.ready.record()
    except Exception:
        ring.give_back(slot)
        raise
    out = DeviceFlow(shape, slot.flow_ptr, slot.ready, ring=ring, slot=slot)
    # a vector clipped to [-j, W-1-j] at column j lands, times wf, at output column j*wf + a (0 <= a < wf) in
    # [a, (W-1)*wf + a]: inside the frame, and likewise down the rows.  A merge of several flows promises nothing.
    out.in_frame = bool(flows[0].in_frame) and (kind == "first" or len(flows) == 1)
    return out


def merge_upscale(kind: str, flows, wf: int = 1, hf: int = 1, fallback=None):
    """Pipeline.FLOW_MERGING_FUNCTIONS[kind](flows), then utils.upscale_array(., wf, hf) where a factor is not 1."""
    if _served(kind, flows) and isinstance(wf, (int, np.integer)) and isinstance(hf, (int, np.integer)) and wf >= 1 and hf >= 1:
        if kind == "first" and wf == 1 and hf == 1:
            return flows[0]                        # the reference's `flows[0]`: the flow itself
        return _seam_dev(kind, flows, int(wf), int(hf))
    if fallback is not None:
        return fallback(kind, flows, wf, hf)
    from . import flowops
    merged = flowops.merge_flows(kind, flows)
    return merged if wf == 1 and hf == 1 else flowops.upscale_array(merged, wf, hf)


def merge(kind: str, flows, fallback=None):
    """Pipeline.FLOW_MERGING_FUNCTIONS[kind](flows); `fallback(flows)` serves what the device route does not."""
    if _served(kind, flows):
        return merge_upscale(kind, flows)
    if fallback is not None:
        return fallback(flows)
    from . import flowops
    return flowops.merge_flows(kind, flows)


def upscale(flow, wf: int, hf: int, fallback=None):
    """utils.upscale_array(flow, wf, hf); `fallback(flow, wf, hf)` serves what the device route does not."""
    if (is_resident(flow) and isinstance(wf, (int, np.integer)) and isinstance(hf, (int, np.integer)) and wf >= 1
            and hf >= 1):
        return _seam_dev("first", [flow], int(wf), int(hf))
    if fallback is not None:
        return fallback(flow, wf, hf)
    from . import flowops
    return flowops.upscale_array(flow, wf, hf)


# ---- the magnitude expression -------------------------------------------------------------------------------------------

class _Lazy(NDArrayOperatorsMixin):
    """A step of numpy.sqrt(numpy.sum(numpy.power(flow, 2), axis=2)) over a DeviceFlow, not yet computed: the array it
    stands for to everything numpy, computed from the flow's host values at the first use that needs them."""

    dtype = np.dtype(np.float32)

    def __init__(self, flow: DeviceFlow):
        self._flow = flow
        self._host = None

    def _compute(self) -> np.ndarray:
        raise NotImplementedError

    def _value(self) -> np.ndarray:
        if self._host is None:
            self._host = self._compute()
        return self._host

    @property
    def flow(self) -> DeviceFlow:
        return self._flow

    @property
    def ndim(self) -> int:
        return len(self.shape)

    def _lazy_step(self, ufunc, method, inputs, kwargs):
        return None

    def _lazy_function(self, func, args, kwargs):
        return None

    def __array__(self, dtype=None, copy=None):
        a = self._value()
        if dtype is not None and np.dtype(dtype) != a.dtype:
            return a.astype(dtype)
        return a.copy() if copy else a

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        step = self._lazy_step(ufunc, method, inputs, kwargs)
        if step is not None:
            return step
        return getattr(ufunc, method)(*[x._value() if isinstance(x, _Lazy) else x for x in inputs], **kwargs)

    def __array_function__(self, func, types, args, kwargs):
        step = self._lazy_function(func, args, kwargs)
        if step is not None:
            return step

        def down(x):
            if isinstance(x, _Lazy):
                return x._value()
            if isinstance(x, (list, tuple)):
                return type(x)(down(v) for v in x)
            return x
        return func(*down(args), **{k: down(v) for k, v in kwargs.items()})

    def __len__(self) -> int:
        return self.shape[0]

    def __getitem__(self, key):
        return self._value()[key]

    def __iter__(self):
        return iter(self._value())

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._value(), name)

    def __repr__(self):
        return f"{type(self).__name__}(shape={self.shape}, {'computed' if self._host is not None else 'lazy'})"


class FlowSquares(_Lazy):
    """numpy.power(flow, 2)."""

    def __init__(self, flow):
        super().__init__(flow)
        self.shape = flow.shape

    def _compute(self):
        return np.power(self._flow.host(), 2)

    def _lazy_function(self, func, args, kwargs):
        if func is np.sum and self._host is None:
            axis = args[1] if len(args) == 2 else kwargs.get("axis")
            if (args and args[0] is self and len(args) + len(kwargs) == 2 and (len(args) == 2 or "axis" in kwargs)
                    and isinstance(axis, (int, np.integer)) and axis == 2):
                return FlowSquareSum(self._flow)
        return None


class FlowSquareSum(_Lazy):
    """numpy.sum(numpy.power(flow, 2), axis=2)."""

    def __init__(self, flow):
        super().__init__(flow)
        self.shape = flow.shape[:2]

    def _compute(self):
        return np.sum(np.power(self._flow.host(), 2), axis=2)

    def _lazy_step(self, ufunc, method, inputs, kwargs):
        if ufunc is np.sqrt and method == "__call__" and not kwargs and len(inputs) == 1 and self._host is None:
            return FlowMagnitude(self._flow)
        return None


class FlowMagnitude(_Lazy):
    """numpy.sqrt(numpy.sum(numpy.power(flow, 2), axis=2)): what FlowView.view_magnitude renders from the flow itself."""

    def __init__(self, flow):
        super().__init__(flow)
        self.shape = flow.shape[:2]

    def _compute(self):
        return np.sqrt(np.sum(np.power(self._flow.host(), 2), axis=2))

    @property
    def resident(self) -> bool:
        return self._host is None and is_resident(self._flow)


def lazy_squares(flow: DeviceFlow, inputs, kwargs):
    """DeviceFlow.__array_ufunc__'s question while DEVICE_VIEW is on: is this call numpy.power(flow, 2) and nothing
    more?  The FlowSquares if so, else None.  The exponent is a scalar equal to 2 that leaves the result float32 (a
    Python number, or a numpy scalar no wider than float32)."""
    if kwargs or len(inputs) != 2 or inputs[0] is not flow or not is_resident(flow):
        return None
    e = inputs[1]
    if isinstance(e, bool) or not isinstance(e, (int, float, np.integer, np.floating)) or e != 2:
        return None
    if isinstance(e, np.generic) and np.result_type(np.float32, e.dtype) != np.float32:
        return None
    return FlowSquares(flow)


# ---- the views ------------------------------------------------------------------------------------------------------------

class FlowView:
    """--view-flow and --view-flow-magnitude of a resident flow: rendered into a CompImage's device address, handed
    out in the form the compositor's frames leave in (the keyword arguments are HipCompositor's frame-form options:
    lazy_frames, jpeg_frames, png_frames, png_code, jpeg_optimize, jpeg_subsampling, yuv_frames, yuv_matrix,
    yuv_range), by the compositor's own code: a HipCompositor without layers."""

    def __init__(self, **frame_options):
        self.frame_options = dict(frame_options)
        self._compositor = None

    def _image(self, shape):
        from .compositor import HipCompositor
        h, w = int(shape[0]), int(shape[1])
        c = self._compositor
        if c is None or (c.height, c.width) != (h, w):
            self.close()
            c = self._compositor = HipCompositor(h, w, [], **self.frame_options)
        return c._image()

    def view2d(self, flow: DeviceFlow, scale: float = 1, colors=None):
        """output/render.py:30-48 of a resident flow."""
        if not is_resident(flow):
            raise ValueError("FlowView.view2d takes a float32 DeviceFlow whose device copy is current")
        comp = self._image(flow.shape)
        n = flow.shape[0] * flow.shape[1]
        flow.wait_on_stream()
        check(_lib.load().tf_flow_render2d_dev(C.c_void_p(flow.dev_ptr), C.c_void_p(comp.image_ptr()), n, float(scale),
                                               _colors(colors or ("#ffff00", "#0000ff", "#ff00ff", "#00ff00"), 4)))
        flow.mark_used()
        return self._compositor._frame_of(comp)

    def view_magnitude(self, mag: FlowMagnitude, scale: float = 1, colors=None, binary: bool = False):
        """output/render.py:9-27 of the magnitude of a resident flow, which is never stored."""
        if not isinstance(mag, FlowMagnitude) or not mag.resident:
            raise ValueError("FlowView.view_magnitude takes the FlowMagnitude of a float32 DeviceFlow whose device copy is current")
        flow = mag.flow
        comp = self._image(flow.shape)
        n = flow.shape[0] * flow.shape[1]
        flow.wait_on_stream()
        check(_lib.load().tf_flow_view_magnitude_dev(C.c_void_p(flow.dev_ptr), C.c_void_p(comp.image_ptr()), n, float(scale),
                                                     _colors(colors or ("#000000", "#ffffff"), 2), int(bool(binary))))
        flow.mark_used()
        return self._compositor._frame_of(comp)

    def close(self):
        if self._compositor is not None:
            self._compositor.close()
            self._compositor = None


def close_rings() -> None:
    """Frees the result rings (callers that hold no result any more)."""
    for ring in _RINGS.values():
        ring.close()
    _RINGS.clear()
