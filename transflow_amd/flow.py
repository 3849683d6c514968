"""Flow sources backed by libtfhip.so, behind the reference's FlowSource surface.

`FlowSource` mirrors transflow/flow/sources/source.py:17-415 (Direction, LockMode,
Builder with its seek/duration/repeat/lock arithmetic, the iterator protocol and
post_process); `HipFlowSource` mirrors CvFlowSource
(transflow/flow/sources/cv.py:366-524): frames come from a frame provider, the
flow from the GPU, by the method the config names (the table `_METHODS`).  Items yielded are numpy float32 arrays of shape (H, W, 2),
picklable, exactly what pipeline.py:85-86 puts on its queue.

No HIP call happens before Builder.__enter__/build(): the reference forks the
flow source into a child process (pipeline.py:56-64).
"""
from __future__ import annotations

import dataclasses
import enum
import logging
import os
import warnings
import numpy as np

from .config import (CONFIG_CLASSES, FlowConfig, HornSchunckConfig, LiteFlowNetConfig, LucasKanadeConfig,
                     flow_config_from_arg, flow_config_from_reference)

logger = logging.getLogger(__name__)


class FlowFilter:
    """A flow filter of the reference (transflow/flow/filters.py): `name=expr`.  scale / threshold /
    clip: expr is a Python expression of t evaluated on the host for every frame, the arithmetic on
    the flow runs on the GPU.  polar: `polar=expr_radius:expr_theta`, expressions of (t, r, a)
    compiled for the device (transflow_amd/exprs.py)."""

    NAMES = ("scale", "threshold", "clip", "polar")

    def __init__(self, name: str, expr_string: str):
        if name not in self.NAMES:
            raise ValueError(f"Unknown filter name '{name}'")                     # filters.py:33
        self.name = name
        self.expr_string = expr_string
        if name == "polar":
            from .exprs import PolarFilter
            parts = expr_string.split(":")
            if len(parts) != 2:
                raise ValueError(f"Invalid number of arguments: {name} {tuple(parts)}")   # filters.py:29-30
            self.polar = PolarFilter(parts[0], parts[1])
            self.expr = None
            return
        import math
        import random
        import re

        import numpy
        # the names the reference's utils module (where its eval runs, utils.py:407-412) offers
        scope = {"math": math, "numpy": numpy, "random": random, "re": re, "os": os}
        self.expr = eval("lambda t: " + expr_string, scope)

    @classmethod
    def from_string(cls, text: str):
        """'scale=2*t' -> FlowFilter('scale', '2*t')   (source.py:143-149)"""
        i = text.index("=")
        args = tuple(text[i + 1:].strip().split(":"))
        if len(args) != 1 and text[:i].strip() != "polar":
            raise ValueError(f"Invalid number of arguments: {text[:i].strip()} {args}")  # filters.py:21-31
        return cls(text[:i].strip(), args[0] if len(args) == 1 else ":".join(args))


def _enum_from_arg(enum_cls, arg, default, what):
    """The argument forms the reference accepts for its two enums (source.py:24-56): None, a member
    (ours or the reference's own, matched by name), the integer value, or the lower-case name."""
    if arg is None:
        return default
    if isinstance(arg, enum.Enum):
        if arg.name in enum_cls.__members__:
            return enum_cls[arg.name]
    elif isinstance(arg, int):
        return enum_cls(arg)
    elif isinstance(arg, str) and arg.upper() in enum_cls.__members__ and arg == arg.lower():
        return enum_cls[arg.upper()]
    raise ValueError(f"Invalid {what}: {arg}")


@dataclasses.dataclass
class Timeline:
    """What a source's frame range and output length come to (source.py:151-197), as one value."""
    base_length: int | None     # frames the input holds; None = a stream
    repeat: int
    seek_time: float | None
    start_frame: int
    end_frame: int
    length: int | None          # flows the source will yield; None = endless
    ckpt_start_frame: int       # where the FIRST pass starts when resuming from a checkpoint

    @property
    def is_stream(self) -> bool:
        return self.base_length is None


def plan_timeline(base_length, framerate, seek_time, duration_time, repeat, seek_ckpt, stay_pairs) -> Timeline:
    """The seek / duration / repeat / checkpoint arithmetic of FlowSource.Builder.build
    (source.py:151-197).  A non-positive base length means a stream: it cannot repeat or seek (both
    are dropped with the reference's warnings).  Every STAY lock adds its duration to the length."""
    frames = base_length if (base_length is not None and base_length > 0) else None
    if frames is None:
        if repeat > 1:
            warnings.warn("Flow source is a stream, cannot repeat it!")
            repeat = 1
        if seek_time is not None and seek_time > 0:
            warnings.warn("Flow source is a stream, seek time is ignored!")
            seek_time = None
    first = 0
    if frames is not None and seek_time is not None:
        first = int(seek_time * framerate)
    last = 0 if frames is None else frames
    if duration_time is not None:
        # three decimals before truncating: 0.1 s at 29.97 fps must not lose a frame to 2.9969999
        last = first + int(round(duration_time * framerate, 3))
        if frames is not None and last > frames:
            last = frames
    if repeat == 0:
        total = None
    else:
        total = last if frames is None else repeat * (last - first)
        for _, held in (stay_pairs or ()):
            total += int(held * framerate)
    resume = first
    if seek_ckpt is not None:
        resume = first + seek_ckpt % (last - first)
    return Timeline(frames, repeat, seek_time, first, last, total, resume)


class LockSchedule:
    """When the source repeats its previous flow instead of reading a new one (source.py:296-311).
    STAY: (start, duration) pairs in output time; SKIP: a predicate of t (and the input advances)."""

    def __init__(self, mode, stay_pairs, skip_predicate):
        self.mode, self.pairs, self.predicate = mode, stay_pairs, skip_predicate
        self.which = 0              # the STAY pair in force or awaited
        self.since = None           # output time at which the current STAY lock began

    def locked(self, t: float) -> bool:
        if self.mode == FlowSource.LockMode.SKIP:
            return bool(self.predicate(t)) if self.predicate is not None else False
        if self.pairs is None:
            return False
        if self.since is not None:
            if t - self.since < self.pairs[self.which][1]:
                return True
            self.since = None
            self.which += 1
        # past the last pair this indexes out of range: the reference raises the same IndexError
        # (source.py:304-307), and the pipeline's source process stops on it (pipeline.py:90-97)
        if t >= self.pairs[self.which][0]:
            self.since = t
            return True
        return False


class FlowSource:
    """Base class with the reference's constructor, attributes and iteration protocol
    (transflow/flow/sources/source.py:17-415); the bodies are this package's own."""

    @enum.unique
    class Direction(enum.Enum):
        FORWARD = 0   # past to present
        BACKWARD = 1  # present to past

        @classmethod
        def from_arg(cls, arg):
            return _enum_from_arg(cls, arg, cls.FORWARD, "Flow Direction")     # None -> FORWARD, source.py:26-28

    @enum.unique
    class LockMode(enum.Enum):
        STAY = 0
        SKIP = 1

        @classmethod
        def from_arg(cls, arg):
            return _enum_from_arg(cls, arg, cls.STAY, "Lock Mode")

    class Builder:
        """Context manager: `build()` resolves the arguments, `__enter__` makes the source
        (source.py:58-209).  Attribute names are the reference's: its callers and subclasses read them."""

        def __init__(self, direction="backward", mask_path=None, kernel_path=None, flow_filters=None,
                     seek_ckpt=None, seek_time=None, duration_time=None, repeat: int = 1, lock_expr=None,
                     lock_mode="stay", resident_steps: bool = False):
            self.direction = FlowSource.Direction.from_arg(direction)
            self.resident_steps = bool(resident_steps)     # (FlowSource.__init__ says what it asks for)
            self.lock_mode = FlowSource.LockMode.from_arg(lock_mode)
            self.mask_path, self.kernel_path = mask_path, kernel_path
            self.flow_filters_string, self.lock_expr_string = flow_filters, lock_expr
            self.seek_ckpt, self.seek_time, self.duration_time, self.repeat = seek_ckpt, seek_time, duration_time, repeat
            # filled by build() (subclasses set width / height / framerate / base_length before calling it)
            self.width = self.height = None
            self.framerate: float = 30
            self.base_length = self.length = None
            self.is_stream = False
            self.start_frame = self.ckpt_start_frame = self.end_frame = 0
            self.mask = self.kernel = None
            self.flow_filters: list = []
            self.lock_expr_stay = self.lock_expr_skip = None
            self.source: FlowSource | None = None

        @property
        def cls(self):
            return FlowSource

        def args(self) -> list:
            return [getattr(self, name) for name in ("direction", "width", "height", "framerate", "length",
                                                     "start_frame", "ckpt_start_frame", "end_frame")]

        def kwargs(self) -> dict:
            return {name: getattr(self, name) for name in ("mask", "kernel", "flow_filters", "lock_mode",
                                                           "lock_expr_stay", "lock_expr_skip", "resident_steps")}

        def _load_inputs(self):
            if self.mask_path is not None:                       # a float mask, one trailing axis (source.py:127-129)
                from .masks import load_float_mask
                self.mask = load_float_mask(self.mask_path)[..., np.newaxis]
            if self.kernel_path is not None:                     # source.py:131-132
                self.kernel = np.load(self.kernel_path)
            if self.flow_filters_string is not None:             # "name=expr; name=expr" (source.py:141-149)
                self.flow_filters = [FlowFilter.from_string(part) for part in self.flow_filters_string.strip().split(";")]
            text = self.lock_expr_string
            if text is None:
                return
            if self.lock_mode == FlowSource.LockMode.SKIP:       # a predicate of t (source.py:138-139)
                self.lock_expr_skip = eval("lambda t: " + text)
            else:                                                # "a,b" or "(a,b),(c,d)": (start, duration) pairs
                self.lock_expr_stay = tuple(eval("[" + (text if "(" in text else "(" + text + ")") + ",]"))

        def build(self):
            self._load_inputs()
            plan = plan_timeline(self.base_length, self.framerate, self.seek_time, self.duration_time, self.repeat,
                                 self.seek_ckpt,
                                 self.lock_expr_stay if self.lock_mode == FlowSource.LockMode.STAY else None)
            self.base_length, self.is_stream = plan.base_length, plan.is_stream
            self.repeat, self.seek_time = plan.repeat, plan.seek_time
            self.start_frame, self.end_frame, self.length = plan.start_frame, plan.end_frame, plan.length
            self.ckpt_start_frame = plan.ckpt_start_frame

        def __enter__(self):
            self.build()
            source = self.cls(*self.args(), **self.kwargs())
            source.validate()
            logger.debug("Built '%s'", type(source).__name__)
            self.source = source          # what __exit__ closes
            return source

        def __exit__(self, *exc):
            if self.source is not None:
                self.source.close()

    def __init__(self, direction, width: int, height: int, framerate: float, length, start_frame: int,
                 ckpt_start_frame: int, end_frame: int, mask=None, kernel=None, flow_filters=(),
                 lock_mode=None, lock_expr_stay=None, lock_expr_skip=None, resident_steps: bool = False):
        """resident_steps (opt-in): a convolution kernel and polar filters ride the resident tail of a source that has
        one (_post_process_steps) instead of sending it down the host route; off, such a source takes the route it
        took before the argument existed."""
        self.resident_steps = bool(resident_steps)
        self.direction = FlowSource.Direction.from_arg(direction)
        self.width, self.height, self.framerate = width, height, framerate
        self.length, self.end_frame = length, end_frame
        self.mask, self.kernel, self.flow_filters = mask, kernel, list(flow_filters)
        if kernel is not None:
            from .flowops import kernel_result_type
            if not isinstance(kernel, np.ndarray):
                raise ValueError(f"Attribute kernel has incorrect type {type(kernel)}")   # source.py:281
            kernel_result_type(kernel)   # float32 / float64 results only
        if not all(isinstance(f, FlowFilter) for f in self.flow_filters):
            raise ValueError("flow_filters must be transflow_amd.flow.FlowFilter objects")
        self.lock_mode = FlowSource.LockMode.from_arg(lock_mode)
        self.lock_expr_stay, self.lock_expr_skip = lock_expr_stay, lock_expr_skip
        self._locks = LockSchedule(self.lock_mode, lock_expr_stay, lock_expr_skip)
        self.output_frame_index = 0
        self.prev_flow = None
        self._pp = None  # what post_process runs on (a flowops.PostProcess, or a resident method's handle), made on first use
        # the resident tail (below): what read_next_flow handed out whose flow is still on the device, the mask on the
        # device, and where the yielded arrays / DeviceFlows (transflow_amd/deviceflow.py) live
        self._pending = self._mask_dev = self._flow_pool = self._flow_ring = None
        self._kernel_dev = None  # (the convolution kernel on the device, its shape): _kernel_on_device
        self._scratch = {}       # device buffers of the out-of-place tail (_device_scratch)
        # the first pass starts where a checkpoint left off, later passes at start_frame (source.py:246-248)
        self.input_frame_index = 0
        self.start_frame, later_passes = ckpt_start_frame, start_frame
        self.rewind()                                    # subclasses decode up to start_frame here
        self.start_frame = later_passes
        # source.py:250-263 builds per-pixel clip tables on the host (a 1.2 s Python loop at
        # 1080p); the kernels derive the bounds from the pixel index instead

    # the STAY bookkeeping under the reference's attribute names (its checkpoints and tests read them)
    lock_start = property(lambda self: self._locks.since)
    lock_expr_stay_index = property(lambda self: self._locks.which)

    def __len__(self):
        return self.length

    def validate(self):
        """source.py:268-284: the constructor arguments have the types the pipeline relies on."""
        expected = {"direction": FlowSource.Direction, "width": int, "height": int, "framerate": float,
                    "length": (int, type(None)), "start_frame": int, "end_frame": int, "flow_filters": list,
                    "lock_mode": FlowSource.LockMode, "lock_expr_stay": (tuple, type(None))}
        for name, types in expected.items():
            value = getattr(self, name)
            if not isinstance(value, types):
                raise ValueError(f"Attribute {name} has incorrect type {type(value)}")

    @property
    def t(self) -> float:
        """Output time in seconds."""
        return self.output_frame_index / self.framerate if self.framerate is not None else 0

    def read_next_flow(self):
        """One input flow; the input wraps to start_frame when it reaches end_frame (source.py:286-291)."""
        if self.input_frame_index == self.end_frame:
            self.rewind()
        flow = self.next()
        self.input_frame_index += 1
        return flow

    def __iter__(self):
        return self

    def __next__(self):
        """One output flow (source.py:293-321): a locked source hands out its previous flow again
        (and, in SKIP mode, still consumes an input flow); everything goes through post_process."""
        if self.length is not None and self.output_frame_index >= self.length:
            raise StopIteration
        if self._locks.locked(self.t):
            if self.prev_flow is None:
                raise RuntimeError("Flow is locked but has not been initialized. Maybe lock the flow later?")
            flow = self.prev_flow
            if self.lock_mode == FlowSource.LockMode.SKIP:
                self.read_next_flow()
        else:
            flow = self.prev_flow = self.read_next_flow()
        self.output_frame_index += 1
        return self.post_process(flow)

    def next(self):
        raise NotImplementedError()

    def rewind(self):
        self.input_frame_index = self.start_frame

    def post_process(self, raw):
        """source.py:337-363 on the GPU (flowops.PostProcess): FORWARD inverts the push
        field with last-write-wins, both directions clip to the frame.  In place, like the
        reference (so `prev_flow` sees the processed array, source.py:317): the filters work on the array given, the
        mask and the convolution kernel each make a new one, which the steps after them work on."""
        if self._pending is not None and raw is self._pending:
            return self._post_process_resident(raw)
        from .flowops import convolve_post_process, polar_filter
        # 1. a rounded archive (pipeline.py:506 writes numpy.round(flow).astype(int)): the reference clips and inverts
        # the integer array in place; small integers are exact in float32
        archive = raw if (isinstance(raw, np.ndarray) and np.issubdtype(raw.dtype, np.integer) and not self.flow_filters
                          and self.mask is None and self.kernel is None) else None
        flow = raw if archive is None else raw.astype(np.float32)
        # 2. the library works on contiguous float32
        if not (isinstance(flow, np.ndarray) and flow.dtype == np.float32 and flow.flags.c_contiguous):
            flow = np.ascontiguousarray(flow, dtype=np.float32)
        pp, direction = self._post_handle(), self.direction.value
        # 3. the filters, in order and in place (source.py:339-341; filters.py: lambdas of t, evaluated here): runs of
        # scale/threshold/clip go to the device as one launch each, every polar filter as its own.  Where that is one
        # run and nothing comes between it and the direction handling, the two share a launch (step 5).
        fused = self.mask is None and self.kernel is None and not any(f.name == "polar" for f in self.flow_filters)
        run = []
        for f in [*self.flow_filters, None]:
            if f is not None and f.name != "polar":
                run.append((f.name, f.expr(self.t)))
                continue
            if run and not fused:
                pp.post_process_host_ex(flow, None, run)
                run = []
            if f is not None:
                polar_filter(flow, f.polar, self.t)
        # 4. the mask multiply makes a NEW array (source.py:342-343: prev_flow sees the filters and not the mask); it
        # shares its launch with the direction handling unless the convolution comes between them
        if self.mask is not None:
            flow = flow.copy()
            pp.post_process_host_ex(flow, None if self.kernel is not None else direction, (), self.mask)
        # 5. the convolution of both channels (source.py:344-348: a NEW array of the convolution's type, float64 unless
        # the kernel is float32) which the direction handling and the clip then work on; or these two alone
        if self.kernel is not None:
            flow = convolve_post_process(flow, self.kernel, direction)
        elif self.mask is None:
            pp.post_process_host_ex(flow, direction, run)
        if archive is None:
            return flow
        archive[...] = flow.astype(archive.dtype)
        return archive

    # ---- the resident tail ---------------------------------------------------------------------
    # __next__ (source.py:293-321) calls read_next_flow() and hands its result straight to post_process().  When
    # nothing can look at the raw flow in between (_resident_ok) a source that makes its flows on the device keeps
    # them there through the filters (polar ones too), the mask, the convolution kernel and the direction handling
    # (_post_process_steps where a polar filter or a kernel is set, with resident_steps), and only the final flow comes down, or
    # none (a DeviceFlow).  Such a source's read_next_flow leaves the raw flow in a post-processing handle and
    # returns _take_output(); post_process, given that very object back, fills it.  It says where the flow sits
    # (_resident_flow) and how a host array is filled from there (_download).
    device = None     # the device argument of the sources that take one

    def _post_handle(self):
        if self._pp is None:
            from .flowops import PostProcess
            self._pp = PostProcess(self.width, self.height, device=self.device)
        return self._pp

    def _resident_ok(self) -> bool:
        """Nothing reads a raw flow or prev_flow on the host (the lock expressions do), and every step of
        post_process has a device form (a convolution kernel of a type the device does not convolve in has none: the
        host route raises for it, as before)."""
        if self.lock_expr_stay is not None or self.lock_expr_skip is not None:
            return False
        steps = self.kernel is not None or any(f.name == "polar" for f in self.flow_filters)
        if steps and not self.resident_steps:
            return False         # (the device form of these two is asked for: resident_steps)
        try:
            self._output_dtype()
        except NotImplementedError:
            return False
        return True

    def _output_dtype(self) -> np.dtype:
        """The type post_process returns: float32, or the convolution's (source.py:344-348), float64 unless the kernel
        is float32."""
        if self.kernel is None:
            return np.dtype(np.float32)
        from .flowops import kernel_result_type
        return np.dtype(kernel_result_type(self.kernel))

    def _take_output(self, device_flows, depth: int):
        """What the resident post_process fills: a DeviceFlow over a buffer of the source's ring (device_flows: True
        or "ipc"), else a pinned host array of its pool; `depth` of them can be out at a time.  Both are of the type
        post_process returns (_output_dtype): float64 behind a float64 convolution kernel."""
        shape, dtype = (self.height, self.width, 2), self._output_dtype()
        if device_flows:
            from .deviceflow import DeviceFlow, FlowRing
            if self._flow_ring is None:
                self._flow_ring = FlowRing(shape, slots=depth, dtype=dtype)
            slot = self._flow_ring.take()
            self._pending = DeviceFlow(shape, slot.flow_ptr, slot.ready, ring=self._flow_ring, slot=slot,
                                       cross_process="ipc" if device_flows == "ipc" else None, dtype=dtype)
        else:
            if self._flow_pool is None:
                from .device import ArrayPool
                self._flow_pool = ArrayPool(shape, dtype, limit=depth, pinned=True)
            self._pending = self._flow_pool.take()
        return self._pending

    def _resident_flow(self):
        """(handle, pair): where the flow behind `_pending` sits."""
        raise NotImplementedError()

    def _download(self, handle, pair: int, out: np.ndarray) -> None:
        raise NotImplementedError()

    def _chain_route(self):
        """None: the handle post-processes its flow where it sits (post_process_ex).  Else (src, chain): the flow is
        read from the device address `src`, which is left as it is, and post-processed into the output's own buffer
        (tf_flow_post_process_chain_dev); `chain`, if not None, is where the next call's initial flow is left."""
        return None

    def _device_scratch(self, name: str, nbytes: int):
        """A device buffer of the out-of-place tail ("winner": FORWARD's winner map; "staging": where a flow that goes
        to a host array is post-processed before its one download), made on first use."""
        if name not in self._scratch:
            from .device import DevBuffer
            self._scratch[name] = DevBuffer(max(1, nbytes))
        return self._scratch[name]

    def _output_buffer(self, raw) -> int:
        """Where the last launch of the out-of-place tail writes: the DeviceFlow's own buffer, or the staging buffer a
        host array's one download starts from."""
        if not isinstance(raw, np.ndarray):
            return raw.dev_ptr
        return self._device_scratch(f"staging {raw.dtype.name}", raw.dtype.itemsize * 2 * self.width * self.height).ptr

    def _winner_buffer(self):
        if self.direction != FlowSource.Direction.FORWARD:
            return None
        return self._device_scratch("winner", 4 * self.width * self.height).ptr

    def _hand_out(self, raw, dst: int):
        """The flow at `dst` (_output_buffer) is complete on this thread's stream: down into the host array, or marked."""
        if isinstance(raw, np.ndarray):
            # (with hip_prefetch this is the worker thread: the copy waits on that thread's stream, the consumer does not)
            if raw.nbytes:
                import ctypes as C

                from . import _lib
                _lib.check(_lib.load().tf_dev_download(C.c_void_p(raw.ctypes.data), C.c_void_p(dst), raw.nbytes))
            return raw
        raw._ready.record()
        raw.in_frame = True          # both directions of post_process end with the clip (source.py:361-362)
        return raw

    def _chain_launch(self, src: int, dst: int, chain, direction: int, ops, mask_ptr) -> None:
        import ctypes as C

        from . import _lib
        from .flowops import flow_ops_array
        arr, n = flow_ops_array(ops)
        winner = self._winner_buffer() if direction == 0 else None
        _lib.check(_lib.load().tf_flow_post_process_chain_dev(
            C.c_void_p(src), C.c_void_p(dst), C.c_void_p(chain) if chain else None, self.width, self.height,
            direction, n, arr, C.c_void_p(mask_ptr) if mask_ptr else None, C.c_void_p(winner) if winner else None))

    def _chain_written(self, chain) -> None:
        """The out-of-place tail has run; `chain`, if not None, now holds the next call's initial flow."""

    def _post_process_chain(self, raw, src: int, chain, ops, mask_ptr):
        dst = self._output_buffer(raw)
        self._chain_launch(src, dst, chain, self.direction.value, ops, mask_ptr)
        self._chain_written(chain)
        return self._hand_out(raw, dst)

    def _kernel_on_device(self):
        """The convolution kernel in the convolution's type, converted once and kept for the life of the source."""
        if self._kernel_dev is None:
            from .device import DevBuffer
            k = np.ascontiguousarray(self.kernel, dtype=self._output_dtype())
            if k.ndim != 2 or k.size == 0:
                raise ValueError("the convolution kernel must be a non-empty 2-D array")
            self._kernel_dev = (DevBuffer.from_array(k), k.shape)
        return self._kernel_dev

    def _post_process_steps(self, raw, handle, pair: int, route, mask_ptr):
        """The resident tail with a polar filter or a convolution kernel, in the reference's order (source.py:337-363):
        runs of scale / threshold / clip as one launch each, every polar filter in place where it falls, then the mask,
        then the kernel (tf_flow_convolve_post_process_dev: the direction handling and the clip in the convolution's
        type, straight into the output).  A flow that sits in a method handle's buffer (`route`, _chain_route) is left
        as it is: the first launch that has to write moves it into a scratch of the source's.  With a kernel the chain
        state -- the reference's prev_flow -- is the float32 flow after the filters and before the mask and the kernel;
        without one it is what tf_flow_post_process_chain_dev leaves, as ever."""
        import ctypes as C

        from . import _lib
        from .flowops import flow_ops_array, polar_filter_dev
        lib, P = _lib.load(), C.c_void_p
        w, h, px, direction = self.width, self.height, self.width * self.height, self.direction.value
        if route is None:
            cur, writable, chain = handle.flow_ptr(pair), True, None
        else:
            (cur, chain), writable = route, False

        def in_place(ops, mask):
            if ops or mask:
                arr, n = flow_ops_array(ops)
                _lib.check(lib.tf_flow_post_process_ex_dev(P(cur), 0, w, h, -1, n, arr, P(mask) if mask else None, None))

        run = []
        for f in self.flow_filters:
            if f.name != "polar":
                run.append((f.name, f.expr(self.t)))
                continue
            if not writable:
                work = self._device_scratch("filtered", 8 * px).ptr
                self._chain_launch(cur, work, None, -1, run, None)
                cur, writable = work, True
            else:
                in_place(run, None)
            run = []
            polar_filter_dev(cur, px, f.polar, self.t)
        if self.kernel is None:
            if route is None:
                handle.post_process_ex(pair, direction, run, mask_ptr)
                return None               # (the handle's own way out: _post_process_resident)
            return self._post_process_chain(raw, cur, chain, run, mask_ptr)
        if writable and not chain:
            in_place(run, mask_ptr)
        elif chain and not run and not mask_ptr:
            # the chain state is the flow as it is: its one copy, and the convolution reads the flow where it sits
            _lib.check(lib.tf_dev_copy(P(chain), P(cur), 8 * px))
        elif run or mask_ptr or chain:
            masked = self._device_scratch("masked", 8 * px).ptr
            self._chain_launch(cur, masked, chain, -1, run, mask_ptr)
            cur = masked
        kernel, (kh, kw) = self._kernel_on_device()
        dst, winner = self._output_buffer(raw), self._winner_buffer()
        _lib.check(lib.tf_flow_convolve_post_process_dev(
            P(cur), P(kernel.ptr), kh, kw, int(self._output_dtype() == np.float64), P(dst), w, h, direction,
            P(winner) if winner else None))
        if route is not None:
            self._chain_written(chain)
        return self._hand_out(raw, dst)

    def _post_process_resident(self, raw):
        self._pending = None
        handle, pair = self._resident_flow()
        if self.mask is not None and self._mask_dev is None:
            from .device import DevBuffer
            self._mask_dev = DevBuffer.from_array(
                np.ascontiguousarray(self.mask, dtype=np.float32).reshape(self.height, self.width))
        mask_ptr = None if self.mask is None else self._mask_dev.ptr
        route = self._chain_route()
        if self.kernel is not None or any(f.name == "polar" for f in self.flow_filters):
            out = self._post_process_steps(raw, handle, pair, route, mask_ptr)
            if out is not None:
                return out
        else:
            ops = [(f.name, f.expr(self.t)) for f in self.flow_filters]
            if route is not None:
                return self._post_process_chain(raw, route[0], route[1], ops, mask_ptr)
            handle.post_process_ex(pair, self.direction.value, ops, mask_ptr)
        if isinstance(raw, np.ndarray):
            self._download(handle, pair, raw)
            return raw
        # a DeviceFlow: out of the handle's buffer (which the source writes again) into the flow's own, device to
        # device on this thread's stream; the event behind the copy is what consumers wait for
        import ctypes as C

        from . import _lib
        _lib.check(_lib.load().tf_dev_copy(C.c_void_p(raw.dev_ptr), C.c_void_p(handle.flow_ptr(pair)), raw.nbytes))
        raw._ready.record()
        raw.in_frame = True          # both directions of post_process end with the clip (source.py:361-362)
        return raw

    def close(self):
        if self._mask_dev is not None:
            self._mask_dev.close()
            self._mask_dev = None
        if self._kernel_dev is not None:
            self._kernel_dev[0].close()
            self._kernel_dev = None
        self._pending = None
        if self._flow_ring is not None:
            # flows that left this process as IPC tokens: multiprocessing's Queue.get() frees the queue's slot before it
            # unpickles, so the last put() of SourceProcess.run (pipeline.py:85-86) can return -- and this process end --
            # before the consumer has opened the last flow's handle.  Wait (bounded) until every token on its way has
            # been made and acknowledged; our own reference to the last flow goes first.
            self.prev_flow = None
            self._flow_ring.drain()
        self._flow_ring = None      # (buffers live as long as a DeviceFlow the caller still holds)
        self._flow_pool = None
        for buf in self._scratch.values():
            buf.close()
        self._scratch = {}
        if self._pp is not None:
            self._pp.close()
            self._pp = None


class ArrayFrameProvider:
    """Frames held in memory: a sequence of uint8 arrays, grey (H, W) or BGR (Hs, Ws, 3).  `size` = (width,
    height) the source reports (cv2.CAP_PROP_FRAME_WIDTH / HEIGHT, cv.py:420-427); BGR frames of another size
    are brought to it by the nearest-neighbour resize of cv.py:461, on the device."""

    def __init__(self, frames, framerate: float = 30.0, size=None):
        self.frames = frames
        self.framerate = float(framerate)
        first = np.asarray(frames[0])
        self.height, self.width = first.shape[:2]
        if size is not None:
            self.width, self.height = int(size[0]), int(size[1])
        self.frame_count = len(frames)
        self.pos = 0

    def seek_start(self):
        self.pos = 0

    def read(self):
        if self.pos >= self.frame_count:
            return None
        f = np.asarray(self.frames[self.pos])
        self.pos += 1
        return f

    def release(self):
        pass


class Cv2FrameProvider:
    """Video decode through cv2.VideoCapture, as CvFlowSource does (cv.py:416-429, 447-466).
    Decode stays on the CPU and is out of this backend's scope; it needs opencv-python."""

    def __init__(self, file: str, size=None):
        import re

        import cv2
        self.cv2 = cv2
        self.capture = cv2.VideoCapture(int(file)) if re.match(r"\d+", file) else cv2.VideoCapture(file)
        if size is not None:
            self.capture.set(cv2.CAP_PROP_FRAME_WIDTH, size[0])
            self.capture.set(cv2.CAP_PROP_FRAME_HEIGHT, size[1])
        self.width = int(self.capture.get(cv2.CAP_PROP_FRAME_WIDTH))
        self.height = int(self.capture.get(cv2.CAP_PROP_FRAME_HEIGHT))
        self.framerate = float(self.capture.get(cv2.CAP_PROP_FPS))
        self.frame_count = int(self.capture.get(cv2.CAP_PROP_FRAME_COUNT))

    def seek_start(self):
        self.capture.set(self.cv2.CAP_PROP_POS_MSEC, 0)

    def read(self):
        ok, frame = self.capture.read()
        if not ok or frame is None:
            return None
        return frame     # as decoded: the resize of cv.py:461 and the grey conversion run on the device

    def release(self):
        self.capture.release()


class _Prefetch:
    """A worker thread that iterates a flow source ahead of its consumer (HipFlowSource.__next__)."""

    def __init__(self, source, depth: int):
        import queue
        import threading
        self.source = source
        self.queue = queue.Queue(maxsize=max(1, int(depth)))
        self.halt = threading.Event()
        self.finished = None                       # ("stop", None) or ("error", exception) once the worker has ended
        self.thread = threading.Thread(target=self._run, name="tfhip-flow-prefetch", daemon=True)
        self.thread.start()

    def _put(self, item) -> bool:
        import queue
        while not self.halt.is_set():
            try:
                self.queue.put(item, timeout=0.05)
                return True
            except queue.Full:
                continue
        return False

    def _run(self):
        from . import _lib
        try:
            _lib.check(_lib.load().tf_thread_stream(1))
            # Flow t's download (started by post_process) runs beside frame t + 1's upload and kernels: the worker issues
            # t + 1 first and only then waits for t's transfer and hands the array over.
            held = None                              # (flow, token of its download) not yet handed over

            def hand_over():
                nonlocal held
                if held is None:
                    return True
                flow, token = held
                held = None
                if token is not None:
                    self.source._fb.get_flow_end(token)
                return self._put(("flow", flow))
            while not self.halt.is_set():
                try:
                    self.source._download_token = None
                    flow = FlowSource.__next__(self.source)
                except StopIteration:
                    if hand_over():
                        self._put(("stop", None))
                    return
                except BaseException:
                    hand_over()                      # the flows before the failure still reach the consumer, in order
                    raise
                token = self.source._download_token
                if not hand_over():
                    return
                held = (flow, token)
        except BaseException as err:            # noqa: BLE001 -- re-raised in the consumer's thread
            self._put(("error", err))

    def get(self):
        if self.finished is None:
            kind, value = self.queue.get()
            if kind == "flow":
                return value
            self.finished = (kind, value)
        if self.finished[0] == "error":
            raise self.finished[1]
        raise StopIteration

    def stop(self):
        import queue
        self.halt.set()
        while self.thread.is_alive():
            try:
                self.queue.get_nowait()
            except queue.Empty:
                pass
            self.thread.join(timeout=0.05)


def _open_farneback(source):
    from .farneback import Farneback

    # Exactness belongs to the handle (tf_fb_set_exact): this source states what its configuration says, on OR off,
    # and touches nothing process-wide -- sources that disagree may be open together, in any threads.
    batch = source._batch_size()
    fb = Farneback(source.width, source.height, device=source.device, frame_slots=batch + 1, max_pairs=batch,
                   exact=bool(source.config.hip_exact_sums), **source.config.fb_kwargs())
    fb.keep_expansions(True)  # the frame that was "next" stays expanded for its turn as "prev"
    if source.config.hip_prefetch:
        fb.async_io(True)     # the next frame up and the previous flow down beside this pair's kernels
    return fb


def _open_horn_schunck(source):
    from .hornschunck import HornSchunck
    return HornSchunck(source.width, source.height, device=source.device)      # (every call chains: one pair)


def _open_lucas_kanade(source):
    from .lucaskanade import LucasKanade
    batch = source._batch_size()      # 1 unless hip_resident
    return LucasKanade(source.width, source.height, frame_slots=batch + 1, max_pairs=batch, device=source.device)


def _open_liteflownet(source):
    from .liteflownet import LiteFlowNet
    batch = source._batch_size()
    return LiteFlowNet(source.width, source.height, source.config.weights, frame_slots=batch + 1, max_pairs=batch,
                       device=source.device, precision=source.config.hip_lfn_precision)


def _previous_flow_or_zeros(source):
    if source.prev_flow is not None:
        return source.prev_flow
    return np.zeros((source.height, source.width, 2), np.float32)


# The chain state on the device (hip_resident): what the reference keeps in `prev_flow` (source.py:314-321, 337-363; the
# rule is DESIGN.md section 10's), written by tf_flow_post_process_chain_dev behind every call and read by the next.
def _hs_chain_buffer(source, handle) -> int:
    return source._device_scratch("chain", 8 * source.width * source.height).ptr      # the source's own, 8 B/px


def _hs_chain_start(source, handle, valid: bool) -> None:
    # borrowed by the handle until its next call has read it; no chain yet (the start, a rewind): the float64 chain
    handle.set_initial_flow_dev(0, _hs_chain_buffer(source, handle) if valid else None)


def _fb_chain_buffer(source, handle) -> int:
    return handle.initial_flow_ptr(0)              # the handle reads its initial flow where the chain is written


def _fb_chain_start(source, handle, valid: bool) -> None:
    if not valid:
        handle.set_initial_flow(0, _previous_flow_or_zeros(source))     # (prev_flow is None here: float32 zeros)


@dataclasses.dataclass(frozen=True)
class _Method:
    """What HipFlowSource needs of a flow method, by the class of its config (_METHODS): this is where a method is
    wired into the source."""
    open: object                            # (source) -> the method's handle (imported here: no HIP call before build())
    calc_kwargs: object = lambda config: {}     # (config) -> the keyword arguments of the handle's calc_slots
    # (source) -> the flow set_initial_flow gets before a call; None: the method takes none.  `initial_flow_switch`:
    # (config) -> whether the configuration asks for it; None: there is no switch, every call gets one.
    initial_flow: object = None
    initial_flow_switch: object = None
    colour: bool = False                    # the method reads colour frames: grey ones are refused
    # the handle post-processes its flows where they are (post_process_ex) and brings them down beside its kernels
    # (async_io, get_flow_begin): the resident path exists.  For the others it is not built: their flows come down
    # raw and FlowSource.post_process works on the host array, through a flowops.PostProcess (a flow, a winner map and
    # the mask on the device; no second flow handle).
    resident: bool = False
    # What the out-of-place resident tail (hip_resident; FlowSource._post_process_chain) needs of a handle that has no
    # post_process_ex, or whose calls chain.  `flow_ptr`: (handle, pair) -> where the flow of a pair of the last call
    # sits.  A method whose calls chain -- each starts from the previous output: `initial_flow` above, where its switch
    # says so -- also says where that output is kept on the device, `chain_buffer`: (source, handle) -> address, and
    # how a call is started from it, `chain_start`: (source, handle, valid); `valid` false: there is no previous output.
    flow_ptr: object = lambda handle, pair: handle.flow_ptr(pair)
    chain_buffer: object = None
    chain_start: object = None


_METHODS = {
    # cv.py:473-490; cv.py:478 with cv2.OPTFLOW_USE_INITIAL_FLOW: a copy of the previous flow, zeros before the first
    FlowConfig: _Method(_open_farneback, initial_flow=_previous_flow_or_zeros,
                        initial_flow_switch=lambda config: bool(config.fb_flags & 4), resident=True,
                        chain_buffer=_fb_chain_buffer, chain_start=_fb_chain_start),
    # cv.py:491-500: the previous (post-processed) flow, or None (the float64 chain from zeros)
    HornSchunckConfig: _Method(_open_horn_schunck, HornSchunckConfig.hs_kwargs, initial_flow=lambda source: source.prev_flow,
                               chain_buffer=_hs_chain_buffer, chain_start=_hs_chain_start),
    # cv.py:501-508: no initial flow
    LucasKanadeConfig: _Method(_open_lucas_kanade, LucasKanadeConfig.lk_kwargs),
    # cv.py:464-465, 509-516: the two frames only, in colour
    LiteFlowNetConfig: _Method(_open_liteflownet, colour=True),
}
assert set(_METHODS) == set(CONFIG_CLASSES)


class HipFlowSource(FlowSource):
    """CvFlowSource's flow methods on the GPU (cv.py:434-521).  The config says which: its class is the key of
    _METHODS above, where everything this source needs to know of a method is said.  Flows of a method without a
    resident path come down to the host, where the post-process runs, unless the config says `hip_resident`: then
    they go through the out-of-place tail (FlowSource._post_process_chain) and a chaining method's previous output
    stays on the device too."""

    class Builder(FlowSource.Builder):

        def __init__(self, provider, config=None, size=None, device: int | None = None, **kwargs):
            super().__init__(**kwargs)
            self.provider_arg, self.size, self.device = provider, size, device
            self.config = flow_config_from_reference(config)
            self.provider = None

        @property
        def cls(self):
            return HipFlowSource

        def build(self):
            p = self.provider_arg
            self.provider = Cv2FrameProvider(p, self.size) if isinstance(p, str) else p
            self.width, self.height = int(self.provider.width), int(self.provider.height)
            self.framerate = float(self.provider.framerate)
            self.base_length = int(self.provider.frame_count) - 1                        # cv.py:428
            super().build()

        def args(self):
            return [self.provider, self.config, *FlowSource.Builder.args(self)]

        def kwargs(self):
            kw = super().kwargs()
            kw["device"] = self.device
            return kw

    def __init__(self, provider, config: FlowConfig, *args, device: int | None = None, **kwargs):
        self.config = config
        # (validate() refuses a config of no method's class)
        self._method = next((m for cls, m in _METHODS.items() if isinstance(config, cls)), None)
        self.provider = provider
        self.device = device
        self._prev_frame = None  # the decoded frame behind prev_gray
        self._fb = None
        self._prev_slot = None   # frame slot holding prev_gray on the device
        self._batch_left = 0     # FlowConfig.hip_batch: flows of the last call not handed out yet ...
        self._batch_pos = 0      # ... and which pair of the call comes next
        self._pending_pair = 0   # the pair of the call behind the array read_next_flow handed out
        self._prefetch = None
        self._download_token = None
        self.chain_valid = False  # hip_resident: the chain buffer holds the previous output (what prev_flow stands for)
        FlowSource.__init__(self, *args, **kwargs)

    def validate(self):
        super().validate()
        if self._method is None:
            raise ValueError("Attribute config has incorrect type")

    def _handle(self):
        if self._fb is None:
            self._fb = self._method.open(self)
            if self._method.resident:
                self._pp = self._fb  # one handle serves both calls
        return self._fb

    # The frame the reference keeps as `prev_gray` (cv.py:456, 519) lives in a frame slot of the handle; on the
    # host only the decoded frame it came from is kept (to fill the slot again after a rewind).  Frames are
    # made grey ON THE DEVICE (tf_fb_set_frame_bgr: cv2.resize INTER_NEAREST + COLOR_BGR2GRAY of cv.py:461-466
    # as one kernel into the slot, OpenCV 4's 15-bit weights); a provider of grey frames is taken as it is.
    @property
    def prev_gray(self):
        f = self._prev_frame
        if f is None or np.asarray(f).ndim == 2:
            return f
        from .flowops import bgr_to_grey
        return bgr_to_grey(f, (self.width, self.height))

    @prev_gray.setter
    def prev_gray(self, value):
        self._prev_frame = value
        self._prev_slot = None
        self.chain_valid = False
        self._batch_left = self._batch_pos = 0     # flows of a hip_batch call made before the seek are not handed out after it

    def _ingest(self, slot: int, frame) -> None:
        from .pixmap import DevicePixmap
        # A frame decoded on the device stays there.  A provider hands BGR, as every provider's host frames are
        # (MjpegFrameProvider.read's default order): a three-channel DevicePixmap is read as BGR, whatever made it.
        if isinstance(frame, DevicePixmap) and hasattr(self._handle(), "set_frame_bgr_dev") and frame.shape[2] == 3:
            self._handle().set_frame_bgr_dev(slot, frame)
            return
        a = np.asarray(frame)
        if self._method.colour and a.ndim != 3:
            raise ValueError(f"the {self.config.method} method needs colour (BGR) frames; the frame provider gives grey ones")
        if a.ndim == 2:
            self._handle().set_frame(slot, a)
        else:
            self._handle().set_frame_bgr(slot, a)

    def rewind(self):
        """cv.py:447-458: decode from the start up to the start frame, keep it as `prev`."""
        FlowSource.rewind(self)
        self.provider.seek_start()
        frame = None
        for i in range(self.input_frame_index + 1):
            frame = self.provider.read()
            if frame is None:
                raise RuntimeError(f"An error occurred while reading frame at index {i}")
        self._prev_frame = frame
        self.prev_flow = None
        self.chain_valid = False
        self._prev_slot = None
        self._batch_left = self._batch_pos = 0     # (an external rewind while a hip_batch call still had flows queued)

    def _batch_size(self) -> int:
        # a call that starts from the previous output computes one pair, whatever hip_batch says
        return max(1, int(self.config.hip_batch)) if self._resident_ok() and not self._chains() else 1

    def _advance(self, want: int = 1, resident: bool = False) -> int:
        """cv.py:460-490 up to the call: read a frame, make it grey in a slot no pair still needs, order (prev, next) by
        direction, run the method's handle on the two slots.  The flow stays on the device.  `want` > 1 (FlowConfig.hip_batch): read
        up to that many frames and run their consecutive pairs in ONE call -- frame slots are a ring of hip_batch + 1, the
        last frame of a call is the first of the next; returns how many pairs were computed."""
        frames = []
        for _ in range(max(1, want)):
            frame = self.provider.read()
            if frame is None:
                break
            frames.append(frame)
        if not frames:
            raise StopIteration
        if self._prev_frame is None:
            raise ValueError("Missing reference frames")
        fb = self._handle()                          # (the first GPU call of a source: after the provider has spoken)
        if self._prev_slot is None:                  # first frame, or after a rewind
            self._ingest(0, self._prev_frame)
            self._prev_slot = 0
        ring = fb.frame_slots
        older, newer = [], []
        slot = self._prev_slot
        for frame in frames:
            new_slot = (slot + 1) % ring
            self._ingest(new_slot, frame)
            older.append(slot)
            newer.append(new_slot)
            slot = new_slot
        method = self._method
        if self._chains():
            if resident:
                method.chain_start(self, fb, self.chain_valid)
            else:
                fb.set_initial_flow(0, method.initial_flow(self))
        kw = method.calc_kwargs(self.config)
        if self.direction == FlowSource.Direction.FORWARD:      # cv.py:467-472
            fb.calc_slots(older, newer, **kw)
        elif self.direction == FlowSource.Direction.BACKWARD:
            fb.calc_slots(newer, older, **kw)
        else:
            raise ValueError(f"Invalid flow direction '{self.direction}'")
        self._prev_slot, self._prev_frame = slot, frames[-1]
        return len(frames)

    # ---- resident form of one iteration (FlowSource's resident tail): only the new frame goes up and only the final
    # flow comes down -- one transfer each instead of two frames up and the flow down, up and down again.  The
    # public next() / post_process() pair keeps working on host arrays for any other caller.
    def _uses_initial_flow(self) -> bool:
        """The configuration's switch for an initial flow (cv2.OPTFLOW_USE_INITIAL_FLOW) is on."""
        switch = self._method.initial_flow_switch
        return switch is not None and switch(self.config)

    def _chains(self) -> bool:
        """Every call starts from the previous OUTPUT (cv.py:478, 495 pass prev_flow, which __next__ has post-processed
        in place): Horn-Schunck always, Farnebäck where its switch is on."""
        method = self._method
        return method.initial_flow is not None and (method.initial_flow_switch is None or self._uses_initial_flow())

    def _own_tail(self) -> bool:
        """The handle post-processes its flows where they are, and no call reads a previous output: Farnebäck's own
        resident path."""
        return self._method.resident and not self._chains()

    def _resident_ok(self) -> bool:
        # a previous output lives on the host, and so does the raw flow of a method without a resident path, unless
        # hip_resident keeps both on the device (the out-of-place tail and the chain buffer)
        return (self._own_tail() or bool(self.config.hip_resident)) and FlowSource._resident_ok(self)

    def _chain_route(self):
        if self._own_tail():
            return None
        chain = self._method.chain_buffer(self, self._fb) if self._chains() else None
        return self._method.flow_ptr(self._fb, self._pending_pair), chain

    def _chain_written(self, chain):
        self.chain_valid = chain is not None

    def read_next_flow(self):
        if not self._resident_ok():
            return FlowSource.read_next_flow(self)
        if self.input_frame_index == self.end_frame:
            self.rewind()
            self._batch_left = 0
        if self._batch_left == 0:
            # never across the wrap of the input (source.py:286-291: the frame after end_frame is start_frame's)
            until_wrap = self.end_frame - self.input_frame_index if self.end_frame > self.input_frame_index else self._batch_size()
            self._batch_left = self._advance(min(self._batch_size(), max(1, until_wrap)), resident=True)
            self._batch_pos = 0
        self._pending_pair = self._batch_pos
        self._batch_pos += 1
        self._batch_left -= 1
        self.input_frame_index += 1
        # hip_device_flows: the flow stays in HBM, in a DeviceFlow that post_process fills
        return self._take_output(self.config.hip_device_flows, 4 + self.config.hip_prefetch)

    def _resident_flow(self):
        return self._fb, self._pending_pair

    def _download(self, fb, pair, out):
        if self._prefetch is not None:
            # the worker thread: the flow starts its way down and the worker goes on to the next frame; it hands this
            # array to the consumer only once the transfer has ended (_Prefetch._run)
            self._download_token = fb.get_flow_begin(pair, out)
        else:
            fb.get_flow_into(pair, out)

    def next(self):
        """cv.py:460-490: (prev, next) ordered by direction, one call of the method; the flow as a host array."""
        self._advance()
        return self._handle().get_flow(0)

    # ---- prefetch (FlowConfig.hip_prefetch) ----------------------------------------------------
    # The reference runs its flow source in a child process that fills a queue (pipeline.py:56-64, 85-86), so flow
    # t + 1 is computed while the compositor works on flow t.  A source iterated in-process gets the same from a
    # worker thread: it runs FlowSource.__next__ -- the whole recurrence, locks and rewinds included -- up to
    # `hip_prefetch` flows ahead, queueing everything it launches on a library stream of its own (tf_thread_stream),
    # beside the compositor's uploads, kernels and downloads.  ctypes releases the GIL inside every library call.
    def __next__(self):
        if not self.config.hip_prefetch:
            return FlowSource.__next__(self)
        if self._prefetch is None:
            self._prefetch = _Prefetch(self, self.config.hip_prefetch)
        return self._prefetch.get()

    def close(self):
        if self._prefetch is not None:
            self._prefetch.stop()
            self._prefetch = None
            if self._fb is not None and self._method.resident:
                self._fb.async_io(False)    # waits for a download the worker left on its way
        fb, self._fb = self._fb, None
        if self._pp is fb:
            self._pp = None                 # (one handle serves both calls: closed once, below)
        FlowSource.close(self)
        if fb is not None:
            fb.close()
        self.provider.release()

    @classmethod
    def from_args(cls, flow_path, use_mvs: bool = False, mask_path=None, kernel_path=None, cv_config=None,
                  flow_filters=None, size=None, direction=None, seek_ckpt=None, seek_time=None,
                  duration_time=None, repeat: int = 1, lock_expr=None, lock_mode="stay", lucas_kanade: bool = False,
                  liteflownet=None, archive_device_inflate: bool = False, resident_steps: bool = False):
        """Same signature as FlowSource.from_args (source.py:365-411); `flow_path` may also be
        a frame provider object.  lucas_kanade: a config naming "lukas-kanade" is served (else it raises ValueError);
        liteflownet: the network's weights (a path or a dict of arrays), with which a config naming "liteflownet" is.  `.flow.zip` archives go to ArchiveFlowSource (source.py:397-399), with archive_device_inflate to its
        device_inflate form (indexed members are inflated on the device);
        resident_steps: a convolution kernel and polar filters stay on the device where the source has a resident tail
        (FlowSource.__init__);
        use_mvs: codec motion vectors (source.py:400-402) go to MotionVectorFlowSource (transflow_amd/motionvectors.py),
        `flow_path` being a video path for PyAV (`avformat::path` as the reference splits it) or a vector provider."""
        common = dict(direction=direction, mask_path=mask_path, kernel_path=kernel_path, flow_filters=flow_filters,
                      seek_ckpt=seek_ckpt, seek_time=seek_time, duration_time=duration_time, repeat=repeat,
                      lock_expr=lock_expr, lock_mode=lock_mode, resident_steps=resident_steps)
        if isinstance(flow_path, str) and flow_path.split("::")[-1].endswith(".flow.zip"):
            from .archive import ArchiveFlowSource
            return ArchiveFlowSource.Builder(flow_path.split("::")[-1], device_inflate=archive_device_inflate, **common)
        if use_mvs:                                        # source.py:381-384, 400-402
            from .motionvectors import MotionVectorFlowSource
            avformat = None
            if isinstance(flow_path, str) and "::" in flow_path:
                avformat, flow_path = flow_path.split("::")
            return MotionVectorFlowSource.Builder(flow_path, avformat, **common)
        config = flow_config_from_arg(cv_config, lucas_kanade=lucas_kanade, liteflownet=liteflownet)
        if isinstance(flow_path, str) and "::" in flow_path:
            flow_path = flow_path.split("::")[1]
        return cls.Builder(flow_path, config, size, **common)
