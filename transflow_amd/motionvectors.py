"""Codec motion vectors as a flow source: the reference's `transflow -m` / `use_mvs=True` input
(transflow/flow/sources/av.py) on the GPU.

AvFlowSource.next() (av.py:61-77) paints, for every motion vector of a decoded frame in list order, the constant
(-motion_x / motion_scale, -motion_y / motion_scale) into the numpy slice of an (H, W, 2) float32 array that is centred
on the vector's SOURCE position: one Python slice assignment per macroblock partition, 8 k - 130 k of them per frame at
1080p - 4K.  Here the vector table (about 1 MB) goes to the device and two kernels paint it (tf_mv_*, csrc/motionvectors.hip),
bit for bit what the reference paints: last writer wins, numpy's wrapping of negative slice bounds, -0.0 for a zero
motion, the float64 quotient rounded to float32.

* `vectors_to_records(vectors)`: a frame's vectors as an array of `MV_DTYPE` (the C struct tf_mv_vector);
* `MotionVectors(width, height)`: the handle -- `rasterize(vectors)` gives the host array, `rasterize_into(vectors, ptr)`
  paints into device memory;
* `ArrayVectorProvider` / `AvVectorProvider`: where the tables come from (memory / PyAV);
* `MotionVectorFlowSource`: the FlowSource over a provider.  With nothing looking at the raw flow in between (no lock
  expressions, no convolution kernel, no polar filter) the flow is painted straight into the post-process handle's
  buffer, filtered, masked and clipped there, and comes down once -- or not at all (`device_flows`).

Demuxing and decoding stay PyAV's job.  No HIP call happens at import or before the first flow is asked for (the
reference forks its flow source into a child process, pipeline.py:56-64).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .flow import FlowSource

FIELDS = ("source", "w", "h", "src_x", "src_y", "motion_x", "motion_y", "motion_scale")
# tf_mv_vector (include/tfhip.h): the fields of libavutil's AVMotionVector that av.py:69-75 reads, as int32
MV_DTYPE = np.dtype([(name, np.int32) for name in FIELDS])


def vectors_to_records(vectors) -> np.ndarray:
    """A frame's motion vectors as a C-contiguous array of MV_DTYPE.  `vectors`: None (a frame without MOTION_VECTORS
    side data: no records); a numpy structured array with AVMotionVector's field names (what PyAV's
    MotionVectors.to_ndarray() returns; converted field by field, without a Python loop); or any iterable of objects
    with those attributes (what iterating a PyAV MotionVectors yields)."""
    if vectors is None:
        return np.empty(0, MV_DTYPE)
    if isinstance(vectors, np.ndarray):
        if vectors.dtype == MV_DTYPE:
            return np.ascontiguousarray(vectors).reshape(-1)
        names = vectors.dtype.names or ()
        missing = [name for name in FIELDS if name not in names]
        if missing:
            raise ValueError(f"motion vector table without the fields {missing} (dtype {vectors.dtype})")
        out = np.empty(vectors.size, MV_DTYPE)
        flat = vectors.reshape(-1)
        for name in FIELDS:
            out[name] = flat[name]
        return out
    rows = [tuple(int(getattr(v, name)) for name in FIELDS) for v in vectors]
    return np.array(rows, dtype=MV_DTYPE).reshape(-1)


def stage_resolve_rects(width: int, height: int, vectors):
    """av.py:70-75 per vector, as the library does it on the host (no device needed): (rects, values), rects int32
    (n, 4) = {i0, i1, j0, j1} after numpy's slice resolution, values float32 (n, 2) = {-dx, -dy}.  ValueError for a
    vector the reference rejects (source != -1, motion_scale == 0)."""
    rec = vectors_to_records(vectors)
    rects = np.empty((rec.size, 4), np.int32)
    values = np.empty((rec.size, 2), np.float32)
    check(_lib.load().tf_mv_stage_resolve_rects(int(width), int(height), C.c_void_p(rec.ctypes.data), rec.size,
                                                C.c_void_p(rects.ctypes.data), C.c_void_p(values.ctypes.data)))
    return rects, values


class MotionVectors:
    """Thin object over the tf_mv_* entry points.  The device handle is made by the first call that paints."""

    def __init__(self, width: int, height: int, device: int | None = None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.width, self.height, self.device = int(width), int(height), device
        if self.width < 1 or self.height < 1:
            raise ValueError(f"bad size {self.width}x{self.height}")

    def _handle(self):
        if not self._h.value:
            if self.device is not None:
                check(self._lib.tf_init(int(self.device)))
            check(self._lib.tf_mv_create(C.byref(self._h), self.width, self.height))
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tf_mv_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rasterize(self, vectors, out: np.ndarray | None = None) -> np.ndarray:
        """av.py:62-77 for one frame: a new float32 (H, W, 2) array (or `out`, C-contiguous float32 of that shape)."""
        rec = vectors_to_records(vectors)
        if out is None:
            out = np.empty((self.height, self.width, 2), np.float32)
        elif out.dtype != np.float32 or not out.flags.c_contiguous or out.shape != (self.height, self.width, 2):
            raise ValueError("rasterize needs a C-contiguous float32 array of shape (H, W, 2)")
        check(self._lib.tf_mv_rasterize(self._handle(), C.c_void_p(rec.ctypes.data) if rec.size else None, rec.size,
                                        C.c_void_p(out.ctypes.data)))
        return out

    def rasterize_into(self, vectors, dev_ptr: int) -> None:
        """The same into device memory at `dev_ptr` ([H][W][2] float32), queued on this thread's library stream."""
        rec = vectors_to_records(vectors)
        check(self._lib.tf_mv_rasterize_dev(self._handle(), C.c_void_p(rec.ctypes.data) if rec.size else None, rec.size,
                                            C.c_void_p(int(dev_ptr))))


class ArrayVectorProvider:
    """Vector tables held in memory, one per frame (None: a frame without motion vectors) -- for tests, and for
    anyone with a demuxer of their own.  read() raises StopIteration past the last frame, as the reference's
    `next(self.iterator)` does (av.py:63)."""

    def __init__(self, tables, width: int, height: int, framerate: float = 30.0):
        self.tables = tables
        self.width, self.height, self.framerate = int(width), int(height), float(framerate)
        self.frame_count = len(tables)
        self.pos = 0

    def seek_start(self):
        self.pos = 0

    def read(self):
        if self.pos >= self.frame_count:
            raise StopIteration
        table = self.tables[self.pos]
        self.pos += 1
        return table

    def release(self):
        pass


class AvVectorProvider:
    """Motion vectors decoded by PyAV, as AvFlowSource.Builder.build does it (av.py:28-38): the codec context gets
    `flags2=+export_mvs`, width and height come from the first decoded frame, the frame rate from the codec context
    (30 when it has none), the frame count from the stream.  PyAV is imported here, when the provider is built: a
    missing PyAV is an ImportError then, never at import of the package.  Where this package is built and tested PyAV
    is not installed: this class is exercised against a stub `av` module only (tests/test_motionvectors_host.py)."""

    def __init__(self, path: str, avformat: str | None = None):
        import av.container
        self.container = av.container.open(format=avformat, file=path)
        stream = self.container.streams.video[0]
        context = stream.codec_context
        context.options = {"flags2": "+export_mvs"}
        first = next(self.container.decode(video=0))
        self.width, self.height = int(first.width), int(first.height)
        self.framerate = float(context.framerate) if context.framerate else 30.0
        self.frame_count = int(stream.frames)
        self.iterator = None

    def seek_start(self):
        self.container.seek(0)
        self.iterator = self.container.decode(video=0)

    def read(self):
        """The next frame's vectors (a structured array where the side data can make one, else the side data itself
        to iterate), None for a frame without them; StopIteration at the end of the stream."""
        if self.iterator is None:
            self.seek_start()
        frame = next(self.iterator)
        vectors = frame.side_data.get("MOTION_VECTORS")
        if vectors is None:
            return None
        return vectors.to_ndarray() if hasattr(vectors, "to_ndarray") else vectors

    def release(self):
        self.container.close()


class MotionVectorFlowSource(FlowSource):
    """AvFlowSource (av.py) over a vector provider: every input frame's vectors painted on the GPU."""

    class Builder(FlowSource.Builder):

        def __init__(self, provider, avformat: str | None = None, device: int | None = None, device_flows=False, **kwargs):
            super().__init__(**kwargs)
            self.provider_arg, self.avformat, self.device, self.device_flows = provider, avformat, device, device_flows
            self.provider = None

        @property
        def cls(self):
            return MotionVectorFlowSource

        def build(self):
            p = self.provider_arg
            self.provider = AvVectorProvider(p, self.avformat) if isinstance(p, str) else p
            self.width, self.height = int(self.provider.width), int(self.provider.height)
            self.framerate = float(self.provider.framerate)
            self.base_length = int(self.provider.frame_count) - 1                        # av.py:37
            super().build()

        def args(self):
            return [self.provider, *FlowSource.Builder.args(self)]

        def kwargs(self):
            kw = super().kwargs()
            kw.update(device=self.device, device_flows=self.device_flows)
            return kw

    def __init__(self, provider, *args, device: int | None = None, device_flows=False, **kwargs):
        """device_flows: True or "ipc" -- the source yields DeviceFlows (transflow_amd/deviceflow.py) where the
        resident path applies, as FlowConfig.hip_device_flows does for Farnebäck."""
        self.provider = provider
        self.device, self.device_flows = device, device_flows
        self._mv = None
        FlowSource.__init__(self, *args, **kwargs)

    def validate(self):
        super().validate()
        for name in ("seek_start", "read", "release"):
            if not callable(getattr(self.provider, name, None)):
                raise ValueError(f"Attribute provider has incorrect type {type(self.provider)}")

    def _handle(self) -> MotionVectors:
        if self._mv is None:
            self._mv = MotionVectors(self.width, self.height, device=self.device)
        return self._mv

    def rewind(self):
        """av.py:55-59: seek to the start and skip the frames up to and including the start frame."""
        FlowSource.rewind(self)
        self.provider.seek_start()
        for _ in range(self.input_frame_index + 1):
            self.provider.read()

    def next(self):
        """av.py:61-77: the next frame's vectors painted into a new host array."""
        return self._handle().rasterize(self.provider.read())

    # ---- resident form of one iteration (FlowSource's resident tail): the painted flow never leaves the device before
    # the filters, the mask and the direction handling have run on it
    def read_next_flow(self):
        if not self._resident_ok():
            return FlowSource.read_next_flow(self)
        if self.input_frame_index == self.end_frame:
            self.rewind()
        vectors = self.provider.read()
        self._handle().rasterize_into(vectors, self._post_handle().flow_ptr(0))
        self.input_frame_index += 1
        return self._take_output(self.device_flows, 4)

    def _resident_flow(self):
        return self._pp, 0

    def _download(self, pp, pair, out):
        check(_lib.load().tf_dev_download(C.c_void_p(out.ctypes.data), C.c_void_p(pp.flow_ptr(pair)), out.nbytes))

    def close(self):
        FlowSource.close(self)
        if self._mv is not None:
            self._mv.close()
            self._mv = None
        self.provider.release()
