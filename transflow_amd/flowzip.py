"""Flow archive members deflated where the flow is (tf_flowzip_*, transflow_amd/csrc/flowzip.hip).

The reference's flow export (`--export-flow`, `--export-rounded-flow`; transflow/pipeline.py:363-377, 505-506) brings every
flow down and runs zlib over `numpy.save`'s bytes on one CPU thread.  `FlowZipEncoder` makes the same member -- a raw
deflate stream that inflates to exactly those bytes, and their CRC-32 -- on the device, from a flow that is there anyway
(DESIGN.md section 17), and only the member comes down.  `DeviceFlowArchiveWriter` (transflow_amd/archive.py) puts the
members into the zip.

An encoder is anything with

    encode_host(prefix: bytes, array: numpy.ndarray, distance: int) -> (stream: bytes, crc32: int)
    encode_device(prefix: bytes, dev_ptr: int, nbytes: int, distance: int) -> (stream: bytes, crc32: int)

(and `close()`): tests/flowzip_ref.py has one in numpy, for writing whole archives without a GPU.  An encoder may also have

    last_band_sizes() -> [int]      the compressed bytes of each band of the last encode, in stream order

which is what `DeviceFlowArchiveWriter(index=True)` writes into the archive's band index.

`RoundedFlow` and `DeviceInt64Flow` are what `numpy.round(flow)` and `numpy.round(flow).astype(int)` are while
`deviceflow.DEVICE_ROUND` is on: the rounding runs on the device (tf_flow_round_i64_dev) and its int64 values stay there
for the writer; any other use gives the host values numpy would have given.
"""
from __future__ import annotations

import ctypes as C
import io

import numpy as np
from numpy.lib.mixins import NDArrayOperatorsMixin

# The "same byte D back" distance per dtype (Measured): a float32's neighbour bytes, the same byte
# of the vector one pixel back for the 8-byte types (H, W, 2: 16 bytes a pixel).
DISTANCES = {np.dtype(np.float32): 1, np.dtype(np.float64): 16, np.dtype(np.int64): 16}

_prefixes: dict = {}


def npy_prefix(shape, dtype) -> bytes:
    """The header numpy.save writes in front of a C-order array of this shape and dtype."""
    key = (tuple(int(v) for v in shape), np.dtype(dtype))
    if key not in _prefixes:
        dummy = np.lib.stride_tricks.as_strided(np.zeros(1, key[1]), key[0], (0,) * len(key[0]))
        buf = io.BytesIO()
        np.lib.format.write_array_header_1_0(buf, np.lib.format.header_data_from_array_1_0(dummy))
        _prefixes[key] = buf.getvalue()
    return _prefixes[key]


def default_band_bytes() -> int:
    """The band the library chooses (the call loads it and touches no GPU)."""
    from . import _lib
    return int(_lib.load().tf_flowzip_default_band_bytes())


class FlowZipEncoder:
    """tf_flowzip: one band size; its device buffers are allocated for the largest stream seen so far.  `views`: the
    stream comes back as a memoryview of the encoder's page-locked buffer, valid until the next encode (what the archive
    writer asks for: it writes the member at once); otherwise as bytes of its own."""

    def __init__(self, band_bytes: int | None = None, views: bool = False):
        from . import _lib
        self._lib = _lib.load()
        self._check = _lib.check
        self._err_arg = _lib.TF_ERR_ARG
        self._want_band = 0 if band_bytes is None else int(band_bytes)
        self._h = C.c_void_p()
        self._room = 0
        self._out = None
        self.views = bool(views)
        self.band_bytes = self._want_band or default_band_bytes()
        self.last_needed = 0

    def _handle(self, stream_bytes: int):
        if stream_bytes > self._room:
            self.close()
            self._check(self._lib.tf_flowzip_create(C.byref(self._h), stream_bytes, self._want_band))
            self._room = stream_bytes
            self.band_bytes = int(self._lib.tf_flowzip_band_bytes(self._h))
        return self._h

    def _encode(self, entry, prefix: bytes, ptr: int, nbytes: int, distance: int):
        h = self._handle(len(prefix) + nbytes)
        total = len(prefix) + nbytes
        bound = total + 5 * (total // min(self.band_bytes, 65535) + 2) + 5         # no stream is longer (section 17)
        if self._out is None or self._out.nbytes < bound:
            from .device import pinned_empty
            self._out = pinned_empty((bound,), np.uint8)                           # page-locked: the copy runs at the link's rate
        n, crc = C.c_size_t(), C.c_uint32()
        rc = entry(h, prefix, len(prefix), C.c_void_p(ptr), nbytes, int(distance), C.c_void_p(self._out.ctypes.data),
                   self._out.nbytes, C.byref(n), C.byref(crc))
        self.last_needed = n.value
        if rc == self._err_arg and n.value > self._out.nbytes:                     # still in the handle: copy, no kernel
            self._out = np.empty(n.value, np.uint8)
            rc = self._lib.tf_flowzip_copy_last(h, C.c_void_p(self._out.ctypes.data), self._out.nbytes, C.byref(n))
        self._check(rc)
        stream = self._out[:n.value]
        return (memoryview(stream) if self.views else stream.tobytes()), int(crc.value)

    def encode_device(self, prefix: bytes, dev_ptr: int, nbytes: int, distance: int):
        return self._encode(self._lib.tf_flowzip_encode_dev, bytes(prefix), int(dev_ptr), int(nbytes), distance)

    def encode_host(self, prefix: bytes, array: np.ndarray, distance: int):
        array = np.ascontiguousarray(array)
        return self._encode(self._lib.tf_flowzip_encode, bytes(prefix), array.ctypes.data, array.nbytes, distance)

    def last_lengths(self) -> list:
        out = (C.c_uint8 * 286)()
        self._check(self._lib.tf_flowzip_last_lengths(self._h, out))
        return list(out)

    def last_band_sizes(self) -> list:
        """The compressed bytes of each band of the last encode (tf_flowzip_last_band_sizes: read from the handle, no
        kernel runs); with the final block's five bytes they sum to the stream's length."""
        n = C.c_size_t()
        room = max(1, -(-max(1, self._room) // self.band_bytes))
        out = (C.c_uint32 * room)()
        self._check(self._lib.tf_flowzip_last_band_sizes(self._h, out, room, C.byref(n)))
        return list(out[:n.value])

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tf_flowzip_destroy(self._h)
            self._h = C.c_void_p()
            self._room = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- numpy.round(flow).astype(int) on the device ---------------------------------------------------------------------------
_spare: dict = {}       # nbytes -> device buffers of rounded flows that are garbage, at most two each


class DeviceInt64Flow:
    """int64 (H, W, 2) in device memory: numpy.round(flow).astype(int) of a DeviceFlow.  The archive writer reads it where
    it is; anything else gets the host array."""

    dtype = np.dtype(np.int64)
    ndim = 3
    on_host = False     # (DeviceFlow's word for "the host values are the current ones": never, nothing writes here)

    def __init__(self, shape, buf, ready):
        self.shape = tuple(int(v) for v in shape)
        self._buf, self._ready, self._host = buf, ready, None

    @property
    def dev_ptr(self) -> int:
        return self._buf.ptr

    @property
    def nbytes(self) -> int:
        return int(np.prod(self.shape)) * 8

    def wait_on_stream(self) -> None:
        self._ready.stream_wait()

    def host(self) -> np.ndarray:
        if self._host is None:
            self.wait_on_stream()
            self._host = self._buf.download(self.shape, np.int64)
        return self._host

    def __array__(self, dtype=None, copy=None):
        a = self.host()
        if dtype is not None and np.dtype(dtype) != a.dtype:
            return a.astype(dtype)
        return a.copy() if copy else a

    def __len__(self) -> int:
        return self.shape[0]

    def __getitem__(self, key):
        return self.host()[key]

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.host(), name)

    def __del__(self):
        try:
            spare = _spare.setdefault(self._buf.nbytes, [])
            if len(spare) < 2:
                spare.append(self._buf)
        except Exception:
            pass


def round_i64_dev(flow) -> DeviceInt64Flow:
    """tf_flow_round_i64_dev of a DeviceFlow whose device copy is current."""
    from . import _lib
    from .device import DevBuffer
    from .deviceflow import _Event
    if np.dtype(flow.dtype) != np.float32:
        raise TypeError(f"the device rounds float32 flows for export, not {np.dtype(flow.dtype).name} ones")
    nbytes = flow.size * 8
    spare = _spare.get(nbytes)
    buf = spare.pop() if spare else DevBuffer(nbytes)
    flow.wait_on_stream()
    _lib.check(_lib.load().tf_flow_round_i64_dev(C.c_void_p(flow.dev_ptr), flow.size, 0, C.c_void_p(buf.ptr)))
    flow.mark_used()
    ready = _Event()
    ready.record()
    return DeviceInt64Flow(flow.shape, buf, ready)


class RoundedFlow(NDArrayOperatorsMixin):
    """numpy.round(flow) of a DeviceFlow, not yet computed.  `.astype(int)` is the device's int64 array; every other use
    computes numpy.round of the host values, as it would have been."""

    dtype = np.dtype(np.float32)
    ndim = 3

    def __init__(self, flow):
        self._flow = flow
        self.shape = flow.shape
        self._host = None

    def _value(self) -> np.ndarray:
        if self._host is None:
            self._host = np.round(self._flow.host())
        return self._host

    def astype(self, dtype, *args, **kwargs):
        if not args and not kwargs and np.dtype(dtype) == np.int64 and self._host is None and not self._flow.on_host:
            return round_i64_dev(self._flow)
        return self._value().astype(dtype, *args, **kwargs)

    def __array__(self, dtype=None, copy=None):
        a = self._value()
        if dtype is not None and np.dtype(dtype) != a.dtype:
            return a.astype(dtype)
        return a.copy() if copy else a

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        args = [x._value() if isinstance(x, RoundedFlow) else x for x in inputs]
        return getattr(ufunc, method)(*args, **kwargs)

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
