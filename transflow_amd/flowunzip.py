"""Flow archive members inflated where the flow is wanted (tf_flowunzip_*, transflow_amd/csrc/flowunzip.hip).

The inverse of transflow_amd/flowzip.py for a member whose bands' compressed sizes are known -- the band index
`DeviceFlowArchiveWriter(index=True)` leaves in the archive: every band is inflated by a wave of
its own, the array's bytes land where the caller wants them in device memory, and only the `.npy` header and the CRC-32
come down.  `ArchiveFlowSource(device_inflate=True)` (transflow_amd/archive.py) replays archives through it.

A band is any sequence of deflate blocks with BFINAL 0 whose matches stay inside the band and whose last block ends on
the band's last bit: this package's bands and zlib's Z_FULL_FLUSH bands both are.  Anything else is rejected:
`BandRejected` names the first such band.
"""
from __future__ import annotations

import ctypes as C

import numpy as np


class BandRejected(ValueError):
    """A band of the member is no valid band (TF_ERR_STATE of tf_flowunzip_decode*)."""

    def __init__(self, band: int, message: str):
        ValueError.__init__(self, message)
        self.band = band


class FlowUnzipDecoder:
    """tf_flowunzip: its device buffers are allocated for the largest member seen so far.  The compressed bytes are
    staged in a page-locked buffer (`staging(n)`: read the member from the file straight into it, then pass the view)."""

    def __init__(self):
        from . import _lib
        self._lib = _lib.load()
        self._check = _lib.check
        self._err_state = _lib.TF_ERR_STATE
        self._last_error = self._lib.tf_last_error
        self._h = C.c_void_p()
        self._room = (0, 0)
        self._staging = None
        self._head = np.empty(4096, np.uint8)

    def staging(self, nbytes: int) -> np.ndarray:
        """`nbytes` of the page-locked staging buffer, as uint8 (valid until the next call)."""
        if self._staging is None or self._staging.nbytes < nbytes:
            from .device import pinned_empty
            self._staging = pinned_empty((max(nbytes, 1),), np.uint8)
        return self._staging[:nbytes]

    def _handle(self, stream_bytes: int, n_bands: int):
        if stream_bytes > self._room[0] or n_bands > self._room[1]:
            room = (max(stream_bytes, self._room[0]), max(n_bands, self._room[1]))
            self.close()
            self._check(self._lib.tf_flowunzip_create(C.byref(self._h), room[0], room[1]))
            self._room = room
        return self._h

    def _stage(self, stream) -> np.ndarray:
        view = np.frombuffer(stream, np.uint8) if not isinstance(stream, np.ndarray) else stream
        if self._staging is not None and view.size and np.shares_memory(view, self._staging):
            return view
        staged = self.staging(view.size)
        staged[...] = view
        return staged

    def _run(self, entry, stream, band_sizes, band_bytes: int, usize: int, split: int, data_ptr: int):
        staged = self._stage(stream)
        sizes = np.ascontiguousarray(band_sizes, dtype=np.uint32)
        h = self._handle(max(1, staged.size), max(1, sizes.size))
        crc, bad = C.c_uint32(), C.c_uint32()
        rc = entry(h, C.c_void_p(staged.ctypes.data), staged.size, C.c_void_p(sizes.ctypes.data), sizes.size, int(band_bytes),
                   int(usize), int(split), C.c_void_p(self._head.ctypes.data), C.c_void_p(data_ptr), C.byref(crc), C.byref(bad))
        if rc == self._err_state:
            message = self._last_error()
            raise BandRejected(int(bad.value), message.decode() if message else "a band was rejected")
        self._check(rc)
        return self._head[:split].tobytes(), int(crc.value)

    def decode_device(self, stream, band_sizes, band_bytes: int, usize: int, split: int, dev_ptr: int):
        """Inflates the member into device memory at dev_ptr (usize - split bytes): (the first `split` bytes, CRC-32)."""
        return self._run(self._lib.tf_flowunzip_decode_dev, stream, band_sizes, band_bytes, usize, split, int(dev_ptr))

    def decode(self, stream, band_sizes, band_bytes: int, usize: int, split: int = 0):
        """(the first `split` bytes, the other bytes, CRC-32) in host memory."""
        out = np.empty(max(1, usize - split), np.uint8)
        head, crc = self._run(self._lib.tf_flowunzip_decode, stream, band_sizes, band_bytes, usize, split, out.ctypes.data)
        return head, out[:usize - split].tobytes(), crc

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tf_flowunzip_destroy(self._h)
            self._h = C.c_void_p()
            self._room = (0, 0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def i64_to_f32_dev(src_ptr: int, n_values: int, dst_ptr: int) -> None:
    """tf_flow_i64_to_f32_dev: astype(float32) of int64 values in device memory; queued, does not wait."""
    from . import _lib
    _lib.check(_lib.load().tf_flow_i64_to_f32_dev(C.c_void_p(int(src_ptr)), int(n_values), C.c_void_p(int(dst_ptr))))
