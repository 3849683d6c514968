"""Baseline JPEG decoded where the frame is wanted (tf_jpegdec_*, transflow_amd/csrc/jpegdec.hip).

The inverse of transflow_amd/jpeg.py, for more than this package's own files: the compressed bytes go up the link (a
4K frame is about 2 MB instead of 25 MB), the restart intervals are decoded side by side on the device, and the pixels
-- libjpeg's, bit for bit -- are a `DevicePixmap` that never existed on the host.  A file the device does not take
(progressive, another sampling, a damaged scan ...) is rejected with a reason: `JpegRejected`; `decode_or_host` then
decodes it with Pillow.

`MjpegFrameProvider` is a frame provider for `HipFlowSource` (the protocol of `ArrayFrameProvider`,
transflow_amd/flow.py) over a raw MJPEG stream file, a `%0Nd.jpg` pattern or a sequence of files in memory.
"""
from __future__ import annotations

import ctypes as C
import io
import os

import numpy as np

from .pixmap import MJPEG_EXTS, DevicePixmap, _recorded_event  # noqa: F401  (MJPEG_EXTS: the one list of stream extensions)

# jpegdec_common.h's Reject (tests/jpegdec_ref.py mirrors the names)
REJECT_NAMES = ("ok", "not_jpeg", "truncated", "bad_segment", "progressive", "arithmetic", "sof_kind", "precision",
                "components", "sampling", "multi_scan", "dnl", "adobe_transform", "dqt_16bit", "missing_table", "bad_dht",
                "no_eoi", "stray_marker", "rst_count", "rst_order", "bad_code", "bad_symbol", "run_past_63", "category",
                "dc_range", "exhausted")


class JpegRejected(ValueError):
    """The device does not take the file: `reason` is the name of jpegdec_common.h's Reject."""

    def __init__(self, reason: str):
        ValueError.__init__(self, f"the device JPEG decoder does not take this file: {reason}")
        self.reason = reason


class JpegInfo:
    """tf_jpegdec_info: what the header says."""

    __slots__ = ("width", "height", "components", "h_samp", "v_samp", "restart_mcus", "intervals")

    def __init__(self, info):
        for name in self.__slots__:
            setattr(self, name, int(getattr(info, name)))

    def __repr__(self):
        return "JpegInfo(" + ", ".join(f"{n}={getattr(self, n)}" for n in self.__slots__) + ")"


def _bytes_of(data) -> bytes:
    return data.data if hasattr(data, "data") and isinstance(getattr(data, "data"), (bytes, bytearray)) else bytes(data)


def reject_name(reject: int) -> str:
    from . import _lib
    return _lib.load().tf_jpegdec_reject_name(int(reject)).decode()


def probe(data) -> JpegInfo:
    """The file's geometry from its header (no GPU call); `JpegRejected` for a header the device does not take."""
    from . import _lib
    raw = _bytes_of(data)
    info = _lib.TfJpegdecInfo()
    _lib.check(_lib.load().tf_jpegdec_probe(raw, len(raw), C.byref(info)))
    if info.reject:
        raise JpegRejected(reject_name(info.reject))
    return JpegInfo(info)


def pillow_decode(data, order: str = "rgb") -> np.ndarray:
    """The host's way: libjpeg through Pillow."""
    import PIL.Image
    rgb = np.array(PIL.Image.open(io.BytesIO(_bytes_of(data))).convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1]) if order == "bgr" else rgb


class JpegDecoder:
    """tf_jpegdec: frames of up to max_width x max_height; its device buffers are allocated once (and again for a file
    larger than any before it)."""

    ORDERS = {"rgb": 0, "bgr": 1}

    def __init__(self, max_width: int, max_height: int, device: int | None = None, max_file_bytes: int | None = None):
        from . import _lib
        self._lib = _lib.load()
        self._check = _lib.check
        if device is not None:
            self._check(self._lib.tf_init(int(device)))
        self.max_width, self.max_height = int(max_width), int(max_height)
        self._file_room = int(max_file_bytes) if max_file_bytes else self.max_width * self.max_height * 3 // 2 + 65536
        self._h = C.c_void_p()
        self._check(self._lib.tf_jpegdec_create(C.byref(self._h), self.max_width, self.max_height, self._file_room))
        self.fallbacks = 0

    def _room_for(self, nbytes: int) -> None:
        if nbytes > self._file_room:
            self.close()
            self._file_room = int(nbytes) * 2
            self._check(self._lib.tf_jpegdec_create(C.byref(self._h), self.max_width, self.max_height, self._file_room))

    def decode(self, data, order: str = "rgb", info: JpegInfo | None = None) -> DevicePixmap:
        """The file's pixels, uint8 (H, W, 3) in `order`, in device memory.  `JpegRejected` for a file the device does
        not take; ValueError for a frame larger than the decoder was made for.  info: `probe(data)`, from a caller
        that has looked at the header already."""
        from .pixmap import _dev_alloc
        raw = _bytes_of(data)
        if info is None:
            info = probe(raw)
        if info.width > self.max_width or info.height > self.max_height:
            raise ValueError(f"a frame of {info.width}x{info.height}; the decoder is for {self.max_width}x{self.max_height}")
        self._room_for(len(raw))
        buf = _dev_alloc(info.height * info.width * 3)
        reject = C.c_uint32()
        self._check(self._lib.tf_jpegdec_decode_dev(self._h, raw, len(raw), C.c_void_p(buf.ptr), self.ORDERS[order], C.byref(reject)))
        if reject.value:
            buf.close()
            raise JpegRejected(reject_name(reject.value))
        return DevicePixmap((info.height, info.width, 3), buf, _recorded_event())

    def decode_or_host(self, data, order: str = "rgb", info: JpegInfo | None = None) -> DevicePixmap:
        """`decode`, or Pillow's pixels sent up for a file the device rejects (`fallbacks` counts those)."""
        try:
            return self.decode(data, order, info)
        except JpegRejected:
            self.fallbacks += 1
            return DevicePixmap.from_host(pillow_decode(data, order))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tf_jpegdec_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def index_mjpeg_stream(data) -> list:
    """(offset, size) of every JPEG file of a raw MJPEG stream (files back to back, what `ffmpeg -f mjpeg` writes):
    the segments are walked by their lengths to SOS, and the file ends with the next FF D9 -- which cannot occur inside
    a scan, where an FF is followed by 00 or by RSTn."""
    out, at, n = [], 0, len(data)
    while True:
        at = data.find(b"\xff\xd8", at)
        if at < 0:
            return out
        p = at + 2
        while p + 4 <= n and data[p] == 0xFF and data[p + 1] != 0xDA:
            p += 2 + int.from_bytes(data[p + 2:p + 4], "big")
        if p + 4 > n or data[p] != 0xFF:
            return out
        end = data.find(b"\xff\xd9", p + 2 + int.from_bytes(data[p + 2:p + 4], "big"))
        if end < 0:
            return out
        out.append((at, end + 2 - at))
        at = end + 2


class MjpegFrameProvider:
    """A frame provider (transflow_amd/flow.py: `width`, `height`, `framerate`, `frame_count`, `seek_start`, `read`,
    `release`) whose frames are JPEG files decoded on the device.

    source: a raw MJPEG stream file (.mjpeg / .mjpg), a `%0Nd.jpg` pattern (numbered from the first of 0 or 1 that
    exists), or a sequence of `bytes` / `JpegFrame`.  `read()` returns a BGR `DevicePixmap`: `HipFlowSource` hands
    it to a Farnebäck handle by its device address, and `np.asarray` of it is the host frame for everything else.
    With `require_restart`, a frame without a restart interval is decoded on the host (one wave would decode the whole
    frame otherwise); `fallbacks` counts the frames that went that way, rejected ones included.  `device_decode=False`
    decodes every frame with Pillow.  Containers (AVI ...) are not read."""

    def __init__(self, source, framerate: float = 25.0, size=None, device_decode: bool = True, require_restart: bool = True,
                 device: int | None = None):
        self.framerate = float(framerate)
        self.device_decode, self.require_restart, self.device = bool(device_decode), bool(require_restart), device
        self._data = None
        if isinstance(source, (str, os.PathLike)):
            path = os.fspath(source)
            if "%" in path:
                first = next((k for k in (0, 1) if os.path.isfile(path % k)), None)
                if first is None:
                    raise FileNotFoundError(f"no frame {path % 0} or {path % 1}")
                self._files = []
                k = first
                while os.path.isfile(path % k):
                    self._files.append(path % k)
                    k += 1
                self._get = self._file_frame
                self.frame_count = len(self._files)
            else:
                self._stream_path = path
                self._index = index_mjpeg_stream(self._stream())     # the file is mapped, not read: a clip can be gigabytes
                self._get = self._stream_frame
                self.frame_count = len(self._index)
        else:
            self._frames = list(source)
            self._get = self._memory_frame
            self.frame_count = len(self._frames)
        if self.frame_count == 0:
            raise ValueError("the MJPEG source holds no frame")
        first = self._get(0)
        try:
            info = probe(first)
            self._frame_size = (info.width, info.height)
        except JpegRejected:
            import PIL.Image
            self._frame_size = PIL.Image.open(io.BytesIO(first)).size
        self.width, self.height = self._frame_size if size is None else (int(size[0]), int(size[1]))
        self._decoder = None
        self._host_fallbacks = 0
        self.pos = 0

    def _stream(self):
        if self._data is None:
            import mmap
            with open(self._stream_path, "rb") as f:
                self._data = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if os.fstat(f.fileno()).st_size else b""
        return self._data

    def _stream_frame(self, i: int) -> bytes:
        at, size = self._index[i]
        return self._stream()[at:at + size]

    def __getstate__(self):                          # a mapping and a decoder's handle belong to their process
        state = dict(self.__dict__)
        if getattr(self, "_stream_path", None) is not None:
            state["_data"] = None
        if state.get("_decoder") is not None:
            state["_host_fallbacks"] = self.fallbacks
            state["_decoder"] = None
        state.pop("_get", None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        if getattr(self, "_stream_path", None) is not None:
            self._get = self._stream_frame
        elif hasattr(self, "_files"):
            self._get = self._file_frame
        else:
            self._get = self._memory_frame

    def _file_frame(self, i: int) -> bytes:
        with open(self._files[i], "rb") as f:
            return f.read()

    def _memory_frame(self, i: int) -> bytes:
        return _bytes_of(self._frames[i])

    @property
    def fallbacks(self) -> int:
        return self._host_fallbacks + (self._decoder.fallbacks if self._decoder is not None else 0)

    def seek_start(self):
        self.pos = 0

    def decode_frame(self, index: int, order: str = "bgr") -> DevicePixmap:
        raw = self._get(index)
        if not self.device_decode:
            self._host_fallbacks += 1
            return DevicePixmap.from_host(pillow_decode(raw, order))
        try:
            info = probe(raw)
        except JpegRejected:
            info = None
        if info is None or (self.require_restart and info.restart_mcus == 0):
            self._host_fallbacks += 1
            return DevicePixmap.from_host(pillow_decode(raw, order))
        if self._decoder is None or info.width > self._decoder.max_width or info.height > self._decoder.max_height:
            room = (max(info.width, self._frame_size[0]), max(info.height, self._frame_size[1]))
            if self._decoder is not None:            # a larger frame: the old handle's buffers go now, not with the collector
                room = (max(room[0], self._decoder.max_width), max(room[1], self._decoder.max_height))
                self._host_fallbacks += self._decoder.fallbacks
                self._decoder.close()
            self._decoder = JpegDecoder(room[0], room[1], self.device)
        return self._decoder.decode_or_host(raw, order, info)

    def read(self, order: str = "bgr"):
        if self.pos >= self.frame_count:
            return None
        frame = self.decode_frame(self.pos, order)
        self.pos += 1
        return frame

    def release(self):
        if self._decoder is not None:
            self._host_fallbacks += self._decoder.fallbacks
            self._decoder.close()
            self._decoder = None
        if getattr(self, "_stream_path", None) is not None and self._data is not None:
            if hasattr(self._data, "close"):
                self._data.close()
            self._data = None
