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

from .framecodec import CompressedFrameProvider, FrameDecoder, bytes_of as _bytes_of, pillow_decode
from .pixmap import MJPEG_EXTS, DevicePixmap  # noqa: F401  (MJPEG_EXTS: the one list of stream extensions)

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


class JpegDecoder(FrameDecoder):
    """tf_jpegdec: frames of up to max_width x max_height.

    parallel_scan: a file without a restart interval -- one interval, hence one wave and seconds a frame otherwise -- is
    cut into subsequences of bytes that are decoded side by side (tf_jpegdec_set_scan_mode 1; DESIGN.md section 19,
    "scans without restart markers"): the same pixels and the same verdicts.  Files with a restart interval go the way
    they always went.  Measured on one MI355X: a 4K quality-90 4:2:0 frame 2.95 ms (the one-wave
    path 1394 ms, Pillow 41.0 ms), 1080p 2.18 ms (346 ms, Pillow 5.8 ms); a 1080p frame of noise at quality 100 35.5 ms,
    SLOWER than Pillow's 18.4 ms -- such a file stays out of step for tens of KB.  Off by default."""

    CREATE, DECODE_DEV, DESTROY = "tf_jpegdec_create", "tf_jpegdec_decode_dev", "tf_jpegdec_destroy"

    def __init__(self, max_width: int, max_height: int, device: int | None = None, max_file_bytes: int | None = None,
                 parallel_scan: bool = False):
        self.parallel_scan = bool(parallel_scan)
        FrameDecoder.__init__(self, max_width, max_height, device, max_file_bytes)

    def _create(self) -> None:
        FrameDecoder._create(self)
        if self.parallel_scan:
            self._check(self._lib.tf_jpegdec_set_scan_mode(self._h, 1))

    def par_stats(self) -> dict:
        """tf_jpegdec_par_stats of the last decode that took the parallel path."""
        out = (C.c_uint32 * 4)()
        self._check(self._lib.tf_jpegdec_par_stats(self._h, out))
        return dict(zip(("subsequences", "groups", "launches", "rounds"), (int(v) for v in out)))

    def _verdict(self, rc: int, reject: int) -> None:
        self._check(rc)
        if reject:
            raise JpegRejected(reject_name(reject))

    def decode(self, data, order: str = "rgb", info: JpegInfo | None = None) -> DevicePixmap:
        """The file's pixels, uint8 (H, W, 3) in `order`, in device memory.  `JpegRejected` for a file the device does
        not take; ValueError for a frame larger than the decoder was made for.  info: `probe(data)`, from a caller
        that has looked at the header already."""
        raw = _bytes_of(data)
        return self._decode(raw, order, probe(raw) if info is None else info)

    def decode_or_host(self, data, order: str = "rgb", info: JpegInfo | None = None) -> DevicePixmap:
        """`decode`, or Pillow's pixels sent up for a file the device rejects (`fallbacks` counts those)."""
        try:
            return self.decode(data, order, info)
        except JpegRejected:
            self.fallbacks += 1
            return DevicePixmap.from_host(pillow_decode(data, order))


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


class MjpegFrameProvider(CompressedFrameProvider):
    """A `CompressedFrameProvider` of JPEG files.

    source: a raw MJPEG stream file (.mjpeg / .mjpg), a `%0Nd.jpg` pattern, or a sequence of `bytes` / `JpegFrame`.
    With `require_restart`, a frame without a restart interval is decoded on the host (one wave would decode the whole
    frame otherwise); `fallbacks` counts the frames that went that way, rejected ones included.  With `parallel_scan`
    such a frame is decoded on the device whatever `require_restart` says, by `JpegDecoder(parallel_scan=True)` (its
    docstring has the times: faster than Pillow at ordinary qualities, slower on noise at quality 100); everything else
    routes as without it.  `device_decode=False` decodes every frame with Pillow.  Containers (AVI ...)
    are not read."""

    DECODER, EMPTY = JpegDecoder, "the MJPEG source holds no frame"
    _stream_path = _data = None
    parallel_scan = False                            # (a provider pickled before the option existed)

    def __init__(self, source, framerate: float = 25.0, size=None, device_decode: bool = True, require_restart: bool = True,
                 device: int | None = None, parallel_scan: bool = False):
        self.require_restart = bool(require_restart)
        self.parallel_scan = bool(parallel_scan)
        CompressedFrameProvider.__init__(self, source, framerate, size, device_decode, device)

    def _open_path(self, path: str) -> int:
        if "%" in path:
            return CompressedFrameProvider._open_path(self, path)
        self._stream_path = path
        self._index = index_mjpeg_stream(self._stream())         # the file is mapped, not read: a clip can be gigabytes
        return len(self._index)

    def _first_size(self, raw: bytes):
        try:
            info = probe(raw)
            return info.width, info.height
        except JpegRejected:
            import PIL.Image
            return PIL.Image.open(io.BytesIO(raw)).size

    def _stream(self):
        if self._data is None:
            import mmap
            with open(self._stream_path, "rb") as f:
                self._data = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if os.fstat(f.fileno()).st_size else b""
        return self._data

    def _get(self, i: int) -> bytes:
        if self._stream_path is None:
            return CompressedFrameProvider._get(self, i)
        at, size = self._index[i]
        return self._stream()[at:at + size]

    def __getstate__(self):                          # a mapping belongs to its process, as the decoder's handle does
        state = CompressedFrameProvider.__getstate__(self)
        state.pop("_data", None)
        return state

    def decode_frame(self, index: int, order: str = "bgr") -> DevicePixmap:
        raw = self._get(index)
        if not self.device_decode:
            return self._host_frame(raw, order)
        try:
            info = probe(raw)
        except JpegRejected:
            info = None
        if info is None or (self.require_restart and not self.parallel_scan and info.restart_mcus == 0):
            return self._host_frame(raw, order)
        return self._decoder_for(info).decode_or_host(raw, order, info)

    def _new_decoder(self, max_width: int, max_height: int) -> FrameDecoder:
        if not self.parallel_scan:
            return CompressedFrameProvider._new_decoder(self, max_width, max_height)
        return self.DECODER(max_width, max_height, self.device, parallel_scan=True)

    def release(self):
        self._drop_decoder()
        if hasattr(self._data, "close"):
            self._data.close()
        self._data = None
