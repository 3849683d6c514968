"""Banded PNG frames decoded where the frame is wanted (tf_pngdec_*, transflow_amd/csrc/pngdec.hip).

The inverse of transflow_amd/png.py for the files it writes with `PngEncoder(index=True)`: the compressed file goes up
the link, its bands are inflated side by side, the row filters are undone on the device, and the pixels are a
`DevicePixmap` that never existed on the host.  `probe` sorts a file into one of three: indexed (for the device), a
well-formed PNG of another kind (no index, another colour type or depth, interlaced: Pillow decodes it, which is no
error), or rejected with a reason: `PngRejected`.  Corrupt data is never masked by a fallback.

`PngSequenceFrameProvider` is a frame provider for `HipFlowSource` (the protocol of `ArrayFrameProvider`,
transflow_amd/flow.py) over a `%0Nd.png` pattern or a sequence of files in memory.
"""
from __future__ import annotations

import ctypes as C
import io
import os

import numpy as np

from .pixmap import DevicePixmap, _recorded_event

# pngdec_common.h's Reject (tests/pngdec_ref.py has the same names)
REJECT_NAMES = {0: "ok", 1: "signature", 2: "truncated", 3: "ihdr", 4: "size", 5: "index", 6: "zlib_header", 7: "tail",
                8: "no_iend", 9: "idat_order", 10: "chunk_crc", 11: "adler", 12: "filter_type", 17: "band_bfinal",
                18: "band_btype", 19: "band_stored_len", 20: "band_bad_code", 21: "band_repeat_first",
                22: "band_repeat_past", 23: "band_bad_symbol", 24: "band_distance", 25: "band_overrun", 26: "band_short",
                27: "band_exhausted"}
WHY_NOT = ("indexed", "no_index", "format", "interlaced", "version")
# The bound on what an untrusted file may ask of the device (DESIGN.md sections 18 and 20): a band's decoding time is
# bounded by its compressed bits.
MAX_BAND_BYTES = 1 << 20


def max_band_compressed(band_bytes: int) -> int:
    return 2 * int(band_bytes) + 1024


class PngRejected(ValueError):
    """The file is malformed, or the device found it corrupt: `reason` is the name of pngdec_common.h's Reject, `where`
    the chunk (chunk_crc), the row (filter_type) or the band (band_*) where there is one, `frame` the frame of a
    sequence."""

    def __init__(self, reason: str, where: int | None = None, frame=None):
        at = "" if where is None else f" at {where}"
        of = "" if frame is None else f" (frame {frame})"
        ValueError.__init__(self, f"the PNG file is rejected: {reason}{at}{of}")
        self.reason, self.where, self.frame = reason, where, frame


def _rejected(word: int, frame=None) -> PngRejected:
    reason = word & 0xFF
    has_where = reason == 10 or reason == 12 or reason >= 16
    return PngRejected(reject_name(word), (word >> 8) if has_where else None, frame)


class PngInfo:
    """tf_pngdec_info: what the chunks say.  `indexed`: a file for the device; else `why_not` names why it is not
    ("no_index", "format", "interlaced", "version").  `bands`: (offset, size) of every band's compressed bytes."""

    __slots__ = ("width", "height", "band_rows", "n_bands", "indexed", "why_not", "max_band_bytes", "bands")

    def __init__(self, info, bands=()):
        for name in ("width", "height", "band_rows", "n_bands", "max_band_bytes"):
            setattr(self, name, int(getattr(info, name)))
        self.indexed = bool(info.indexed)
        self.why_not = WHY_NOT[int(info.why_not)]
        self.bands = list(bands)

    @property
    def band_bytes(self) -> int:
        """The filtered bytes of a whole band."""
        return self.band_rows * (1 + 3 * self.width)

    @property
    def within_bound(self) -> bool:
        """Whether the file asks no more of the device than an untrusted file may."""
        return self.band_bytes <= MAX_BAND_BYTES and self.max_band_bytes <= max_band_compressed(self.band_bytes)

    def __repr__(self):
        return "PngInfo(" + ", ".join(f"{n}={getattr(self, n)}" for n in self.__slots__[:-1]) + ")"


def _bytes_of(data) -> bytes:
    return data.data if hasattr(data, "data") and isinstance(getattr(data, "data"), (bytes, bytearray)) else bytes(data)


def reject_name(reject: int) -> str:
    from . import _lib
    return _lib.load().tf_pngdec_reject_name(int(reject)).decode()


def probe(data) -> PngInfo:
    """What kind of file this is, from its chunks (no GPU call; the CRCs are the decoder's to check).  `PngRejected` for
    a malformed file."""
    from . import _lib
    lib = _lib.load()
    raw = _bytes_of(data)
    info = _lib.TfPngdecInfo()
    _lib.check(lib.tf_pngdec_probe(raw, len(raw), C.byref(info)))
    if info.reject:
        raise _rejected(info.reject)
    bands = ()
    if info.indexed:
        n = int(info.n_bands)
        offsets, sizes = (C.c_uint32 * n)(), (C.c_uint32 * n)()
        info.band_offsets, info.band_sizes, info.band_capacity = offsets, sizes, n
        _lib.check(lib.tf_pngdec_probe(raw, len(raw), C.byref(info)))
        bands = list(zip(offsets, sizes))
    return PngInfo(info, bands)


def pillow_decode(data, order: str = "rgb") -> np.ndarray:
    """The host's way: Pillow."""
    import PIL.Image
    rgb = np.array(PIL.Image.open(io.BytesIO(_bytes_of(data))).convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1]) if order == "bgr" else rgb


class PngDecoder:
    """tf_pngdec: frames of up to max_width x max_height; its staging and device buffers are allocated once (and again
    for a file larger than any before it)."""

    ORDERS = {"rgb": 0, "bgr": 1}

    def __init__(self, max_width: int, max_height: int, device: int | None = None, max_file_bytes: int | None = None):
        from . import _lib
        self._lib = _lib.load()
        self._check = _lib.check
        self._state = _lib.TF_ERR_STATE
        if device is not None:
            self._check(self._lib.tf_init(int(device)))
        self.max_width, self.max_height = int(max_width), int(max_height)
        self._file_room = int(max_file_bytes) if max_file_bytes else self.max_width * self.max_height * 3 // 2 + 65536
        self._h = C.c_void_p()
        self._check(self._lib.tf_pngdec_create(C.byref(self._h), self.max_width, self.max_height, self._file_room))
        self.fallbacks = 0

    def _room_for(self, nbytes: int) -> None:
        if nbytes > self._file_room:
            self.close()
            self._file_room = int(nbytes) * 2
            self._check(self._lib.tf_pngdec_create(C.byref(self._h), self.max_width, self.max_height, self._file_room))

    def decode(self, data, order: str = "rgb", info: PngInfo | None = None) -> DevicePixmap:
        """The file's pixels, uint8 (H, W, 3) in `order`, in device memory.  `PngRejected` for a malformed file and for
        one the device finds corrupt; ValueError for a file that is not for the device (`probe(data).indexed`), for one
        that asks more of the device than an untrusted file may (`probe(data).within_bound`: a band of at most 1 MiB
        and of at most twice that and 1024 compressed bytes) and for a frame larger than the decoder was made for.
        `decode_or_host` takes the first two the host's way.  info: `probe(data)`, from a caller that has looked
        already."""
        from .pixmap import _dev_alloc
        raw = _bytes_of(data)
        if info is None:
            info = probe(raw)
        if not info.indexed:
            raise ValueError(f"not a file for the device: {info.why_not}")
        if not info.within_bound:
            raise ValueError(f"a band of {info.band_bytes} bytes in up to {info.max_band_bytes} compressed: beyond the bound on "
                             f"what goes to the device ({MAX_BAND_BYTES}, {max_band_compressed(info.band_bytes)})")
        if info.width > self.max_width or info.height > self.max_height:
            raise ValueError(f"a frame of {info.width}x{info.height}; the decoder is for {self.max_width}x{self.max_height}")
        self._room_for(len(raw))
        buf = _dev_alloc(info.height * info.width * 3)
        reject = C.c_uint32()
        rc = self._lib.tf_pngdec_decode_dev(self._h, raw, len(raw), C.c_void_p(buf.ptr), self.ORDERS[order], C.byref(reject))
        if rc != 0:
            buf.close()
            if rc == self._state and reject.value:
                raise _rejected(reject.value)
            self._check(rc)
        return DevicePixmap((info.height, info.width, 3), buf, _recorded_event())

    def decode_or_host(self, data, order: str = "rgb", info: PngInfo | None = None) -> DevicePixmap:
        """`decode`, or Pillow's pixels sent up for a file that is not for the device or asks more of it than an
        untrusted file may (`fallbacks` counts those).  A malformed or corrupt file raises `PngRejected` all the same."""
        raw = _bytes_of(data)
        if info is None:
            info = probe(raw)
        if not info.indexed or not info.within_bound:
            self.fallbacks += 1
            return DevicePixmap.from_host(pillow_decode(raw, order))
        return self.decode(raw, order, info)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tf_pngdec_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def is_png_sequence(path) -> bool:
    """A path with a `%...d` field that ends in .png and whose first frame (0 or 1) exists."""
    import re
    if not isinstance(path, str) or not path.lower().endswith(".png") or re.search(r"%\d*d", path) is None:
        return False
    try:
        return any(os.path.isfile(path % k) for k in (0, 1))
    except (TypeError, ValueError):
        return False


class PngSequenceFrameProvider:
    """A frame provider (transflow_amd/flow.py: `width`, `height`, `framerate`, `frame_count`, `seek_start`, `read`,
    `release`) whose frames are PNG files decoded on the device.

    source: a `%0Nd.png` pattern (numbered from the first of 0 or 1 that exists) or a sequence of `bytes` /
    `PngFrame`.  `read()` returns a BGR `DevicePixmap`: `HipFlowSource` hands it to a Farnebäck handle by its device
    address, and `np.asarray` of it is the host frame for everything else.  A frame without a band index, or of another
    kind of PNG, is decoded by Pillow; `fallbacks` counts the frames that went that way.  A malformed or corrupt frame
    raises `PngRejected` with the frame's number.  `device_decode=False` decodes every frame with Pillow."""

    def __init__(self, source, framerate: float = 25.0, size=None, device_decode: bool = True, device: int | None = None):
        self.framerate = float(framerate)
        self.device_decode, self.device = bool(device_decode), device
        if isinstance(source, (str, os.PathLike)):
            path = os.fspath(source)
            first = next((k for k in (0, 1) if os.path.isfile(path % k)), None)
            if first is None:
                raise FileNotFoundError(f"no frame {path % 0} or {path % 1}")
            self._files = []
            k = first
            while os.path.isfile(path % k):
                self._files.append(path % k)
                k += 1
            self.frame_count = len(self._files)
        else:
            self._frames = list(source)
            self.frame_count = len(self._frames)
        if self.frame_count == 0:
            raise ValueError("the PNG sequence holds no frame")
        try:
            info = probe(self._get(0))
        except PngRejected as err:
            raise PngRejected(err.reason, err.where, 0) from None
        self._frame_size = (info.width, info.height)
        self.width, self.height = self._frame_size if size is None else (int(size[0]), int(size[1]))
        self._decoder = None
        self._host_fallbacks = 0
        self.pos = 0

    def _get(self, i: int) -> bytes:
        if hasattr(self, "_files"):
            with open(self._files[i], "rb") as f:
                return f.read()
        return _bytes_of(self._frames[i])

    def __getstate__(self):                          # a decoder's handle belongs to its process
        state = dict(self.__dict__)
        if state.get("_decoder") is not None:
            state["_host_fallbacks"] = self.fallbacks
            state["_decoder"] = None
        return state

    @property
    def fallbacks(self) -> int:
        return self._host_fallbacks + (self._decoder.fallbacks if self._decoder is not None else 0)

    def seek_start(self):
        self.pos = 0

    def decode_frame(self, index: int, order: str = "bgr") -> DevicePixmap:
        raw = self._get(index)
        try:
            info = probe(raw)
            if not self.device_decode or not info.indexed:
                self._host_fallbacks += 1
                return DevicePixmap.from_host(pillow_decode(raw, order))
            if self._decoder is None or info.width > self._decoder.max_width or info.height > self._decoder.max_height:
                room = (max(info.width, self._frame_size[0]), max(info.height, self._frame_size[1]))
                if self._decoder is not None:        # a larger frame: the old handle's buffers go now, not with the collector
                    room = (max(room[0], self._decoder.max_width), max(room[1], self._decoder.max_height))
                    self._host_fallbacks += self._decoder.fallbacks
                    self._decoder.close()
                self._decoder = PngDecoder(room[0], room[1], self.device)
            return self._decoder.decode_or_host(raw, order, info)
        except PngRejected as err:
            raise PngRejected(err.reason, err.where, index) from None

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
