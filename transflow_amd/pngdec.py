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
import os

from .framecodec import CompressedFrameProvider, FrameDecoder, bytes_of as _bytes_of, pillow_decode
from .pixmap import DevicePixmap

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


class PngDecoder(FrameDecoder):
    """tf_pngdec: frames of up to max_width x max_height."""

    CREATE, DECODE_DEV, DESTROY = "tf_pngdec_create", "tf_pngdec_decode_dev", "tf_pngdec_destroy"

    def _verdict(self, rc: int, reject: int) -> None:
        if rc == self._state and reject:
            raise _rejected(reject)
        self._check(rc)

    def decode(self, data, order: str = "rgb", info: PngInfo | None = None) -> DevicePixmap:
        """The file's pixels, uint8 (H, W, 3) in `order`, in device memory.  `PngRejected` for a malformed file and for
        one the device finds corrupt; ValueError for a file that is not for the device (`probe(data).indexed`), for one
        that asks more of the device than an untrusted file may (`probe(data).within_bound`: a band of at most 1 MiB
        and of at most twice that and 1024 compressed bytes) and for a frame larger than the decoder was made for.
        `decode_or_host` takes the first two the host's way.  info: `probe(data)`, from a caller that has looked
        already."""
        raw = _bytes_of(data)
        if info is None:
            info = probe(raw)
        if not info.indexed:
            raise ValueError(f"not a file for the device: {info.why_not}")
        if not info.within_bound:
            raise ValueError(f"a band of {info.band_bytes} bytes in up to {info.max_band_bytes} compressed: beyond the bound on "
                             f"what goes to the device ({MAX_BAND_BYTES}, {max_band_compressed(info.band_bytes)})")
        return self._decode(raw, order, info)

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


def is_png_sequence(path) -> bool:
    """A path with a `%...d` field that ends in .png and whose first frame (0 or 1) exists."""
    import re
    if not isinstance(path, str) or not path.lower().endswith(".png") or re.search(r"%\d*d", path) is None:
        return False
    try:
        return any(os.path.isfile(path % k) for k in (0, 1))
    except (TypeError, ValueError):
        return False


class PngSequenceFrameProvider(CompressedFrameProvider):
    """A `CompressedFrameProvider` of PNG files.

    source: a `%0Nd.png` pattern or a sequence of `bytes` / `PngFrame`.  A frame without a band index, or of another
    kind of PNG, is decoded by Pillow; `fallbacks` counts the frames that went that way.  A malformed or corrupt frame
    raises `PngRejected` with the frame's number.  `device_decode=False` decodes every frame with Pillow."""

    DECODER, EMPTY = PngDecoder, "the PNG sequence holds no frame"

    def __init__(self, source, framerate: float = 25.0, size=None, device_decode: bool = True, device: int | None = None):
        CompressedFrameProvider.__init__(self, source, framerate, size, device_decode, device)

    def _first_size(self, raw: bytes):
        try:
            info = probe(raw)
        except PngRejected as err:
            raise PngRejected(err.reason, err.where, 0) from None
        return info.width, info.height

    def decode_frame(self, index: int, order: str = "bgr") -> DevicePixmap:
        raw = self._get(index)
        try:
            info = probe(raw)
            if not self.device_decode or not info.indexed:
                return self._host_frame(raw, order)
            return self._decoder_for(info).decode_or_host(raw, order, info)
        except PngRejected as err:
            raise PngRejected(err.reason, err.where, index) from None
