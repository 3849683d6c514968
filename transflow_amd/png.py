"""PNG of a frame that is on the device (tf_png_*, transflow_amd/csrc/png.hip).

The reference's frame-sequence output writes `cv2.imwrite(template % counter, frame)` (transflow/output/frames.py): its
product is a lossless compressed frame.  `PngEncoder` makes that file where the frame is -- 8-bit RGB, every row
filtered, the zlib stream cut into bands that are coded side by side -- and only the file comes
down.  Any PNG decoder returns the frame's pixels exactly.  `PngFrame` is what then travels: the bytes and the shape.
"""
from __future__ import annotations

import ctypes as C
import io

import numpy as np

from .framecodec import EncodedFrame, FrameEncoder


def pillow_encode_png(image: np.ndarray) -> bytes:
    """A PNG of the same pixels made on the host by Pillow (zlib level 1): what a process without a GPU does with a
    raw frame (transflow_amd/output.py).  Not the same bytes as the device's file; the same picture."""
    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(np.ascontiguousarray(image, dtype=np.uint8)).save(buf, format="PNG", compress_level=1)
    return buf.getvalue()


def default_band_rows(height: int, width: int) -> int:
    """The rows of a band the library chooses for this size, asked of the library (the call loads it and touches no
    GPU)."""
    from . import _lib
    return int(_lib.load().tf_png_default_band_rows(int(height), int(width)))


def code_lengths() -> list:
    """The lengths of the library's literal/length code, 286 symbols (no GPU)."""
    from . import _lib
    out = (C.c_uint8 * 286)()
    _lib.check(_lib.load().tf_png_code_lengths(out))
    return list(out)


class PngFrame(EncodedFrame):
    """A frame as a PNG file: `data`, the `shape` (H, W, 3) of the image it decodes to, `band_rows`."""

    __slots__ = ("band_rows",)

    def __init__(self, data: bytes, shape, band_rows: int):
        super().__init__(data, shape)
        self.band_rows = int(band_rows)


class PngEncoder(FrameEncoder):
    """tf_png: one size, one band height; its device buffers are allocated once."""

    ENCODE_DEV, ENCODE, COPY_LAST, DESTROY = "tf_png_encode_dev", "tf_png_encode", "tf_png_copy_last", "tf_png_destroy"

    CODES = {"fixed": 0, "frame": 1}

    def __init__(self, height: int, width: int, band_rows: int | None = None, index: bool = False, code: str = "fixed"):
        """index: the files carry the band index (the ancillary chunk tfBX) that lets
        transflow_amd/pngdec.py decode them on the device; without it they are the bytes they always were.
        code: "fixed", the library's constant literal/length code; "frame", the code of the frame's own tokens, and a
        band that would not shrink stored: smaller files, the same pixels."""
        if code not in self.CODES:
            raise ValueError(f"code {code!r}: one of {sorted(self.CODES)}")
        super().__init__(height, width)
        self._check(self._lib.tf_png_create(C.byref(self._h), self.height, self.width,
                                            0 if band_rows is None else int(band_rows)))
        self.band_rows = int(self._lib.tf_png_band_rows(self._h))
        self.index = bool(index)
        if self.index:
            self._check(self._lib.tf_png_set_index(self._h, 1))
        self.code = "fixed"
        self.set_code(code)

    def set_code(self, code: str) -> None:
        """The code of the later encodes (no GPU call)."""
        if code not in self.CODES:
            raise ValueError(f"code {code!r}: one of {sorted(self.CODES)}")
        self._check(self._lib.tf_png_set_code(self._h, self.CODES[code]))
        self.code = code

    def last_code(self):
        """(the 286 code lengths, how often the weights were halved) of the last frame encoded with code="frame"."""
        lengths, repairs = (C.c_uint8 * 286)(), C.c_uint32()
        self._check(self._lib.tf_png_last_code(self._h, lengths, C.byref(repairs)))
        return list(lengths), int(repairs.value)

    def last_bands(self):
        """(the bytes of each band's deflate data, whether each band is stored) of the same frame."""
        n_bands = -(-self.height // self.band_rows)
        sizes, stored, n = (C.c_uint32 * n_bands)(), (C.c_uint8 * n_bands)(), C.c_size_t()
        self._check(self._lib.tf_png_last_bands(self._h, sizes, stored, n_bands, C.byref(n)))
        return list(sizes[:n.value]), [bool(v) for v in stored[:n.value]]

    def _first_capacity(self) -> int:   # rendered frames are a part of this
        return self.height * self.width * 3 // 2 + 4096

    def frame(self, image) -> PngFrame:
        return PngFrame(self.encode(image), (self.height, self.width, 3), self.band_rows)
