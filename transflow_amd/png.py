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


class PngFrame:
    """A frame as a PNG file: `data`, the `shape` (H, W, 3) of the image it decodes to, `band_rows`."""

    __slots__ = ("data", "shape", "band_rows")

    def __init__(self, data: bytes, shape, band_rows: int):
        self.data = bytes(data)
        self.shape = tuple(int(v) for v in shape)
        self.band_rows = int(band_rows)

    def __bytes__(self) -> bytes:
        return self.data

    def tobytes(self) -> bytes:
        return self.data

    def __len__(self) -> int:
        return len(self.data)

    def decode(self) -> np.ndarray:
        """The uint8 (H, W, 3) RGB array the file holds (Pillow's decoder)."""
        import PIL.Image
        with PIL.Image.open(io.BytesIO(self.data)) as im:
            return np.asarray(im.convert("RGB"))

    def __reduce__(self):
        return (PngFrame, (self.data, self.shape, self.band_rows))

    def __eq__(self, other):
        return isinstance(other, PngFrame) and (self.data, self.shape, self.band_rows) == (
            other.data, other.shape, other.band_rows)

    __hash__ = None

    def __repr__(self):
        return f"PngFrame({len(self.data)} bytes, shape={self.shape}, band_rows={self.band_rows})"


class PngEncoder:
    """tf_png: one size, one band height; its device buffers are allocated once."""

    def __init__(self, height: int, width: int, band_rows: int | None = None):
        from . import _lib
        self._lib = _lib.load()
        self._check = _lib.check
        self.height, self.width = int(height), int(width)
        self._h = C.c_void_p()
        self._check(self._lib.tf_png_create(C.byref(self._h), self.height, self.width,
                                            0 if band_rows is None else int(band_rows)))
        self.band_rows = int(self._lib.tf_png_band_rows(self._h))
        self.last_needed = 0        # the size the last encode() reported, also when the buffer was too small
        self._out = None

    def _source(self, image):
        """(device address or None, host array or None) of an ndarray, a DevicePixmap or a CompImage."""
        shape = (self.height, self.width, 3)
        if hasattr(image, "image_ptr"):                              # CompImage
            if (image.height, image.width) != shape[:2]:
                raise ValueError(f"the encoder is for {shape[:2]} frames, the image is {(image.height, image.width)}")
            return image.image_ptr(), None
        if tuple(image.shape) != shape:
            raise ValueError(f"the encoder is for {shape} frames, the image is {tuple(image.shape)}")
        if getattr(image, "dev_ptr", None) is not None:              # DevicePixmap
            image.wait_on_stream()
            return image.dev_ptr, None
        return None, np.ascontiguousarray(image, dtype=np.uint8)

    def encode_into(self, image, out: np.ndarray) -> int:
        """The file into `out` (uint8, C-contiguous); returns its size.  ValueError if it does not fit: `last_needed`
        then says how much room it takes, and `out` is as it was."""
        self.last_needed = 0
        dev, host = self._source(image)
        n = C.c_size_t()
        dst = C.c_void_p(out.ctypes.data)
        if dev is not None:
            rc = self._lib.tf_png_encode_dev(self._h, C.c_void_p(dev), dst, out.nbytes, C.byref(n))
        else:
            rc = self._lib.tf_png_encode(self._h, C.c_void_p(host.ctypes.data), dst, out.nbytes, C.byref(n))
        self.last_needed = n.value
        self._check(rc)
        return n.value

    def encode(self, image) -> bytes:
        """The PNG file of `image`: a uint8 (H, W, 3) ndarray, a DevicePixmap or a CompImage."""
        if self._out is None:       # rendered frames are a part of this; one that is not makes the buffer grow
            self._out = np.empty(self.height * self.width * 3 // 2 + 4096, np.uint8)
        try:
            n = self.encode_into(image, self._out)
        except ValueError:
            if self.last_needed <= self._out.nbytes:
                raise
            self._out = np.empty(self.last_needed, np.uint8)      # the bands are still in the handle: pack and copy
            size = C.c_size_t()
            self._check(self._lib.tf_png_copy_last(self._h, C.c_void_p(self._out.ctypes.data), self._out.nbytes,
                                                   C.byref(size)))
            n = size.value
        return self._out[:n].tobytes()

    def frame(self, image) -> PngFrame:
        return PngFrame(self.encode(image), (self.height, self.width, 3), self.band_rows)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tf_png_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
