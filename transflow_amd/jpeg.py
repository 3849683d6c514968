"""Baseline JPEG of a frame that is on the device (tf_jpeg_*, transflow_amd/csrc/jpeg.hip).

The reference's MJPEG output serves `cv2.imencode(".jpg", frame, [IMWRITE_JPEG_QUALITY, 50])` of the last frame
(transflow/output/mjpeg.py:58-60): its product is a compressed frame.  `JpegEncoder` makes that file where the frame
is -- 8-bit YCbCr 4:2:0, the standard tables, a restart interval: the bytes of Pillow's
`save(quality=q, subsampling=2, restart_marker_blocks=r)` -- and only the file comes down, a few percent of the
(H, W, 3) array.  `JpegFrame` is what then travels: the bytes and four numbers.
"""
from __future__ import annotations

import ctypes as C
import io

import numpy as np


def pillow_encode(image: np.ndarray, quality: int, restart_mcus: int) -> bytes:
    """The same file made on the host by libjpeg (Pillow >= 10.2 for `restart_marker_blocks`): what a process without
    a GPU does with a raw frame (transflow_amd/output.py)."""
    import PIL
    import PIL.Image
    if tuple(int(v) for v in PIL.__version__.split(".")[:2]) < (10, 2):
        # an older save() ignores the option without a word: the file would announce an interval and hold no marker
        raise RuntimeError(f"Pillow {PIL.__version__} has no restart_marker_blocks; 10.2 or later is needed")
    buf = io.BytesIO()
    PIL.Image.fromarray(np.ascontiguousarray(image, dtype=np.uint8)).save(
        buf, format="JPEG", quality=int(quality), subsampling=2, restart_marker_blocks=int(restart_mcus))
    return buf.getvalue()


class JpegFrame:
    """A frame as a JPEG file: `data`, the `shape` (H, W, 3) of the image it decodes to, `quality`, `restart_mcus`."""

    __slots__ = ("data", "shape", "quality", "restart_mcus")

    def __init__(self, data: bytes, shape, quality: int, restart_mcus: int):
        self.data = bytes(data)
        self.shape = tuple(int(v) for v in shape)
        self.quality = int(quality)
        self.restart_mcus = int(restart_mcus)

    def __bytes__(self) -> bytes:
        return self.data

    def tobytes(self) -> bytes:
        return self.data

    def __len__(self) -> int:
        return len(self.data)

    def decode(self) -> np.ndarray:
        """The uint8 (H, W, 3) RGB array a viewer sees (Pillow's decoder)."""
        import PIL.Image
        with PIL.Image.open(io.BytesIO(self.data)) as im:
            return np.asarray(im.convert("RGB"))

    def __reduce__(self):
        return (JpegFrame, (self.data, self.shape, self.quality, self.restart_mcus))

    def __eq__(self, other):
        return isinstance(other, JpegFrame) and (self.data, self.shape, self.quality, self.restart_mcus) == (
            other.data, other.shape, other.quality, other.restart_mcus)

    __hash__ = None

    def __repr__(self):
        return f"JpegFrame({len(self.data)} bytes, shape={self.shape}, quality={self.quality}, restart_mcus={self.restart_mcus})"


class JpegEncoder:
    """tf_jpeg: one size, one quality, one restart interval; its device buffers are allocated once."""

    def __init__(self, height: int, width: int, quality: int = 50, restart_mcus: int | None = None):
        from . import _lib
        self._lib = _lib.load()
        self._check = _lib.check
        self.height, self.width, self.quality = int(height), int(width), int(quality)
        self._h = C.c_void_p()
        self._check(self._lib.tf_jpeg_create(C.byref(self._h), self.height, self.width, self.quality,
                                             0 if restart_mcus is None else int(restart_mcus)))
        self.header = self._header()
        # the interval the library chose is in the header's DRI segment, the 4 bytes before SOS's 14
        self.restart_mcus = int.from_bytes(self.header[-16:-14], "big") if restart_mcus is None else int(restart_mcus)
        self.last_needed = 0        # the size the last encode() reported, also when the buffer was too small
        self._out = None

    def _header(self) -> bytes:
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.tf_jpeg_header(self._h, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value)

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
            rc = self._lib.tf_jpeg_encode_dev(self._h, C.c_void_p(dev), dst, out.nbytes, C.byref(n))
        else:
            rc = self._lib.tf_jpeg_encode(self._h, C.c_void_p(host.ctypes.data), dst, out.nbytes, C.byref(n))
        self.last_needed = n.value
        self._check(rc)
        return n.value

    def encode(self, image) -> bytes:
        """The JPEG file of `image`: a uint8 (H, W, 3) ndarray, a DevicePixmap or a CompImage."""
        if self._out is None:       # most frames are a small part of this; one that is not makes the buffer grow
            self._out = np.empty(len(self.header) + self.height * self.width * 3 // 4 + 4096, np.uint8)
        try:
            n = self.encode_into(image, self._out)
        except ValueError:
            if self.last_needed <= self._out.nbytes:
                raise
            self._out = np.empty(self.last_needed, np.uint8)      # the intervals are still in the handle: pack and copy
            size = C.c_size_t()
            self._check(self._lib.tf_jpeg_copy_last(self._h, C.c_void_p(self._out.ctypes.data), self._out.nbytes,
                                                    C.byref(size)))
            n = size.value
        return self._out[:n].tobytes()

    def frame(self, image) -> JpegFrame:
        return JpegFrame(self.encode(image), (self.height, self.width, 3), self.quality, self.restart_mcus)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tf_jpeg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
