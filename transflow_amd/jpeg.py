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

from .framecodec import EncodedFrame, FrameEncoder


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


class JpegFrame(EncodedFrame):
    """A frame as a JPEG file: `data`, the `shape` (H, W, 3) of the image it decodes to, `quality`, `restart_mcus`."""

    __slots__ = ("quality", "restart_mcus")

    def __init__(self, data: bytes, shape, quality: int, restart_mcus: int):
        super().__init__(data, shape)
        self.quality = int(quality)
        self.restart_mcus = int(restart_mcus)


class JpegEncoder(FrameEncoder):
    """tf_jpeg: one size, one quality, one restart interval; its device buffers are allocated once."""

    ENCODE_DEV, ENCODE, COPY_LAST, DESTROY = "tf_jpeg_encode_dev", "tf_jpeg_encode", "tf_jpeg_copy_last", "tf_jpeg_destroy"

    def __init__(self, height: int, width: int, quality: int = 50, restart_mcus: int | None = None):
        super().__init__(height, width)
        self.quality = int(quality)
        self._check(self._lib.tf_jpeg_create(C.byref(self._h), self.height, self.width, self.quality,
                                             0 if restart_mcus is None else int(restart_mcus)))
        self.header = self._header()
        # the interval the library chose is in the header's DRI segment, the 4 bytes before SOS's 14
        self.restart_mcus = int.from_bytes(self.header[-16:-14], "big") if restart_mcus is None else int(restart_mcus)

    def _header(self) -> bytes:
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.tf_jpeg_header(self._h, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value)

    def _first_capacity(self) -> int:   # most frames are a small part of this
        return len(self.header) + self.height * self.width * 3 // 4 + 4096

    def frame(self, image) -> JpegFrame:
        return JpegFrame(self.encode(image), (self.height, self.width, 3), self.quality, self.restart_mcus)
