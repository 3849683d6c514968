"""Baseline JPEG of a frame that is on the device (tf_jpeg_*, transflow_amd/csrc/jpeg.hip).

The reference's MJPEG output serves `cv2.imencode(".jpg", frame, [IMWRITE_JPEG_QUALITY, 50])` of the last frame
(transflow/output/mjpeg.py:58-60): its product is a compressed frame.  `JpegEncoder` makes that file where the frame
is -- 8-bit YCbCr 4:2:0, the standard tables, a restart interval: the bytes of Pillow's
`save(quality=q, subsampling=2, restart_marker_blocks=r)` -- and only the file comes down, a few percent of the
(H, W, 3) array.  `JpegFrame` is what then travels: the bytes and four numbers.

`optimize=True` is libjpeg's `optimize_coding`, Pillow's `save(..., optimize=True)`: the same pixels coded with the
frame's own Huffman tables (tf_jpeg_set_optimize), a file some 5 % smaller for about twice the entropy kernel.

`subsampling=0` / `1` (or "4:4:4" / "4:2:2") keeps the chroma at full or half-horizontal resolution: Pillow's
`save(..., subsampling=0 / 1)`, byte for byte.  The default, 2, is the 4:2:0 file written before there was a choice.
"""
from __future__ import annotations

import ctypes as C
import io

import numpy as np

from .framecodec import EncodedFrame, FrameEncoder


# Pillow's numbering of the chroma layouts, which tf_jpeg_create_sub takes too: value -> (name, MCU height, MCU width,
# blocks per MCU)
SUBSAMPLINGS = {0: ("4:4:4", 8, 8, 3), 1: ("4:2:2", 8, 16, 4), 2: ("4:2:0", 16, 16, 6)}


def subsampling_value(subsampling) -> int:
    """0 / 1 / 2 of 0 / 1 / 2 or "4:4:4" / "4:2:2" / "4:2:0"; a ValueError for anything else."""
    for value, (name, *_) in SUBSAMPLINGS.items():
        if (isinstance(subsampling, str) and subsampling == name) or \
                (isinstance(subsampling, (int, np.integer)) and not isinstance(subsampling, bool) and subsampling == value):
            return value
    raise ValueError(f"subsampling is 0 (\"4:4:4\"), 1 (\"4:2:2\") or 2 (\"4:2:0\"), not {subsampling!r}")


def default_restart_mcus(subsampling=2) -> int:
    """The device encoder's default interval for a layout, asked of the library (the call loads it and touches no GPU)."""
    from . import _lib
    return int(_lib.load().tf_jpeg_default_restart_mcus_for(subsampling_value(subsampling)))


def pillow_encode(image: np.ndarray, quality: int, restart_mcus: int, optimize: bool = False, subsampling=2) -> bytes:
    """The same file made on the host by libjpeg (Pillow >= 10.2 for `restart_marker_blocks`): what a process without
    a GPU does with a raw frame (transflow_amd/output.py).
    With `optimize` libjpeg writes nothing before the whole image is counted, and Pillow's encoder then needs its
    buffer to hold the file at once ("broken data stream" for a 1 x 65500 image otherwise): PIL.ImageFile.MAXBLOCK is
    raised for the call to the most the file can take -- the header and jpeg_common.h's bound on the scan, 1665 bits
    per block stuffed (2498 bytes for a 4:2:0 MCU), a marker per interval -- and put back behind it."""
    subsampling = subsampling_value(subsampling)
    _, mcu_h, mcu_w, mcu_blocks = SUBSAMPLINGS[subsampling]
    import PIL
    import PIL.Image
    import PIL.ImageFile
    if tuple(int(v) for v in PIL.__version__.split(".")[:2]) < (10, 2):
        # an older save() ignores the option without a word: the file would announce an interval and hold no marker
        raise RuntimeError(f"Pillow {PIL.__version__} has no restart_marker_blocks; 10.2 or later is needed")
    buf = io.BytesIO()
    picture = PIL.Image.fromarray(np.ascontiguousarray(image, dtype=np.uint8))
    if not optimize:
        picture.save(buf, format="JPEG", quality=int(quality), subsampling=subsampling,
                     restart_marker_blocks=int(restart_mcus))
        return buf.getvalue()
    n_mcus = -(-picture.height // mcu_h) * -(-picture.width // mcu_w)
    before = PIL.ImageFile.MAXBLOCK
    PIL.ImageFile.MAXBLOCK = max(before, 2048 + n_mcus * ((mcu_blocks * 1665 + 3) // 4 + 2))
    try:
        picture.save(buf, format="JPEG", quality=int(quality), subsampling=subsampling,
                     restart_marker_blocks=int(restart_mcus), optimize=True)
    finally:
        PIL.ImageFile.MAXBLOCK = before
    return buf.getvalue()


class JpegFrame(EncodedFrame):
    """A frame as a JPEG file: `data`, the `shape` (H, W, 3) of the image it decodes to, `quality`, `restart_mcus`,
    `optimize`: whether the file carries the frame's own Huffman tables, and `subsampling`: 0, 1, 2 for 4:4:4, 4:2:2,
    4:2:0 (a state pickled before there was a choice has none: 2)."""

    __slots__ = ("quality", "restart_mcus", "optimize", "subsampling")

    def __init__(self, data: bytes, shape, quality: int, restart_mcus: int, optimize: bool = False, subsampling=2):
        super().__init__(data, shape)
        self.quality = int(quality)
        self.restart_mcus = int(restart_mcus)
        self.optimize = bool(optimize)
        self.subsampling = subsampling_value(subsampling)


class JpegEncoder(FrameEncoder):
    """tf_jpeg: one size, one quality, one restart interval, one chroma layout; its device buffers are allocated once.
    `optimize`: the files carry the frame's own Huffman tables; `header` is then the last file's, and there is none
    before the first.  `subsampling`: 0 / "4:4:4", 1 / "4:2:2" or 2 / "4:2:0" (Pillow's numbering); `restart_mcus`
    counts MCUs of that layout (8 x 8, 16 x 8, 16 x 16 pixels), and None is the library's default for it."""

    ENCODE_DEV, ENCODE, COPY_LAST, DESTROY = "tf_jpeg_encode_dev", "tf_jpeg_encode", "tf_jpeg_copy_last", "tf_jpeg_destroy"

    def __init__(self, height: int, width: int, quality: int = 50, restart_mcus: int | None = None, optimize: bool = False,
                 subsampling=2):
        super().__init__(height, width)
        self.quality = int(quality)
        self.optimize = bool(optimize)
        self.subsampling = subsampling_value(subsampling)
        self._check(self._lib.tf_jpeg_create_sub(C.byref(self._h), self.height, self.width, self.quality,
                                                 0 if restart_mcus is None else int(restart_mcus), self.subsampling))
        self.restart_mcus = (int(self._lib.tf_jpeg_default_restart_mcus_for(self.subsampling)) if restart_mcus is None
                             else int(restart_mcus))
        self._fixed_header = self._header()      # the Annex K tables': made once
        if self.optimize:
            try:
                self._check(self._lib.tf_jpeg_set_optimize(self._h, 1))
            except Exception:
                self.close()
                raise

    def _header(self) -> bytes:
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.tf_jpeg_header(self._h, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value)

    @property
    def header(self) -> bytes:
        """The bytes before the scan: the same for every file, or with `optimize` the last file's (an error before it)."""
        return self._header() if self.optimize else self._fixed_header

    def _first_capacity(self) -> int:   # most frames are a small part of this (no own header is longer than Annex K's + 400)
        # a quarter of the raw frame for 4:2:0's 1.5 samples a pixel; the same per sample for 4:2:2's 2 and 4:4:4's 3
        _, mcu_h, mcu_w, mcu_blocks = SUBSAMPLINGS[self.subsampling]
        samples_x2 = mcu_blocks * 128 // (mcu_h * mcu_w)              # 3, 4, 6
        return len(self._fixed_header) + 400 + self.height * self.width * samples_x2 // 4 + 4096

    def last_tables(self, counts: bool = False):
        """What the last `optimize` encode built, in the DHT segments' order (DC luma, AC luma, DC chroma, AC chroma):
        a list of four (bits, vals), and with `counts` the uint32 (4, 257) histograms behind them."""
        bits, vals = np.zeros((4, 16), np.uint8), np.zeros((4, 256), np.uint8)
        hist = np.zeros((4, 257), np.uint32) if counts else None
        self._check(self._lib.tf_jpeg_last_tables(self._h, C.c_void_p(bits.ctypes.data), C.c_void_p(vals.ctypes.data),
                                                  C.c_void_p(hist.ctypes.data) if counts else None))
        tables = [(bits[t].tolist(), vals[t, :int(bits[t].sum())].tolist()) for t in range(4)]
        return (tables, hist) if counts else tables

    def frame(self, image) -> JpegFrame:
        return JpegFrame(self.encode(image), (self.height, self.width, 3), self.quality, self.restart_mcus, self.optimize,
                         self.subsampling)
