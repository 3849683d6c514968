"""Planar YUV of a frame that is on the device (tf_yuv_*, transflow_amd/csrc/yuv.hip).

The reference's default output hands every frame to an ffmpeg child as `rgb24` and asks it for `-pix_fmt yuv420p`
(transflow/output/ffmpeg.py:32-54): 3 bytes a pixel come down and cross the pipe, and swscale converts and subsamples
them on one CPU thread.  `YuvEncoder` makes the planes the codec wants where the frame is -- yuv444p, yuv422p, yuv420p
or nv12, BT.601 or BT.709, tv or pc range -- and only they come down: half the bytes at 4:2:0.
`YuvFrame` is what then travels: the planes in one buffer and five fields.  `host_convert` is the same arithmetic in
numpy for a raw array that reaches one of the outputs (transflow_amd/output.py); it never opens the GPU.

These are the project's own pixels, stated exactly; they are not swscale's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .framecodec import FrameEncoder

# name -> (the library's number, log2 of the chroma block's width, of its height)
LAYOUTS = {"yuv444p": (0, 0, 0), "yuv422p": (1, 1, 0), "yuv420p": (2, 1, 1), "nv12": (3, 1, 1)}
MATRICES = {"bt601": 0, "bt709": 1}
RANGES = {"tv": 0, "pc": 1}


def _named(value, table: dict, what: str):
    if not isinstance(value, str) or value not in table:
        raise ValueError(f"{what} {value!r}: one of {sorted(table)}")
    return table[value]


def check_options(layout, matrix, range) -> None:
    """ValueError for a name that is none (no library call)."""
    _named(layout, LAYOUTS, "layout"), _named(matrix, MATRICES, "matrix"), _named(range, RANGES, "range")


def chroma_shape(height: int, width: int, layout: str) -> tuple:
    """(rows, columns) of a chroma plane: a sample per block, an odd edge's block counted whole."""
    _, bwl, bhl = _named(layout, LAYOUTS, "layout")
    return (-(-int(height) >> bhl), -(-int(width) >> bwl))


def frame_bytes(height: int, width: int, layout: str) -> int:
    """The bytes of a frame in a layout, asked of the library (the call loads it and touches no GPU)."""
    from . import _lib
    return int(_lib.load().tf_yuv_frame_bytes(int(width), int(height), _named(layout, LAYOUTS, "layout")[0]))


def coefficients(matrix: str = "bt601", range: str = "tv"):
    """(int32 (3, 3): the Y, U and V rows over (R, G, B), with 16 fractional bits; the Y offset, 16 or 0) as the library
    builds them (no GPU)."""
    from . import _lib
    rows, offset = (C.c_int32 * 9)(), C.c_int32()
    _lib.check(_lib.load().tf_yuv_coefficients(_named(matrix, MATRICES, "matrix"), _named(range, RANGES, "range"), rows,
                                               C.byref(offset)))
    return np.array(rows, np.int32).reshape(3, 3), int(offset.value)


class YuvFrame:
    """A frame as planes: one uint8 buffer in `layout`, the `shape` (H, W, 3) of the image it was made of, `matrix` and
    `range`.  `tobytes()` copies; `memoryview()` and `planes()` do not.  Pickles as its bytes and the four fields."""

    __slots__ = ("_data", "shape", "layout", "matrix", "range")

    def __init__(self, data, shape, layout: str = "yuv420p", matrix: str = "bt601", range: str = "tv"):
        check_options(layout, matrix, range)
        self.shape = tuple(int(v) for v in shape)
        self.layout, self.matrix, self.range = layout, matrix, range
        if not (isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.ndim == 1 and data.flags.c_contiguous):
            data = np.frombuffer(bytes(data), np.uint8)
        ch, cw = chroma_shape(self.shape[0], self.shape[1], layout)
        if len(self.shape) != 3 or self.shape[2] != 3 or data.nbytes != self.shape[0] * self.shape[1] + 2 * ch * cw:
            raise ValueError(f"{data.nbytes} bytes are no {layout} frame of shape {self.shape}")
        self._data = data

    def tobytes(self) -> bytes:
        return self._data.tobytes()

    def __bytes__(self) -> bytes:
        return self._data.tobytes()

    def memoryview(self) -> memoryview:
        """The buffer itself, for `write`: no copy."""
        return memoryview(self._data)

    def __len__(self) -> int:
        return self._data.nbytes

    def planes(self) -> tuple:
        """Views: (Y, U, V), or (Y, UV) with UV of shape (rows, columns, 2) for nv12."""
        h, w = self.shape[:2]
        ch, cw = chroma_shape(h, w, self.layout)
        y = self._data[:h * w].reshape(h, w)
        if self.layout == "nv12":
            return y, self._data[h * w:].reshape(ch, cw, 2)
        return y, self._data[h * w:h * w + ch * cw].reshape(ch, cw), self._data[h * w + ch * cw:].reshape(ch, cw)

    def __reduce__(self):
        return (type(self), (self._data.tobytes(), self.shape, self.layout, self.matrix, self.range))

    def __eq__(self, other):
        return (isinstance(other, YuvFrame)
                and (self.shape, self.layout, self.matrix, self.range) == (other.shape, other.layout, other.matrix, other.range)
                and np.array_equal(self._data, other._data))

    __hash__ = None

    def __repr__(self):
        return f"YuvFrame({len(self)} bytes, shape={self.shape}, {self.layout}, {self.matrix}, {self.range})"


def host_convert(rgb, layout: str = "yuv420p", matrix: str = "bt601", range: str = "tv") -> YuvFrame:
    """The frame of a uint8 (H, W, 3) RGB array, by the device's arithmetic in numpy with the
    library's own table: the same bytes by construction.  Never opens the GPU."""
    _, bwl, bhl = _named(layout, LAYOUTS, "layout")
    coef, y_offset = coefficients(matrix, range)
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != np.uint8 or 0 in rgb.shape:
        raise ValueError(f"a uint8 (H, W, 3) array is meant, not {rgb.dtype} {rgb.shape}")
    h, w = rgb.shape[:2]
    px = rgb.astype(np.int32)
    luma = np.clip((px @ coef[0] + ((y_offset << 16) + 32768)) >> 16, 0, 255)
    ch, cw = chroma_shape(h, w, layout)
    # an odd edge repeats its last column or row: every block has 2^k terms
    px = np.pad(px, ((0, (ch << bhl) - h), (0, (cw << bwl) - w), (0, 0)), mode="edge")
    sums = px.reshape(ch, 1 << bhl, cw, 1 << bwl, 3).sum(axis=(1, 3), dtype=np.int32)
    k = bwl + bhl
    chroma = np.clip((sums @ coef[1:].T + ((128 << (16 + k)) + (1 << (15 + k)))) >> (16 + k), 0, 255)     # (ch, cw, 2)
    out = np.empty(h * w + 2 * ch * cw, np.uint8)
    out[:h * w] = luma.reshape(-1)
    if layout == "nv12":
        out[h * w:] = chroma.reshape(-1)
    else:
        out[h * w:h * w + ch * cw] = chroma[:, :, 0].reshape(-1)
        out[h * w + ch * cw:] = chroma[:, :, 1].reshape(-1)
    return YuvFrame(out, (h, w, 3), layout, matrix, range)


class YuvEncoder(FrameEncoder):
    """tf_yuv: one size, one layout, matrix and range; its device and staging buffers are allocated once.  `frame()`
    brings the planes down into page-locked memory of a small pool and returns a YuvFrame over it."""

    ENCODE_DEV, ENCODE, DESTROY = "tf_yuv_convert_dev", "tf_yuv_convert", "tf_yuv_destroy"

    def __init__(self, height: int, width: int, layout: str = "yuv420p", matrix: str = "bt601", range: str = "tv"):
        check_options(layout, matrix, range)
        super().__init__(height, width)
        self.layout, self.matrix, self.range = layout, matrix, range
        self._check(self._lib.tf_yuv_create(C.byref(self._h), self.height, self.width, LAYOUTS[layout][0], MATRICES[matrix],
                                            RANGES[range]))
        self.nbytes = int(self._lib.tf_yuv_frame_bytes(self.width, self.height, LAYOUTS[layout][0]))
        self._pool = None

    def _first_capacity(self) -> int:   # every frame has this size
        return self.nbytes

    def convert_to_dev(self, image, out_dev: int) -> None:
        """The planes of a resident `image` (a DevicePixmap, a CompImage or a device address) into `nbytes` bytes of
        device memory at `out_dev`: queued on the calling thread's stream, not waited for."""
        dev = image if isinstance(image, int) else self._source(image)[0]
        if dev is None:
            raise ValueError("convert_to_dev takes a frame that is on the device")
        self._check(self._lib.tf_yuv_convert_to_dev(self._h, C.c_void_p(dev), C.c_void_p(int(out_dev))))

    def frame(self, image) -> YuvFrame:
        if self._pool is None:
            from .device import ArrayPool
            self._pool = ArrayPool((self.nbytes,), np.uint8, pinned=True)
        out = self._pool.take()
        self.encode_into(image, out)
        return YuvFrame(out, (self.height, self.width, 3), self.layout, self.matrix, self.range)
