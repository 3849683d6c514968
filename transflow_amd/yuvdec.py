"""Planar YUV frames turned back into pixels where the frame is wanted (tf_yuvdec_*, transflow_amd/csrc/yuvdec.hip;
DESIGN.md section 22).

The way back of transflow_amd/yuv.py: the planes of a Y4M file or of a headerless `.yuv` file -- yuv444p, yuv422p,
yuv420p or nv12, BT.601 or BT.709, tv or pc range -- go up the link as they are (half the RGB frame's bytes at 4:2:0)
and become a `DevicePixmap` by a stated integer rule; the host converts nothing.  `probe_y4m` reads the header line or
rejects the file with a reason (`YuvRejected`); `Y4mFrameProvider` and `RawYuvFrameProvider` are frame providers for
`HipFlowSource` (the protocol of `ArrayFrameProvider`, transflow_amd/flow.py) over a memory-mapped file;
`host_convert_back` is the same arithmetic in numpy, for `device_decode=False` and for where there is no GPU.

The luma plane is never taken for the flow's grey: the frame is converted to BGR and goes the way every frame goes.
These are the project's own pixels, stated exactly; they are not swscale's.  Chroma is expanded by replication
(`chroma="replicate"`, the geometric inverse of section 21's block mean) or by the centre-sited triangle filter
(`chroma="linear"`); Y4M's siting tags (C420jpeg, C420mpeg2, C420paldv, plain C420) all take that same filter: the tag
is kept as `.siting` and otherwise ignored.
"""
from __future__ import annotations

import ctypes as C
import os
from fractions import Fraction

import numpy as np

from .framecodec import FrameDecoder
from .pixmap import DevicePixmap, _dev_alloc, _recorded_event
from .yuv import LAYOUTS, MATRICES, RANGES, _named, chroma_shape

CHROMAS = {"replicate": 0, "linear": 1}
# why a file is no Y4M file for this reader (tests/yuvdec_ref.py has the same names)
REJECT_REASONS = ("not_y4m", "bad_header", "interlaced", "chroma", "bad_frame_header")
# the C tags that are read -> the layout; mono, 4:1:1, alpha and the deeper formats are rejected ("chroma")
Y4M_TAGS = {"C420jpeg": "yuv420p", "C420mpeg2": "yuv420p", "C420paldv": "yuv420p", "C420": "yuv420p", "C422": "yuv422p",
            "C444": "yuv444p"}
Y4M_MAGIC = b"YUV4MPEG2"
MAX_HEADER, MAX_FRAME_HEADER = 256, 80
Y4M_EXTS = (".y4m",)


class YuvRejected(ValueError):
    """The file is no Y4M file this reader takes: `reason` is one of REJECT_REASONS, `frame` the frame where there is
    one."""

    def __init__(self, reason: str, frame=None):
        of = "" if frame is None else f" (frame {frame})"
        ValueError.__init__(self, f"the Y4M file is rejected: {reason}{of}")
        self.reason, self.frame = reason, frame


class Y4mInfo:
    """What the header line says.  `siting`: the C tag as written, None without one; `header_bytes`: the line's length,
    its newline included."""

    __slots__ = ("width", "height", "framerate", "layout", "range", "siting", "header_bytes")

    def __init__(self, width, height, framerate, layout, range, siting, header_bytes):
        self.width, self.height, self.framerate, self.layout = int(width), int(height), framerate, layout
        self.range, self.siting, self.header_bytes = range, siting, int(header_bytes)

    def __repr__(self):
        return "Y4mInfo(" + ", ".join(f"{n}={getattr(self, n)}" for n in self.__slots__) + ")"


def _number(text: bytes) -> int:
    if not text.isdigit():
        raise YuvRejected("bad_header")
    return int(text)


def probe_y4m(data) -> Y4mInfo:
    """The header line of a Y4M file (its first 256 bytes are enough); `YuvRejected` for anything else."""
    head = bytes(data[:MAX_HEADER + 1])
    if head[:len(Y4M_MAGIC) + 1] not in (Y4M_MAGIC + b" ", Y4M_MAGIC + b"\n"):
        raise YuvRejected("not_y4m")
    end = head.find(b"\n", 0, MAX_HEADER)
    if end < 0:
        raise YuvRejected("bad_header")
    width = height = rate = None
    tag, full, interlace = None, False, b"p"
    for field in head[len(Y4M_MAGIC):end].split(b" "):
        if not field:
            continue
        key, value = field[:1], field[1:]
        if key == b"W":
            width = _number(value)
        elif key == b"H":
            height = _number(value)
        elif key == b"F":
            num, colon, den = value.partition(b":")
            if not colon:
                raise YuvRejected("bad_header")
            num, den = _number(num), _number(den)
            if num == 0 or den == 0:
                raise YuvRejected("bad_header")
            rate = Fraction(num, den)
        elif key == b"I":
            interlace = value
        elif key == b"C":
            tag = field.decode("ascii", "replace")
        elif field == b"XCOLORRANGE=FULL":
            full = True
    if width is None or height is None or rate is None or width < 1 or height < 1:
        raise YuvRejected("bad_header")
    if interlace not in (b"p", b"?"):
        raise YuvRejected("interlaced")
    if tag is not None and tag not in Y4M_TAGS:
        raise YuvRejected("chroma")
    return Y4mInfo(width, height, rate, Y4M_TAGS[tag] if tag is not None else "yuv420p", "pc" if full else "tv", tag, end + 1)


def index_y4m(data, info: Y4mInfo) -> tuple:
    """([the offset of every whole frame's planes], the bytes behind the last whole frame).  The frame headers are
    walked, since a FRAME line may carry parameters; a trailing partial frame is not a frame."""
    nbytes = frame_bytes(info.width, info.height, info.layout)
    at, total, offsets = info.header_bytes, len(data), []
    while total - at >= 6 + nbytes:
        line = bytes(data[at:at + MAX_FRAME_HEADER])
        end = line.find(b"\n")
        if line[:5] != b"FRAME" or end < 0 or line[5:6] not in (b" ", b"\n"):
            raise YuvRejected("bad_frame_header", len(offsets))
        if total - (at + end + 1) < nbytes:
            break
        offsets.append(at + end + 1)
        at += end + 1 + nbytes
    return offsets, total - at


def frame_bytes(width: int, height: int, layout: str) -> int:
    """The bytes of a frame's planes (no library call)."""
    ch, cw = chroma_shape(height, width, layout)
    return int(height) * int(width) + 2 * ch * cw


def coefficients(matrix: str = "bt601", range: str = "tv") -> np.ndarray:
    """int32 (5,): cy, rv, gu, gv, bu with 16 fractional bits, as the library builds them (no GPU)."""
    from . import _lib
    out = (C.c_int32 * 5)()
    _lib.check(_lib.load().tf_yuvdec_coefficients(_named(matrix, MATRICES, "matrix"), _named(range, RANGES, "range"), out))
    return np.array(out, np.int32)


def _as_bytes(planes) -> np.ndarray:
    if isinstance(planes, np.ndarray) and planes.dtype == np.uint8 and planes.flags.c_contiguous:
        return planes.reshape(-1)
    if hasattr(planes, "memoryview"):                   # a YuvFrame
        planes = planes.memoryview()
    return np.frombuffer(planes, np.uint8)


def _check_frame(raw: np.ndarray, width: int, height: int, layout: str) -> None:
    if width < 1 or height < 1 or raw.nbytes != frame_bytes(width, height, layout):
        raise ValueError(f"{raw.nbytes} bytes are no {layout} frame of {width}x{height}")


def _linear_columns(s: np.ndarray, width: int, shift: int, even_add: int, odd_add: int) -> np.ndarray:
    """The triangle filter along a row: every sample twice, three parts itself and one part its neighbour on the
    pixel's side, the edge's neighbour the edge itself."""
    padded = np.pad(s, ((0, 0), (1, 1)), mode="edge")
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int32)
    out[:, 0::2] = (3 * s + padded[:, :-2] + even_add) >> shift
    out[:, 1::2] = (3 * s + padded[:, 2:] + odd_add) >> shift
    return out[:, :width]


def _expand(p: np.ndarray, width: int, height: int, bwl: int, bhl: int, linear: bool) -> np.ndarray:
    """A chroma plane at the picture's size, int32."""
    p = p.astype(np.int32)
    if not bwl:
        return p
    if not linear:
        return p.repeat(1 << bhl, axis=0).repeat(2, axis=1)[:height, :width]
    if not bhl:
        return _linear_columns(p, width, 2, 1, 2)
    padded = np.pad(p, ((1, 1), (0, 0)), mode="edge")
    sums = np.empty((2 * p.shape[0], p.shape[1]), np.int32)
    sums[0::2] = 3 * p + padded[:-2]                    # an even row leans on the chroma row above, an odd one below
    sums[1::2] = 3 * p + padded[2:]
    return _linear_columns(sums[:height], width, 4, 8, 7)


def host_convert_back(planes, width: int, height: int, layout: str = "yuv420p", matrix: str = "bt601", range: str = "tv",
                      chroma: str = "replicate", order: str = "bgr") -> np.ndarray:
    """The uint8 (H, W, 3) pixels of a frame's planes, by the device's arithmetic in numpy with
    the library's own table: the same bytes by construction.  Never opens the GPU."""
    _, bwl, bhl = _named(layout, LAYOUTS, "layout")
    linear = bool(_named(chroma, CHROMAS, "chroma"))
    flip = bool(_named(order, FrameDecoder.ORDERS, "order"))
    cy, rv, gu, gv, bu = (int(v) for v in coefficients(matrix, range))
    width, height = int(width), int(height)
    raw = _as_bytes(planes)
    _check_frame(raw, width, height, layout)
    ch, cw = chroma_shape(height, width, layout)
    n = width * height
    if layout == "nv12":
        pairs = raw[n:].reshape(ch, cw, 2)
        u_plane, v_plane = pairs[:, :, 0], pairs[:, :, 1]
    else:
        u_plane, v_plane = raw[n:n + ch * cw].reshape(ch, cw), raw[n + ch * cw:].reshape(ch, cw)
    base = cy * (raw[:n].reshape(height, width).astype(np.int32) - (16 if range == "tv" else 0)) + 32768
    u = _expand(u_plane, width, height, bwl, bhl, linear) - 128
    v = _expand(v_plane, width, height, bwl, bhl, linear) - 128
    red, green, blue = (base + rv * v) >> 16, (base + gu * u + gv * v) >> 16, (base + bu * u) >> 16
    out = np.stack([blue, green, red] if flip else [red, green, blue], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


class YuvDecoder(FrameDecoder):
    """tf_yuvdec: frames of up to max_width x max_height in any layout; its staging and device buffers are allocated
    once.  `decode` takes a frame's planes from the host, `decode_dev` planes that are on the device already (what
    `YuvEncoder.convert_to_dev` made); both queue the kernel on the calling thread's stream and return a `DevicePixmap`
    whose event stands behind it."""

    CREATE, DESTROY = "tf_yuvdec_create", "tf_yuvdec_destroy"

    def _create(self) -> None:
        self._check(getattr(self._lib, self.CREATE)(C.byref(self._h), self.max_width, self.max_height))

    def _numbers(self, width, height, layout, matrix, range, chroma, order) -> tuple:
        return (int(width), int(height), _named(layout, LAYOUTS, "layout")[0], _named(matrix, MATRICES, "matrix"),
                _named(range, RANGES, "range"), _named(chroma, CHROMAS, "chroma"), _named(order, self.ORDERS, "order"))

    def convert_into(self, planes, width, height, layout, out_dev: int, matrix="bt601", range="tv", chroma="replicate",
                     order="bgr") -> None:
        """The pixels of a host frame into 3 * width * height bytes of device memory at `out_dev`: queued, not waited
        for."""
        w, h, lay, mat, rng, chr_, ordr = self._numbers(width, height, layout, matrix, range, chroma, order)
        raw = _as_bytes(planes)
        self._check(self._lib.tf_yuvdec_convert(self._h, C.c_void_p(raw.ctypes.data), raw.nbytes, w, h, lay, mat, rng, chr_,
                                                C.c_void_p(int(out_dev)), ordr))

    def convert_dev_into(self, planes_dev: int, nbytes: int, width, height, layout, out_dev: int, matrix="bt601", range="tv",
                         chroma="replicate", order="bgr") -> None:
        """The same for `nbytes` bytes of planes at the device address `planes_dev`."""
        w, h, lay, mat, rng, chr_, ordr = self._numbers(width, height, layout, matrix, range, chroma, order)
        self._check(self._lib.tf_yuvdec_convert_dev(self._h, C.c_void_p(int(planes_dev)), int(nbytes), w, h, lay, mat, rng, chr_,
                                                    C.c_void_p(int(out_dev)), ordr))

    def _pixmap(self, width, height, convert) -> DevicePixmap:
        if width < 1 or height < 1 or width > self.max_width or height > self.max_height:
            raise ValueError(f"a frame of {width}x{height}; the decoder is for {self.max_width}x{self.max_height}")
        buf = _dev_alloc(height * width * 3)
        try:
            convert(buf.ptr)
        except Exception:
            buf.close()
            raise
        return DevicePixmap((height, width, 3), buf, _recorded_event())

    def decode(self, planes, width: int, height: int, layout: str, matrix: str = "bt601", range: str = "tv",
               chroma: str = "replicate", order: str = "bgr") -> DevicePixmap:
        """The frame's pixels, uint8 (H, W, 3) in `order`, in device memory.  planes: the tightly packed frame -- bytes,
        a memoryview, a uint8 array or a YuvFrame.  ValueError for a name that is none, for a frame larger than the
        decoder was made for and for planes of another size than the frame's."""
        width, height = int(width), int(height)
        return self._pixmap(width, height, lambda out: self.convert_into(planes, width, height, layout, out, matrix, range,
                                                                         chroma, order))

    def decode_dev(self, planes_dev: int, nbytes: int, width: int, height: int, layout: str, matrix: str = "bt601",
                   range: str = "tv", chroma: str = "replicate", order: str = "bgr") -> DevicePixmap:
        width, height = int(width), int(height)
        return self._pixmap(width, height, lambda out: self.convert_dev_into(planes_dev, nbytes, width, height, layout, out,
                                                                             matrix, range, chroma, order))


class PlanarFrameProvider:
    """A frame provider (transflow_amd/flow.py: `width`, `height`, `framerate`, `frame_count`, `pos`, `seek_start`,
    `read`, `release`) over a file of planar YUV frames, memory-mapped, or over the file's bytes.  `read()` returns a BGR
    `DevicePixmap` made on the device; with `device_decode=False` it returns the uint8 array `host_convert_back` makes,
    and no GPU is opened.  A subclass finds `_offsets`, the place of every frame's planes, and sets `layout`, `range`,
    `_frame_size`.  Pickles without its mapping and its decoder's handle."""

    _path = _data = _decoder = None
    siting = None
    trailing_bytes = 0

    def _setup(self, source, size, matrix, chroma, device_decode, device) -> None:
        _named(matrix, MATRICES, "matrix"), _named(chroma, CHROMAS, "chroma")
        self.matrix, self.chroma = matrix, chroma
        self.device_decode, self.device = bool(device_decode), device
        if isinstance(source, (str, os.PathLike)):
            self._path = os.fspath(source)
        else:
            self._data = bytes(source)
        self._size = None if size is None else (int(size[0]), int(size[1]))
        self.pos = 0

    def _finish(self, frame_size, empty: str) -> None:
        self.frame_count = len(self._offsets)
        if self.frame_count == 0:
            raise ValueError(empty)
        self._frame_size = frame_size
        self.width, self.height = frame_size if self._size is None else self._size
        self._nbytes = frame_bytes(frame_size[0], frame_size[1], self.layout)

    def _stream(self):
        if self._data is None:
            import mmap
            with open(self._path, "rb") as f:
                self._data = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if os.fstat(f.fileno()).st_size else b""
        return self._data

    def _get(self, i: int) -> np.ndarray:
        return np.frombuffer(self._stream(), np.uint8, self._nbytes, self._offsets[i])

    def __getstate__(self):                              # a mapping and a handle belong to their process
        state = dict(self.__dict__)
        state["_decoder"] = None
        if self._path is not None:
            state.pop("_data", None)
        return state

    def decode_frame(self, index: int, order: str = "bgr"):
        w, h = self._frame_size
        planes = self._get(index)
        if not self.device_decode:
            return host_convert_back(planes, w, h, self.layout, self.matrix, self.range, self.chroma, order)
        if self._decoder is None:
            self._decoder = YuvDecoder(w, h, self.device)
        return self._decoder.decode(planes, w, h, self.layout, self.matrix, self.range, self.chroma, order)

    def seek_start(self):
        self.pos = 0

    def read(self, order: str = "bgr"):
        if self.pos >= self.frame_count:
            return None
        frame = self.decode_frame(self.pos, order)
        self.pos += 1
        return frame

    def release(self):
        if self._decoder is not None:
            self._decoder.close()
            self._decoder = None
        if self._path is not None and self._data is not None:
            data, self._data = self._data, None
            try:
                if hasattr(data, "close"):
                    data.close()
            except BufferError:                          # an array over the mapping is still alive: the collector's
                pass


class Y4mFrameProvider(PlanarFrameProvider):
    """A `PlanarFrameProvider` of a YUV4MPEG2 file (a path, or the file's bytes): what `ffmpeg -i any.mp4 out.y4m` and
    `HipY4mOutput` write.  The frame headers are walked once; a trailing partial frame is not a frame (`trailing_bytes`
    counts what lies behind the last whole one).  range=None takes the header's range (XCOLORRANGE=FULL is pc, anything
    else tv); the matrix is the caller's to know, Y4M has no tag for it.  `siting` is the header's C tag, kept and
    otherwise ignored: every 4:2:0 siting takes the same centre-sited filter.  `YuvRejected` for a file this reader
    does not take."""

    def __init__(self, source, size=None, matrix: str = "bt601", range: str | None = None, chroma: str = "replicate",
                 device_decode: bool = True, device: int | None = None):
        self._setup(source, size, matrix, chroma, device_decode, device)
        info = probe_y4m(self._stream())
        self.layout, self.siting = info.layout, info.siting
        self.range = info.range if range is None else range
        _named(self.range, RANGES, "range")
        self.framerate = float(info.framerate)
        self._offsets, self.trailing_bytes = index_y4m(self._stream(), info)
        self._finish((info.width, info.height), "the Y4M file holds no frame")


class RawYuvFrameProvider(PlanarFrameProvider):
    """A `PlanarFrameProvider` of a headerless file of frames back to back (`.yuv`; nv12 included): the size and the
    layout are the caller's to know.  frame_count = size // frame_bytes; `trailing_bytes` counts the rest."""

    def __init__(self, source, width: int, height: int, layout: str = "yuv420p", framerate: float = 25.0, size=None,
                 matrix: str = "bt601", range: str = "tv", chroma: str = "replicate", device_decode: bool = True,
                 device: int | None = None):
        self._setup(source, size, matrix, chroma, device_decode, device)
        _named(layout, LAYOUTS, "layout"), _named(range, RANGES, "range")
        if int(width) < 1 or int(height) < 1:
            raise ValueError(f"a frame of {width}x{height}")
        self.layout, self.range, self.framerate = layout, range, float(framerate)
        nbytes, total = frame_bytes(width, height, layout), len(self._stream())
        self._offsets = (np.arange(total // nbytes, dtype=np.int64) * nbytes).tolist()
        self.trailing_bytes = total - len(self._offsets) * nbytes
        self._finish((int(width), int(height)), "the file holds no frame")


def is_y4m(path) -> bool:
    """An existing file whose name ends in .y4m."""
    return isinstance(path, str) and os.path.splitext(path)[1].lower() in Y4M_EXTS and os.path.isfile(path)
