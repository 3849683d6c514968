"""What the device's frame codecs have in common on the Python side.  For the encoders (transflow_amd/jpeg.py,
transflow_amd/png.py): the frame that travels as a compressed file, and the wrapper of a handle that encodes frames of
one size.  For the decoders (transflow_amd/jpegdec.py, transflow_amd/pngdec.py): the host's way to the same pixels, the
wrapper of a handle that decodes frames up to a size, and the frame provider over a sequence of compressed files."""
from __future__ import annotations

import ctypes as C
import io
import os

import numpy as np

from .pixmap import DevicePixmap, _dev_alloc, _recorded_event


class EncodedFrame:
    """A frame as a compressed file: `data`, the `shape` (H, W, 3) of the image it decodes to, and the subclass's own
    fields -- its `__slots__`, in the order of its constructor's arguments."""

    __slots__ = ("data", "shape")

    def __init__(self, data: bytes, shape):
        self.data = bytes(data)
        self.shape = tuple(int(v) for v in shape)

    def _fields(self) -> tuple:
        return (self.data, self.shape, *(getattr(self, name) for name in type(self).__slots__))

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
        return (type(self), self._fields())

    def __eq__(self, other):
        return isinstance(other, type(self)) and self._fields() == other._fields()

    __hash__ = None

    def __repr__(self):
        own = "".join(f", {name}={getattr(self, name)}" for name in type(self).__slots__)
        return f"{type(self).__name__}({len(self.data)} bytes, shape={self.shape}{own})"


class FrameEncoder:
    """A handle of the library that encodes frames of one size; its device buffers are allocated once.  A subclass names
    its C entry points (ENCODE_DEV, ENCODE, COPY_LAST, DESTROY), creates the handle `_h` in its constructor, and has
    `_first_capacity()` -- the output buffer encode() starts with -- and `frame(image)`."""

    ENCODE_DEV = ENCODE = COPY_LAST = DESTROY = None

    def __init__(self, height: int, width: int):
        from . import _lib
        self._lib = _lib.load()
        self._check = _lib.check
        self.height, self.width = int(height), int(width)
        self._h = C.c_void_p()
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
            rc = getattr(self._lib, self.ENCODE_DEV)(self._h, C.c_void_p(dev), dst, out.nbytes, C.byref(n))
        else:
            rc = getattr(self._lib, self.ENCODE)(self._h, C.c_void_p(host.ctypes.data), dst, out.nbytes, C.byref(n))
        self.last_needed = n.value
        self._check(rc)
        return n.value

    def encode(self, image) -> bytes:
        """The file of `image`: a uint8 (H, W, 3) ndarray, a DevicePixmap or a CompImage."""
        if self._out is None:       # most frames are a part of this; one that is not makes the buffer grow
            self._out = np.empty(self._first_capacity(), np.uint8)
        try:
            n = self.encode_into(image, self._out)
        except ValueError:
            if self.last_needed <= self._out.nbytes:
                raise
            self._out = np.empty(self.last_needed, np.uint8)      # the slots are still in the handle: pack and copy
            size = C.c_size_t()
            self._check(getattr(self._lib, self.COPY_LAST)(self._h, C.c_void_p(self._out.ctypes.data), self._out.nbytes,
                                                           C.byref(size)))
            n = size.value
        return self._out[:n].tobytes()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._lib, self.DESTROY)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bytes_of(data) -> bytes:
    return data.data if hasattr(data, "data") and isinstance(getattr(data, "data"), (bytes, bytearray)) else bytes(data)


def pillow_decode(data, order: str = "rgb") -> np.ndarray:
    """The host's way: Pillow (libjpeg, zlib)."""
    import PIL.Image
    rgb = np.array(PIL.Image.open(io.BytesIO(bytes_of(data))).convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1]) if order == "bgr" else rgb


class FrameDecoder:
    """A handle of the library that decodes frames of up to max_width x max_height; its staging and device buffers are
    allocated once (and again for a file larger than any before it).  A subclass names its C entry points (CREATE,
    DECODE_DEV, DESTROY) and has `_verdict(rc, reject)`, which raises what a failed call means, and `decode`."""

    CREATE = DECODE_DEV = DESTROY = None
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
        self._create()
        self.fallbacks = 0

    def _create(self) -> None:
        self._check(getattr(self._lib, self.CREATE)(C.byref(self._h), self.max_width, self.max_height, self._file_room))

    def _room_for(self, nbytes: int) -> None:
        if nbytes > self._file_room:
            self.close()
            self._file_room = int(nbytes) * 2
            self._create()

    def _decode(self, raw: bytes, order: str, info) -> DevicePixmap:
        """What every `decode` ends with: `raw`, whose header says `info`, into a new device buffer."""
        if info.width > self.max_width or info.height > self.max_height:
            raise ValueError(f"a frame of {info.width}x{info.height}; the decoder is for {self.max_width}x{self.max_height}")
        self._room_for(len(raw))
        buf = _dev_alloc(info.height * info.width * 3)
        reject = C.c_uint32()
        rc = getattr(self._lib, self.DECODE_DEV)(self._h, raw, len(raw), C.c_void_p(buf.ptr), self.ORDERS[order], C.byref(reject))
        try:
            self._verdict(rc, reject.value)
        except Exception:
            buf.close()
            raise
        return DevicePixmap((info.height, info.width, 3), buf, _recorded_event())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._lib, self.DESTROY)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CompressedFrameProvider:
    """A frame provider (transflow_amd/flow.py: `width`, `height`, `framerate`, `frame_count`, `seek_start`, `read`,
    `release`) whose frames are compressed files decoded on the device: a `%0Nd` pattern (numbered from the first of 0
    or 1 that exists) or a sequence of `bytes` / `EncodedFrame`.  `read()` returns a BGR `DevicePixmap`: `HipFlowSource`
    hands it to a Farnebäck handle by its device address, and `np.asarray` of it is the host frame for everything else.
    `fallbacks` counts the frames Pillow decoded.  A subclass names its DECODER and what an EMPTY source is told, and
    has `_first_size(raw)` -- (width, height) of the first frame -- and `decode_frame(index, order)`."""

    DECODER = EMPTY = None

    def __init__(self, source, framerate: float, size, device_decode: bool, device: int | None):
        self.framerate = float(framerate)
        self.device_decode, self.device = bool(device_decode), device
        if isinstance(source, (str, os.PathLike)):
            self.frame_count = self._open_path(os.fspath(source))
        else:
            self._frames = list(source)
            self.frame_count = len(self._frames)
        if self.frame_count == 0:
            raise ValueError(self.EMPTY)
        self._frame_size = self._first_size(self._get(0))
        self.width, self.height = self._frame_size if size is None else (int(size[0]), int(size[1]))
        self._decoder = None
        self._host_fallbacks = 0
        self.pos = 0

    def _open_path(self, path: str) -> int:
        first = next((k for k in (0, 1) if os.path.isfile(path % k)), None)
        if first is None:
            raise FileNotFoundError(f"no frame {path % 0} or {path % 1}")
        self._files = []
        while os.path.isfile(path % (first + len(self._files))):
            self._files.append(path % (first + len(self._files)))
        return len(self._files)

    def _get(self, i: int) -> bytes:
        if hasattr(self, "_files"):
            with open(self._files[i], "rb") as f:
                return f.read()
        return bytes_of(self._frames[i])

    def __getstate__(self):                          # a decoder's handle belongs to its process
        state = dict(self.__dict__)
        if state.get("_decoder") is not None:
            state["_host_fallbacks"] = self.fallbacks
            state["_decoder"] = None
        return state

    @property
    def fallbacks(self) -> int:
        return self._host_fallbacks + (self._decoder.fallbacks if self._decoder is not None else 0)

    def _host_frame(self, raw: bytes, order: str) -> DevicePixmap:
        self._host_fallbacks += 1
        return DevicePixmap.from_host(pillow_decode(raw, order))

    def _decoder_for(self, info) -> FrameDecoder:
        if self._decoder is None or info.width > self._decoder.max_width or info.height > self._decoder.max_height:
            room = (max(info.width, self._frame_size[0]), max(info.height, self._frame_size[1]))
            if self._decoder is not None:            # a larger frame: the old handle's buffers go now, not with the collector
                room = (max(room[0], self._decoder.max_width), max(room[1], self._decoder.max_height))
                self._drop_decoder()
            self._decoder = self._new_decoder(room[0], room[1])
        return self._decoder

    def _new_decoder(self, max_width: int, max_height: int) -> FrameDecoder:
        return self.DECODER(max_width, max_height, self.device)

    def seek_start(self):
        self.pos = 0

    def read(self, order: str = "bgr"):
        if self.pos >= self.frame_count:
            return None
        frame = self.decode_frame(self.pos, order)
        self.pos += 1
        return frame

    def _drop_decoder(self):                        # its count stays
        if self._decoder is not None:
            self._host_fallbacks += self._decoder.fallbacks
            self._decoder.close()
            self._decoder = None

    def release(self):
        self._drop_decoder()
