"""What the device's frame codecs (transflow_amd/jpeg.py, transflow_amd/png.py) have in common on the Python side: the
frame that travels as a compressed file, and the wrapper of a handle that encodes frames of one size."""
from __future__ import annotations

import ctypes as C
import io

import numpy as np


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
