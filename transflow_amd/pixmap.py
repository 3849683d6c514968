"""Still pixmap sources whose image lives in HBM.

The pixmap is the image whose pixels the compositor's layers move (transflow/pixmap/source.py, still.py).  The
reference's still sources make one array in `__enter__` and hand out a fresh copy of it per frame (still.py:32-34); the
compositor's layers then upload the same bytes again for every frame.  The classes here mirror the reference's -- same
names with a `Hip` in front, same constructor signatures and attributes, same iterator and context-manager protocol,
same pixels for the same seed -- and keep the one image on the device:

* the random draws stay on the host and use numpy's and `random`'s global streams call for call (a noise array goes up
  once; the streams are left as the reference leaves them);
* a given or drawn colour is filled on the device (tf_pixmap_fill_dev); the gradient's random expression tree is drawn
  on the host, flattened to postfix order and evaluated per pixel on the device (tf_pixmap_gradient_dev) instead of by
  still.py:157-162's Python loop;
* the alteration overlay (source.py:40-69) is constant for a still: it is applied once, on the host, with numpy.put;
* `__next__` yields the same `DevicePixmap` every time.  `RemapLayer.gather / stage_pixmap / introduce` take it by
  device address; anything numpy reads it through a host copy made at most once, as READ-ONLY views (the reference's
  copy per frame was writable: INTEGRATION.md);
* a pickle of it, a `multiprocessing` queue included, is the pickle of the plain host array.

`HipPixmapInterface` is what a layer's `sources` hold when everything runs in one process: the reference's
PixmapSourceInterface (compositor/pixmap_source_interface.py:12-37) without the queue.
"""
from __future__ import annotations

import ctypes as C
import os
import random
import re

import numpy as np
from numpy.lib.mixins import NDArrayOperatorsMixin

MJPEG_EXTS = (".mjpeg", ".mjpg")       # the extensions a raw MJPEG stream file is known by, here and in jpegdec.py
NODE_I, NODE_J, NODE_RGB, NODE_MIX, NODE_TRIPLE, NODE_Z, NODE_B = range(7)     # still.py:86-92
MAX_NODES = 40                                                                 # TF_PX_MAX_NODES


class TfPxNode(C.Structure):
    _fields_ = [("type", C.c_int), ("a", C.c_double), ("b", C.c_double), ("c", C.c_double)]


# ---- the library calls of this module, in one place ---------------------------------------------------------------
def _dev_alloc(nbytes: int):
    from .device import DevBuffer
    return DevBuffer(max(4, int(nbytes)))


def _dev_upload(buf, array: np.ndarray) -> None:
    buf.upload(array)


def _dev_download(buf, shape) -> np.ndarray:
    return buf.download(shape, np.uint8)


def _dev_fill(buf, n_pixels: int, rgb) -> None:
    from . import _lib
    _lib.check(_lib.load().tf_pixmap_fill_dev(C.c_void_p(buf.ptr), int(n_pixels), (C.c_uint8 * 3)(*[int(v) for v in rgb])))


def _dev_gradient(buf, width: int, height: int, nodes) -> None:
    from . import _lib
    arr = (TfPxNode * max(1, len(nodes)))(*[TfPxNode(int(t), float(a), float(b), float(c)) for t, a, b, c in nodes])
    _lib.check(_lib.load().tf_pixmap_gradient_dev(C.c_void_p(buf.ptr), int(width), int(height), len(nodes), arr))


def _recorded_event():
    from .deviceflow import _Event
    ev = _Event()
    ev.record()
    return ev


class DevicePixmap(NDArrayOperatorsMixin):
    """uint8 (H, W, 3 or 4) pixmap in HBM; see the module text."""

    dtype = np.dtype(np.uint8)
    ndim = 3
    __array_priority__ = 0.0

    def __init__(self, shape, buf, ready=None, host: np.ndarray | None = None):
        self.shape = tuple(int(v) for v in shape)
        self._buf = buf            # the allocation: lives as long as this object
        self._ready = ready        # recorded behind the launch or upload that made the image
        self._host = host          # the array that went up, where there was one

    @classmethod
    def from_host(cls, array: np.ndarray) -> "DevicePixmap":
        a = np.ascontiguousarray(array, dtype=np.uint8)
        if a.ndim != 3:
            raise ValueError(f"a pixmap is (H, W, channels), not {a.shape}")
        buf = _dev_alloc(a.nbytes)
        _dev_upload(buf, a)
        return cls(a.shape, buf, _recorded_event(), host=a)

    # ---- what the layers use ------------------------------------------------------------------------------------
    @property
    def dev_ptr(self) -> int:
        return self._buf.ptr

    @property
    def channels(self) -> int:
        return self.shape[2]

    def wait_on_stream(self) -> None:
        """The calling thread's library stream waits, on the device, for the image to be complete."""
        if self._ready is not None:
            self._ready.stream_wait()

    def synchronize(self) -> None:
        """The host waits for the image to be complete: for a reader on a stream of its own."""
        if self._ready is not None:
            self._ready.synchronize()

    # ---- the array it stands for --------------------------------------------------------------------------------
    @property
    def size(self) -> int:
        return int(np.prod(self.shape))

    @property
    def nbytes(self) -> int:
        return self.size

    def __len__(self) -> int:
        return self.shape[0]

    def host(self) -> np.ndarray:
        """The image on the host: downloaded on first use, the same array afterwards."""
        if self._host is None:
            self.wait_on_stream()
            self._host = _dev_download(self._buf, self.shape)
        return self._host

    def _read(self) -> np.ndarray:
        v = self.host().view()
        v.flags.writeable = False      # the device copy is the one the layers read: nobody changes the other
        return v

    def __array__(self, dtype=None, copy=None):
        a = self._read()
        if dtype is not None and np.dtype(dtype) != a.dtype:
            return a.astype(dtype)
        return a.copy() if copy else a

    def __array_ufunc__(self, ufunc, method, *inputs, out=None, **kwargs):
        args = [x._read() if isinstance(x, DevicePixmap) else x for x in inputs]
        if out is not None:            # (a DevicePixmap among them is read-only: numpy says so)
            kwargs["out"] = tuple(o._read() if isinstance(o, DevicePixmap) else o for o in out)
        return getattr(ufunc, method)(*args, **kwargs)

    def __array_function__(self, func, types, args, kwargs):
        def down(x):
            if isinstance(x, DevicePixmap):
                return x._read()
            if isinstance(x, (list, tuple)):
                return type(x)(down(v) for v in x)
            return x
        return func(*down(args), **{k: down(v) for k, v in kwargs.items()})

    def __getitem__(self, key):
        return self._read()[key]

    def __iter__(self):
        return iter(self._read())

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._read(), name)          # copy, astype, tobytes, reshape, T, mean ...: the host array's

    def __repr__(self):
        return f"DevicePixmap(shape={self.shape}, uint8, {'on the device' if self._host is None else 'host copy made'})"

    def __reduce__(self):
        return (np.array, (self.host(),))           # checkpoints, queues, deepcopy: the array and nothing else

    def close(self):
        if self._buf is not None:
            self._buf.close()
            self._buf = None


# ---- the gradient's tree ------------------------------------------------------------------------------------------
def generate_tree(node_type: int = NODE_TRIPLE, depth: int = 5) -> tuple:
    """GradientPixmapSource.generate (still.py:94-119): the same draws from `random`, in the same order."""
    if depth <= 0 and node_type != NODE_Z:
        return generate_tree(NODE_Z, 0)
    if node_type in (NODE_TRIPLE, NODE_MIX):
        return (node_type, generate_tree(NODE_B, depth - 1), generate_tree(NODE_B, depth - 1),
                generate_tree(NODE_B, depth - 1))
    if node_type == NODE_B:
        if random.random() < .25:
            return generate_tree(NODE_Z, depth - 1)
        return generate_tree(NODE_MIX, depth - 1)
    if node_type == NODE_Z:
        x = random.random()
        if x < .333:
            return (NODE_I, None, None, None)
        if x < .666:
            return (NODE_J, None, None, None)
        return (NODE_RGB, random.random() * 2 - 1, random.random() * 2 - 1, random.random() * 2 - 1)
    raise ValueError(f"Unkown node type {node_type}")


def flatten_tree(tree: tuple) -> list:
    """Postfix order (children before their parent, the root last): [(type, a, b, c)], the numbers 0.0 where unused."""
    nt, a, b, c = tree
    if nt in (NODE_MIX, NODE_TRIPLE):
        return flatten_tree(a) + flatten_tree(b) + flatten_tree(c) + [(nt, 0.0, 0.0, 0.0)]
    if nt == NODE_RGB:
        return [(nt, float(a), float(b), float(c))]
    if nt in (NODE_I, NODE_J):
        return [(nt, 0.0, 0.0, 0.0)]
    raise NotImplementedError(f"Unknown node type {nt}")                                # still.py:149


def unflatten_tree(nodes) -> tuple:
    stack = []
    for nt, a, b, c in nodes:
        nt = int(nt)
        if nt in (NODE_MIX, NODE_TRIPLE):
            if len(stack) < 3:
                raise ValueError("malformed postfix order")
            kids = stack[-3:]
            del stack[-3:]
            stack.append((nt, *kids))
        elif nt == NODE_RGB:
            stack.append((nt, float(a), float(b), float(c)))
        elif nt in (NODE_I, NODE_J):
            stack.append((nt, None, None, None))
        else:
            raise NotImplementedError(f"Unknown node type {nt}")
    if len(stack) != 1:
        raise ValueError("malformed postfix order")
    return stack[0]


# ---- the sources --------------------------------------------------------------------------------------------------
class HipPixmapSource:
    """transflow/pixmap/source.py:15-120."""

    IMAGE_EXTS = {".jpg", ".jpeg", ".png", ".webp", ".bmp", ".ico", ".tiff"}
    MJPEG_EXTS = MJPEG_EXTS               # raw MJPEG streams: decoded on the device (HipMjpegPixmapSource)
    STILL_RE = r"^(color:[a-z0-9\(\)#, ]+|color|#?[0-9a-f]{6}|noise|bwnoise|cnoise|gradient|first)$"   # source.py:83

    def __init__(self, alteration_path: str | None, length: int | None = None):
        self.alteration_path = alteration_path
        self.width: int | None = None
        self.height: int | None = None
        self.framerate: int | None = None
        self.alteration = None
        self.length = length

    def __enter__(self):
        return self

    def __next__(self):
        raise NotImplementedError()

    def __iter__(self):
        return self

    def __exit__(self, exc_type, exc_value, exc_traceback):
        pass

    def load_alteration(self):
        """source.py:40-60 without its loop: flat indices (i * width + j) * 3 + (0, 1, 2) and the RGB values of every
        overlay pixel whose alpha is not 0, in row-major order."""
        if self.alteration_path is None:
            return
        import PIL.Image
        image = np.array(PIL.Image.open(self.alteration_path))
        while image.shape[2] < 4:
            image = np.append(image, np.ones((*image.shape[:2], 1), dtype=np.uint8), 2)
        if self.width is None:
            raise ValueError("Width not initialized")
        ii, jj = np.nonzero(image[:, :, 3] != 0)
        k = (ii.astype(np.int64) * int(self.width) + jj) * 3
        self.alteration = ((k[:, None] + np.arange(3)).reshape(-1), image[ii, jj, :3].reshape(-1))

    def setup(self):
        self.load_alteration()

    def alter(self, array: np.ndarray) -> np.ndarray:
        if self.alteration is None:
            return array
        np.put(array, self.alteration[0], self.alteration[1])                           # source.py:68
        return array

    @classmethod
    def from_args(cls, path: str, size, seek=None, seed=None, seek_time=None, alteration_path=None, repeat: int = 1,
                  flow_path=None, mjpeg_parallel_scan: bool = False, y4m_inputs=False, y4m_matrix: str = "bt601"):
        """source.py:71-120; of the video paths (CvPixmapSource there) a raw MJPEG stream file and a `%0Nd.png` frame
        sequence are served, and with `y4m_inputs` (True, or "linear" for that chroma filter) a .y4m file, read with
        `y4m_matrix`.  mjpeg_parallel_scan: HipMjpegPixmapSource's `parallel_scan`."""
        ext = os.path.splitext(path)[1]
        still_match = re.match(cls.STILL_RE, path.lower().strip())
        if still_match is not None:
            width, height = size
            still_class = still_match.group(1)
            if still_class == "color":
                return HipColorPixmapSource(width, height, seed=seed, alteration_path=alteration_path)
            if still_class.startswith("color:"):
                return HipColorPixmapSource(width, height, still_class.split(":", 1)[1], seed=seed,
                                            alteration_path=alteration_path)
            if re.match(r"#?[0-9a-f]{6}", still_class):
                return HipColorPixmapSource(width, height, still_class, seed=seed, alteration_path=alteration_path)
            if still_class == "noise":
                return HipNoisePixmapSource(width, height, seed, alteration_path)
            if still_class == "bwnoise":
                return HipBwNoisePixmapSource(width, height, seed, alteration_path)
            if still_class == "cnoise":
                return HipColoredNoisePixmapSource(width, height, seed, alteration_path)
            if still_class == "gradient":
                return HipGradientPixmapSource(width, height, seed)                     # source.py:108: no alteration
            if still_class == "first":
                assert flow_path is not None
                return HipVideoStillPixmapSource(flow_path, alteration_path)
            raise ValueError(f"Unknown pixmap source '{still_match.group(1)}'")
        if os.path.isfile(path) and ext.lower() in cls.IMAGE_EXTS:
            return HipImagePixmapSource(path, alteration_path)
        if os.path.isfile(path) and ext.lower() in cls.MJPEG_EXTS:
            return HipMjpegPixmapSource(path, seek, seek_time, alteration_path, repeat, parallel_scan=mjpeg_parallel_scan)
        from .pngdec import is_png_sequence
        if is_png_sequence(path):
            return HipPngSequencePixmapSource(path, seek, seek_time, alteration_path, repeat)
        if y4m_inputs and os.path.isfile(path) and ext.lower() == ".y4m":
            return HipY4mPixmapSource(path, seek, seek_time, alteration_path, repeat, matrix=y4m_matrix,
                                      chroma="linear" if y4m_inputs == "linear" else "replicate")
        raise NotImplementedError(f"video pixmap source '{path}': not served by this backend (CvPixmapSource)")


class HipStillPixmapSource(HipPixmapSource):
    """still.py:12-34.  `_init_array` returns the image as a host array (it then goes up once) or as a DevicePixmap a
    kernel made."""

    def __init__(self, width: int | None = None, height: int | None = None, seed: int | None = None,
                 alteration_path: str | None = None):
        HipPixmapSource.__init__(self, alteration_path, length=None)
        self.width = width
        self.height = height
        self.seed = seed
        self.array: DevicePixmap | None = None

    def _init_array(self):
        raise NotImplementedError()

    def _size(self):
        if self.width is None or self.height is None:
            raise ValueError("Width or height not initialized")
        return int(self.height), int(self.width)

    def __enter__(self):
        made = self._init_array()
        self.width = made.shape[1]
        self.height = made.shape[0]
        self.setup()
        if isinstance(made, DevicePixmap):
            if self.alteration is not None:          # the overlay is numpy's put on the host: down, altered, up again
                host = np.array(made.host())
                made.close()
                made = DevicePixmap.from_host(self.alter(host))
        else:
            made = DevicePixmap.from_host(self.alter(made))
        self.array = made
        return self

    def __next__(self) -> DevicePixmap:
        assert self.array is not None
        return self.array

    def __exit__(self, exc_type, exc_value, exc_traceback):
        if self.array is not None:
            self.array.close()
            self.array = None


class HipColorPixmapSource(HipStillPixmapSource):

    def __init__(self, width: int, height: int, color: str | None = None, seed: int | None = None,
                 alteration_path: str | None = None):
        HipStillPixmapSource.__init__(self, width, height, seed, alteration_path)
        self.color = color

    def _init_array(self):
        from .masks import parse_color
        np.random.seed(self.seed)
        if self.color is None:
            color = list(np.random.randint(0, 256, size=(3), dtype=np.uint8))
        else:
            color = parse_color(self.color)
        h, w = self._size()
        rgb = np.zeros(3, dtype=np.uint8)
        rgb[:] = color                               # numpy's own conversion (and its errors), as still.py:53
        buf = _dev_alloc(h * w * 3)
        _dev_fill(buf, h * w, rgb)
        return DevicePixmap((h, w, 3), buf, _recorded_event())


class HipNoisePixmapSource(HipStillPixmapSource):

    def _init_array(self):
        np.random.seed(self.seed)
        h, w = self._size()
        return np.repeat(np.random.randint(0, 256, size=(h, w, 1), dtype=np.uint8), 3, axis=2)


class HipBwNoisePixmapSource(HipStillPixmapSource):

    def _init_array(self):
        np.random.seed(self.seed)
        h, w = self._size()
        return np.repeat(np.random.choice([0, 255], size=(h, w, 1)), 3, axis=2).astype(np.uint8)


class HipColoredNoisePixmapSource(HipStillPixmapSource):

    def _init_array(self):
        np.random.seed(self.seed)
        h, w = self._size()
        return np.random.randint(0, 256, size=(h, w, 3), dtype=np.uint8)


class HipGradientPixmapSource(HipStillPixmapSource):

    NODE_I, NODE_J, NODE_RGB, NODE_MIX, NODE_TRIPLE, NODE_Z, NODE_B = range(7)

    def generate(self, node_type: int, depth: int) -> tuple:
        return generate_tree(node_type, depth)

    def _init_array(self):
        random.seed(self.seed)
        self.tree = self.generate(self.NODE_TRIPLE, 5)
        h, w = self._size()
        nodes = flatten_tree(self.tree)
        # still.py:144, 147 divide by (height - 1), (width - 1) in every node of the tree, for the first pixel already
        if h > 0 and w > 0 and ((h == 1 and any(n[0] == NODE_I for n in nodes))
                                or (w == 1 and any(n[0] == NODE_J for n in nodes))):
            raise ZeroDivisionError("division by zero")
        buf = _dev_alloc(h * w * 3)
        if h > 0 and w > 0:
            _dev_gradient(buf, w, h, nodes)
        return DevicePixmap((h, w, 3), buf, _recorded_event())


class HipImagePixmapSource(HipStillPixmapSource):

    def __init__(self, path, alteration_path: str | None = None):
        HipStillPixmapSource.__init__(self, alteration_path=alteration_path)
        self.path = path

    def _init_array(self):
        import PIL.Image
        image = PIL.Image.open(self.path)
        array = np.array(image)[:, :, :]
        image.close()
        assert array.shape[2] == 3 or array.shape[2] == 4, f"Pixmap image has unsupported dimension: {array.shape}"
        return array


class HipVideoStillPixmapSource(HipImagePixmapSource):
    """still.py:181-189: the first frame of a video, BGR -> RGB.  `path`: a file (decoded with cv2, as the reference
    does) or any frame provider (`read()` -> BGR frame or None, `release()`: transflow_amd/flow.py)."""

    def _init_array(self):
        provider = self.path
        if isinstance(provider, str):
            from .flow import Cv2FrameProvider
            provider = Cv2FrameProvider(provider)     # ImportError where cv2 is missing
        frame = provider.read()
        assert frame is not None, "Could not open video for still bitmap source"
        array = np.ascontiguousarray(np.asarray(frame)[:, :, ::-1])                     # cv2.COLOR_BGR2RGB
        provider.release()
        return array


class HipMjpegPixmapSource(HipPixmapSource):
    """CvPixmapSource (pixmap/cv.py:11-66) over a raw MJPEG stream file (.mjpeg / .mjpg), a `%0Nd.jpg` pattern or a
    sequence of JPEG files in memory: the same rewind, seek, `repeat` and `length`, every frame decoded on the device
    (transflow_amd/jpegdec.py) and handed out as an RGB `DevicePixmap` -- the compressed bytes go up and the pixels never
    exist on the host.  With an alteration the frame comes down, is altered by numpy.put and goes up again, as the
    stills' overlay does.  (The overlay is loaded once the size is known; the reference loads it before, cv.py:33.)"""

    def __init__(self, path, seek: int | None = None, seek_time: float | None = None, alteration_path: str | None = None,
                 repeat: int = 1, framerate: float = 25.0, parallel_scan: bool = False):
        HipPixmapSource.__init__(self, alteration_path)
        self.path = path
        self.parallel_scan = bool(parallel_scan)    # MjpegFrameProvider's: frames without a restart interval on the device
        self.capture = None                          # the frame provider, under the reference's name for it
        self.seek = seek
        self.seek_time = seek_time
        self.repeat = repeat
        self.loop_index = 1
        self._framerate = framerate

    def rewind(self):
        if self.capture is None:
            raise ValueError("Capture not initialized")
        self.capture.seek_start()
        if self.seek is not None:                    # cv.py:28-30 reads and drops the frames: nothing to decode for that
            self.capture.pos = min(max(0, int(self.seek)), self.capture.frame_count)

    def _open(self):
        """The frame provider over `path` (a subclass has another)."""
        from .jpegdec import MjpegFrameProvider
        return MjpegFrameProvider(self.path, framerate=self._framerate, parallel_scan=self.parallel_scan)

    def __enter__(self):
        self.capture = self._open()
        self.width = int(self.capture.width)
        self.height = int(self.capture.height)
        self.framerate = round(self.capture.framerate)
        self.setup()
        frame_count = self.capture.frame_count
        if self.repeat > 0 and frame_count > 0:
            self.length = int(frame_count) * self.repeat
        if self.seek_time is not None:
            self.seek = int(self.seek_time * self.framerate)
            if self.length is not None:
                self.length -= self.seek * self.repeat
        self.rewind()
        return self

    def __next__(self) -> DevicePixmap:
        assert self.capture is not None
        while True:
            frame = self.capture.read("rgb")
            if frame is not None:
                break
            if self.repeat == 0 or self.loop_index < self.repeat:
                self.loop_index += 1
                self.rewind()
                continue
            raise StopIteration
        if self.alteration is not None:              # numpy's put on the host: down, altered, up again
            host = np.array(frame.host())
            frame.close()
            frame = DevicePixmap.from_host(self.alter(host))
        return frame

    def __exit__(self, exc_type, exc_value, exc_traceback):
        if self.capture is not None:
            self.capture.release()


class HipPngSequencePixmapSource(HipMjpegPixmapSource):
    """CvPixmapSource (pixmap/cv.py:11-66) over a `%0Nd.png` pattern or a sequence of PNG files in memory: the same
    rewind, seek, `repeat`, `length` and alteration as `HipMjpegPixmapSource`, every frame that carries a band index
    decoded on the device (transflow_amd/pngdec.py) and handed out as an RGB `DevicePixmap`."""

    def _open(self):
        from .pngdec import PngSequenceFrameProvider
        return PngSequenceFrameProvider(self.path, framerate=self._framerate)


class HipY4mPixmapSource(HipMjpegPixmapSource):
    """CvPixmapSource (pixmap/cv.py:11-66) over a YUV4MPEG2 file: the same rewind, seek, `repeat`, `length` and alteration
    as `HipMjpegPixmapSource`; the planes go up as they are and every frame is converted on the device
    (transflow_amd/yuvdec.py) and handed out as an RGB `DevicePixmap`.  The frame rate is the header's; `matrix`, `range`
    (None: the header's) and `chroma` are Y4mFrameProvider's."""

    def __init__(self, path, seek: int | None = None, seek_time: float | None = None, alteration_path: str | None = None,
                 repeat: int = 1, matrix: str = "bt601", range: str | None = None, chroma: str = "replicate"):
        HipMjpegPixmapSource.__init__(self, path, seek, seek_time, alteration_path, repeat)
        self.matrix, self.range, self.chroma = matrix, range, chroma

    def _open(self):
        from .yuvdec import Y4mFrameProvider
        return Y4mFrameProvider(self.path, matrix=self.matrix, range=self.range, chroma=self.chroma)


class EndOfPixmap(StopIteration):
    pass


class HipPixmapInterface:
    """PixmapSourceInterface (compositor/pixmap_source_interface.py:12-37) over a source of this process: no queue."""

    def __init__(self, source, introduction_mask):
        self.source = source
        self.image = None
        self.counter: int = -1
        self.introduction_mask = introduction_mask

    def get(self):
        assert self.image is not None
        return self.image

    def next(self, timeout: float = 1):
        try:
            image = next(self.source)
        except StopIteration:
            raise EndOfPixmap from None
        if image is None:
            raise EndOfPixmap
        assert len(image.shape) == 3
        assert image.dtype == np.uint8
        self.image = image
        self.counter += 1
        return self.image

    @property
    def frame_number(self) -> int:
        return self.counter
