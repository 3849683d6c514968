"""The MJPEG output for frames that arrive compressed (transflow/output/mjpeg.py:160-189 is the one it mirrors).

The reference's MjpegOutput keeps the last raw frame and encodes it whenever a client's turn comes
(mjpeg.py:54-65, :90-94).  `HipMjpegOutput` keeps the last frame as it came: a `JpegFrame` (transflow_amd/jpeg.py: the
compositor encoded it on the device) is served as it is; a raw array is encoded on request, on the host, by Pillow at
the same quality, subsampling and restart interval -- the same bytes by construction, and the output process never
opens the GPU.  The reference's server and handler are used unchanged and imported only in `__enter__`: everything
else here works without aiohttp, netifaces or cv2.

`HipFramesOutput` is the same for the frame-sequence output (transflow/output/frames.py, `-o out/%05d.png`): a `PngFrame`
(transflow_amd/png.py) is written to its file as it is, a raw array is encoded by Pillow on the host.  A template that
ends in `.jpg` / `.jpeg` takes `JpegFrame`s the same way.

`HipMjpegFileOutput` appends the frames' JPEG files to one file, a raw MJPEG stream: the form the device decoder's
inputs are read in (`MJPEG_EXTS`; transflow_amd/jpegdec.py MjpegFrameProvider, transflow_amd/pixmap.py), so a render
recorded this way can be fed back as a flow or pixmap input without leaving the device path.

`HipFfmpegOutput` is the reference's default output (transflow/output/ffmpeg.py, every `-o out.mp4`) for frames that
arrive as planes: a `YuvFrame` (transflow_amd/yuv.py: the compositor converted it on the device) is written to the ffmpeg
child's pipe as it is, and the child is told the layout instead of `rgb24`, so its software scaler has nothing to do.
`HipY4mOutput` writes the same frames to a `.y4m` file, the uncompressed container ffmpeg, mpv and the x264 / x265
command lines read.  A raw array fed to either is converted by `host_convert`, the same arithmetic in numpy.
"""
from __future__ import annotations

import os
import pathlib
import re

import numpy as np

from .jpeg import JpegFrame, pillow_encode, subsampling_value
from .png import PngFrame, pillow_encode_png
from .yuv import YuvFrame, check_options, host_convert


def default_restart_mcus(subsampling=None) -> int:
    """What a raw frame is encoded with on the host: the device encoder's default interval, asked of the library (the
    call loads it and touches no GPU).  With a `subsampling`, that layout's default."""
    from . import _lib
    if subsampling is None:
        return int(_lib.load().tf_jpeg_default_restart_mcus())
    return int(_lib.load().tf_jpeg_default_restart_mcus_for(subsampling_value(subsampling)))


def _host_jpeg(frame, quality: int, restart_mcus, optimize: bool, subsampling: int) -> bytes:
    """A raw frame as the device encoder would have written it: Pillow with the same settings (restart_mcus None: the
    library's default for the layout)."""
    if restart_mcus is None:
        restart_mcus = default_restart_mcus(subsampling)
    return pillow_encode(np.asarray(frame), quality, restart_mcus, optimize, subsampling)


class _Encoded:
    """What the reference's handler asks of a processed frame: `.tobytes()` (mjpeg.py:94)."""

    def __init__(self, data: bytes):
        self._data = data

    def tobytes(self) -> bytes:
        return self._data

    def __len__(self) -> int:
        return len(self._data)


class HipMjpegStream:
    """MjpegStream's surface (mjpeg.py:26-73) for the reference's _StreamHandler and MjpegServer.add_stream:
    `name`, `fps`, `set_frame`, `get_frame`, `get_frame_processed`, `get_bandwidth`."""

    def __init__(self, name: str, size, quality: int = 50, fps: float = 30, restart_mcus: int | None = None,
                 optimize: bool = False, subsampling=2):
        self.optimize = bool(optimize)                     # a raw frame is encoded with its own Huffman tables
        self.subsampling = subsampling_value(subsampling)  # ... and with this chroma layout
        self.name = name.lower().casefold().replace(" ", "_")
        self.size = size                                   # (width, height)
        self.quality = max(1, min(int(quality), 100))
        self.fps = fps
        self.restart_mcus = None if restart_mcus is None else int(restart_mcus)    # None: the library's default
        self._frame = None
        self._sizes = []

    def set_frame(self, frame) -> None:
        self._frame = frame

    def processed(self) -> _Encoded:
        frame = self._frame
        if frame is None:                                  # nothing fed yet: a grey frame of the stream's size
            frame = np.full((self.size[1], self.size[0], 3), 128, np.uint8)
        if isinstance(frame, JpegFrame):
            data = frame.tobytes()
        else:
            if self.restart_mcus is None:
                self.restart_mcus = default_restart_mcus(self.subsampling)
            data = _host_jpeg(frame, self.quality, self.restart_mcus, self.optimize, self.subsampling)
        self._sizes = (self._sizes + [len(data)])[-30:]
        return _Encoded(data)

    def get_bandwidth(self) -> float:
        return sum(self._sizes)

    async def get_frame(self):
        return self._frame

    async def get_frame_processed(self) -> _Encoded:
        return self.processed()


class HipMjpegOutput:
    """Same constructor, context-manager protocol and `feed` as transflow's MjpegOutput."""

    def __init__(self, host: str, port: int, width: int, height: int, framerate: float, quality: int = 50,
                 optimize: bool = False, subsampling=2):
        self.width, self.height = int(width), int(height)
        self.host, self.port = host, port
        self.framerate = framerate
        self.quality = quality
        self.stream = HipMjpegStream("transflow", (self.width, self.height), quality=quality, fps=framerate, optimize=optimize,
                                     subsampling=subsampling)
        self.server = None

    @property
    def output_path(self):
        """VideoOutput.output_path (video_output.py:62-64): pipeline.py:479-481 reads it of every output; no file."""
        return None

    def __enter__(self):
        from transflow.output.mjpeg import MjpegServer     # aiohttp, netifaces, cv2: only a served stream needs them
        self.server = MjpegServer(self.host, self.port)
        self.server.add_stream(self.stream)
        self.server.start()
        return self

    def feed(self, frame):
        if isinstance(frame, tuple):                       # mjpeg.py:182-183
            frame = frame[0]
        if tuple(frame.shape[:2]) != (self.height, self.width):
            raise ValueError(f"the stream is {self.height} x {self.width}, the frame {tuple(frame.shape[:2])}")
        self.stream.set_frame(frame)

    def __exit__(self, exc_type, exc_value, exc_traceback):
        if self.server is not None:
            self.server.stop()


MJPEG_PATH = re.compile(r"^mjpeg(:[:a-z0-9A-Z\-]+)?$", re.IGNORECASE)        # video_output.py:37


def mjpeg_address(path):
    """(host, port) of an `mjpeg[:port[:host]]` output path (video_output.py:37-52), None for any other path."""
    m = MJPEG_PATH.match(path) if isinstance(path, str) else None
    if m is None:
        return None
    args = m.group(1)[1:].split(":") if m.group(1) else []
    if len(args) > 2:
        raise ValueError(f"Invalid number of MJPEG arguments: {len(args)}")
    return (args[1] if len(args) == 2 else "localhost"), (int(args[0]) if args else 8080)


FRAMES_PATH = re.compile(r"%(\d+)?d")                                         # video_output.py:55


def png_template(path) -> bool:
    """Whether an output path is a frame-sequence template (video_output.py:55-58) whose files are PNGs."""
    return isinstance(path, str) and FRAMES_PATH.search(path) is not None and path.lower().endswith(".png")


JPEG_FILE_EXTS = (".jpg", ".jpeg")


def jpeg_template(path) -> bool:
    """Whether an output path is a frame-sequence template whose files are JPEGs."""
    return isinstance(path, str) and FRAMES_PATH.search(path) is not None and path.lower().endswith(JPEG_FILE_EXTS)


def mjpeg_file_path(path) -> bool:
    """Whether an output path names a raw MJPEG stream file: an extension the device decoder's inputs are found by."""
    from .pixmap import MJPEG_EXTS
    return isinstance(path, str) and FRAMES_PATH.search(path) is None and os.path.splitext(path)[1].lower() in MJPEG_EXTS


class HipFramesOutput:
    """Same constructor, context-manager protocol and `feed` as transflow's FramesVideoOutput (frames.py:15-36): frame
    n goes to `template % (initial_counter + n)`.  A PngFrame's bytes are the file; a raw array (what the pipeline
    feeds when the output is a flow rendering) is encoded by Pillow here.  A template that ends in .jpg / .jpeg writes
    JPEG files instead: a JpegFrame's bytes are the file, and a raw array is encoded by `pillow_encode` with this
    output's `quality`, `subsampling`, `restart_mcus` (None: the library's default for the layout) and `optimize`.
    Never opens the GPU."""

    def __init__(self, template: str, width: int, height: int, initial_counter: int = 0, execute: bool = False,
                 quality: int = 50, subsampling=2, restart_mcus: int | None = None, optimize: bool = False):
        self.width, self.height = int(width), int(height)
        self.template = template
        self.directory = pathlib.Path(self.template).parent
        self.execute = execute
        self.counter = initial_counter
        self.jpeg = template.lower().endswith(JPEG_FILE_EXTS)
        self.quality = max(1, min(int(quality), 100))
        self.subsampling = subsampling_value(subsampling)
        self.restart_mcus = None if restart_mcus is None else int(restart_mcus)
        self.optimize = bool(optimize)

    @property
    def output_path(self):
        """VideoOutput.output_path (video_output.py:62-64), which FramesVideoOutput inherits: no single file."""
        return None

    def __enter__(self):
        if not os.path.isdir(self.directory):                # frames.py:25-26
            os.makedirs(self.directory)
        return self

    def feed(self, frame):
        if isinstance(frame, tuple):
            frame = frame[0]
        if tuple(frame.shape[:2]) != (self.height, self.width):
            raise ValueError(f"the output is {self.height} x {self.width}, the frame {tuple(frame.shape[:2])}")
        if self.jpeg:
            if isinstance(frame, PngFrame):
                raise TypeError(f"HipFramesOutput writes JPEG files to {self.template}, not PNG files: "
                                "install(png_frames=True) serves %d ... .png frame templates")
            data = frame.tobytes() if isinstance(frame, JpegFrame) else _host_jpeg(frame, self.quality, self.restart_mcus,
                                                                                   self.optimize, self.subsampling)
        else:
            if isinstance(frame, JpegFrame):
                raise TypeError("HipFramesOutput writes PNG files, not JPEG files: install(jpeg_frames=...) serves the mjpeg "
                                "output, %d ... .jpg frame templates and .mjpeg files")
            data = frame.tobytes() if isinstance(frame, PngFrame) else pillow_encode_png(np.asarray(frame))
        with open(self.template % self.counter, "wb") as f:
            f.write(data)
        self.counter += 1

    def __exit__(self, exc_type, exc_value, exc_traceback):
        if self.execute:                                     # frames.py:35-36
            from transflow.utils import startfile
            startfile(self.directory.as_posix())


def _unique_path(path: str) -> str:
    """The reference's find_unique_path (utils.py:147-160), as FFmpegVideoOutput uses it (ffmpeg.py:21); where transflow
    is not importable, this package's statement of the same naming (transflow_amd/archive.py)."""
    try:
        from transflow.utils import find_unique_path
    except ImportError:
        from .archive import unique_path as find_unique_path
    return find_unique_path(path)


class HipMjpegFileOutput:
    """A raw MJPEG stream file: every frame's JPEG file appended to `path`, back to back -- what `ffmpeg -f mjpeg`
    writes and what `MJPEG_EXTS` inputs are read as.  Same context-manager protocol and `feed` as the other outputs
    (the constructor is FFmpegVideoOutput's, ffmpeg.py:17-25, with the JPEG settings in place of the codec).  A
    JpegFrame's bytes are appended as they are; a raw array is encoded by `pillow_encode` with this output's `quality`,
    `subsampling`, `restart_mcus` (None: the library's default for the layout) and `optimize`.  `path` is used as given
    if `replace`, otherwise the first free name of the reference's rule.  The stream carries no frame rate: `framerate`
    is kept for the reader to pass on.  Never opens the GPU."""

    def __init__(self, path: str, width: int, height: int, framerate: float, quality: int = 50, subsampling=2,
                 restart_mcus: int | None = None, optimize: bool = False, execute: bool = False, replace: bool = False):
        self.width, self.height = int(width), int(height)
        self.path = path if replace else _unique_path(path)
        self.framerate = framerate
        self.quality = max(1, min(int(quality), 100))
        self.subsampling = subsampling_value(subsampling)
        self.restart_mcus = None if restart_mcus is None else int(restart_mcus)
        self.optimize = bool(optimize)
        self.execute = execute
        self.frames = 0
        self._file = None

    @property
    def output_path(self):
        """VideoOutput.output_path (ffmpeg.py:65-67): pipeline.py:481-483 writes the config beside it."""
        return self.path

    def __enter__(self):
        dirname = os.path.dirname(self.path)                 # ffmpeg.py:28-30
        if not os.path.isdir(dirname) and dirname != "":
            os.makedirs(dirname)
        self._file = open(self.path, "wb")
        return self

    def feed(self, frame):
        if self._file is None:
            raise ValueError("the output is not open")
        if isinstance(frame, tuple):
            frame = frame[0]
        if isinstance(frame, PngFrame):
            raise TypeError(f"HipMjpegFileOutput writes JPEG files to {self.path}, not PNG files: install(png_frames=True) "
                            "serves %d ... .png frame templates")
        if tuple(frame.shape[:2]) != (self.height, self.width):
            raise ValueError(f"the output is {self.height} x {self.width}, the frame {tuple(frame.shape[:2])}")
        data = frame.tobytes() if isinstance(frame, JpegFrame) else _host_jpeg(frame, self.quality, self.restart_mcus,
                                                                               self.optimize, self.subsampling)
        self._file.write(data)
        self.frames += 1

    def __exit__(self, exc_type, exc_value, exc_traceback):
        if self._file is not None:
            self._file.close()
            self._file = None
        if self.execute:                                     # ffmpeg.py:62-63
            from transflow.utils import startfile
            startfile(self.path)


def y4m_path(path) -> bool:
    """Whether an output path names a Y4M file: no frame template, and the extension."""
    return isinstance(path, str) and FRAMES_PATH.search(path) is None and path.lower().endswith(".y4m")


def ffmpeg_path(path) -> bool:
    """Whether video_output.py:55-60 sends an output path to FFmpegVideoOutput: a string that is neither an `mjpeg`
    address nor a frame template."""
    return isinstance(path, str) and MJPEG_PATH.match(path) is None and FRAMES_PATH.search(path) is None


class _YuvOutput:
    """What the two outputs of planes share: the settings, and the frame a `feed` ends with."""

    def __init__(self, width: int, height: int, layout: str, matrix: str, range: str):
        check_options(layout, matrix, range)
        self.width, self.height = int(width), int(height)
        self.layout, self.matrix, self.range = layout, matrix, range
        self.frames = 0

    def _planes(self, frame) -> YuvFrame:
        """A YuvFrame of this output's settings as it is; a raw array by way of `host_convert`."""
        if isinstance(frame, tuple):
            frame = frame[0]
        if isinstance(frame, (JpegFrame, PngFrame)):
            kind = "JPEG" if isinstance(frame, JpegFrame) else "PNG"
            raise TypeError(f"{type(self).__name__} writes {self.layout} planes, not {kind} files: install(yuv_frames=...) "
                            "serves the ffmpeg and .y4m outputs")
        if tuple(frame.shape[:2]) != (self.height, self.width):
            raise ValueError(f"the output is {self.height} x {self.width}, the frame {tuple(frame.shape[:2])}")
        if not isinstance(frame, YuvFrame):
            return host_convert(np.asarray(frame).astype(np.uint8, copy=False), self.layout, self.matrix, self.range)
        if (frame.layout, frame.matrix, frame.range) != (self.layout, self.matrix, self.range):
            raise ValueError(f"the output takes {self.layout} / {self.matrix} / {self.range}, the frame is "
                             f"{frame.layout} / {frame.matrix} / {frame.range}")
        return frame


class HipFfmpegOutput(_YuvOutput):
    """Same constructor, context-manager protocol, `feed` and `output_path` as transflow's FFmpegVideoOutput
    (ffmpeg.py:15-67), and `layout`, `matrix`, `range` and `ffmpeg_bin`.  The child's argv is the reference's
    (ffmpeg.py:32-48) with the input `-pix_fmt` set to the layout; the output `-pix_fmt` stays yuv420p.  With bt601 and
    tv nothing else is added and the file is tagged as the reference's is.
    `feed` writes a YuvFrame's buffer to the pipe without a copy.  Never opens the GPU."""

    def __init__(self, path: str, width: int, height: int, framerate: float, vcodec: str = "h264", execute: bool = False,
                 replace: bool = False, layout: str = "yuv420p", matrix: str = "bt601", range: str = "tv",
                 ffmpeg_bin: str = "ffmpeg"):
        super().__init__(width, height, layout, matrix, range)
        self.path = path if replace else _unique_path(path)
        self.framerate = framerate
        self.vcodec = vcodec
        self.execute = execute
        self.ffmpeg_bin = ffmpeg_bin
        self.process = None

    @property
    def output_path(self):
        return self.path

    def colour_flags(self) -> list:
        """What tells ffmpeg a matrix or a range other than the one it assumes; given once for the input, once for the
        output.  NOT VERIFIED: the spelling of these flags (`-colorspace bt709`, `-color_range pc`) is taken from
        ffmpeg's documentation and has not been run against an ffmpeg.  The default settings add none
        of them."""
        flags = []
        if self.matrix != "bt601":
            flags += ["-colorspace", self.matrix]
        if self.range != "tv":
            flags += ["-color_range", self.range]
        return flags

    def argv(self) -> list:
        colour = self.colour_flags()
        return [self.ffmpeg_bin,
                "-hide_banner",
                "-loglevel", "error",
                "-f", "rawvideo",
                "-vcodec", "rawvideo",
                "-s", f"{self.width}x{self.height}",
                "-pix_fmt", self.layout,
                "-r", f"{self.framerate}",
                *colour,
                "-i", "-",
                "-r", f"{self.framerate}",
                "-pix_fmt", "yuv420p",
                *colour,
                "-an",
                "-vcodec", self.vcodec,
                self.path,
                "-y"]

    def __enter__(self):
        import subprocess
        dirname = os.path.dirname(self.path)                 # ffmpeg.py:28-30
        if not os.path.isdir(dirname) and dirname != "":
            os.makedirs(dirname)
        self.process = subprocess.Popen(self.argv(), stdin=subprocess.PIPE)
        return self

    def feed(self, frame):
        if self.process is None or self.process.stdin is None:
            raise ValueError("Process not initialized")      # ffmpeg.py:52-53
        self.process.stdin.write(self._planes(frame).memoryview())
        self.frames += 1

    def __exit__(self, exc_type, exc_value, exc_traceback):
        if self.process is not None and self.process.stdin is not None:
            self.process.stdin.close()
        if self.process is not None:
            self.process.wait()
        if self.execute:                                     # ffmpeg.py:62-63
            from transflow.utils import startfile
            startfile(self.path)


Y4M_CHROMA = {"yuv420p": "C420jpeg", "yuv422p": "C422", "yuv444p": "C444"}      # centre-sited samples
Y4M_RANGE = {"tv": "LIMITED", "pc": "FULL"}


class HipY4mOutput(_YuvOutput):
    """A YUV4MPEG2 file: the header line, then `FRAME` and the planes for every frame.  The constructor is
    FFmpegVideoOutput's (ffmpeg.py:17-25) with the layout, matrix and range in place of the codec; `path` is used as given
    if `replace`, otherwise the first free name of the reference's rule.  The frame rate is written as a fraction of a
    denominator up to 1001 (30000:1001 for 30000 / 1001, 2997:100 for 29.97).  Y4M has no tag for nv12 and none for the
    matrix: the first is a ValueError here, the second is the reader's to know.  Never opens the GPU."""

    def __init__(self, path: str, width: int, height: int, framerate: float, layout: str = "yuv420p", matrix: str = "bt601",
                 range: str = "tv", execute: bool = False, replace: bool = False):
        super().__init__(width, height, layout, matrix, range)
        if layout not in Y4M_CHROMA:
            raise ValueError(f"Y4M has no tag for {layout}: one of {sorted(Y4M_CHROMA)}")
        self.path = path if replace else _unique_path(path)
        self.framerate = framerate
        self.execute = execute
        self._file = None

    @property
    def output_path(self):
        return self.path

    def header(self) -> bytes:
        import fractions
        rate = fractions.Fraction(self.framerate).limit_denominator(1001)
        return (f"YUV4MPEG2 W{self.width} H{self.height} F{rate.numerator}:{rate.denominator} Ip A1:1 "
                f"{Y4M_CHROMA[self.layout]} XCOLORRANGE={Y4M_RANGE[self.range]}\n").encode("ascii")

    def __enter__(self):
        dirname = os.path.dirname(self.path)                 # ffmpeg.py:28-30
        if not os.path.isdir(dirname) and dirname != "":
            os.makedirs(dirname)
        self._file = open(self.path, "wb")
        self._file.write(self.header())
        return self

    def feed(self, frame):
        if self._file is None:
            raise ValueError("the output is not open")
        planes = self._planes(frame)
        self._file.write(b"FRAME\n")
        self._file.write(planes.memoryview())
        self.frames += 1

    def __exit__(self, exc_type, exc_value, exc_traceback):
        if self._file is not None:
            self._file.close()
            self._file = None
        if self.execute:                                     # ffmpeg.py:62-63
            from transflow.utils import startfile
            startfile(self.path)


class RawFramesOnly:
    """Another output of the reference's, as it is, except that a JpegFrame, a PngFrame or a YuvFrame fed to it is refused
    by name: those outputs take pixels (`install(jpeg_frames=...)` is for the MJPEG output, `%d ... .jpg` templates and
    .mjpeg files, `install(png_frames=True)` for `%d ... .png` templates, `install(yuv_frames=...)` for the ffmpeg and
    .y4m outputs)."""

    def __init__(self, output):
        self._output = output

    def __enter__(self):
        self._output.__enter__()
        return self

    def __exit__(self, exc_type, exc_value, exc_traceback):
        return self._output.__exit__(exc_type, exc_value, exc_traceback)

    def feed(self, frame):
        first = frame[0] if isinstance(frame, tuple) else frame
        if isinstance(first, JpegFrame):
            raise TypeError(f"{type(self._output).__name__} takes raw frames, not JPEG files: install(jpeg_frames=...) "
                            "serves the mjpeg output only")
        if isinstance(first, PngFrame):
            raise TypeError(f"{type(self._output).__name__} takes raw frames, not PNG files: install(png_frames=True) "
                            "serves %d ... .png frame templates only")
        if isinstance(first, YuvFrame):
            raise TypeError(f"{type(self._output).__name__} takes raw frames, not YUV planes: install(yuv_frames=...) "
                            "serves the ffmpeg and .y4m outputs only")
        return self._output.feed(frame)

    def __getattr__(self, name):
        if name == "_output":       # not set yet (an instance being unpickled): no attribute, not a recursion
            raise AttributeError(name)
        return getattr(self._output, name)                  # output_path (pipeline.py:479-481) and whatever else it has
