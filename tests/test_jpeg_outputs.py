"""Where a JpegFrame can go besides the HTTP stream: `%d ... .jpg` templates (HipFramesOutput) and raw MJPEG stream files
(HipMjpegFileOutput), the chroma layout on the host side of the JPEG path, and the drop-in's routing.  No GPU: the frames
are Pillow's files of the layout, wrapped as JpegFrames."""
import inspect
import os
import pickle
import sys
import types

import numpy as np
import pytest

from tests import jpeg_cases, jpeg_ref

W, H = 41, 23


def _pillow_with_restart():
    try:
        import PIL.JpegImagePlugin as plugin
    except ImportError:
        return False
    return "restart_marker_blocks" in inspect.getsource(plugin._save)


pytestmark = pytest.mark.skipif(not _pillow_with_restart(), reason="no Pillow with restart_marker_blocks")


def _frames(subsampling, n=3, quality=70, restart=5, optimize=False):
    from transflow_amd.jpeg import JpegFrame, pillow_encode
    images = [jpeg_cases.noise_image(H, W, seed=20 + i) // 2 + jpeg_cases.formula_image(H, W) // 2 for i in range(n)]
    return images, [JpegFrame(pillow_encode(im, quality, restart, optimize, subsampling), im.shape, quality, restart, optimize,
                              subsampling) for im in images]


# ---- JpegFrame, pillow_encode ------------------------------------------------------------------------------------------
def test_jpeg_frame_carries_its_subsampling_and_older_states_are_420():
    from transflow_amd.jpeg import JpegFrame
    _, (frame, *_) = _frames("4:4:4")
    assert frame.subsampling == 0
    back = pickle.loads(pickle.dumps(frame))
    assert back == frame and back.subsampling == 0
    older = JpegFrame(*frame._fields()[:5])                                 # what a frame pickled before the field rebuilds from
    assert older.subsampling == 2
    assert JpegFrame(b"", (8, 8, 3), 50, 8).subsampling == 2
    for bad in (3, -1, "4:1:1", None, 1.5, True):
        with pytest.raises(ValueError):
            JpegFrame(b"", (8, 8, 3), 50, 8, False, bad)


def test_pillow_encode_takes_numbers_and_names():
    from transflow_amd.jpeg import pillow_encode, subsampling_value
    image = jpeg_cases.formula_image(H, W)
    for value, name in ((0, "4:4:4"), (1, "4:2:2"), (2, "4:2:0")):
        assert subsampling_value(value) == subsampling_value(name) == value
        for optimize in (False, True):
            data = pillow_encode(image, 60, 3, optimize, subsampling=name)
            assert data == pillow_encode(image, 60, 3, optimize, subsampling=value)
            assert data == jpeg_ref.encode(image, 60, 3, value, optimize)
    assert pillow_encode(image, 60, 3) == pillow_encode(image, 60, 3, subsampling=2)
    with pytest.raises(ValueError):
        pillow_encode(image, 60, 3, subsampling=3)


def test_optimized_host_encode_of_a_long_thin_444_image_has_room():
    """8188 MCUs of 8 x 8 in a row, noise at quality 100: Pillow's buffer must hold the whole file at once (MAXBLOCK
    follows the MCU size)."""
    from transflow_amd.jpeg import pillow_encode
    image = jpeg_cases.noise_image(1, 65500, seed=4)
    data = pillow_encode(image, 100, 16, optimize=True, subsampling=0)
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9" and len(data) > 65536


def test_default_intervals_keep_48_blocks():
    from transflow_amd import _lib, output
    from transflow_amd.jpeg import default_restart_mcus
    lib = _lib.load()                                                      # loads the library, opens no GPU
    assert [lib.tf_jpeg_default_restart_mcus_for(s) for s in (0, 1, 2)] == [16, 12, 8]
    assert lib.tf_jpeg_default_restart_mcus() == 8
    assert lib.tf_jpeg_default_restart_mcus_for(3) == _lib.TF_ERR_UNSUPPORTED
    assert [default_restart_mcus(s) for s in ("4:4:4", "4:2:2", "4:2:0")] == [16, 12, 8]
    assert output.default_restart_mcus() == 8 and output.default_restart_mcus(0) == 16


# ---- HipMjpegOutput ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subsampling", [0, 1])
def test_mjpeg_stream_host_encodes_a_raw_frame_with_the_same_sampling(subsampling):
    from transflow_amd import output
    from transflow_amd.jpeg import pillow_encode
    images, _ = _frames(subsampling, n=1)
    out = output.HipMjpegOutput("localhost", 8080, W, H, 30.0, quality=70, subsampling=subsampling)
    out.feed(images[0])
    want = pillow_encode(images[0], 70, output.default_restart_mcus(subsampling), subsampling=subsampling)
    assert out.stream.processed().tobytes() == want


# ---- HipFramesOutput ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [".jpg", ".JPEG"])
def test_jpg_templates_get_the_bytes_and_the_counter(tmp_path, ext):
    from transflow_amd.jpeg import pillow_encode
    from transflow_amd.output import HipFramesOutput
    from transflow_amd.png import PngFrame
    images, frames = _frames(0)
    template = str(tmp_path / "sub" / ("%04d" + ext))
    out = HipFramesOutput(template, W, H, initial_counter=7, quality=70, subsampling=0, restart_mcus=5)
    assert out.output_path is None
    with out as entered:
        entered.feed(frames[0])
        entered.feed((frames[1], None))
        entered.feed(images[2])                                            # a raw array: encoded here, with the output's settings
        assert out.counter == 10
        with pytest.raises(TypeError, match="png_frames"):
            entered.feed(PngFrame(b"", (H, W, 3), 8))
        with pytest.raises(ValueError):
            entered.feed(np.zeros((H, W + 1, 3), np.uint8))
        assert out.counter == 10
    written = [open(template % n, "rb").read() for n in (7, 8, 9)]
    assert written[0] == frames[0].data and written[1] == frames[1].data
    assert written[2] == pillow_encode(images[2], 70, 5, subsampling=0) == frames[2].data
    assert sorted(os.listdir(tmp_path / "sub")) == [os.path.basename(template % n) for n in (7, 8, 9)]


def test_a_raw_frame_without_an_interval_takes_the_layouts_default(tmp_path):
    from transflow_amd.jpeg import pillow_encode
    from transflow_amd.output import HipFramesOutput
    images, _ = _frames(1, n=1)
    template = str(tmp_path / "%d.jpg")
    with HipFramesOutput(template, W, H, quality=55, subsampling="4:2:2", optimize=True) as out:
        out.feed(images[0])
    assert open(template % 0, "rb").read() == pillow_encode(images[0], 55, 12, True, 1)


def test_png_templates_still_refuse_a_jpeg_frame(tmp_path):
    from transflow_amd.output import HipFramesOutput
    _, frames = _frames(0, n=1)
    with HipFramesOutput(str(tmp_path / "%04d.png"), W, H) as out:
        with pytest.raises(TypeError, match="jpeg_frames"):
            out.feed(frames[0])
        assert out.counter == 0 and os.listdir(tmp_path) == []


# ---- HipMjpegFileOutput ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subsampling", [0, 1, 2])
def test_mjpeg_file_splits_back_into_its_frames(tmp_path, subsampling):
    from transflow_amd import jpegdec
    from transflow_amd.jpeg import pillow_encode
    from transflow_amd.output import HipMjpegFileOutput
    from transflow_amd.png import PngFrame
    images, frames = _frames(subsampling)
    path = str(tmp_path / "deep" / "er" / "out.mjpeg")
    out = HipMjpegFileOutput(path, W, H, 25.0, quality=70, subsampling=subsampling, restart_mcus=5)
    assert out.output_path == path and out.framerate == 25.0
    with pytest.raises(ValueError):
        out.feed(frames[0])                                                # not entered
    with out as entered:
        entered.feed(frames[0])
        entered.feed((frames[1], None))
        entered.feed(images[2])
        with pytest.raises(TypeError, match="png_frames"):
            entered.feed(PngFrame(b"", (H, W, 3), 8))
        with pytest.raises(ValueError):
            entered.feed(np.zeros((H + 1, W, 3), np.uint8))
        assert out.frames == 3
    data = open(path, "rb").read()
    index = jpegdec.index_mjpeg_stream(data)
    assert [data[at:at + n] for at, n in index] == [f.data for f in frames]
    assert frames[2].data == pillow_encode(images[2], 70, 5, subsampling=subsampling)
    h_samp, v_samp = {0: (1, 1), 1: (2, 1), 2: (2, 2)}[subsampling]
    for at, n in index:
        info = jpegdec.probe(data[at:at + n])
        assert (info.width, info.height, info.components, info.h_samp, info.v_samp, info.restart_mcus) == (W, H, 3, h_samp, v_samp, 5)
        mcus = -(-W // (8 * h_samp)) * -(-H // (8 * v_samp))
        assert info.intervals == -(-mcus // 5)


def test_mjpeg_file_replace_rule(tmp_path):
    from transflow_amd.output import HipMjpegFileOutput
    _, frames = _frames(0, n=2)
    path = str(tmp_path / "out.mjpg")
    with HipMjpegFileOutput(path, W, H, 25.0) as out:
        out.feed(frames[0])
    assert out.output_path == path
    second = HipMjpegFileOutput(path, W, H, 25.0)                          # not replace: the first free name
    assert second.output_path == str(tmp_path / "out.000.mjpg")
    with second:
        second.feed(frames[1])
    assert HipMjpegFileOutput(path, W, H, 25.0).output_path == str(tmp_path / "out.001.mjpg")
    assert open(path, "rb").read() == frames[0].data and open(second.output_path, "rb").read() == frames[1].data
    third = HipMjpegFileOutput(path, W, H, 25.0, replace=True)             # replace: the path as given
    assert third.output_path == path
    with third:
        third.feed(frames[1])
    assert open(path, "rb").read() == frames[1].data


def test_output_path_predicates():
    from transflow_amd.output import jpeg_template, mjpeg_file_path
    assert jpeg_template("out/%05d.jpg") and jpeg_template("%d.JPEG") and not jpeg_template("out.jpg")
    assert not jpeg_template("out/%05d.png") and not jpeg_template(None)
    assert mjpeg_file_path("out.mjpeg") and mjpeg_file_path("a/b.MJPG")
    assert not mjpeg_file_path("out.mp4") and not mjpeg_file_path("mjpeg:9000") and not mjpeg_file_path("%03d.mjpeg")
    assert not mjpeg_file_path(None)


# ---- the compositor's flag ---------------------------------------------------------------------------------------------
def test_compositor_flag_is_plain_state():
    from transflow_amd.compositor import HipCompositor
    comp = HipCompositor(8, 8, [], jpeg_frames=80, jpeg_subsampling="4:4:4")
    back = pickle.loads(pickle.dumps(comp))
    assert back.jpeg_subsampling == 0 and back.jpeg_frames == 80 and back._jpeg is None
    assert pickle.loads(pickle.dumps(HipCompositor(8, 8, [], jpeg_frames=80))).jpeg_subsampling == 2
    state = HipCompositor(8, 8, [], jpeg_frames=80).__getstate__()
    del state["jpeg_subsampling"]                                          # a compositor pickled before the option existed
    older = HipCompositor.__new__(HipCompositor)
    older.__setstate__(state)
    assert older.jpeg_subsampling == 2
    with pytest.raises(ValueError, match="jpeg_frames"):
        HipCompositor(8, 8, [], jpeg_subsampling=0)
    with pytest.raises(ValueError):
        HipCompositor(8, 8, [], jpeg_frames=80, jpeg_subsampling=3)
    with pytest.raises(ValueError):
        HipCompositor.from_args(8, 8, [], jpeg_frames=80, jpeg_subsampling="4:1:1")


# ---- the drop-in's routing, over stubs of the two reference classes it patches ---------------------------------------
@pytest.fixture
def stub_transflow():
    saved = {m: sys.modules[m] for m in list(sys.modules) if m == "transflow" or m.startswith("transflow.")}
    for m in saved:
        del sys.modules[m]

    class VideoOutput:
        fed = []

        def __init__(self, path):
            self.path = path

        @property
        def output_path(self):                                            # video_output.py:62-64
            return self.path

        def feed(self, frame):
            VideoOutput.fed.append(frame)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return None

        @classmethod
        def from_args(cls, path, width, height, framerate=None, vcodec="h264", execute=False, replace=False,
                      initial_counter=0):
            return cls(path)

    class Compositor:
        @classmethod
        def from_args(cls, height, width, layer_configs, background_color="#ffffff"):
            return "the reference's"

    names = {"transflow": {}, "transflow.output": {}, "transflow.output.video_output": {"VideoOutput": VideoOutput},
             "transflow.compositor": {}, "transflow.compositor.compositor": {"Compositor": Compositor}}
    for name, attrs in names.items():
        mod = types.ModuleType(name)
        mod.__path__ = []
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
    try:
        yield types.SimpleNamespace(VideoOutput=VideoOutput, Compositor=Compositor)
    finally:
        for name in names:
            sys.modules.pop(name, None)
        sys.modules.update(saved)


def test_install_routes_jpeg_outputs_and_uninstall_restores(stub_transflow, tmp_path):
    from transflow_amd import dropin
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    from transflow_amd.output import HipFramesOutput, HipMjpegFileOutput, HipMjpegOutput, RawFramesOnly
    Out, Comp = stub_transflow.VideoOutput, stub_transflow.Compositor
    out_original, comp_original = Out.__dict__["from_args"], Comp.__dict__["from_args"]
    with pytest.raises(ValueError, match="jpeg_frames"):
        dropin.install(flow=False, jpeg_subsampling=0)
    with pytest.raises(ValueError):
        dropin.install(flow=False, jpeg_frames=60, jpeg_subsampling=5)
    assert Out.__dict__["from_args"] is out_original and Comp.__dict__["from_args"] is comp_original
    dropin.install(flow=False, jpeg_frames=60, jpeg_subsampling="4:4:4", jpeg_optimize=True)
    try:
        comp = Comp.from_args(8, 8, [LayerConfig(0)])
        assert isinstance(comp, HipCompositor) and (comp.jpeg_frames, comp.jpeg_subsampling, comp.jpeg_optimize) == (60, 0, True)
        stream = Out.from_args("mjpeg:9001", W, H, framerate=12.5)
        assert isinstance(stream, HipMjpegOutput) and stream.stream.subsampling == 0 and stream.stream.optimize
        template = str(tmp_path / "%05d.jpg")
        frames = Out.from_args(template, W, H, initial_counter=3)
        assert isinstance(frames, HipFramesOutput) and frames.jpeg
        assert (frames.template, frames.width, frames.height, frames.counter) == (template, W, H, 3)
        assert (frames.quality, frames.subsampling, frames.optimize, frames.restart_mcus) == (60, 0, True, None)
        path = str(tmp_path / "out.mjpeg")
        open(path, "wb").close()                                           # something is there already
        stream_file = Out.from_args(path, W, H, framerate=12.5)
        assert isinstance(stream_file, HipMjpegFileOutput)
        assert stream_file.output_path == str(tmp_path / "out.000.mjpeg") and stream_file.framerate == 12.5
        assert (stream_file.quality, stream_file.subsampling, stream_file.optimize) == (60, 0, True)
        assert Out.from_args(path, W, H, replace=True).output_path == path
        assert Out.from_args(path, W, H, replace=True).framerate == 30
        _, (frame,) = _frames(0, n=1)
        for other_path in ("out.mp4", str(tmp_path / "%05d.png"), "out.avi"):
            other = Out.from_args(other_path, W, H)                        # every other output: the reference's, wrapped as before
            assert isinstance(other, RawFramesOnly) and other.output_path == other_path
            with other as entered:
                with pytest.raises(TypeError, match="jpeg_frames"):
                    entered.feed(frame)
    finally:
        dropin.uninstall()
    assert Out.__dict__["from_args"] is out_original and Comp.__dict__["from_args"] is comp_original
    dropin.install(flow=False, jpeg_frames=60)                             # without the option: 4:2:0 everywhere, as before
    try:
        assert Comp.from_args(8, 8, [LayerConfig(0)]).jpeg_subsampling == 2
        assert Out.from_args("mjpeg", W, H).stream.subsampling == 2
        assert Out.from_args(str(tmp_path / "%d.jpeg"), W, H).subsampling == 2
    finally:
        dropin.uninstall()
