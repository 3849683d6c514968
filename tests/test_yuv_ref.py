"""The YUV format of DESIGN.md section 21 without a GPU: the coefficient rule and the library's table, greys, the
derived bound against the float64 model, host_convert against the independent restatement, the frame object, the
compositor's and the drop-in's options, and the two outputs (the Y4M file parsed back; ffmpeg replaced by a stand-in)."""
import pickle
import sys
import types

import numpy as np
import pytest

from tests import yuv_cases, yuv_ref

# |restatement - model| on every sample.  Derived, not measured: the one final rounding costs 0.5; each of the nine
# coefficients is off by at most 2^-17 and the G correction moves one by a few 2^-16 more, which times 255 stays under 0.01.
BOUND = 0.51


# ---- the rule ----------------------------------------------------------------------------------------------------------
def test_rule_reproduces_the_table_and_the_library_returns_it():
    from transflow_amd import yuv
    for (matrix, rng), table in yuv_ref.TABLE.items():
        rows, offset = yuv_ref.rule(matrix, rng)
        assert [list(r) for r in rows] == table, (matrix, rng)
        got, got_offset = yuv.coefficients(matrix, rng)
        assert got.tolist() == table and got_offset == offset == (16 if rng == "tv" else 0), (matrix, rng)
        assert sum(rows[0]) == (56284 if rng == "tv" else 65536)            # rint(219 / 255 * 65536)
        assert sum(rows[1]) == 0 and sum(rows[2]) == 0
    assert yuv_ref.rint_even(yuv_ref.scales("tv")[0] * 65536) == 56284
    with pytest.raises(ValueError):
        yuv.coefficients("bt2020", "tv")
    with pytest.raises(ValueError):
        yuv.coefficients("bt601", "full")


def test_frame_bytes_is_the_layouts_sum_and_zero_for_none():
    from transflow_amd import _lib, yuv
    for layout in yuv_cases.LAYOUTS:
        for h, w in ((1, 1), (3, 3), (5, 17), (270, 480), (2160, 3840)):
            assert yuv.frame_bytes(h, w, layout) == yuv_ref.frame_bytes(h, w, layout)
    assert yuv.frame_bytes(2160, 3840, "yuv420p") == 12441600
    lib = _lib.load()
    assert lib.tf_yuv_frame_bytes(8, 8, 4) == 0 and lib.tf_yuv_frame_bytes(8, 8, -1) == 0 and lib.tf_yuv_frame_bytes(0, 8, 2) == 0


# ---- greys -------------------------------------------------------------------------------------------------------------
def test_greys_have_neutral_chroma_and_the_ranges_ends():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2).repeat(3, axis=0)      # (3, 256, 3): a grey a column
    for matrix, rng in yuv_ref.PAIRS:
        for layout in yuv_cases.LAYOUTS:
            y, u, v = yuv_ref.planes(grey, layout, matrix, rng)
            assert (u == 128).all() and (v == 128).all(), (matrix, rng, layout)
            if rng == "tv":
                assert y[0, 0] == 16 and y[0, 255] == 235
            else:
                assert (y[0] == np.arange(256)).all()


# ---- the bound ---------------------------------------------------------------------------------------------------------
def _worst(sums, k, matrix, rng):
    rows, _ = yuv_ref.rule(matrix, rng)
    ideal = yuv_ref.model(sums, 1 << k, matrix, rng)
    worst = []
    if k == 0:
        worst.append(np.abs(yuv_ref.luma_of(sums.astype(np.uint8), matrix, rng) - ideal[0]).max())
    for row, want in zip(rows[1:], ideal[1:]):
        worst.append(np.abs(yuv_ref.chroma_of_sums(sums, row, k) - want).max())
    return max(worst)


def test_bound_on_the_whole_cube_bt601_tv():
    worst = max(_worst(rgb, 0, "bt601", "tv") for rgb in yuv_ref.cube_slices())
    print(f"bt601/tv, 2^24 triples: max |restatement - model| = {worst:.4f}")
    assert worst <= BOUND


@pytest.mark.parametrize("matrix,rng", yuv_cases.OTHER_PAIRS)
def test_bound_on_a_sample_of_the_other_pairs(matrix, rng):
    triples = np.random.default_rng(601709).integers(0, 256, (2_000_000, 3), dtype=np.uint8)
    worst = _worst(triples, 0, matrix, rng)
    print(f"{matrix}/{rng}, 2e6 triples: max |restatement - model| = {worst:.4f}")
    assert worst <= BOUND


@pytest.mark.parametrize("matrix,rng", yuv_ref.PAIRS)
def test_bound_on_block_sums(matrix, rng):
    sums = np.random.default_rng(2020).integers(0, 1021, (2_000_000, 3))
    worst = _worst(sums, 2, matrix, rng)
    print(f"{matrix}/{rng}, 2e6 sums of 2x2 blocks: max |restatement - model| = {worst:.4f}")
    assert worst <= BOUND


# ---- host_convert, edges -----------------------------------------------------------------------------------------------
def test_host_convert_equals_the_restatement_on_every_gpu_case():
    from transflow_amd.yuv import host_convert
    n = 0
    for name, rgb, layout, matrix, rng in yuv_cases.all_cases():
        frame = host_convert(rgb, layout, matrix, rng)
        assert frame.tobytes() == yuv_ref.convert(rgb, layout, matrix, rng), name
        assert len(frame) == yuv_ref.frame_bytes(rgb.shape[0], rgb.shape[1], layout)
        n += 1
    assert n > 500


@pytest.mark.parametrize("layout", yuv_cases.LAYOUTS)
def test_odd_edges_equal_the_replicated_image(layout):
    from transflow_amd.yuv import host_convert
    rgb = yuv_cases.noise(3, 3, 9)
    padded = np.pad(rgb, ((0, 1), (0, 1), (0, 0)), mode="edge")
    for convert in (lambda im: yuv_ref.planes(im, layout), lambda im: _yuv_planes(host_convert(im, layout))):
        for odd, even in zip(convert(rgb)[1:], convert(padded)[1:]):       # U, then V
            rows, cols = odd.shape
            assert np.array_equal(odd[:, -1], even[:rows, cols - 1]) and np.array_equal(odd[-1], even[rows - 1, :cols])


def _yuv_planes(frame):
    """(Y, U, V) of a YuvFrame, nv12's pairs taken apart."""
    got = frame.planes()
    return (got[0], got[1][:, :, 0], got[1][:, :, 1]) if frame.layout == "nv12" else got


# ---- the frame ---------------------------------------------------------------------------------------------------------
def test_yuv_frame_pickles_as_its_bytes_and_fields():
    from transflow_amd.yuv import YuvFrame, host_convert
    rgb = yuv_cases.noise(5, 7, 3)
    for layout in yuv_cases.LAYOUTS:
        frame = host_convert(rgb, layout, "bt709", "pc")
        assert frame.shape == (5, 7, 3) and (frame.layout, frame.matrix, frame.range) == (layout, "bt709", "pc")
        back = pickle.loads(pickle.dumps(frame))
        assert back == frame and back.tobytes() == frame.tobytes() == bytes(frame.memoryview())
        assert (back.shape, back.layout, back.matrix, back.range) == (frame.shape, layout, "bt709", "pc")
        cls, args = frame.__reduce__()
        assert cls is YuvFrame and isinstance(args[0], bytes)               # never an address
        view = frame.memoryview()
        assert view.obj is frame._data and view.nbytes == len(frame)        # the buffer itself
        for got, want in zip(_yuv_planes(frame), yuv_ref.planes(rgb, layout, "bt709", "pc")):
            assert np.array_equal(got, want) and got.base is not None
    assert YuvFrame(bytes(6), (2, 2, 3)).layout == "yuv420p"
    with pytest.raises(ValueError):
        YuvFrame(bytes(7), (2, 2, 3))
    with pytest.raises(ValueError):
        YuvFrame(bytes(6), (2, 2, 3), "yuv411p")


# ---- options -----------------------------------------------------------------------------------------------------------
def test_compositor_options_exclude_each_other_and_survive_pickling():
    from transflow_amd.compositor import HipCompositor
    for other in (dict(lazy_frames=True), dict(jpeg_frames=80), dict(png_frames=True)):
        with pytest.raises(ValueError, match="a frame leaves in one form"):
            HipCompositor(8, 8, [], yuv_frames="yuv420p", **other)
    for alone in (dict(yuv_matrix="bt709"), dict(yuv_range="pc")):
        with pytest.raises(ValueError, match="yuv_frames"):
            HipCompositor(8, 8, [], **alone)
    for bad in (dict(yuv_frames="yuv411p"), dict(yuv_frames="nv12", yuv_matrix="bt2020"), dict(yuv_frames="nv12", yuv_range="jpeg")):
        with pytest.raises(ValueError):
            HipCompositor(8, 8, [], **bad)
    comp = HipCompositor.from_args(8, 8, [], yuv_frames="nv12", yuv_range="pc")
    assert (comp.yuv_frames, comp.yuv_matrix, comp.yuv_range) == ("nv12", "bt601", "pc")
    back = pickle.loads(pickle.dumps(comp))
    assert (back.yuv_frames, back.yuv_matrix, back.yuv_range) == ("nv12", "bt601", "pc") and back._yuv is None
    plain = HipCompositor(8, 8, [])
    assert plain.yuv_frames is None
    state = plain.__getstate__()
    for key in ("yuv_frames", "yuv_matrix", "yuv_range"):
        del state[key]                                                      # a state pickled before there was the option
    older = object.__new__(HipCompositor)
    older.__setstate__(state)
    assert older.yuv_frames is None and older._yuv is None


@pytest.fixture
def stub_transflow():
    """Stubs of the two reference classes the drop-in patches here."""
    saved = {m: sys.modules[m] for m in list(sys.modules) if m == "transflow" or m.startswith("transflow.")}
    for m in saved:
        del sys.modules[m]

    class VideoOutput:
        def __init__(self, path):
            self.path = path

        @property
        def output_path(self):
            return self.path

        def feed(self, frame):
            raise AssertionError("fed")

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


def test_install_routes_the_outputs_and_uninstall_restores(stub_transflow, tmp_path):
    from transflow_amd import dropin
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    from transflow_amd.output import HipFfmpegOutput, HipY4mOutput, RawFramesOnly
    from transflow_amd.yuv import host_convert
    Out, Comp = stub_transflow.VideoOutput, stub_transflow.Compositor
    out_original, comp_original = Out.__dict__["from_args"], Comp.__dict__["from_args"]
    for other in (dict(jpeg_frames=60), dict(png_frames=True), dict(lazy_frames=True)):
        with pytest.raises(ValueError, match="yuv_frames"):
            dropin.install(flow=False, yuv_frames="yuv420p", **other)
    for alone in (dict(yuv_matrix="bt709"), dict(yuv_range="pc")):
        with pytest.raises(ValueError, match="yuv_frames"):
            dropin.install(flow=False, **alone)
    with pytest.raises(ValueError):
        dropin.install(flow=False, yuv_frames="yuv410p")
    assert Out.__dict__["from_args"] is out_original and Comp.__dict__["from_args"] is comp_original
    dropin.install(flow=False, yuv_frames="yuv422p", yuv_matrix="bt709")
    try:
        comp = Comp.from_args(8, 8, [LayerConfig(0)])
        assert isinstance(comp, HipCompositor) and (comp.yuv_frames, comp.yuv_matrix, comp.yuv_range) == ("yuv422p", "bt709", "tv")
        video = Out.from_args(str(tmp_path / "out.mp4"), 16, 8, framerate=25, vcodec="hevc", replace=True)
        assert isinstance(video, HipFfmpegOutput) and video.output_path == str(tmp_path / "out.mp4")
        assert (video.width, video.height, video.framerate, video.vcodec) == (16, 8, 25, "hevc")
        assert (video.layout, video.matrix, video.range) == ("yuv422p", "bt709", "tv")
        assert Out.from_args("out.avi", 16, 8, replace=True).framerate == 30
        path = str(tmp_path / "out.y4m")
        open(path, "wb").close()                                            # something is there already
        y4m = Out.from_args(path, 16, 8, framerate=24)
        assert isinstance(y4m, HipY4mOutput) and y4m.output_path == str(tmp_path / "out.000.y4m")
        assert (y4m.layout, y4m.matrix, y4m.range, y4m.framerate) == ("yuv422p", "bt709", "tv", 24)
        assert Out.from_args(path, 16, 8, replace=True).output_path == path
        frame = host_convert(yuv_cases.noise(8, 16, 1), "yuv422p", "bt709", "tv")
        for other_path in ("mjpeg:9001", str(tmp_path / "%05d.png"), str(tmp_path / "%d.y4m"), None):
            other = Out.from_args(other_path, 16, 8)                        # every other output: the reference's, wrapped
            assert isinstance(other, RawFramesOnly) and other.output_path == other_path
            with other as entered:
                with pytest.raises(TypeError, match="yuv_frames"):
                    entered.feed(frame)
    finally:
        dropin.uninstall()
    assert Out.__dict__["from_args"] is out_original and Comp.__dict__["from_args"] is comp_original


# ---- the Y4M output ----------------------------------------------------------------------------------------------------
def read_y4m(path):
    """(the header's fields, the frames' (Y, U, V))."""
    data = open(path, "rb").read()
    end = data.index(b"\n")
    fields = data[:end].decode("ascii").split(" ")
    assert fields[0] == "YUV4MPEG2"
    tags = {f[0]: f[1:] for f in fields[1:] if not f.startswith("X")}
    w, h = int(tags["W"]), int(tags["H"])
    cw, ch = {"420jpeg": ((w + 1) // 2, (h + 1) // 2), "422": ((w + 1) // 2, h), "444": (w, h)}[tags["C"]]
    at, frames = end + 1, []
    while at < len(data):
        assert data[at:at + 6] == b"FRAME\n"
        at += 6
        planes = []
        for rows, cols in ((h, w), (ch, cw), (ch, cw)):
            planes.append(np.frombuffer(data, np.uint8, rows * cols, at).reshape(rows, cols))
            at += rows * cols
        frames.append(tuple(planes))
    return fields, frames


@pytest.mark.parametrize("layout,tag", [("yuv420p", "C420jpeg"), ("yuv422p", "C422"), ("yuv444p", "C444")])
def test_y4m_file_parses_back_into_the_planes_fed(tmp_path, layout, tag):
    from transflow_amd.output import HipY4mOutput
    from transflow_amd.yuv import host_convert
    images = [yuv_cases.noise(3, 5, 40 + i) for i in range(3)]
    path = str(tmp_path / "deep" / "out.y4m")
    with HipY4mOutput(path, 5, 3, 30000 / 1001, layout, "bt601", "pc") as out:
        assert out.output_path == path
        out.feed(host_convert(images[0], layout, "bt601", "pc"))
        out.feed(images[1])                                                 # a raw array: host_convert's planes
        out.feed((host_convert(images[2], layout, "bt601", "pc"), None))    # the pipeline's tuples
        with pytest.raises(ValueError):
            out.feed(host_convert(images[0], layout, "bt709", "pc"))        # another matrix than the file's
        with pytest.raises(ValueError):
            out.feed(yuv_cases.noise(4, 5, 1))
    fields, frames = read_y4m(path)
    assert fields == ["YUV4MPEG2", "W5", "H3", "F30000:1001", "Ip", "A1:1", tag, "XCOLORRANGE=FULL"]
    assert len(frames) == 3 and out.frames == 3
    for image, got in zip(images, frames):
        for a, b in zip(got, yuv_ref.planes(image, layout, "bt601", "pc")):
            assert np.array_equal(a, b)
    with HipY4mOutput(path, 5, 3, 25, layout) as again:                     # not `replace`: the next free name
        assert again.output_path == str(tmp_path / "deep" / "out.000.y4m")
    assert read_y4m(again.output_path)[0][3] == "F25:1" and read_y4m(again.output_path)[0][7] == "XCOLORRANGE=LIMITED"
    assert b" F2997:100 " in HipY4mOutput(path, 5, 3, 29.97, layout, replace=True).header()


def test_y4m_refuses_nv12_and_compressed_frames(tmp_path):
    from transflow_amd.jpeg import JpegFrame
    from transflow_amd.output import HipY4mOutput
    from transflow_amd.png import PngFrame
    with pytest.raises(ValueError, match="nv12"):
        HipY4mOutput(str(tmp_path / "a.y4m"), 4, 4, 30, "nv12")
    with HipY4mOutput(str(tmp_path / "a.y4m"), 4, 4, 30) as out:
        with pytest.raises(TypeError, match="JPEG"):
            out.feed(JpegFrame(b"", (4, 4, 3), 50, 8))
        with pytest.raises(TypeError, match="PNG"):
            out.feed(PngFrame(b"", (4, 4, 3), 1))


# ---- the ffmpeg output, over a stand-in --------------------------------------------------------------------------------
STAND_IN = """#!{python}
import sys
open({argv!r}, "w").write("\\n".join(sys.argv[1:]))
with open({data!r}, "wb") as f:
    while True:
        chunk = sys.stdin.buffer.read(65536)
        if not chunk:
            break
        f.write(chunk)
open({done!r}, "w").write("done")
"""


def reference_argv(width, height, framerate, vcodec, path):
    """transflow/output/ffmpeg.py:32-48 without the program's name."""
    return ["-hide_banner", "-loglevel", "error", "-f", "rawvideo", "-vcodec", "rawvideo", "-s", f"{width}x{height}",
            "-pix_fmt", "rgb24", "-r", f"{framerate}", "-i", "-", "-r", f"{framerate}", "-pix_fmt", "yuv420p", "-an",
            "-vcodec", vcodec, path, "-y"]


@pytest.mark.parametrize("layout,matrix,rng", [("yuv420p", "bt601", "tv"), ("nv12", "bt709", "pc")])
def test_ffmpeg_output_argv_and_bytes(tmp_path, layout, matrix, rng):
    import os

    from transflow_amd.output import HipFfmpegOutput
    from transflow_amd.yuv import host_convert
    files = {k: str(tmp_path / k) for k in ("argv", "data", "done")}
    stand_in = tmp_path / "ffmpeg"
    stand_in.write_text(STAND_IN.format(python=sys.executable, **files))
    os.chmod(stand_in, 0o755)
    images = [yuv_cases.noise(6, 10, 60 + i) for i in range(3)]
    target = str(tmp_path / "sub" / "out.mp4")
    out = HipFfmpegOutput(target, 10, 6, 29.97, "libx264", False, True, layout=layout, matrix=matrix, range=rng,
                          ffmpeg_bin=str(stand_in))
    with pytest.raises(ValueError):
        out.feed(images[0])                                                 # not entered (ffmpeg.py:52-53)
    with out:
        assert out.output_path == target and os.path.isdir(tmp_path / "sub")
        out.feed(host_convert(images[0], layout, matrix, rng))
        out.feed(images[1])
        out.feed((host_convert(images[2], layout, matrix, rng), None))
    assert os.path.exists(files["done"]) and out.process.returncode == 0    # __exit__ waited for the child
    want = reference_argv(10, 6, 29.97, "libx264", target)
    want[want.index("rgb24")] = layout
    if (matrix, rng) != ("bt601", "tv"):
        colour = ["-colorspace", matrix, "-color_range", rng]
        at = want.index("-i")
        want[at:at] = colour
        at = want.index("-an")
        want[at:at] = colour
    assert open(files["argv"]).read().split("\n") == want
    assert open(files["data"], "rb").read() == b"".join(yuv_ref.convert(im, layout, matrix, rng) for im in images)


def test_ffmpeg_output_writes_the_frames_buffer_itself():
    from transflow_amd.output import HipFfmpegOutput
    from transflow_amd.yuv import host_convert
    written = []
    out = HipFfmpegOutput("out.mp4", 10, 6, 30, replace=True)
    out.process = types.SimpleNamespace(stdin=types.SimpleNamespace(write=written.append, close=lambda: None), wait=lambda: 0)
    frame = host_convert(yuv_cases.noise(6, 10, 1), "yuv420p")
    out.feed(frame)
    assert isinstance(written[0], memoryview) and written[0].obj is frame._data     # no intermediate copy
