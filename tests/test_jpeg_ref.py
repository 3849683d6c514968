"""The numpy restatement of libjpeg's baseline encoder (tests/jpeg_ref.py) against libjpeg's own files, and the host
side of the JPEG frame path: JpegFrame, HipMjpegOutput, the drop-in's routing.  No GPU."""
import asyncio
import glob
import inspect
import io
import os
import pickle
import sys
import types

import numpy as np
import pytest

from tests import jpeg_cases, jpeg_ref
from tests.jpeg_cases import GOLDEN
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "jpeg_*.npz")))


def _pillow_with_restart():
    try:
        import PIL.JpegImagePlugin as plugin
    except ImportError:
        return False
    return "restart_marker_blocks" in inspect.getsource(plugin._save)


needs_pillow_restart = pytest.mark.skipif(not _pillow_with_restart(), reason="no Pillow with restart_marker_blocks")


def test_every_case_has_its_fixture():
    assert sorted(os.path.basename(p)[5:-4] for p in FIXTURES) == sorted(jpeg_cases.BASELINE_CASES)
    for path in FIXTURES:
        image, quality, restart, _, _, expected = jpeg_cases.load_case(path)
        h, w, _, q, r = jpeg_cases.BASELINE_CASES[os.path.basename(path)[5:-4]]
        assert image.shape == (h, w, 3) and image.dtype == np.uint8 and (quality, restart) == (q, r)
        assert os.path.getsize(path) < (1 << 20)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[5:-4])
def test_restatement_equals_libjpegs_file(path):
    image, quality, restart, _, _, expected = jpeg_cases.load_case(path)
    got = jpeg_ref.encode(image, quality, restart)
    assert len(got) == len(expected)
    assert got == expected


def test_fixtures_exercise_what_they_are_for():
    """The failure modes the cases are chosen for do occur in their files."""
    def scan(name):
        data = jpeg_cases.load_case(jpeg_cases.fixture_path("jpeg", name)).jpeg
        return data[data.index(b"\xff\xda") + 14:-2]
    noisy = scan("33x47_noise_q100")
    assert b"\xff\x00" in noisy                                            # byte stuffing
    wrapped = scan("45x61_r1")                                             # 12 intervals: RST0 .. RST7, RST0, RST1, RST2
    assert [wrapped.count(bytes([0xFF, 0xD0 + k])) for k in range(8)] == [2, 2, 2, 1, 1, 1, 1, 1]
    assert not any(bytes([0xFF, 0xD0 + k]) in scan("45x61_r100") for k in range(8))            # one interval: no marker
    # category 11: a DC step of 2040 between neighbouring blocks of the checkerboard
    y = jpeg_ref.ycc(jpeg_cases.checkerboard(32, 32))[0]
    dc = jpeg_ref.blocks_quantised(y, jpeg_ref.quant_table(jpeg_ref.QUANT_LUMA, 100))[..., 0]
    assert int(abs(dc[0, 1] - dc[0, 0])).bit_length() == 11


@needs_pillow_restart
@pytest.mark.parametrize("shape,quality,restart", [((16, 16), 75, 1), ((10, 10), 50, 1), ((40, 24), 90, 2), ((23, 57), 30, 5),
                                                   ((49, 31), 100, 7), ((8, 8), 1, 3)])
def test_restatement_equals_live_pillow(shape, quality, restart):
    from transflow_amd.jpeg import pillow_encode
    for image in (jpeg_cases.stored_image(*shape, seed=quality), jpeg_cases.rng_noise_image(*shape, seed=restart)):
        assert jpeg_ref.encode(image, quality, restart) == pillow_encode(image, quality, restart)


@needs_pillow_restart
@pytest.mark.parametrize("image,quality,restart", [
    (lambda: jpeg_cases.directed_luma(96, 96, 3), 100, 3), (lambda: jpeg_cases.directed_luma(40, 56, 4), 90, 2),
    (lambda: jpeg_cases.directed_chroma(96, 96, 3), 100, 4), (lambda: jpeg_cases.directed_chroma(50, 70, 4), 75, 1),
    (lambda: jpeg_cases.binary_noise(32, 48, 5), 100, 2), (lambda: jpeg_cases.chroma_checker(48, 80), 100, 3),
    (lambda: jpeg_cases.formula_image(16, 16400), 50, 1)],                # 1025 intervals
    ids=["directed_luma", "directed_luma_ragged", "directed_chroma", "directed_chroma_ragged", "binary_noise",
         "chroma_checker", "1025_intervals"])
def test_restatement_equals_live_pillow_on_directed_content(image, quality, restart):
    """Seeds and sizes that no fixture has."""
    from transflow_amd.jpeg import pillow_encode
    image = image()
    assert jpeg_ref.encode(image, quality, restart) == pillow_encode(image, quality, restart)


# ---- what the fixtures reach, by the restatement's own account of what it coded -------------------------------------
ALL_AC = {0x00, 0xF0} | {(run << 4) | size for run in range(16) for size in range(1, 11)}      # 162 per table
_traced = {}


def _trace(name):
    """The trace of a fixture's image, whose file is the fixture's: made once."""
    if name not in _traced:
        image, quality, restart, _, _, expected = jpeg_cases.load_case(jpeg_cases.fixture_path("jpeg", name))
        _traced[name] = jpeg_ref.trace(image, quality, restart)
        assert _traced[name].data == expected
    return _traced[name]


def _small_cases():
    """Every case but the `formula` ones, which are there for their sizes and interval counts, not for their symbols."""
    return [name for name, case in jpeg_cases.BASELINE_CASES.items() if case[2] != "formula"]


def test_trace_is_encodes_own_account():
    image, quality, restart, _, _, expected = jpeg_cases.load_case(jpeg_cases.fixture_path("jpeg", "45x61_r3"))
    t = _trace("45x61_r3")
    assert len(t.mcu_bits) == len(t.flushed) == len(t.interval_end) == 12
    assert t.interval_end == [False, False, True] * 4
    scan = expected[len(jpeg_ref.header(45, 61, quality, restart)):-2]
    # the flushed bytes, stuffed and with a marker behind each interval but the last, are the scan
    again = bytearray()
    for n, (chunk, end) in enumerate(zip(t.flushed, t.interval_end)):
        again += chunk.replace(b"\xff", b"\xff\x00")
        if end and n != 11:
            again += bytes([0xFF, 0xD0 + (n // 3) % 8])
    assert bytes(again) == scan
    # bits carried from MCU to MCU within an interval, padded at its end
    for first in range(0, 12, 3):
        assert sum(len(c) for c in t.flushed[first:first + 3]) == (sum(t.mcu_bits[first:first + 3]) + 7) // 8
    assert t.most_zrls(0)[0] <= 3 and 0x00 in t.ac_symbols[0] and t.widest_lane[0] <= 59 and t.widest_lane[1] <= 56


def test_fixtures_reach_the_symbols_and_widths_they_are_for():
    """Conditions on the inputs, not on any kernel.  The floors are those of the issue that asked for the cases; what
    the fixtures reach is in DESIGN.md section 15."""
    total = jpeg_ref.Trace()
    for name in _small_cases():
        total.merge(_trace(name))
    luma, chroma = total.ac_symbols
    assert luma <= ALL_AC and chroma <= ALL_AC
    print(f"AC symbols: luma {len(luma)}, missing {sorted(map(hex, ALL_AC - luma))}; "
          f"chroma {len(chroma)}, missing {sorted(map(hex, ALL_AC - chroma))}")
    print(f"ZRLs -> largest size: {total.zrl_sizes}; widest lanes {total.widest_lane}; fattest MCU {max(total.mcu_bits)} bits")
    assert len(luma) >= 150 and len(chroma) >= 130
    assert {(run << 4) | size for run in range(16) for size in range(1, 8)} <= luma
    for table, lane_bits in ((0, 55), (1, 50)):
        assert total.zrl_sizes[table].get(3, 0) >= 5                       # three ZRLs in front of a size of 5 or more
        assert total.widest_lane[table] >= lane_bits
        assert total.dc_categories[table] == set(range(12))
    assert max(total.mcu_bits) >= 4600


def test_fattest_case_puts_ff_at_the_edges_of_the_flush_loop():
    """An MCU's bytes leave 64 at a time, a ballot placing the stuffed ones: an 0xFF in the last lane of a trip, in the
    first lane of a later trip, and as the last byte of an interval (1-padding, then FF 00 FF Dn)."""
    t = _trace("32x48_binary_q100")
    assert max(t.mcu_bits) >= 4600 and max(len(c) for c in t.flushed) > 8 * 64
    assert any(byte == 0xFF and j % 64 == 63 for chunk in t.flushed for j, byte in enumerate(chunk))
    assert any(byte == 0xFF and j % 64 == 0 and j >= 64 for chunk in t.flushed for j, byte in enumerate(chunk))
    ends = [chunk for chunk, end in zip(t.flushed, t.interval_end) if end]
    assert len(ends) == 3 and any(chunk[-1] == 0xFF for chunk in ends[:-1])
    expected = jpeg_cases.load_case(jpeg_cases.fixture_path("jpeg", "32x48_binary_q100")).jpeg
    assert any(bytes([0xFF, 0x00, 0xFF, 0xD0 + k]) in expected for k in range(2))


@pytest.mark.parametrize("name,intervals", [("512x512_r1", 1024), ("16x16400_r1", 1025), ("730x725_r1", 2116),
                                            ("1x65500", 512), ("65500x1", 512), ("40x4099", 97)])
def test_interval_counts_are_the_ones_the_cases_are_for(name, intervals):
    """Counted from the file: RST markers plus one.  (An 0xFF of the entropy-coded data has an 0x00 behind it.)"""
    data = jpeg_cases.load_case(jpeg_cases.fixture_path("jpeg", name)).jpeg
    scan = data[data.index(b"\xff\xda") + 14:-2]
    markers = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert len(markers) + 1 == intervals
    assert markers == [0xD0 + i % 8 for i in range(intervals - 1)]


# ---- JpegFrame ---------------------------------------------------------------------------------------------------------
def _frame(shape=(24, 40), quality=50, restart=4, seed=3):
    from transflow_amd.jpeg import JpegFrame
    image = jpeg_cases.stored_image(*shape, seed=seed)
    return image, JpegFrame(jpeg_ref.encode(image, quality, restart), image.shape, quality, restart)


def test_jpeg_frame_pickles_as_its_fields_only():
    from transflow_amd.jpeg import JpegFrame
    image, frame = _frame()
    blob = pickle.dumps(frame)
    back = pickle.loads(blob)
    assert isinstance(back, JpegFrame) and back == frame
    assert (back.data, back.shape, back.quality, back.restart_mcus) == (frame.data, (24, 40, 3), 50, 4)
    assert len(blob) < len(frame.data) + 200                              # the file and four numbers: no array
    assert bytes(frame) == frame.tobytes() == frame.data and len(frame) == len(frame.data)


def test_jpeg_frame_decodes_to_the_picture():
    pytest.importorskip("PIL")
    image, frame = _frame(quality=95)
    decoded = frame.decode()
    assert decoded.shape == image.shape and decoded.dtype == np.uint8
    # chroma is halved and the picture noisy: close in the mean, not pixel by pixel
    assert np.abs(decoded.astype(int) - image.astype(int)).mean() < 16


# ---- HipMjpegOutput ----------------------------------------------------------------------------------------------------
def test_mjpeg_output_serves_a_jpeg_frame_as_it_is():
    from transflow_amd.output import HipMjpegOutput
    image, frame = _frame()
    out = HipMjpegOutput("localhost", 8080, 40, 24, 30.0, quality=50)
    out.feed(frame)
    served = asyncio.run(out.stream.get_frame_processed())
    assert served.tobytes() is frame.data
    out.feed((frame, None))                                                # pipeline.py feeds tuples too (mjpeg.py:182)
    assert out.stream.processed().tobytes() is frame.data
    assert out.stream.get_bandwidth() == 2 * len(frame.data)
    with pytest.raises(ValueError):
        out.feed(_frame(shape=(16, 16))[1])
    with pytest.raises(ValueError):
        out.feed(np.zeros((24, 41, 3), np.uint8))


@needs_pillow_restart
def test_mjpeg_output_encodes_a_raw_frame_to_the_same_bytes():
    from transflow_amd import output
    image, frame = _frame(restart=output.default_restart_mcus())         # asked of the library: no GPU is opened
    out = output.HipMjpegOutput("localhost", 8080, 40, 24, 30.0, quality=50)
    out.feed(image)
    assert out.stream.processed().tobytes() == frame.data                 # what the device encoder's frame would be


def test_mjpeg_address():
    from transflow_amd.output import mjpeg_address
    assert mjpeg_address("mjpeg") == ("localhost", 8080)
    assert mjpeg_address("MJPEG:9000") == ("localhost", 9000)
    assert mjpeg_address("mjpeg:9000:my-host") == ("my-host", 9000)
    assert mjpeg_address("out.mp4") is None and mjpeg_address(None) is None
    with pytest.raises(ValueError):
        mjpeg_address("mjpeg:1:2:3")


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


def test_install_routes_outputs_and_uninstall_restores(stub_transflow):
    from transflow_amd import dropin
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    from transflow_amd.output import HipMjpegOutput
    Out, Comp = stub_transflow.VideoOutput, stub_transflow.Compositor
    out_original, comp_original = Out.__dict__["from_args"], Comp.__dict__["from_args"]
    dropin.install(flow=False)                                            # the default: the outputs are not touched
    try:
        assert Out.__dict__["from_args"] is out_original
        assert Comp.from_args(8, 8, [LayerConfig(0)]).jpeg_frames is None
    finally:
        dropin.uninstall()
    assert Comp.__dict__["from_args"] is comp_original
    with pytest.raises(ValueError):
        dropin.install(flow=False, jpeg_frames=50, lazy_frames=True)
    dropin.install(flow=False, jpeg_frames=60)
    try:
        comp = Comp.from_args(8, 8, [LayerConfig(0)])
        assert isinstance(comp, HipCompositor) and comp.jpeg_frames == 60
        out = Out.from_args("mjpeg:9001", 40, 24, framerate=12.5)
        assert isinstance(out, HipMjpegOutput)
        assert (out.host, out.port, out.width, out.height, out.framerate, out.quality) == ("localhost", 9001, 40, 24, 12.5, 60)
        assert out.output_path is None                                    # pipeline.py:479-481 reads it of every output
        other = Out.from_args("out.mp4", 40, 24)
        assert other.output_path == "out.mp4"                             # ... the wrapped one's is the reference's
        image, frame = _frame()
        with other as entered:
            entered.feed(image)                                           # pixels pass through to the reference's output
            assert Out.fed[-1] is image and other.path == "out.mp4"
            with pytest.raises(TypeError, match="jpeg_frames"):
                entered.feed(frame)
            with pytest.raises(TypeError, match="jpeg_frames"):
                entered.feed((frame, None))
    finally:
        dropin.uninstall()
    assert Out.__dict__["from_args"] is out_original and Comp.__dict__["from_args"] is comp_original


def test_wrapped_output_survives_pickling_and_copying():
    """An object whose __init__ has not run (what unpickling makes first) has no `_output`: an AttributeError, not a
    recursion."""
    import copy
    from transflow_amd.output import RawFramesOnly
    blank = RawFramesOnly.__new__(RawFramesOnly)
    with pytest.raises(AttributeError):
        blank.feed_count
    wrapped = RawFramesOnly(types.SimpleNamespace(output_path="x.mp4", feed=lambda frame: None))
    again = copy.copy(wrapped)
    assert again.output_path == "x.mp4"


def test_host_encode_refuses_a_pillow_without_restart_markers(monkeypatch):
    PIL = pytest.importorskip("PIL")
    from transflow_amd.jpeg import pillow_encode
    monkeypatch.setattr(PIL, "__version__", "9.5.0")
    with pytest.raises(RuntimeError, match="restart_marker_blocks"):
        pillow_encode(np.zeros((8, 8, 3), np.uint8), 50, 4)


def test_compositor_flag_is_plain_state():
    from transflow_amd.compositor import HipCompositor
    comp = HipCompositor(8, 8, [], jpeg_frames=50)
    back = pickle.loads(pickle.dumps(comp))
    assert back.jpeg_frames == 50 and back._jpeg is None
    assert pickle.loads(pickle.dumps(HipCompositor(8, 8, []))).jpeg_frames is None
    with pytest.raises(ValueError):
        HipCompositor(8, 8, [], jpeg_frames=50, lazy_frames=True)
    with pytest.raises(ValueError):
        HipCompositor(8, 8, [], jpeg_frames=0)
