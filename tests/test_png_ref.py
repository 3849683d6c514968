"""The numpy restatement of the device's PNG encoder (tests/png_ref.py) against Pillow's decoder and zlib, the cases'
reach, the library's host-side calls, and the host side of the PNG frame path: PngFrame, HipFramesOutput, the drop-in's
routing.  No GPU."""
import glob
import io
import os
import pickle
import sys
import types
import zlib
from fractions import Fraction

import numpy as np
import pytest

from tests import png_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "png_case_*.npz")))
NAMES = list(png_ref.CASES)

_traced = {}


def _trace(name):
    """(image, band_rows, trace): made once."""
    if name not in _traced:
        image, band_rows = png_ref.case(name)
        image.setflags(write=False)
        _traced[name] = (image, band_rows, png_ref.trace(image, band_rows))
    return _traced[name]


def _decode(data: bytes) -> np.ndarray:
    import PIL.Image
    with PIL.Image.open(io.BytesIO(data)) as im:
        assert im.mode == "RGB"
        return np.asarray(im)


# ---- the file -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_pillow_decodes_the_restatements_file_to_the_input(name):
    image, band_rows, t = _trace(name)
    np.testing.assert_array_equal(_decode(t.data), image)


@pytest.mark.parametrize("name", NAMES)
def test_chunks_crcs_and_the_zlib_stream(name):
    image, band_rows, t = _trace(name)
    chunks = png_ref.chunks(t.data)
    assert [k for k, _, _ in chunks] == [b"IHDR"] + [b"IDAT"] * (t.bands + 2) + [b"IEND"]
    for kind, payload, crc in chunks:
        assert crc == zlib.crc32(kind + payload)
    idat = [p for k, p, _ in chunks if k == b"IDAT"]
    assert idat[0] == b"\x78\x01" and idat[-1][:5] == b"\x01\x00\x00\xff\xff" and len(idat[-1]) == 9
    stream = png_ref.filtered(image)
    assert zlib.decompress(b"".join(idat)) == stream                      # which also checks the Adler-32
    assert int.from_bytes(idat[-1][5:], "big") == zlib.adler32(stream)
    for band in idat[1:-1]:                                                # byte-aligned and self-contained
        assert band[-4:] == b"\x00\x00\xff\xff"
    rows = t.band_rows * t.row_bytes
    for n, band in enumerate(idat[1:-1]):
        inflater = zlib.decompressobj(wbits=-15)                           # a band alone is a deflate stream that has not ended
        assert inflater.decompress(band) == stream[n * rows:(n + 1) * rows] and not inflater.eof
    assert len(t.data) <= png_ref.file_bound(image.shape[0], image.shape[1], band_rows)


def test_filtering_is_the_png_specifications():
    """Pillow reverses the filters by the specification: a wrong predictor would not decode.  The choice itself: the
    smallest sum of min(b, 256 - b), ties to the lowest type, checked against a per-row loop."""
    image = png_ref.noise_image(6, 9, 21)
    image[2] = image[1]                                                    # Up is all zeros here
    image[4, :, :] = image[4, :1, :]                                       # Sub is zeros behind the first pixel
    types, rows = png_ref.filter_rows(image)
    cand = png_ref._candidates(image)
    for y in range(6):
        sums = [int(np.minimum(c[y].astype(int), 256 - c[y].astype(int)).sum()) for c in cand]
        assert types[y] == sums.index(min(sums)) and rows[y, 0] == types[y]
        assert (rows[y, 1:] == cand[types[y], y]).all()
    assert types[2] == 2 and types[4] in (1, 4)


# ---- the code -------------------------------------------------------------------------------------------------------------
def test_code_is_complete_and_short():
    assert len(png_ref.LENGTHS) == 286 and min(png_ref.LENGTHS) >= 1
    assert sum(Fraction(1, 2 ** n) for n in png_ref.LENGTHS) == 1
    assert max(png_ref.LENGTHS) <= 15
    print(f"longest code {max(png_ref.LENGTHS)}, longest literal {max(png_ref.LENGTHS[:256])}, end-of-block {png_ref.LENGTHS[256]}")
    # prefix-free by construction of canonical codes from a complete set of lengths; the codes are distinct
    assert len({(n, c) for n, c in zip(png_ref.LENGTHS, png_ref.CODES)}) == 286
    assert png_ref.TABLE_BITS == 1222 and png_ref.TABLE_BITS - 3 == 1219


def test_library_has_the_restatements_code_and_default_bands():
    """Two calls that touch no GPU."""
    from transflow_amd import png
    assert png.code_lengths() == png_ref.LENGTHS
    for h, w in [(1, 1), (1, 21), (7, 1), (24, 40), (9, 50), (1, 6000), (1080, 1920), (2160, 3840), (3, 2730), (3, 2731),
                 (65535, 1), (5, 1365), (100, 2)]:
        assert png.default_band_rows(h, w) == png_ref.default_band_rows(h, w), (h, w)
    assert png_ref.default_band_rows(2160, 3840) == 1 and png_ref.default_band_rows(1080, 1920) == 2
    assert png_ref.default_band_rows(100, 2) == 100 and png_ref.default_band_rows(5000, 2) == 1171


# ---- what the cases reach, by the restatement's own account of what it coded -----------------------------------------
def _runs(name):
    image, band_rows, t = _trace(name)
    return t, t.runs


def test_cases_reach_all_five_filter_types():
    for b in (1, 2, 3, 5, 24, 1000):
        assert set(_trace(f"24x40_noise_b{b}")[2].filter_types) == {0, 1, 2, 3, 4}
    assert set(_trace("9x50_black_b3")[2].filter_types) == {0}             # None wins every tie
    assert _trace("1x6000_ramp")[2].filter_types == [1]                    # Sub
    assert _trace("runs_3_to_258")[2].filter_types == [0]                  # None, by the formula
    assert _trace("1x523_edges")[2].filter_types == [0]


def test_cases_reach_all_length_symbols_and_every_run_length():
    t, runs = _runs("runs_3_to_258")
    assert t.length_symbols == set(range(257, 286))
    assert sorted(n for _, _, n in runs) == list(range(3, 259))
    everything = set()
    for name in NAMES:
        everything |= {n for _, _, n in _runs(name)[1]}
    assert {2, 3, 258, 259, 260, 261, 516} <= everything
    assert sorted(n for _, _, n in _runs("1x523_edges")[1]) == [2, 258, 259, 260, 261, 516]


def test_cases_reach_the_edges_of_trips_rows_and_bands():
    t, runs = _runs("9x50_black_b3")
    assert t.bands == 3 and runs == [(b, 1, 452) for b in range(3)]       # a run from the band's first byte, across its rows
    assert all(s // t.row_bytes != (s + n - 1) // t.row_bytes for _, s, n in runs) and t.longest_run > 258
    t, runs = _runs("40x300_smear")
    assert any(s // png_ref.TRIP != (s + n - 1) // png_ref.TRIP for _, s, n in runs)
    assert t.band_rows > 1 and t.longest_run >= 258 and len(runs) > 40     # long runs ended by literals
    t, runs = _runs("1x6000_ramp")
    stream = png_ref.filtered(_trace("1x6000_ramp")[0])
    assert stream[:5] == b"\x01\x00\x00\x00\xff" and stream.count(b"\xff") == 17997
    assert runs == [(0, 2, 2), (0, 5, 17996)] and 17996 // 258 == 69
    assert _trace("1025x1_b1")[2].bands == 1025 > png_ref.SCAN_CHUNK       # the scan's second chunk
    assert _trace("2049x2_b1")[2].bands == 2049 > 2 * png_ref.SCAN_CHUNK   # ... and its carry read twice
    assert _trace("24x40_noise_b5")[2].bands == 5 and 24 % 5                # a ragged last band
    assert _trace("1x21")[2].row_bytes == 64 and _trace("1x22")[2].row_bytes == 67
    widest = max(_trace(name)[2].widest_trip for name in NAMES)
    print(f"widest trip {widest} bits of {64 * 3 * max(png_ref.LENGTHS[:256])} possible")
    assert widest > 64 * 8                                                 # costlier than stored bytes: noise does that


# ---- the sweep, the band ends and the wide rows: the conditions of the GPU tests ----------------------------------------
def test_sweep_images_are_filtered_with_none_and_hold_every_pair():
    """A row of 0, 1 and a few 2: Up equals None, None wins, and the filtered stream is the designed one -- a 0 and the
    row.  Over the three images every length of SWEEP starts at every stream position mod 64, exactly once; a match of
    258 comes from each of the 64 lanes, one and two pending literals from lane 0 (prev_last's byte) and lane 1."""
    assert sum(png_ref.SWEEP_PARTS.values(), ()) == png_ref.SWEEP
    assert png_ref.SWEEP == (1, 2, 3, 4, 257, 258, 259, 260, 261, 515, 516, 517, 518, 774)
    lanes, pending, at_lane_0 = set(), set(), set()
    for part, lengths in png_ref.SWEEP_PARTS.items():
        image, band_rows, t = _trace(f"sweep_{part}")
        assert image.shape[0] == 1 and image.shape[1] <= 65535 and band_rows == 1 and t.bands == 1
        assert t.filter_types == [0]
        stream = png_ref.filtered(image)
        assert stream == b"\x00" + image.tobytes()
        values = np.bincount(np.frombuffer(stream, np.uint8))
        assert len(values) == 3 and values[2] <= 65 * len(lengths)         # bytes 0 and 1; a 2 where the parity turns
        assert sorted((s % png_ref.TRIP, n) for _, s, n in t.runs) == sorted((p, n) for n in lengths for p in range(64))
        assert t.phase_lengths == {(p, n) for n in lengths for p in range(64)}
        lanes |= t.match_258_lanes
        pending |= t.pending_literals
        if part != "a":
            assert t.match_258_lanes == set(range(64))
        for _, start, n in t.runs:                                         # lane 0's pending literals are the trip before's
            if (start + n) % 64 == 0 and n % 258 in (1, 2):
                assert stream[start + n - 1] == 0 and stream[start + n + 63] == 1
                at_lane_0.add(n % 258)
    assert lanes == set(range(64)) and at_lane_0 == {1, 2}
    assert {(0, 1), (0, 2), (1, 1), (1, 2)} <= pending
    assert {(0, 1), (0, 2), (1, 1), (1, 2)} <= _trace("sweep_a")[2].pending_literals


def test_band_end_cases_have_bands_of_256_and_512_that_end_in_a_stretch():
    """N % 256 == 0: end-of-block's lane is alone in a fresh block of four trips.  The black bands carry a stretch of
    N - 1 into it (a match), the grey tails one of 2 (two pending literals of prev_last's byte) and of 5; the noise
    bands end in no stretch."""
    sizes = {"4x85_%s_b1": [256] * 4, "4x85_%s_b2": [512] * 2, "4x21_%s_b4": [256]}
    for pattern, want in sizes.items():
        for kind in ("noise", "black", "tail"):
            assert _trace(pattern % kind)[2].band_bytes == want
        assert _trace(pattern % "noise")[2].ends_at_band_end == set()
        assert _trace(pattern % "black")[2].ends_at_band_end == {(want[0], want[0] - 1)}
        assert (want[0], 2) in _trace(pattern % "tail")[2].ends_at_band_end
    assert (256, 5) in _trace("4x85_tail_b1")[2].ends_at_band_end
    assert _trace("4x85_black_b2")[2].runs == [(0, 1, 511), (1, 1, 511)] and 511 - 258 >= 3


def test_wide_rows_are_longer_than_adlers_base():
    """A row of 65524 bytes: the rows' sums are combined with row_bytes mod 65521 = 3, not with row_bytes."""
    for name, bands in (("2x21841_noise_b1", 2), ("3x21841_black", 3)):
        image, band_rows, t = _trace(name)
        assert t.row_bytes == 65524 > 65521 and t.band_rows == 1 and t.bands == bands
        stream = png_ref.filtered(image)
        idat = b"".join(p for k, p, _ in png_ref.chunks(t.data) if k == b"IDAT")
        assert zlib.decompress(idat) == stream
        assert int.from_bytes(idat[-4:], "big") == zlib.adler32(stream) == png_ref.adler32(stream)
    assert zlib.adler32(png_ref.filtered(_trace("3x21841_black")[0])) == (3 * 65524 % 65521) << 16 | 1


# ---- the regression pin ---------------------------------------------------------------------------------------------------
def test_golden_files_are_the_restatements():
    """tools/capture_golden_png.py wrote them: the code-length table, and per case its parameters and file."""
    table = np.load(os.path.join(GOLDEN, "png_code_lengths.npz"))
    assert table["lengths"].tolist() == png_ref.LENGTHS and table["codes"].tolist() == png_ref.CODES
    assert sorted(os.path.basename(p)[9:-4] for p in FIXTURES) == sorted(NAMES)
    for path in FIXTURES:
        assert os.path.getsize(path) < (1 << 20)
        with np.load(path) as z:
            name = str(z["name"])
            image, band_rows, t = _trace(name)
            assert (int(z["height"]), int(z["width"]), int(z["band_rows"])) == (image.shape[0], image.shape[1], band_rows)
            assert z["png"].tobytes() == t.data, name


# ---- PngFrame -------------------------------------------------------------------------------------------------------------
def _frame(name="24x40_noise_b5"):
    from transflow_amd.png import PngFrame
    image, band_rows, t = _trace(name)
    return image, PngFrame(t.data, image.shape, t.band_rows)


def test_png_frame_pickles_as_its_fields_only():
    from transflow_amd.png import PngFrame
    image, frame = _frame()
    blob = pickle.dumps(frame)
    back = pickle.loads(blob)
    assert isinstance(back, PngFrame) and back == frame
    assert (back.data, back.shape, back.band_rows) == (frame.data, (24, 40, 3), 5)
    assert len(blob) < len(frame.data) + 200                              # the file and the numbers: no array
    assert bytes(frame) == frame.tobytes() == frame.data and len(frame) == len(frame.data)
    np.testing.assert_array_equal(frame.decode(), image)


def test_pillow_encode_png_is_lossless():
    from transflow_amd.png import pillow_encode_png
    image = png_ref.noise_image(9, 13, 2)
    np.testing.assert_array_equal(_decode(pillow_encode_png(image)), image)


# ---- HipFramesOutput ------------------------------------------------------------------------------------------------------
def test_frames_output_writes_both_kinds_of_frame(tmp_path):
    from transflow_amd.output import HipFramesOutput
    image, frame = _frame()
    template = str(tmp_path / "deep" / "er" / "f_%05d.png")
    out = HipFramesOutput(template, 40, 24, initial_counter=7)
    assert out.output_path is None and not (tmp_path / "deep").exists()
    raw = png_ref.smear_image(24, 40, 5, 7, 3)
    with out as entered:
        assert entered is out and (tmp_path / "deep" / "er").is_dir()
        out.feed(frame)                                                    # the file as it is
        out.feed(raw)                                                      # pixels: encoded here
        out.feed((frame, None))                                            # the pipeline feeds tuples too
        assert out.counter == 10
        with pytest.raises(ValueError):
            out.feed(np.zeros((24, 41, 3), np.uint8))
    names = sorted(p.name for p in (tmp_path / "deep" / "er").iterdir())
    assert names == ["f_00007.png", "f_00008.png", "f_00009.png"]
    assert (tmp_path / "deep" / "er" / "f_00007.png").read_bytes() == frame.data
    assert (tmp_path / "deep" / "er" / "f_00009.png").read_bytes() == frame.data
    np.testing.assert_array_equal(_decode((tmp_path / "deep" / "er" / "f_00007.png").read_bytes()), image)
    np.testing.assert_array_equal(_decode((tmp_path / "deep" / "er" / "f_00008.png").read_bytes()), raw)


def test_png_template():
    from transflow_amd.output import png_template
    assert png_template("out/%05d.png") and png_template("%d.PNG") and png_template("a_%3d_b.png")
    assert not png_template("out/%05d.jpg") and not png_template("out.png") and not png_template("mjpeg")
    assert not png_template(None) and not png_template("out/%05d.png.mp4")


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


def test_install_routes_png_outputs_and_uninstall_restores(stub_transflow, tmp_path):
    from transflow_amd import dropin
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    from transflow_amd.jpeg import JpegFrame
    from transflow_amd.output import HipFramesOutput, HipMjpegOutput
    Out, Comp = stub_transflow.VideoOutput, stub_transflow.Compositor
    out_original, comp_original = Out.__dict__["from_args"], Comp.__dict__["from_args"]
    dropin.install(flow=False)                                            # the default: the outputs are not touched
    try:
        assert Out.__dict__["from_args"] is out_original
        assert Comp.from_args(8, 8, [LayerConfig(0)]).png_frames is False
    finally:
        dropin.uninstall()
    for clash in (dict(jpeg_frames=50), dict(lazy_frames=True)):
        with pytest.raises(ValueError):
            dropin.install(flow=False, png_frames=True, **clash)
        assert Out.__dict__["from_args"] is out_original and Comp.__dict__["from_args"] is comp_original
    dropin.install(flow=False, png_frames=True)
    try:
        comp = Comp.from_args(8, 8, [LayerConfig(0)])
        assert isinstance(comp, HipCompositor) and comp.png_frames is True and comp.jpeg_frames is None
        template = str(tmp_path / "%04d.png")
        out = Out.from_args(template, 40, 24, initial_counter=3, execute=False)
        assert isinstance(out, HipFramesOutput)
        assert (out.template, out.width, out.height, out.counter, out.execute) == (template, 40, 24, 3, False)
        assert out.output_path is None                                    # pipeline.py:479-481 reads it of every output
        image, frame = _frame()
        for path in ("out.mp4", "mjpeg:9001", str(tmp_path / "%04d.jpg")):
            other = Out.from_args(path, 40, 24)
            assert not isinstance(other, (HipFramesOutput, HipMjpegOutput)) and other.output_path == path
            with other as entered:
                entered.feed(image)                                       # pixels pass through to the reference's output
                assert Out.fed[-1] is image
                with pytest.raises(TypeError, match="png_frames"):
                    entered.feed(frame)
                with pytest.raises(TypeError, match="png_frames"):
                    entered.feed((frame, None))
                with pytest.raises(TypeError, match="jpeg_frames"):        # as before
                    entered.feed(JpegFrame(b"", (24, 40, 3), 50, 8))
    finally:
        dropin.uninstall()
    assert Out.__dict__["from_args"] is out_original and Comp.__dict__["from_args"] is comp_original


def test_compositor_flag_is_plain_state():
    from transflow_amd.compositor import HipCompositor
    comp = HipCompositor(8, 8, [], png_frames=True)
    back = pickle.loads(pickle.dumps(comp))
    assert back.png_frames is True and back._png is None and back.jpeg_frames is None
    assert pickle.loads(pickle.dumps(HipCompositor(8, 8, []))).png_frames is False
    with pytest.raises(ValueError):
        HipCompositor(8, 8, [], png_frames=True, lazy_frames=True)
    with pytest.raises(ValueError):
        HipCompositor(8, 8, [], png_frames=True, jpeg_frames=50)
    with pytest.raises(ValueError):
        HipCompositor.from_args(8, 8, [], png_frames=True, jpeg_frames=50)
