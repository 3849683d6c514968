"""tf_jpeg_create_sub on the GPU: 4:4:4 and 4:2:2 files against libjpeg's own (tests/golden/jpegsub_*.npz, written by
tools/capture_golden_jpeg.py), the whole file, byte for byte -- with the Annex K tables and with the frame's own --
and the way such files go on: the device decoder, the compositor, the MJPEG file output."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from tests import jpeg_cases, jpeg_ref
from tests.jpeg_cases import GOLDEN, first_difference

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "jpegsub_*.npz")))
SUBS = [0, 1]
SUB_IDS = ["444", "422"]


def _case(name, sub):
    return jpeg_cases.load_case(jpeg_cases.fixture_path("jpegsub", name, sub))


def test_every_case_is_here():
    names = sorted(os.path.basename(jpeg_cases.fixture_path("jpegsub", name, sub))
                   for name in jpeg_cases.LAYOUT_CASES for sub in SUBS)
    assert sorted(os.path.basename(p) for p in FIXTURES) == names


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_encoder_writes_libjpegs_file(path):
    from transflow_amd.jpeg import JpegEncoder
    image, quality, restart, sub, optimize, expected = jpeg_cases.load_case(path)
    enc = JpegEncoder(image.shape[0], image.shape[1], quality, restart, optimize=optimize, subsampling=sub)
    try:
        assert enc.subsampling == sub and enc.restart_mcus == restart
        if not optimize:
            assert enc.header == expected[:len(enc.header)] == jpeg_ref.header(*image.shape[:2], quality, restart, sub)
        got = enc.encode(image)
        assert got == expected, first_difference(got, expected)
        if optimize:
            assert enc.header == expected[:len(enc.header)]
        frame = enc.frame(image)
        assert frame.data == expected and (frame.subsampling, frame.optimize, frame.restart_mcus) == (sub, optimize, restart)
    finally:
        enc.close()


@pytest.mark.parametrize("optimize", [False, True], ids=["annex_k", "own_tables"])
@pytest.mark.parametrize("sub", SUBS, ids=SUB_IDS)
def test_one_encoder_keeps_no_state_between_images(sub, optimize):
    """Fat MCUs, then a flat image of a few bytes per MCU, then the first again: bits left in the LDS buffer past the
    words a small trip zeroes, in the second MCU's blocks of a trip of one, or in the staging slots, would show."""
    from transflow_amd.jpeg import JpegEncoder
    a, quality, restart, _, _, want_a = _case("33x47_noise_q100_opt" if optimize else "33x47_noise_q100", sub)
    b = np.empty((33, 47, 3), np.uint8)
    b[:] = (90, 160, 30)
    want_b = jpeg_ref.encode(b, quality, restart, sub, optimize)
    enc = JpegEncoder(33, 47, quality, restart, optimize=optimize, subsampling=sub)
    try:
        assert enc.encode(a) == want_a
        assert enc.encode(b) == want_b
        assert enc.encode(a) == want_a
    finally:
        enc.close()


@pytest.mark.parametrize("sub", SUBS, ids=SUB_IDS)
def test_a_buffer_one_byte_short_is_refused_and_left_alone(sub):
    from transflow_amd.jpeg import JpegEncoder
    image, quality, restart, _, _, expected = _case("33x47_noise_q100", sub)
    enc = JpegEncoder(33, 47, quality, restart, subsampling=sub)
    try:
        guard = 64
        buf = np.full(len(expected) + guard, 0xA5, np.uint8)
        short = buf[:len(expected) - 1]
        with pytest.raises(ValueError):
            enc.encode_into(image, short)
        assert enc.last_needed == len(expected)                            # the library says what it takes
        assert (buf == 0xA5).all()                                         # nothing written, within or beyond
        for capacity in (0, 10, len(enc.header), len(enc.header) + 5):
            with pytest.raises(ValueError):
                enc.encode_into(image, buf[:capacity])
            assert enc.last_needed == len(expected) and (buf == 0xA5).all()
        exact = buf[:len(expected)]
        assert enc.encode_into(image, exact) == len(expected)
        assert exact.tobytes() == expected and (buf[len(expected):] == 0xA5).all()
    finally:
        enc.close()


@pytest.mark.parametrize("name", ["23x41_r3_opt", "33x47_binary_q10_opt", "8x8_opt"])
@pytest.mark.parametrize("sub", SUBS, ids=SUB_IDS)
def test_gathered_histograms_are_the_restatements(sub, name):
    from transflow_amd.jpeg import JpegEncoder
    image, quality, restart, _, _, expected = _case(name, sub)
    enc = JpegEncoder(image.shape[0], image.shape[1], quality, restart, optimize=True, subsampling=sub)
    try:
        assert enc.encode(image) == expected
        tables, counts = enc.last_tables(counts=True)
        np.testing.assert_array_equal(counts, jpeg_ref.histograms(image, quality, restart, sub))
        assert tables == [(list(b), list(v)) for b, v in jpeg_ref.tables(image, quality, restart, sub)]
    finally:
        enc.close()


def test_bad_subsampling_values_are_refused():
    from transflow_amd import _lib
    from transflow_amd.jpeg import JpegEncoder
    for bad in (3, -1, "4:1:1", "444", None, 1.0, True):
        with pytest.raises(ValueError):
            JpegEncoder(8, 8, 50, subsampling=bad)
    lib = _lib.load()
    for bad in (3, -1, 22):
        h = C.c_void_p(1)
        assert lib.tf_jpeg_create_sub(C.byref(h), 8, 8, 50, 0, bad) == _lib.TF_ERR_UNSUPPORTED and not h.value
        with pytest.raises(NotImplementedError, match="subsampling"):
            _lib.check(_lib.TF_ERR_UNSUPPORTED)
    for args in ((0, 8, 50), (8, 8, 101), (8, 8, 50, 65536)):                # the other arguments are checked as ever
        with pytest.raises(ValueError):
            JpegEncoder(*args, subsampling=0)


def test_names_and_numbers_make_the_same_encoder():
    from transflow_amd.jpeg import JpegEncoder
    image = jpeg_cases.formula_image(17, 33)
    for name, value in (("4:4:4", 0), ("4:2:2", 1), ("4:2:0", 2)):
        enc = JpegEncoder(17, 33, 50, 4, subsampling=name)
        try:
            assert enc.subsampling == value
            assert enc.encode(image) == jpeg_ref.encode(image, 50, 4, value)
        finally:
            enc.close()


@pytest.mark.parametrize("optimize", [False, True], ids=["annex_k", "own_tables"])
@pytest.mark.parametrize("sub", [0, 1, 2], ids=["444", "422", "420"])
def test_default_interval_is_the_one_the_host_encodes_with(sub, optimize):
    """16, 12 and 8 MCUs: 2.1, 2.8 and 1.5 intervals of this image's MCU rows, so intervals wrap rows."""
    from transflow_amd import _lib
    from transflow_amd.jpeg import JpegEncoder, pillow_encode
    default = int(_lib.load().tf_jpeg_default_restart_mcus_for(sub))
    assert default == (16, 12, 8)[sub]
    image = jpeg_cases.noise_image(45, 61, seed=9) // 2 + jpeg_cases.formula_image(45, 61) // 2
    enc = JpegEncoder(45, 61, 75, optimize=optimize, subsampling=sub)
    try:
        assert enc.restart_mcus == default
        got, want = enc.encode(image), pillow_encode(image, 75, default, optimize, sub)
        assert got == want, first_difference(got, want)
    finally:
        enc.close()


@pytest.mark.parametrize("sub", SUBS, ids=SUB_IDS)
def test_device_decoder_returns_pillows_pixels_of_a_device_made_file(sub):
    from transflow_amd.framecodec import pillow_decode
    from transflow_amd.jpeg import JpegEncoder
    from transflow_amd.jpegdec import JpegDecoder, probe
    image = jpeg_cases.noise_image(23, 41, seed=2) // 2 + jpeg_cases.formula_image(23, 41) // 2
    enc = JpegEncoder(23, 41, 90, 3, subsampling=sub)
    dec = JpegDecoder(41, 23)
    try:
        data = enc.encode(image)
        info = probe(data)
        assert (info.width, info.height, info.h_samp, info.v_samp, info.restart_mcus) == (41, 23, 2 - (sub == 0), 1, 3)
        pixels = dec.decode_or_host(data)
        np.testing.assert_array_equal(np.asarray(pixels), pillow_decode(data))
        assert dec.fallbacks == 0
        pixels.close()
    finally:
        enc.close()
        dec.close()


# ---- the compositor returns the file ------------------------------------------------------------------------------------
H, W, FRAMES = 40, 56, 3


class _HostSource:
    def __init__(self, array, introduction_mask):
        self.array, self.introduction_mask, self.counter = array, introduction_mask, -1

    def next(self, timeout=1):
        self.counter += 1
        return self.array

    @property
    def frame_number(self):
        return self.counter


def _render_all(jpeg_frames, **options):
    from oracle import remap_ref as OR
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    rng = np.random.default_rng(1)
    comp = HipCompositor.from_args(H, W, [LayerConfig(0, classname="moveref")], background_color="#204060",
                                   jpeg_frames=jpeg_frames, **options)
    comp.set_sources({0: [_HostSource(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), np.ones((H, W), bool))]})
    flow_rng = np.random.default_rng(4)
    out = []
    try:
        for _ in range(FRAMES):
            comp.update(OR.post_process(flow_rng.normal(0, 2.5, (H, W, 2)).astype(np.float32), OR.BACKWARD))
            frame = comp.render()
            out.append(frame if jpeg_frames is not None else np.array(frame))   # (a raw frame is the pool's array: copy)
    finally:
        comp.close()
    return out


@pytest.fixture(scope="module")
def plain_render():
    return _render_all(None)


@pytest.mark.parametrize("optimize", [False, True], ids=["annex_k", "own_tables"])
@pytest.mark.parametrize("sub", SUBS, ids=SUB_IDS)
def test_compositor_returns_the_file_of_its_plain_render(plain_render, sub, optimize):
    from transflow_amd import _lib
    from transflow_amd.jpeg import JpegFrame
    files = _render_all(60, jpeg_subsampling=sub, jpeg_optimize=optimize)
    default = int(_lib.load().tf_jpeg_default_restart_mcus_for(sub))
    assert (plain_render[0] != plain_render[-1]).any()
    for t, (frame, raw) in enumerate(zip(files, plain_render)):
        assert isinstance(frame, JpegFrame) and frame.shape == (H, W, 3)
        assert (frame.quality, frame.subsampling, frame.optimize, frame.restart_mcus) == (60, sub, optimize, default)
        want = jpeg_ref.encode(raw, 60, default, sub, optimize)
        assert frame.data == want, f"frame {t}: " + first_difference(frame.data, want)


# ---- recorded, and fed back ---------------------------------------------------------------------------------------------
def test_a_recorded_444_stream_is_read_back_on_the_device(tmp_path):
    """Three 4:4:4 frames from the encoder through HipMjpegFileOutput, read back by MjpegFrameProvider."""
    from transflow_amd.framecodec import pillow_decode
    from transflow_amd.jpeg import JpegEncoder
    from transflow_amd.jpegdec import MjpegFrameProvider
    from transflow_amd.output import HipMjpegFileOutput
    images = [jpeg_cases.noise_image(23, 41, seed=30 + i) // 2 + jpeg_cases.formula_image(23, 41) // 2 for i in range(3)]
    enc = JpegEncoder(23, 41, 85, subsampling="4:4:4")
    try:
        frames = [enc.frame(image) for image in images]
    finally:
        enc.close()
    with HipMjpegFileOutput(str(tmp_path / "render.mjpeg"), 41, 23, 25.0, quality=85, subsampling=0) as out:
        for frame in frames:
            out.feed(frame)
    provider = MjpegFrameProvider(out.output_path, framerate=25.0)
    try:
        assert (provider.frame_count, provider.width, provider.height) == (3, 41, 23)
        for frame in frames:
            assert frame.subsampling == 0
            got = provider.read(order="rgb")
            np.testing.assert_array_equal(np.asarray(got), pillow_decode(frame.data))
            got.close()
        assert provider.read() is None and provider.fallbacks == 0
    finally:
        provider.release()
