"""The device's JPEG decoder (transflow_amd/csrc/jpegdec.hip) held to libjpeg's pixels -- the
Pillow decodes kept in tests/golden/jpegdec_valid.npz -- exactly, and to the Python restatement (tests/jpegdec_ref.py)
for what it rejects and why.  tests/test_jpegdec_ref.py runs every file here through the decoder's shared core on the
CPU, under the sanitizers, first.  Every decode writes into a buffer with guard bytes either side."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import jpegdec_ref as JR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 256
MAX_W = MAX_H = 512


def _load(name):
    z = np.load(os.path.join(GOLDEN, name))
    return z, [str(n) for n in z["names"]]


VALID, VALID_NAMES = _load("jpegdec_valid.npz")
MALFORMED, MALFORMED_NAMES = _load("jpegdec_malformed.npz")


class Handle:
    """tf_jpegdec through the C ABI, decoding into the middle of a guarded device buffer."""

    def __init__(self, max_w=MAX_W, max_h=MAX_H, max_file=1 << 20):
        from transflow_amd import _lib
        from transflow_amd.device import DevBuffer
        self.lib, self.check, self.ok = _lib.load(), _lib.check, _lib.TF_OK
        self.h = C.c_void_p()
        self.check(self.lib.tf_jpegdec_create(C.byref(self.h), max_w, max_h, max_file))
        self.room = max_w * max_h * 3
        self.buf = DevBuffer(self.room + 2 * GUARD)

    def decode(self, data: bytes, shape, order: int = 0, shift: int = 0):
        """(return code, reject, pixels of `shape`): the buffer is filled with 0xA5 first, the guards are checked after.
        shift: the output starts that many bytes into the buffer's middle (an output that is not dword-aligned)."""
        n = int(np.prod(shape))
        assert n + shift <= self.room
        self.buf.upload(np.full(self.buf.nbytes, 0xA5, np.uint8))
        reject = C.c_uint32(0xFFFF)
        rc = self.lib.tf_jpegdec_decode_dev(self.h, data, len(data), C.c_void_p(self.buf.ptr + GUARD + shift), order, C.byref(reject))
        back = self.buf.download((self.buf.nbytes,), np.uint8)
        assert (back[:GUARD + shift] == 0xA5).all(), "bytes in front of the output were written"
        assert (back[GUARD + shift + n:] == 0xA5).all(), "bytes behind the output were written"
        return rc, int(reject.value), back[GUARD + shift:GUARD + shift + n].reshape(shape)

    def close(self):
        self.lib.tf_jpegdec_destroy(self.h)
        self.buf.close()


@pytest.fixture(scope="module")
def handle():
    h = Handle()
    yield h
    h.close()


def _valid(name):
    return VALID[name + ".file"].tobytes(), VALID[name + ".rgb"]


def _exact(handle, name, order=0, shift=0):
    data, rgb = _valid(name)
    rc, reject, got = handle.decode(data, rgb.shape, order, shift)
    assert rc == handle.ok
    assert reject == 0, f"{name}: rejected as {JR.REJECT[reject] if reject < len(JR.REJECT) else reject}"
    np.testing.assert_array_equal(got, rgb[:, :, ::-1] if order else rgb)


@pytest.mark.parametrize("name", VALID_NAMES)
def test_valid_files_decode_to_libjpegs_pixels(handle, name):
    """Geometry (partial MCUs right and bottom, the chroma context rows at the edges, 4:2:2, 4:4:4, grey), intervals
    (1, 2, 5, 6 MCUs, none, RSTn wrapping past 7, 4096 of them) and symbols (noise at quality 100 and 1, a flat image,
    optimised and hand-built tables): every file comes back with reject == 0 and Pillow's pixels, exactly."""
    _exact(handle, name)


def test_the_large_case_passes_one_work_groups_share():
    """iv_512_grey_r1 has 4096 intervals, hence 4095 markers, in a scan of more than 16 * 1024 bytes.  The marker scan
    gives a thread 16 bytes (CHUNK) and a work-group 256 threads: 4096 bytes a work-group, so this scan takes more than
    four of them, and its more than 1024 chunk counts take the one-work-group slot scan (SCAN_BLOCK = 1024 a trip)
    through more than one trip, with a carry between them."""
    data, _ = _valid("iv_512_grey_r1")
    hd = JR.parse_header(data)
    scan = len(data) - hd["scan_offset"]
    assert hd["intervals"] == 4096
    assert scan > 16 * 1024 and (scan + 15) // 16 > 1024


@pytest.mark.parametrize("name", ["sym_noise_q100", "sym_noise_q1"])
def test_the_noise_files_hold_stuffed_bytes_and_zrls(name):
    data, _ = _valid(name)
    trace = {}
    JR.decode(data, trace=trace)
    assert trace["ff00"] >= 1 and trace["ac_symbols"].count(0xF0) >= 1


def test_bgr_is_rgb_reversed(handle):
    for name in ("geo_420_37x19", "geo_422_37x19", "geo_grey_37x19"):
        _exact(handle, name, order=1)


def test_an_output_that_is_not_dword_aligned(handle):
    for shift in (1, 2, 3):
        _exact(handle, "geo_420_33x31", shift=shift)


def test_one_handle_takes_frames_of_any_size_and_sampling_back_to_back(handle):
    """Stale tables, stale planes, stale status: each frame must be exact whatever came before it."""
    order = ["geo_420_48x32", "geo_grey_37x19", "geo_444_37x19", "sym_optimize", "geo_420_8x8", "iv_37x19_nodri",
             "geo_422_37x19", "sym_handmade", "iv_160x16_r1", "geo_420_17x9", "sym_noise_q100", "geo_420_16x16"]
    for name in order + order[::-1]:
        _exact(handle, name)


def test_host_copy_entry_point(handle):
    data, rgb = _valid("geo_420_37x19")
    out = np.zeros(rgb.shape, np.uint8)
    reject = C.c_uint32(0xFFFF)
    handle.check(handle.lib.tf_jpegdec_decode(handle.h, data, len(data), C.c_void_p(out.ctypes.data), 0, C.byref(reject)))
    assert reject.value == 0
    np.testing.assert_array_equal(out, rgb)


def test_a_frame_larger_than_the_handle_is_an_argument_error():
    small = Handle(max_w=32, max_h=32, max_file=4096)
    try:
        data, rgb = _valid("geo_420_48x32")
        rc, _, _ = small.decode(data, (32, 32, 3))
        assert rc != small.ok
        data, rgb = _valid("geo_420_17x9")
        rc, reject, got = small.decode(data, rgb.shape)
        assert rc == small.ok and reject == 0
        np.testing.assert_array_equal(got, rgb)
    finally:
        small.close()


def test_round_trip_through_the_device_encoder():
    """A seeded 4:2:0 frame through JpegEncoder at the library's default interval and through JpegDecoder: the
    restatement's decode of those bytes, and Pillow's where Pillow is importable."""
    from transflow_amd.jpeg import JpegEncoder
    from transflow_amd.jpegdec import JpegDecoder, probe
    rng = np.random.default_rng(7)
    h, w = 75, 133
    yy, xx = np.mgrid[0:h, 0:w]
    image = np.clip(np.stack([128 + 90 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0) for c in range(3)], -1) + rng.normal(0, 10, (h, w, 3)),
                    0, 255).astype(np.uint8)
    enc = JpegEncoder(h, w, quality=85)
    data = enc.encode(image)
    info = probe(data)
    assert (info.width, info.height, info.restart_mcus) == (w, h, enc.restart_mcus) and info.intervals > 1
    dec = JpegDecoder(w, h)
    got = np.asarray(dec.decode(data, "rgb"))
    np.testing.assert_array_equal(got, JR.decode(data))
    try:
        from transflow_amd.jpegdec import pillow_decode
        want = pillow_decode(data)
    except ImportError:
        want = None
    if want is not None:
        np.testing.assert_array_equal(got, want)
    dec.close()


def test_python_decoder_rejects_and_falls_back():
    from transflow_amd.jpegdec import JpegDecoder, JpegRejected
    dec = JpegDecoder(64, 64)
    data = MALFORMED["rst_swapped.file"].tobytes()
    with pytest.raises(JpegRejected) as e:
        dec.decode(data)
    assert e.value.reason == "rst_order"
    with pytest.raises(JpegRejected) as e:
        dec.decode(MALFORMED["progressive.file"].tobytes())
    assert e.value.reason == "progressive"
    data, rgb = _valid("geo_420_37x19")
    np.testing.assert_array_equal(np.asarray(dec.decode_or_host(data, "bgr")), rgb[:, :, ::-1])
    assert dec.fallbacks == 0
    try:
        import PIL  # noqa: F401
    except ImportError:                                  # no host decoder here: the fallback has nothing to fall back to
        with pytest.raises(ImportError):
            dec.decode_or_host(MALFORMED["progressive.file"].tobytes())
    else:
        pix = dec.decode_or_host(MALFORMED["progressive.file"].tobytes())
        assert dec.fallbacks == 1 and pix.shape == (16, 16, 3)
    dec.close()


MALFORMED_GROUPS = {
    "cut": [n for n in MALFORMED_NAMES if n.startswith("cut_")],
    "restart": [n for n in MALFORMED_NAMES if n.startswith(("rst_", "interval_"))],
    "symbols": ["bad_code", "run_past_63", "zrl_past_63"],
    "header": ["progressive", "sof_411", "sof_12bit", "sof_4_components", "dqt_16bit", "sos_ns_1"],
}


def test_every_malformed_file_is_in_a_group():
    assert sorted(sum(MALFORMED_GROUPS.values(), [])) == sorted(MALFORMED_NAMES)


@pytest.mark.parametrize("group", list(MALFORMED_GROUPS))
def test_malformed_files_are_rejected_with_the_restatements_reason(handle, group):
    """TF_OK, the reason the restatement gives, the guards intact -- and a valid decode on the same handle right after
    each is still exact.  Where the header parses, the output is exactly the H x W x 3 bytes it announces and the guards
    begin right behind them; a file whose header is rejected on the host gets one pixel."""
    for name in MALFORMED_GROUPS[group]:
        data = MALFORMED[name + ".file"].tobytes()
        want = int(MALFORMED[name + ".reject"])
        assert want != 0 and JR.R[JR.verdict(data)] == want
        info = JR.probe(data)
        shape = (info["height"], info["width"], 3) if info["reject"] == "ok" else (1, 1, 3)
        rc, reject, _ = handle.decode(data, shape)
        assert rc == handle.ok, name
        assert reject == want, f"{name}: {JR.REJECT[reject] if reject < len(JR.REJECT) else reject}, not {JR.REJECT[want]}"
        assert handle.lib.tf_jpegdec_reject_name(reject).decode() == JR.REJECT[want]
        _exact(handle, "geo_420_17x9")
