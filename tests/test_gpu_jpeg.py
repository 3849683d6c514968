"""tf_jpeg_* on the GPU against libjpeg's own files (tests/golden/jpeg_*.npz, written by tools/capture_golden_jpeg.py):
the whole file, byte for byte."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from tests import jpeg_cases, jpeg_ref
from tests.jpeg_cases import GOLDEN, first_difference

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "jpeg_*.npz")))


def _case(name):
    case = jpeg_cases.load_case(jpeg_cases.fixture_path("jpeg", name))
    return case.image, case.quality, case.restart_mcus, case.jpeg


def test_every_case_is_here():
    assert sorted(os.path.basename(p)[5:-4] for p in FIXTURES) == sorted(jpeg_cases.BASELINE_CASES)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[5:-4])
def test_encoder_writes_libjpegs_file(path):
    from transflow_amd.jpeg import JpegEncoder
    image, quality, restart, _, _, expected = jpeg_cases.load_case(path)
    enc = JpegEncoder(image.shape[0], image.shape[1], quality, restart)
    try:
        assert enc.header == expected[:len(enc.header)] == jpeg_ref.header(image.shape[0], image.shape[1], quality, restart)
        got = enc.encode(image)
        assert got == expected, first_difference(got, expected)
    finally:
        enc.close()


def test_default_interval_is_the_one_the_host_encodes_with():
    from transflow_amd import output
    from transflow_amd.jpeg import JpegEncoder
    image, quality, restart, expected = _case("45x61_r8")
    assert restart == output.default_restart_mcus()                       # the fixture was captured with it
    enc = JpegEncoder(45, 61, quality)
    try:
        assert enc.restart_mcus == output.default_restart_mcus()          # (read from the header's DRI segment)
        assert enc.encode(image) == expected
    finally:
        enc.close()


def test_one_encoder_keeps_no_state_between_images():
    from transflow_amd.jpeg import JpegEncoder
    a, quality, restart, want_a = _case("33x47_noise_q100")
    b = jpeg_cases.stored_image(33, 47, seed=5)                            # far fewer bits: what a stale buffer would show in
    want_b = jpeg_ref.encode(b, quality, restart)
    enc = JpegEncoder(33, 47, quality, restart)
    try:
        assert enc.encode(a) == want_a
        assert enc.encode(b) == want_b
        assert enc.encode(a) == want_a
    finally:
        enc.close()


def test_fat_mcus_leave_nothing_behind_for_the_next_image():
    """600-byte MCUs, then a flat image of a few bytes per MCU, then the first again: bits left in the LDS buffer past
    the words a small MCU zeroes, or in the staging slots, would show in the second file."""
    from transflow_amd.jpeg import JpegEncoder
    a, quality, restart, want_a = _case("32x48_binary_q100")
    b = np.empty((32, 48, 3), np.uint8)
    b[:] = (90, 160, 30)
    want_b = jpeg_ref.encode(b, quality, restart)
    assert len(want_b) - 629 < (len(want_a) - 629) // 10                    # (the header is 629 bytes of each)
    enc = JpegEncoder(32, 48, quality, restart)
    try:
        assert enc.encode(a) == want_a
        assert enc.encode(b) == want_b
        assert enc.encode(a) == want_a
    finally:
        enc.close()


def test_device_inputs_give_the_host_arrays_bytes():
    from transflow_amd.jpeg import JpegEncoder, JpegFrame
    from transflow_amd.pixmap import DevicePixmap
    from transflow_amd.remap import CompImage
    image, quality, restart, expected = _case("45x61_r3")
    enc = JpegEncoder(45, 61, quality, restart)
    pixmap = DevicePixmap.from_host(image)
    comp = CompImage(45, 61, (10, 200, 90))
    try:
        assert enc.encode(pixmap) == expected
        comp.begin()
        flat = np.empty((45, 61, 3), np.uint8)
        flat[:] = (10, 200, 90)
        assert enc.encode(comp) == jpeg_ref.encode(flat, quality, restart)
        frame = enc.frame(pixmap)
        assert isinstance(frame, JpegFrame) and frame.data == expected
        assert (frame.shape, frame.quality, frame.restart_mcus) == ((45, 61, 3), quality, restart)
        with pytest.raises(ValueError):
            enc.encode(np.zeros((45, 60, 3), np.uint8))
    finally:
        enc.close()
        pixmap.close()
        comp.close()


def test_bad_arguments_are_refused():
    from transflow_amd.jpeg import JpegEncoder
    for args in ((0, 8, 50), (8, 0, 50), (8, 8, 0), (8, 8, 101), (8, 8, 50, -1), (8, 8, 50, 65536), (70000, 8, 50)):
        with pytest.raises(ValueError):
            JpegEncoder(*args)


def test_a_buffer_one_byte_short_is_refused_and_left_alone():
    from transflow_amd.jpeg import JpegEncoder
    image, quality, restart, expected = _case("33x47_noise_q100")
    enc = JpegEncoder(33, 47, quality, restart)
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


def test_a_buffer_one_byte_short_is_refused_past_the_first_scan_chunk():
    """The same contract where k_jpeg_pack's offsets come from the second and third trips of k_slot_scan."""
    from transflow_amd.jpeg import JpegEncoder
    image, quality, restart, expected = _case("730x725_r1")
    enc = JpegEncoder(730, 725, quality, restart)
    try:
        guard = 64
        buf = np.full(len(expected) + guard, 0xA5, np.uint8)
        short = buf[:len(expected) - 1]
        with pytest.raises(ValueError):
            enc.encode_into(image, short)
        assert enc.last_needed == len(expected)                            # the library says what it takes
        assert (buf == 0xA5).all()                                         # nothing written, within or beyond
        for capacity in (0, 10, len(enc.header), len(enc.header) + 5, len(expected) // 2):
            with pytest.raises(ValueError):
                enc.encode_into(image, buf[:capacity])
            assert enc.last_needed == len(expected) and (buf == 0xA5).all()
        exact = buf[:len(expected)]
        assert enc.encode_into(image, exact) == len(expected)
        assert exact.tobytes() == expected and (buf[len(expected):] == 0xA5).all()
    finally:
        enc.close()


def test_a_file_larger_than_the_encoders_buffer_is_packed_again_not_encoded_again():
    from transflow_amd import _lib
    from transflow_amd.jpeg import JpegEncoder
    lib = _lib.load()
    image, quality, restart, expected = _case("33x47_noise_q100")
    enc = JpegEncoder(33, 47, quality, restart)
    try:
        n = C.c_size_t()
        small = np.zeros(700, np.uint8)
        rc = lib.tf_jpeg_copy_last(enc._h, C.c_void_p(small.ctypes.data), small.nbytes, C.byref(n))
        assert rc == _lib.TF_ERR_STATE                                     # nothing encoded yet
        enc._out = small                                                   # the header and 71 bytes: far too small
        _lib.profile(True, "jpeg_")
        try:
            assert enc.encode(image) == expected
            report = _lib.profile_report()
        finally:
            _lib.profile(False)
        assert report["jpeg_encode"][0] == 1 and report["jpeg_pack"][0] == 2
        assert enc._out.nbytes == len(expected) and (small[len(enc.header):] == 0).all()
        with pytest.raises(ValueError):                                    # a wrong shape is not mistaken for a short buffer
            enc.encode(np.zeros((33, 48, 3), np.uint8))
    finally:
        enc.close()


@pytest.mark.parametrize("optimize, launches", [
    (False, {"jpeg_encode": 1, "jpeg_scan": 1, "jpeg_pack": 1}),
    (True, {"jpeg_gather": 1, "jpeg_tables": 1, "jpeg_emit": 1, "jpeg_scan": 1, "jpeg_pack": 1}),
], ids=["annex_k", "own_tables"])
def test_an_encode_and_a_copy_last_launch_what_they_always_did(optimize, launches):
    """Every label and count of one encode into a buffer that is large enough, and of one tf_jpeg_copy_last: a single
    pack.  17 x 33 at the default restart length."""
    from transflow_amd import _lib
    from transflow_amd.jpeg import JpegEncoder
    image = jpeg_cases.stored_image(17, 33, seed=3)
    enc = JpegEncoder(17, 33, optimize=optimize)
    try:
        out, again, n = np.zeros(1 << 16, np.uint8), np.zeros(1 << 16, np.uint8), C.c_size_t()
        _lib.profile(True, "jpeg_")
        try:
            size = enc.encode_into(image, out)
            encode = {label: count for label, (count, _) in _lib.profile_report().items()}
            _lib.profile(True, "jpeg_")                                   # (resets the counts)
            _lib.check(enc._lib.tf_jpeg_copy_last(enc._h, C.c_void_p(again.ctypes.data), again.nbytes, C.byref(n)))
            copy = {label: count for label, (count, _) in _lib.profile_report().items()}
        finally:
            _lib.profile(False)
        assert encode == launches
        assert copy == {"jpeg_pack": 1}
        assert n.value == size and again[:size].tobytes() == out[:size].tobytes()
    finally:
        enc.close()


def _intervals(scan: bytes):
    """The scan (EOI stripped) split at its RST markers: (the intervals' bytes, the markers' low bytes).  An 0xFF of the
    entropy-coded data has an 0x00 behind it, so FF D0 .. FF D7 is a marker wherever it stands."""
    b = np.frombuffer(scan, np.uint8)
    at = np.flatnonzero((b[:-1] == 0xFF) & (b[1:] >= 0xD0) & (b[1:] <= 0xD7))
    starts, ends = np.concatenate([[0], at + 2]), np.concatenate([at, [len(b)]])
    return [scan[s:e] for s, e in zip(starts, ends)], [int(b[i + 1]) for i in at]


def test_every_interval_is_where_libjpeg_has_it_across_scan_chunks():
    """2116 intervals: k_slot_scan carries its total over two chunk boundaries and ends on a partial chunk.  Through
    the C ABI, interval by interval, so that a lost carry reads as `interval 1024`, not as a byte offset."""
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer
    lib = _lib.load()
    image, quality, restart, expected = _case("730x725_r1")
    h = C.c_void_p()
    _lib.check(lib.tf_jpeg_create(C.byref(h), 730, 725, quality, restart))
    dev = DevBuffer.from_array(image)
    try:
        out = np.full(len(expected) + 4096, 0x5A, np.uint8)
        n = C.c_size_t()
        _lib.check(lib.tf_jpeg_encode_dev(h, C.c_void_p(dev.ptr), C.c_void_p(out.ctypes.data), out.nbytes, C.byref(n)))
        got = out[:n.value].tobytes()
        hdr = len(jpeg_ref.header(730, 725, quality, restart))
        assert got[:hdr] == expected[:hdr] and got[-2:] == b"\xff\xd9"
        want_iv, want_rst = _intervals(expected[hdr:-2])
        got_iv, got_rst = _intervals(got[hdr:-2])
        assert len(want_iv) == 2116
        wrong = [i for i in range(min(len(got_iv), len(want_iv))) if got_iv[i] != want_iv[i]]
        assert len(got_iv) == len(want_iv) and not wrong, (
            f"{len(got_iv)} intervals against {len(want_iv)}; {len(wrong)} differ, the first is interval "
            f"{wrong[0] if wrong else None} (chunk {wrong[0] // 1024 if wrong else None}); "
            + first_difference(got, expected))
        assert got_rst == want_rst
        assert n.value == len(expected) and got == expected
        assert (out[n.value:] == 0x5A).all()
    finally:
        lib.tf_jpeg_destroy(h)
        dev.close()


@pytest.mark.parametrize("height,width", [(1, 65535), (65535, 1)], ids=["1x65535", "65535x1"])
def test_the_largest_sizes_the_format_has(height, width):
    """tf_jpeg_create admits the format's 65535; libjpeg stops at 65500 (JPEG_MAX_DIMENSION), where the fixtures
    1x65500 and 65500x1 are its files.  Beyond it the restatement is the reference: 4096 MCUs in a row or a column,
    512 intervals, every luma block below or beside the first a dummy."""
    from transflow_amd.jpeg import JpegEncoder
    image = jpeg_cases.formula_image(height, width)
    enc = JpegEncoder(height, width, 50)
    try:
        want = jpeg_ref.encode(image, 50, enc.restart_mcus)
        got = enc.encode(image)
        assert len(_intervals(want[len(enc.header):-2])[0]) == 512
        assert got == want, first_difference(got, want)
    finally:
        enc.close()


# ---- the compositor returns the file ------------------------------------------------------------------------------------
H, W, FRAMES = 48, 64, 3


class _HostSource:
    def __init__(self, array, introduction_mask):
        self.array, self.introduction_mask, self.counter = array, introduction_mask, -1

    def next(self, timeout=1):
        self.counter += 1
        return self.array

    @property
    def frame_number(self):
        return self.counter


def _flows(seed, device):
    from oracle import remap_ref as OR
    rng = np.random.default_rng(seed)
    flows = [OR.post_process((rng.normal(0, 2.5, (H, W, 2))).astype(np.float32), OR.BACKWARD) for _ in range(FRAMES)]
    if not device:
        return flows
    from transflow_amd.device import DevBuffer
    from transflow_amd.deviceflow import DeviceFlow, _Event
    out = []
    for f in flows:
        buf = DevBuffer.from_array(f)
        ev = _Event()
        ev.record()
        flow = DeviceFlow(f.shape, buf.ptr, ev, owner=buf)
        flow.in_frame = True                 # clipped by post_process: the one-launch step may take it
        out.append(flow)
    return out


def _render_all(layers, device_flows, jpeg_frames, deferred=None):
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    rng = np.random.default_rng(1)
    comp = HipCompositor.from_args(H, W, [LayerConfig(i, classname=c) for i, c in enumerate(layers)],
                                   background_color="#204060", jpeg_frames=jpeg_frames)
    masks = [np.ones((H, W), bool), np.zeros((H, W), bool)]
    masks[1][H // 3:, 5:W // 2] = True
    comp.set_sources({i: [_HostSource(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), masks[i])] for i in range(len(layers))})
    out = []
    try:
        for flow in _flows(4, device_flows):
            comp.update(flow)
            if deferred is not None:
                deferred.append(comp.layers[0]._deferred is not None)
            frame = comp.render()
            out.append(frame if jpeg_frames is not None else np.array(frame))   # (a raw frame is the pool's array: copy)
    finally:
        comp.close()
    return out


@pytest.mark.parametrize("layers,device_flows", [(["moveref", "sum"], False), (["moveref"], True)],
                         ids=["two_layers", "deferred_single_layer"])
def test_compositor_returns_the_file_of_its_plain_render(layers, device_flows):
    from transflow_amd.jpeg import JpegEncoder, JpegFrame
    deferred = []
    plain = _render_all(layers, device_flows, None)
    files = _render_all(layers, device_flows, 50, deferred)
    assert deferred == [device_flows] * FRAMES                             # the one-launch path is the one under test
    assert (np.array(plain[0]) != np.array(plain[-1])).any()
    enc = JpegEncoder(H, W, 50)
    try:
        for t, (frame, raw) in enumerate(zip(files, plain)):
            assert isinstance(frame, JpegFrame) and frame.shape == (H, W, 3) and frame.quality == 50
            want = enc.encode(np.array(raw))
            assert frame.data == want, f"frame {t}: " + first_difference(frame.data, want)
            assert want == jpeg_ref.encode(np.array(raw), 50, enc.restart_mcus)
    finally:
        enc.close()


def test_abi_reports_the_needed_size():
    """tf_jpeg_encode_dev itself: TF_ERR_ARG and *n_bytes for a short buffer, device pointer in."""
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer
    lib = _lib.load()
    image, quality, restart, expected = _case("17x33")
    h = C.c_void_p()
    _lib.check(lib.tf_jpeg_create(C.byref(h), 17, 33, quality, restart))
    dev = DevBuffer.from_array(image)
    try:
        out = np.full(len(expected) + 16, 0x5A, np.uint8)
        n = C.c_size_t()
        rc = lib.tf_jpeg_encode_dev(h, C.c_void_p(dev.ptr), C.c_void_p(out.ctypes.data), len(expected) - 1, C.byref(n))
        assert rc == _lib.TF_ERR_ARG and n.value == len(expected) and (out == 0x5A).all()
        rc = lib.tf_jpeg_encode_dev(h, C.c_void_p(dev.ptr), C.c_void_p(out.ctypes.data), out.nbytes, C.byref(n))
        assert rc == _lib.TF_OK and out[:n.value].tobytes() == expected and (out[n.value:] == 0x5A).all()
    finally:
        lib.tf_jpeg_destroy(h)
        dev.close()
