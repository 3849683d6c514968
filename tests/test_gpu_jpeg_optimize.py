"""tf_jpeg in mode 1, the frame's own Huffman tables, on the GPU against libjpeg's optimize_coding
(tests/golden/jpegopt_*.npz, written by tools/capture_golden_jpeg.py, and tests/jpeg_ref.py with `optimize`): the
whole file, byte for byte, the tables and the counts behind them."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

from tests import jpeg_cases, jpeg_ref
from tests.jpeg_cases import GOLDEN, first_difference

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "jpegopt_*.npz")))


def _case(name):
    case = jpeg_cases.load_case(jpeg_cases.fixture_path("jpegopt", name))
    return case.image, case.quality, case.restart_mcus, case.jpeg


@functools.lru_cache(maxsize=None)
def _histograms(name):
    """The restatement's counts of a case: computed once, shared, never written."""
    _, _, _, quality, restart = jpeg_cases.OWN_TABLES_CASES[name]
    hist = jpeg_ref.histograms(jpeg_cases.case_image("jpegopt", name), quality, restart)
    hist.setflags(write=False)
    return hist


def test_every_case_is_here():
    assert sorted(os.path.basename(p)[8:-4] for p in FIXTURES) == sorted(jpeg_cases.OWN_TABLES_CASES)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_encoder_writes_libjpegs_optimised_file(path):
    from transflow_amd.jpeg import JpegEncoder
    image, quality, restart, _, _, expected = jpeg_cases.load_case(path)
    enc = JpegEncoder(image.shape[0], image.shape[1], quality, restart, optimize=True)
    try:
        with pytest.raises(RuntimeError):
            enc.header                                                     # the frame's: none before the first encode
        got = enc.encode(image)
        assert got == expected, first_difference(got, expected)
        assert enc.header == expected[:len(enc.header)] and expected[len(enc.header) - 14:len(enc.header) - 12] == b"\xff\xda"
    finally:
        enc.close()


@pytest.mark.parametrize("name", sorted(jpeg_cases.OWN_TABLES_CASES))
def test_last_tables_are_the_restatements(name):
    from transflow_amd.jpeg import JpegEncoder
    h, w, _, quality, restart = jpeg_cases.OWN_TABLES_CASES[name]
    enc = JpegEncoder(h, w, quality, restart, optimize=True)
    try:
        with pytest.raises(RuntimeError):
            enc.last_tables()                                              # TF_ERR_STATE: nothing encoded
        enc.encode(jpeg_cases.case_image("jpegopt", name))
        tables, counts = enc.last_tables(counts=True)
        want = _histograms(name)
        wrong = np.argwhere(counts != want)
        assert not len(wrong), f"{len(wrong)} counters differ, the first [table, symbol] {wrong[0]}: " \
                               f"{counts[tuple(wrong[0])]} against {want[tuple(wrong[0])]}"
        for t in range(4):
            assert tables[t] == jpeg_ref.gen_optimal_table(want[t]), jpeg_ref.TABLE_NAMES[t]
    finally:
        enc.close()


def test_wide_lane_is_not_cut_at_64_bits():
    """Three 16-bit ZRLs, a 16-bit code and its 6 value bits in one lane: 70 bits."""
    from transflow_amd.jpeg import JpegEncoder
    image, quality, restart, expected = _case("224x224_wide_lane")
    enc = JpegEncoder(224, 224, quality, restart, optimize=True)
    try:
        got = enc.encode(image)
        hdr = len(enc.header)
        assert got[:hdr] == expected[:hdr], "the tables differ: " + first_difference(got[:hdr], expected[:hdr])
        # block (0, 0) is the first of the scan: a cut lane shows within the first bytes behind the header
        assert got[hdr:hdr + 16] == expected[hdr:hdr + 16], first_difference(got, expected)
        assert got == expected, first_difference(got, expected)
    finally:
        enc.close()


# ---- the table stage alone ---------------------------------------------------------------------------------------------
class _Stage:
    def __init__(self):
        from transflow_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.h = C.c_void_p()
        _lib.check(self.lib.tf_jpeg_create(C.byref(self.h), 16, 16, 50, 0))

    def tables(self, counts):
        """(return code, fault word, four (bits, vals)) of uint32 (4, 257) counts."""
        counts = np.ascontiguousarray(counts, np.uint32)
        assert counts.shape == (4, 257)
        bits, vals, fault = np.full((4, 16), 0xEE, np.uint8), np.full((4, 256), 0xEE, np.uint8), C.c_uint32(0xEEEEEEEE)
        rc = self.lib.tf_jpeg_tables_from_counts(self.h, C.c_void_p(counts.ctypes.data), C.c_void_p(bits.ctypes.data),
                                                 C.c_void_p(vals.ctypes.data), C.byref(fault))
        return rc, fault.value, [(bits[t].tolist(), vals[t, :int(bits[t].astype(int).sum()) % 257].tolist()) for t in range(4)]

    def close(self):
        self.lib.tf_jpeg_destroy(self.h)


@pytest.fixture()
def stage():
    s = _Stage()
    yield s
    s.close()


def _four(*tables):
    """uint32 (4, 257) of 256-count histograms (the last repeated), entry 256 a value the library must ignore."""
    rows = list(tables) + [tables[-1]] * (4 - len(tables))
    return np.stack([np.concatenate([np.asarray(r, np.uint32)[:256], [12345]]) for r in rows]).astype(np.uint32)


@pytest.mark.parametrize("name", ["45x61", "33x47_noise_q100", "270x480_q95", "224x224_wide_lane", "1x1"])
def test_tables_from_the_restatements_counts(stage, name):
    counts = _histograms(name)
    rc, fault, tables = stage.tables(_four(*counts))
    assert (rc, fault) == (stage._lib.TF_OK, 0)
    for t in range(4):
        assert tables[t] == jpeg_ref.gen_optimal_table(counts[t]), jpeg_ref.TABLE_NAMES[t]


def test_tables_of_hand_made_counts(stage):
    one = np.zeros(256, np.uint32)
    one[0x21] = 7
    hists = [one, np.full(256, 3, np.uint32), jpeg_cases.limiting_counts(), jpeg_cases.fibonacci_counts(32)]
    rc, fault, tables = stage.tables(_four(*hists))
    assert (rc, fault) == (stage._lib.TF_OK, 0)
    for t in range(4):
        assert tables[t] == jpeg_ref.gen_optimal_table(hists[t]), t
    assert tables[1][1] == list(range(256)) and tables[1][0][8] == 1          # equal counts: symbol 255 shares the 9 bits


def test_fibonacci_counts_give_the_fault(stage):
    good = _histograms("45x61")
    for table in range(4):
        hists = [good[t] for t in range(4)]
        hists[table] = jpeg_cases.fibonacci_counts(33)
        rc, fault, _ = stage.tables(_four(*hists))
        assert rc == stage._lib.TF_ERR_STATE and fault == 1 << table
        message = stage.lib.tf_last_error().decode()
        assert jpeg_ref.TABLE_NAMES[table] in message and "32" in message, message
    rc, fault, _ = stage.tables(_four(jpeg_cases.fibonacci_counts(40)))
    assert rc == stage._lib.TF_ERR_STATE and fault == 0xF


def test_counts_without_a_symbol_are_refused(stage):
    good = _histograms("45x61")
    rc, _, _ = stage.tables(_four(np.zeros(256, np.uint32)))
    assert rc == stage._lib.TF_ERR_ARG
    rc, _, _ = stage.tables(_four(good[0], good[1], np.zeros(256, np.uint32), good[3]))
    assert rc == stage._lib.TF_ERR_ARG
    over = np.zeros(256, np.uint32)
    over[:2] = 600000000                                                  # the sum passes libjpeg's selection sentinel
    rc, _, _ = stage.tables(_four(over))
    assert rc == stage._lib.TF_ERR_ARG
    rc, fault, _ = stage.tables(_four(*good))                              # and the handle is as good as before
    assert (rc, fault) == (stage._lib.TF_OK, 0)


def test_bad_modes_are_refused(stage):
    assert stage.lib.tf_jpeg_set_optimize(stage.h, 2) == stage._lib.TF_ERR_ARG
    assert stage.lib.tf_jpeg_set_optimize(stage.h, -1) == stage._lib.TF_ERR_ARG
    assert stage.lib.tf_jpeg_set_optimize(None, 1) == stage._lib.TF_ERR_ARG
    assert stage.lib.tf_jpeg_set_optimize(stage.h, 1) == stage._lib.TF_OK
    p, n = C.c_void_p(), C.c_size_t()
    assert stage.lib.tf_jpeg_header(stage.h, C.byref(p), C.byref(n)) == stage._lib.TF_ERR_STATE
    assert stage.lib.tf_jpeg_set_optimize(stage.h, 0) == stage._lib.TF_OK
    assert stage.lib.tf_jpeg_header(stage.h, C.byref(p), C.byref(n)) == stage._lib.TF_OK
    assert C.string_at(p.value, n.value) == jpeg_ref.header(16, 16, 50, stage.lib.tf_jpeg_default_restart_mcus())


# ---- intervals, modes, state ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", [1, 3, 8, 100])
def test_gather_pass_restarts_dc_prediction_like_the_emit_pass(restart):
    from transflow_amd.jpeg import JpegEncoder
    image = jpeg_cases.stored_image(45, 61, seed=45061)
    enc = JpegEncoder(45, 61, 50, restart, optimize=True)
    try:
        want = jpeg_ref.encode(image, 50, restart, optimize=True)
        got = enc.encode(image)
        _, counts = enc.last_tables(counts=True)
        want_counts = jpeg_ref.histograms(image, 50, restart)
        assert (counts[0] == want_counts[0]).all() and (counts[2] == want_counts[2]).all(), "the DC histograms differ"
        assert (counts == want_counts).all()
        assert got == want, first_difference(got, want)
    finally:
        enc.close()
    if restart in (1, 3):                                                  # (the intervals change the DC histograms at all)
        assert (jpeg_ref.histograms(image, 50, restart)[0] != jpeg_ref.histograms(image, 50, 100)[0]).any()


def test_modes_alternate_on_one_handle():
    from transflow_amd import _lib
    from transflow_amd.jpeg import JpegEncoder
    image, quality, restart, own = _case("45x61")
    plain = jpeg_cases.load_case(jpeg_cases.fixture_path("jpeg", "45x61")).jpeg
    enc = JpegEncoder(45, 61, quality, restart)
    try:
        assert enc.encode(image) == plain
        for mode, want in ((1, own), (0, plain), (1, own), (1, own), (0, plain)):
            _lib.check(enc._lib.tf_jpeg_set_optimize(enc._h, mode))
            enc.optimize = bool(mode)
            got = enc.encode(image)
            assert got == want, f"mode {mode}: " + first_difference(got, want)
            assert enc.header == want[:len(enc.header)]
            assert enc.frame(image).optimize == bool(mode)
        _lib.check(enc._lib.tf_jpeg_set_optimize(enc._h, 1))               # the mode changed: the last file is not this mode's
        n = C.c_size_t()
        out = np.zeros(len(plain) + 64, np.uint8)
        assert enc._lib.tf_jpeg_copy_last(enc._h, C.c_void_p(out.ctypes.data), out.nbytes, C.byref(n)) == _lib.TF_ERR_STATE
    finally:
        enc.close()


def test_one_encoder_keeps_no_counts_between_images():
    from transflow_amd.jpeg import JpegEncoder
    a, quality, restart, want_a = _case("33x47_noise_q100")
    b = jpeg_cases.stored_image(33, 47, seed=5)                            # far fewer symbols: stale counts would change its tables
    want_b = jpeg_ref.encode(b, quality, restart, optimize=True)
    assert jpeg_ref.tables(a, quality, restart) != jpeg_ref.tables(b, quality, restart)
    enc = JpegEncoder(33, 47, quality, restart, optimize=True)
    try:
        assert enc.encode(a) == want_a
        got = enc.encode(b)
        assert got == want_b, first_difference(got, want_b)
        assert (enc.last_tables(counts=True)[1] == jpeg_ref.histograms(b, quality, restart)).all()
        assert enc.encode(a) == want_a
    finally:
        enc.close()


def _pillow_or_none(image, quality, restart):
    try:
        from transflow_amd.jpeg import pillow_encode
        return pillow_encode(image, quality, restart, optimize=True)
    except (ImportError, RuntimeError):
        return None


def test_grey_image_and_one_pixel_give_pillows_file():
    """A grey image: the chroma AC table holds EOB alone, the chroma DC table category 0 alone."""
    from transflow_amd.jpeg import JpegEncoder
    i, j = np.mgrid[0:40, 0:56]
    grey = np.repeat(((3 * i + 5 * j + ((i * j) >> 3)) & 255).astype(np.uint8)[..., None], 3, axis=-1)
    for image in (grey, np.array([[[200, 30, 90]]], np.uint8)):
        enc = JpegEncoder(image.shape[0], image.shape[1], 75, 4, optimize=True)
        try:
            want = jpeg_ref.encode(image, 75, 4, optimize=True)
            got = enc.encode(image)
            assert got == want, first_difference(got, want)
            tables = enc.last_tables()
            if image.shape[0] > 1:
                assert tables[3] == ([1] + [0] * 15, [0x00]) and tables[2] == ([1] + [0] * 15, [0])
            pillow = _pillow_or_none(image, 75, 4)
            assert pillow is None or got == pillow
        finally:
            enc.close()


def test_a_buffer_one_byte_short_is_refused_and_left_alone():
    from transflow_amd import _lib
    from transflow_amd.jpeg import JpegEncoder
    image, quality, restart, expected = _case("33x47_noise_q100")
    enc = JpegEncoder(33, 47, quality, restart, optimize=True)
    try:
        guard = 64
        buf = np.full(len(expected) + guard, 0xA5, np.uint8)
        _lib.profile(True, "jpeg_")
        try:
            for capacity in (len(expected) - 1, 0, 10, 300, len(expected) // 2):
                with pytest.raises(ValueError):
                    enc.encode_into(image, buf[:capacity])
                assert enc.last_needed == len(expected)                    # the library says what it takes
                assert (buf == 0xA5).all()                                 # nothing written, within or beyond
            report = _lib.profile_report()
            encodes = report["jpeg_emit"][0]
            n = C.c_size_t()
            rc = enc._lib.tf_jpeg_copy_last(enc._h, C.c_void_p(buf.ctypes.data), len(expected) - 1, C.byref(n))
            assert rc == _lib.TF_ERR_ARG and n.value == len(expected) and (buf == 0xA5).all()
            _lib.check(enc._lib.tf_jpeg_copy_last(enc._h, C.c_void_p(buf.ctypes.data), len(expected), C.byref(n)))
            report = _lib.profile_report()
        finally:
            _lib.profile(False)
        assert report["jpeg_emit"][0] == encodes == report["jpeg_gather"][0] == report["jpeg_tables"][0]   # no second encode
        assert n.value == len(expected) and buf[:n.value].tobytes() == expected and (buf[len(expected):] == 0xA5).all()
        buf[:] = 0xA5
        assert enc.encode_into(image, buf[:len(expected)]) == len(expected)
        assert buf[:len(expected)].tobytes() == expected and (buf[len(expected):] == 0xA5).all()
    finally:
        enc.close()


def test_a_file_larger_than_the_encoders_buffer_is_copied_again():
    from transflow_amd.jpeg import JpegEncoder
    image, quality, restart, expected = _case("33x47_noise_q100")
    enc = JpegEncoder(33, 47, quality, restart, optimize=True)
    try:
        enc._out = np.zeros(700, np.uint8)                                 # far too small
        assert enc.encode(image) == expected
        assert enc._out.nbytes == len(expected)
    finally:
        enc.close()


def test_one_lane_tables_kernel_builds_the_same_tables(monkeypatch):
    """k_jpeg_tables without its wave reductions (the form it was measured against) is the same rule."""
    from transflow_amd.jpeg import JpegEncoder
    monkeypatch.setenv("TF_JPEG_TABLES_ONE_LANE", "1")
    image, quality, restart, expected = _case("224x224_wide_lane")
    enc = JpegEncoder(224, 224, quality, restart, optimize=True)
    try:
        got = enc.encode(image)
        assert got == expected, first_difference(got, expected)
    finally:
        enc.close()


def test_device_decoder_reads_the_optimised_file():
    from transflow_amd.jpeg import JpegEncoder
    from transflow_amd.jpegdec import JpegDecoder
    image, quality, restart, expected = _case("45x61")
    plain = jpeg_cases.load_case(jpeg_cases.fixture_path("jpeg", "45x61")).jpeg
    enc, dec = JpegEncoder(45, 61, quality, restart, optimize=True), JpegDecoder(61, 45)
    try:
        frame = enc.frame(image)
        assert frame.data == expected and frame.optimize
        np.testing.assert_array_equal(np.asarray(dec.decode(frame.data, "rgb")), np.asarray(dec.decode(plain, "rgb")))
    finally:
        enc.close()
        dec.close()


# ---- the compositor returns the file -------------------------------------------------------------------------------------
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


def _render_all(layers, device_flows, **options):
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    rng = np.random.default_rng(1)
    comp = HipCompositor.from_args(H, W, [LayerConfig(i, classname=c) for i, c in enumerate(layers)],
                                   background_color="#204060", **options)
    masks = [np.ones((H, W), bool), np.zeros((H, W), bool)]
    masks[1][H // 3:, 5:W // 2] = True
    comp.set_sources({i: [_HostSource(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), masks[i])] for i in range(len(layers))})
    out = []
    try:
        for flow in _flows(4, device_flows):
            comp.update(flow)
            frame = comp.render()
            out.append(frame if options else np.array(frame))              # (a raw frame is the pool's array: copy)
    finally:
        comp.close()
    return out


@pytest.mark.parametrize("layers,device_flows", [(["moveref", "sum"], False), (["moveref"], True)],
                         ids=["two_layers", "deferred_single_layer"])
def test_compositor_returns_the_optimised_file_of_its_plain_render(layers, device_flows):
    from transflow_amd.jpeg import JpegFrame
    from transflow_amd.output import default_restart_mcus
    plain = _render_all(layers, device_flows)
    files = _render_all(layers, device_flows, jpeg_frames=50, jpeg_optimize=True)
    assert (plain[0] != plain[-1]).any()
    for t, (frame, raw) in enumerate(zip(files, plain)):
        assert isinstance(frame, JpegFrame) and frame.shape == (H, W, 3) and frame.quality == 50 and frame.optimize
        assert frame.restart_mcus == default_restart_mcus()
        want = jpeg_ref.encode(raw, 50, frame.restart_mcus, optimize=True)
        assert frame.data == want, f"frame {t}: " + first_difference(frame.data, want)
        assert len(want) < len(jpeg_ref.encode(raw, 50, frame.restart_mcus))


def test_jpeg_optimize_without_jpeg_frames_raises():
    from transflow_amd.compositor import HipCompositor
    with pytest.raises(ValueError):
        HipCompositor(H, W, [], jpeg_optimize=True)
    with pytest.raises(ValueError):
        HipCompositor.from_args(H, W, [], jpeg_optimize=True)
    comp = HipCompositor(H, W, [], jpeg_frames=50, jpeg_optimize=True)
    state = comp.__getstate__()
    again = HipCompositor.__new__(HipCompositor)
    again.__setstate__(state)
    assert again.jpeg_optimize and again.jpeg_frames == 50
