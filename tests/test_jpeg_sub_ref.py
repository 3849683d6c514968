"""The restatement of libjpeg's encoder at 4:4:4, 4:2:2 and 4:2:0 (tests/jpeg_sub_ref.py) against Pillow on this machine
and against libjpeg's own files in tests/golden/jpegsub_*.npz.  No GPU."""
import glob
import inspect
import os

import numpy as np
import pytest

from tests import jpeg_optimize_ref, jpeg_ref, jpeg_sub_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "jpegsub_*.npz")))


def _pillow_with_restart():
    try:
        import PIL.JpegImagePlugin as plugin
    except ImportError:
        return False
    return "restart_marker_blocks" in inspect.getsource(plugin._save)


needs_pillow_restart = pytest.mark.skipif(not _pillow_with_restart(), reason="no Pillow with restart_marker_blocks")


def _images(size):
    return (("noise", jpeg_sub_ref.noise_image(*size, seed=size[0] * 100 + size[1])), ("smooth", jpeg_sub_ref.smooth_image(*size)))


@needs_pillow_restart
@pytest.mark.parametrize("optimize", [False, True], ids=["annex_k", "optimize"])
@pytest.mark.parametrize("subsampling", [0, 1, 2], ids=["444", "422", "420"])
@pytest.mark.parametrize("size", jpeg_sub_ref.GRID_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_live_pillow(size, subsampling, optimize):
    """11 sizes x 2 images x 4 qualities x 3 intervals x 3 layouts, and again with the frame's own tables."""
    from transflow_amd.jpeg import pillow_encode
    for kind, image in _images(size):
        for quality in jpeg_sub_ref.GRID_QUALITIES:
            for restart in jpeg_sub_ref.GRID_INTERVALS:
                expected = pillow_encode(image, quality, restart, optimize=optimize, subsampling=subsampling)
                got = jpeg_sub_ref.encode(image, quality, restart, subsampling, optimize)
                assert got == expected, (kind, quality, restart)


@pytest.mark.parametrize("size", [(9, 17), (23, 41)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_420_is_jpeg_refs(size):
    """At subsampling 2 the module says what tests/jpeg_ref.py and tests/jpeg_optimize_ref.py say."""
    image = jpeg_sub_ref.noise_image(*size, seed=3)
    for restart in (1, 3):
        assert jpeg_sub_ref.encode(image, 90, restart, 2) == jpeg_ref.encode(image, 90, restart)
        assert jpeg_sub_ref.encode(image, 90, restart, 2, optimize=True) == jpeg_optimize_ref.encode(image, 90, restart)
        np.testing.assert_array_equal(jpeg_sub_ref.histograms(image, 90, restart, 2), jpeg_optimize_ref.histograms(image, 90, restart))


def test_header_changes_one_byte():
    base = jpeg_ref.header(23, 41, 50, 3)
    for sub, byte in ((0, 0x11), (1, 0x21), (2, 0x22)):
        head = jpeg_sub_ref.header(23, 41, 50, 3, sub)
        diff = [i for i in range(len(base)) if base[i] != head[i]]
        assert len(head) == len(base) and (diff == [] if sub == 2 else len(diff) == 1 and head[diff[0]] == byte)


def test_trace_accounts_for_the_file():
    """The trace's per-MCU bits and flushed bytes are the scan: MCUs of the layout's size, dummy blocks included."""
    image = jpeg_sub_ref.noise_image(23, 41, seed=5)
    for sub, n_mcus in ((0, 3 * 6), (1, 3 * 3), (2, 2 * 3)):
        for optimize in (False, True):
            t = jpeg_sub_ref.trace(image, 90, 5, sub, optimize)
            assert t.data == jpeg_sub_ref.encode(image, 90, 5, sub, optimize)
            assert len(t.mcu_bits) == len(t.flushed) == n_mcus
            assert [i for i, end in enumerate(t.interval_end) if end] == sorted(set(range(4, n_mcus, 5)) | {n_mcus - 1})
            scan = t.data[t.data.index(b"\xff\xda") + 14:-2]
            for k in range(8):                                             # (a data 0xFF is followed by 0x00, never by RSTn)
                scan = scan.replace(bytes([0xFF, 0xD0 + k]), b"")
            assert b"".join(t.flushed) == scan.replace(b"\xff\x00", b"\xff")
    # a 4:2:2 MCU of an 8-wide image has a dummy second block: two luma DC symbols per MCU, the second category 0
    t = jpeg_sub_ref.trace(jpeg_sub_ref.smooth_image(8, 8), 50, 4, 1)
    assert len(t.mcu_bits) == 1 and 0 in t.dc_categories[0]


def test_every_case_has_its_fixtures():
    names = sorted(jpeg_sub_ref.fixture_name(name, sub) for name in jpeg_sub_ref.CASES for sub in (0, 1))
    assert sorted(os.path.basename(p) for p in FIXTURES) == names
    for path in FIXTURES:
        assert os.path.getsize(path) < 16384                              # recipes, not pixels


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_restatement_equals_libjpegs_file(path):
    image, quality, restart, sub, optimize, expected = jpeg_sub_ref.load_case(path)
    got = jpeg_sub_ref.encode(image, quality, restart, sub, optimize)
    assert got == expected


def test_fixtures_exercise_what_they_are_for():
    def load(name, sub):
        return jpeg_sub_ref.load_case(os.path.join(GOLDEN, jpeg_sub_ref.fixture_name(name, sub)))

    def scan(name, sub):
        data = load(name, sub)[5]
        return data[data.index(b"\xff\xda") + 14:-2]
    for sub in (0, 1):
        assert b"\xff\x00" in scan("33x47_noise_q100", sub)                # byte stuffing
        wrapped = scan("40x72_r1", sub)                                    # RSTn wraps
        n = (5 * 9 if sub == 0 else 5 * 5) - 1
        assert sum(wrapped.count(bytes([0xFF, 0xD0 + k])) for k in range(8)) == n and n > 8
        image, quality, restart = load("33x47_binary_q10", sub)[:3]
        assert 0xF0 in jpeg_sub_ref.trace(image, quality, restart, sub).ac_symbols[0]     # ZRLs
        # the fattest MCU pair of the quality-100 noise is more than one trip of the flush (64 bytes) ...
        image, quality, restart = load("33x47_noise_q100", sub)[:3]
        t = jpeg_sub_ref.trace(image, quality, restart, sub)
        assert max(t.mcu_bits) > 64 * 8
        # ... and intervals of 3 and 5 MCUs end on an odd MCU count
        assert restart % 2 == 1
