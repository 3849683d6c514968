"""The restatement of libjpeg's encoder at 4:4:4, 4:2:2 and 4:2:0 (tests/jpeg_ref.py) against Pillow on this machine and
against libjpeg's own files in tests/golden/jpegsub_*.npz.  No GPU."""
import glob
import inspect
import os

import numpy as np
import pytest

from tests import jpeg_cases, jpeg_ref
from tests.jpeg_cases import GOLDEN

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "jpegsub_*.npz")))


def _pillow_with_restart():
    try:
        import PIL.JpegImagePlugin as plugin
    except ImportError:
        return False
    return "restart_marker_blocks" in inspect.getsource(plugin._save)


needs_pillow_restart = pytest.mark.skipif(not _pillow_with_restart(), reason="no Pillow with restart_marker_blocks")


def _images(size):
    return (("noise", jpeg_cases.noise_image(*size, seed=size[0] * 100 + size[1])), ("smooth", jpeg_cases.formula_image(*size)))


@needs_pillow_restart
@pytest.mark.parametrize("optimize", [False, True], ids=["annex_k", "optimize"])
@pytest.mark.parametrize("subsampling", [0, 1, 2], ids=["444", "422", "420"])
@pytest.mark.parametrize("size", jpeg_cases.GRID_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_live_pillow(size, subsampling, optimize):
    """11 sizes x 2 images x 4 qualities x 3 intervals x 3 layouts, and again with the frame's own tables."""
    from transflow_amd.jpeg import pillow_encode
    for kind, image in _images(size):
        for quality in jpeg_cases.GRID_QUALITIES:
            for restart in jpeg_cases.GRID_INTERVALS:
                expected = pillow_encode(image, quality, restart, optimize=optimize, subsampling=subsampling)
                got = jpeg_ref.encode(image, quality, restart, subsampling, optimize)
                assert got == expected, (kind, quality, restart)


@needs_pillow_restart
@pytest.mark.parametrize("size", [(9, 17), (23, 41)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_420_is_the_default_layout(size):
    """A call that names no layout means subsampling 2 and Annex K, and is libjpeg's file; the gather pass at subsampling
    2 counts what libjpeg's counts: the tables in a live file's DHT segments are `gen_optimal_table` of `histograms`."""
    from transflow_amd.jpeg import pillow_encode
    image = jpeg_cases.noise_image(*size, seed=3)
    for restart in (1, 3):
        plain, own = pillow_encode(image, 90, restart), pillow_encode(image, 90, restart, optimize=True)
        assert jpeg_ref.encode(image, 90, restart, 2) == jpeg_ref.encode(image, 90, restart) == plain
        assert jpeg_ref.encode(image, 90, restart, 2, optimize=True) == jpeg_ref.encode(image, 90, restart, optimize=True) == own
        hist = jpeg_ref.histograms(image, 90, restart, 2)
        np.testing.assert_array_equal(hist, jpeg_ref.histograms(image, 90, restart))
        dht = jpeg_ref.dht_tables(own)
        assert [dht[tc_th] for tc_th in (0x00, 0x10, 0x01, 0x11)] == [jpeg_ref.gen_optimal_table(h) for h in hist]


def _segments(head: bytes):
    """[(marker, first byte, one past the last)] of a header's segments behind SOI."""
    out, i = [], 2
    while i < len(head):
        n = 2 + int.from_bytes(head[i + 2:i + 4], "big")
        out.append((head[i + 1], i, i + n))
        i += n
    return out


def test_header_states_the_layout_in_one_byte_and_the_tables_in_dht():
    base = jpeg_ref.header(23, 41, 50, 3)
    (sof_first, sof_end), = [(a, b) for marker, a, b in _segments(base) if marker == 0xC0]
    for sub, byte in ((0, 0x11), (1, 0x21), (2, 0x22)):
        head = jpeg_ref.header(23, 41, 50, 3, sub)
        diff = [i for i in range(len(base)) if base[i] != head[i]]
        assert len(head) == len(base) and (diff == [] if sub == 2 else len(diff) == 1 and head[diff[0]] == byte)
        assert all(sof_first <= i < sof_end for i in diff)
        assert head[sof_first + 11] == byte                                # marker, length, precision, height, width, count, id
    # the frame's own tables change the DHT segments and nothing else
    four = jpeg_ref.tables(jpeg_cases.noise_image(23, 41, seed=3), 50, 3, 1)
    assert four != list(jpeg_ref.ANNEX_K)
    for sub in (0, 1, 2):
        annex_k, own = jpeg_ref.header(23, 41, 50, 3, sub), jpeg_ref.header(23, 41, 50, 3, sub, tables=four)
        order = [marker for marker, _, _ in _segments(annex_k)]
        assert order == [marker for marker, _, _ in _segments(own)]
        assert order == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
        for (marker, a, b), (_, c, d) in zip(_segments(annex_k), _segments(own)):
            if marker == 0xC4:
                assert annex_k[a:b] != own[c:d]
            else:
                assert annex_k[a:b] == own[c:d], hex(marker)
        assert jpeg_ref.dht_tables(own) == dict(zip((0x00, 0x10, 0x01, 0x11), four))


def test_trace_accounts_for_the_file():
    """The trace's per-MCU bits and flushed bytes are the scan: MCUs of the layout's size, dummy blocks included."""
    image = jpeg_cases.noise_image(23, 41, seed=5)
    for sub, n_mcus in ((0, 3 * 6), (1, 3 * 3), (2, 2 * 3)):
        for optimize in (False, True):
            t = jpeg_ref.trace(image, 90, 5, sub, optimize)
            assert t.data == jpeg_ref.encode(image, 90, 5, sub, optimize)
            assert len(t.mcu_bits) == len(t.flushed) == n_mcus
            assert [i for i, end in enumerate(t.interval_end) if end] == sorted(set(range(4, n_mcus, 5)) | {n_mcus - 1})
            scan = t.data[t.data.index(b"\xff\xda") + 14:-2]
            for k in range(8):                                             # (a data 0xFF is followed by 0x00, never by RSTn)
                scan = scan.replace(bytes([0xFF, 0xD0 + k]), b"")
            assert b"".join(t.flushed) == scan.replace(b"\xff\x00", b"\xff")
    # a 4:2:2 MCU of an 8-wide image has a dummy second block: two luma DC symbols per MCU, the second category 0
    t = jpeg_ref.trace(jpeg_cases.formula_image(8, 8), 50, 4, 1)
    assert len(t.mcu_bits) == 1 and 0 in t.dc_categories[0]


def test_every_case_has_its_fixtures():
    names = sorted(os.path.basename(jpeg_cases.fixture_path("jpegsub", name, sub))
                   for name in jpeg_cases.LAYOUT_CASES for sub in jpeg_cases.LAYOUT_CASE_SUBSAMPLINGS)
    assert sorted(os.path.basename(p) for p in FIXTURES) == names
    for path in FIXTURES:
        assert os.path.getsize(path) < 16384                              # recipes, not pixels


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_restatement_equals_libjpegs_file(path):
    image, quality, restart, sub, optimize, expected = jpeg_cases.load_case(path)
    got = jpeg_ref.encode(image, quality, restart, sub, optimize)
    assert got == expected


def test_fixtures_exercise_what_they_are_for():
    def load(name, sub):
        return jpeg_cases.load_case(jpeg_cases.fixture_path("jpegsub", name, sub))

    def scan(name, sub):
        data = load(name, sub)[5]
        return data[data.index(b"\xff\xda") + 14:-2]
    for sub in (0, 1):
        assert b"\xff\x00" in scan("33x47_noise_q100", sub)                # byte stuffing
        wrapped = scan("40x72_r1", sub)                                    # RSTn wraps
        n = (5 * 9 if sub == 0 else 5 * 5) - 1
        assert sum(wrapped.count(bytes([0xFF, 0xD0 + k])) for k in range(8)) == n and n > 8
        image, quality, restart = load("33x47_binary_q10", sub)[:3]
        assert 0xF0 in jpeg_ref.trace(image, quality, restart, sub).ac_symbols[0]     # ZRLs
        # the fattest MCU pair of the quality-100 noise is more than one trip of the flush (64 bytes) ...
        image, quality, restart = load("33x47_noise_q100", sub)[:3]
        t = jpeg_ref.trace(image, quality, restart, sub)
        assert max(t.mcu_bits) > 64 * 8
        # ... and intervals of 3 and 5 MCUs end on an odd MCU count
        assert restart % 2 == 1
