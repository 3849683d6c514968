"""The restatement of the PNG encoder's mode "frame" (tests/png_frame_code_ref.py) against Pillow's decoder, zlib and
the restatement of the device's decoder, the cases' reach by its own trace, the golden files, and the host side of the
option: PngEncoder's argument, the compositor's state, the drop-in's routing.  No GPU."""
import glob
import io
import os
import pickle
import zlib

import numpy as np
import pytest

from tests import flowzip_ref as Z
from tests import png_frame_code_ref as F
from tests import png_ref as P
from tests import pngdec_ref as D
from tests.test_png_ref import stub_transflow  # noqa: F401  (the fixture: stubs of the two classes the drop-in patches)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = list(F.CASES)

_traced = {}


def _trace(name):
    """(image, band_rows, trace, the indexed file): made once."""
    if name not in _traced:
        image, band_rows = F.case(name)
        image.setflags(write=False)
        t = F.trace(image, band_rows)
        _traced[name] = (image, band_rows, t, D.with_index(t.data, t.band_rows))
    return _traced[name]


def _decode(data: bytes) -> np.ndarray:
    import PIL.Image
    with PIL.Image.open(io.BytesIO(data)) as im:
        assert im.mode == "RGB"
        return np.asarray(im)


# ---- the file -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_file_holds_the_pixels_and_is_no_larger_than_the_fixed_codes(name):
    image, band_rows, t, indexed = _trace(name)
    np.testing.assert_array_equal(_decode(t.data), image)
    chunks = P.chunks(t.data)
    assert [k for k, _, _ in chunks] == [b"IHDR"] + [b"IDAT"] * (t.bands + 2) + [b"IEND"]
    for kind, payload, crc in chunks:
        assert crc == zlib.crc32(kind + payload)
    idat = [p for k, p, _ in chunks if k == b"IDAT"]
    assert idat[0] == b"\x78\x01" and idat[-1][:5] == b"\x01\x00\x00\xff\xff" and len(idat[-1]) == 9
    stream = P.filtered(image)
    assert zlib.decompress(b"".join(idat)) == stream                      # which also checks the Adler-32
    at = 0
    for n, band, stored, size in zip(t.band_bytes, idat[1:-1], t.band_stored, t.band_sizes):
        inflater = zlib.decompressobj(wbits=-15)                           # a band alone is a deflate stream that has not ended
        assert inflater.decompress(band) == stream[at:at + n] and not inflater.eof
        assert len(band) == size
        if stored:
            assert band == Z.stored_band(np.frombuffer(stream[at:at + n], np.uint8)) and size == Z.stored_bytes(n)
        else:
            assert band[-4:] == b"\x00\x00\xff\xff" and size < Z.stored_bytes(n)
        at += n
    assert at == len(stream)
    fixed = P.encode(image, band_rows)
    print(f"{name}: {len(t.data)} bytes, the fixed code's {len(fixed)}, raw {image.size}")
    assert len(t.data) <= len(fixed)
    assert len(t.data) <= P.file_bound(image.shape[0], image.shape[1], band_rows)      # the staging slots are unchanged


@pytest.mark.parametrize("name", NAMES)
def test_the_decoders_restatement_reads_the_indexed_file(name):
    image, band_rows, t, indexed = _trace(name)
    assert indexed == F.encode(image, band_rows, index=True)
    np.testing.assert_array_equal(D.decode(indexed), image)


def test_the_code_is_the_histograms():
    """Complete over the used symbols, nothing for the others, at most 15 bits; the histogram counts what is coded."""
    for name in NAMES:
        image, band_rows, t, _ = _trace(name)
        used = [n for n in t.lengths if n]
        assert [n > 0 for n in t.lengths] == [c > 0 for c in t.histogram] and max(used) <= 15
        assert sum(2.0 ** -n for n in used) == 1.0, name
        assert t.histogram[256] == t.bands
        assert (t.lengths, t.repairs) == tuple(Z.build_lengths(t.histogram))
        literals = sum(t.histogram[:256])
        assert literals + t.bands <= sum(t.band_bytes) + t.bands and (t.matches > 0) == (literals < sum(t.band_bytes))


# ---- what the cases reach, by the restatement's own account ---------------------------------------------------------------
def test_cases_reach_coded_and_stored_bands_in_one_frame():
    t = _trace("8x700_stripes_b1")[2]
    assert t.band_stored == [True, False] * 4                              # noise rows stored, flat rows coded
    assert t.stored_blocks == [1] * 4
    t = _trace("2x21841_noise_b2")[2]
    assert t.band_bytes == [131048] and t.band_stored == [True] and t.stored_blocks == [2]
    assert t.band_sizes == [131048 + 10]
    for name in P.NOISE_CASES:                                             # the header outweighs a small or a noisy band
        assert all(_trace(name)[2].band_stored), name
    for name in ("9x50_black_b3", "1x6000_ramp", "runs_3_to_258", "40x300_smear", "1x523_edges", "sweep_a", "sweep_b", "sweep_c"):
        assert not any(_trace(name)[2].band_stored), name


def test_cases_reach_a_repaired_code():
    image, band_rows, t, _ = _trace("1x15455_fibonacci")
    assert image.shape == (1, 15455, 3) and set(np.unique(image)) == set(range(1, 23))
    assert t.repairs >= 1 and max(t.lengths) <= 15 and t.band_stored == [False]
    assert max(Z.huffman_lengths(t.histogram)) > 15                        # the unrepaired code is too deep
    print(f"fibonacci: filter {t.filter_types}, repairs {t.repairs}, longest code {max(t.lengths)}")


def test_cases_reach_no_match_unused_symbols_and_many_bands():
    assert _trace("1x4099_noise")[2].matches == 0 and not any(_trace("1x4099_noise")[2].lengths[257:])
    assert _trace("1x1")[2].matches == 0 and sum(1 for n in _trace("1x1")[2].lengths if n) <= 5
    t = _trace("40x300_smear")[2]
    assert not any(t.band_stored) and 0 in t.lengths[:256] and 0 in t.lengths[257:] and any(t.lengths[257:])
    assert _trace("1025x1_b1")[2].bands == 1025 > P.SCAN_CHUNK
    assert _trace("2049x2_b1")[2].bands == 2049 > 2 * P.SCAN_CHUNK
    t = _trace("runs_3_to_258")[2]
    assert all(t.lengths[257:])                                            # every length symbol coded


# ---- the regression pin ---------------------------------------------------------------------------------------------------
def test_golden_files_are_the_restatements():
    """tools/capture_golden_png_frame_code.py wrote them: per small case its parameters, file, code and bands."""
    fixtures = sorted(glob.glob(os.path.join(GOLDEN, "png_fc_*.npz")))
    assert sorted(os.path.basename(p)[7:-4] for p in fixtures) == sorted(F.GOLDEN_CASES)
    for path in fixtures:
        assert os.path.getsize(path) < (1 << 20)
        with np.load(path) as z:
            name = str(z["name"])
            image, band_rows, t, _ = _trace(name)
            assert (int(z["height"]), int(z["width"]), int(z["band_rows"])) == (image.shape[0], image.shape[1], band_rows)
            assert z["png"].tobytes() == t.data, name
            assert z["lengths"].tolist() == t.lengths and int(z["repairs"]) == t.repairs
            assert z["band_sizes"].tolist() == t.band_sizes and z["band_stored"].tolist() == t.band_stored


# ---- the option's host side -------------------------------------------------------------------------------------------------
def test_compositor_keeps_the_code_as_plain_state():
    from transflow_amd.compositor import HipCompositor
    comp = HipCompositor(8, 8, [], png_frames="indexed", png_code="frame")
    back = pickle.loads(pickle.dumps(comp))
    assert (back.png_frames, back.png_index, back.png_code, back._png) == (True, True, "frame", None)
    assert pickle.loads(pickle.dumps(HipCompositor(8, 8, [], png_frames=True))).png_code == "fixed"
    state = comp.__getstate__()
    del state["png_code"]                                                  # a state from before the option
    old = HipCompositor.__new__(HipCompositor)
    old.__setstate__(state)
    assert old.png_code == "fixed" and old.png_frames is True
    assert HipCompositor.from_args(8, 8, [], png_frames=True, png_code="frame").png_code == "frame"
    with pytest.raises(ValueError):
        HipCompositor(8, 8, [], png_code="frame")                          # no PNG frames to code
    with pytest.raises(ValueError):
        HipCompositor(8, 8, [], png_frames=True, png_code="best")


def test_install_passes_the_code_to_the_compositors(stub_transflow):  # noqa: F811
    from transflow_amd import dropin
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    Out, Comp = stub_transflow.VideoOutput, stub_transflow.Compositor
    out_original, comp_original = Out.__dict__["from_args"], Comp.__dict__["from_args"]
    for bad in (dict(png_code="frame"), dict(png_frames=True, png_code="best")):
        with pytest.raises(ValueError):
            dropin.install(flow=False, **bad)
        assert Out.__dict__["from_args"] is out_original and Comp.__dict__["from_args"] is comp_original
    for frames in (True, "indexed"):
        dropin.install(flow=False, png_frames=frames, png_code="frame")
        try:
            comp = Comp.from_args(8, 8, [LayerConfig(0)])
            assert isinstance(comp, HipCompositor) and comp.png_frames is True and comp.png_code == "frame"
            assert comp.png_index is (frames == "indexed")
        finally:
            dropin.uninstall()
    dropin.install(flow=False, png_frames=True)
    try:
        assert Comp.from_args(8, 8, [LayerConfig(0)]).png_code == "fixed"
    finally:
        dropin.uninstall()
    assert Out.__dict__["from_args"] is out_original and Comp.__dict__["from_args"] is comp_original
