"""The banded-PNG decoder without a GPU: the index in the encoder's format, the Python restatement
(tests/pngdec_ref.py) against Pillow over the corpus (tests/pngdec_cases.py), tf_pngdec_probe -- host code of the
library, called through ctypes -- against the restatement, the shared headers under the sanitizers in a stand-alone
program (tools/pngdec_host_check.cpp), and what the corpus reaches."""
import io
import os
import shutil
import subprocess
import zlib

import numpy as np
import PIL.Image
import pytest

from tests.helpers import build_host_check
from tests import png_ref as P
from tests import pngdec_cases as K
from tests import pngdec_ref as D
from transflow_amd import pngdec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pngdec_corpus.npz")


def pillow(data: bytes) -> np.ndarray:
    return np.array(PIL.Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("name", ["1x1", "7x1", "24x40_noise_b3", "9x50_black_b3", "40x300_smear", "4x85_tail_b2", "1x523_edges"])
def test_index_in_the_encoders_format(name):
    """A png_ref.encode file with tfBX put in: Pillow's pixels are the image, every chunk's CRC holds, zlib takes the
    concatenated IDATs, and the library's walk reads the index back; without the index the file is png_ref.encode's,
    byte for byte, and the walk says that it has none."""
    image, band_rows = P.case(name)
    plain = P.encode(image, band_rows)
    rows = min(image.shape[0], band_rows if band_rows else P.default_band_rows(*image.shape[:2]))
    data = D.with_index(plain, rows)
    assert data[:33] == plain[:33] and data[33 + 24:] == plain[33:] and len(data) == len(plain) + 24
    np.testing.assert_array_equal(pillow(data), image)
    chunks = P.chunks(data)
    assert all(zlib.crc32(kind + payload) == crc for kind, payload, crc in chunks)
    assert [kind for kind, _, _ in chunks[:3]] == [b"IHDR", b"tfBX", b"IDAT"]
    assert zlib.decompress(b"".join(p for kind, p, _ in chunks if kind == b"IDAT")) == P.filtered(image)
    info = pngdec.probe(data)
    assert info.indexed and (info.height, info.width, info.band_rows, info.n_bands) == (*image.shape[:2], rows, -(-image.shape[0] // rows))
    assert [n for _, n in info.bands] == [len(p) for kind, p, _ in chunks if kind == b"IDAT"][1:-1]
    without = pngdec.probe(plain)
    assert not without.indexed and without.why_not == "no_index"


@pytest.mark.parametrize("name", sorted(K.valid()))
def test_restatement_decodes_to_pillows_pixels(name):
    data, image = K.valid()[name]
    np.testing.assert_array_equal(pillow(data), image)
    np.testing.assert_array_equal(D.decode(data), image)
    # every band inflates alone, in zlib's eyes too
    lay = D.walk(data)
    for band, (off, size) in enumerate(lay.bands):
        want = min(lay.band_rows, lay.height - band * lay.band_rows) * (1 + 3 * lay.width)
        assert D.U.zlib_accepts(data[off:off + size], want) is not None, band


def _verdict(fn, data):
    try:
        return fn(data), None
    except (D.Rejected, pngdec.PngRejected) as err:
        return None, (err.reason, err.where)


def test_probe_agrees_with_the_restatement_on_the_corpus():
    """tf_pngdec_probe (no GPU) and tests/pngdec_ref.walk: the same class, geometry, bands and reasons for every file."""
    files = {"valid." + k: v[0] for k, v in K.valid().items()}
    files.update({"host." + k: v[0] for k, v in K.host().items()})
    files.update({"bound." + k: v[0] for k, v in K.bound().items()})
    files.update({"bad." + k: v[0] for k, v in K.malformed().items()})
    for name, data in files.items():
        lay, why = _verdict(D.walk, data)
        info, reason = _verdict(pngdec.probe, data)
        assert why == reason, name
        if lay is not None:
            assert (info.indexed, info.why_not, info.width, info.height, info.band_rows, info.n_bands, info.bands, info.max_band_bytes) == \
                (lay.indexed, lay.why_not, lay.width, lay.height, lay.band_rows, lay.n_bands, lay.bands, lay.max_band_bytes), name
    for name, (data, why_not) in K.host().items():
        assert pngdec.probe(data).why_not == why_not, name
    for name, (data, image) in K.bound().items():
        info = pngdec.probe(data)
        assert info.indexed and not info.within_bound, name
        np.testing.assert_array_equal(D.decode(data), image)
    assert all(pngdec.probe(data).within_bound for data, _ in K.valid().values())


@pytest.mark.parametrize("name", sorted(K.malformed()))
def test_malformed_cases_are_rejected_for_their_reason(name):
    data, reason, where, at_walk = K.malformed()[name]
    if at_walk:
        with pytest.raises(pngdec.PngRejected) as err:
            pngdec.probe(data)
        assert (err.value.reason, err.value.where) == (reason, None)
        with pytest.raises(D.Rejected) as ref:
            D.walk(data)
        assert ref.value.reason == reason
    else:
        assert pngdec.probe(data).indexed and D.walk(data).indexed     # only the decoder can tell
        with pytest.raises(D.Rejected) as ref:
            D.decode(data)
        assert (ref.value.reason, ref.value.where) == (reason, where)
        assert pngdec.reject_name(ref.value.word) == reason


def test_reject_names_are_the_librarys():
    for name, number in D.REJECT_NUMBER.items():
        assert pngdec.reject_name(number) == name == pngdec.REJECT_NAMES[number]
        assert pngdec.reject_name(number | (5 << 8)) == name
    assert sorted(pngdec.REJECT_NAMES) == sorted(D.REJECT_NAME)


def _build_host_check(tmp_path):
    """tools/pngdec_host_check.cpp, with the sanitizers where they run here: (program, sanitized)."""
    return build_host_check(tmp_path, "pngdec_host_check.cpp")


def _run_host_check(tmp_path, lines):
    """The host-check program run over the listed files: its output, after no sanitizer report.  The verdicts and
    images it prints are held to the restatement by the caller whether or not the sanitizers could be linked."""
    program, sanitized = _build_host_check(tmp_path)
    print("sanitized" if sanitized else "not sanitized: the sanitizer runtime does not link here")
    listing = tmp_path / "list.txt"
    listing.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([program, str(listing)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    return run.stdout


def test_host_check_program(tmp_path):
    """tools/pngdec_host_check.cpp -- the walk, the machine and the unfilter arithmetic of the shared headers, every
    buffer a heap block of the size the decoder is entitled to -- over the whole corpus: no sanitizer report, and every
    verdict, every geometry and every decoded image the restatement's."""
    assert pngdec.probe(K.valid()["enc.1x1"][0]).indexed
    files = {"valid." + k: v[0] for k, v in K.valid().items()}
    files.update({"host." + k: v[0] for k, v in K.host().items()})
    files.update({"bound." + k: v[0] for k, v in K.bound().items()})
    files.update({"bad." + k: v[0] for k, v in K.malformed().items()})
    lines, want = [], {}
    for i, (name, data) in enumerate(files.items()):
        path = tmp_path / f"case_{i}.png"
        path.write_bytes(data)
        lines.append(f"{name} {path}")
        try:
            lay = D.walk(data)
            if lay.indexed:
                crc = zlib.crc32(np.ascontiguousarray(D.decode(data)).tobytes())
            else:
                crc = 0
            want[name] = (0, int(lay.indexed), D.WHY_NOT.index(lay.why_not), lay.width, lay.height, lay.band_rows, lay.n_bands, crc)
        except D.Rejected as err:
            want[name] = (err.word,)
    got = {}
    for line in _run_host_check(tmp_path, lines).splitlines():
        name, *values = line.split()
        values = tuple(int(v) for v in values)
        got[name] = values if values[0] == 0 else values[:1]
    assert len(got) == len(want)
    wrong = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
    assert not wrong, sorted(wrong.items())[:10]


def test_the_corpus_reaches_what_the_kernels_must_handle():
    assert pngdec.REJECT_NAMES[0] == "ok"
    t = D.Trace()
    for data, _ in K.valid().values():
        D.decode(data, t)
    five = {0, 1, 2, 3, 4}
    assert t.types == five and t.row0_types == five and t.band_first_types == five
    assert t.paeth_picks == {"a", "b", "c"}
    assert t.paeth_ties == {"pa=pb", "pb=pc", "pa=pc", "all"}
    assert t.average_overflow and t.sub_wrap and t.up_wrap
    assert 1 in t.segments and max(t.segments) > 2 * D.MARCH_ROWS
    assert {D.MARCH_ROWS - 1, D.MARCH_ROWS, D.MARCH_ROWS + 1} <= t.segments
    assert t.max_band_bytes > D.RING_BYTES and t.max_distance > D.RING_BYTES - 258
    assert t.stored_bands > 0
    assert any(h == 1 for h, _ in t.shapes) and any(w == 1 for _, w in t.shapes)
    assert {w for _, w in t.shapes} >= {1, 2, 3, 4, 21, 22, 85, 86, 341, 342, 700}


def test_golden_files_decode_to_their_pixels():
    """tests/golden/pngdec_corpus.npz (tools/capture_golden_pngdec.py): files recorded once, so that what the decoders
    are held to does not move with the zlib that builds the corpus."""
    golden = np.load(GOLDEN)
    names = [str(n) for n in golden["names"]]
    assert len(names) >= 8
    for i, name in enumerate(names):
        data = golden[f"file_{i}"].tobytes()
        assert pngdec.probe(data).indexed, name
        np.testing.assert_array_equal(D.decode(data), golden[f"image_{i}"], err_msg=name)
        np.testing.assert_array_equal(pillow(data), golden[f"image_{i}"], err_msg=name)


# ---- routing (no GPU call: a provider's constructor walks chunks only) ------------------------------------------------------
@pytest.fixture
def sequence_path(tmp_path):
    for k, name in enumerate(("zlib.40x24_random_b5", "zlib.40x24_paeth_b5", "zlib.40x24_none_b5"), 1):
        (tmp_path / ("%05d.png" % k)).write_bytes(K.valid()[name][0])
    return str(tmp_path / "%05d.png")


def test_dropin_routes_png_sequences_only_on_request(sequence_path, tmp_path):
    from transflow_amd import dropin
    from transflow_amd.flow import HipFlowSource
    from transflow_amd.pixmap import HipPngSequencePixmapSource
    assert pngdec.is_png_sequence(sequence_path)
    still = str(tmp_path / "00001.png")
    for other in (still, str(tmp_path / "missing_%05d.png"), str(tmp_path / "%05d.jpg"), "clip.mp4", 3):
        assert not pngdec.is_png_sequence(other)

    def flow_holder(**options):
        class Ref:
            from_args = dropin._flow_from_args(lambda *a, **k: "the reference's", **options)
        return Ref

    builder = flow_holder(png_inputs=True).from_args(sequence_path)
    assert isinstance(builder, HipFlowSource.Builder) and isinstance(builder.provider_arg, pngdec.PngSequenceFrameProvider)
    assert (builder.provider_arg.width, builder.provider_arg.height, builder.provider_arg.frame_count) == (40, 24, 3)
    assert flow_holder().from_args(sequence_path).provider_arg == sequence_path          # without it: a path for cv2, as before
    assert flow_holder(mjpeg_inputs=True).from_args(sequence_path).provider_arg == sequence_path
    assert flow_holder(png_inputs=True).from_args("clip.mp4").provider_arg == "clip.mp4"

    def pixmap_holder(**options):
        class Ref:
            from_args = dropin._pixmap_from_args(lambda *a, **k: "the reference's", **options)
        return Ref

    routed = pixmap_holder(stills=False, png_inputs=True).from_args(sequence_path, (40, 24), seek=1, repeat=2)
    assert isinstance(routed, HipPngSequencePixmapSource) and (routed.seek, routed.repeat) == (1, 2)
    assert pixmap_holder(stills=False).from_args(sequence_path, (40, 24)) == "the reference's"
    assert pixmap_holder(stills=False, mjpeg_inputs=True).from_args(sequence_path, (40, 24)) == "the reference's"
    assert pixmap_holder(stills=False, png_inputs=True).from_args(still, (40, 24)) == "the reference's"     # one still image


def test_index_option_reaches_the_compositor_and_pickles():
    import pickle

    from transflow_amd.compositor import HipCompositor
    assert pngdec.MAX_BAND_BYTES == 1 << 20 and pngdec.max_band_compressed(100) == 1224
    for arg, frames, index in ((False, False, False), (True, True, False), ("indexed", True, True)):
        comp = HipCompositor(24, 40, [], png_frames=arg)
        assert (comp.png_frames, comp.png_index) == (frames, index)
        again = pickle.loads(pickle.dumps(comp))
        assert (again.png_frames, again.png_index) == (frames, index)
