"""tests/jpeg_ref.py with `optimize` against libjpeg's optimize_coding (Pillow, live), the fixtures tests/golden/jpegopt_*.npz
against the restatement, `gen_optimal_table` on hand-made histograms, what the directed cases reach, and
tools/jpeg_huff_host_check.cpp -- the rule as the device runs it (transflow_amd/csrc/jpeg_huff.h) on the CPU, under the
sanitizers where they link."""
import glob
import os
import subprocess

import numpy as np
import pytest

from tests import jpeg_cases, jpeg_ref
from tests.jpeg_cases import GOLDEN, first_difference
from tests.helpers import build_host_check

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "jpegopt_*.npz")))
CASES = jpeg_cases.OWN_TABLES_CASES


def _pillow():
    PIL = pytest.importorskip("PIL")
    if tuple(int(v) for v in PIL.__version__.split(".")[:2]) < (10, 2):
        pytest.skip(f"Pillow {PIL.__version__} has no restart_marker_blocks; 10.2 or later is needed")
    from transflow_amd.jpeg import pillow_encode
    return pillow_encode


def _own_header(image, quality, restart):
    return jpeg_ref.header(image.shape[0], image.shape[1], quality, restart, tables=jpeg_ref.tables(image, quality, restart))


def test_every_case_is_here():
    assert sorted(os.path.basename(p)[8:-4] for p in FIXTURES) == sorted(CASES)
    assert len(CASES) == 2 + sum(1 for c in jpeg_cases.BASELINE_CASES.values() if c[0] <= 96 and c[1] <= 96)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_is_pillows_file(name):
    pillow_encode = _pillow()
    _, _, _, quality, restart = CASES[name]
    image = jpeg_cases.case_image("jpegopt", name)
    got, want = jpeg_ref.encode(image, quality, restart, optimize=True), pillow_encode(image, quality, restart, optimize=True)
    assert got == want, first_difference(got, want)
    assert want[:len(_own_header(image, quality, restart))] == _own_header(image, quality, restart)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_fixture_is_the_restatements_file(path):
    image, quality, restart, _, _, expected = jpeg_cases.load_case(path)
    name = os.path.basename(path)[8:-4]
    assert (image.shape[0], image.shape[1], quality, restart) == CASES[name][:2] + CASES[name][3:]
    assert (image == jpeg_cases.case_image("jpegopt", name)).all()
    got = jpeg_ref.encode(image, quality, restart, optimize=True)
    assert got == expected, first_difference(got, expected)


def test_optimised_files_decode_to_the_default_files_pixels():
    """The same pixels in a smaller file."""
    pillow_decode = pytest.importorskip("transflow_amd.framecodec").pillow_decode
    for name in ("45x61", "33x47_noise_q100"):
        _, _, _, quality, restart = CASES[name]
        image = jpeg_cases.case_image("jpegopt", name)
        plain, own = jpeg_ref.encode(image, quality, restart), jpeg_ref.encode(image, quality, restart, optimize=True)
        assert len(own) < len(plain)
        assert (pillow_decode(own) == pillow_decode(plain)).all()


def test_pillow_encode_takes_the_longest_row():
    """1 x 65500: the optimised file does not fit Pillow's default encoder buffer; pillow_encode makes room."""
    pillow_encode = _pillow()
    image = jpeg_cases.formula_image(1, 65500)
    want = jpeg_ref.encode(image, 50, 8, optimize=True)
    assert pillow_encode(image, 50, 8, optimize=True) == want
    assert pillow_encode(image, 50, 8) == jpeg_ref.encode(image, 50, 8)       # and the default call is what it was


# ---- the rule on hand-made histograms ---------------------------------------------------------------------------------
def _kraft(bits):
    return sum(n * 2 ** (16 - (i + 1)) for i, n in enumerate(bits))


def test_one_used_symbol():
    counts = np.zeros(256, np.uint32)
    counts[0x21] = 7
    assert jpeg_ref.gen_optimal_table(counts) == ([1] + [0] * 15, [0x21])           # one bit: the other is the reserved symbol's


def test_no_symbol_is_refused():
    with pytest.raises(ValueError):
        jpeg_ref.gen_optimal_table(np.zeros(256, np.uint32))


def test_equal_counts_exercise_the_ties():
    bits, vals = jpeg_ref.gen_optimal_table(np.full(256, 3, np.uint32))
    assert sum(bits) == 256 and sorted(vals) == list(range(256))
    # 257 leaves of which the reserved one (weight 1) pairs with symbol 255 first: 255 of 8 bits, 2 of 9, one of them real
    assert bits == [0] * 7 + [255, 1] + [0] * 7
    # c1 is the reserved symbol, c2 the LARGEST index among the equal counts: 255 shares the 9 bits (the smallest index
    # first would have sent 0 there)
    assert vals == list(range(256))
    codes = jpeg_ref.huff_codes(bits, vals)
    assert codes[255] == (0x1FE, 9) and all(codes[s] == (s, 8) for s in range(255))


def test_fibonacci_counts_to_depth_33_are_refused():
    assert jpeg_ref.code_sizes_before_limiting(jpeg_cases.fibonacci_counts(32)) == 32
    bits, vals = jpeg_ref.gen_optimal_table(jpeg_cases.fibonacci_counts(32))                  # the deepest libjpeg takes
    assert sum(bits) == 32 and max(i + 1 for i, n in enumerate(bits) if n) == 16
    assert jpeg_ref.code_sizes_before_limiting(jpeg_cases.fibonacci_counts(33)) == 33
    with pytest.raises(jpeg_ref.CodeLengthOverflow):
        jpeg_ref.gen_optimal_table(jpeg_cases.fibonacci_counts(33))


def test_limiting_loop_runs_more_than_once():
    counts = jpeg_cases.limiting_counts()
    assert jpeg_ref.code_sizes_before_limiting(counts) >= 19                         # lengths 17, 18, 19 ... each need the loop
    bits, vals = jpeg_ref.gen_optimal_table(counts)
    assert sum(bits) == int((counts > 0).sum()) == len(vals)
    assert max(i + 1 for i, n in enumerate(bits) if n) == 16
    assert _kraft(bits) <= 2 ** 16 - 1                                        # a prefix code with the all-ones code free


def test_every_table_is_a_prefix_code_with_room_for_the_reserved_symbol():
    for name in ("45x61", "270x480_q95", "224x224_wide_lane"):
        _, _, _, quality, restart = CASES[name]
        for bits, vals in jpeg_ref.tables(jpeg_cases.case_image("jpegopt", name), quality, restart):
            assert sum(bits) == len(vals) == len(set(vals)) and _kraft(bits) <= 2 ** 16 - 1


# ---- what the directed cases reach -----------------------------------------------------------------------------------
def test_wide_lane_case_has_a_lane_of_more_than_64_bits():
    _, _, _, quality, restart = CASES["224x224_wide_lane"]
    image = jpeg_cases.case_image("jpegopt", "224x224_wide_lane")
    t = jpeg_ref.trace(image, quality, restart, optimize=True)
    assert t.widest_lane[0] > 64, t.widest_lane                               # 70: three 16-bit ZRLs, a 16-bit code, 6 bits
    assert t.most_zrls(0)[0] == 3
    hist = jpeg_ref.histograms(image, quality, restart)
    assert hist[1][0xF0] == 3                                                 # the only ZRLs of the image
    assert jpeg_ref.huff_codes(*jpeg_ref.gen_optimal_table(hist[1]))[0xF0][1] == 16
    assert jpeg_ref.code_sizes_before_limiting(hist[1]) == 17


def test_q95_case_reaches_the_16_bit_limit():
    image, quality, restart, _, _, expected = jpeg_cases.load_case(jpeg_cases.fixture_path("jpegopt", "270x480_q95"))
    bits, _ = jpeg_ref.dht_tables(expected)[0x10]
    assert max(i + 1 for i, n in enumerate(bits) if n) == 16
    assert jpeg_ref.code_sizes_before_limiting(jpeg_ref.histograms(image, quality, restart)[1]) == 17


def test_headers_differ_in_length_from_frame_to_frame():
    a, b = jpeg_cases.case_image("jpegopt", "45x61"), jpeg_cases.case_image("jpegopt", "33x47_noise_q100")
    assert len(_own_header(a, 50, 4)) != len(_own_header(b, 100, 4))
    assert len(_own_header(a, 50, 4)) < len(jpeg_ref.header(45, 61, 50, 4))


# ---- the shared C++ rule on the CPU ------------------------------------------------------------------------------------
def _hostile():
    rng_free = jpeg_cases._hash(3, 1, 256).astype(np.uint64)
    big = np.zeros(256, np.uint32)
    big[7], big[200] = 999999990, 9                                           # the sum just below the selection sentinel
    one = np.zeros(256, np.uint32)
    one[255] = 1
    return {
        "none": np.zeros(256, np.uint32), "one": one, "equal": np.full(256, 3, np.uint32),
        "fib32": jpeg_cases.fibonacci_counts(32), "fib33": jpeg_cases.fibonacci_counts(33),
        "fib40": jpeg_cases.fibonacci_counts(40),
        "limiting": jpeg_cases.limiting_counts(), "big": big,
        "hashed": (rng_free % np.uint64(3000000)).astype(np.uint32),
        "sparse": np.where(rng_free % np.uint64(5) == 0, rng_free % np.uint64(1000), 0).astype(np.uint32),
    }


def test_host_check_program(tmp_path):
    """jpeg_huff.h on the CPU over the fixtures' histograms and the hostile ones: no sanitizer report, and every
    (fault, bits, vals) is the restatement's."""
    program, sanitized = build_host_check(tmp_path, "jpeg_huff_host_check.cpp")
    rows = {}
    for name in ("1x1", "45x61", "33x47_noise_q100", "32x32_checker_q100", "270x480_q95", "224x224_wide_lane"):
        _, _, _, quality, restart = CASES[name]
        for t, hist in enumerate(jpeg_ref.histograms(jpeg_cases.case_image("jpegopt", name), quality, restart)):
            rows[f"{name}.{t}"] = ("ac" if t & 1 else "dc", hist[:256])
    for name, counts in _hostile().items():
        rows[name] = ("ac", counts)
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("".join(f"{name} {kind} {' '.join(str(int(v)) for v in counts)}\n" for name, (kind, counts) in rows.items()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([program, str(corpus)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    got = {line.split()[0]: line.split()[1:] for line in run.stdout.splitlines()}
    assert sorted(got) == sorted(rows)
    for name, (kind, counts) in rows.items():
        try:
            bits, vals = jpeg_ref.gen_optimal_table(counts)
            want = ["0", bytes(bits).hex(), bytes(vals).hex()]
        except jpeg_ref.CodeLengthOverflow:
            want = ["1", "00" * 16, "-"]
        except ValueError:
            want = ["2", "00" * 16, "-"]
        assert got[name][:3] == want, name
        if want[0] == "0":
            codes = jpeg_ref.huff_codes(bits, vals)
            n = 16 if kind == "dc" else 256
            assert int(got[name][3]) == sum((s + 1) * ((length << 16) | code) for s, (code, length) in codes.items() if s < n), name
    print("sanitized" if sanitized else "not sanitized: the sanitizer runtime does not link here")


# ---- the options on the Python side (no GPU is touched) -----------------------------------------------------------------
def test_jpeg_frame_carries_optimize():
    import pickle

    from transflow_amd.jpeg import JpegFrame
    plain, own = JpegFrame(b"ab", (8, 8, 3), 50, 8), JpegFrame(b"ab", (8, 8, 3), 50, 8, True)
    assert not plain.optimize and own.optimize and plain != own
    assert pickle.loads(pickle.dumps(own)) == own and pickle.loads(pickle.dumps(own)).optimize
    assert "optimize=True" in repr(own)


def test_jpeg_optimize_needs_jpeg_frames():
    from transflow_amd import dropin
    from transflow_amd.compositor import HipCompositor
    with pytest.raises(ValueError):
        HipCompositor(48, 64, [], jpeg_optimize=True)
    with pytest.raises(ValueError):
        dropin.install(jpeg_optimize=True)                                 # refused before anything is installed
    comp = HipCompositor(48, 64, [], jpeg_frames=50, jpeg_optimize=True)
    again = HipCompositor.__new__(HipCompositor)
    again.__setstate__(comp.__getstate__())
    assert again.jpeg_optimize and again.jpeg_frames == 50
    old = dict(comp.__getstate__())
    del old["jpeg_optimize"]                                               # a state pickled before the option existed
    again.__setstate__(old)
    assert again.jpeg_optimize is False


def test_mjpeg_stream_encodes_raw_frames_with_the_same_setting():
    pillow_encode = _pillow()
    from transflow_amd.output import HipMjpegStream
    image = jpeg_cases.case_image("jpegopt", "45x61")
    stream = HipMjpegStream("s", (61, 45), quality=50, restart_mcus=4, optimize=True)
    stream.set_frame(image)
    want = jpeg_ref.encode(image, 50, 4, optimize=True)
    assert stream.processed().tobytes() == want == pillow_encode(image, 50, 4, optimize=True)
    plain = HipMjpegStream("s", (61, 45), quality=50, restart_mcus=4)
    plain.set_frame(image)
    assert plain.processed().tobytes() == jpeg_ref.encode(image, 50, 4)
