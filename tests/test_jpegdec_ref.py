"""The numpy restatement of the device JPEG decoder (tests/jpegdec_ref.py) held to libjpeg: equal to Pillow's pixels,
bit for bit, on every valid case, generated here at test time and as kept in tests/golden; the reject reason of every
malformed case; and tools/jpegdec_host_check.cpp -- the decoder's shared core on the CPU, under the sanitizers where
they link -- held to the restatement over all of them.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import build_host_check
from tests import jpegdec_ref as JR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _pillow_cases():
    PIL = pytest.importorskip("PIL")
    if tuple(int(v) for v in PIL.__version__.split(".")[:2]) < (10, 2):
        pytest.skip("Pillow before 10.2 has no restart_marker_blocks")
    from tests import jpegdec_cases as JC
    return JC


@pytest.fixture(scope="module")
def generated():
    JC = _pillow_cases()
    return JC, JC.valid_cases(), JC.malformed_cases(), JC.hostile_cases()


def test_names_mirror_the_header():
    """The Reject enum of jpegdec_common.h, the restatement's names and the package's are one list."""
    text = open(os.path.join(ROOT, "transflow_amd", "csrc", "jpegdec_common.h")).read()
    body = text[text.index("enum Reject"):]
    body = body[:body.index("};")]
    enum = [(m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"R_([A-Z0-9_]+) = (\d+)", body)]
    assert enum[-1] == ("count", len(JR.REJECT))
    assert [name for name, _ in enum[:-1]] == JR.REJECT and [v for _, v in enum[:-1]] == list(range(len(JR.REJECT)))
    names = re.findall(r'case R_[A-Z0-9_]+: return "([a-z0-9_]+)";', text)
    assert names == JR.REJECT
    src = open(os.path.join(ROOT, "transflow_amd", "jpegdec.py")).read()
    listed = re.search(r"REJECT_NAMES = \((.*?)\)", src, re.S).group(1)
    assert re.findall(r'"([a-z0-9_]+)"', listed) == JR.REJECT


def test_restatement_equals_pillow_on_every_valid_case(generated):
    JC, valid, _, _ = generated
    for name, data in valid:
        np.testing.assert_array_equal(JR.decode(data), JC.pillow_pixels(data), err_msg=name)
        np.testing.assert_array_equal(JR.decode(data, "bgr"), JC.pillow_pixels(data)[:, :, ::-1], err_msg=name)


def test_restatement_equals_the_fixtures_pixels():
    """The same against the Pillow decodes kept in tests/golden (whatever Pillow, if any, is installed here)."""
    z = np.load(os.path.join(GOLDEN, "jpegdec_valid.npz"))
    assert len(z["names"]) >= 20
    for name in z["names"]:
        np.testing.assert_array_equal(JR.decode(z[f"{name}.file"].tobytes()), z[f"{name}.rgb"], err_msg=str(name))
    s = np.load(os.path.join(GOLDEN, "jpegdec_stream.npz"))
    for i in range(int(s["count"])):
        np.testing.assert_array_equal(JR.decode(s[f"{i}.file"].tobytes()), s[f"{i}.rgb"])


def test_fixtures_are_what_the_generator_makes(generated):
    _, valid, malformed, _ = generated
    z = np.load(os.path.join(GOLDEN, "jpegdec_valid.npz"))
    assert [str(n) for n in z["names"]] == [n for n, _ in valid]
    m = np.load(os.path.join(GOLDEN, "jpegdec_malformed.npz"))
    assert [str(n) for n in m["names"]] == [n for n, _ in malformed]


# ---- the pixel stages' corpus (jpegdec_cases.geometry_cases, tests/golden/jpegdec_geometry.npz) -------------------------------
def _geometry_fixture():
    z = np.load(os.path.join(GOLDEN, "jpegdec_geometry.npz"))
    return z, [str(n) for n in z["names"]]


def test_the_geometry_corpus_is_the_sizes_it_is_for():
    from tests import jpegdec_cases as JC
    z, names = _geometry_fixture()
    want = [JC.geometry_name(layout, w, h, dri) for dri in (False, True) for layout in JC.GEOMETRY_LAYOUTS for w, h in JC.geometry_sizes(dri)]
    assert names == want and len(set(names)) == len(names) == 4 * (11 * 7 + 2 + 7 * 4)
    sampling = {"grey": (1, 1, 1), "444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)}
    for dri in (False, True):
        for layout in JC.GEOMETRY_LAYOUTS:
            for w, h in JC.geometry_sizes(dri):
                info = JR.probe(z[JC.geometry_name(layout, w, h, dri) + ".file"].tobytes())
                assert info["reject"] == "ok" and (info["width"], info["height"], info["restart_mcus"]) == (w, h, int(dri))
                assert (info["components"], info["h_samp"], info["v_samp"]) == sampling[layout]
    assert os.path.getsize(os.path.join(GOLDEN, "jpegdec_geometry.npz")) < os.path.getsize(os.path.join(GOLDEN, "jpegdec_par_valid.npz"))


def test_restatement_equals_pillow_on_every_geometry_case():
    """Live Pillow on freshly made files, and the fixture is those files with those pixels.  Before the restatement took
    libjpeg's replicating upsampler for downsampled_width <= 2 this failed for 4:2:2 at W = 2, 3, 4 and for 4:2:0 at
    W = 1, 2, 3, 4, and for nothing else."""
    JC = _pillow_cases()
    z, names = _geometry_fixture()
    cases = JC.geometry_cases()
    assert [name for name, _ in cases] == names
    for name, data in cases:
        want = JC.pillow_pixels(data)
        np.testing.assert_array_equal(JR.decode(data), want, err_msg=name)
        np.testing.assert_array_equal(JR.decode(data, "bgr"), want[:, :, ::-1], err_msg=name)
        assert z[name + ".file"].tobytes() == data, name
        np.testing.assert_array_equal(z[name + ".rgb"], want, err_msg=name)


def test_restatement_equals_the_geometry_fixtures_pixels():
    """The same against the Pillow decodes kept in tests/golden (whatever Pillow, if any, is installed here)."""
    z, names = _geometry_fixture()
    for name in names:
        np.testing.assert_array_equal(JR.decode(z[name + ".file"].tobytes()), z[name + ".rgb"], err_msg=name)


def test_the_geometry_corpus_tells_replication_from_blending():
    """For every subsampled case up to 4 pixels wide, blending at every width (the rule the restatement and the kernel had)
    gives other pixels than replication, so a decoder with either rule alone cannot pass: a smooth image would let both.
    The exceptions are no choice at all: at W = 1 there is only column 0, where the h2v1 filter copies the sample (4:2:2
    at W = 1), and the h2v2 filter gives (4 s + 8) >> 4 of s = 3 a + b, which is a where the context row b is the one
    chroma row a again (4:2:0 at W = 1, H <= 2).  There, and from W = 5 on, the two are the same function."""
    from tests import jpegdec_cases as JC
    z, _ = _geometry_fixture()
    told_apart = 0
    for dri in (False, True):
        for layout in ("422", "420"):
            for w, h in JC.geometry_sizes(dri):
                name = JC.geometry_name(layout, w, h, dri)
                data = z[name + ".file"].tobytes()
                same = np.array_equal(JR._decode_blending_at_every_width(data), JR.decode(data))
                if w > 4 or (w == 1 and (layout == "422" or h <= 2)):
                    assert same, name
                else:
                    assert not same, f"{name}: either upsampling rule gives these pixels"
                    told_apart += 1
    # W = 2, 3, 4 (2, 4 with DRI), 4 x 4 and 3 x 5 in both layouts; 4:2:0 at W = 1, H >= 3
    assert told_apart == 2 * (3 * 7 + 2 + 2 * 4) + (5 + 3)


def test_geometry_of_the_valid_cases(generated):
    _, valid, _, _ = generated
    info = {name: JR.probe(data) for name, data in valid}
    assert all(i["reject"] == "ok" for i in info.values())
    assert [info[f"iv_37x19_r{r}"]["intervals"] for r in (1, 2, 5, 6)] == [6, 3, 2, 1]
    assert info["iv_37x19_nodri"]["restart_mcus"] == 0 and info["iv_37x19_nodri"]["intervals"] == 1
    assert info["iv_160x16_r1"]["intervals"] == 10 and info["iv_512_grey_r1"]["intervals"] == 4096
    assert (info["geo_422_37x19"]["h_samp"], info["geo_422_37x19"]["v_samp"]) == (2, 1)
    assert (info["geo_444_37x19"]["h_samp"], info["geo_grey_37x19"]["components"]) == (1, 1)


def test_symbol_cases_hold_what_they_are_for(generated):
    _, valid, _, _ = generated
    files = dict(valid)
    for name in ("sym_noise_q100", "sym_noise_q1"):
        trace = {}
        JR.decode(files[name], trace=trace)
        assert trace["ff00"] >= 1 and trace["ac_symbols"].count(0xF0) >= 1, name
    trace = {}
    JR.decode(files["sym_flat"], trace=trace)
    assert set(trace["ac_symbols"]) == {0x00} and trace["dc_sizes"] == {0}
    annex_k = files["geo_420_37x19"]
    dht = lambda d: d[JR.find_segment(d, 0xC4)[0]:][:40]
    assert dht(files["sym_optimize"]) != dht(annex_k)


EXPECTED = {"rst_removed": "rst_count", "rst_swapped": "rst_order", "rst_duplicated": "rst_count", "rst_without_dri": "rst_count",
            "interval_emptied": "exhausted", "bad_code": "bad_code", "run_past_63": "run_past_63", "zrl_past_63": "run_past_63",
            "progressive": "progressive", "sof_411": "sampling", "sof_12bit": "precision", "sof_4_components": "components",
            "dqt_16bit": "dqt_16bit", "sos_ns_1": "multi_scan"}


def test_reject_reasons_of_the_malformed_cases(generated):
    JC, _, malformed, _ = generated
    files = dict(malformed)
    for name, reason in EXPECTED.items():
        assert JR.verdict(files[name]) == reason, name
    whole = JC.encode(JC.image(9, 17, 50), restart=1)
    scan_offset = JR.parse_header(whole)["scan_offset"]
    cuts = [n for n in files if n.startswith("cut_")]
    assert len(cuts) == (len(whole) + 9) // 10 and sorted(cuts + list(EXPECTED)) == sorted(files)
    for name in cuts:
        cut = int(name[4:])
        assert JR.verdict(files[name]) == ("truncated" if cut < scan_offset else "no_eoi"), name
    m = np.load(os.path.join(GOLDEN, "jpegdec_malformed.npz"))
    for name, data in malformed:
        assert m[f"{name}.file"].tobytes() == data and int(m[f"{name}.reject"]) == JR.R[JR.verdict(data)], name


def test_more_headers_are_rejected_with_a_reason(generated):
    JC, valid, _, _ = generated
    base = dict(valid)["geo_420_37x19"]
    sof, _ = JR.find_segment(base, 0xC0)
    patched = lambda at, v: base[:at] + bytes([v]) + base[at + 1:]
    assert JR.verdict(patched(sof + 1, 0xC9)) == "arithmetic"
    assert JR.verdict(patched(sof + 1, 0xC1)) == "sof_kind"
    assert JR.verdict(base[:sof + 5] + b"\x00\x00" + base[sof + 7:]) == "dnl"
    dht, _ = JR.find_segment(base, 0xC4)
    assert JR.verdict(patched(dht + 5, 3)) == "bad_dht"                     # three codes of one bit
    sos, _ = JR.find_segment(base, 0xDA)
    assert JR.verdict(patched(sos + 6, 0x33)) == "missing_table"
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    assert JR.verdict(base[:2] + adobe + base[2:]) == "adobe_transform"
    assert JR.verdict(base[:2] + adobe[:-1] + b"\x01" + base[2:]) == "ok"
    assert JR.verdict(base[:2] + b"\xff\xfe\x00\x05abc" + base[2:]) == "ok"      # COM is skipped
    assert JR.verdict(b"GIF89a") == "not_jpeg"
    scan = JR.parse_header(base)["scan_offset"]
    assert JR.verdict(base[:scan + 3] + b"\xff\xc4" + base[scan + 5:]) == "stray_marker"


def test_stream_index():
    files = [data for _, data in _golden_cases()[0][:5]]
    blob = b"".join(files)
    index = JR.index_stream(blob)
    assert [blob[a:a + n] for a, n in index] == files
    from transflow_amd.jpegdec import index_mjpeg_stream
    assert index_mjpeg_stream(blob + b"\xff\xd8\xff") == index


def _golden_cases():
    """(valid, malformed) as [(name, file bytes)] from tests/golden: what the device tests run, whatever Pillow is here."""
    out = []
    for kind in ("valid", "malformed"):
        z = np.load(os.path.join(GOLDEN, f"jpegdec_{kind}.npz"))
        out.append([(str(name), z[f"{name}.file"].tobytes()) for name in z["names"]])
    return out


def test_reject_reasons_of_the_fixtures():
    """The malformed fixtures carry the restatement's reason, and the named ones the reason they were built for."""
    _, malformed = _golden_cases()
    z = np.load(os.path.join(GOLDEN, "jpegdec_malformed.npz"))
    files = dict(malformed)
    assert set(EXPECTED) <= set(files) and all(n in EXPECTED or n.startswith("cut_") for n in files)
    for name, data in malformed:
        reason = JR.verdict(data)
        assert reason != "ok" and JR.R[reason] == int(z[f"{name}.reject"]), name
        assert name not in EXPECTED or reason == EXPECTED[name], name


def _build_host_check(tmp_path):
    """tools/jpegdec_host_check.cpp, with the sanitizers where they run here: (program, sanitized)."""
    return build_host_check(tmp_path, "jpegdec_host_check.cpp")


def test_host_check_program(tmp_path):
    """The shared core of jpegdec_common.h on the CPU, every buffer a heap block of the size the decoder is entitled
    to, over the valid and the malformed fixtures, the hostile files and the hand-built files of tests/jpegdec_sweep.py:
    no sanitizer report, and every verdict and coefficient CRC-32 the restatement's.  The hostile files are taken (their coefficients are as large as the rules
    allow: the IDCT's arithmetic must stay defined)."""
    from tests import jpegdec_cases as JC
    valid, malformed = _golden_cases()
    from tests import jpegdec_sweep as SW
    hostile = JC.hostile_cases()
    sweep = [(name, built.data) for name, built in SW.all_cases()]
    cases = valid + malformed + hostile + sweep
    program, sanitized = _build_host_check(tmp_path)
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(f"{name} {data.hex() or '-'}" for name, data in cases) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([program, str(corpus)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    got = {}
    for line in run.stdout.splitlines():
        name, verdict, crc = line.split()
        got[name] = (int(verdict), int(crc))
    want = {}
    for name, data in cases:
        try:
            _, coefs = JR.decode_coefficients(data)
            want[name] = (0, JR.coefficients_crc(coefs))
        except JR.Rejected as e:
            want[name] = (JR.R[e.reason], 0)
    assert len(sweep) >= 38 and len(got) == len(want) >= 110 + 38
    wrong = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
    assert not wrong, sorted(wrong.items())[:10]
    assert all(want[name][0] == 0 for name, _ in valid + hostile) and all(want[name][0] != 0 for name, _ in malformed)
    assert [name for name, _ in sweep if want[name][0] != 0] == ["f_dht_cut_short"]
    print("sanitized" if sanitized else "not sanitized: the sanitizer runtime does not link here")


# ---- routing (no GPU call: a provider's constructor reads headers only) ----------------------------------------------------
REF = "/root/reference"


@pytest.fixture
def stream_path(tmp_path):
    z = np.load(os.path.join(GOLDEN, "jpegdec_stream.npz"))
    path = tmp_path / "clip.mjpeg"
    path.write_bytes(b"".join(z[f"{i}.file"].tobytes() for i in range(3)))
    return str(path)


def test_dropin_routes_mjpeg_flow_paths_only_on_request(stream_path):
    from transflow_amd import dropin
    from transflow_amd.flow import HipFlowSource
    from transflow_amd.jpegdec import MjpegFrameProvider

    def holder(**options):
        class Ref:
            from_args = dropin._flow_from_args(lambda *a, **k: "the reference's", **options)
        return Ref

    builder = holder(mjpeg_inputs=True).from_args(stream_path)
    assert isinstance(builder, HipFlowSource.Builder) and isinstance(builder.provider_arg, MjpegFrameProvider)
    assert (builder.provider_arg.width, builder.provider_arg.height, builder.provider_arg.frame_count) == (64, 48, 3)
    assert holder().from_args(stream_path).provider_arg == stream_path                   # without it: a path for cv2, as before
    assert holder(mjpeg_inputs=True).from_args("clip.mp4").provider_arg == "clip.mp4"    # not a stream file


def test_dropin_routes_mjpeg_pixmap_paths_only_on_request(stream_path):
    import sys
    import types
    import typing
    if not os.path.isdir(os.path.join(REF, "transflow")):
        pytest.skip("reference tree not present")
    from transflow_amd import dropin
    from transflow_amd.pixmap import HipMjpegPixmapSource
    had_self = hasattr(typing, "Self")
    if not had_self:
        typing.Self = typing.Any
    stubbed = "cv2" not in sys.modules
    if stubbed:
        sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, REF)
    try:
        from transflow.pixmap import source, still
        RefSource = source.PixmapSource
        original = RefSource.__dict__["from_args"]
        dropin.install(flow=False, compositor=False, mjpeg_inputs=True)
        try:
            routed = RefSource.from_args(stream_path, (64, 48), seek=1, repeat=2)
            assert isinstance(routed, HipMjpegPixmapSource) and (routed.seek, routed.repeat) == (1, 2)
            assert isinstance(RefSource.from_args("cnoise", (8, 6), seed=1), still.ColoredNoisePixmapSource)   # stills stay
            from transflow_amd.pixmap import HipColoredNoisePixmapSource
            dropin.install(flow=False, compositor=False, pixmaps=True)          # a later call adds its option to the first's
            assert isinstance(RefSource.from_args("cnoise", (8, 6), seed=1), HipColoredNoisePixmapSource)
            assert isinstance(RefSource.from_args(stream_path, (64, 48)), HipMjpegPixmapSource)
        finally:
            dropin.uninstall()
        assert RefSource.__dict__["from_args"] is original
        dropin.install(flow=False, compositor=False, pixmaps=True)              # and in the other order
        try:
            dropin.install(flow=False, compositor=False, mjpeg_inputs=True)
            assert isinstance(RefSource.from_args(stream_path, (64, 48)), HipMjpegPixmapSource)
            assert isinstance(RefSource.from_args("cnoise", (8, 6), seed=1), HipColoredNoisePixmapSource)
        finally:
            dropin.uninstall()
        assert RefSource.__dict__["from_args"] is original
    finally:
        sys.path.remove(REF)
        for m in [m for m in sys.modules if m == "transflow" or m.startswith("transflow.")]:
            del sys.modules[m]
        if stubbed:
            del sys.modules["cv2"]
        if not had_self:
            del typing.Self
