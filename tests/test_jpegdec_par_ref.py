"""The parallel path of the device JPEG decoder for scans without restart markers, on the CPU: the Python restatement
(tests/jpegdec_par_ref.py) held to the serial decoder of tests/jpegdec_ref.py over tests/golden/jpegdec_par_*.npz, and
tools/jpegdec_par_host_check.cpp -- the lane function the kernels run (transflow_amd/csrc/jpegdec_par_common.h), under
the sanitizers where their runtime links -- held to the restatement.  No GPU, no Pillow."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import build_host_check
from tests import jpegdec_par_ref as PR
from tests import jpegdec_ref as JR
from tests import jpegdec_sweep as SW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SUBS = (16, 32, 128)

VALID = np.load(os.path.join(GOLDEN, "jpegdec_par_valid.npz"))
MALFORMED = np.load(os.path.join(GOLDEN, "jpegdec_par_malformed.npz"))
VALID_NAMES = [str(n) for n in VALID["names"]]
MALFORMED_NAMES = [str(n) for n in MALFORMED["names"]]
HOSTILE_NAMES = [str(n) for n in MALFORMED["hostile_names"]]
# the hand-built files of tests/jpegdec_sweep.py without DRI that the header walker takes: more of the accepted kind
SWEEP = {name: built.data for name, built in SW.all_cases() if JR.probe(built.data).get("restart_mcus") == 0}
SWEEP_NAMES = list(SWEEP)

_TRUTH = {}


def _truth(name):
    """The serial decoder's word on a file, computed once: (verdict, dequantised coefficients or None)."""
    if name not in _TRUTH:
        data = SWEEP[name] if name in SWEEP else (VALID if name in VALID_NAMES else MALFORMED)[name + ".file"].tobytes()
        try:
            _, coefs = JR.decode_coefficients(data)
            _TRUTH[name] = (data, "ok", coefs)
        except JR.Rejected as e:
            _TRUTH[name] = (data, e.reason, None)
    return _TRUTH[name]


def test_the_lenient_rules_are_the_headers():
    """The restatement's docstring and the shared header list the same five rules."""
    text = open(os.path.join(ROOT, "transflow_amd", "csrc", "jpegdec_par_common.h")).read()
    for phrase in ("skip one bit", "the block ends", "largest legal category", "the lane ends at the end of the data"):
        assert phrase in text and phrase in PR.__doc__, phrase
    assert f"PAR_REASON_BITS = {PR.REASON_BITS};" in text


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("name", VALID_NAMES)
def test_valid_fixtures(name, sub):
    """The fixed point's entries are the serial decode's states, its coefficients tests/jpegdec_ref.py's, and it is
    reached within `subsequences` rounds."""
    data, verdict, want = _truth(name)
    assert verdict == "ok"
    ps = PR.ParScan(data, sub)
    coef, got, entries, rows, rounds = ps.decode()
    assert got == "ok"
    assert entries == ps.serial_entries()
    assert 1 <= rounds <= ps.n_subs
    np.testing.assert_array_equal(ps.dequantised(coef), want)
    if sub in (16, 128):                                                 # what the fixture holds for the device
        stored = VALID[f"{name}.entries{sub}"]
        mine = np.array([[p & 0xFFFFFFFF, p >> 32, b, k, *row] for (p, b, k), row in zip(entries, rows)], np.uint32)
        np.testing.assert_array_equal(stored, mine)


@pytest.mark.parametrize("name", MALFORMED_NAMES)
def test_malformed_fixtures(name):
    """The verdict is the serial decoder's, whatever the subsequence size; the fixture's number is that verdict's."""
    data, want, _ = _truth(name)
    assert want != "ok" and JR.R[want] == int(MALFORMED[name + ".reject"])
    for sub in SUBS:
        assert PR.verdict(data, sub) == want, sub
        if want not in ("rst_count",):
            ps = PR.ParScan(data, sub)
            assert ps.decode()[4] <= ps.n_subs


def test_hostile_fixtures_reach_a_fixed_point():
    """Random bytes under real tables: the lenient decode ends, within the bound, and equals the serial lenient decode."""
    for name in HOSTILE_NAMES:
        data = MALFORMED[name + ".file"].tobytes()
        for sub in SUBS:
            ps = PR.ParScan(data, sub)
            entries, _, rounds = ps.fixed_point()
            assert entries == ps.serial_entries() and rounds <= ps.n_subs, (name, sub)


def _build_host_check(tmp_path):
    """tools/jpegdec_par_host_check.cpp, with the sanitizers where they run here: (program, sanitized)."""
    return build_host_check(tmp_path, "jpegdec_par_host_check.cpp")


def test_host_check_program(tmp_path):
    """The shared lane function on the CPU, lane after lane, the scan, the entries and the coefficients heap blocks of
    the size the decoder is entitled to, over the valid, the malformed and the hostile files and the hand-built ones of
    tests/jpegdec_sweep.py without DRI, at every subsequence size: no sanitizer report; every verdict and coefficient CRC-32 is the serial decoder's, every round count the
    restatement's."""
    program, sanitized = _build_host_check(tmp_path)
    names = VALID_NAMES + MALFORMED_NAMES + HOSTILE_NAMES + SWEEP_NAMES
    assert len(SWEEP_NAMES) >= 30 and len(names) >= 32 + 30
    files = {n: _truth(n)[0] if n in SWEEP else (VALID if n in VALID_NAMES else MALFORMED)[n + ".file"].tobytes() for n in names}
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(f"{name} {data.hex() or '-'}" for name, data in files.items()) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for sub in SUBS:
        run = subprocess.run([program, str(corpus), str(sub)], capture_output=True, text=True, env=env)
        assert run.returncode == 0, run.stderr[-4000:]
        assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
        got = {}
        for line in run.stdout.splitlines():
            name, verdict, crc, rounds = line.split()
            got[name] = (int(verdict), int(crc), int(rounds))
        assert sorted(got) == sorted(names)
        for name in VALID_NAMES + MALFORMED_NAMES + SWEEP_NAMES:
            _, verdict, coefs = _truth(name)
            want = (JR.R[verdict], JR.coefficients_crc(coefs) if coefs is not None else 0)
            assert got[name][:2] == want, (name, sub, got[name], want)
        for name in names:
            if name == "rst_without_dri":
                continue
            ps = PR.ParScan(files[name], sub)
            coef, verdict, _, _, rounds = ps.decode()
            crc = JR.coefficients_crc(ps.dequantised(coef)) if verdict == "ok" else 0
            assert got[name] == (JR.R[verdict], crc, rounds), (name, sub)
    print("sanitized" if sanitized else "not sanitized: the sanitizer runtime does not link here")


def test_hostile_fixtures_get_the_serial_verdict():
    """The first strict fault of the parallel decode is the serial decoder's, also where the scan is random bytes."""
    for name in HOSTILE_NAMES:
        data = MALFORMED[name + ".file"].tobytes()
        want = JR.verdict(data)
        for sub in SUBS:
            assert PR.verdict(data, sub) == want, (name, sub)


# ---- routing (no GPU call: a provider's constructor reads headers only) ----------------------------------------------------
def test_parallel_scan_routes_through_the_python_layers(tmp_path):
    import pickle

    from transflow_amd import dropin
    from transflow_amd.flow import HipFlowSource
    from transflow_amd.jpegdec import MjpegFrameProvider
    from transflow_amd.pixmap import HipMjpegPixmapSource
    z = np.load(os.path.join(GOLDEN, "jpegdec_stream.npz"))
    path = tmp_path / "clip.mjpeg"
    path.write_bytes(b"".join(z[f"{i}.file"].tobytes() for i in range(3)))

    def holder(factory, **options):
        class Ref:
            from_args = factory(lambda *a, **k: "the reference's", **options)
        return Ref

    for options, want in ((dict(mjpeg_inputs=True, mjpeg_parallel=True), True), (dict(mjpeg_inputs=True), False)):
        builder = holder(dropin._flow_from_args, **options).from_args(str(path))
        assert isinstance(builder, HipFlowSource.Builder) and isinstance(builder.provider_arg, MjpegFrameProvider)
        assert builder.provider_arg.parallel_scan is want
        source = holder(dropin._pixmap_from_args, stills=False, **options).from_args(str(path), (64, 48))
        assert isinstance(source, HipMjpegPixmapSource) and source.parallel_scan is want
    provider = MjpegFrameProvider(str(path), parallel_scan=True)
    assert provider.require_restart is True and pickle.loads(pickle.dumps(provider)).parallel_scan is True
    assert MjpegFrameProvider(str(path)).parallel_scan is False


def test_install_takes_parallel_for_mjpeg_inputs(tmp_path):
    """dropin.install(mjpeg_inputs="parallel") over the reference's own factory; True keeps meaning what it meant."""
    import sys
    import types
    import typing
    ref = "/root/reference"
    if not os.path.isdir(os.path.join(ref, "transflow")):
        pytest.skip("reference tree not present")
    from transflow_amd import dropin
    from transflow_amd.pixmap import HipMjpegPixmapSource
    z = np.load(os.path.join(GOLDEN, "jpegdec_stream.npz"))
    path = tmp_path / "clip.mjpeg"
    path.write_bytes(z["0.file"].tobytes())
    had_self = hasattr(typing, "Self")
    if not had_self:
        typing.Self = typing.Any
    stubbed = "cv2" not in sys.modules
    if stubbed:
        sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, ref)
    try:
        from transflow.pixmap import source
        original = source.PixmapSource.__dict__["from_args"]
        for value, want in (("parallel", True), (True, False)):
            dropin.install(flow=False, compositor=False, mjpeg_inputs=value)
            try:
                routed = source.PixmapSource.from_args(str(path), (64, 48))
                assert isinstance(routed, HipMjpegPixmapSource) and routed.parallel_scan is want
            finally:
                dropin.uninstall()
            assert source.PixmapSource.__dict__["from_args"] is original
    finally:
        sys.path.remove(ref)
        for m in [m for m in sys.modules if m == "transflow" or m.startswith("transflow.")]:
            del sys.modules[m]
        if stubbed:
            del sys.modules["cv2"]
        if not had_self:
            del typing.Self
