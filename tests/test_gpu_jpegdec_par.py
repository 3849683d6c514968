"""The device JPEG decoder's parallel path for scans without restart markers (tf_jpegdec_set_scan_mode 1;
transflow_amd/csrc/jpegdec.hip, jpegdec_par_common.h) held to libjpeg's pixels -- Pillow's decodes
kept in tests/golden/jpegdec_par_valid.npz -- exactly, to the serial decoder's state at every subsequence boundary, and
to tests/jpegdec_ref.py for what it rejects and why.  The subsequence and work-group sizes are forced small
(jd_par_sub_bytes 16 and 128, jd_par_group_subs 64), so that a 33 KB file spans tens of work-groups.
tests/test_jpegdec_par_ref.py runs every file here through the shared lane function on the CPU, under the sanitizers,
first.  Every decode writes into a buffer with guard bytes either side."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import jpegdec_ref as JR
from tests.test_gpu_jpegdec import Handle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VALID = np.load(os.path.join(GOLDEN, "jpegdec_par_valid.npz"))
MALFORMED = np.load(os.path.join(GOLDEN, "jpegdec_par_malformed.npz"))
DRI = np.load(os.path.join(GOLDEN, "jpegdec_valid.npz"))
STREAM = np.load(os.path.join(GOLDEN, "jpegdec_stream.npz"))
VALID_NAMES = [str(n) for n in VALID["names"]]
MALFORMED_NAMES = [str(n) for n in MALFORMED["names"]]
SUBS = (16, 128)
GROUP = 64


def _valid(name):
    rgb = VALID[str(VALID[name + ".rgb_of"]) + ".rgb"] if name + ".rgb_of" in VALID.files else VALID[name + ".rgb"]
    return VALID[name + ".file"].tobytes(), rgb


class ParHandle(Handle):
    """A guarded handle in scan mode `mode`."""

    def __init__(self, mode=1, **kw):
        Handle.__init__(self, **kw)
        self.check(self.lib.tf_jpegdec_set_scan_mode(self.h, mode))

    def stats(self):
        out = (C.c_uint32 * 4)()
        self.check(self.lib.tf_jpegdec_par_stats(self.h, out))
        return [int(v) for v in out]

    def entries(self, capacity=1 << 16):
        rows = np.zeros((capacity, 8), np.uint32)
        n = C.c_uint32()
        self.check(self.lib.tf_jpegdec_par_entries(self.h, C.c_void_p(rows.ctypes.data), capacity, C.byref(n)))
        return rows[:n.value]


@pytest.fixture(scope="module")
def handle():
    h = ParHandle()
    yield h
    h.close()


@pytest.fixture
def sizes():
    """Forces the path's sizes for a test and gives the defaults back."""
    from transflow_amd import _lib
    lib = _lib.load()

    def force(sub, group=GROUP, staged=0):
        _lib.check(lib.tf_set_option(b"jd_par_sub_bytes", sub))
        _lib.check(lib.tf_set_option(b"jd_par_group_subs", group))
        _lib.check(lib.tf_set_option(b"jd_par_staged", staged))

    yield force
    force(0, 0, 0)


def _exact(handle, name, order=0, shift=0):
    data, rgb = _valid(name)
    rc, reject, got = handle.decode(data, rgb.shape, order, shift)
    assert rc == handle.ok
    assert reject == 0, f"{name}: rejected as {JR.REJECT[reject] if reject < len(JR.REJECT) else reject}"
    np.testing.assert_array_equal(got, rgb[:, :, ::-1] if order else rgb)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("name", VALID_NAMES)
def test_valid_files_decode_to_libjpegs_pixels(handle, sizes, name, sub):
    """Pillow's pixels in RGB and BGR, aligned and a byte off, the guards intact; the entries the serial decoder's
    states; the launches within groups + 1 and the rounds within the group's lanes."""
    sizes(sub)
    _exact(handle, name)
    subs, groups, launches, rounds = handle.stats()
    stored = VALID[f"{name}.entries{sub}"]
    assert subs == len(stored) and groups == -(-subs // GROUP)
    assert 1 <= launches <= groups + 1 and 1 <= rounds <= GROUP
    np.testing.assert_array_equal(handle.entries(), stored)
    if name.startswith("noise_"):
        assert launches >= 2 and groups >= 4
    _exact(handle, name, order=1)
    _exact(handle, name, shift=1)
    _exact(handle, name, order=1, shift=1)


@pytest.mark.parametrize("sub", SUBS)
def test_the_scan_read_from_lds(handle, sizes, sub):
    """jd_par_staged = 1: a work-group's share of the scan in LDS, the last lane's window reaching past it into memory.
    The same pixels, the same entries, the same verdicts."""
    sizes(sub, staged=1)
    for name in VALID_NAMES:
        _exact(handle, name)
        subs, groups, launches, rounds = handle.stats()
        assert launches <= groups + 1 and rounds <= GROUP
        np.testing.assert_array_equal(handle.entries(), VALID[f"{name}.entries{sub}"])
    for name in MALFORMED_NAMES:
        data = MALFORMED[name + ".file"].tobytes()
        info = JR.probe(data)
        rc, reject, _ = handle.decode(data, (info["height"], info["width"], 3))
        assert rc == handle.ok and reject == int(MALFORMED[name + ".reject"]), name


def test_the_default_sizes(handle):
    for name in ("noise_128_q100", "scene_256_q90", "geo_420_37x19", "short_grey_8x8", "garbage_behind_the_last_mcu"):
        _exact(handle, name)
        subs, groups, launches, rounds = handle.stats()
        assert launches <= groups + 1 and rounds <= 64


@pytest.mark.parametrize("sub", SUBS)
def test_malformed_files_are_rejected_with_the_serial_decoders_reason(handle, sizes, sub):
    """TF_OK, the reason tests/jpegdec_ref.py gives, the guards intact, and a valid decode right after is exact."""
    sizes(sub)
    for name in MALFORMED_NAMES:
        data = MALFORMED[name + ".file"].tobytes()
        want = int(MALFORMED[name + ".reject"])
        assert want != 0
        info = JR.probe(data)
        rc, reject, _ = handle.decode(data, (info["height"], info["width"], 3))
        assert rc == handle.ok, name
        assert reject == want, f"{name}: {JR.REJECT[reject] if reject < len(JR.REJECT) else reject}, not {JR.REJECT[want]}"
        _exact(handle, "geo_420_37x19")


def test_hostile_files_end(handle, sizes):
    """Random bytes under real tables: the call returns, with a verdict, the guards intact."""
    sizes(16)
    for name in (str(n) for n in MALFORMED["hostile_names"]):
        data = MALFORMED[name + ".file"].tobytes()
        info = JR.probe(data)
        rc, reject, _ = handle.decode(data, (info["height"], info["width"], 3))
        assert rc == handle.ok and reject == JR.R[JR.verdict(data)], name
        subs, groups, launches, rounds = handle.stats()
        assert launches <= groups + 1 and rounds <= GROUP


def test_files_with_a_restart_interval_keep_their_path(handle, sizes):
    sizes(16)
    _exact(handle, "scene_256_q90")
    before = handle.stats()
    for name in ("geo_420_37x19", "iv_37x19_r5", "sym_noise_q100"):
        data, rgb = DRI[name + ".file"].tobytes(), DRI[name + ".rgb"]
        rc, reject, got = handle.decode(data, rgb.shape)
        assert rc == handle.ok and reject == 0
        np.testing.assert_array_equal(got, rgb)
    assert handle.stats() == before                                      # none of them took the parallel path


def test_mode_0_decodes_the_same_files_the_old_way():
    old = ParHandle(mode=0)
    try:
        for name in ("geo_420_37x19", "geo_grey_64x48", "gradient_160x120"):
            _exact(old, name)
        assert old.stats() == [0, 0, 0, 0]
    finally:
        old.close()


def test_one_handle_alternates_and_grows(sizes):
    """Mode-1 files, files with DRI, a larger frame after a smaller one: stale entries, sums and coefficients of the
    frame before must not show."""
    sizes(16)
    h = ParHandle()
    try:
        order = ["geo_420_37x19", "scene_256_q90", "short_grey_8x8", "noise_128_q100", "geo_444_64x48", "flat_128"]
        for name in order + order[::-1]:
            _exact(h, name)
            data, rgb = DRI["iv_37x19_r2.file"].tobytes(), DRI["iv_37x19_r2.rgb"]
            rc, reject, got = h.decode(data, rgb.shape)
            assert rc == h.ok and reject == 0
            np.testing.assert_array_equal(got, rgb)
    finally:
        h.close()


def test_provider_decodes_frames_without_dri_on_the_device():
    from transflow_amd.jpegdec import MjpegFrameProvider
    last = int(STREAM["count"]) - 1
    data, rgb = STREAM[f"{last}.file"].tobytes(), STREAM[f"{last}.rgb"]
    assert JR.probe(data)["restart_mcus"] == 0
    p = MjpegFrameProvider([data, data], parallel_scan=True)
    frame = p.read("rgb")
    assert hasattr(frame, "dev_ptr") and p.fallbacks == 0
    np.testing.assert_array_equal(np.asarray(frame), rgb)
    np.testing.assert_array_equal(np.asarray(p.read("bgr")), rgb[:, :, ::-1])
    assert p.fallbacks == 0 and p._decoder.par_stats()["subsequences"] > 0
    p.release()
    import pickle
    assert pickle.loads(pickle.dumps(MjpegFrameProvider([data], parallel_scan=True))).parallel_scan is True
    default = MjpegFrameProvider([data])
    np.testing.assert_array_equal(np.asarray(default.read("rgb")), rgb)
    assert default.fallbacks == 1 and default.parallel_scan is False
    default.release()


def test_dropin_wires_parallel_through(tmp_path):
    """install(mjpeg_inputs="parallel"): the flow source's provider and the pixmap source carry parallel_scan; True does
    not."""
    from transflow_amd import dropin
    from transflow_amd.pixmap import HipMjpegPixmapSource
    last = int(STREAM["count"]) - 1
    data, rgb = STREAM[f"{last}.file"].tobytes(), STREAM[f"{last}.rgb"]
    path = tmp_path / "clip.mjpeg"
    path.write_bytes(data + data)

    def holders(value):
        class Pix:
            from_args = dropin._pixmap_from_args(lambda *a, **k: "the reference's", stills=False, mjpeg_inputs=True,
                                                 mjpeg_parallel=value == "parallel")
        return Pix

    for value, want in (("parallel", True), (True, False)):
        src = holders(value).from_args(str(path), None)
        assert isinstance(src, HipMjpegPixmapSource) and src.parallel_scan is want
        with src:
            frame = next(src)
            np.testing.assert_array_equal(np.asarray(frame), rgb)
            assert src.capture.parallel_scan is want and src.capture.fallbacks == (0 if want else 1)
