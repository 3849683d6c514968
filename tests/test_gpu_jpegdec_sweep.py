"""Both device JPEG decoders (transflow_amd/csrc/jpegdec.hip; DESIGN.md section 19, "Hand-built scans") over the hand-built
files of tests/jpegdec_sweep.py as kept in tests/golden/jpegdec_sweep.npz: every code length at every bit phase, every
symbol of the standard tables, the FAST_BITS seam, the serial reader's window refilled at every phase and at FF 00 pairs
split by its edge, blocks as long as the window's margin allows for, the largest categories, 4:2:0 with a refill inside
an MCU, and the segment forms the header walker takes.  The expected pixels are tests/jpegdec_ref.py's, which
tests/test_jpegdec_sweep_ref.py holds equal to Pillow's on every family but C (there the samples leave the range in which
libjpeg's own IDCTs agree, and the restatement alone pins them); that module also asserts what each family covers and
runs every file through the shared core on the CPU, under the sanitizers, first.  Every decode writes into a buffer with
guard bytes either side."""
import os

import numpy as np
import pytest

from tests import jpegdec_ref as JR
from tests.test_gpu_jpegdec import Handle
from tests.test_gpu_jpegdec_par import GROUP, ParHandle, sizes  # noqa: F401  (sizes: the fixture that forces the path's sizes)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SWEEP = np.load(os.path.join(GOLDEN, "jpegdec_sweep.npz"))
NAMES = [str(n) for n in SWEEP["names"]]
FAMILIES = {key: [n for n in NAMES if n[0] == key] for key in "abcdef"}
ACCEPTED = [n for n in NAMES if int(SWEEP[n + ".reject"]) == 0]
REJECTED = [n for n in NAMES if n not in ACCEPTED]
NO_DRI = [n for n in ACCEPTED if n + ".entries16" in SWEEP.files]
WITH_DRI = [n for n in ACCEPTED if n not in NO_DRI]
DEFAULT_SUB = 64                                                        # the rows the fixture keeps for the default size


def test_every_family_is_there():
    assert all(len(FAMILIES[key]) >= 2 for key in FAMILIES) and len(NAMES) >= 38
    assert len(NO_DRI) >= 25 and len(WITH_DRI) >= 7 and REJECTED == ["f_dht_cut_short"]
    longest = max(len(SWEEP[n + ".file"]) for n in NAMES)
    assert 4096 < longest < 26000


@pytest.fixture(scope="module")
def serial():
    h = ParHandle(mode=0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def parallel():
    h = ParHandle(mode=1)
    yield h
    h.close()


def _exact(handle, name, order=0, shift=0):
    data, rgb = SWEEP[name + ".file"].tobytes(), SWEEP[name + ".rgb"]
    rc, reject, got = handle.decode(data, rgb.shape, order, shift)
    assert rc == handle.ok, name
    assert reject == 0, f"{name}: rejected as {JR.REJECT[reject] if reject < len(JR.REJECT) else reject}"
    np.testing.assert_array_equal(got, rgb[:, :, ::-1] if order else rgb, err_msg=name)


def _rejected(handle, name):
    data, want = SWEEP[name + ".file"].tobytes(), int(SWEEP[name + ".reject"])
    info = JR.probe(data)
    shape = (info["height"], info["width"], 3) if info["reject"] == "ok" else (1, 1, 3)
    rc, reject, _ = handle.decode(data, shape)
    assert rc == handle.ok and reject == want != 0, f"{name}: {reject}, not {want}"


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_serial_kernel(serial, family):
    """Scan mode 0, one wave per interval: reject == 0 and exactly the expected pixels in RGB, in BGR and with the output
    a byte off the dword; the file the header walker rejects is rejected with the restatement's reason."""
    assert FAMILIES[family]
    for name in FAMILIES[family]:
        if name in REJECTED:
            _rejected(serial, name)
            continue
        _exact(serial, name)
        _exact(serial, name, order=1)
        _exact(serial, name, shift=1)
    assert serial.stats() == [0, 0, 0, 0]


@pytest.mark.parametrize("staged", (0, 1))
@pytest.mark.parametrize("sub", (16, 128, 0))
def test_the_parallel_path(parallel, sizes, sub, staged):
    """Scan mode 1 over every file without DRI, at subsequences of 16 and 128 bytes and the default, the scan read from
    memory and from LDS: the same pixels, the entries the serial decoder's states, the launches within groups + 1 and
    the rounds within the group's lanes."""
    sizes(sub, GROUP if sub else 0, staged)
    assert NO_DRI
    for name in NO_DRI:
        _exact(parallel, name)
        subs, groups, launches, rounds = parallel.stats()
        stored = SWEEP[f"{name}.entries{sub or DEFAULT_SUB}"]
        assert subs == len(stored) and groups == -(-subs // GROUP), (name, subs, groups, len(stored))
        assert 1 <= launches <= groups + 1 and 1 <= rounds <= GROUP, (name, launches, rounds)
        np.testing.assert_array_equal(parallel.entries(), stored, err_msg=name)
        if sub == 16:
            _exact(parallel, name, order=1)
            _exact(parallel, name, shift=1)
    for name in REJECTED:
        _rejected(parallel, name)


def test_files_with_a_restart_interval_keep_their_path(parallel, sizes):
    sizes(16)
    _exact(parallel, "a_seam_9_10")
    before = parallel.stats()
    assert before[0] > 0 and WITH_DRI
    for name in WITH_DRI:
        _exact(parallel, name)
        _exact(parallel, name, order=1, shift=1)
    assert parallel.stats() == before                                    # none of them took the parallel path


@pytest.mark.parametrize("mode", (0, 1))
def test_one_handle_decodes_the_whole_sweep_back_to_back(sizes, mode):
    """Every file on one handle, a Pillow-written 37 x 19 4:2:0 frame between each two: a stale window, stale sums or
    stale coefficients of the file before would show in the next."""
    sizes(16)
    z = np.load(os.path.join(GOLDEN, "jpegdec_valid.npz" if mode == 0 else "jpegdec_par_valid.npz"))
    between, between_rgb = z["geo_420_37x19.file"].tobytes(), z["geo_420_37x19.rgb"]
    assert (JR.probe(between)["restart_mcus"] == 0) == (mode == 1)
    h = ParHandle(mode=mode)
    try:
        for name in NAMES + NAMES[::-1]:
            if name in REJECTED:
                _rejected(h, name)
            else:
                _exact(h, name)
            rc, reject, got = h.decode(between, between_rgb.shape)
            assert rc == h.ok and reject == 0, name
            np.testing.assert_array_equal(got, between_rgb, err_msg=f"behind {name}")
    finally:
        h.close()
