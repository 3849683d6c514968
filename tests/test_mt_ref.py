"""The host side of the device MT19937 stream (transflow_amd/csrc/mt19937_common.h through tf_mt_stage_*, and the
stand-alone tools/mt_host_check.cpp under the sanitizers) against numpy's RandomState and the plain-Python restatement
tests/mt_ref.py.  No GPU.  Everything is compared bit for bit: words as integers, doubles as uint64."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import mt_ref as M
from tests.helpers import build_host_check

JUMPS = [1, 623, 624, 625, 2 * 48 * 64, 2 * 2160 * 3840]
POSITIONS = [624, 0, 1, 397, 623]
COUNTS = [1, 311, 312, 313, 1000]


@pytest.fixture(scope="module")
def lib():
    from transflow_amd import _lib
    return _lib.load()


def _check(rc):
    from transflow_amd._lib import check
    check(rc)


def _jump_poly(lib, J):
    out = np.zeros(312, np.uint64)
    _check(lib.tf_mt_stage_jump_poly(J, C.c_void_p(out.ctypes.data)))
    return out


def _apply(lib, poly, key):
    key = np.ascontiguousarray(key, np.uint32)
    out = np.zeros(624, np.uint32)
    _check(lib.tf_mt_stage_apply(C.c_void_p(poly.ctypes.data), C.c_void_p(key.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def state_at(seed, pos):
    """A RandomState whose state tuple has this pos: 624 fresh from the seed, 1..623 after that many 32-bit draws, 0 by
    set_state of the first block with pos = 0 (no draw leaves numpy there)."""
    rs = np.random.RandomState(seed)
    if pos == 0:
        rs.randint(0, 2**32, 624, dtype=np.uint32)
        rs.set_state(("MT19937", rs.get_state()[1], 0))
    elif pos != 624:
        rs.randint(0, 2**32, pos, dtype=np.uint32)
    assert rs.get_state()[2] == pos
    return rs


def test_restatement_is_numpys_stream():
    """tests/mt_ref.py itself: its words, tempered, are RandomState's 32-bit draws, and its doubles random_sample's."""
    rs = np.random.RandomState(7)
    key, pos = rs.get_state()[1:3]
    x = M.raw_stream(M.window_at(key, pos), 2000)
    assert list(M.seed_key(7)) == [int(v) for v in key]
    words = rs.randint(0, 2**32, 1000, dtype=np.uint32)
    assert [M.temper(v) for v in x[:1000]] == [int(v) for v in words]
    doubles = rs.random_sample(500).view(np.uint64)
    assert [M.to_double_bits(M.temper(x[1000 + 2 * i]), M.temper(x[1001 + 2 * i])) for i in range(500)] == [int(v) for v in doubles]


def test_characteristic_polynomial(lib):
    degree = C.c_int()
    words = np.zeros(312, np.uint64)
    _check(lib.tf_mt_stage_charpoly(C.byref(degree), C.c_void_p(words.ctypes.data)))
    phi = sum(int(w) << (64 * i) for i, w in enumerate(words)) | (1 << degree.value)
    assert degree.value == 19937
    assert bin(phi).count("1") == 135
    assert phi == M.charpoly()


@pytest.mark.parametrize("J", JUMPS)
def test_jump_polynomial(lib, J):
    assert [int(w) for w in _jump_poly(lib, J)] == M.poly_words(M.jump_poly(J))


@pytest.mark.parametrize("J", [1, 624000])
def test_apply_is_the_stream_advanced_by_drawing(lib, J):
    """All 624 words of the jumped state: against the restatement's stream walked word by word, and -- handed to a fresh
    RandomState with pos = 0 -- against numpy's own object after it has drawn J words."""
    rs = np.random.RandomState(5)
    rs.random_sample(10)                                   # inside a block: every word of the window is a produced one
    key, pos = rs.get_state()[1:3]
    window = M.window_at(key, pos)
    out = _apply(lib, _jump_poly(lib, J), window)
    assert [int(v) for v in out] == M.raw_stream(window, J + 624)[J:]
    rs.randint(0, 2**32, J, dtype=np.uint32)               # one word each
    fresh = np.random.RandomState(0)
    fresh.set_state(("MT19937", out, 0))
    np.testing.assert_array_equal(fresh.random_sample(1000).view(np.uint64), rs.random_sample(1000).view(np.uint64))


def test_apply_on_a_seeded_key(lib):
    """A seeded key's word 0 is the seed, a word the recurrence never produced (only its top bit is state): the jumped
    state must not depend on its low bits."""
    key = np.random.RandomState(5).get_state()[1]
    assert int(key[0]) == 5
    out = _apply(lib, _jump_poly(lib, 624000), key)
    assert [int(v) for v in out] == M.raw_stream(key, 624000 + 624)[624000:]
    other = key.copy()
    other[0] ^= 0x7FFFFFFF
    np.testing.assert_array_equal(_apply(lib, _jump_poly(lib, 624000), other), out)


@pytest.mark.parametrize("pos", POSITIONS)
def test_random_sample(lib, pos):
    for n in COUNTS:
        rs = state_at(11, pos)
        key = np.ascontiguousarray(rs.get_state()[1], np.uint32)
        out = np.full(n + 2, -1.0)
        _check(lib.tf_mt_stage_random_sample(C.c_void_p(key.ctypes.data), pos, n, C.c_void_p(out[1:].ctypes.data)))
        assert out[0] == -1.0 and out[-1] == -1.0
        np.testing.assert_array_equal(out[1:-1].view(np.uint64), rs.random_sample(n).view(np.uint64), err_msg=f"n={n}")


def test_stage_arguments_are_checked(lib):
    key = np.zeros(624, np.uint32)
    out = np.zeros(4)
    with pytest.raises(ValueError):
        _check(lib.tf_mt_stage_random_sample(C.c_void_p(key.ctypes.data), 625, 4, C.c_void_p(out.ctypes.data)))
    with pytest.raises(ValueError):
        _check(lib.tf_mt_stage_random_sample(None, 0, 4, C.c_void_p(out.ctypes.data)))
    with pytest.raises(ValueError):
        _check(lib.tf_mt_stage_jump_poly(1, None))
    bad = np.zeros(312, np.uint64)
    bad[311] = 1 << 63                                      # degree 19967
    with pytest.raises(ValueError):
        _check(lib.tf_mt_stage_apply(C.c_void_p(bad.ctypes.data), C.c_void_p(key.ctypes.data), C.c_void_p(key.ctypes.data)))


def test_host_check_program(tmp_path):
    """tools/mt_host_check.cpp -- Berlekamp-Massey, the jump polynomial, its application and the CPU random_sample of
    the shared header, every case's buffers heap blocks of their own size -- under AddressSanitizer and UBSan where this
    machine links them: the same answers, and nothing for the sanitizers to say."""
    program, sanitized = build_host_check(tmp_path, "mt_host_check.cpp")
    cases = ["charpoly", "jump 1", "jump 624", "jump 6144", "apply 5 0 1", "apply 5 0 624000", "apply 5 311 6144",
             "sample 11 0 1", "sample 11 1 313", "sample 11 397 312", "sample 11 623 1000", "sample 11 624 311"]
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(cases) + "\n")
    ran = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stderr[-2000:]
    if sanitized:
        assert "ERROR" not in ran.stderr and "runtime error" not in ran.stderr, ran.stderr[-2000:]
    lines = ran.stdout.splitlines()
    assert len(lines) == len(cases)
    for case, line in zip(cases, lines):
        f = line.split()
        what = case.split()
        if what[0] == "charpoly":
            words = [int(f[3][16 * i:16 * i + 16], 16) for i in range(312)]
            assert (int(f[1]), int(f[2])) == (19937, 135)
            assert sum(w << (64 * i) for i, w in enumerate(words)) | (1 << 19937) == M.charpoly()
        elif what[0] == "jump":
            assert [int(f[3][16 * i:16 * i + 16], 16) for i in range(312)] == M.poly_words(M.jump_poly(int(what[1])))
        elif what[0] == "apply":
            seed, pos, J = (int(v) for v in what[1:])
            window = M.window_at(M.seed_key(seed), pos)
            assert [int(f[4][8 * i:8 * i + 8], 16) for i in range(624)] == M.raw_stream(window, J + 624)[J:]
        else:
            seed, skip, n = (int(v) for v in what[1:])
            rs = np.random.RandomState(seed)
            rs.randint(0, 2**32, skip, dtype=np.uint32)
            expect = rs.random_sample(n).view(np.uint64)
            assert [int(f[4][16 * i:16 * i + 16], 16) for i in range(n)] == [int(v) for v in expect]
