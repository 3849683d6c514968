"""The device MT19937 stream (tf_mt_*, transflow_amd/csrc/mt19937.hip) against numpy's RandomState: fields, the seams
between segments, jumped states, and the state it hands back.  Doubles are compared as uint64, every one of them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 16                                  # doubles either side of a field
CANARY_BITS = np.uint64(0xC0FFEE00DEADBEEF)
POSITIONS = [624, 0, 1, 397, 623]
SIZES = [1, 311, 312, 313, 48 * 64, 53 * 37, 200000]


def state_at(seed, pos):
    """A RandomState whose state tuple has this pos: 624 fresh from the seed (word 0 of its key is the seed itself),
    1..623 after that many 32-bit draws, 0 by set_state of the seeded key with pos = 0."""
    rs = np.random.RandomState(seed)
    if pos == 0:
        rs.set_state(("MT19937", rs.get_state()[1], 0))
    elif pos != 624:
        rs.randint(0, 2**32, pos, dtype=np.uint32)
    assert rs.get_state()[2] == pos
    return rs


def draw(mt, n):
    """The handle's next n doubles as uint64, drawn between two canaries that must survive."""
    from transflow_amd.device import DevBuffer
    buf = DevBuffer.from_array(np.full(n + 2 * CANARY, CANARY_BITS, np.uint64))
    try:
        mt.random_sample_dev(buf.ptr + 8 * CANARY, n)
        got = buf.download((n + 2 * CANARY,), np.uint64)
    finally:
        buf.close()
    assert (got[:CANARY] == CANARY_BITS).all() and (got[-CANARY:] == CANARY_BITS).all(), "wrote outside the field"
    return got[CANARY:-CANARY]


def adopt(mt, rs):
    key, pos = rs.get_state()[1:3]
    mt.set_state(key, pos)


def continues(mt, rs, what):
    """tf_mt_get_state put into a fresh RandomState gives the next 2000 doubles of numpy's own object (which is left
    where it was)."""
    key, pos = mt.get_state()
    assert pos == 0
    fresh = np.random.RandomState(0)
    fresh.set_state(("MT19937", key, pos))
    saved = rs.get_state()
    np.testing.assert_array_equal(fresh.random_sample(2000).view(np.uint64), rs.random_sample(2000).view(np.uint64), err_msg=what)
    rs.set_state(saved)


@pytest.fixture
def mt():
    from transflow_amd.mtstream import Mt19937
    h = Mt19937()
    yield h
    h.close()


@pytest.fixture
def segments():
    """Sets the library's mt_segments for a test and puts the default back."""
    from transflow_amd import _lib

    def set_segments(g):
        _lib.set_option("mt_segments", g)
    yield set_segments
    _lib.set_option("mt_segments", 0)


@pytest.mark.parametrize("pos", POSITIONS)
def test_fields(mt, pos):
    for n in SIZES:
        rs = state_at(3, pos)
        adopt(mt, rs)
        np.testing.assert_array_equal(draw(mt, n), rs.random_sample(n).view(np.uint64), err_msg=f"n={n}")


def test_default_seed_and_unset_state(mt):
    """A handle nobody gave a state is the generator's own default (seed 5489); get_state before any draw is that."""
    key, pos = mt.get_state()
    rs = np.random.RandomState(5489)
    fresh = np.random.RandomState(0)
    fresh.set_state(("MT19937", key, pos))
    np.testing.assert_array_equal(fresh.random_sample(700).view(np.uint64), rs.random_sample(700).view(np.uint64))
    np.testing.assert_array_equal(draw(mt, 700), np.random.RandomState(5489).random_sample(700).view(np.uint64))


def test_get_state_before_a_draw_keeps_word_zero(mt):
    """pos = 0 on a seeded key: word 0 is the seed, handed out as the next word although only its top bit is state."""
    rs = state_at(9, 0)
    adopt(mt, rs)
    continues(mt, rs, "before any draw")
    np.testing.assert_array_equal(draw(mt, 5), rs.random_sample(5).view(np.uint64))
    continues(mt, rs, "after five doubles")


@pytest.mark.parametrize("shape", [(48, 64), (53, 37)])
@pytest.mark.parametrize("g", [2, 3, 4, 7])
def test_seams_and_jumped_states(mt, segments, shape, g):
    """mt_segments forced so that the segment length does not divide the field and the last segment is short; the second
    to fourth fields come from jumped states."""
    h, w = shape
    segments(g)
    rs = state_at(21, 397)
    adopt(mt, rs)
    for t in range(4):
        got = draw(mt, h * w)
        info = mt.info()
        words = -(-2 * h * w // g)
        assert info["segments"] == g and info["segment_words"] == words + (words & 1)   # an even length
        if shape == (53, 37) or g == 7:
            assert (2 * h * w) % info["segment_words"] != 0                               # the last segment is short
        np.testing.assert_array_equal(got.reshape(h, w), rs.random_sample((h, w)).view(np.uint64), err_msg=f"field {t}")
        continues(mt, rs, f"after field {t}")


def test_default_segments_jump(mt):
    """The default plan of a field large enough to be cut: several segments, four consecutive fields."""
    n = 200000
    rs = state_at(4, 624)
    adopt(mt, rs)
    for t in range(4):
        got = draw(mt, n)
        assert mt.info()["segments"] > 1
        np.testing.assert_array_equal(got, rs.random_sample(n).view(np.uint64), err_msg=f"field {t}")
    continues(mt, rs, "after four fields")


def test_size_change_stays_on_the_stream(mt, segments):
    for g in (0, 3):
        segments(g)
        rs = state_at(8, 1)
        adopt(mt, rs)
        for t, (h, w) in enumerate([(48, 64), (53, 37), (48, 64), (48, 64)]):
            np.testing.assert_array_equal(draw(mt, h * w).reshape(h, w), rs.random_sample((h, w)).view(np.uint64),
                                          err_msg=f"segments {g}, field {t}")
            continues(mt, rs, f"segments {g}, after field {t}")


def test_option_change_between_draws(mt, segments):
    rs = state_at(6, 624)
    adopt(mt, rs)
    for g in (0, 4, 1, 7):
        segments(g)
        np.testing.assert_array_equal(draw(mt, 48 * 64), rs.random_sample(48 * 64).view(np.uint64), err_msg=f"segments {g}")


def test_arguments_are_checked(mt):
    from transflow_amd.device import DevBuffer
    buf = DevBuffer(64)
    try:
        with pytest.raises(ValueError):
            mt.random_sample_dev(buf.ptr, 0)
        with pytest.raises(ValueError):
            mt.random_sample_dev(buf.ptr + 4, 1)
        with pytest.raises(ValueError):
            mt.set_state(np.zeros(624, np.uint32), 625)
        with pytest.raises(ValueError):
            mt.set_state(np.zeros(623, np.uint32), 0)
    finally:
        buf.close()
