"""The motion-vector checker (tests/mv_ref.py) against flows the reference painted, and the library's host stage
(tf_mv_stage_resolve_rects) against the checker.  No GPU: everything here is host arithmetic."""
import glob
import os

import numpy as np
import pytest

from tests import mv_ref
from tests.helpers import GOLDEN

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "mv_*.npz")))


def _load(path):
    z = np.load(path)
    vectors = z["vectors"] if bool(z["has_vectors"]) else None
    return vectors, int(z["width"]), int(z["height"]), z["flow"]


def test_fixtures_are_present():
    names = {os.path.basename(p) for p in FIXTURES}
    assert {"mv_known.npz", "mv_nosidedata.npz", "mv_h264_37x53.npz", "mv_h264_120x160.npz", "mv_h264_480x854.npz",
            "mv_hostile_120x160.npz"} <= names
    for p in FIXTURES:
        assert os.path.getsize(p) < 1 << 20


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_restatement_paints_what_the_reference_painted(path):
    vectors, w, h, flow = _load(path)
    assert flow.dtype == np.float32 and flow.shape == (h, w, 2)
    np.testing.assert_array_equal(mv_ref.bits(mv_ref.paint(vectors, w, h)), mv_ref.bits(flow))


def test_known_answer():
    """A 40 x 64 frame and four vectors (mv_ref.KNOWN_VECTORS) that show every point of the semantics at once: a
    negative bound wraps instead of clipping (vector 1 paints nothing, vector 2 lands at the far corner), the last writer
    wins (3 over 2), a zero motion paints -0.0, scale 3 gives float32(-1/3), and w = 9, h = 7 paint 8 x 6 before the
    clamp.  534 pixels end up with a bit set."""
    w, h = mv_ref.KNOWN_SIZE
    flow = mv_ref.paint(mv_ref.records(mv_ref.KNOWN_VECTORS), w, h)
    b = mv_ref.bits(flow)
    assert int(np.count_nonzero(b.reshape(-1, 2).any(axis=1))) == 534
    assert (b[0:16, 0:16, 0] == 0x80000000).all() and (flow[0:16, 0:16, 1] == 0.75).all()      # vector 0
    third = np.float32(-(1 / 3))
    assert (flow[22:35, 46:62] == third).all() and (flow[35:38, 46:56] == third).all()          # vector 2 ...
    assert (flow[35:40, 56:64] == np.array([0.5, -0.25], np.float32)).all()                     # ... under vector 3
    assert b[8, 8, 0] == 0x80000000 and flow[8, 8, 1] == 0.75
    assert not b[16:22].any() and not b[0:22, 16:].any()       # vector 1 (rows -4:12 -> 36:12) painted nothing
    z = np.load(os.path.join(GOLDEN, "mv_known.npz"))
    np.testing.assert_array_equal(b, mv_ref.bits(z["flow"]))


def test_resolve_slice_is_pythons():
    for n in (1, 2, 16, 37, 300):
        for a in range(-2 * n - 3, 2 * n + 4):
            for b in range(-2 * n - 3, 2 * n + 4, 3):
                lo, hi, _ = slice(a, b).indices(n)
                assert mv_ref.resolve_slice(a, b, n) == (lo, hi), (a, b, n)


def _tables():
    yield 64, 40, mv_ref.records(mv_ref.KNOWN_VECTORS)
    for (w, h, seed) in ((53, 37, 1), (1, 1, 2), (300, 1, 3), (1920, 1080, 4)):
        yield w, h, mv_ref.h264_like(w, h, seed)
        yield w, h, mv_ref.hostile(w, h, 2000, seed + 10)


def test_library_stage_matches_the_restatement():
    """tf_mv_stage_resolve_rects: the library's own slice resolution and division, vector by vector (empty
    rectangles included, as they resolve), against the restatement's; and every rectangle that paints lies inside
    the frame -- the paint kernel relies on it."""
    from transflow_amd.motionvectors import stage_resolve_rects
    for w, h, table in _tables():
        rects, values = stage_resolve_rects(w, h, table)
        exp_rects, exp_values = mv_ref.rects_and_values(table, w, h)
        np.testing.assert_array_equal(rects, exp_rects)
        np.testing.assert_array_equal(values.view(np.uint32), exp_values.view(np.uint32))
        assert (rects >= 0).all() and (rects[:, :2] <= h).all() and (rects[:, 2:] <= w).all()
    rects, values = stage_resolve_rects(7, 5, None)
    assert rects.shape == (0, 4) and values.shape == (0, 2)


def test_double_rounding_and_negative_zero():
    """float32(-(float64(m) / float64(s))), not a float32 division; motion 0 paints -0.0 (and +0.0 under a negative scale)."""
    from transflow_amd.motionvectors import stage_resolve_rects
    rng = np.random.default_rng(5)
    rows = [(-1, 16, 16, 20, 20, int(mx), int(my), int(s)) for mx, my, s in
            zip(rng.integers(-2 ** 31, 2 ** 31, 4000), rng.integers(-2 ** 15, 2 ** 15, 4000),
                rng.choice([1, 3, 7, 4, 16, 11, 65535, -3], 4000))]
    rows += [(-1, 16, 16, 20, 20, 0, 0, 4), (-1, 16, 16, 20, 20, 0, 5, -4)]
    _, values = stage_resolve_rects(64, 64, mv_ref.records(rows))
    exp = np.array([[np.float32(-(r[5] / r[7])), np.float32(-(r[6] / r[7]))] for r in rows], np.float32)
    np.testing.assert_array_equal(values.view(np.uint32), exp.view(np.uint32))
    assert values.view(np.uint32)[-2].tolist() == [0x80000000, 0x80000000]
    assert values.view(np.uint32)[-1].tolist() == [0, np.float32(1.25).view(np.uint32)]


def test_rejected_records_raise_value_errors_that_name_the_index():
    """source != -1 is the reference's AssertionError, motion_scale == 0 its ZeroDivisionError: no flow either way."""
    from transflow_amd.motionvectors import stage_resolve_rects
    good = (-1, 16, 16, 8, 8, 1, 1, 4)
    with pytest.raises(ValueError, match=r"vector 2 has source 1\b"):
        stage_resolve_rects(64, 40, mv_ref.records([good, good, (1, 16, 16, 8, 8, 1, 1, 4), good]))
    with pytest.raises(ValueError, match=r"vector 1 has motion_scale 0"):
        stage_resolve_rects(64, 40, mv_ref.records([good, (-1, 16, 16, 8, 8, 1, 1, 0)]))
    with pytest.raises(ValueError, match="vector 0"):
        mv_ref.paint(mv_ref.records([(0, 16, 16, 8, 8, 1, 1, 4)]), 64, 40)
    with pytest.raises(ValueError, match="vector 0"):
        mv_ref.paint(mv_ref.records([(-1, 16, 16, 8, 8, 1, 1, 0)]), 64, 40)
