"""The Lucas-Kanade cases of tests/lk_cases.py on the CPU: each family covers what it was built for, as the restatement
(tests/lk_ref.py) says of it -- pair sums above 2^24 and up to the reachable maximum, every trace code and every reason
to stop, both sides of the eigenvalue test, Scharr values at both ends, pyrDown's rounding tie, every window residue,
eight pyramid levels -- and the restatement's two forms agree, as bits, where neither had been run before.  These are
the conditions that keep tests/test_gpu_lucaskanade_extremes.py from sliding back to easy inputs.  No GPU."""
import numpy as np
import pytest

from tests import lk_cases as LC
from tests import lk_ref

CONTENT = [c.name for c in LC.family("content")]
BY_PAIR = {name: [f"content_{name}_w{win}" for win in LC.CONTENT_WINDOWS] for name in LC.content_pairs()}
SATURATED = {"binary": LC.binary(), "blocks": LC.blocks()}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_every_family_has_its_cases():
    counts = {key: len(LC.family(key)) for key in ("content", "window", "geometry", "deep")}
    assert counts == {"content": 66, "window": 21, "geometry": 28, "deep": 4}, counts
    assert len({c.name for c in LC.all_cases()}) == len(LC.all_cases()) == sum(counts.values())
    for c in LC.all_cases():
        assert c.prev.dtype == c.next.dtype == np.uint8 and c.prev.shape == c.next.shape, c.name
        assert c.prev.size <= 520 * 600 and len(lk_ref.grid_points(*c.prev.shape, c.step)) <= 40 * 56, c.name
    assert all(c.prev.shape == (LC.H, LC.W) and c.max_level == 2 for c in LC.family("content"))
    assert {c.prev.shape for c in LC.family("geometry")} == set(LC.GEOMETRY_SHAPES) | {(LC.H, LC.W)}


# ---- content ---------------------------------------------------------------------------------------------------------
def test_pair_sums_pass_2_24_reach_the_maximum_and_fit_int32():
    """Above 2^24 float(a + b) and float(a) + float(b) differ, and so do the pairings (k, k + 4) and (k, k + 1); the
    kernel's int32 says what the restatement's int64 says as long as nothing passes 2^31 - 1."""
    pair = {c.name: LC.run(c.name).probe["max_pair_sum"] for c in LC.all_cases()}
    prod = {c.name: LC.run(c.name).probe["max_product"] for c in LC.all_cases()}
    above = sorted(n for n, v in pair.items() if v > 1 << 24)
    print(f"largest product {max(prod.values())}, largest pair sum {max(pair.values())}; {len(above)} cases above 2^24")
    for name in BY_PAIR:
        print(f"  {name}: pair sums by window {[pair[n] for n in BY_PAIR[name]]}")
    assert len(above) >= 20
    assert LC.PAIR_SUM_MAX == 66585600
    for name in ("blocks_rolled", "blocks_inverse"):
        assert [pair[f"content_{name}_w{win}"] for win in (9, 15)] == [LC.PAIR_SUM_MAX] * 2
    assert max(pair.values()) == LC.PAIR_SUM_MAX and max(prod.values()) == LC.PAIR_SUM_MAX // 2
    assert max(pair.values()) <= (1 << 31) - 1 and max(prod.values()) <= (1 << 31) - 1
    # a window below 8 has no pairs at all: its b is the scalar tail alone
    assert all(pair[n] == 0 for n in pair if LC.case(n).win < 8)


def test_the_grid_points_end_in_every_way():
    codes = LC.code_counts(CONTENT)
    stops = LC.stop_counts(CONTENT)
    print(f"content: trace codes {codes}; stops {stops}")
    for name, names in BY_PAIR.items():
        print(f"  {name}: codes {LC.code_counts(names)} stops {LC.stop_counts(names)}")
    assert codes[lk_ref.TR_DONE] > 1000 and codes[lk_ref.TR_LOST_EIG] > 1000 and codes[lk_ref.TR_LOST_NEXT] > 1000
    assert codes[lk_ref.TR_LOST_PREV] == 0                       # a grid point's window always touches the frame
    assert min(stops[s] for s in (lk_ref.STOP_EPS, lk_ref.STOP_OSC, lk_ref.STOP_COUNT, lk_ref.STOP_LOST)) > 1000
    assert stops[lk_ref.STOP_NONE] == codes[lk_ref.TR_LOST_EIG]
    assert stops[lk_ref.STOP_LOST] == codes[lk_ref.TR_LOST_NEXT]
    # a point that ran all its steps ran 30 of them, and one that ran none was lost first
    for name in CONTENT:
        r = LC.run(name)
        steps, stop = r.trace[:, :, 2], r.probe["stop"]
        assert (steps[stop == lk_ref.STOP_COUNT] == lk_ref.MAX_COUNT).all()
        assert (steps[stop == lk_ref.STOP_NONE] == 0).all()
        assert (steps[stop == lk_ref.STOP_OSC] >= 2).all() and (steps[stop == lk_ref.STOP_EPS] >= 1).all()
    # the axis-only and the flat frames lose every point at every level
    for name in ("step_edge", "black_white", "white_white", "faint"):
        c = LC.code_counts(BY_PAIR[name])
        assert c[lk_ref.TR_DONE] == c[lk_ref.TR_LOST_NEXT] == 0 < c[lk_ref.TR_LOST_EIG], name
        assert not any(LC.run(n).flow.any() for n in BY_PAIR[name])


def test_one_frame_has_tracked_and_lost_points():
    for name in BY_PAIR["bright_pixel"]:
        level0 = LC.run(name).trace[:, 0, 3]
        done, lost = int(np.sum(level0 == lk_ref.TR_DONE)), int(np.sum(level0 == lk_ref.TR_LOST_EIG))
        print(f"{name}: level 0: {done} done, {lost} lost by the eigenvalue")
        assert done >= 9 and lost >= 1000 and done + lost >= len(level0) - 2


def test_faint_texture_sits_at_the_eigenvalue_test():
    """minEig < 1e-4f decides; D < FLT_EPSILON never decides alone (minEig >= 1e-4 means both eigenvalues of A are at
    least 1e-4 * win^2 >= 9e-4, and D is their product).  {0, 1} noise stays under the test, {0, 2} noise straddles
    it."""
    for name in BY_PAIR["faint"]:
        eig = LC.run(name).probe["min_eig"]
        assert 0 < eig.max() < lk_ref.MIN_EIG, name
    assert max(LC.run(n).probe["min_eig"].max() for n in BY_PAIR["faint"]) > 0.9e-4
    for name in BY_PAIR["faint_0_2"]:
        p = LC.run(name).probe
        eig, det = p["min_eig"][:, 0], p["det"][:, 0]
        under, over = int(np.sum(eig < lk_ref.MIN_EIG)), int(np.sum(eig >= lk_ref.MIN_EIG))
        print(f"{name}: level 0: {under} under, {over} over, largest {eig.max():.3e}")
        assert not np.any((eig >= lk_ref.MIN_EIG) & (det < lk_ref.FLT_EPSILON))
        if LC.case(name).win != 16:
            assert under >= 30 and over >= 30, name
        else:
            assert over == 0 and eig.max() > 0.9e-4, name       # fractional weights smooth the derivatives


def test_scharr_and_pyrdown_reach_their_ends():
    """The tie (s + 128) >> 8 with s % 256 == 128 needs white pixels whose kernel weights add up to 128 of the 256.
    Binary noise has such sums in both pyrDowns of its pyramid.  4x4 blocks have none: an even column's five taps split
    between two blocks as 5 | 11 or 15 | 1, and no sum of products of those is 128; their sums reach 0 and 255 * 256."""
    for key, img in SATURATED.items():
        dx, dy = lk_ref.scharr(img)
        assert (dx.min(), dx.max(), dy.min(), dy.max()) == (-4080, 4080, -4080, 4080), key
        ties = []
        for level in lk_ref.pyramid(img, 3, 2)[:2]:
            acc = lk_ref.pyr_down_sum(level)
            np.testing.assert_array_equal(((acc + 128) >> 8).astype(np.uint8), lk_ref.pyr_down(level))
            ties.append(int(np.sum(acc % 256 == 128)))
        print(f"{key}: pyrDown sums that are rounding ties, by level: {ties}")
        acc = lk_ref.pyr_down_sum(img)
        if key == "binary":
            assert min(ties) >= 1
        else:
            assert ties == [0, 0] and acc.min() == 0 and acc.max() == 255 * 256
    a = LC.window_cases()[0].prev
    assert set(np.unique(a)) == {0, 255} and np.abs(lk_ref.scharr(a)[0]).max() == 4080


# ---- windows, geometry, pyramids -------------------------------------------------------------------------------------
def test_windows_cover_every_tail():
    wins = [c.win for c in LC.family("window")]
    assert set(wins) >= {3, 4, 5, 7, 8, 9, 12, 16, 24, 31, 32, 33, 40, 63, 64, 65, 127, 255}
    assert {w % 8 for w in wins} == set(range(8))
    assert {w % 4 for w in wins if w >= 32} == set(range(4))
    assert {w % 8 for w in LC.CONTENT_WINDOWS} == {3, 7, 0, 1} and min(LC.CONTENT_WINDOWS) < 4
    points = {c.name: len(lk_ref.grid_points(*c.prev.shape, c.step)) for c in LC.family("window")}
    assert max(points.values()) == 12 and points["window_w127"] == 6 and points["window_w255"] == 4
    c = LC.case("window_w255")
    assert c.win > max(c.prev.shape) and lk_ref.level_count(80, 64, 255, c.max_level) == 0
    assert LC.run("window_w255").probe["max_pair_sum"] == LC.PAIR_SUM_MAX


def test_geometry_ends():
    points = {c.name: len(lk_ref.grid_points(*c.prev.shape, c.step)) for c in LC.family("geometry")}
    assert points["geometry_step100_w3"] == points["geometry_step56_w3"] == 1 and points["geometry_step55_w3"] == 2
    for step in (100, 56):
        flow = LC.run(f"geometry_step{step}_w15").flow
        assert flow.any() and (flow == flow[0, 0]).all()
    flow = LC.run("geometry_step55_w15").flow
    assert (flow[:, :55] == flow[0, 0]).all() and (flow[:, 55] == flow[0, 55]).all()
    assert (flow[0, 55] != flow[0, 0]).any()
    small = [c for c in LC.family("geometry") if c.prev.size < 100]
    assert any(LC.run(c.name).flow.any() for c in small)
    assert LC.run("geometry_1x1_w3").flow.shape == (1, 1, 2)


def test_deep_pyramids():
    h, w = LC.DEEP_SHAPE
    for win in (3, 4):
        assert lk_ref.level_count(w, h, win, 12) == lk_ref.level_count(w, h, win, 50) == 7
        a, b = LC.run(f"deep_w{win}_l12"), LC.run(f"deep_w{win}_l50")
        assert a.trace.shape == (195, 8, 4)
        np.testing.assert_array_equal(bits(a.flow), bits(b.flow))
        np.testing.assert_array_equal(a.trace, b.trace)
        steps = LC.level_steps(f"deep_w{win}_l12")
        print(f"deep_w{win}: (sum, max) of steps per level {steps}")
        assert len(steps) == 8 and all(m == lk_ref.MAX_COUNT for _, m in steps[:7])
    assert [img.shape for img in lk_ref.pyramid(LC.case("deep_w3_l12").prev, 3, 12)][-3:] == [(17, 19), (9, 10), (5, 5)]


# ---- the restatement's two forms -------------------------------------------------------------------------------------
def _sample(c):
    """About 60 points, fewer under wide windows: the scalar form takes a Python step per window pixel and step."""
    return LC.sample_points(c, int(np.clip(3600 // c.win ** 2, 12, 60)))


@pytest.mark.parametrize("name", list(BY_PAIR))
def test_vectorised_equals_scalar_on_content(name):
    reached = 0
    for n in BY_PAIR[name]:
        c = LC.case(n)
        pts = _sample(c)
        probe = {}
        v = lk_ref.calc_pyr_lk(c.prev, c.next, pts, c.win, c.max_level, probe=probe)
        s = lk_ref.calc_pyr_lk_scalar(c.prev, c.next, pts, c.win, c.max_level)
        np.testing.assert_array_equal(bits(v), bits(s), err_msg=n)
        reached = max(reached, probe["max_pair_sum"])
    print(f"{name}: the sampled points reach a pair sum of {reached}")
    if name in ("binary_rolled", "binary_independent", "blocks_rolled", "blocks_inverse"):
        assert reached > 1 << 24
    if name == "blocks_inverse":
        assert reached == LC.PAIR_SUM_MAX


def test_vectorised_equals_scalar_on_windows():
    cases = [c for c in LC.family("window") if c.win <= 34]
    assert len(cases) == 15
    for c in cases:
        pts = lk_ref.grid_points(*c.prev.shape, c.step)
        pts = pts if c.win <= 16 else pts[[0, 5, 6, 11]]
        v = lk_ref.calc_pyr_lk(c.prev, c.next, pts, c.win, c.max_level)
        s = lk_ref.calc_pyr_lk_scalar(c.prev, c.next, pts, c.win, c.max_level)
        np.testing.assert_array_equal(bits(v), bits(s), err_msg=c.name)
