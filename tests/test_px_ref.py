"""CPU tests of the still pixmap sources: the numpy restatement (tests/px_ref.py) against what the reference's own
classes returned (tests/golden/px_*.npz, tools/capture_golden_px.py) and, where the reference package is importable,
against the classes themselves; then the host side of transflow_amd/pixmap.py -- dispatch, draws, tree flattening,
alteration, errors, pickling -- with its library calls replaced by that restatement.  No GPU."""
import glob
import os
import pickle
import random
import sys
import types
import typing

import numpy as np
import pytest

from tests import px_ref
from tests.conftest import GOLDEN

REF = "/root/reference"
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "px_*.npz")))


def _name(path):
    return os.path.basename(path)[3:-4]


_save_png = px_ref.save_png


def restated(z):
    """The fixture's array by px_ref."""
    kind, h, w = str(z["kind"]), int(z["height"]), int(z["width"])
    seed = int(z["seed"])
    if kind == "gradient":
        out = px_ref.gradient(h, w, seed)
    elif kind == "color":
        out = px_ref.color(h, w, str(z["color"]) or None, seed)
    elif kind == "image":
        out = np.array(z["image"])
    else:
        out = getattr(px_ref, kind)(h, w, seed)
    if "overlay" in z.files:
        out = px_ref.alter(out, z["overlay"])
    return out


def test_fixtures_are_all_there():
    names = {_name(p) for p in FIXTURES}
    assert {f"gradient_s{s}_{h}x{w}" for s, h, w in px_ref.GRADIENT_CASES} <= names
    assert {f"{k}_s{s}" for k in ("noise", "bwnoise", "cnoise", "color_random") for s in (0, 3)} <= names
    assert {"color_hex", "color_rgb", "image_rgb", "image_rgba", "altered_same", "altered_smaller"} <= names
    for p in FIXTURES:
        z = np.load(p)
        assert z["array"].shape[0] <= 64 and z["array"].shape[1] <= 200 and z["array"].shape[0] * z["array"].shape[1] <= 64 * 96


@pytest.mark.parametrize("path", FIXTURES, ids=_name)
def test_px_ref_equals_fixture(path):
    z = np.load(path)
    got = restated(z)
    assert got.dtype == np.uint8 and got.shape == z["array"].shape
    np.testing.assert_array_equal(got, z["array"])
    if str(z["kind"]) == "gradient":       # the tree the reference drew is the tree the restatement draws
        np.testing.assert_array_equal(px_ref.tree_rows(px_ref.gradient_tree(int(z["seed"]))), z["tree"])
        np.testing.assert_array_equal(px_ref.gradient_from_tree(px_ref.unflatten(z["tree"]), *z["array"].shape[:2]), z["array"])


def test_vectorised_gradient_equals_the_pixel_loop():
    for tree, h, w in ((px_ref.gradient_tree(31), 7, 9), (px_ref.gradient_tree(32), 2, 13), (px_ref.full_tree(3), 6, 5),
                       (px_ref.leaf_tree((px_ref.NODE_RGB,) * 3, rgb=(1.0, -1.0, 0.0)), 2, 2)):
        np.testing.assert_array_equal(px_ref.gradient_from_tree(tree, h, w), px_ref.gradient_loop(tree, h, w))


# ---- the reference itself, where it can be imported -----------------------------------------------------------------
@pytest.fixture
def reference():
    """transflow.pixmap.still / .source of the reference tree (over a stub cv2), removed from sys.modules afterwards."""
    if not os.path.isdir(os.path.join(REF, "transflow")):
        pytest.skip("reference tree not present")
    had_self = hasattr(typing, "Self")
    if not had_self:
        typing.Self = typing.Any
    stubbed = "cv2" not in sys.modules
    if stubbed:
        sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, REF)
    try:
        from transflow.pixmap import source, still
        yield types.SimpleNamespace(still=still, source=source)
    finally:
        sys.path.remove(REF)
        for m in [m for m in sys.modules if m == "transflow" or m.startswith("transflow.")]:
            del sys.modules[m]
        if stubbed:
            del sys.modules["cv2"]
        if not had_self:
            del typing.Self


def _run(source):
    with source as s:
        return np.asarray(next(s))


def test_px_ref_equals_live_reference(reference):
    S = reference.still
    for seed, h, w in ((21, 5, 7), (22, 3, 33), (23, 16, 9), (24, 2, 2), (25, 31, 2)):
        np.testing.assert_array_equal(px_ref.gradient(h, w, seed), _run(S.GradientPixmapSource(w, h, seed)), err_msg=f"gradient {seed}")
    for seed, h, w in ((4, 9, 11), (5, 1, 1), (6, 32, 3)):
        np.testing.assert_array_equal(px_ref.noise(h, w, seed), _run(S.NoisePixmapSource(w, h, seed)))
        np.testing.assert_array_equal(px_ref.bwnoise(h, w, seed), _run(S.BwNoisePixmapSource(w, h, seed)))
        np.testing.assert_array_equal(px_ref.cnoise(h, w, seed), _run(S.ColoredNoisePixmapSource(w, h, seed)))
        np.testing.assert_array_equal(px_ref.color(h, w, None, seed), _run(S.ColorPixmapSource(w, h, None, seed)))


# ---- transflow_amd.pixmap over a pretend device -----------------------------------------------------------------------
class _Buf:
    def __init__(self, nbytes):
        self.mem = np.zeros(nbytes, np.uint8)
        self.ptr = 0x1000
        self.nbytes = nbytes

    def close(self):
        self.ptr = None


class _Ev:
    def stream_wait(self):
        pass


@pytest.fixture
def P(monkeypatch):
    """transflow_amd.pixmap with its library calls replaced by numpy and px_ref; P.calls counts them."""
    from transflow_amd import pixmap as P
    calls = {"fill": 0, "gradient": 0, "upload": 0, "download": 0}

    def upload(buf, a):
        calls["upload"] += 1
        buf.mem[:a.size] = a.reshape(-1)

    def download(buf, shape):
        calls["download"] += 1
        return buf.mem[:int(np.prod(shape))].reshape(shape).copy()

    def fill(buf, n, rgb):
        calls["fill"] += 1
        buf.mem[:n * 3] = np.tile(np.asarray(rgb, np.uint8), n)

    def gradient(buf, w, h, nodes):
        calls["gradient"] += 1
        assert len(nodes) <= P.MAX_NODES
        buf.mem[:h * w * 3] = px_ref.gradient_from_tree(px_ref.unflatten(nodes), h, w).reshape(-1)

    monkeypatch.setattr(P, "_dev_alloc", _Buf)
    monkeypatch.setattr(P, "_dev_upload", upload)
    monkeypatch.setattr(P, "_dev_download", download)
    monkeypatch.setattr(P, "_dev_fill", fill)
    monkeypatch.setattr(P, "_dev_gradient", gradient)
    monkeypatch.setattr(P, "_recorded_event", _Ev)
    P.calls = calls
    yield P
    del P.calls


hip_source = px_ref.hip_source


@pytest.mark.parametrize("path", FIXTURES, ids=_name)
def test_host_side_reproduces_fixture(P, path, tmp_path):
    z = np.load(path)
    src = hip_source(P, z, tmp_path)
    with src as s:
        first = next(s)
        assert next(s) is first and isinstance(first, P.DevicePixmap)
        assert (s.height, s.width) == z["array"].shape[:2] and first.channels == z["array"].shape[2]
        np.testing.assert_array_equal(np.asarray(first), z["array"])
        np.asarray(first), first[0], first.tobytes()
        assert P.calls["download"] <= 1                   # the host copy is made at most once
    kind = str(z["kind"])
    if kind == "color":
        assert P.calls["fill"] == 1 and P.calls["upload"] == 0
    elif kind == "gradient":
        assert P.calls["gradient"] == 1 and P.calls["upload"] == 0
        np.testing.assert_array_equal(np.array(P.flatten_tree(src.tree), np.float64), z["tree"])
    else:
        assert P.calls["upload"] == 1 and P.calls["download"] == 0      # made on the host, sent up once


FROM_ARGS = [("color", "ColorPixmapSource"), ("COLOR", "ColorPixmapSource"), ("color:rgb(1, 2, 3)", "ColorPixmapSource"),
             ("color:#102030", "ColorPixmapSource"), ("color:red", "ColorPixmapSource"), ("#a0b1c2", "ColorPixmapSource"),
             ("a0b1c2", "ColorPixmapSource"), ("noise", "NoisePixmapSource"), (" Noise ", "NoisePixmapSource"),
             ("bwnoise", "BwNoisePixmapSource"), ("cnoise", "ColoredNoisePixmapSource"), ("gradient", "GradientPixmapSource"),
             ("first", "VideoStillPixmapSource")]


def test_from_args_dispatch(P, tmp_path):
    image = _save_png(np.zeros((3, 4, 3), np.uint8), tmp_path, "pix.PNG")
    for path, name in FROM_ARGS + [(image, "ImagePixmapSource")]:
        s = P.HipPixmapSource.from_args(path, (8, 6), seed=3, alteration_path="alt.png", flow_path="flow.mp4")
        assert type(s).__name__ == "Hip" + name, path
        assert s.seed == (3 if name not in ("ImagePixmapSource", "VideoStillPixmapSource") else None)
        assert s.alteration_path == (None if name == "GradientPixmapSource" else "alt.png")      # source.py:108
        assert s.length is None and s.framerate is None
        if name not in ("ImagePixmapSource", "VideoStillPixmapSource"):
            assert (s.width, s.height) == (8, 6)
    assert P.HipPixmapSource.from_args("color:rgb(1, 2, 3)", (8, 6)).color == "rgb(1, 2, 3)"
    assert P.HipPixmapSource.from_args("#A0B1C2", (8, 6)).color == "#a0b1c2"
    assert P.HipPixmapSource.from_args("first", (8, 6), flow_path="flow.mp4").path == "flow.mp4"
    for video in ("clip.mp4", "gradient2", str(tmp_path / "missing.png")):
        with pytest.raises(NotImplementedError):
            P.HipPixmapSource.from_args(video, (8, 6))


def test_from_args_dispatch_equals_the_reference(P, reference, tmp_path):
    image = _save_png(np.zeros((3, 4, 3), np.uint8), tmp_path, "pix.png")
    for path, _ in FROM_ARGS + [(image, None)]:
        kw = dict(seed=3, alteration_path="alt.png", flow_path="flow.mp4")
        ref = reference.source.PixmapSource.from_args(path, (8, 6), **kw)
        got = P.HipPixmapSource.from_args(path, (8, 6), **kw)
        assert type(got).__name__ == "Hip" + type(ref).__name__, path
        for attr in ("width", "height", "framerate", "length", "seed", "alteration_path", "color", "path"):
            assert getattr(got, attr, "absent") == getattr(ref, attr, "absent"), (path, attr)


def test_alteration_indices_equal_the_loop(P, tmp_path):
    rng = np.random.default_rng(5)
    for k, (shape, width) in enumerate((((5, 7, 4), 7), ((3, 4, 4), 9), ((4, 4, 3), 6), ((2, 3, 2), 5), ((3, 3, 4), 3))):
        overlay = rng.integers(0, 256, shape, dtype=np.uint8)
        if shape[2] >= 2:
            overlay[:, :, -1] *= rng.random(shape[:2]) < 0.6          # alpha (or the last channel): many zeros
        path = _save_png(overlay, tmp_path, f"o{k}.png")
        src = P.HipPixmapSource(path)
        src.width = width
        src.load_alteration()
        import PIL.Image
        inds, vals = px_ref.alteration_loop(np.array(PIL.Image.open(path)), width)
        assert src.alteration[0].tolist() == inds and src.alteration[1].tolist() == vals
        a, b = px_ref.alteration(np.array(PIL.Image.open(path)), width)
        assert a.tolist() == inds and b.tolist() == vals
    none = P.HipPixmapSource(None)
    none.load_alteration()
    assert none.alteration is None


def test_alteration_equals_the_reference(P, reference, tmp_path):
    overlay = np.random.default_rng(8).integers(0, 256, (6, 5, 4), dtype=np.uint8)
    overlay[::2, ::3, 3] = 0
    path = _save_png(overlay, tmp_path, "o.png")
    ref = reference.source.PixmapSource(path)
    ref.width = 11
    ref.load_alteration()
    got = P.HipPixmapSource(path)
    got.width = 11
    got.load_alteration()
    assert got.alteration[0].tolist() == ref.alteration[0] and got.alteration[1].tolist() == ref.alteration[1]


def test_overlay_larger_than_the_pixmap_is_an_index_error(P, tmp_path):
    overlay = np.full((9, 4, 4), 255, np.uint8)
    with pytest.raises(IndexError):
        P.HipColoredNoisePixmapSource(4, 5, 0, _save_png(overlay, tmp_path, "big.png")).__enter__()


def test_tree_flattening_round_trips(P):
    for seed in range(40):
        random.seed(seed)
        tree = P.generate_tree(P.NODE_TRIPLE, 5)
        assert tree == px_ref.gradient_tree(seed)
        nodes = P.flatten_tree(tree)
        assert 4 <= len(nodes) <= P.MAX_NODES and nodes[-1][0] == P.NODE_TRIPLE
        assert P.unflatten_tree(nodes) == tree
        assert nodes == [tuple(r) for r in px_ref.flatten(tree)]
    assert len(P.flatten_tree(px_ref.full_tree())) == 40
    with pytest.raises(ValueError):
        P.unflatten_tree([(P.NODE_I, 0, 0, 0), (P.NODE_MIX, 0, 0, 0)])
    with pytest.raises(ValueError):
        P.unflatten_tree([(P.NODE_I, 0, 0, 0), (P.NODE_J, 0, 0, 0)])


def _seed_with(P, kind, want):
    """A seed whose tree does (want) / does not contain a node of `kind`."""
    for seed in range(1000):
        if any(n[0] == kind for n in px_ref.flatten(px_ref.gradient_tree(seed))) == want:
            return seed
    raise AssertionError("no such seed")


def test_gradient_zero_division(P):
    with pytest.raises(ZeroDivisionError):
        P.HipGradientPixmapSource(7, 1, _seed_with(P, P.NODE_I, True)).__enter__()
    with pytest.raises(ZeroDivisionError):
        P.HipGradientPixmapSource(1, 7, _seed_with(P, P.NODE_J, True)).__enter__()
    with pytest.raises(ZeroDivisionError):
        px_ref.gradient(1, 7, _seed_with(P, P.NODE_I, True))
    seed = _seed_with(P, P.NODE_I, False)
    with P.HipGradientPixmapSource(7, 1, seed) as s:                   # no row node: a single row is fine
        np.testing.assert_array_equal(np.asarray(next(s)), px_ref.gradient(1, 7, seed))
    assert P.calls["gradient"] == 1


def test_gradient_zero_division_equals_the_reference(P, reference):
    seed = _seed_with(P, P.NODE_I, True)
    with pytest.raises(ZeroDivisionError):
        reference.still.GradientPixmapSource(7, 1, seed).__enter__()


STATE_CASES = [("HipColorPixmapSource", (6, 5, None, 4), lambda: px_ref.color(5, 6, None, 4)),
               ("HipColorPixmapSource", (6, 5, "#102030", 4), lambda: px_ref.color(5, 6, "#102030", 4)),
               ("HipNoisePixmapSource", (6, 5, 4), lambda: px_ref.noise(5, 6, 4)),
               ("HipBwNoisePixmapSource", (6, 5, 4), lambda: px_ref.bwnoise(5, 6, 4)),
               ("HipColoredNoisePixmapSource", (6, 5, 4), lambda: px_ref.cnoise(5, 6, 4)),
               ("HipGradientPixmapSource", (6, 5, 4), lambda: px_ref.gradient(5, 6, 4))]


def _states():
    return np.random.get_state(), random.getstate()


def _assert_same_states(a, b):
    assert a[1] == b[1]
    assert a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and a[0][2:] == b[0][2:]


@pytest.mark.parametrize("cls,args,restatement", STATE_CASES, ids=[f"{c[0]}-{c[1][2]}" for c in STATE_CASES])
def test_global_streams_are_left_as_the_restatement_leaves_them(P, cls, args, restatement):
    saved = _states()
    try:
        np.random.seed(99), random.seed(99)
        restatement()
        want = _states()
        np.random.seed(99), random.seed(99)
        getattr(P, cls)(*args).__enter__()
        _assert_same_states(_states(), want)
    finally:
        np.random.set_state(saved[0]), random.setstate(saved[1])


def test_global_streams_are_left_as_the_reference_leaves_them(P, reference):
    saved = _states()
    try:
        for cls, args, _ in STATE_CASES:
            np.random.seed(99), random.seed(99)
            getattr(reference.still, cls[3:])(*args).__enter__()
            want = _states()
            np.random.seed(99), random.seed(99)
            getattr(P, cls)(*args).__enter__()
            _assert_same_states(_states(), want)
    finally:
        np.random.set_state(saved[0]), random.setstate(saved[1])


def test_device_pixmap_is_the_array_to_numpy_and_pickles_as_one(P):
    a = px_ref.cnoise(5, 7, 1)
    pm = P.DevicePixmap.from_host(a)
    assert not isinstance(pm, np.ndarray)
    assert pm.shape == (5, 7, 3) and pm.dtype == np.uint8 and pm.ndim == 3 and len(pm) == 5 and pm.channels == 3
    assert pm.dev_ptr == 0x1000 and pm.size == 105 and pm.nbytes == 105
    np.testing.assert_array_equal(np.asarray(pm), a)
    np.testing.assert_array_equal(pm[1:3, ::2], a[1:3, ::2])
    np.testing.assert_array_equal(pm + 1, a + 1)
    np.testing.assert_array_equal(np.concatenate([pm, pm]), np.concatenate([a, a]))
    assert int(pm.sum()) == int(a.sum()) and pm.tobytes() == a.tobytes()
    assert not np.asarray(pm).flags.writeable and not pm[0].flags.writeable
    with pytest.raises(ValueError):
        np.asarray(pm)[0, 0, 0] = 1                       # readers get read-only views
    with pytest.raises(ValueError):
        np.add(pm, 1, out=pm)
    with pytest.raises(TypeError):
        pm[0, 0, 0] = 1
    for dumped in (pickle.dumps(pm), pickle.dumps(pm, protocol=2)):
        back = pickle.loads(dumped)
        assert type(back) is np.ndarray and back.dtype == np.uint8 and len(back.shape) == 3 and back.flags.writeable
        np.testing.assert_array_equal(back, a)
    from multiprocessing.reduction import ForkingPickler
    back = pickle.loads(bytes(ForkingPickler.dumps(pm)))    # what a multiprocessing queue sends
    assert type(back) is np.ndarray
    np.testing.assert_array_equal(back, a)
    pm.wait_on_stream()


def test_pixmap_interface(P):
    mask = np.ones((5, 6), bool)
    with P.HipColoredNoisePixmapSource(6, 5, 2) as src:
        itf = P.HipPixmapInterface(src, mask)
        assert itf.counter == -1 and itf.frame_number == -1 and itf.image is None and itf.introduction_mask is mask
        with pytest.raises(AssertionError):
            itf.get()
        first = itf.next()
        assert itf.next(timeout=1) is first and itf.get() is first and itf.image is first
        assert itf.counter == 1 and itf.frame_number == 1
    with pytest.raises(StopIteration):
        P.HipPixmapInterface(iter(()), mask).next()


def test_video_still_takes_a_frame_provider(P):
    bgr = np.random.default_rng(3).integers(0, 256, (4, 6, 3), dtype=np.uint8)

    class Provider:
        released = False

        def read(self):
            return bgr

        def release(self):
            self.released = True

    prov = Provider()
    with P.HipVideoStillPixmapSource(prov) as s:
        np.testing.assert_array_equal(np.asarray(next(s)), bgr[:, :, ::-1])
        assert (s.width, s.height) == (6, 4) and prov.released
    try:
        import cv2  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            P.HipVideoStillPixmapSource("clip.mp4").__enter__()


def test_dropin_swaps_and_restores_the_pixmap_factory(P, reference, tmp_path):
    from transflow_amd import dropin
    RefSource = reference.source.PixmapSource
    original = RefSource.__dict__["from_args"]
    dropin.install(flow=False, compositor=False)
    try:
        assert RefSource.__dict__["from_args"] is original                 # without the argument nothing changes
    finally:
        dropin.uninstall()
    dropin.install(flow=False, compositor=False, pixmaps=True)
    try:
        assert RefSource.__dict__["from_args"] is not original
        assert isinstance(RefSource.from_args("cnoise", (8, 6), seed=1), P.HipColoredNoisePixmapSource)
        assert isinstance(RefSource.from_args("gradient", (8, 6), seed=1), P.HipGradientPixmapSource)
        image = _save_png(np.zeros((3, 4, 3), np.uint8), tmp_path, "pix.png")
        assert isinstance(RefSource.from_args(image, (8, 6)), P.HipImagePixmapSource)
        seen = []
        import transflow.pixmap as ref_pixmap
        fake_cv = types.ModuleType("transflow.pixmap.cv")
        fake_cv.CvPixmapSource = lambda *a: seen.append(a) or "the reference's"
        sys.modules["transflow.pixmap.cv"] = fake_cv
        ref_pixmap.cv = fake_cv
        assert RefSource.from_args("clip.mp4", (8, 6), seek=2, repeat=3) == "the reference's"    # a video falls through
        assert seen == [("clip.mp4", 2, None, None, 3)]
    finally:
        dropin.uninstall()
    assert RefSource.__dict__["from_args"] is original
