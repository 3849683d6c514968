"""GPU tests of the device-resident still pixmaps: tf_pixmap_fill_dev / tf_pixmap_gradient_dev against the numpy
restatement (tests/px_ref.py) and the reference's recorded arrays (tests/golden/px_*.npz), bit for bit; and every
compositor layer class fed the same pixmaps once as host arrays and once as DevicePixmaps -- same frames, same layer
state, and in the device run no pixmap upload at all."""
import glob
import os
import threading

import numpy as np
import pytest

from tests import px_ref
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "px_*.npz")))
GUARD = 64          # bytes behind the image that no kernel may touch
SENTINEL = 0xA5


def _name(path):
    return os.path.basename(path)[3:-4]


@pytest.mark.parametrize("path", FIXTURES, ids=_name)
def test_sources_reproduce_the_reference_fixtures(path, tmp_path):
    from transflow_amd import pixmap as P
    z = np.load(path)
    with px_ref.hip_source(P, z, tmp_path) as source:
        pm = next(source)
        assert isinstance(pm, P.DevicePixmap) and next(source) is pm and pm.dev_ptr
        got = np.asarray(pm)
        assert got.dtype == np.uint8 and got.shape == z["array"].shape
        np.testing.assert_array_equal(got, z["array"])
        # what the layers read is the device copy: look at it too
        np.testing.assert_array_equal(pm._buf.download(z["array"].shape, np.uint8), z["array"])


class _Guarded:
    """A device buffer of n bytes + GUARD, all of it the sentinel."""

    def __init__(self, n):
        from transflow_amd.device import DevBuffer
        self.n = n
        self.buf = DevBuffer.from_array(np.full(n + GUARD, SENTINEL, np.uint8))
        self.ptr = self.buf.ptr

    def image(self, shape):
        return self.buf.download(shape, np.uint8)

    def guard_untouched(self):
        return bool((self.buf.download((GUARD,), np.uint8, offset=self.n) == SENTINEL).all())


def _gradient_dev(tree, h, w):
    from transflow_amd import pixmap as P
    g = _Guarded(h * w * 3)
    P._dev_gradient(g, w, h, px_ref.flatten(tree))
    out = g.image((h, w, 3))
    assert g.guard_untouched(), "the kernel wrote behind the image"
    return out


J, I, RGB = px_ref.NODE_J, px_ref.NODE_I, px_ref.NODE_RGB
MIXED_ROOT = (px_ref.NODE_MIX, (I, None, None, None),
              (px_ref.NODE_TRIPLE, (J, None, None, None), (RGB, .1, .2, .3), (I, None, None, None)), (RGB, -1.0, 1.0, 0.0))
GRADIENT_SHAPES = [
    ("2x2", lambda: px_ref.gradient_tree(11), 2, 2),
    ("1x7_j_and_rgb_leaves", lambda: px_ref.leaf_tree((J, RGB, J)), 1, 7),
    ("37x53_tail", lambda: px_ref.gradient_tree(0), 37, 53),              # 159 bytes a row; 1961 pixels = 490 x 4 + 1
    ("37x53_tail_other_tree", lambda: px_ref.gradient_tree(5), 37, 53),
    ("9x200", lambda: px_ref.gradient_tree(2), 9, 200),
    ("64x96", lambda: px_ref.gradient_tree(7), 64, 96),
    ("270x481", lambda: px_ref.gradient_tree(0), 270, 481),               # 129870 pixels = 4 x 32467 + 2: many blocks, a tail of 2
    ("3x5_tail_of_3", lambda: px_ref.gradient_tree(1), 3, 5),
    ("40_nodes_every_slot_a_mix", lambda: px_ref.full_tree(1), 37, 53),
    ("every_top_slot_a_leaf", lambda: px_ref.leaf_tree((I, J, RGB)), 9, 20),
    ("constants_plus_minus_one_and_zero", lambda: px_ref.leaf_tree((RGB,) * 3, rgb=(1.0, -1.0, 0.0)), 3, 5),
    ("constants_just_outside", lambda: px_ref.leaf_tree((RGB,) * 3, rgb=(-1.0 - 2.0 ** -52, 1.0 + 2.0 ** -52, -0.0)), 3, 5),
    ("mix_of_constants_at_the_ends", lambda: (px_ref.NODE_TRIPLE, *[(px_ref.NODE_MIX, (RGB, a, a, a), (RGB, -1.0, -1.0, -1.0),
                                                                   (RGB, 1.0, 1.0, 1.0)) for a in (-1.0, 0.0, 1.0)]), 2, 3),
    ("root_a_mix_with_a_triple_inside", lambda: MIXED_ROOT, 11, 13),
]


@pytest.mark.parametrize("name,tree,h,w", GRADIENT_SHAPES, ids=[c[0] for c in GRADIENT_SHAPES])
def test_gradient_kernel_equals_the_restatement(name, tree, h, w):
    tree = tree()
    if name.startswith("40_nodes"):
        assert px_ref.count_nodes(tree) == 40
    want = px_ref.gradient_from_tree(tree, h, w)
    if name.startswith("constants_plus"):
        assert want[0, 0].tolist() == [255, 0, 127]
    np.testing.assert_array_equal(_gradient_dev(tree, h, w), want)


def test_gradient_trees_of_many_seeds():
    """Trees as generate() makes them, 40 seeds at an odd size: every slot pattern that comes up."""
    for seed in range(100, 140):
        tree = px_ref.gradient_tree(seed)
        np.testing.assert_array_equal(_gradient_dev(tree, 13, 21), px_ref.gradient_from_tree(tree, 13, 21), err_msg=f"seed {seed}")


def test_gradient_refuses_bad_trees_without_a_launch():
    from transflow_amd import _lib
    from transflow_amd import pixmap as P
    leaf = (I, 0.0, 0.0, 0.0)
    deep = (px_ref.NODE_MIX, (px_ref.NODE_MIX, (px_ref.NODE_MIX, *[(I, None, None, None)] * 3), *[(I, None, None, None)] * 2),
            *[(J, None, None, None)] * 2)
    g = _Guarded(4 * 4 * 3)
    _lib.profile(True, "pixmap_")
    try:
        for nodes, error in (([leaf] * 41, ValueError),                                        # more than 40 nodes
                             ([], ValueError),
                             ([(7, 0.0, 0.0, 0.0)], ValueError),                               # an unknown type
                             ([(px_ref.NODE_Z, 0.0, 0.0, 0.0)], ValueError),                   # the reference's inner markers too
                             ([leaf, (px_ref.NODE_MIX, 0.0, 0.0, 0.0)], ValueError),           # a mix over one value
                             ([leaf, leaf], ValueError),                                       # two trees
                             (px_ref.flatten((px_ref.NODE_TRIPLE, deep, deep, deep)), NotImplementedError)):
            with pytest.raises(error):
                P._dev_gradient(g, 4, 4, nodes)
        with pytest.raises(ValueError):
            P._dev_gradient(g, 4, 1, [leaf])                       # a row node with height 1: the reference divides by zero
        with pytest.raises(ValueError):
            P._dev_gradient(g, 1, 4, [(J, 0.0, 0.0, 0.0)])
        from transflow_amd.device import sync
        sync()
        assert not [k for k in _lib.profile_report() if k.startswith("pixmap_")]
        P._dev_gradient(g, 4, 4, [leaf])                           # (the profiler does see a launch when there is one)
        sync()
        assert _lib.profile_report()["pixmap_gradient"][0] == 1
    finally:
        _lib.profile(False)
    assert g.guard_untouched()


@pytest.mark.parametrize("h,w", [(1, 1), (37, 53), (64, 96), (1, 4), (1, 7)])
def test_fill_kernel(h, w):
    from transflow_amd import pixmap as P
    g = _Guarded(h * w * 3)
    P._dev_fill(g, h * w, (16, 32, 48))
    want = np.empty((h, w, 3), np.uint8)
    want[:, :] = (16, 32, 48)
    np.testing.assert_array_equal(g.image((h, w, 3)), want)
    assert g.guard_untouched()
    P._dev_fill(g, 0, (1, 2, 3))
    np.testing.assert_array_equal(g.image((h, w, 3)), want)


def test_gradient_source_needs_no_host_copy_and_raises_zero_division():
    from transflow_amd import pixmap as P
    with P.HipGradientPixmapSource(53, 37, 0) as s:
        pm = next(s)
        assert pm._host is None and pm.shape == (37, 53, 3)
        np.testing.assert_array_equal(np.asarray(pm), px_ref.gradient(37, 53, 0))
        assert np.asarray(pm) is not None and pm._host is not None and not np.asarray(pm).flags.writeable
    seed = next(s for s in range(1000) if any(n[0] == I for n in px_ref.flatten(px_ref.gradient_tree(s))))
    with pytest.raises(ZeroDivisionError):
        P.HipGradientPixmapSource(7, 1, seed).__enter__()


# ---- the layers take it by address --------------------------------------------------------------------------------------
H, W, FRAMES = 48, 64, 5


class HostSource:
    """PixmapSourceInterface stand-in over a host array."""

    def __init__(self, array, introduction_mask):
        self.array, self.introduction_mask, self.counter = array, introduction_mask, -1

    def next(self, timeout=1):
        self.counter += 1
        return self.array

    @property
    def frame_number(self):
        return self.counter


def _flows(seed, n=FRAMES):
    from oracle import remap_ref as OR
    rng = np.random.default_rng(seed)
    return [OR.post_process((rng.normal(0, 2.5, (H, W, 2))).astype(np.float32), OR.BACKWARD) for _ in range(n)]


def _masks(two):
    if not two:
        return [np.ones((H, W), bool)]
    left = np.zeros((H, W), bool)
    left[:, :W // 2 + 3] = True
    lower = np.zeros((H, W), bool)
    lower[H // 3:, 5:] = True
    return [left, lower]


def _refuse_uploads(monkeypatch):
    """In the device run the host forms of the pixmap entry points raise: nothing can have gone up."""
    from transflow_amd import _lib
    lib = _lib.load()

    def refuse(name):
        def raiser(*args):
            raise AssertionError(f"{name} was called: a pixmap was uploaded")
        return raiser
    for name in ("tf_remap_gather", "tf_remap_gather_beside", "tf_remap_stage_pixmap", "tf_remap_introduce"):
        monkeypatch.setattr(lib, name, refuse(name))


def _device_flows(flows):
    from transflow_amd.device import DevBuffer
    from transflow_amd.deviceflow import DeviceFlow, _Event
    out = []
    for f in flows:
        buf = DevBuffer.from_array(f)
        ev = _Event()
        ev.record()
        flow = DeviceFlow(f.shape, buf.ptr, ev, owner=buf)
        flow.in_frame = True                 # clipped by post_process: the one-launch step may take it
        out.append(flow)
    return out


def _run_compositor(classname, sources, flows, seed=7, **cfg):
    """frames, data and rgba after every frame."""
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    comp = HipCompositor.from_args(H, W, [LayerConfig(0, classname=classname, **cfg)], background_color="#204060")
    comp.set_sources({0: sources})
    layer = comp.layers[0]
    saved = np.random.get_state()
    np.random.seed(seed)
    out = []
    try:
        for flow in flows:
            comp.update(flow)
            frame = np.array(comp.render())
            data = None if classname == "static" else np.array(layer.data)
            out.append((frame, data, np.array(layer.rgba)))
    finally:
        np.random.set_state(saved)
        comp.close()
    return out


def _pixmap_sources(P, kinds):
    """Entered sources, one per kind; "rgba" is a 4-channel image made from a noise."""
    out = []
    for k, kind in enumerate(kinds):
        if kind == "rgba":
            rng = np.random.default_rng(30 + k)
            a = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
            a[:, :, 3] = np.where(rng.random((H, W)) < 0.3, 0, 255)

            class Rgba(P.HipStillPixmapSource):
                def _init_array(self, a=a):
                    return a
            out.append(Rgba().__enter__())
        elif kind == "gradient":
            out.append(P.HipGradientPixmapSource(W, H, 3 + k).__enter__())
        elif kind == "color":
            out.append(P.HipColorPixmapSource(W, H, "#c08040").__enter__())
        else:
            out.append(P.HipColoredNoisePixmapSource(W, H, 11 + k).__enter__())
    return out


LAYER_CASES = [
    ("moveref_rgb", "moveref", ["cnoise"], {}),
    ("moveref_rgba", "moveref", ["rgba"], {}),
    ("moveref_reset_random_gradient", "moveref", ["gradient"], dict(reset_mode="random", reset_random_factor=0.2)),
    ("moveref_two_sources_two_masks", "moveref", ["cnoise", "rgba"], dict(reset_mode="linear", reset_source=True)),
    ("sum_rgb", "sum", ["cnoise"], {}),
    ("sum_two_sources_rgba", "sum", ["rgba", "gradient"], dict(reset_mode="constant", reset_constant_step=2)),
    ("static_rgb", "static", ["gradient"], {}),
    ("static_two_sources_rgba", "static", ["color", "rgba"], {}),
    ("introduction_rgb", "introduction", ["cnoise"], {}),
    ("introduction_rgba_two_sources", "introduction", ["rgba", "cnoise"], dict(moving_pixels_leave_empty_spot=True)),
    ("introduction_once", "introduction", ["cnoise"], dict(introduce_once=True)),
]


def _assert_same_runs(host, dev):
    assert len(host) == len(dev) == FRAMES
    for t, ((f0, d0, r0), (f1, d1, r1)) in enumerate(zip(host, dev)):
        np.testing.assert_array_equal(f1, f0, err_msg=f"frame {t}")
        if d0 is not None:
            np.testing.assert_array_equal(d1, d0, err_msg=f"data {t}")
        np.testing.assert_array_equal(r1, r0, err_msg=f"rgba {t}")


@pytest.mark.parametrize("name,classname,kinds,cfg", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_layers_take_device_pixmaps_by_address(name, classname, kinds, cfg, monkeypatch):
    from transflow_amd import pixmap as P
    sources = _pixmap_sources(P, kinds)
    masks = _masks(len(kinds) == 2)
    flows = _flows(5)
    try:
        host = _run_compositor(classname, [HostSource(np.array(next(s)), m) for s, m in zip(sources, masks)], flows, **cfg)
        assert host[0][0].shape == (H, W, 3)
        assert classname == "static" or (host[0][0] != host[-1][0]).any()        # the flows do move something
        with monkeypatch.context() as mp:
            _refuse_uploads(mp)
            interfaces = [P.HipPixmapInterface(s, m) for s, m in zip(sources, masks)]
            dev = _run_compositor(classname, interfaces, flows, **cfg)
        _assert_same_runs(host, dev)
        if cfg.get("introduce_once"):
            assert [i.counter for i in interfaces] == [0]            # asked for one frame only (introduction.py:21-22)
        else:
            assert [i.counter for i in interfaces] == [FRAMES - 1] * len(kinds)
    finally:
        for s in sources:
            s.__exit__(None, None, None)


@pytest.mark.parametrize("kind", ["cnoise", "rgba"])
def test_one_launch_step_reads_the_device_pixmap(kind, monkeypatch):
    """A lone moveref layer, one source, DeviceFlows: update() defers and render() runs tf_remap_step_dev -- with the
    pixmap's own address, nothing staged."""
    from transflow_amd import _lib
    from transflow_amd import pixmap as P
    lib = _lib.load()
    (source,) = _pixmap_sources(P, [kind])
    flows = _flows(9)
    try:
        mask = np.ones((H, W), bool)
        host = _run_compositor("moveref", [HostSource(np.array(next(source)), mask)], flows)
        host_dev_flows = _run_compositor("moveref", [HostSource(np.array(next(source)), mask)], _device_flows(flows))
        _assert_same_runs(host, host_dev_flows)
        steps = []
        real = lib.tf_remap_step_dev
        with monkeypatch.context() as mp:
            _refuse_uploads(mp)
            mp.setattr(lib, "tf_remap_step_dev", lambda *a: steps.append(a[6].value) or real(*a))
            dev = _run_compositor("moveref", [P.HipPixmapInterface(source, mask)], _device_flows(flows))
        _assert_same_runs(host, dev)
        assert steps == [next(source).dev_ptr] * FRAMES
    finally:
        source.__exit__(None, None, None)


def test_layer_refuses_a_device_pixmap_of_another_size():
    from transflow_amd import pixmap as P
    from transflow_amd.remap import RemapLayer
    layer = RemapLayer(H, W)
    layer.set_sources([np.ones((H, W), np.uint8)])
    with P.HipColorPixmapSource(W + 1, H, "#010203") as s:
        for call in (lambda: layer.gather(0, next(s)), lambda: layer.stage_pixmap(next(s)), lambda: layer.introduce(0, next(s), 0)):
            with pytest.raises(ValueError):
                call()
    layer.close()


def test_pixmap_made_on_a_worker_threads_stream_is_consumed_from_another(monkeypatch):
    """The prefetch layout: a worker thread with a library stream of its own makes the pixmap (the gradient's launch
    and its event are on that stream); the main thread's layers wait for the event on the device and read it."""
    from transflow_amd import _lib
    from transflow_amd import pixmap as P
    made = {}

    def worker():
        try:
            _lib.check(_lib.load().tf_thread_stream(1))
            made["source"] = P.HipGradientPixmapSource(W, H, 17).__enter__()
        except BaseException as err:       # noqa: BLE001
            made["error"] = err

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert "error" not in made, made.get("error")
    source = made["source"]
    want = px_ref.gradient(H, W, 17)
    flows = _flows(13)
    mask = np.ones((H, W), bool)
    try:
        with monkeypatch.context() as mp:
            _refuse_uploads(mp)
            dev = _run_compositor("moveref", [P.HipPixmapInterface(source, mask)], flows)
        host = _run_compositor("moveref", [HostSource(want, mask)], flows)
        _assert_same_runs(host, dev)
        np.testing.assert_array_equal(np.asarray(next(source)), want)
    finally:
        source.__exit__(None, None, None)
