"""Random reset with rng="mt19937": the compositor draws numpy's own stream on the device (transflow_amd/mtstream.py) and
gives the frames, layer states and following host draws of rng="numpy", byte for byte."""
import sys
import types

import numpy as np
import pytest

from oracle import remap_ref as R

H, W, FRAMES = 40, 64, 5


class Source:
    """PixmapSourceInterface stand-in (pixmap_source_interface.py:12-37)."""

    def __init__(self, frames, introduction_mask):
        self.frames, self.introduction_mask, self.counter = list(frames), introduction_mask, -1

    def next(self, timeout=1):
        self.counter += 1
        return self.frames[self.counter % len(self.frames)]


def _inputs():
    rng = np.random.default_rng(12)
    flows = [R.post_process(rng.normal(0, 2.5, (H, W, 2)).astype(np.float32), R.BACKWARD) for _ in range(FRAMES)]
    pix = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    reset_mask = rng.random((H, W)).astype(np.float32)
    return flows, pix, reset_mask


def _run(rngs, seed=77, lone=False, device_flows=False, reseed_at=None):
    """Five frames of the two-layer compositor (or the lone moveref layer) with one rng per layer: frames, every layer's
    data and rgba, and the eight values numpy draws on the host afterwards."""
    from transflow_amd.compositor import LAYER_CLASSES, HipCompositor
    from transflow_amd.config import LayerConfig
    from transflow_amd.device import DevBuffer
    from transflow_amd.deviceflow import DeviceFlow
    from transflow_amd.mtstream import Mt19937Stream
    flows, pix, reset_mask = _inputs()
    configs = [LayerConfig(0, classname="moveref", reset_mode="random", reset_random_factor=0.3)]
    if not lone:
        configs.append(LayerConfig(1, classname="sum", reset_mode="random", reset_random_factor=0.5, reset_source=True))
    layers = [LAYER_CLASSES[c.classname](c, H, W, [], rng=r) for c, r in zip(configs, rngs)]
    layers[0].reset_mask = reset_mask
    comp = HipCompositor(H, W, layers, "#204060")
    ones = np.ones((H, W), bool)
    comp.set_sources({0: [Source(pix, ones)], 1: [Source(pix[::-1], ones)]})
    np.random.seed(seed)
    frames, kept = [], []
    try:
        for t, flow in enumerate(flows):
            if t == reseed_at:
                np.random.seed(seed + 1)
            if device_flows:
                buf = DevBuffer.from_array(flow)
                kept.append(buf)
                flow = DeviceFlow(flow.shape, buf.ptr, None, owner=buf)
                flow.in_frame = True
            comp.update(flow)
            if lone and device_flows and rngs[0] != "numpy":
                assert layers[0]._deferred is not None          # the frame waits for render(): the one-launch step
            frames.append(np.array(comp.render()))
        states = [(layer.data.copy(), np.array(layer.rgba)) for layer in layers]
        Mt19937Stream.sync_active()
        tail = np.random.random(8)
    finally:
        comp.close()
        for buf in kept:
            buf.close()
    return frames, states, tail


def _same(a, b):
    for t, (x, y) in enumerate(zip(a[0], b[0])):
        assert x.tobytes() == y.tobytes(), f"frame {t}"
    for i, ((d0, r0), (d1, r1)) in enumerate(zip(a[1], b[1])):
        assert d0.tobytes() == d1.tobytes(), f"data of layer {i}"
        assert r0.tobytes() == r1.tobytes(), f"rgba of layer {i}"
    assert a[2].tobytes() == b[2].tobytes(), "numpy's draws afterwards"


@pytest.fixture(scope="module")
def numpy_route():
    return _run(("numpy", "numpy"))


@pytest.mark.gpu
def test_two_layers(numpy_route):
    _same(numpy_route, _run(("mt19937", "mt19937")))


@pytest.mark.gpu
@pytest.mark.parametrize("rngs", [("numpy", "mt19937"), ("mt19937", "numpy")])
def test_mixed_layers(numpy_route, rngs):
    _same(numpy_route, _run(rngs))


@pytest.mark.gpu
def test_resets_happen(numpy_route):
    """The comparison is not of layers nothing resets: with the reset off the frames differ."""
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    flows, pix, _ = _inputs()
    comp = HipCompositor.from_args(H, W, [LayerConfig(0), LayerConfig(1, classname="sum")], "#204060")
    ones = np.ones((H, W), bool)
    comp.set_sources({0: [Source(pix, ones)], 1: [Source(pix[::-1], ones)]})
    for flow in flows:
        comp.update(flow)
        frame = np.array(comp.render())
    comp.close()
    assert frame.tobytes() != numpy_route[0][-1].tobytes()


@pytest.mark.gpu
def test_lone_layer_on_device_flows_takes_the_one_launch_step():
    _same(_run(("numpy",), lone=True, device_flows=True), _run(("mt19937",), lone=True, device_flows=True))


@pytest.mark.gpu
def test_lone_layer_on_host_flows():
    _same(_run(("numpy",), lone=True), _run(("mt19937",), lone=True))


@pytest.mark.gpu
def test_seed_between_frames_is_picked_up():
    _same(_run(("numpy", "numpy"), reseed_at=3), _run(("mt19937", "mt19937"), reseed_at=3))
    _same(_run(("numpy",), lone=True, device_flows=True, reseed_at=2), _run(("mt19937",), lone=True, device_flows=True, reseed_at=2))


@pytest.mark.gpu
def test_checkpoint_syncs_the_stream():
    """Pickling a layer writes the stream's position into numpy's state: the process that resumes draws on from there."""
    import pickle

    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    flows, pix, _ = _inputs()
    tails = []
    for rng in ("numpy", "mt19937"):
        comp = HipCompositor.from_args(H, W, [LayerConfig(0, reset_mode="random", reset_random_factor=0.3)], rng=rng)
        comp.set_sources({0: [Source(pix, np.ones((H, W), bool))]})
        np.random.seed(5)
        for flow in flows[:3]:
            comp.update(flow)
            comp.render()
        for layer in comp.layers:
            layer.sources = []
        blob = pickle.dumps(comp)
        tails.append((np.random.random(8).tobytes(), pickle.loads(blob).layers[0]._pending_state[0].tobytes()))
        comp.close()
    assert tails[0] == tails[1]


def test_unknown_rng_is_refused():
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    with pytest.raises(ValueError, match="rng"):
        HipCompositor.from_args(8, 8, [LayerConfig(0)], rng="pcg64")
    for rng in ("numpy", "device", "mt19937"):
        assert HipCompositor.from_args(8, 8, [LayerConfig(0)], rng=rng).layers[0].rng == rng


@pytest.fixture
def stub_transflow():
    """Just enough of the reference's package for dropin.install(flow=False) to patch."""
    saved = {k: v for k, v in sys.modules.items() if k == "transflow" or k.startswith("transflow.")}
    for name in saved:
        del sys.modules[name]

    class Compositor:
        @classmethod
        def from_args(cls, height, width, layer_configs, background_color="#ffffff"):
            return "the reference's"

    names = {"transflow": {}, "transflow.compositor": {}, "transflow.compositor.compositor": {"Compositor": Compositor}}
    for name, attrs in names.items():
        mod = types.ModuleType(name)
        mod.__path__ = []
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
    try:
        yield Compositor
    finally:
        for name in names:
            sys.modules.pop(name, None)
        sys.modules.update(saved)


def test_dropin_reset_rng_reaches_from_args(stub_transflow):
    from transflow_amd import dropin
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    Comp = stub_transflow
    original = Comp.__dict__["from_args"]
    configs = [LayerConfig(0, reset_mode="random"), LayerConfig(1, classname="sum", reset_mode="random")]
    with pytest.raises(ValueError, match="reset_rng"):
        dropin.install(flow=False, reset_rng="pcg64")
    assert Comp.__dict__["from_args"] is original
    dropin.install(flow=False, reset_rng="mt19937")
    try:
        comp = Comp.from_args(8, 8, configs)
        assert isinstance(comp, HipCompositor) and [layer.rng for layer in comp.layers] == ["mt19937", "mt19937"]
    finally:
        dropin.uninstall()
    assert Comp.__dict__["from_args"] is original
    dropin.install(flow=False)                      # the default: "numpy" layers, as before
    try:
        comp = Comp.from_args(8, 8, configs)
        assert isinstance(comp, HipCompositor) and [layer.rng for layer in comp.layers] == ["numpy", "numpy"]
    finally:
        dropin.uninstall()
