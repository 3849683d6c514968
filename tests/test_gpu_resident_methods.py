"""`hip_resident`: Horn-Schunck, Lucas-Kanade and LiteFlowNet flows -- and Farnebäck's with OPTFLOW_USE_INITIAL_FLOW --
stay on the device through the post-process, and so does the previous output a chaining call starts from.  Every case is
a three-way comparison in the idiom of the methods' test_flow_source_matches_host_loop: the source with hip_resident, the
same source without it (the route before the key existed), and a host loop over the method's numpy restatement.

The chain state is the reference's `prev_flow` (source.py:314-321, 337-363): the post-processed flow, or -- with a mask,
whose multiply makes a new array -- the flow after the filters and before the mask."""
import numpy as np
import pytest

from oracle import remap_ref as R
from tests import hs_ref, lk_ref
from tests.helpers import synth_pair

gpu = pytest.mark.gpu
H, W = 60, 84


def _bits(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32).view(np.uint32)


def _frames(h, w, n, seed=5):
    return [synth_pair(h, w, seed=seed, shift=(0.8 * i, 0.5 * i))[1] for i in range(n)]


def _run(frames, cfg, host_next=None, host_post=None, **kw):
    """The flows of a HipFlowSource over `frames`, as host arrays.  host_next / host_post: the source's next() /
    post_process() are replaced by these (functions of the source, ...): the host loop."""
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    with HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), cv_config=cfg, **kw) as source:
        if host_next is not None:
            body = {"next": host_next}
            if host_post is not None:
                body["post_process"] = host_post
            source.__class__ = type("HostLoop", (HipFlowSource,), body)
        return [np.array(f, copy=True) for f in source]


def _pair_of(source, frame):
    """(left, right) of cv.py:467-472 for the frame just read; the frame becomes the previous one."""
    from transflow_amd.flow import FlowSource
    prev = source._prev_frame
    source._prev_frame = frame
    return (prev, frame) if source.direction == FlowSource.Direction.FORWARD else (frame, prev)


def _host_next(calc):
    def next(self):
        frame = self.provider.read()
        if frame is None:
            raise StopIteration
        left, right = _pair_of(self, frame)
        return calc(self, left, right)
    return next


def _reference_post_process(self, raw):
    """source.py:337-363 by the oracle: the filters in place on `raw` (which is prev_flow), the mask a new array."""
    ops = [(f.name, f.expr(self.t)) for f in self.flow_filters]
    return R.post_process(R.pre_steps(raw, ops, self.mask), self.direction.value)


def _same(got, exp, what):
    assert len(got) == len(exp), what
    for k, (g, e) in enumerate(zip(got, exp)):
        np.testing.assert_array_equal(_bits(g), _bits(e), err_msg=f"{what}, flow {k}")


# ---- Horn-Schunck ----------------------------------------------------------------------------------------------------

def _hs_calc(cfg):
    return lambda self, left, right: hs_ref.horn_schunck(
        left, right, self.prev_flow.copy() if self.prev_flow is not None else None, **cfg.hs_kwargs())


def _hs_cfg(decay, **kw):
    from transflow_amd.config import HornSchunckConfig
    return HornSchunckConfig(hs_decay=decay, hs_iterations=6, hs_delta=0.5, **kw)


@gpu
@pytest.mark.parametrize("repeat", [1, 2])
@pytest.mark.parametrize("decay", [0, 0.95])
@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_horn_schunck_three_ways(direction, decay, repeat):
    frames = _frames(H, W, 5)
    kw = dict(direction=direction, repeat=repeat)
    resident = _run(frames, _hs_cfg(decay, hip_resident=True), **kw)
    plain = _run(frames, _hs_cfg(decay), **kw)
    host = _run(frames, _hs_cfg(decay), _host_next(_hs_calc(_hs_cfg(decay))), _reference_post_process, **kw)
    assert len(resident) == 4 * repeat
    _same(resident, plain, "resident against the host route")
    _same(resident, host, "resident against the restatement")
    if repeat == 2:        # the rewind dropped the chain: the second pass starts from flow=None like the first
        _same(resident[4:], resident[:4], "second pass")


# The case that tells the two chain states apart: a scale filter and a mask that is zero over the left half, where the
# flow is not.  prev_flow is the scaled flow BEFORE the mask.
MASK_FILTERS = "scale=1.5"


def _half_mask(tmp_path):
    import PIL.Image
    mask = np.zeros((H, W), np.uint8)
    mask[:, W // 2:] = 255
    path = str(tmp_path / "half.png")
    PIL.Image.fromarray(mask).save(path)
    return path, (mask / np.float32(255)).astype(np.float32)[..., None]


def _hs_host_chain(frames, cfg, mask, from_masked: bool):
    """The recurrence on the CPU with hs_ref alone, BACKWARD: chaining from the filtered flow (the reference) or from
    the masked output (what a chain buffer filled after the mask would hold)."""
    prev, out = None, []
    for t in range(1, len(frames)):
        raw = hs_ref.horn_schunck(frames[t], frames[t - 1], None if prev is None else prev.copy(), **cfg.hs_kwargs())
        filtered = R.pre_steps(raw, [("scale", 1.5)], None)
        final = R.post_process(R.pre_steps(filtered, (), mask), R.BACKWARD)
        out.append(final)
        prev = final if from_masked else filtered
    return out


def test_masked_chain_inputs_tell_the_two_chain_states_apart(tmp_path):
    """No GPU: with these inputs, chaining from the MASKED flow gives other bits than the reference's recurrence -- so
    the GPU test below can fail for the reason it exists."""
    frames = _frames(H, W, 5)
    _, mask = _half_mask(tmp_path)
    cfg = _hs_cfg(0.95)
    right = _hs_host_chain(frames, cfg, mask, from_masked=False)
    wrong = _hs_host_chain(frames, cfg, mask, from_masked=True)
    first = R.pre_steps(hs_ref.horn_schunck(frames[1], frames[0], None, **cfg.hs_kwargs()), [("scale", 1.5)], None)
    assert (right[0][:, :W // 2] == 0).all() and (first[:, :W // 2] != 0).any()   # the mask hides flow that is there
    assert np.array_equal(_bits(right[0]), _bits(wrong[0]))                       # (the first call has no chain)
    assert any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(right[1:], wrong[1:]))


@gpu
@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_horn_schunck_chain_is_the_flow_before_the_mask(tmp_path, direction):
    frames = _frames(H, W, 5)
    path, mask = _half_mask(tmp_path)
    kw = dict(direction=direction, repeat=2, flow_filters=MASK_FILTERS, mask_path=path)
    resident = _run(frames, _hs_cfg(0.95, hip_resident=True), **kw)
    plain = _run(frames, _hs_cfg(0.95), **kw)
    host = _run(frames, _hs_cfg(0.95), _host_next(_hs_calc(_hs_cfg(0.95))), _reference_post_process, **kw)
    _same(resident, plain, "resident against the host route")
    _same(resident, host, "resident against the restatement")
    if direction == "backward":
        _same(resident[:4], _hs_host_chain(frames, _hs_cfg(0.95), mask, from_masked=False), "the CPU recurrence")


@gpu
def test_horn_schunck_initial_flow_from_a_device_address():
    """tf_hs_set_initial_flow_dev against tf_hs_set_initial_flow: a batch of two pairs, one with an initial flow and one
    without, at an odd size."""
    from transflow_amd.device import DevBuffer
    from transflow_amd.hornschunck import HornSchunck
    h, w = 37, 53
    frames = _frames(h, w, 3, seed=9)
    init = np.random.default_rng(3).normal(0, 1.5, (h, w, 2)).astype(np.float32)
    init[::3, ::2] = np.float32(-0.0)
    hs = HornSchunck(w, h, frame_slots=3, max_pairs=2)
    dev = DevBuffer.from_array(init)
    try:
        for k, f in enumerate(frames):
            hs.set_frame(k, f)
        results = []
        for from_device in (False, True):
            for with_init in ((True, False), (False, True)):
                for pair, on in enumerate(with_init):
                    if from_device:
                        hs.set_initial_flow_dev(pair, dev.ptr if on else None)
                    else:
                        hs.set_initial_flow(pair, init if on else None)
                hs.calc_slots([0, 1], [1, 2], max_iters=5, decay=0.95, delta=None)
                results.append([hs.get_flow(0), hs.get_flow(1)])
        for host, device in zip(results[:2], results[2:]):
            for a, b in zip(host, device):
                np.testing.assert_array_equal(_bits(a), _bits(b))
        assert not np.array_equal(_bits(results[2][0]), _bits(results[3][0]))     # (the initial flow matters)
        # an initial flow serves one call: the next one runs the float64 chain again
        hs.calc_slots([0, 1], [1, 2], max_iters=5, decay=0.95, delta=None)
        np.testing.assert_array_equal(_bits(hs.get_flow(0)), _bits(results[3][0]))
        with pytest.raises(ValueError):
            hs.set_initial_flow_dev(2, dev.ptr)
        with pytest.raises(ValueError):
            hs.set_initial_flow_dev(0, dev.ptr + 4)
    finally:
        hs.close()
        dev.close()


# ---- Lucas-Kanade ----------------------------------------------------------------------------------------------------

def _lk_cfg(**kw):
    from transflow_amd.config import LucasKanadeConfig
    return LucasKanadeConfig(lk_window_size=9, lk_max_level=2, lk_step=4, **kw)


def _ramp_mask(tmp_path, h, w):
    import PIL.Image
    path = str(tmp_path / "ramp.png")
    PIL.Image.fromarray((np.add.outer(np.arange(h), np.arange(w)) * 255 // (h + w)).astype(np.uint8)).save(path)
    return path


@gpu
@pytest.mark.parametrize("repeat", [1, 2])
@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_lucas_kanade_three_ways(tmp_path, direction, repeat):
    frames = _frames(H, W, 5)
    kw = dict(direction=direction, repeat=repeat, flow_filters="scale=2;clip=6", mask_path=_ramp_mask(tmp_path, H, W))
    calc = lambda self, left, right: lk_ref.lukas_kanade(left, right, **_lk_cfg().lk_kwargs())    # noqa: E731
    resident = _run(frames, _lk_cfg(hip_resident=True), **kw)
    _same(resident, _run(frames, _lk_cfg(), **kw), "resident against the host route")
    _same(resident, _run(frames, _lk_cfg(), _host_next(calc), **kw), "resident against the restatement")
    _same(resident, _run(frames, _lk_cfg(hip_resident=True, hip_batch=3), **kw), "a batch of three against one")
    assert len(resident) == 4 * repeat


# ---- LiteFlowNet -----------------------------------------------------------------------------------------------------
LFN_H, LFN_W = 40, 46      # the smallest size of tests/test_gpu_liteflownet.py (the network cannot run at 32 px or less)


def _lfn_setup():
    from tests import lfn_ref
    weights = lfn_ref.synthetic_weights(3, 0.25)[0]
    frames = [lfn_ref.textured_pair(LFN_H, LFN_W, 30, (i, 2 * i))[0] for i in range(5)]
    return lfn_ref, weights, frames


@gpu
@pytest.mark.parametrize("repeat", [1, 2])
@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_liteflownet_resident_equals_the_host_route(tmp_path, direction, repeat):
    from transflow_amd.config import LiteFlowNetConfig
    _, weights, frames = _lfn_setup()
    kw = dict(direction=direction, repeat=repeat, flow_filters="scale=2;clip=6", mask_path=_ramp_mask(tmp_path, LFN_H, LFN_W))
    resident = _run(frames, LiteFlowNetConfig(weights=weights, hip_resident=True), **kw)
    _same(resident, _run(frames, LiteFlowNetConfig(weights=weights), **kw), "resident against the host route")
    _same(resident, _run(frames, LiteFlowNetConfig(weights=weights, hip_resident=True, hip_batch=3), **kw), "a batch of three")
    assert len(resident) == 4 * repeat


@gpu
def test_liteflownet_resident_within_the_restatement_bound():
    """Against a host loop over lfn_ref, BACKWARD and without filters (the clip to the frame is 1-Lipschitz, so the
    bound of tests/test_gpu_liteflownet.py's _check_network holds for the post-processed flow as for the raw one)."""
    import torch

    from transflow_amd.config import LiteFlowNetConfig
    lfn_ref, weights, frames = _lfn_setup()
    resident = _run(frames, LiteFlowNetConfig(weights=weights, hip_resident=True), direction="backward")
    assert len(resident) == 4
    for t, got in enumerate(resident):
        f64 = lfn_ref.estimate(weights, frames[t + 1], frames[t], torch.float64)
        f32 = lfn_ref.estimate(weights, frames[t + 1], frames[t], torch.float32)
        exp64 = R.post_process(np.ascontiguousarray(f64, dtype=np.float32), R.BACKWARD).astype(np.float64)
        exp32 = R.post_process(np.ascontiguousarray(f32, dtype=np.float32), R.BACKWARD)
        ref_err = float(np.abs(exp32 - exp64).max())
        err = float(np.abs(got - exp64).max())
        bound = 4 * ref_err + 1e-5 * max(1.0, float(np.abs(exp64).max()))
        print(f"flow {t}: max|gpu - f64| {err:.3g}, bound {bound:.3g}")
        assert err <= bound, f"flow {t}: {err:.3g} > {bound:.3g}"


# ---- Farnebäck with OPTFLOW_USE_INITIAL_FLOW ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("repeat", [1, 2])
@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_farneback_initial_flow_three_ways(direction, repeat):
    """In the exact mode (hip_exact_sums), whose flows are the CPU path's bit for bit: the default mode's tests compare
    within a tolerance."""
    from oracle import farneback as OF
    from transflow_amd.config import FlowConfig
    h, w = 120, 160
    frames = _frames(h, w, 5)
    kw = dict(direction=direction, repeat=repeat, flow_filters="scale=2")      # (the frames move by less than a pixel)
    calc = lambda self, left, right: OF.calc(left, right, flags=4, flow=self.prev_flow)      # noqa: E731
    cfg = dict(fb_flags=4, hip_exact_sums=True)
    resident = _run(frames, FlowConfig(hip_resident=True, **cfg), **kw)
    assert len(resident) == 4 * repeat
    _same(resident, _run(frames, FlowConfig(**cfg), **kw), "resident against the host route")
    _same(resident, _run(frames, FlowConfig(hip_resident=True, hip_batch=3, **cfg), **kw), "hip_batch on a chaining source")
    host = _run(frames, FlowConfig(**cfg), _host_next(calc), _reference_post_process, **kw)
    for k, (g, e) in enumerate(zip(resident, host)):
        print(f"flow {k}: max|resident - restatement| {float(np.abs(g - e).max()):.3g}")
    _same(resident, host, "resident against the restatement")
    # and the chain is in use: it is not the plain recurrence
    plain = _run(frames, FlowConfig(hip_exact_sums=True), **kw)
    assert any((g != 0).any() for g in resident)
    if direction == "backward":      # (FORWARD's inverted field is whole pixels: the two recurrences can round alike)
        assert any(not np.array_equal(_bits(g), _bits(e)) for g, e in zip(resident[1:4], plain[1:4]))


# ---- what rides the resident tail ------------------------------------------------------------------------------------

def _configs():
    from tests import lfn_ref
    from transflow_amd.config import FlowConfig, LiteFlowNetConfig
    weights = lfn_ref.synthetic_weights(3, 0.25)[0]
    return {"horn-schunck": (lambda **kw: _hs_cfg(0.95, **kw), (H, W)),
            "lukas-kanade": (_lk_cfg, (H, W)),
            "liteflownet": (lambda **kw: LiteFlowNetConfig(weights=weights, **kw), (LFN_H, LFN_W)),
            "farneback": (lambda **kw: FlowConfig(fb_flags=4, hip_exact_sums=True, **kw), (120, 160))}


def _method_frames(method, h, w):
    if method == "liteflownet":
        return _lfn_setup()[2]
    return _frames(h, w, 5)


@gpu
@pytest.mark.parametrize("method,prefetch", [("horn-schunck", 0), ("horn-schunck", 2), ("lukas-kanade", 0), ("lukas-kanade", 2),
                                             ("liteflownet", 0), ("farneback", 0), ("farneback", 2)])   # (liteflownet takes no hip_prefetch)
def test_device_flows_of_every_method(method, prefetch):
    """hip_device_flows with hip_resident: DeviceFlows, in the frame, whose downloads are the host route's arrays and
    which a moveref compositor renders to the same frames."""
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    from transflow_amd.deviceflow import DeviceFlow
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    make, (h, w) = _configs()[method]
    frames = _method_frames(method, h, w)
    pix = np.random.default_rng(8).integers(0, 256, (h, w, 3), dtype=np.uint8)

    class Src:
        introduction_mask = np.ones((h, w), bool)

        def next(self, timeout=1):
            return pix

    def run(cfg):
        comp = HipCompositor.from_args(h, w, [LayerConfig(0)])
        comp.set_sources({0: [Src()]})
        flows, images = [], []
        with HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), direction="forward", cv_config=cfg, repeat=2,
                                     flow_filters="scale=1.5") as source:
            for flow in source:
                if cfg.hip_device_flows:
                    assert isinstance(flow, DeviceFlow) and flow.shape == (h, w, 2) and flow.in_frame
                comp.update(flow)
                images.append(comp.render().copy())
                flows.append(flow)
        return flows, images
    extra = {"hip_prefetch": prefetch} if prefetch else {}
    plain_flows, plain_images = run(make())
    dev_flows, dev_images = run(make(hip_resident=True, hip_device_flows=True, **extra))
    host_flows, _ = run(make(hip_resident=True, **extra))
    assert len(dev_flows) == len(plain_flows) == 8
    assert not any(f._host is not None for f in dev_flows)               # nothing came down: the compositor read HBM
    for a, b in zip(plain_images, dev_images):
        np.testing.assert_array_equal(a, b)
    _same([np.asarray(f) for f in dev_flows], plain_flows, "device flows")    # eight held, a ring of four: all intact
    _same(host_flows, plain_flows, "resident host arrays" + (" behind the worker thread" if prefetch else ""))


@gpu
@pytest.mark.parametrize("what", ["lock", "kernel"])
@pytest.mark.parametrize("method", ["horn-schunck", "lukas-kanade"])
def test_lock_or_kernel_takes_the_host_route(tmp_path, method, what):
    """A lock expression reads prev_flow on the host and a convolution kernel has no resident form: hip_resident then
    changes nothing, and a handle that would have run hip_batch pairs a call is opened for one."""
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    frames = _frames(H, W, 5)
    kw = dict(direction="backward")
    if what == "lock":
        kw.update(lock_expr="0.1,0.1", lock_mode="stay")
    else:
        path = str(tmp_path / "kernel.npy")
        np.save(path, np.random.default_rng(4).normal(0, 0.3, (3, 3)).astype(np.float32))
        kw.update(kernel_path=path)
    make = (lambda **keys: _hs_cfg(0.95, **keys)) if method == "horn-schunck" else _lk_cfg
    with HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), cv_config=make(hip_resident=True, hip_batch=3),
                                 **kw) as source:
        assert not source._resident_ok() and source._batch_size() == 1
        resident = [np.array(f, copy=True) for f in source]
        assert not source.chain_valid and (source._fb.frame_slots, source._fb.max_pairs) == (2, 1)
    plain = _run(frames, make(), **kw)
    assert len(resident) == len(plain) >= 4
    for g, e in zip(resident, plain):
        assert g.dtype == e.dtype
        np.testing.assert_array_equal(g, e)


@gpu
def test_chain_flag_follows_prev_flow():
    """chain_valid is set by the first resident post-process and cleared wherever prev_flow becomes None: rewind() and
    the prev_gray setter."""
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    frames = _frames(H, W, 5)
    with HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), direction="backward",
                                 cv_config=_hs_cfg(0.95, hip_resident=True, hip_batch=3)) as source:
        assert source._resident_ok() and source._batch_size() == 1 and not source.chain_valid
        first = np.array(next(source), copy=True)
        assert source.chain_valid and source.prev_flow is not None
        next(source)
        source.rewind()
        assert not source.chain_valid and source.prev_flow is None
        np.testing.assert_array_equal(_bits(next(source)), _bits(first))
        assert source.chain_valid
        source.prev_gray = frames[0]
        assert not source.chain_valid
