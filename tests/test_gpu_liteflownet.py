"""LiteFlowNet on the GPU (transflow_amd/liteflownet.py, csrc/liteflownet.hip) against the reference's own float32 output
(tests/golden/lfn_*.npz, tools/capture_golden_lfn.py) and the float64 restatement tests/lfn_ref.py.

Whole network: max|gpu - f64| <= 4 max|f32_ref - f64| + 1e-5 max(1, max|f64|), NaN positions equal.  Stages: each
against a float64 statement fed the GPU's own float32 inputs, with the bound its docstring derives; the correlation
bit for bit."""
import glob
import os

import numpy as np
import pytest

from tests.helpers import GOLDEN
from transflow_amd import liteflownet as LF
from transflow_amd.liteflownet import LiteFlowNet


class _Lazy:
    """A module imported at its first use: collecting this file must not import torch (tests/test_gpu_batch.py
    checks that the C ABI runs without it in the same session)."""

    def __init__(self, name):
        self._name = name

    def __getattr__(self, attr):
        if attr.startswith("_"):       # what pytest's collection probes (__test__, fixture markers): not the module's
            raise AttributeError(attr)
        import importlib
        return getattr(importlib.import_module(self._name), attr)


torch = _Lazy("torch")
F = _Lazy("torch.nn.functional")
lfn_ref = _Lazy("tests.lfn_ref")

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "lfn_*.npz")))
U = 2.0 ** -24
_W = {}


def weights(seed, gain):
    if (seed, gain) not in _W:
        _W[(seed, gain)] = lfn_ref.synthetic_weights(seed, gain)[0]
    return _W[(seed, gain)]


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_network(got, f64, f32_ref, what):
    assert got.dtype == np.float32 and got.shape == f64.shape
    assert np.array_equal(np.isnan(got), np.isnan(f64)), what
    ok = ~np.isnan(f64)
    ref_err = float(np.abs(f32_ref[ok] - f64[ok]).max()) if ok.any() else 0.0
    err = float(np.abs(got[ok] - f64[ok]).max()) if ok.any() else 0.0
    bound = 4 * ref_err + 1e-5 * max(1.0, float(np.abs(f64[ok]).max()))
    assert err <= bound, f"{what}: max|gpu - f64| {err:.3g} > {bound:.3g} (f32 reference {ref_err:.3g})"
    return err / ref_err if ref_err else 0.0


def _textured(h, w, seed, shift):
    return lfn_ref.textured_pair(h, w, seed, shift)


def test_fixtures_present():
    assert len(FIXTURES) >= 8


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[4:-4] for p in FIXTURES])
def test_matches_reference_fixture(path):
    z = np.load(path)
    one, two = z["prev"], z["next"]
    h, w = one.shape[:2]
    W, sha = lfn_ref.synthetic_weights(int(z["seed"]), float(z["gain"]))
    assert sha == str(z["sha256"])
    if "raises" in z:      # at 32 px or less the reference divides by zero: the handle refuses the size
        assert str(z["raises"]) == "ZeroDivisionError"
        with pytest.raises(ValueError):
            LiteFlowNet(w, h, W)
        return
    net = LiteFlowNet(w, h, W)
    got = net.calc(one, two)
    ratio = _check_network(got, z["flow64"], z["flow"], os.path.basename(path))
    print(f"{os.path.basename(path)}: error ratio {ratio:.3f}")


def _random_cases():
    rng = np.random.default_rng(2024)
    cases = []
    for seed in (1, 2, 3):
        for gain in (0.25, 1.0):
            for _ in range(10):
                h, w = (int(v) for v in rng.integers(33, 131, 2))
                cases.append((seed, gain, h, w, int(rng.integers(0, 1 << 30)), (int(rng.integers(-4, 5)), int(rng.integers(-4, 5)))))
    return cases


@pytest.mark.parametrize("seed,gain,h,w,fseed,shift", _random_cases())
def test_random_cases_match_restatement(seed, gain, h, w, fseed, shift):
    W = weights(seed, gain)
    one, two = _textured(h, w, fseed, shift)
    got = LiteFlowNet(w, h, W).calc(one, two)
    ratio = _check_network(got, lfn_ref.estimate(W, one, two, torch.float64),
                           lfn_ref.estimate(W, one, two, torch.float32), f"{h}x{w} seed {seed} gain {gain}")
    print(f"random {h}x{w} seed {seed} gain {gain}: error ratio {ratio:.3f}")


# ---- stages ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def net():
    return LiteFlowNet(64, 64, weights(1, 1.0))


def _conv64(x, layer, W):
    wt = torch.from_numpy(W[layer.name + ".weight"]).double()
    b = torch.from_numpy(W[layer.name + ".bias"]).double()
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    y = F.conv2d(xt, wt, b, stride=layer.stride, padding=(layer.ph, layer.pw))
    mag = F.conv2d(xt.abs(), wt.abs(), None, stride=layer.stride, padding=(layer.ph, layer.pw))
    return y.permute(0, 2, 3, 1).numpy(), mag.permute(0, 2, 3, 1).numpy(), np.abs(W[layer.name + ".bias"]).astype(np.float64)


CONV_LAYERS = [i for i, l in enumerate(LF.layers()) if not l.deconv]


@pytest.mark.parametrize("li", CONV_LAYERS, ids=[LF.layers()[i].name for i in CONV_LAYERS])
def test_stage_conv_every_layer(net, li):
    """Bound: the float32 sum of K products and a bias, in any order, is within (K + 2) 2^-24 (sum|w x| + |b|) of the
    exact value (each of the K + 1 additions and K products rounds once, relative 2^-24 of at most that magnitude);
    LeakyReLU does not increase the error; a residual adds one rounding of the result.  The inputs are a channel slice
    of a wider buffer and the output goes into a slice of one whose other channels must stay."""
    layer = LF.layers()[li]
    W = weights(1, 1.0)
    rng = np.random.default_rng(li)
    h, w = (11, 13) if layer.stride == 1 else (12, 15)
    extra_in, off_in = 3, 2
    x = rng.standard_normal((2, h, w, layer.cin + extra_in)).astype(np.float32)
    ho, wo = layer.out_size(h, w)
    out0 = rng.standard_normal((2, ho, wo, layer.cout + 4)).astype(np.float32)
    res = rng.standard_normal((2, ho, wo, layer.cout + 1)).astype(np.float32) if layer.cout == 2 else None
    got = net.stage_conv(li, x, out=out0, in_off=off_in, out_off=1, residual=res, res_off=1)
    assert np.array_equal(got[..., :1], out0[..., :1]) and np.array_equal(got[..., 1 + layer.cout:], out0[..., 1 + layer.cout:])
    y, mag, babs = _conv64(np.ascontiguousarray(x[..., off_in:off_in + layer.cin]), layer, W)
    if layer.leaky:
        y = np.where(y > 0, y, y * 0.1)
    bound = (layer.kh * layer.kw * layer.cin + 2) * U * (mag + babs)
    if res is not None:
        y = res[..., 1:1 + layer.cout].astype(np.float64) + y
        bound = bound + U * np.abs(y)
    g = got[..., 1:1 + layer.cout].astype(np.float64)
    err = np.abs(g - y)
    assert (err <= bound).all(), float((err / bound).max())
    assert float(np.median(err / np.maximum(mag, 1e-30))) <= 1e-6


@pytest.mark.parametrize("li", [i for i, l in enumerate(LF.layers()) if l.deconv])
def test_stage_deconv(net, li):
    """4 products and 3 additions per output: within 6 2^-24 sum|w x| of the exact value."""
    layer = LF.layers()[li]
    W = weights(1, 1.0)
    x = np.random.default_rng(li).standard_normal((2, 7, 9, layer.cout)).astype(np.float32)
    got = net.stage_deconv(li, x)
    wt = torch.from_numpy(W[layer.name + ".weight"]).double()
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    y = F.conv_transpose2d(xt, wt, None, stride=2, padding=1, groups=layer.cout).permute(0, 2, 3, 1).numpy()
    mag = F.conv_transpose2d(xt.abs(), wt.abs(), None, stride=2, padding=1, groups=layer.cout).permute(0, 2, 3, 1).numpy()
    assert (np.abs(got - y) <= 6 * U * mag + 1e-30).all()


@pytest.mark.parametrize("stride,c,h,w", [(1, 64, 9, 13), (1, 96, 6, 7), (1, 192, 4, 5), (2, 64, 13, 17), (2, 64, 12, 16)])
def test_stage_correlation_bit_exact(net, stride, c, h, w):
    rng = np.random.default_rng(c + h)
    one = rng.standard_normal((2, h, w, c)).astype(np.float32)
    two = rng.standard_normal((2, h, w, c)).astype(np.float32)
    got = net.stage_correlation(one, two, stride)
    exp = F.leaky_relu(lfn_ref.correlation(torch.from_numpy(one).permute(0, 3, 1, 2).contiguous(),
                                           torch.from_numpy(two).permute(0, 3, 1, 2).contiguous(), stride,
                                           torch.float32), 0.1).permute(0, 2, 3, 1).numpy()
    assert _bits_equal(got, np.ascontiguousarray(exp))


@pytest.mark.parametrize("scale", [10.0, 0.625])
def test_stage_backwarp(net, scale):
    """Against grid_sample in float64 on the same float32 inputs.  The sampling position is a handful of float32
    operations on values below w + |u s| (pixel units), so it is off by at most 2^-20 (w + |u s|) per axis; bilinear
    interpolation changes by at most 2 max|x| per pixel of position (neighbour differences), and its own 4 products and
    3 additions round within 2^-21 max|x|.  Flows reach well outside the frame."""
    rng = np.random.default_rng(int(scale * 8))
    n, h, w, c = 2, 10, 14, 5
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    flow = (rng.standard_normal((n, h, w, 2)) * 12 / scale).astype(np.float32)
    got = net.stage_backwarp(x, flow, scale)
    ft = torch.from_numpy(flow).permute(0, 3, 1, 2).double() * scale
    exp = lfn_ref.backwarp(torch.from_numpy(x).permute(0, 3, 1, 2).double(), ft).permute(0, 2, 3, 1).numpy()
    us = np.abs(flow.astype(np.float64) * scale)
    pos = 2.0 ** -20 * ((w + us[..., 0]) + (h + us[..., 1]))
    bound = np.abs(x).max() * (2 * pos + 2.0 ** -21)
    assert (np.abs(got - exp) <= bound[..., None]).all()
    assert (np.abs(flow * scale) > w).any()


@pytest.mark.parametrize("level", [2, 3, 5])
def test_stage_regularize_tail(net, level):
    """Against lfn_ref.regularize_tail in float64.  Each e_c = exp(-d_c^2 - max) is within a few ulps (the square, the
    subtraction, expf), so each term w_c e_c u_c and the sum of the e_c carry a relative error below 16 2^-24 each,
    and their k^2-term sums add k^2 roundings: |err| <= 64 k^2 2^-24 (sum_c |w_c| e_c |u_c| + |b|) / sum_c e_c."""
    k = LF.UNFOLD[level]
    W = weights(1, 1.0)
    rng = np.random.default_rng(level)
    n, h, w = 2, 9, 11
    dist = (rng.standard_normal((n, h, w, k * k)) * 1.5).astype(np.float32)
    flow = (rng.standard_normal((n, h, w, 2)) * 3).astype(np.float32)
    got = net.stage_regularize_tail(level, dist, flow)
    p = f"netRegularization.{level - 2}"
    wd = {s: torch.from_numpy(W[f"{p}.netScale{s}"]).double() for s in ("X.weight", "X.bias", "Y.weight", "Y.bias")}
    dt = torch.from_numpy(dist).permute(0, 3, 1, 2).double()
    ft = torch.from_numpy(flow).permute(0, 3, 1, 2).double()
    exp = lfn_ref.regularize_tail(dt, ft, wd["X.weight"], wd["X.bias"], wd["Y.weight"], wd["Y.bias"])
    exp = exp.permute(0, 2, 3, 1).numpy()
    d = -dt.square()
    e = (d - d.max(1, keepdim=True)[0]).exp()
    out = []
    for j, s in enumerate(("X", "Y")):
        ufl = F.unfold(ft[:, j:j + 1].abs(), kernel_size=k, padding=(k - 1) // 2).view_as(e)
        mag = F.conv2d(e * ufl, wd[s + ".weight"].abs(), wd[s + ".bias"].abs()) / e.sum(1, keepdim=True)
        out.append(mag)
    mag = torch.cat(out, 1).permute(0, 2, 3, 1).numpy()
    assert (np.abs(got - exp) <= 64 * k * k * U * mag).all()


def test_stage_prep_both_roles():
    """x 1/255, a bilinear resize (2 products and 1 addition per axis) and the mean: within 2^-20 of the float64
    statement (values below 1)."""
    h, w = 45, 61
    one, two = _textured(h, w, 3, (1, 1))
    net = LiteFlowNet(w, h, weights(1, 1.0))
    net.set_frame_bgr(0, one)
    net.set_frame_bgr(1, two)
    for slot, frame in ((0, one), (1, two)):
        for role in (0, 1):
            got = net.stage_prep(slot, role)
            exp = lfn_ref.prep(frame, role, torch.float64)[0].permute(1, 2, 0).numpy()
            assert got.shape == (64, 64, 3)
            assert np.abs(got - exp).max() <= 2.0 ** -20


def test_bgr_ingest_of_an_odd_size_frame():
    """A 53 x 37 decoded frame into a 61 x 45 slot: the INTER_NEAREST map (cv.py:464), then the same prep."""
    rng = np.random.default_rng(9)
    wide = rng.integers(0, 256, (37, 70, 3), dtype=np.uint8)
    src = wide[:, :53]                                       # rows 210 bytes apart: the row-strided upload
    assert src.strides == (210, 3, 1)
    h, w = 45, 61
    ys = np.minimum(np.floor(np.arange(h) * (1.0 / (h / 37))).astype(int), 36)
    xs = np.minimum(np.floor(np.arange(w) * (1.0 / (w / 53))).astype(int), 52)
    resized = src[ys][:, xs]
    net = LiteFlowNet(w, h, weights(1, 1.0))
    net.set_frame_bgr(0, src)
    exp = lfn_ref.prep(resized, 0, torch.float64)[0].permute(1, 2, 0).numpy()
    assert np.abs(net.stage_prep(0, 0) - exp).max() <= 2.0 ** -20


# ---- determinism, batches -------------------------------------------------------------------------------------------

def test_run_to_run_and_batch_of_4_bit_identical():
    h, w = 70, 100
    W = weights(2, 1.0)
    frames = [_textured(h, w, 20 + i, (i, -i))[0] for i in range(5)]
    net = LiteFlowNet(w, h, W, frame_slots=5, max_pairs=4)
    for s, f in enumerate(frames):
        net.set_frame_bgr(s, f)
    net.calc_slots([0, 1, 2, 3], [1, 2, 3, 4])
    batch = [net.get_flow(i) for i in range(4)]
    net.calc_slots([0, 1, 2, 3], [1, 2, 3, 4])
    assert all(_bits_equal(a, net.get_flow(i)) for i, a in enumerate(batch))
    for i in range(4):
        net.calc_slots([i], [i + 1])
        assert _bits_equal(net.get_flow(0), batch[i]), i
    net.calc_slots([3, 1], [2, 0])                       # roles swap: features are not reused across roles
    alone = LiteFlowNet(w, h, W)
    assert _bits_equal(net.get_flow(0), alone.calc(frames[3], frames[2]))
    assert _bits_equal(net.get_flow(1), alone.calc(frames[1], frames[0]))


def test_errors_are_codes():
    W = weights(1, 1.0)
    with pytest.raises(ValueError):
        LiteFlowNet(32, 64, W)
    net = LiteFlowNet(40, 40, W)
    with pytest.raises(ValueError):
        net.set_weights(np.zeros(10, np.float32))
    with pytest.raises(ValueError):
        net.calc_slots([0], [5])
    with pytest.raises(ValueError):
        net.get_flow(3)
    with pytest.raises(ValueError):
        net.set_frame(0, np.zeros((40, 40), np.uint8))


# ---- flow source and drop-in -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_flow_source_matches_handle_loop(tmp_path, direction):
    """HipFlowSource with a LiteFlowNetConfig, filters and a mask, against the same source whose next() calls a
    separate handle on the frames ordered by direction (cv.py:467-472); the post-process is the same on both."""
    import PIL.Image
    from transflow_amd.config import LiteFlowNetConfig
    from transflow_amd.flow import ArrayFrameProvider, FlowSource, HipFlowSource
    h, w = 48, 72
    W = weights(3, 0.25)
    frames = [_textured(h, w, 30, (i, 2 * i))[0] for i in range(4)]
    cfg = LiteFlowNetConfig(weights=W)
    mask = (np.add.outer(np.arange(h), np.arange(w)) * 255 // (h + w)).astype(np.uint8)
    mask_path = str(tmp_path / "mask.png")
    PIL.Image.fromarray(mask).save(mask_path)
    handle = LiteFlowNet(w, h, W)

    class HandleLoop(HipFlowSource):
        def next(self):
            frame = self.provider.read()
            if frame is None:
                raise StopIteration
            prev = self._prev_frame
            left, right = (prev, frame) if self.direction == FlowSource.Direction.FORWARD else (frame, prev)
            self._prev_frame = frame
            return handle.calc(left, right)

    kw = dict(direction=direction, cv_config=cfg, flow_filters="scale=2;clip=6", mask_path=mask_path)
    with HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), **kw) as source:
        got = [f.copy() for f in source]
    with HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), **kw) as oracle:
        oracle.__class__ = HandleLoop
        exp = [f.copy() for f in oracle]
    assert len(got) == len(exp) >= 3
    for g, e in zip(got, exp):
        assert _bits_equal(g, e)


def test_flow_source_refuses_grey_frames():
    from transflow_amd.config import LiteFlowNetConfig
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    frames = [np.zeros((40, 40), np.uint8)] * 3
    with HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), cv_config=LiteFlowNetConfig(weights=weights(1, 1.0))) as s:
        with pytest.raises(ValueError):
            next(iter(s))


def test_dropin_install_serves_liteflownet_with_weights(tmp_path):
    import json
    import sys
    import types
    from transflow_amd import dropin
    from transflow_amd.config import LiteFlowNetConfig
    from transflow_amd.flow import HipFlowSource

    class RefFlowSource:
        @classmethod
        def from_args(cls, flow_path, **kw):
            return "reference"

    mods = {name: types.ModuleType(name) for name in
            ("transflow", "transflow.flow", "transflow.flow.sources", "transflow.flow.sources.source")}
    mods["transflow.flow.sources.source"].FlowSource = RefFlowSource
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    path = str(tmp_path / "liteflownet.json")
    with open(path, "w") as f:
        json.dump({"method": "liteflownet"}, f)
    W = weights(1, 1.0)
    try:
        dropin.install(flow=True, compositor=False, liteflownet=W)
        b = RefFlowSource.from_args("clip.mp4", cv_config=path)
        assert isinstance(b, HipFlowSource.Builder) and isinstance(b.config, LiteFlowNetConfig)
        assert b.config.weights is W
    finally:
        dropin.uninstall()
    try:
        dropin.install(flow=True, compositor=False)
        assert RefFlowSource.from_args("clip.mp4", cv_config=path) == "reference"
    finally:
        dropin.uninstall()
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


# ---- large frames ---------------------------------------------------------------------------------------------------

def test_854x480_pair_matches_float64():
    """One 854 x 480 pair; the float32 statement's own error sets the bound, as for the fixtures."""
    h, w = 480, 854
    W = weights(2, 1.0)
    one, two = _textured(h, w, 77, (3, -5))
    got = LiteFlowNet(w, h, W).calc(one, two)
    ratio = _check_network(got, lfn_ref.estimate(W, one, two, torch.float64),
                           lfn_ref.estimate(W, one, two, torch.float32), "854x480")
    print(f"854x480: error ratio {ratio:.3f}")


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_large_pairs_finite_and_deterministic(w, h):
    W = weights(1, 0.25)
    rng = np.random.default_rng(w)
    base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
    one = np.ascontiguousarray(np.kron(base, np.ones((8, 8, 1), np.uint8))[:h, :w])
    two = np.ascontiguousarray(np.roll(one, (2, 3), (0, 1)))
    net = LiteFlowNet(w, h, W)
    a = net.calc(one, two)
    b = net.calc(one, two)
    assert np.isfinite(a).all() and _bits_equal(a, b)
