"""LiteFlowNet's bf16 and bf16x3 precision modes on the GPU (tf_lfn_set_precision, csrc/lfn_conv_bf16.hip) against the
quantised restatement tests/lfn_q_ref.py.

With q(v) = v rounded to bfloat16 (ties to even), every convolution of the network computes sum q(x) q(w) + b (bf16) or,
with xh = q(x), xl = q(x - xh) and the same for w, sum (xh wh + xh wl + xl wh) + b (bf16x3), summed in float32.

Stages: each convolution layer against the float64 convolution of the quantised operands of the GPU's own float32 input,
within the bound of a float32 summation of exact products.  Whole network: max|gpu - q64| <= 4 max|q32 - q64| +
1e-5 max(1, max|f64|) with q64, q32 the quantised restatement in float64 and float32, NaN positions equal."""
import glob
import json
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
        if attr.startswith("_"):
            raise AttributeError(attr)
        import importlib
        return getattr(importlib.import_module(self._name), attr)


torch = _Lazy("torch")
F = _Lazy("torch.nn.functional")
lfn_ref = _Lazy("tests.lfn_ref")
lfn_q_ref = _Lazy("tests.lfn_q_ref")

pytestmark = pytest.mark.gpu

MODES = ("bf16", "bf16x3")
FIXTURES = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "lfn_*.npz"))) if "raises" not in np.load(p)]
U = 2.0 ** -24
_W, _F64 = {}, {}


def weights(seed, gain):
    if (seed, gain) not in _W:
        _W[(seed, gain)] = lfn_ref.synthetic_weights(seed, gain)[0]
    return _W[(seed, gain)]


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_network(got, q64, q32, f64, what):
    """The project's network bound on the quantised yardstick; prints the ratio and what the mode costs against the
    unquantised float64 flow."""
    assert got.dtype == np.float32 and got.shape == q64.shape
    assert np.array_equal(np.isnan(got), np.isnan(q64)), what
    ok = ~np.isnan(q64)
    ref_err = float(np.abs(q32[ok] - q64[ok]).max())
    err = float(np.abs(got[ok] - q64[ok]).max())
    bound = 4 * ref_err + 1e-5 * max(1.0, float(np.abs(f64[ok]).max()))
    print(f"{what}: max|gpu - q64| / max|q32 - q64| = {err:.3g} / {ref_err:.3g} = {err / ref_err if ref_err else 0.0:.3f}; "
          f"max|gpu - f64| {float(np.abs(got[ok] - f64[ok]).max()):.3g} (max|f64| {float(np.abs(f64[ok]).max()):.3g})")
    assert err <= bound, f"{what}: max|gpu - q64| {err:.3g} > {bound:.3g} (float32 restatement {ref_err:.3g})"


def _yardsticks(W, one, two, mode, key):
    """(q64, q32, f64) of a pair; the unquantised float64 flow is computed once per pair and shared by the modes."""
    if key not in _F64:
        _F64[key] = lfn_ref.estimate(W, one, two, torch.float64)
    return (lfn_q_ref.estimate(W, one, two, torch.float64, mode), lfn_q_ref.estimate(W, one, two, torch.float32, mode),
            _F64[key])


# ---- every convolution layer ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def net():
    return LiteFlowNet(64, 64, weights(1, 1.0))


CONV_LAYERS = [i for i, l in enumerate(LF.layers()) if not l.deconv]
# each layer with the misaligned slices of tests/test_gpu_liteflownet.py, and, where Cin is a multiple of 4, with every
# offset and channel stride a multiple of 4 as well: the kernel gathers the second kind with 128-bit loads
STAGE_CASES = [(i, False) for i in CONV_LAYERS] + [(i, True) for i in CONV_LAYERS if LF.layers()[i].cin % 4 == 0]


def _conv64(parts, layer, bias):
    """sum over the (x, w) pairs of the float64 convolution, plus the bias; and the same of the absolute values."""
    kw = dict(stride=layer.stride, padding=(layer.ph, layer.pw))
    y = sum(F.conv2d(x, w, None, **kw) for x, w in parts) + bias.view(1, -1, 1, 1)
    mag = sum(F.conv2d(x.abs(), w.abs(), None, **kw) for x, w in parts) + bias.abs().view(1, -1, 1, 1)
    return y.permute(0, 2, 3, 1).numpy(), mag.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("li,aligned", STAGE_CASES,
                         ids=[LF.layers()[i].name + ("-aligned" if a else "") for i, a in STAGE_CASES])
def test_stage_conv_every_layer(net, li, aligned, mode):
    """Products of bfloat16 pairs are exact in float32 (tests/test_lfn_q_ref.py), so only additions round: a float32
    sum of T exact terms and a bias, in any order, is within (T + 2) 2^-24 (sum|terms| + |b|) of the exact value, with
    T = K (bf16) or 3 K (bf16x3); LeakyReLU does not increase the error; a residual adds one rounding of the result.
    The yardstick is the float64 convolution of the quantised operands of the GPU's own float32 input.  An unquantised
    float32 convolution would miss it by thousands of times the bound."""
    layer = LF.layers()[li]
    W = weights(1, 1.0)
    rng = np.random.default_rng(li)
    h, w = (11, 13) if layer.stride == 1 else (12, 15)
    ho, wo = layer.out_size(h, w)
    if aligned:
        off_in, cs_in, off_out, cs_out, off_res, cs_res = 4, layer.cin + 8, 4, (layer.cout + 8 + 3) // 4 * 4, 4, 8
    else:
        off_in, cs_in, off_out, cs_out, off_res, cs_res = 2, layer.cin + 3, 1, layer.cout + 4, 1, layer.cout + 1
    x = rng.standard_normal((2, h, w, cs_in)).astype(np.float32)
    out0 = rng.standard_normal((2, ho, wo, cs_out)).astype(np.float32)
    res = rng.standard_normal((2, ho, wo, cs_res)).astype(np.float32) if layer.cout == 2 else None
    from transflow_amd import _lib
    net.set_precision(mode)
    assert net.precision == mode
    _lib.profile(True, "lfn_conv")
    try:
        got = net.stage_conv(li, x, out=out0, in_off=off_in, out_off=off_out, residual=res, res_off=off_res)
        _lib.check(_lib.load().tf_sync())
        labels = _lib.profile_report()
    finally:
        _lib.profile(False)
    # the launch's label says which gather ran: `<class>_v` with 128-bit loads, `<class>` one channel at a time
    assert len(labels) == 1 and next(iter(labels)).endswith("_v") == aligned, labels
    assert np.array_equal(got[..., :off_out], out0[..., :off_out])
    assert np.array_equal(got[..., off_out + layer.cout:], out0[..., off_out + layer.cout:])
    xt = torch.from_numpy(np.ascontiguousarray(x[..., off_in:off_in + layer.cin])).permute(0, 3, 1, 2)
    wt = torch.from_numpy(W[layer.name + ".weight"])
    bias = torch.from_numpy(W[layer.name + ".bias"]).double()
    xh, xl = lfn_q_ref.split(xt, torch.float64)
    wh, wl = lfn_q_ref.split(wt, torch.float64)
    K = layer.kh * layer.kw * layer.cin
    if mode == "bf16":
        y, mag = _conv64([(xh, wh)], layer, bias)
        terms = K
    else:
        y, mag = _conv64([(xh, wh), (xh, wl), (xl, wh)], layer, bias)
        terms = 3 * K
    if layer.leaky:
        y = np.where(y > 0, y, y * 0.1)
    bound = (terms + 2) * U * mag
    if res is not None:
        y = res[..., off_res:off_res + layer.cout].astype(np.float64) + y
        bound = bound + U * np.abs(y)
    err = np.abs(got[..., off_out:off_out + layer.cout].astype(np.float64) - y)
    print(f"{layer.name} {mode}{' aligned' if aligned else ''}: max err / bound {float((err / bound).max()):.3g}")
    assert (err <= bound).all(), float((err / bound).max())


# ---- whole network ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[4:-4] for p in FIXTURES])
def test_fixtures_match_quantised_restatement(path, mode):
    z = np.load(path)
    one, two = z["prev"], z["next"]
    h, w = one.shape[:2]
    W = lfn_ref.synthetic_weights(int(z["seed"]), float(z["gain"]))[0]
    got = LiteFlowNet(w, h, W, precision=mode).calc(one, two)
    q64 = lfn_q_ref.estimate(W, one, two, torch.float64, mode)
    q32 = lfn_q_ref.estimate(W, one, two, torch.float32, mode)
    _check_network(got, q64, q32, z["flow64"], f"{os.path.basename(path)} {mode}")


def _random_cases():
    rng = np.random.default_rng(2024)
    cases = []
    for seed in (1, 2, 3):
        for gain in (0.25, 1.0):
            for _ in range(2):
                h, w = (int(v) for v in rng.integers(33, 131, 2))
                cases.append((seed, gain, h, w, int(rng.integers(0, 1 << 30)), (int(rng.integers(-4, 5)), int(rng.integers(-4, 5)))))
    return cases


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed,gain,h,w,fseed,shift", _random_cases())
def test_random_cases_match_quantised_restatement(seed, gain, h, w, fseed, shift, mode):
    W = weights(seed, gain)
    one, two = lfn_ref.textured_pair(h, w, fseed, shift)
    got = LiteFlowNet(w, h, W, precision=mode).calc(one, two)
    q64, q32, f64 = _yardsticks(W, one, two, mode, (seed, gain, h, w, fseed))
    _check_network(got, q64, q32, f64, f"random {h}x{w} seed {seed} gain {gain} {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_854x480_pair(mode):
    """One 854 x 480 pair per mode: finite, the same twice, and within the network bound."""
    h, w = 480, 854
    W = weights(2, 1.0)
    one, two = lfn_ref.textured_pair(h, w, 77, (3, -5))
    net = LiteFlowNet(w, h, W, precision=mode)
    got = net.calc(one, two)
    assert np.isfinite(got).all() and _bits_equal(got, net.calc(one, two))
    q64, q32, f64 = _yardsticks(W, one, two, mode, "854x480")
    _check_network(got, q64, q32, f64, f"854x480 {mode}")


# ---- determinism, switching, errors -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_run_to_run_and_batch_of_4_bit_identical(mode):
    h, w = 64, 96
    W = weights(2, 1.0)
    frames = [lfn_ref.textured_pair(h, w, 20 + i, (i, -i))[0] for i in range(5)]
    net = LiteFlowNet(w, h, W, frame_slots=5, max_pairs=4, precision=mode)
    for s, f in enumerate(frames):
        net.set_frame_bgr(s, f)
    net.calc_slots([0, 1, 2, 3], [1, 2, 3, 4])
    batch = [net.get_flow(i) for i in range(4)]
    net.calc_slots([0, 1, 2, 3], [1, 2, 3, 4])
    assert all(_bits_equal(a, net.get_flow(i)) for i, a in enumerate(batch))
    for i in range(4):
        net.calc_slots([i], [i + 1])
        assert _bits_equal(net.get_flow(0), batch[i]), i
    alone = LiteFlowNet(w, h, W, precision=mode)
    assert _bits_equal(alone.calc(frames[2], frames[3]), batch[2])


def test_switching_modes_on_one_handle():
    h, w = 48, 72
    W = weights(1, 1.0)
    one, two = lfn_ref.textured_pair(h, w, 5, (2, -1))
    net = LiteFlowNet(w, h, W)
    assert net.precision == "f32"
    flows = []
    for mode in ("f32", "bf16", "bf16x3", "f32"):
        net.set_precision(mode)
        assert net.precision == mode
        flows.append(net.calc(one, two))
    assert _bits_equal(flows[0], flows[3])
    assert _bits_equal(flows[0], LiteFlowNet(w, h, W).calc(one, two))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(flows[a], flows[b])
    assert np.abs(flows[2] - flows[0]).max() < np.abs(flows[1] - flows[0]).max()
    # new weights in a bf16 mode: the bf16 planes are made again (a stale repack would give the old weights' flow)
    net.set_precision("bf16")
    W3 = weights(3, 1.0)
    net.set_weights(W3)
    got = net.calc(one, two)
    assert _bits_equal(got, LiteFlowNet(w, h, W3, precision="bf16").calc(one, two))
    assert not np.array_equal(got, flows[1])


def test_bad_precision_is_an_argument_error_and_keeps_the_mode():
    from transflow_amd import _lib
    import ctypes as C
    net = LiteFlowNet(40, 40, weights(1, 1.0), precision="bf16x3")
    for bad in (7, -1, 3):
        assert net._lib.tf_lfn_set_precision(net._h, bad) == _lib.TF_ERR_ARG
        code = C.c_int(-5)
        assert net._lib.tf_lfn_get_precision(net._h, C.byref(code)) == 0 and code.value == 2
    assert net.precision == "bf16x3"
    with pytest.raises(ValueError):
        net.set_precision("fp8")
    assert net.precision == "bf16x3"


# ---- flow source --------------------------------------------------------------------------------------------------------

def _source_flows(frames, handle=None, **kw):
    """The flows of a HipFlowSource over the frames; with `handle`, of the same source with its next() replaced by a
    loop over that handle (as tests/test_gpu_liteflownet.py does): the post-process is then the same on both."""
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource

    class HandleLoop(HipFlowSource):
        def next(self):
            frame = self.provider.read()
            if frame is None:
                raise StopIteration
            prev, self._prev_frame = self._prev_frame, frame
            return handle.calc(frame, prev)            # direction "backward" (cv.py:467-472)

    with HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), direction="backward", **kw) as source:
        if handle is not None:
            source.__class__ = HandleLoop
        return [f.copy() for f in source]


def test_flow_source_follows_the_config_key(tmp_path):
    from transflow_amd.config import LiteFlowNetConfig
    h, w = 48, 72
    W = weights(3, 0.25)
    frames = [lfn_ref.textured_pair(h, w, 30, (i, 2 * i))[0] for i in range(4)]
    kw = dict(flow_filters="scale=2")
    cfg = LiteFlowNetConfig(weights=W, hip_lfn_precision="bf16")
    got = _source_flows(frames, cv_config=cfg, **kw)
    exp = _source_flows(frames, handle=LiteFlowNet(w, h, W, precision="bf16"), cv_config=cfg, **kw)
    plain = _source_flows(frames, cv_config=LiteFlowNetConfig(weights=W), **kw)
    assert len(got) == len(exp) == len(plain) >= 3
    for g, e, p in zip(got, exp, plain):
        assert _bits_equal(g, e) and not np.array_equal(g, p)
    path = str(tmp_path / "liteflownet.json")
    with open(path, "w") as f:
        json.dump({"method": "liteflownet", "hip_lfn_precision": "bf16"}, f)
    from_file = _source_flows(frames, cv_config=path, liteflownet=W, **kw)
    assert len(from_file) == len(exp) and all(_bits_equal(g, e) for g, e in zip(from_file, exp))
