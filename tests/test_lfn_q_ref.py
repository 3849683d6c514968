"""CPU checks of LiteFlowNet's precision modes: the rounding and the split the quantised restatement (tests/lfn_q_ref.py)
rests on, that restatement on the fixtures, the `hip_lfn_precision` config key and the handle's name table."""
import glob
import os
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import GOLDEN
from tests.lfn_exact_cases import _rne_bf16, _values
from transflow_amd import liteflownet as LF


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
lfn_ref = _Lazy("tests.lfn_ref")
lfn_q_ref = _Lazy("tests.lfn_q_ref")

FIXTURES = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "lfn_*.npz"))) if "raises" not in np.load(p)]


def test_q_is_round_to_nearest_even_on_the_bits():
    x = _values()
    got = lfn_q_ref.q(torch.from_numpy(x)).numpy()
    exp = _rne_bf16(x)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert np.isinf(got).sum() >= 4 and (got.view(np.uint32) & 0xffff == 0).all()
    g64 = lfn_q_ref.q(torch.from_numpy(x).double()).numpy()
    assert g64.dtype == np.float64 and np.array_equal(g64, exp.astype(np.float64))


def test_hi_plus_lo_reproduces_float32_to_2_pow_minus_16():
    x = _values()
    x = x[np.isfinite(_rne_bf16(x)) & (np.abs(x) > 1e-30)]
    xh, xl = (t.numpy().astype(np.float64) for t in lfn_q_ref.split(torch.from_numpy(x)))
    assert (np.abs(xh + xl - x) <= 2.0 ** -16 * np.abs(x)).all()
    assert np.array_equal(xh.astype(np.float32), _rne_bf16(x))


def test_products_of_bfloat16_pairs_are_exact_in_float32():
    """8 significant bits times 8 is at most 16: the float32 product carries no rounding (the bounds of
    tests/test_gpu_liteflownet_precision.py count roundings of the additions only)."""
    from tests.lfn_ref import _round_f32
    rng = np.random.default_rng(6)
    a = _rne_bf16((rng.standard_normal(400) * 10.0 ** rng.integers(-6, 6, 400)).astype(np.float32))
    b = _rne_bf16((rng.standard_normal(400) * 10.0 ** rng.integers(-6, 6, 400)).astype(np.float32))
    prod = a * b
    assert prod.dtype == np.float32
    for x, y, p in zip(a, b, prod):
        exact = Fraction(float(x)) * Fraction(float(y))
        assert Fraction(float(p)) == exact
        assert _round_f32(exact) == p


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[4:-4] for p in FIXTURES])
def test_bf16x3_is_closer_to_float64_than_bf16(path):
    z = np.load(path)
    W, _ = lfn_ref.synthetic_weights(int(z["seed"]), float(z["gain"]))
    f64 = z["flow64"]
    d = {m: float(np.abs(lfn_q_ref.estimate(W, z["prev"], z["next"], torch.float64, m) - f64).max())
         for m in ("bf16", "bf16x3")}
    print(f"{os.path.basename(path)}: max|bf16 - f64| {d['bf16']:.3g}, max|bf16x3 - f64| {d['bf16x3']:.3g} "
          f"(max|f64| {float(np.abs(f64).max()):.3g})")
    assert d["bf16x3"] < d["bf16"]


def test_estimate_f32_mode_is_lfn_ref():
    z = np.load(FIXTURES[0])
    W, _ = lfn_ref.synthetic_weights(int(z["seed"]), float(z["gain"]))
    assert np.array_equal(lfn_q_ref.estimate(W, z["prev"], z["next"], torch.float32, "f32"),
                          lfn_ref.estimate(W, z["prev"], z["next"], torch.float32))
    with pytest.raises(ValueError):
        lfn_q_ref.estimate(W, z["prev"], z["next"], torch.float32, "fp8")


# ---- the config key ---------------------------------------------------------------------------------------------------

def test_config_key_round_trips_and_defaults_stay_out(tmp_path):
    import json
    from transflow_amd.config import LiteFlowNetConfig, flow_config_from_arg, flow_config_from_dict
    W = {"any": "weights"}
    assert LiteFlowNetConfig(weights=W).hip_lfn_precision == "f32"
    assert LiteFlowNetConfig(weights=W, hip_lfn_precision=None).hip_lfn_precision == "f32"
    assert LiteFlowNetConfig(weights=W, hip_lfn_precision="f32").to_dict() == {"method": "liteflownet"}
    for name in ("bf16", "bf16x3"):
        cfg = LiteFlowNetConfig(weights=W, hip_lfn_precision=name)
        assert cfg.hip_lfn_precision == name
        d = cfg.to_dict()
        assert d == {"method": "liteflownet", "hip_lfn_precision": name}
        back = flow_config_from_dict(d, liteflownet=W)
        assert isinstance(back, LiteFlowNetConfig) and back.hip_lfn_precision == name and back.to_dict() == d
        path = str(tmp_path / f"{name}.json")
        cfg.to_file(path)
        assert json.load(open(path)) == d
        assert flow_config_from_arg(path, liteflownet=W).hip_lfn_precision == name


@pytest.mark.parametrize("bad", ["fp8", "BF16", "", 1, True, 16.0, ["bf16"]])
def test_config_key_bad_values(bad):
    from transflow_amd.config import LiteFlowNetConfig
    with pytest.raises(ValueError, match="hip_lfn_precision"):
        LiteFlowNetConfig(weights="w.pt", hip_lfn_precision=bad)


def test_other_methods_refuse_or_carry_the_key():
    from transflow_amd.config import FlowConfig, HornSchunckConfig, LiteFlowNetConfig, LucasKanadeConfig
    for cls in (HornSchunckConfig, LucasKanadeConfig):
        with pytest.raises(ValueError, match="'hip_lfn_precision' is not available with the"):
            cls(hip_lfn_precision="bf16")
        assert cls.HIP_KEYS == ("hip_prefetch",)
    assert FlowConfig.HIP_KEYS == ("hip_exact_sums", "hip_prefetch", "hip_device_flows", "hip_batch")
    cfg = FlowConfig(hip_lfn_precision="bf16", hip_batch=4)
    assert cfg.extra == {"hip_lfn_precision": "bf16"} and cfg.hip_batch == 4
    assert cfg.to_dict()["hip_lfn_precision"] == "bf16" and cfg.to_dict()["hip_batch"] == 4
    assert LiteFlowNetConfig.HIP_KEYS == ("hip_lfn_precision",)
    with pytest.raises(ValueError, match="'hip_batch' is not available with the liteflownet"):
        LiteFlowNetConfig(weights="w.pt", hip_batch=4)


def test_flow_source_builder_carries_the_key(tmp_path):
    import json
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    path = str(tmp_path / "liteflownet.json")
    with open(path, "w") as f:
        json.dump({"method": "liteflownet", "hip_lfn_precision": "bf16x3"}, f)
    frames = [np.zeros((40, 48, 3), np.uint8)] * 3
    b = HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), cv_config=path, liteflownet="w.pt")
    assert b.config.hip_lfn_precision == "bf16x3"


# ---- the handle's name table ------------------------------------------------------------------------------------------

def test_precision_names():
    assert LF.PRECISIONS == {"f32": 0, "bf16": 1, "bf16x3": 2}
    assert [LF.precision_code(n) for n in ("f32", "bf16", "bf16x3")] == [0, 1, 2]
    for bad in ("fp8", "BF16", None, 1):
        with pytest.raises(ValueError):
            LF.precision_code(bad)
    # a handle without a library: reaching C would raise AttributeError
    net = LF.LiteFlowNet.__new__(LF.LiteFlowNet)
    net._h, net._lib = None, None
    with pytest.raises(ValueError, match="fp8"):
        net.set_precision("fp8")
    with pytest.raises(ValueError, match="fp8"):
        LF.LiteFlowNet(64, 64, None, precision="fp8")
