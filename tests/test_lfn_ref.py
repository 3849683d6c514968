"""CPU checks of the LiteFlowNet method: the weight generator and loader, the float32 / float64 restatement against the
reference's own output (tests/golden/lfn_*.npz), the exact fmaf, and the opt-in wiring (config, flow source,
drop-in)."""
import glob
import json
import os
import sys
import types

import numpy as np
import pytest

from tests.helpers import GOLDEN
from transflow_amd import liteflownet as LF


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

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "lfn_*.npz")))


def test_param_spec_is_the_published_network():
    assert LF.blob_size() == 5381969
    assert len(LF.param_spec()) == 212
    spec = dict(LF.param_spec())
    assert spec["netFeatures.netOne.0.weight"] == (32, 3, 7, 7)
    assert spec["netMatching.0.netUpcorr.weight"] == (49, 1, 4, 4)
    assert spec["netSubpixel.4.netMain.0.weight"] == (128, 386, 3, 3)
    assert spec["netRegularization.0.netDist.0.weight"] == (49, 32, 7, 1)
    assert spec["netRegularization.0.netDist.1.weight"] == (49, 49, 1, 7)
    assert spec["netRegularization.4.netDist.0.weight"] == (9, 32, 3, 3)
    assert "netMatching.4.netUpflow.weight" not in spec and "netRegularization.3.netFeat.0.weight" not in spec


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[4:-4] for p in FIXTURES])
def test_generator_reproduces_fixture_sha(path):
    z = np.load(path)
    assert lfn_ref.synthetic_weights(int(z["seed"]), float(z["gain"]))[1] == str(z["sha256"])


def test_loader_round_trips_module_names_and_names_bad_keys(tmp_path):
    W, _ = lfn_ref.synthetic_weights(4, 1.0)
    path = str(tmp_path / "liteflownet-default")
    torch.save({k: torch.from_numpy(v) for k, v in lfn_ref.with_module_names(W).items()}, path)
    got = LF.load_weights(path)
    assert list(got) == [k for k, _ in LF.param_spec()]
    assert all(np.array_equal(got[k], W[k]) for k in W)
    blob = LF.pack_weights(got)
    assert blob.dtype == np.float32 and blob.size == LF.blob_size()
    assert np.array_equal(blob[:32 * 3 * 49], W["netFeatures.netOne.0.weight"].reshape(-1))
    bad = dict(W)
    del bad["netSubpixel.2.netMain.4.bias"]
    with pytest.raises(ValueError, match="netSubpixel.2.netMain.4.bias"):
        LF.check_weights(bad)
    bad = dict(W)
    bad["netRegularization.1.netScaleX.weight"] = np.zeros((1, 24, 1, 1), np.float32)
    with pytest.raises(ValueError, match="netRegularization.1.netScaleX.weight"):
        LF.check_weights(bad)
    bad = dict(W)
    bad["netExtra.weight"] = np.zeros(3, np.float32)
    with pytest.raises(ValueError, match="netExtra.weight"):
        LF.check_weights(bad)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[4:-4] for p in FIXTURES])
def test_restatement_matches_reference_fixture(path):
    """The float32 restatement reproduces the reference's own float32 output directly: within 3e-5 max(1, max|f64|)
    (on the host that recorded the fixtures the two are identical; other CPUs may sum the convolutions in another
    order).  The float64 restatement is the fixture's to 1e-12 relative (BLAS kernels may differ by host).  Where the
    reference raises, so does the restatement."""
    z = np.load(path)
    W, _ = lfn_ref.synthetic_weights(int(z["seed"]), float(z["gain"]))
    one, two = z["prev"], z["next"]
    if "raises" in z:
        with pytest.raises(ZeroDivisionError):
            lfn_ref.estimate(W, one, two, torch.float32)
        return
    f64 = lfn_ref.estimate(W, one, two, torch.float64)
    scale = max(1.0, float(np.abs(f64).max()))
    np.testing.assert_allclose(f64, z["flow64"], rtol=1e-12, atol=1e-12 * scale)
    f32 = lfn_ref.estimate(W, one, two, torch.float32)
    assert np.array_equal(np.isnan(f32), np.isnan(z["flow"]))
    assert float(np.abs(f32 - z["flow"]).max()) <= 3e-5 * scale
    ref_err = float(np.abs(z["flow"] - f64).max())
    assert float(np.abs(f32 - f64).max()) <= 4 * ref_err + 1e-5 * scale


def test_fmaf_agrees_with_fraction_transcription():
    rng = np.random.default_rng(7)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 4).astype(np.float32)
    # double ties: a b + c rounds in float64 to a value exactly halfway between two float32 values while the exact sum
    # lies just off it (a b = 1 - 2^-46 here), on either side and with either sign; a plain float64 sum rounded to
    # float32 gets every one of these wrong
    one_up, one_dn = 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -23          # one_up one_dn = 1 - 2^-46
    ties = []
    for p in (0, 10, -20):                                     
        q = 2.0 ** p
        ties += [(one_up * q, one_dn, (2.0 ** 24 + 2) * q), (-one_up * q, one_dn, -(2.0 ** 24 + 2) * q),
                 (one_up * q, -one_dn, (2.0 ** 24 + 2) * q), (-one_up * q, -one_dn, -(2.0 ** 24 + 2) * q)]
    a[:len(ties)], b[:len(ties)], c[:len(ties)] = zip(*ties)
    got = lfn_ref.fmaf(a, b, c)
    exp = np.array([lfn_ref.fmaf_fraction(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (naive[:len(ties)] != exp[:len(ties)]).all()          # the samples really are double ties


def test_correlation_float32_is_the_fma_order():
    """A tiny case written out by hand: two channels past 32 so that lanes 0 and 1 hold two terms each."""
    rng = np.random.default_rng(1)
    one = torch.from_numpy(rng.standard_normal((1, 34, 2, 2)).astype(np.float32))
    two = torch.from_numpy(rng.standard_normal((1, 34, 2, 2)).astype(np.float32))
    got = lfn_ref.correlation(one, two, 1, torch.float32).numpy()
    a, b = one[0, :, 1, 0].numpy(), two[0, :, 0, 1].numpy()      # output (1, 0), displacement (-1, +1): d = 2 * 7 + 4
    total = np.float32(0)
    for t in range(32):
        part = np.float32(0)
        for ch in range(t, 34, 32):
            part = lfn_ref.fmaf_fraction(a[ch], b[ch], part)
        total = np.float32(total + part)
    assert got[0, 18, 1, 0] == np.float32(total / np.float32(34))


def test_stage_wrappers_check_shapes_before_the_c_side():
    """The C side reads and writes host arrays by the sizes it computes from (n, h, w) and the layer: a mis-shaped
    argument is refused in Python (a handle without a library: reaching C would raise AttributeError)."""
    net = LF.LiteFlowNet.__new__(LF.LiteFlowNet)
    net._h, net._lib = None, None
    up, head = LF.layer_index("netMatching.0.netUpflow"), LF.layer_index("netMatching.0.netMain.6")
    z = np.zeros
    calls = [lambda: net.stage_conv(0, z((1, 8, 8, 3)), out=z((1, 7, 8, 32))),
             lambda: net.stage_conv(head, z((1, 8, 8, 32)), residual=z((1, 8, 7, 2))),
             lambda: net.stage_conv(up, z((1, 8, 8, 2))),
             lambda: net.stage_conv(0, z((8, 8, 3))),
             lambda: net.stage_deconv(0, z((1, 4, 4, 2))),
             lambda: net.stage_deconv(up, z((1, 4, 4, 3))),
             lambda: net.stage_correlation(z((1, 4, 4, 64)), z((1, 4, 5, 64)), 1),
             lambda: net.stage_correlation(z((1, 4, 4, 64)), z((1, 4, 4, 32)), 1),
             lambda: net.stage_backwarp(z((1, 4, 4, 3)), z((1, 4, 4, 3)), 1.0),
             lambda: net.stage_regularize_tail(2, z((1, 4, 4, 25)), z((1, 4, 4, 2))),
             lambda: net.stage_regularize_tail(3, z((1, 4, 4, 25)), z((1, 4, 5, 2))),
             lambda: net.stage_regularize_tail(7, z((1, 4, 4, 25)), z((1, 4, 4, 2)))]
    for call in calls:
        with pytest.raises(ValueError):
            call()


# ---- opt-in wiring ---------------------------------------------------------------------------------------------------

def test_config_opt_in(tmp_path):
    from transflow_amd.config import (LiteFlowNetConfig, flow_config_from_dict, flow_config_from_file,
                                      flow_config_from_reference)
    W = {"any": "weights"}
    cfg = flow_config_from_dict({"method": "liteflownet"}, liteflownet=W)
    assert isinstance(cfg, LiteFlowNetConfig) and cfg.weights is W and cfg.to_dict() == {"method": "liteflownet"}
    with pytest.raises(ValueError):
        flow_config_from_dict({"method": "liteflownet"})
    path = str(tmp_path / "liteflownet.json")
    with open(path, "w") as f:
        json.dump({"method": "liteflownet"}, f)
    assert isinstance(flow_config_from_file(path, liteflownet="w.pt"), LiteFlowNetConfig)
    with pytest.raises(ValueError):
        flow_config_from_file(path)

    class Method:
        name = "LITEFLOWNET"

    ref = types.SimpleNamespace(method=Method())
    assert isinstance(flow_config_from_reference(ref, liteflownet="w.pt"), LiteFlowNetConfig)
    with pytest.raises(ValueError):
        flow_config_from_reference(ref)
    with pytest.raises(ValueError):
        LiteFlowNetConfig()


def test_flow_source_from_args_opt_in(tmp_path):
    from transflow_amd.config import LiteFlowNetConfig
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    path = str(tmp_path / "liteflownet.json")
    with open(path, "w") as f:
        json.dump({"method": "liteflownet"}, f)
    frames = [np.zeros((40, 48, 3), np.uint8)] * 3
    b = HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), cv_config=path, liteflownet="w.pt")
    assert isinstance(b.config, LiteFlowNetConfig) and b.config.weights == "w.pt"
    with pytest.raises(ValueError):
        HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), cv_config=path)


def test_grey_provider_is_refused():
    """The network reads colour: a provider of grey frames gets a ValueError at its first frame, before any GPU
    call (the handle is created only after the frame's check)."""
    from transflow_amd.config import LiteFlowNetConfig
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    frames = [np.zeros((40, 48), np.uint8)] * 3
    src = HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), cv_config=LiteFlowNetConfig(weights="w.pt"))
    with src as s:
        with pytest.raises(ValueError, match="colour"):
            s._ingest(0, frames[0])


def test_dropin_dispatcher_with_and_without_weights(tmp_path):
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
    try:
        dropin.install(flow=True, compositor=False, liteflownet="w.pt")
        b = RefFlowSource.from_args("clip.mp4", cv_config=path)
        assert isinstance(b, HipFlowSource.Builder) and isinstance(b.config, LiteFlowNetConfig)
        dropin.uninstall()
        dropin.install(flow=True, compositor=False)
        assert RefFlowSource.from_args("clip.mp4", cv_config=path) == "reference"
    finally:
        dropin.uninstall()
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
