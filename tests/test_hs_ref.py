"""CPU checks of Horn-Schunck: the numpy restatement (tests/hs_ref.py) against the fixtures captured from the reference's
function and against the live function where it is importable; HornSchunckConfig, flow_config_from_file and the drop-in
dispatch of flow methods."""
import glob
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from tests import hs_ref
from tests.helpers import GOLDEN, synth_pair
from transflow_amd.config import (FlowConfig, HornSchunckConfig, flow_config_from_file, flow_config_from_reference)

REF = "/root/reference"
GOLDEN_CASES = sorted(glob.glob(os.path.join(GOLDEN, "hs_*.npz")))


def _case_args(z):
    alpha = int(z["alpha"]) if bool(z["alpha_is_int"]) else float(z["alpha"])
    decay = int(z["decay"]) if bool(z["decay_is_int"]) else float(z["decay"])
    delta = float(z["delta"]) if bool(z["has_delta"]) else None
    return dict(alpha=alpha, max_iters=int(z["max_iters"]), decay=decay, delta=delta)


def test_fixture_set_covers_the_cases():
    names = [os.path.basename(p)[3:-4] for p in GOLDEN_CASES]
    assert len(names) >= 50
    for part in ("9x200", "37x53", "120x160", "480x854", "f32", "f64", "static", "delta0", "iters0", "iters50", "alpha3",
                 "alpha0.5", "decay1", "stop21_1.0001", "stop21_0.9999", "stop2_1.0100", "stop2_0.9900"):
        assert any(part in n for n in names), part
    assert all(os.path.getsize(p) < 1 << 20 for p in GOLDEN_CASES)


@pytest.mark.parametrize("path", GOLDEN_CASES, ids=[os.path.basename(p)[3:-4] for p in GOLDEN_CASES])
def test_restatement_equals_reference_fixture(path):
    z = np.load(path)
    flow_in = z["flow_in"] if "flow_in" in z.files else None
    out, n = hs_ref.horn_schunck(z["prev"], z["next"], flow_in, return_iters=True, **_case_args(z))
    if "flow_out" in z.files:
        assert np.array_equal(out.view(np.int32), z["flow_out"].view(np.int32))
    else:
        assert hashlib.sha256(out.tobytes()).hexdigest() == z["flow_sha256"].item().decode()
    assert n == int(z["iters_run"])


def test_stopping_fixtures_straddle_delta():
    """The +-1e-4 pairs stop one iteration apart: the count is pinned by sigma's side of delta, not by luck."""
    for k in (2, 10, 21):
        for chain in ("f32", "f64"):
            lo = np.load(os.path.join(GOLDEN, f"hs_64x96_{chain}_stop{k}_0.9999.npz"))
            hi = np.load(os.path.join(GOLDEN, f"hs_64x96_{chain}_stop{k}_1.0001.npz"))
            assert int(hi["iters_run"]) == k and int(lo["iters_run"]) == k + 1


def _reference_function():
    """The reference's function with a numpy cv2.GaussianBlur (tools/capture_golden_hs.py), or skip."""
    if not os.path.isdir(os.path.join(REF, "transflow")):
        pytest.skip("reference tree not present")
    pytest.importorskip("scipy.ndimage")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.capture_golden_hs import reference_function
    return reference_function()


@pytest.fixture
def reference_hs():
    saved = {m: sys.modules[m] for m in list(sys.modules) if m == "cv2" or m == "transflow" or m.startswith("transflow.")}
    try:
        yield _reference_function()
    finally:
        for m in [m for m in sys.modules if m == "cv2" or m == "transflow" or m.startswith("transflow.")]:
            del sys.modules[m]
        sys.modules.update(saved)
        if REF in sys.path:
            sys.path.remove(REF)


@pytest.mark.parametrize("h,w,chain,decay,delta,iters", [
    (37, 53, "f64", 0, 1, 3), (37, 53, "f32", 0.95, 1, 3), (120, 160, "f32", 0, None, 12), (120, 160, "f64", 0.95, 0.2, 30),
    (61, 47, "f32", 1, 0.05, 25)])
def test_restatement_equals_live_reference(reference_hs, h, w, chain, decay, delta, iters):
    a, b = synth_pair(h, w, seed=h + w, shift=(1.5, 2.0), noise=7.0)
    flow = None if chain == "f64" else np.random.default_rng(h).normal(0, 2, (h, w, 2)).astype(np.float32)
    exp = reference_hs(a, b, flow=None if flow is None else flow.copy(), alpha=1, max_iters=iters, decay=decay, delta=delta)
    got = hs_ref.horn_schunck(a, b, flow, 1, iters, decay, delta)
    assert np.array_equal(got.view(np.int32), exp.view(np.int32))


# the shipped assets/configs/horn-schunck.json, written inline
SHIPPED_HS_JSON = {"method": "horn-schunck", "hs_alpha": 1, "hs_iterations": 3, "hs_decay": 0, "hs_delta": 1}


def test_horn_schunck_config(tmp_path):
    p = tmp_path / "horn-schunck.json"
    p.write_text(json.dumps(SHIPPED_HS_JSON))
    c = flow_config_from_file(str(p))
    assert isinstance(c, HornSchunckConfig)
    assert c.hs_kwargs() == dict(alpha=1, max_iters=3, decay=0, delta=1)
    assert c.to_dict() == SHIPPED_HS_JSON
    d = HornSchunckConfig()                                     # cv.py:282-285 defaults
    assert (d.hs_alpha, d.hs_iterations, d.hs_decay, d.hs_delta) == (1, 3, 0, 1)
    c = HornSchunckConfig(hs_delta=None, hs_decay=0.95, fb_levels=5, show_window=False, hip_prefetch=2)
    assert c.extra == {"fb_levels": 5, "show_window": False} and c.hip_prefetch == 2
    c.to_file(str(p))
    assert json.loads(p.read_text())["hs_delta"] is None        # JSON null round-trips
    c2 = flow_config_from_file(str(p))
    assert c2.to_dict() == c.to_dict() and c2.hs_delta is None
    for key in ("hip_exact_sums", "hip_batch", "hip_device_flows"):
        with pytest.raises(ValueError, match=key):
            HornSchunckConfig(**{key: 1})
    with pytest.raises(ValueError):
        HornSchunckConfig(method="farneback")
    p.write_text(json.dumps({"method": "farneback", "fb_levels": 2}))
    f = flow_config_from_file(str(p))
    assert isinstance(f, FlowConfig) and f.fb_levels == 2
    p.write_text(json.dumps({"fb_levels": 2}))
    assert isinstance(flow_config_from_file(str(p)), FlowConfig)
    # FlowConfig itself is unchanged: it refuses Horn-Schunck and carries hs_* keys
    with pytest.raises(ValueError):
        FlowConfig(method="horn-schunck")
    assert FlowConfig(hs_alpha=2).extra == {"hs_alpha": 2}


@pytest.mark.parametrize("method", ["lukas-kanade", "liteflownet"])
def test_other_methods_are_rejected(tmp_path, method):
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps({"method": method}))
    with pytest.raises(ValueError, match=method):
        flow_config_from_file(str(p))


class _Method:
    """Stands in for CvFlowSource.Method members (an enum: .name)."""

    def __init__(self, name):
        self.name = name


class _RefCvFlowConfig:
    """Stands in for the reference's CvFlowConfig object (cv.py:271-363)."""

    def __init__(self, method, **kw):
        self.method = _Method(method)
        self.fb_levels, self.hs_alpha, self.hs_iterations, self.hs_decay, self.hs_delta = 3, 1, 3, 0, 1
        self.__dict__.update(kw)


def test_reference_config_objects_by_method():
    c = flow_config_from_reference(_RefCvFlowConfig("HORN_SCHUNCK", hs_alpha=2, hs_delta=None))
    assert isinstance(c, HornSchunckConfig) and c.hs_kwargs() == dict(alpha=2, max_iters=3, decay=0, delta=None)
    assert isinstance(flow_config_from_reference(_RefCvFlowConfig("FARNEBACK", fb_levels=4)), FlowConfig)
    assert flow_config_from_reference(_RefCvFlowConfig("FARNEBACK", fb_levels=4)).fb_levels == 4
    for m in ("LUKAS_KANADE", "LITEFLOWNET"):
        with pytest.raises(ValueError):
            flow_config_from_reference(_RefCvFlowConfig(m))
    assert isinstance(flow_config_from_reference(None), FlowConfig)


def test_hip_flow_source_takes_either_config():
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    frames = [np.full((4, 6), i, np.uint8) for i in range(4)]
    b = HipFlowSource.from_args(ArrayFrameProvider(frames, 10.0), cv_config=_RefCvFlowConfig("HORN_SCHUNCK"))
    assert isinstance(b.config, HornSchunckConfig)
    b.build()
    src = HipFlowSource(*b.args(), **b.kwargs())
    src.validate()
    assert not src._resident_ok()              # Horn-Schunck flows come down and are post-processed on the host
    with pytest.raises(ValueError):
        HipFlowSource.from_args(ArrayFrameProvider(frames, 10.0), cv_config=_RefCvFlowConfig("LUKAS_KANADE"))


@pytest.mark.parametrize("horn_schunck", [False, True])
def test_dropin_dispatch_of_flow_methods(tmp_path, horn_schunck):
    """The dispatcher dropin.install() puts on FlowSource.from_args, with the reference's factory patched out."""
    from transflow_amd import dropin
    from transflow_amd.flow import HipFlowSource

    calls = []

    def original(flow_path, **kw):
        calls.append(kw["cv_config"])
        return "reference"

    dispatch = dropin._flow_from_args(original, horn_schunck).__func__
    paths = {}
    for name, d in (("hs", SHIPPED_HS_JSON), ("fb", {"method": "farneback"}), ("lk", {"method": "lukas-kanade"}),
                    ("lfn", {"method": "liteflownet"})):
        paths[name] = str(tmp_path / f"{name}.json")
        with open(paths[name], "w") as f:
            json.dump(d, f)
    fb = dispatch(None, "clip.mp4", cv_config=paths["fb"])
    assert isinstance(fb, HipFlowSource.Builder) and isinstance(fb.config, FlowConfig)
    assert dispatch(None, "clip.mp4", cv_config=paths["lk"]) == "reference"
    assert dispatch(None, "clip.mp4", cv_config=paths["lfn"]) == "reference"
    assert dispatch(None, "clip.mp4", cv_config=_RefCvFlowConfig("LITEFLOWNET")) == "reference"
    hs = dispatch(None, "clip.mp4", cv_config=paths["hs"])
    hs_obj = dispatch(None, "clip.mp4", cv_config=_RefCvFlowConfig("HORN_SCHUNCK"))
    if horn_schunck:
        assert isinstance(hs, HipFlowSource.Builder) and isinstance(hs.config, HornSchunckConfig)
        assert isinstance(hs_obj, HipFlowSource.Builder) and isinstance(hs_obj.config, HornSchunckConfig)
    else:
        assert hs == "reference" and hs_obj == "reference"
    assert dispatch(None, "clip.mp4", cv_config=None).config.method == "farneback"
