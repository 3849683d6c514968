"""CPU checks of the Lucas-Kanade restatement (tests/lk_ref.py) and of the opt-in config and dispatch paths."""
import glob
import json
import os

import numpy as np
import pytest

from tests import lk_ref
from tests.helpers import synth_pair
from transflow_amd.config import (FlowConfig, HornSchunckConfig, LucasKanadeConfig, flow_config_from_dict,
                                  flow_config_from_file, flow_config_from_reference)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LK_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "lk_*.npz")))
CV2_PINS = sorted(glob.glob(os.path.join(GOLDEN, "lk_cv2_*.npz")))
LK_FIXTURES = [p for p in LK_FIXTURES if p not in CV2_PINS]
SHIPPED_LK_JSON = {"method": "lukas-kanade", "lk_window_size": 15, "lk_max_level": 2, "lk_step": 4}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fixtures_exist():
    assert len(LK_FIXTURES) >= 12


@pytest.mark.parametrize("path", LK_FIXTURES, ids=[os.path.basename(p)[3:-4] for p in LK_FIXTURES])
def test_restatement_reproduces_fixture(path):
    z = np.load(path)
    flow = lk_ref.lukas_kanade(z["prev"], z["next"], int(z["win_size"]), int(z["max_level"]), int(z["step"]))
    assert flow.dtype == np.float32 and flow.shape == z["flow"].shape
    np.testing.assert_array_equal(bits(flow), bits(z["flow"]))


@pytest.mark.parametrize("win,levels", [(3, 0), (4, 2), (8, 1), (15, 2), (17, 3), (21, 1)])
def test_vectorised_equals_scalar(win, levels):
    a, b = synth_pair(41, 57, seed=win, shift=(2.5, 1.5), noise=4.0)
    rng = np.random.default_rng(win)
    n = 40
    pts = np.stack([rng.uniform(-4, 60, n), rng.uniform(-4, 44, n)], 1).astype(np.float32)
    pts[: n // 2] = np.round(pts[: n // 2])
    v = lk_ref.calc_pyr_lk(a, b, pts, win, levels)
    s = lk_ref.calc_pyr_lk_scalar(a, b, pts, win, levels)
    np.testing.assert_array_equal(bits(v), bits(s))


def test_both_orders_differ_somewhere_but_agree_vectorised_and_scalar(monkeypatch):
    """SUM_ORDER is honoured by both forms (the pin tool may flip it)."""
    a, b = synth_pair(41, 57, seed=5, shift=(2.5, 1.5), noise=4.0)
    pts = lk_ref.grid_points(41, 57, 3)
    monkeypatch.setattr(lk_ref, "SUM_ORDER", "scalar")
    v = lk_ref.calc_pyr_lk(a, b, pts, 15, 2)
    s = lk_ref.calc_pyr_lk_scalar(a, b, pts[:60], 15, 2)
    np.testing.assert_array_equal(bits(v[:60]), bits(s))


def test_known_answer_identical_frames():
    a, _ = synth_pair(50, 70, seed=7)
    for win, levels, step in ((15, 2, 1), (4, 1, 3), (21, 0, 1)):
        assert not np.any(lk_ref.lukas_kanade(a, a.copy(), win, levels, step))


def test_known_answer_flat_frame_loses_every_point():
    f = np.full((30, 40), 200, np.uint8)
    pts = lk_ref.grid_points(30, 40, 1)
    nxt, trace = lk_ref.calc_pyr_lk(f, f, pts, 9, 1, with_trace=True)
    assert np.all(trace[:, :, 3] == lk_ref.TR_LOST_EIG)
    assert not np.any(lk_ref.lukas_kanade(f, f, 9, 1, 1))


def test_known_answer_integer_translation():
    a, _ = synth_pair(64, 96, seed=9, noise=2.0)
    b = np.roll(a, (2, 3), (0, 1))
    flow = lk_ref.lukas_kanade(a, b, 15, 2, 1)
    inner = flow[16:48, 16:80]
    assert np.abs(inner - np.array([3, 2], np.float32)).max() < 0.05


def test_level_count_cuts_the_pyramid_short():
    assert lk_ref.level_count(160, 120, 15, 5) == 2
    assert lk_ref.level_count(11, 9, 15, 2) == 0
    assert lk_ref.level_count(3840, 2160, 15, 2) == 2


def test_pin_files_match_restatement():
    """tools/pin_lk_with_cv2.py writes lk_cv2_<version>.npz where OpenCV runs; without one the restatement is
    unpinned and this test has nothing to check."""
    if not CV2_PINS:
        pytest.skip("no lk_cv2_*.npz: the restatement is not pinned against a real OpenCV")
    for path in CV2_PINS:
        z = np.load(path)
        for k in range(int(z["n_cases"])):
            p = f"c{k}_"
            got = lk_ref.calc_pyr_lk(z[p + "prev"], z[p + "next"], z[p + "pts"], int(z[p + "win"]), int(z[p + "levels"]))
            np.testing.assert_array_equal(bits(got), bits(z[p + "next_pts"]), err_msg=f"{path} case {k}")


# ---- config and dispatch ---------------------------------------------------------------------------------------------

def test_lk_config_defaults_and_extra():
    c = LucasKanadeConfig()
    assert c.lk_kwargs() == dict(win_size=15, max_level=2, step=1)
    c = LucasKanadeConfig(lk_step=16, fb_levels=3, hs_alpha=2)
    assert c.lk_step == 16 and c.extra == {"fb_levels": 3, "hs_alpha": 2}
    with pytest.raises(ValueError):
        LucasKanadeConfig(method="farneback")
    with pytest.raises(ValueError):
        LucasKanadeConfig(hip_batch=4)
    assert LucasKanadeConfig(hip_prefetch=1).hip_prefetch == 1


def test_lk_config_is_opt_in(tmp_path):
    p = tmp_path / "lk.json"
    p.write_text(json.dumps(SHIPPED_LK_JSON))
    with pytest.raises(ValueError, match="lukas-kanade"):
        flow_config_from_file(str(p))
    c = flow_config_from_file(str(p), lucas_kanade=True)
    assert isinstance(c, LucasKanadeConfig) and c.lk_kwargs() == dict(win_size=15, max_level=2, step=4)
    assert LucasKanadeConfig.from_file(str(p)).to_dict() == SHIPPED_LK_JSON
    assert isinstance(flow_config_from_dict({"method": "lukas-kanade"}, lucas_kanade=True), LucasKanadeConfig)
    with pytest.raises(ValueError):
        flow_config_from_dict({"method": "liteflownet"}, lucas_kanade=True)
    assert isinstance(flow_config_from_dict({"method": "horn-schunck"}, lucas_kanade=True), HornSchunckConfig)
    assert isinstance(flow_config_from_dict({}, lucas_kanade=True), FlowConfig)


class _Method:
    def __init__(self, name):
        self.name = name


class _RefCvFlowConfig:
    def __init__(self, method, **kw):
        self.method = _Method(method)
        self.lk_window_size, self.lk_max_level, self.lk_step = 15, 2, 1
        self.__dict__.update(kw)


def test_reference_objects_opt_in():
    with pytest.raises(ValueError):
        flow_config_from_reference(_RefCvFlowConfig("LUKAS_KANADE"))
    c = flow_config_from_reference(_RefCvFlowConfig("LUKAS_KANADE", lk_step=16), lucas_kanade=True)
    assert isinstance(c, LucasKanadeConfig) and c.lk_step == 16
    mine = LucasKanadeConfig(lk_window_size=21)
    assert flow_config_from_reference(mine) is mine          # an instance passes through, opt-in or not


def test_hip_flow_source_takes_lk_config_when_asked():
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    frames = [np.full((4, 6), i, np.uint8) for i in range(4)]
    with pytest.raises(ValueError):
        HipFlowSource.from_args(ArrayFrameProvider(frames, 10.0), cv_config=_RefCvFlowConfig("LUKAS_KANADE"))
    b = HipFlowSource.from_args(ArrayFrameProvider(frames, 10.0), cv_config=_RefCvFlowConfig("LUKAS_KANADE"),
                                lucas_kanade=True)
    assert isinstance(b.config, LucasKanadeConfig)
    b.build()
    src = HipFlowSource(*b.args(), **b.kwargs())
    src.validate()
    assert isinstance(src.config, LucasKanadeConfig) and not isinstance(src.config, HornSchunckConfig)
    assert not src._resident_ok() and not src._uses_initial_flow()
    b2 = HipFlowSource.from_args(ArrayFrameProvider(frames, 10.0), cv_config=LucasKanadeConfig())
    assert isinstance(b2.config, LucasKanadeConfig)


@pytest.mark.parametrize("lucas_kanade", [False, True])
def test_dropin_dispatch_of_lk(tmp_path, lucas_kanade):
    from transflow_amd import dropin
    from transflow_amd.flow import HipFlowSource

    def original(flow_path, **kw):
        return "reference"

    dispatch = dropin._flow_from_args(original, False, lucas_kanade).__func__
    path = str(tmp_path / "lk.json")
    with open(path, "w") as f:
        json.dump(SHIPPED_LK_JSON, f)
    got = dispatch(None, "clip.mp4", cv_config=path)
    got_obj = dispatch(None, "clip.mp4", cv_config=_RefCvFlowConfig("LUKAS_KANADE"))
    if lucas_kanade:
        assert isinstance(got, HipFlowSource.Builder) and isinstance(got.config, LucasKanadeConfig)
        assert got.config.lk_step == 4
        assert isinstance(got_obj, HipFlowSource.Builder) and isinstance(got_obj.config, LucasKanadeConfig)
    else:
        assert got == "reference" and got_obj == "reference"
    assert dispatch(None, "clip.mp4", cv_config=_RefCvFlowConfig("LITEFLOWNET")) == "reference"
    hs = dispatch(None, "clip.mp4", cv_config=_RefCvFlowConfig("HORN_SCHUNCK"))
    assert hs == "reference"                                  # horn_schunck stays off
