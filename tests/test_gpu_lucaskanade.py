"""Lucas-Kanade on the GPU against the reference's function (tests/golden/lk_*.npz, captured from it) and against the
numpy restatement of OpenCV's lkpyramid.cpp (tests/lk_ref.py), bit for bit: flows are compared as int32 bit patterns."""
import glob
import json
import os

import numpy as np
import pytest

from tests import lk_ref
from tests.helpers import GOLDEN, synth_pair
from transflow_amd.lucaskanade import LucasKanade, level_sizes

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


GOLDEN_CASES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "lk_*.npz"))
                      if not os.path.basename(p).startswith("lk_cv2_"))


def test_fixtures_present():
    assert len(GOLDEN_CASES) >= 12


@pytest.mark.parametrize("path", GOLDEN_CASES, ids=[os.path.basename(p)[3:-4] for p in GOLDEN_CASES])
def test_matches_reference_fixture(path):
    z = np.load(path)
    h, w = z["prev"].shape
    lk = LucasKanade(w, h)
    got = lk.calc(z["prev"], z["next"], int(z["win_size"]), int(z["max_level"]), int(z["step"]))
    lk.close()
    assert _bits_equal(got, z["flow"]), f"{np.count_nonzero(_bits(got) != _bits(z['flow']))} values differ"


def _random_configs(n=100):
    rng = np.random.default_rng(2024)
    out = []
    for k in range(n):
        win = int(rng.integers(3, 32))
        levels = int(rng.integers(0, 6))
        step = int(rng.choice([1, 1, 2, 3, 4, 5, 7, 8, 11, 16]))
        h, w = int(rng.integers(5, 60)) | 1, int(rng.integers(5, 80)) | 1
        out.append((k, win, levels, step, h, w))
    return out


@pytest.mark.parametrize("k,win,levels,step,h,w", _random_configs())
def test_random_configurations_match_restatement(k, win, levels, step, h, w):
    a, b = synth_pair(h, w, seed=100 + k, shift=(3.0, 2.0), noise=5.0)
    exp = lk_ref.lukas_kanade(a, b, win, levels, step)
    lk = LucasKanade(w, h)
    got = lk.calc(a, b, win, levels, step)
    lk.close()
    assert _bits_equal(got, exp), f"{np.count_nonzero(_bits(got) != _bits(exp))} values differ"


def test_4k_defaults_on_sampled_points():
    h, w = 2160, 3840
    a, b = synth_pair(h, w, seed=77, shift=(4.0, 3.0), noise=4.0)
    lk = LucasKanade(w, h)
    got = lk.calc(a, b, 15, 2, 1)
    lk.close()
    idx = np.random.default_rng(77).choice(h * w, 20000, replace=False)
    exp = lk_ref.lukas_kanade_at(a, b, 15, 2, 1, idx)
    assert _bits_equal(got.reshape(-1, 2)[idx], exp)


@pytest.mark.parametrize("win,levels", [(15, 2), (4, 3), (21, 1)])
def test_stage_pyramid_and_scharr(win, levels):
    h, w = 97, 131
    a, b = synth_pair(h, w, seed=win)
    lk = LucasKanade(w, h)
    lk.set_frame(0, a)
    ref = lk_ref.pyramid(a, win, levels)
    assert len(level_sizes(w, h, win, levels)) == len(ref)
    for level, img in enumerate(ref):
        np.testing.assert_array_equal(lk.stage_pyramid(0, win, levels, level), lk_ref.pad101(img, win))
        dx, dy = lk_ref.scharr(img)
        d = lk.stage_scharr(0, win, levels, level)
        np.testing.assert_array_equal(d[..., 0], lk_ref.zero_pad(dx, win))
        np.testing.assert_array_equal(d[..., 1], lk_ref.zero_pad(dy, win))
    lk.close()


def test_stage_trace():
    h, w = 80, 110
    a, b = synth_pair(h, w, seed=3, shift=(3.0, 2.0))
    lk = LucasKanade(w, h)
    lk.set_frame(0, a)
    lk.set_frame(1, b)
    pts = np.array([[0, 0], [55, 40], [109, 79], [3.5, 70.25], [60, 2], [-3, 20], [200, 40]], np.float32)
    for win, levels in ((15, 2), (8, 3), (5, 0)):
        _, trace = lk_ref.calc_pyr_lk(a, b, pts, win, levels, with_trace=True)
        for i, (x, y) in enumerate(pts):
            got = lk.stage_trace(0, 1, win, levels, x, y)
            assert got.shape == trace[i].shape
            assert _bits_equal(got[:, :2], trace[i][:, :2].astype(np.float32)), (win, levels, i)
            np.testing.assert_array_equal(got[:, 2:], trace[i][:, 2:].astype(np.float32))
    lk.close()


def test_n_pairs_in_one_call_equal_each_alone():
    h, w = 70, 90
    frames = [synth_pair(h, w, seed=9, shift=(0.9 * i, 0.6 * i))[1] for i in range(6)]
    batch = LucasKanade(w, h, frame_slots=6, max_pairs=5)
    for s, f in enumerate(frames):
        batch.set_frame(s, f)
    batch.calc_slots([0, 1, 2, 3, 4], [1, 2, 3, 4, 5], win_size=11, max_level=2, step=2, stats=True)
    got = [batch.get_flow(p) for p in range(5)]
    stats = batch.last_stats(0)
    batch.close()
    assert len(stats) == 3 and all(0 <= m <= 30 for _, m in stats)
    single = LucasKanade(w, h)
    for p in range(5):
        assert _bits_equal(got[p], single.calc(frames[p], frames[p + 1], 11, 2, 2))
    single.close()


def test_bgr_ingest_equals_grey_ingest():
    from transflow_amd.flowops import bgr_to_grey
    h, w = 48, 64
    rng = np.random.default_rng(5)
    bgr = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]
    lk = LucasKanade(w, h)
    lk.set_frame_bgr(0, bgr[0])
    lk.set_frame_bgr(1, bgr[1])
    lk.calc_slots([0], [1], 9, 1, 1)
    got = lk.get_flow(0)
    exp = lk.calc(bgr_to_grey(bgr[0], (w, h)), bgr_to_grey(bgr[1], (w, h)), 9, 1, 1)
    lk.close()
    assert _bits_equal(got, exp)


def _frames(h, w, n, seed=5):
    return [synth_pair(h, w, seed=seed, shift=(0.8 * i, 0.5 * i))[1] for i in range(n)]


@pytest.mark.parametrize("direction,step", [("forward", 1), ("backward", 4), ("backward", 1)])
def test_flow_source_matches_host_loop(tmp_path, direction, step):
    """HipFlowSource with a LucasKanadeConfig, filters and a mask, against the same source whose next() runs the
    restatement on the host (frames ordered by direction, cv.py:467-472); the post-process is the same on both."""
    import PIL.Image
    from transflow_amd.config import LucasKanadeConfig
    from transflow_amd.flow import ArrayFrameProvider, FlowSource, HipFlowSource
    h, w = 60, 84
    frames = _frames(h, w, 5)
    cfg = LucasKanadeConfig(lk_window_size=9, lk_max_level=2, lk_step=step)
    mask = (np.add.outer(np.arange(h), np.arange(w)) * 255 // (h + w)).astype(np.uint8)
    mask_path = str(tmp_path / "mask.png")
    PIL.Image.fromarray(mask).save(mask_path)

    class HostLoop(HipFlowSource):
        def next(self):
            frame = self.provider.read()
            if frame is None:
                raise StopIteration
            prev = self._prev_frame
            left, right = (prev, frame) if self.direction == FlowSource.Direction.FORWARD else (frame, prev)
            self._prev_frame = frame
            return lk_ref.lukas_kanade(left, right, **cfg.lk_kwargs())

    kw = dict(direction=direction, cv_config=cfg, flow_filters="scale=2;clip=6", mask_path=mask_path)
    with HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), **kw) as source:
        got = [f.copy() for f in source]
    with HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), **kw) as oracle:
        oracle.__class__ = HostLoop
        exp = [f.copy() for f in oracle]
    assert len(got) == len(exp) >= 4
    for g, e in zip(got, exp):
        assert _bits_equal(g, e)


def test_dropin_install_serves_shipped_lk_config(tmp_path):
    """dropin.install(lucas_kanade=True) builds a HipFlowSource for the shipped lukas-kanade.json (a reference package
    stand-in provides FlowSource; the dispatcher is the one install() puts on it)."""
    import sys
    import types
    from transflow_amd import dropin
    from transflow_amd.config import LucasKanadeConfig
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
    path = str(tmp_path / "lukas-kanade.json")
    with open(path, "w") as f:
        json.dump({"method": "lukas-kanade", "lk_window_size": 15, "lk_max_level": 2, "lk_step": 4}, f)
    try:
        dropin.install(flow=True, compositor=False, lucas_kanade=True)
        b = RefFlowSource.from_args("clip.mp4", cv_config=path)
        assert isinstance(b, HipFlowSource.Builder) and isinstance(b.config, LucasKanadeConfig)
        assert b.config.lk_kwargs() == dict(win_size=15, max_level=2, step=4)
    finally:
        dropin.uninstall()
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert RefFlowSource.from_args("clip.mp4", cv_config=path) == "reference"
