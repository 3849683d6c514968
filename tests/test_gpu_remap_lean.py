"""The lean remap step (k_remap_step_lean, option "remap_lean" = 1, the default) against the general kernel
(k_remap_step_quad, "remap_lean" = 0) in one process: layer state, rgba and every frame the same bytes over three
consecutive steps, through tf_remap_step_dev and through tf_remap_steps_dev.  Every run also reads the launch labels
(tf_prof_report): with the option on a qualifying layer takes "remap_step_lean_*" for every step and nothing else, with it
off -- or a layer that does not qualify -- never.

Shapes (h, w): 1 x 4 one lane, a single row, the rest of the block dead; 3 x 8 six lanes; 5 x 64 and 7 x 260 several rows
per block and a width that is no multiple of the block (7 x 260 = 455 lanes: a whole block and a part of one).
"""
import numpy as np
import pytest

from oracle import remap_ref as R
from tests.test_gpu_remap_quad import BG, pixmaps, same_bytes, start_state

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4), (3, 8), (5, 64), (7, 260)]
IDS = dict(ids=lambda s: f"{s[1]}x{s[0]}")


@pytest.fixture(scope="module")
def remap():
    from transflow_amd import remap
    return remap


def run(remap, lib_option, lean, h, w, cfg, masks, init, ch, flows, pms, seed=0, clip_flow=0, one_call=False, us=None):
    """The steps over `flows` on a fresh layer: (data, rgba, frames, out_of_frame, {launch label: count})."""
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer
    lib_option("remap_lean", lean)
    layer = remap.RemapLayer(h, w, **cfg, **masks)
    layer.set_sources([np.ones((h, w), np.uint8)])
    if init is not None:
        layer.set_state(*init)
    n = len(flows)
    comps = [remap.CompImage(h, w, BG) for _ in range(n)]
    fbuf = [DevBuffer.from_array(np.ascontiguousarray(f)) for f in flows]
    pbuf = [DevBuffer.from_array(np.ascontiguousarray(pm)) for pm in pms]     # exactly h * w * ch bytes each
    ubuf = None if us is None else [DevBuffer.from_array(np.asarray(u, np.float64)) for u in us]
    _lib.profile(True, "remap_step")
    if one_call:
        layer.steps_dev(comps, [x.ptr for x in fbuf], [x.ptr for x in pbuf], ch, clip_flow=clip_flow,
                        uniforms_dev=None if ubuf is None else [x.ptr for x in ubuf], seed=seed)
    else:
        for i in range(n):
            layer.step_dev(comps[i], fbuf[i].ptr, pbuf[i].ptr, ch, clip_flow=clip_flow,
                           uniform_dev=None if ubuf is None else ubuf[i].ptr, seed=seed)
    frames = [c.download() for c in comps]
    data, rgba = layer.get_state()
    oob = layer.out_of_frame()
    launched = {k: v[0] for k, v in _lib.profile_report().items()}
    _lib.profile(False)
    for b in fbuf + pbuf + (ubuf or []):
        b.close()
    for c in comps:
        c.close()
    layer.close()
    return data, rgba, frames, oob, launched


def lean_launches(launched):
    return sum(c for k, c in launched.items() if k.startswith("remap_step_lean"))


def both(remap, lib_option, h, w, cfg, masks, init, ch, flows, pms, what="", qualifies=True, **kw):
    """Lean against general, single steps and one call: the same bytes; the lean kernel ran where it should."""
    got = {(lean, one): run(remap, lib_option, lean, h, w, cfg, masks, init, ch, flows, pms, one_call=one, **kw)
           for lean in (1, 0) for one in (False, True)}
    for one in (False, True):
        same_bytes(got[1, one], got[0, one], f"{what} one call {one}: lean vs general")
        assert lean_launches(got[0, one][4]) == 0
        assert lean_launches(got[1, one][4]) == (len(flows) if qualifies else 0), got[1, one][4]
        assert sum(got[1, one][4].values()) == len(flows), got[1, one][4]
    same_bytes(got[1, True], got[1, False], f"{what}: one call vs single steps")
    return got


def border_flows(rng, h, w, n):
    """Per pixel one of: a small vector; the vector to each border exactly; one to three pixels past each border; far
    outside; NaN in either or both components; +-inf."""
    ii, jj = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for _ in range(n):
        f = rng.normal(0, 2.0, (h, w, 2)).astype(np.float32)
        kind = rng.integers(0, 16, (h, w))
        past = rng.integers(0, 4, (h, w)).astype(np.float32)          # 0: the border itself
        f[..., 0] = np.where(kind == 1, -jj - past, f[..., 0])
        f[..., 0] = np.where(kind == 2, w - 1 - jj + past, f[..., 0])
        f[..., 1] = np.where(kind == 3, -ii - past, f[..., 1])
        f[..., 1] = np.where(kind == 4, h - 1 - ii + past, f[..., 1])
        f[..., 0] = np.where(kind == 5, -jj - past, f[..., 0])        # the corner: both at once
        f[..., 1] = np.where(kind == 5, -ii - past, f[..., 1])
        f[kind == 6] = (1e9, -1e9)
        f[kind == 7] = (np.nan, 1.0)
        f[kind == 8] = (-1.0, np.nan)
        f[kind == 9] = (np.nan, np.nan)
        f[kind == 10] = (np.inf, -np.inf)
        f[kind == 11] = (-np.inf, np.inf)
        f[kind == 12] = (0.5, -0.5)                                   # ties of the rounding
        f[0, 0] = (-1.0, 0.0)                                         # before the first pixel
        f[h - 1, w - 1] = (1.0, 0.0)                                  # past the last one
        out.append(f)
    return out


def winner_maps(rng, h, w, n):
    """clip_flow = 2: source indices anywhere in the frame, -1 (nobody came), the first and the last pixel, and
    indices past the frame (the clip brings them back)."""
    N = h * w
    out = []
    for _ in range(n):
        m = rng.integers(0, N, (h, w)).astype(np.int32)
        m[rng.random((h, w)) < 0.3] = -1
        m.ravel()[rng.integers(0, N, 2)] = [0, N - 1]
        m.ravel()[rng.integers(0, N, 1)] = N + 5
        out.append(m)
    return out


CONFIGS = [
    ("reset off", dict(), False),
    ("random, no mask, transparent can move",
     dict(transparent_pixels_can_move=True, reset_mode="random", reset_random_factor=0.3), False),
    ("random through a mask", dict(reset_mode="random", reset_random_factor=0.5), True),
]


@pytest.mark.parametrize("clip", [0, 1, 2])
@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_lean_gives_the_bytes_of_the_general_kernel(remap, lib_option, shape, ch, clip):
    """Flows at and past every border, NaN and +-inf, with clip_flow 0 (the out-of-frame flag must be raised exactly
    where the general kernel raises it: same_bytes compares it), 1 and 2; a checkpoint with holes and foreign source
    indices (pixels that keep their colour) and the identity state; reset off, random with one threshold, random through
    a mask; transparent_pixels_can_move off and on."""
    h, w = shape
    rng = np.random.default_rng(100 * h + w + 10 * ch + clip)
    flows = winner_maps(rng, h, w, 3) if clip == 2 else border_flows(rng, h, w, 3)
    pms = pixmaps(rng, h, w, ch, 3)
    for name, cfg, with_mask in CONFIGS:
        masks = dict(reset_mask=rng.random((h, w)).astype(np.float32)) if with_mask else {}
        for init in (start_state(rng, h, w), None):
            got = both(remap, lib_option, h, w, cfg, masks, init, ch, flows, pms, seed=20251020, clip_flow=clip,
                       what=f"{w}x{h} {ch} channels clip {clip} {name} init {init is not None}")
            if clip == 0:
                assert got[1, False][3] and got[1, True][3]          # (0, 0) points before the first pixel
            else:
                assert not got[1, False][3]


@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_the_last_pixel_of_an_rgb_pixmap(remap, lib_option, shape):
    """A pixmap of exactly 3 N bytes whose last pixel is gathered by itself (factor 1.0 resets every pixel to the
    identity): its 4-byte load starts a byte early.  Every pixel's colour differs from its neighbours'."""
    h, w = shape
    n = h * w
    idx = np.arange(n, dtype=np.uint32)
    pm = np.stack([(idx * 7 + 1) % 251, (idx * 13 + 2) % 241, (idx * 29 + 3) % 239], axis=-1).astype(np.uint8).reshape(h, w, 3)
    assert np.all(np.any(pm.reshape(n, 3)[1:] != pm.reshape(n, 3)[:-1], axis=1))
    flows = [np.zeros((h, w, 2), np.float32)] * 3
    cfg = dict(reset_mode="random", reset_random_factor=1.0)
    init = start_state(np.random.default_rng(n), h, w, sources=(0, 0))      # holes, every source index 0
    got = both(remap, lib_option, h, w, cfg, {}, init, 3, flows, [pm] * 3, clip_flow=1, what=f"{w}x{h}")
    for frame in got[1, False][2]:
        np.testing.assert_array_equal(frame, pm)
    np.testing.assert_array_equal(got[1, False][1][..., :3], pm)


@pytest.mark.parametrize("factor", [0.5, 1.0])
@pytest.mark.parametrize("shape", [(3, 8), (7, 260)], **IDS)
def test_reset_thresholds_at_the_ends(remap, lib_option, shape, factor):
    """Masks of 0, 1, negative, above 1, NaN and the smallest normal float, side by side in every lane position, and
    each alone over the whole frame."""
    h, w = shape
    rng = np.random.default_rng(w)
    tiny = float(np.finfo(np.float32).tiny)
    values = np.float32([0.0, 1.0, -1.0, 2.5, np.nan, tiny, 0.5])
    mixed = values[(np.arange(h * w) % 7 + np.arange(h * w) // 7) % 7].reshape(h, w)
    cfg = dict(reset_mode="random", reset_random_factor=factor)
    init, flows, pms = start_state(rng, h, w), border_flows(rng, h, w, 3), pixmaps(rng, h, w, 3, 3)
    ident = R.init_data(h, w)
    for mask in [mixed] + [np.full((h, w), v, np.float32) for v in values[:5]]:
        got = both(remap, lib_option, h, w, cfg, dict(reset_mask=mask), init, 3, flows, pms, seed=41, clip_flow=1,
                   what=f"{w}x{h} factor {factor} mask {mask.ravel()[0]}")
        data = got[1, False][0]
        with np.errstate(invalid="ignore"):
            always = np.float32(factor) * mask >= 1          # u < 1 <= thr: reset in every step, so in the last
        np.testing.assert_array_equal(data[always][:, :3], ident[always][:, :3])     # (a reset keeps the source index)


def test_the_option_and_the_layers_that_do_not_qualify(remap, lib_option):
    """remap_lean is a documented option, 1 by default, 0 or 1.  A destination mask, a supplied uniform field,
    reset_source, an alpha mask, pixels that may not move to filled spots, a width that is no multiple of 4 and a state
    that is not one word all take the general kernels, whatever the option says, and give the same bytes."""
    from transflow_amd import _lib
    assert _lib.get_option("remap_lean") == 1
    with pytest.raises(ValueError):
        _lib.set_option("remap_lean", 2)
    h, w = 5, 64
    rng = np.random.default_rng(8)
    init, pms, flows = start_state(rng, h, w), pixmaps(rng, h, w, 3, 3), border_flows(rng, h, w, 3)
    cfg = dict(reset_mode="random", reset_random_factor=0.5)
    rmask = dict(reset_mask=rng.random((h, w)).astype(np.float32))
    mdst = dict(rmask, mask_dst=(rng.random((h, w)) < 0.8).astype(np.uint8))
    both(remap, lib_option, h, w, cfg, mdst, init, 3, flows, pms, seed=5, clip_flow=1, qualifies=False, what="mask_dst")
    us = [rng.random((h, w)) for _ in range(3)]
    both(remap, lib_option, h, w, cfg, rmask, init, 3, flows, pms, seed=5, clip_flow=1, us=us, qualifies=False, what="supplied u")
    both(remap, lib_option, h, w, dict(cfg, reset_source=True), rmask, init, 3, flows, pms, seed=5, clip_flow=1,
         qualifies=False, what="reset_source")
    both(remap, lib_option, h, w, dict(cfg, pixels_can_move_to_filled_spot=False), rmask, init, 3, flows, pms, seed=5,
         clip_flow=1, qualifies=False, what="to_filled off")
    malpha = dict(rmask, mask_alpha=rng.choice([0.0, 1.0], (h, w)).astype(np.float32))
    both(remap, lib_option, h, w, cfg, malpha, init, 3, flows, pms, seed=5, clip_flow=1, qualifies=False, what="mask_alpha")
    h2, w2 = 6, 10
    both(remap, lib_option, h2, w2, cfg, {}, start_state(rng, h2, w2), 3, border_flows(rng, h2, w2, 3), pixmaps(rng, h2, w2, 3, 3),
         seed=5, clip_flow=1, qualifies=False, what="width 10")
    lib_option("remap_no_pack", 2)
    both(remap, lib_option, h, w, cfg, rmask, init, 3, flows, pms, seed=5, clip_flow=1, qualifies=False, what="int16 state")
    lib_option("remap_no_pack", 0)
    both(remap, lib_option, h, w, cfg, rmask, init, 3, flows, pms, seed=5, clip_flow=1, qualifies=True, what="qualifies")
