"""The remap step with four ADJACENT pixels per thread (k_remap_step_quad, option "remap_quad" = 1, the default) against
the same step with its four pixels a block apart (k_remap_step_px, "remap_quad" = 0): layer state, rgba and every frame
the same bytes, through tf_remap_step_dev and through tf_remap_steps_dev, and both equal to the numpy oracle
(oracle/remap_ref.py) fed the same flows and the uniform field the GPU itself drew (tf_remap_uniform_dev).

Shapes (h, w): 5 x 8 one partial block; 7 x 12 a partial block over several rows; 3 x 1028 a pixel count that is no
multiple of 4 x 256 -- the last block's dead lanes, and a lane whose four pixels end a row; 6 x 10 a width that is no
multiple of 4: the step falls back to the block-apart kernel and gives the same bytes; 1 x 4 a single lane.

Two notes on what is run:
  * a layer with two sources is refused by the one-call step (tf_remap_step_dev serves exactly one), so reset_source is
    run with two different introduction masks, one layer each, on a state whose source indices are not all 0;
  * 64 x 33 pixels are 2,112 uniform draws per (seed, frame number); the three frame numbers of a seed make 6,336.
"""
import itertools

import numpy as np
import pytest

from oracle import remap_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(5, 8), (7, 12), (3, 1028), (6, 10), (1, 4)]
STATES = {"word": 0, "int16": 2, "int32": 1}          # option remap_no_pack, as tests/test_gpu_remap.py forces the forms
FLAGS = list(itertools.product([False, True], repeat=3))   # transparent_can_move, to_empty, to_filled (leave_empty: not one kernel)
BG = (7, 130, 251)


@pytest.fixture(scope="module")
def remap():
    from transflow_amd import remap
    return remap


def flag_cfg(flags):
    return dict(transparent_pixels_can_move=flags[0], pixels_can_move_to_empty_spot=flags[1],
                pixels_can_move_to_filled_spot=flags[2])


def start_state(rng, h, w, sources=(0, 1)):
    """A checkpoint every state form can hold: rows and columns anywhere in the frame, alpha 0 in a quarter of the
    pixels, a source index other than 0 in some (those keep the colour they had), and the colours they had."""
    data = R.init_data(h, w)
    data[..., 0] = rng.integers(0, h, (h, w))
    data[..., 1] = rng.integers(0, w, (h, w))
    data[..., 2] = rng.random((h, w)) < 0.75
    data[..., 3] = rng.choice(sources, (h, w), p=[0.85] + [0.15 / (len(sources) - 1)] * (len(sources) - 1))
    return data.astype(np.int32), rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


def pixmaps(rng, h, w, ch, n):
    out = [rng.integers(0, 256, (h, w, ch), dtype=np.uint8) for _ in range(n)]
    if ch == 4:
        for pm in out:
            pm[..., 3] = rng.choice([0, 1, 255], (h, w))
    return out


def backward_flows(rng, h, w, n, sigma=2.5):
    return [R.post_process(rng.normal(0, sigma, (h, w, 2)).astype(np.float32), R.BACKWARD) for _ in range(n)]


def run(remap, lib_option, quad, h, w, cfg, masks, intro, init, ch, flows, pms, us=None, seed=0, clip_flow=0,
        one_call=False, flow_offset=0):
    """The steps over `flows` (float32 [h, w, 2], or int32 [h, w] winner maps with clip_flow = 2) on a fresh layer:
    (data, rgba, frames, out_of_frame, the uniform fields the single steps were about to draw)."""
    from transflow_amd.device import DevBuffer
    lib_option("remap_quad", quad)
    layer = remap.RemapLayer(h, w, **cfg, **masks)
    layer.set_sources([intro])
    if init is not None:
        layer.set_state(*init)
    n = len(flows)
    comps = [remap.CompImage(h, w, BG) for _ in range(n)]
    fbuf = []
    for f in flows:                       # flow_offset: the flow starts that many bytes into its buffer
        raw = np.ascontiguousarray(f).view(np.uint8).ravel()
        fbuf.append(DevBuffer.from_array(np.concatenate([np.zeros(flow_offset, np.uint8), raw])))
    pbuf = [DevBuffer.from_array(pm) for pm in pms]
    ubuf = None if us is None else [DevBuffer.from_array(np.asarray(u, np.float64)) for u in us]
    fptr = [b.ptr + flow_offset for b in fbuf]
    drawn = []
    if one_call:
        layer.steps_dev(comps, fptr, [b.ptr for b in pbuf], ch, clip_flow=clip_flow,
                        uniforms_dev=None if ubuf is None else [b.ptr for b in ubuf], seed=seed)
    else:
        field = DevBuffer(h * w * 8)
        for i in range(n):
            if us is None and cfg.get("reset_mode") == "random":
                layer.uniform_dev(seed, field.ptr)
                drawn.append(field.download((h, w), np.float64))
            layer.step_dev(comps[i], fptr[i], pbuf[i].ptr, ch, clip_flow=clip_flow,
                           uniform_dev=None if ubuf is None else ubuf[i].ptr, seed=seed)
        field.close()
    frames = [c.download() for c in comps]
    data, rgba = layer.get_state()
    oob = layer.out_of_frame()
    for b in fbuf + pbuf + (ubuf or []):
        b.close()
    for c in comps:
        c.close()
    layer.close()
    return data, rgba, frames, oob, drawn


def same_bytes(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=f"{what}: layer state")
    np.testing.assert_array_equal(a[1], b[1], err_msg=f"{what}: rgba")
    assert len(a[2]) == len(b[2])
    for i, (x, y) in enumerate(zip(a[2], b[2])):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: frame {i}")
    assert a[3] == b[3], f"{what}: out-of-frame flag"


def oracle_run(h, w, cfg, masks, intro, init, flows, pms, us):
    """The same steps by the numpy oracle: (data, rgba, frames)."""
    ora = R.MoveRefLayer(h, w, R.LayerParams(**cfg), masks.get("mask_src"), masks.get("mask_dst"), masks.get("mask_alpha"),
                         masks.get("reset_mask"), [np.asarray(intro, bool)])
    if init is not None:
        ora.data[...] = init[0]
        ora.rgba[...] = init[1]
    frames = []
    bg = np.broadcast_to(np.uint8(BG), (h, w, 3))
    for i, f in enumerate(flows):
        ora.update(f, [pms[i]], None if us is None else us[i])
        frames.append(R.composite(bg, [ora.render()]))
    return ora.data, ora.rgba, frames, False


def both_paths(remap, lib_option, h, w, cfg, masks, intro, init, ch, flows, pms, us=None, seed=0, clip_flow=0,
               oracle_flows=None, what=""):
    """Every form of the step over these inputs -- adjacent against block-apart, single steps against one call, after the
    first step and after the last -- and the oracle on the single steps (oracle_flows: the flows as post_process hands
    them to the layer; False: the oracle cannot run these inputs)."""
    random = cfg.get("reset_mode") == "random"
    for n in sorted({1, len(flows)}):
        got = {}
        for quad in (1, 0):
            for one_call in (False, True):
                got[quad, one_call] = run(remap, lib_option, quad, h, w, cfg, masks, intro, init, ch, flows[:n], pms[:n],
                                          None if us is None else us[:n], seed, clip_flow, one_call)
        for one_call in (False, True):
            same_bytes(got[1, one_call], got[0, one_call], f"{what} {n} step(s), one call {one_call}: adjacent vs block-apart")
        same_bytes(got[1, True], got[1, False], f"{what} {n} step(s): one call vs single steps")
        if oracle_flows is not False:
            fields = us if us is not None else (got[1, False][4] if random else None)
            exp = oracle_run(h, w, cfg, masks, intro, init, (flows if oracle_flows is None else oracle_flows)[:n], pms[:n],
                             None if fields is None else fields[:n])
            same_bytes(got[1, False], exp, f"{what} {n} step(s): adjacent vs oracle")
    return got


def all_masks(rng, h, w):
    return dict(mask_src=(rng.random((h, w)) < 0.85).astype(np.uint8), mask_dst=(rng.random((h, w)) < 0.85).astype(np.uint8),
                mask_alpha=rng.choice([0.0, 0.5, 1.0], (h, w)).astype(np.float32),
                reset_mask=rng.random((h, w)).astype(np.float32))


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_adjacent_pixels_give_the_bytes_of_the_block_apart_kernel(remap, lib_option, shape, state, ch):
    """Every move-flag combination the one kernel serves, every mask present, random reset through a mask with the field
    drawn on the GPU, a checkpoint with holes and foreign source indices, three steps."""
    lib_option("remap_no_pack", STATES[state])
    h, w = shape
    rng = np.random.default_rng(1000 * h + w + ch)
    masks = all_masks(rng, h, w)
    init = start_state(rng, h, w)
    flows = backward_flows(rng, h, w, 3)
    pms = pixmaps(rng, h, w, ch, 3)
    for flags in FLAGS:
        cfg = dict(flag_cfg(flags), reset_mode="random", reset_random_factor=0.5)
        both_paths(remap, lib_option, h, w, cfg, masks, np.ones((h, w), np.uint8), init, ch, flows, pms, seed=20251003,
                   what=f"{w}x{h} {state} {ch} channels flags {flags}")


def test_the_option_and_the_fallbacks(remap, lib_option):
    """remap_quad is a documented option, 1 by default, 0 or 1; a flow that does not start on a 16-byte boundary and
    remap_px below 4 take the block-apart kernels and give the same bytes."""
    from transflow_amd import _lib
    assert _lib.get_option("remap_quad") == 1
    with pytest.raises(ValueError):
        _lib.set_option("remap_quad", 2)
    h, w = 7, 12
    rng = np.random.default_rng(5)
    masks, init = all_masks(rng, h, w), start_state(rng, h, w)
    flows, pms = backward_flows(rng, h, w, 3), pixmaps(rng, h, w, 3, 3)
    cfg = dict(reset_mode="random", reset_random_factor=0.5)
    ones = np.ones((h, w), np.uint8)
    ref = run(remap, lib_option, 0, h, w, cfg, masks, ones, init, 3, flows, pms, seed=9)
    same_bytes(run(remap, lib_option, 1, h, w, cfg, masks, ones, init, 3, flows, pms, seed=9, flow_offset=8), ref, "flow at +8 bytes")
    for px in (2, 1):
        lib_option("remap_px", px)
        same_bytes(run(remap, lib_option, 1, h, w, cfg, masks, ones, init, 3, flows, pms, seed=9), ref, f"remap_px {px}")


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("shape", [(7, 12), (3, 1028), (6, 10)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_sources_outside_the_frame_set_the_error_flag(remap, lib_option, shape, state):
    """clip_flow = 0 and vectors that round to sources before the first or past the last pixel: the flag is set, those
    pixels stay put (the oracle on the same flow with those vectors zeroed), everything else moves."""
    lib_option("remap_no_pack", STATES[state])
    h, w = shape
    rng = np.random.default_rng(77 + w)
    flows = backward_flows(rng, h, w, 3)
    for f in flows:
        f[0, :5] = (-3.0, -2.0)              # before the first pixel
        f[h - 1, w - 6:] = (4.0, 1.0)        # past the last one
        f[h // 2, 1] = (0.0, -1e4)
    tame = []
    for f in flows:
        s = np.arange(h * w) + R.flow_to_offsets(f).astype(np.int64)
        g = f.copy()
        g.reshape(-1, 2)[(s < 0) | (s >= h * w)] = 0
        tame.append(g)
    init, pms = start_state(rng, h, w), pixmaps(rng, h, w, 3, 3)
    ones = np.ones((h, w), np.uint8)
    got = both_paths(remap, lib_option, h, w, {}, {}, ones, init, 3, flows, pms, oracle_flows=False, what=f"{w}x{h} {state}")
    assert got[1, False][3] and got[0, False][3] and got[1, True][3]
    exp = oracle_run(h, w, {}, {}, ones, init, tame, pms, None)
    same_bytes(got[1, False][:3] + (False,), exp, "offending pixels stay put")
    inside = both_paths(remap, lib_option, h, w, {}, {}, ones, init, 3, tame, pms, what=f"{w}x{h} {state} inside")
    assert not inside[1, False][3]


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("shape", [(7, 12), (3, 1028), (6, 10), (1, 4)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_clip_of_infinite_and_nan_flows(remap, lib_option, shape, state):
    """clip_flow = 1 (source.py:361-362 in registers) on raw flows far outside the frame and +-inf: the oracle's
    post_process then the step.  With NaN (which numpy's rounding to int32 and the kernels' treat differently: the
    oracle is not asked) the two kernels still agree byte for byte."""
    lib_option("remap_no_pack", STATES[state])
    h, w = shape
    rng = np.random.default_rng(31 + w)
    raws = [rng.normal(0, 6, (h, w, 2)).astype(np.float32) for _ in range(3)]
    for f in raws:
        pick = rng.random((h, w))
        f[pick < 0.1] = (np.inf, -np.inf)
        f[(pick >= 0.1) & (pick < 0.2)] = (-np.inf, 1.0)
        f[(pick >= 0.2) & (pick < 0.3)] = (1e9, -1e9)
    init, pms = start_state(rng, h, w), pixmaps(rng, h, w, 3, 3)
    ones = np.ones((h, w), np.uint8)
    cfg = dict(reset_mode="random", reset_random_factor=0.25)
    got = both_paths(remap, lib_option, h, w, cfg, {}, ones, init, 3, raws, pms, seed=3, clip_flow=1,
                     oracle_flows=[R.post_process(f.copy(), R.BACKWARD) for f in raws], what=f"{w}x{h} {state} inf")
    assert not got[1, False][3]
    for f in raws:
        pick = rng.random((h, w))
        f[pick < 0.15] = (np.nan, 1.0)
        f[(pick >= 0.15) & (pick < 0.3)] = (-1.0, np.nan)
        f[(pick >= 0.3) & (pick < 0.4)] = (np.nan, np.nan)
    both_paths(remap, lib_option, h, w, cfg, {}, ones, init, 3, raws, pms, seed=3, clip_flow=1, oracle_flows=False,
               what=f"{w}x{h} {state} nan")


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_winner_map_form(remap, lib_option, shape, state):
    """clip_flow = 2: the flow is the winner map of a FORWARD post_process (the source pixel's index, -1 where nobody
    came), source.py:359-362 formed in registers.  The oracle gets the flow the map stands for."""
    lib_option("remap_no_pack", STATES[state])
    h, w = shape
    n = h * w
    rng = np.random.default_rng(13 + w)
    maps, flows = [], []
    for _ in range(3):
        ii, jj = np.mgrid[0:h, 0:w]
        si = np.clip(ii + rng.integers(-2, 3, (h, w)), 0, h - 1)
        sj = np.clip(jj + rng.integers(-5, 6, (h, w)), 0, w - 1)
        win = (si * w + sj).astype(np.int32)
        win[rng.random((h, w)) < 0.3] = -1
        win.ravel()[rng.integers(0, n, 2)] = [0, n - 1]            # the first and the last pixel as sources
        src = np.where(win >= 0, win, np.arange(n).reshape(h, w))
        maps.append(win)
        flows.append(np.stack([src % w - jj, src // w - ii], axis=-1).astype(np.float32))
    init, pms = start_state(rng, h, w), pixmaps(rng, h, w, 3, 3)
    cfg = dict(reset_mode="random", reset_random_factor=0.25)
    got = both_paths(remap, lib_option, h, w, cfg, all_masks(rng, h, w), np.ones((h, w), np.uint8), init, 3, maps, pms, seed=8,
                     clip_flow=2, oracle_flows=flows, what=f"{w}x{h} {state}")
    assert not got[1, False][3]


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("supplied_u", [False, True])
def test_random_reset_thresholds(remap, lib_option, state, with_mask, supplied_u):
    """The threshold factor * mask in float32 against u in float64: mask values 0, 1, above 1, negative, the smallest
    normal float (the product is subnormal) and NaN, side by side in every lane position; no mask; the field drawn on
    the GPU or handed in (with exact zeros and values next to the thresholds in it)."""
    lib_option("remap_no_pack", STATES[state])
    tiny = float(np.finfo(np.float32).tiny)
    for h, w in [(7, 12), (3, 1028)]:
        rng = np.random.default_rng(w + 2 * with_mask + supplied_u)
        values = np.float32([0.0, 1.0, 2.5, -1.0, tiny, np.nan, 0.5])
        masks = dict(reset_mask=values[(np.arange(h * w) % 7 + np.arange(h * w) // 7) % 7].reshape(h, w)) if with_mask else {}
        us = None
        if supplied_u:
            us = []
            for _ in range(3):
                u = rng.random((h, w))
                u[rng.random((h, w)) < 0.2] = 0.0
                u[rng.random((h, w)) < 0.1] = np.float64(np.float32(0.5) * np.float32(0.5))       # u == threshold: no reset
                u[rng.random((h, w)) < 0.1] = np.nextafter(0.25, 0.0)
                us.append(u)
        init = start_state(rng, h, w)
        for factor in (0.5, 1.0):
            cfg = dict(reset_mode="random", reset_random_factor=factor)
            both_paths(remap, lib_option, h, w, cfg, masks, np.ones((h, w), np.uint8), init, 3, backward_flows(rng, h, w, 3),
                       pixmaps(rng, h, w, 3, 3), us=us, seed=41, what=f"{w}x{h} {state} factor {factor}")


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("which", [0, 1])
def test_reset_source_with_an_introduction_mask(remap, lib_option, state, which):
    """reset_source: a reset pixel takes the index of the source whose introduction mask covers it -- 0, the one source
    the one-call step serves -- and keeps its index elsewhere: on a checkpoint with indices 0, 3 and 31.  Two masks."""
    lib_option("remap_no_pack", STATES[state])
    for h, w in [(7, 12), (3, 1028)]:
        rng = np.random.default_rng(w + which)
        intro = [(np.arange(h * w).reshape(h, w) % 3 != 0), rng.random((h, w)) < 0.5][which].astype(np.uint8)
        init = start_state(rng, h, w, sources=(0, 3, 31))
        cfg = dict(reset_mode="random", reset_random_factor=0.6, reset_source=True)
        got = both_paths(remap, lib_option, h, w, cfg, dict(reset_mask=rng.random((h, w)).astype(np.float32)), intro, init, 3,
                         backward_flows(rng, h, w, 3), pixmaps(rng, h, w, 3, 3), seed=17, what=f"{w}x{h} {state} mask {which}")
        assert set(np.unique(got[1, False][0][..., 3])) <= {0, 3, 31}


def test_a_second_source_is_refused_either_way(remap, lib_option):
    from transflow_amd.device import DevBuffer
    h, w = 7, 12
    flow, pm = DevBuffer.from_array(np.zeros((h, w, 2), np.float32)), DevBuffer.from_array(np.zeros((h, w, 3), np.uint8))
    for quad in (1, 0):
        lib_option("remap_quad", quad)
        layer = remap.RemapLayer(h, w, reset_mode="random", reset_source=True)
        layer.set_sources([np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8)])
        comp = remap.CompImage(h, w, BG)
        with pytest.raises(ValueError):
            layer.step_dev(comp, flow.ptr, pm.ptr, 3)
        comp.close()
        layer.close()


@pytest.mark.parametrize("present", list(itertools.product([False, True], repeat=3)),
                         ids=lambda p: "-".join(n for n, on in zip(("msrc", "mdst", "malpha"), p) if on) or "none")
def test_optional_masks_present_and_absent(remap, lib_option, present):
    for state in sorted(STATES):
        lib_option("remap_no_pack", STATES[state])
        for (h, w), ch in itertools.product([(7, 12), (3, 1028)], (3, 4)):
            rng = np.random.default_rng(w + ch)
            every = all_masks(rng, h, w)
            masks = {k: every[k] for k, on in zip(("mask_src", "mask_dst", "mask_alpha"), present) if on}
            cfg = dict(transparent_pixels_can_move=True, reset_mode="random", reset_random_factor=0.3)
            both_paths(remap, lib_option, h, w, cfg, masks, np.ones((h, w), np.uint8), start_state(rng, h, w), ch,
                       backward_flows(rng, h, w, 3), pixmaps(rng, h, w, ch, 3), seed=2, what=f"{w}x{h} {state} {sorted(masks)}")


# ---- the generator: Philox2x32-10 in numpy from the constants of transflow_amd/csrc/remap_common.h

PHILOX_M = 0xD256D193
PHILOX_W = 0x9E3779B9       # the key's increment per round, and the multiplier that folds the seed's high half in
FRAME_FOLD = 0x85EBCA6B     # the multiplier that folds the frame number's high half in


def philox_uniform(pixels, frame, seed):
    lo32 = np.uint64(0xFFFFFFFF)
    c0 = np.arange(pixels, dtype=np.uint64)
    c1 = np.full(pixels, (frame & 0xFFFFFFFF) ^ (((frame >> 32) * FRAME_FOLD) & 0xFFFFFFFF), np.uint64)
    k = (seed & 0xFFFFFFFF) ^ (((seed >> 32) * PHILOX_W) & 0xFFFFFFFF)
    for _ in range(10):
        prod = np.uint64(PHILOX_M) * c0          # both factors below 2^32: exact in 64 bits
        c0 = (prod >> np.uint64(32)) ^ np.uint64(k) ^ c1
        c1 = prod & lo32
        k = (k + PHILOX_W) & 0xFFFFFFFF
    return ((c0 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (c1 >> np.uint64(6)).astype(np.float64)) * (1.0 / 9007199254740992.0)


def test_generator_is_philox2x32_10_bit_for_bit(remap):
    """tf_remap_uniform_dev on 64 x 33 for 3 seeds x 3 frame numbers (the layer's own count of steps: 0, 1 and 5):
    2,112 values each, 6,336 per seed, every one equal to numpy's bit for bit."""
    from transflow_amd.device import DevBuffer
    w, h = 64, 33
    flow, pm = DevBuffer.from_array(np.zeros((h, w, 2), np.float32)), DevBuffer.from_array(np.zeros((h, w, 3), np.uint8))
    field = DevBuffer(h * w * 8)
    comp = remap.CompImage(h, w, BG)
    for seed in (0, 20251003, 0xFEDCBA9876543210):
        layer = remap.RemapLayer(h, w)
        layer.set_sources([np.ones((h, w), np.uint8)])
        frame, compared = 0, 0
        for want in (0, 1, 5):
            while frame < want:
                layer.step_dev(comp, flow.ptr, pm.ptr, 3)
                frame += 1
            layer.uniform_dev(seed, field.ptr)
            got = field.download((h * w,), np.float64)
            exp = philox_uniform(h * w, frame, seed)
            np.testing.assert_array_equal(got.view(np.uint64), exp.view(np.uint64), err_msg=f"seed {seed:#x} frame {frame}")
            assert 0.0 <= got.min() and got.max() < 1.0
            compared += got.size
        assert compared == 6336
        layer.close()
    for b in (flow, pm, field):
        b.close()
    comp.close()
