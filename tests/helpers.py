"""Shared helpers for the parity tests (oracle side + golden fixtures)."""
import glob
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import remap_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def layer_case_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "remap_layer_*.npz")))


def _parse(v):
    if v in ("True", "False"):
        return v == "True"
    try:
        return float(v)
    except ValueError:
        return v


def case_cfg(z):
    """cfg kwargs stored by tools/capture_golden.py as two string arrays."""
    return {str(k): _parse(str(v)) for k, v in zip(z["cfg_keys"], z["cfg_vals"])}


PRM_KEYS = ("transparent_pixels_can_move", "pixels_can_move_to_empty_spot",
            "pixels_can_move_to_filled_spot", "moving_pixels_leave_empty_spot",
            "reset_mode", "reset_random_factor", "reset_constant_step",
            "reset_linear_factor", "reset_source")


def oracle_params(cfg):
    return remap_ref.LayerParams(**{k: v for k, v in cfg.items() if k in PRM_KEYS})


def synth_pair(h, w, seed=1234, shift=(3.0, 2.0), noise=6.0):
    """SURVEY.md §8(d) synthetic frame pair: multi-scale sine texture + noise;
    frame B is A's texture evaluated at smoothly displaced coordinates."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.4, 1.0, 6)
    fx = rng.uniform(0.004, 0.06, 6)
    fy = rng.uniform(0.004, 0.06, 6)
    ph = rng.uniform(0, 2 * np.pi, 6)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)

    def tex(x, y):
        v = np.zeros_like(x)
        for m in range(6):
            v += a[m] * np.sin(2 * np.pi * (fx[m] * x + fy[m] * y) + ph[m])
        return 128 + 40 * v / 2.0

    u = shift[0] * np.sin(2 * np.pi * yy / h * 2)
    v = shift[1] * np.cos(2 * np.pi * xx / w * 3)
    n0 = np.random.default_rng(seed + 1).normal(0, 1, (h, w)) * noise
    n1 = np.random.default_rng(seed + 2).normal(0, 1, (h, w)) * noise
    fa = np.clip(np.rint(tex(xx, yy) + n0), 0, 255).astype(np.uint8)
    fb = np.clip(np.rint(tex(xx - u, yy - v) + n1), 0, 255).astype(np.uint8)
    return fa, fb


def layer2_case_files():
    """sum / static / introduction layer recurrences (tools/capture_golden.py --layers2-only)."""
    return sorted(glob.glob(os.path.join(GOLDEN, "layer2_*.npz")))


INTRO_KEYS = ("introduce_pixels_on_empty_spots", "introduce_pixels_on_filled_spots", "introduce_moving_pixels",
              "introduce_unmoving_pixels", "introduce_once", "introduce_on_all_filled_spots",
              "introduce_on_all_empty_spots")


def oracle_layer2(z):
    """The oracle's layer object for one layer2_* fixture."""
    cfg = case_cfg(z)
    h, w, ns = int(z["h"]), int(z["w"]), int(z["nsources"])
    intro = [z[f"intro_{s}"] for s in range(ns)]
    cls = str(z["classname"])
    if cls == "sum":
        return remap_ref.SumLayer(h, w, oracle_params(cfg), mask_alpha=z["mask_alpha"], reset_mask=z["reset_mask"],
                                  introduction_masks=intro)
    if cls == "static":
        return remap_ref.StaticLayer(h, w, mask_alpha=z["mask_alpha"], introduction_masks=intro)
    if cls == "introduction":
        prm = remap_ref.IntroParams(**{k: v for k, v in cfg.items() if k in PRM_KEYS + INTRO_KEYS})
        return remap_ref.IntroductionLayer(h, w, prm, mask_src=z["mask_src"], mask_dst=z["mask_dst"],
                                           mask_alpha=z["mask_alpha"], introduction_masks=intro)
    raise ValueError(cls)


def capture_frame_numbers(prm, t, ns):
    """Frame numbers the capture's sources reported at frame t (FakeSource.frame_number = number of
    next() calls - 1): one call per frame in which the layer introduced, i.e. every frame, or only
    the first with introduce_once."""
    return [0 if prm.introduce_once else t] * ns


# Farneback shapes / parameter sets shared by the GPU parity tests and the oracle's envelope test
FB_CASES = [
    ((270, 480), dict()),                                   # transflow defaults (cv.py:273-281)
    ((480, 854), dict()),                                   # configs[0] geometry (River.mp4 854x480)
    ((135, 241), dict(levels=2)),                           # odd sizes: non-integer resize ratios
    ((200, 260), dict(levels=0)),                           # one scale
    ((96, 128), dict(levels=5, winsize=9, iterations=2, poly_n=7, poly_sigma=1.5)),
    ((40, 50), dict(levels=3)),                             # below min_size: K = 0
    ((64, 300), dict(levels=1, pyr_scale=0.8)),
]


FB_SWEEP = [
    ((360, 642), dict(levels=4, pyr_scale=0.7)),                 # non-dyadic pyramid: every level resized with fractions
    ((358, 639), dict(levels=3, pyr_scale=0.5, winsize=21)),     # odd sizes, window half-width 10
    ((240, 320), dict(levels=2, winsize=25, iterations=5)),      # half-width 12, more iterations
    ((300, 400), dict(levels=3, winsize=5, iterations=1)),       # half-width 2, a single iteration
    ((270, 482), dict(levels=5, poly_n=7, poly_sigma=1.5)),      # width % 4 != 0: no split level images
    ((540, 960), dict(levels=5, poly_n=5, poly_sigma=1.1)),      # quarter-4K: the bench's level structure
    ((128, 4096), dict(levels=2)),                               # wide and flat
    ((2048, 64), dict(levels=1)),                                # tall and narrow
    ((90, 130), dict(levels=1, pyr_scale=0.3)),                  # a big step between two scales
]


# ---- fixtures made by tools/pin_with_cv2.py on a machine with a real OpenCV (none is committed until one was) ----------

def cv2_fixture_files(directory=None):
    return sorted(glob.glob(os.path.join(directory or GOLDEN, "farneback_cv2_*.npz")))


def cv2_fixture_cases(path):
    """(meta, [(case dict, prev, next, initial flow or None, cv2's flow)], skipped) of one fixture.  The inputs are
    regenerated from the stored seeds; a case whose regenerated frames do not have the stored CRCs is listed in
    `skipped` (another numpy drawing other numbers), never compared."""
    import json
    import zlib
    z = np.load(path)
    meta = json.loads(str(z["meta_json"]))
    out, skipped = [], []
    for c in meta["cases"]:
        a, b = synth_pair(c["h"], c["w"], seed=c["seed"])
        if (zlib.crc32(a.tobytes()) & 0xFFFFFFFF, zlib.crc32(b.tobytes()) & 0xFFFFFFFF) != (c["crc_prev"], c["crc_next"]):
            skipped.append(c["key"])
            continue
        init = z[c["initial_flow"]] if c.get("initial_flow") else None
        out.append((c, a, b, init, z[c["key"]]))
    return meta, out, skipped


def cv2_fixture_grey(path):
    """(bgr frame, [(width, height, cv2's grey frame)]) of one fixture, or None when the frame does not regenerate."""
    import json
    import zlib
    z = np.load(path)
    g = json.loads(str(z["meta_json"]))["grey"]
    bgr = np.random.default_rng(g["seed"]).integers(0, 256, tuple(g["shape"]) + (3,), dtype=np.uint8)
    if zlib.crc32(bgr.tobytes()) & 0xFFFFFFFF != g["crc_bgr"]:
        return None
    return bgr, [(o["width"], o["height"], z[o["key"]]) for o in g["outputs"]]


# ---- inputs of the differential tests against the reference (tests/test_oracle_vs_reference_live.py,
# tests/test_host_mirror.py).  Every case is drawn here from a fixed seed; tools/capture_live_reference.py ran the
# reference on the very same cases and stored what it returned under tests/golden/live_*.  The draws keep the order
# in which the tests made them when they ran the reference live.

LIVE_LAYER_SEEDS = {"moveref": 11, "sum": 12, "introduction": 13}


def _live_layer_case(rng, cls):
    h, w = int(rng.integers(1, 26)), int(rng.integers(1, 34))
    cfg = dict(transparent_pixels_can_move=bool(rng.integers(2)), pixels_can_move_to_empty_spot=bool(rng.integers(2)),
               pixels_can_move_to_filled_spot=bool(rng.integers(2)), moving_pixels_leave_empty_spot=bool(rng.integers(2)))
    if cls == "introduction":
        cfg.update({k: bool(rng.integers(2)) for k in INTRO_KEYS})
    else:
        cfg.update(reset_mode=str(rng.choice(["off", "random", "constant", "linear"])),
                   reset_random_factor=float(rng.choice([0.0, 0.3, 1.0])),
                   reset_constant_step=float(rng.choice([0.5, 1.0, 2.5])),
                   reset_linear_factor=float(rng.choice([0.1, 0.5])), reset_source=bool(rng.integers(2)))
    masks = dict(mask_alpha=rng.choice([0.0, 0.5, 1.0], (h, w)).astype(np.float32))
    if cls != "sum":
        masks.update(mask_src=rng.random((h, w)) < 0.85, mask_dst=rng.random((h, w)) < 0.85)
    if cls != "introduction":
        masks.update(reset_mask=rng.random((h, w)).astype(np.float32))
    ns = int(rng.integers(1, 3))
    intro = [rng.random((h, w)) < 0.6 for _ in range(ns)]
    chans = [int(rng.choice([3, 4])) for _ in range(ns)]
    return h, w, cfg, masks, intro, chans


def live_layer_cases(cls, trials=60, nframes=4):
    """Random layer configurations of class `cls` -- every move flag, reset mode and introduce_* flag, masks, one or two
    sources of 3 or 4 channels, shapes down to one pixel -- with their pixmaps, background colour, raw flows and
    uniform fields, one dict per trial."""
    rng = np.random.default_rng(LIVE_LAYER_SEEDS[cls])
    for trial in range(trials):
        h, w, cfg, masks, intro, chans = _live_layer_case(rng, cls)
        pixmaps = [[rng.integers(0, 256, (h, w, c), dtype=np.uint8) for _ in range(nframes)] for c in chans]
        bg = "#%02x%02x%02x" % tuple(int(v) for v in rng.integers(0, 256, 3))
        raws, us = [], []
        for _ in range(nframes):
            raws.append(rng.normal(0, 2.5, (h, w, 2)).astype(np.float32))
            us.append(rng.random((h, w)))
        yield dict(trial=trial, h=h, w=w, cfg=cfg, masks=masks, intro=intro, pixmaps=pixmaps, bg=bg, raws=raws, us=us)


def live_flow_ops_cases(trials=40):
    """Random inputs of flow merging, upscale, post_process with a convolution kernel (random shapes and dtypes; one raw
    flow per direction, FORWARD first), render1d / render2d."""
    rng = np.random.default_rng(2718)
    for trial in range(trials):
        h, w = int(rng.integers(1, 30)), int(rng.integers(1, 40))
        n = int(rng.integers(1, 5))
        flows = [rng.normal(0, 1.5, (h, w, 2)).astype(np.float32) for _ in range(n)]
        for f in flows[1:]:
            f[rng.random((h, w, 2)) < 0.3] = 0
        wf, hf = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        kh, kw_ = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        kernel = rng.normal(0, 0.3, (kh, kw_))
        kernel = [kernel, kernel.astype(np.float32), np.rint(kernel * 4).astype(np.int64)][int(rng.integers(3))]
        raws = [rng.normal(0, 3.0, (h, w, 2)).astype(np.float32) for _ in range(2)]
        arr = np.abs(rng.normal(0, 2, (h, w))).astype(np.float32)
        scale, binary = float(rng.choice([0.25, 0.5, 1.0, 2.0])), bool(rng.integers(2))
        yield dict(trial=trial, h=h, w=w, flows=flows, wf=wf, hf=hf, kernel=kernel, raws=raws, arr=arr, scale=scale,
                   binary=binary)


def live_mask_specs(count=1500):
    """(spec, shape) pairs walking the mask argument grammar at random: every rule name, 0-5 arguments from pixels /
    percentages / blanks / junk, dimensions larger than the frame, ':inv'."""
    import random
    rnd = random.Random(5)
    names = ["border", "border-top", "border-right", "border-bottom", "border-left", "hline", "vline", "circle",
             "rect", "grid", "zeros", "ones", "Border", "CIRCLE", "Rect"]
    tokens = ["", "0", "1", "2", "3", "4", "7", "15", "200", "5%", "50%", "120%", "x"]
    out = []
    for _ in range(count):
        spec = ":".join([rnd.choice(names)] + [rnd.choice(tokens) for _ in range(rnd.choice([0, 1, 1, 2, 2, 3, 4, 5]))])
        spec += rnd.choice(["", ":inv"])
        out.append((spec, rnd.choice([(37, 53), (60, 80), (8, 8), (5, 9), (1, 1)])))
    return out


def live_iteration_cases(trials=300):
    """Random frame ranges, lengths, STAY schedules and SKIP windows of FlowSource's iteration logic: one dict per trial
    (mode 0: no lock, 1: STAY over `pairs`, 2: SKIP while a < t < b)."""
    rng = np.random.default_rng(31337)
    for trial in range(trials):
        fps = float(rng.choice([1.0, 10.0, 24.0, 29.97]))
        start = int(rng.integers(0, 4))
        end = start + int(rng.integers(1, 8))
        ckpt = int(rng.integers(start, end + 1))
        length = None if rng.random() < 0.2 else int(rng.integers(0, 25))
        mode = int(rng.integers(3))
        pairs, window = None, None
        if mode == 1:
            pairs, t0 = [], 0.0
            for _ in range(int(rng.integers(1, 4))):
                t0 += float(rng.uniform(0, 6 / fps))
                d = float(rng.uniform(0, 5 / fps))
                pairs.append((t0, d))
                t0 += d
            pairs = tuple(pairs)
        elif mode == 2:
            window = tuple(sorted(float(v) for v in rng.uniform(0, 20 / fps, 2)))
        yield dict(trial=trial, fps=fps, start=start, end=end, ckpt=ckpt, length=length, mode=mode, pairs=pairs,
                   window=window)


def live_builder_cases(trials=400):
    """Random seek / duration / repeat / checkpoint / lock arguments of FlowSource.Builder over random base lengths and
    frame rates, streams included: (trial, builder kwargs, base_length, fps)."""
    rng = np.random.default_rng(8086)
    for trial in range(trials):
        kw = dict(direction=str(rng.choice(["forward", "backward"])),
                  seek_time=None if rng.random() < 0.4 else float(rng.choice([0.0, 0.25, 1.0, 2.5, 3.3333])),
                  duration_time=None if rng.random() < 0.4 else float(rng.choice([0.1, 0.5, 1.0, 7.0])),
                  repeat=int(rng.choice([0, 1, 1, 2, 5])),
                  seek_ckpt=None if rng.random() < 0.6 else int(rng.integers(0, 200)))
        r = rng.random()
        if r < 0.3:
            kw.update(lock_mode="stay", lock_expr=str(rng.choice(["0.5,0.2", "(0.2,0.4),(1,0.2)", "(0,1)"])))
        elif r < 0.5:
            kw.update(lock_mode="skip", lock_expr="t > 1")
        base_length = int(rng.choice([-1, 0, 1, 7, 50, 300]))
        fps = float(rng.choice([10.0, 25.0, 29.97, 60.0]))
        yield trial, kw, base_length, fps


BUILDER_FIELDS = ("start_frame", "end_frame", "length", "ckpt_start_frame", "is_stream", "repeat", "seek_time",
                  "base_length", "lock_expr_stay")
ARCHIVE_BUILDER_FIELDS = ("width", "height", "framerate", "base_length", "length", "start_frame", "end_frame")
UNIQUE_PATH_NAMES = ("a.flow.zip", "clip.mp4", "x.000.flow.zip", "x.004.map.zip", "noext", "b.7.txt", "c.123", "d.tar.gz")


def live_archive_flows():
    rng = np.random.default_rng(3)
    return [rng.normal(0, 2, (6, 9, 2)).astype(np.float32) for _ in range(3)]


def as_json(value):
    """`value` as it reads back from JSON, tuples and lists kept apart ({"tuple": [...]}, {"list": [...]}) as == keeps
    them apart: the form the stored reference outcomes are compared in."""
    def enc(v):
        if isinstance(v, (tuple, list)):
            return {type(v).__name__: [enc(x) for x in v]}
        return v
    return json.loads(json.dumps(enc(value)))


def polar_values() -> np.ndarray:
    """float32 values x for polar-filter flows (x, 0): r = |x| exactly (the square of a float32 is exact in the
    float32 norm's sqrt away from under- / overflow) and a = 0 or pi.  Signed zeros, the integers 0..64 and
    their negatives, multiples of 0.1f and 0.3f, half-integers (rint's ties), squares that overflow, values
    whose square underflows, NaN, +-inf and a random normal block."""
    f = np.float32
    v = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e19, -1e19, 3e38, -3e38, 1e-20, 1e-39, 1e-45]
    v += list(range(-64, 65))
    v += [k * f(0.1) for k in range(-60, 61)] + [k * f(0.3) for k in range(-40, 41)]
    v += [k + 0.5 for k in range(-12, 12)]
    v += list(np.random.default_rng(21).normal(0, 3, 400)) + list(np.random.default_rng(22).normal(0, 40, 100))
    return np.array(v, f)


def polar_flow(x) -> np.ndarray:
    """The flow (x, 0) as a C-contiguous float32 (1, N, 2) array."""
    x = np.asarray(x, np.float32).ravel()
    return np.ascontiguousarray(np.stack([x, np.zeros_like(x)], axis=-1)[None])


def build_host_check(tmp_path, source_name):
    """tools/<source_name> (a stand-alone program: exit status 2 and a usage line when run without arguments) built by
    the first host compiler there is: with the sanitizers where their runtime links and the program runs, without them
    otherwise.  (program, sanitized).  A machine without any host compiler skips; a compiler that cannot build the plain
    program, or whose program does not start, fails the test with what it said."""
    source = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", source_name)
    compilers = [c for c in ("g++", "clang++", "c++") if shutil.which(c) is not None]
    if not compilers:
        pytest.skip("no host compiler here")

    def build(compiler, flags, tag):
        out = str(tmp_path / ("check_" + compiler.replace("+", "x") + tag))
        built = subprocess.run([compiler, "-O1", "-g", "-std=c++17", *flags, source, "-o", out], capture_output=True, text=True)
        if built.returncode != 0:
            return None, built.stderr
        ran = subprocess.run([out], capture_output=True, text=True)
        if ran.returncode == 2 and "usage" in ran.stderr:
            return out, ""
        return None, ran.stderr

    for compiler in compilers:
        program, _ = build(compiler, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "_san")
        if program:
            return program, True
    said = []
    for compiler in compilers:
        program, stderr = build(compiler, [], "")
        if program:
            return program, False
        said.append(f"{compiler}: {stderr[-2000:]}")
    pytest.fail(f"no host compiler builds tools/{source_name}:\n" + "\n".join(said))
