"""Lucas-Kanade cases beyond helpers.synth_pair: saturated frames, windows up to the largest accepted, frames down to
1x1 and pyramids of eight levels, for tests/test_lk_cases.py (CPU: what each family covers, as the restatement
tests/lk_ref.py says) and tests/test_gpu_lucaskanade_extremes.py (device: the kernels against the restatement on the
same cases).  Pure numpy, deterministic.

Why these: k_lk_track converts int32 products and pair sums df_k * g_k + df_k+4 * g_k+4 to float32.  On sine texture
they stay below 2^24, where the conversion is exact however the sum is grouped; 0/255 frames reach 2 * 8160 * 4080.
A's scalar tail runs win % 4 columns and b's win % 8, so the windows cover every residue.  Frames smaller than the
window, one point for the whole frame, and eight pyramid levels are the ends of the geometry.

  content   eleven pairs of 40x56 frames, each with windows 3, 7, 8, 9, 15 and 16, max_level 2, step 3 (1 where said)
  window    90x120 binary 2x2 blocks against themselves rolled, step 30, max_level 1, windows 3..65; 127 on a 300x400
            synth_pair, step 150; 255 on 64x80, step 40
  geometry  random frames from 1x1 to 6x8 with windows 3 and 15, max_level 2, step 1; 40x56 with steps 100, 56, 55
  deep      520x600 synth_pair, windows 3 and 4, max_level 12 and 50 (both give levels 0..7), step 40
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from . import lk_ref
from .helpers import synth_pair

Case = namedtuple("Case", "name family prev next win max_level step")

H, W = 40, 56
CONTENT_WINDOWS = (3, 7, 8, 9, 15, 16)
# the issue's windows, and 6, 10 and 34: without them no window is 2 or 6 mod 8, and none of at least 32 is 2 mod 4
FAMILY_WINDOWS = (3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 24, 31, 32, 33, 34, 40, 63, 64, 65)
GEOMETRY_SHAPES = ((1, 1), (1, 2), (2, 1), (1, 40), (40, 1), (2, 2), (3, 3), (4, 4), (2, 37), (37, 2), (6, 8))
DEEP_SHAPE = (520, 600)
PAIR_SUM_MAX = 2 * 8160 * 4080          # two products of a difference of 255 * 32 and a Scharr value of 16 * 255


def _roll(a, dy, dx):
    return np.roll(a, (dy, dx), (0, 1))


def binary(h=H, w=W, seed=11):
    return (np.random.default_rng(seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)


def blocks(h=H, w=W, side=4, seed=12):
    cells = np.random.default_rng(seed).integers(0, 2, (-(-h // side), -(-w // side)))
    return (np.kron(cells, np.ones((side, side), np.int64))[:h, :w] * 255).astype(np.uint8)


def step_edge(at, h=H, w=W):
    a = np.zeros((h, w), np.uint8)
    a[:, at:] = 255
    return a


def bright_pixel(y, x, h=H, w=W):
    a = np.full((h, w), 97, np.uint8)
    a[y, x] = 255
    return a


def faint(h=H, w=W, seed=13, amplitude=1):
    """97 plus {0, amplitude} noise.  With amplitude 1 the smaller eigenvalue stays just under the tracker's 1e-4
    (every point is lost, the nearest by a tenth); with 2 it is four times that and falls on both sides."""
    return (97 + amplitude * np.random.default_rng(seed).integers(0, 2, (h, w))).astype(np.uint8)


def ramp(h=H, w=W):
    """9 per column and 6 per row from -120: 0 in one corner region, 255 in the other."""
    y, x = np.mgrid[0:h, 0:w]
    return np.clip(9 * x + 6 * y - 120, 0, 255).astype(np.uint8)


def content_pairs():
    """{name: (prev, next, step)}."""
    bn, bl = binary(), blocks()
    return {
        "binary_rolled": (bn, _roll(bn, 1, 2), 3),
        "binary_independent": (bn, binary(seed=21), 3),
        "blocks_rolled": (bl, _roll(bl, 2, -3), 3),
        "blocks_inverse": (bl, 255 - bl, 3),
        "step_edge": (step_edge(28), step_edge(31), 3),
        "bright_pixel": (bright_pixel(20, 28), bright_pixel(21, 29), 1),
        "faint": (faint(), _roll(faint(), 1, 2), 1),
        "faint_0_2": (faint(amplitude=2), _roll(faint(amplitude=2), 1, 2), 1),
        "ramp": (ramp(), _roll(ramp(), 1, 2), 3),
        "black_white": (np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8), 3),
        "white_white": (np.full((H, W), 255, np.uint8), np.full((H, W), 255, np.uint8), 3),
    }


def content_cases():
    return [Case(f"content_{name}_w{win}", "content", a, b, win, 2, step)
            for name, (a, b, step) in content_pairs().items() for win in CONTENT_WINDOWS]


def window_cases():
    a = blocks(90, 120, side=2, seed=14)
    out = [Case(f"window_w{win}", "window", a, _roll(a, 1, -2), win, 1, 30) for win in FAMILY_WINDOWS]
    a, b = synth_pair(300, 400, seed=15, shift=(3.0, 2.0), noise=5.0)
    out.append(Case("window_w127", "window", a, b, 127, 1, 150))
    a = blocks(64, 80, side=2, seed=16)
    out.append(Case("window_w255", "window", a, _roll(a, 1, -2), 255, 1, 40))
    return out


def geometry_cases():
    out = []
    for k, (h, w) in enumerate(GEOMETRY_SHAPES):
        rng = np.random.default_rng(300 + k)
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        # a's pixels moved by (1, 1), a quarter of them drawn again
        b = np.where(rng.random((h, w)) < 0.25, rng.integers(0, 256, (h, w), dtype=np.uint8), _roll(a, 1, 1))
        for win in (3, 15):
            out.append(Case(f"geometry_{h}x{w}_w{win}", "geometry", a, b.astype(np.uint8), win, 2, 1))
    bn = binary()
    for step in (100, 56, 55):
        for win in (3, 15):
            out.append(Case(f"geometry_step{step}_w{win}", "geometry", bn, _roll(bn, 1, 2), win, 2, step))
    return out


def deep_cases():
    a, b = synth_pair(*DEEP_SHAPE, seed=17, shift=(3.0, 2.0), noise=5.0)
    return [Case(f"deep_w{win}_l{levels}", "deep", a, b, win, levels, 40) for win in (3, 4) for levels in (12, 50)]


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(content_cases() + window_cases() + geometry_cases() + deep_cases())


def case(name):
    (c,) = [c for c in all_cases() if c.name == name]
    return c


def family(key):
    return [c for c in all_cases() if c.family == key]


Run = namedtuple("Run", "flow trace probe")


@functools.lru_cache(maxsize=None)
def run(name) -> Run:
    """The restatement on a case's grid, once: the reference function's flow [h][w][2] (read-only), the trace
    [points][levels][4] and calc_pyr_lk's probe."""
    c = case(name)
    h, w = c.prev.shape
    p0 = lk_ref.grid_points(h, w, c.step)
    probe = {}
    p1, trace = lk_ref.calc_pyr_lk(c.prev, c.next, p0, c.win, c.max_level, with_trace=True, probe=probe)
    q, p = len(range(0, h, c.step)), len(range(0, w, c.step))
    flow = lk_ref.expand((p1 - p0).reshape(q, p, 2), h, w, c.step)
    flow.setflags(write=False)
    return Run(flow, trace, probe)


def level_steps(name):
    """[(sum, max)] per level of the steps the restatement ran over the case's grid points: what last_stats reports."""
    steps = run(name).trace[:, :, 2].astype(np.int64)
    return [(int(steps[:, l].sum()), int(steps[:, l].max())) for l in range(steps.shape[1])]


def code_counts(names):
    """{trace code: count} over the grid points and levels of the named cases."""
    codes = np.concatenate([run(n).trace[:, :, 3].ravel() for n in names]).astype(np.int64)
    return {c: int(np.count_nonzero(codes == c)) for c in range(4)}


def stop_counts(names):
    stops = np.concatenate([run(n).probe["stop"].ravel() for n in names])
    return {s: int(np.count_nonzero(stops == s)) for s in range(5)}


def sample_points(c: Case, at_most: int) -> np.ndarray:
    """At most `at_most` of the case's grid points, evenly spread over the grid's order."""
    p0 = lk_ref.grid_points(*c.prev.shape, c.step)
    return p0[np.unique(np.linspace(0, len(p0) - 1, min(at_most, len(p0))).round().astype(np.int64))]
