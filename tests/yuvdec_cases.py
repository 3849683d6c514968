"""The frames the conversion back from YUV is compared on, for the device (tests/test_gpu_yuvdec.py) and for
host_convert_back (tests/test_yuvdec_ref.py): (name, the frame's bytes as a uint8 array, width, height, layout, matrix,
range, chroma, order).  Any bytes of the right number are a frame: the noise is drawn plane-wide."""
import itertools

import numpy as np

from tests import yuv_cases, yuvdec_ref

LAYOUTS = tuple(yuvdec_ref.LAYOUTS)
CHROMAS = yuvdec_ref.CHROMAS
# either side of the lane's 8 pixels and of odd edges; and the wave's 512 pixels
SIZES = [(w, h) for w in yuv_cases.WIDTHS for h in yuv_cases.HEIGHTS] + [(w, h) for w in (511, 512, 513) for h in (2, 3)]
OTHER_PAIRS = yuv_cases.OTHER_PAIRS
LEVELS = (0, 16, 128, 235, 240, 255)                    # the ranges' ends and middle: most combinations are out of gamut
SOLIDS = {"zero": (0, 0, 0), "full": (255, 255, 255), "black": (16, 128, 128), "white": (235, 128, 128),
          "y-low-v-high": (0, 128, 255), "y-high-u-low": (255, 0, 128), "u-high": (128, 255, 0), "v-high": (128, 0, 255)}
# sizes at which every named wrong form of the linear filter shows: edges on all sides, odd and even, several chroma rows
FILTER_SIZES = ((17, 5), (64, 6), (9, 7))


def noise(w: int, h: int, layout: str, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, yuvdec_ref.frame_bytes(w, h, layout), dtype=np.uint8)


def pack(y: np.ndarray, u: np.ndarray, v: np.ndarray, layout: str) -> np.ndarray:
    parts = [y.reshape(-1), np.stack([u, v], axis=-1).reshape(-1)] if layout == "nv12" else [y.reshape(-1), u.reshape(-1), v.reshape(-1)]
    return np.concatenate(parts).astype(np.uint8)


def blocks(triples: np.ndarray, layout: str):
    """A frame in which every (Y, U, V) of a (rows, columns, 3) grid fills a 2x2 block of pixels: (bytes, w, h)."""
    bw, bh = yuvdec_ref.LAYOUTS[layout]
    rows, cols = triples.shape[:2]
    y = triples[..., 0].repeat(2, axis=0).repeat(2, axis=1)
    u, v = (triples[..., k].repeat(2 // bh, axis=0).repeat(2 // bw, axis=1) for k in (1, 2))
    return pack(y, u, v, layout), 2 * cols, 2 * rows


def size_cases(layout: str, chroma: str):
    for w, h in SIZES:
        yield f"noise-{w}x{h}-{layout}-{chroma}", noise(w, h, layout, 1000 * w + h), w, h, layout, "bt601", "tv", chroma, "rgb"


def pair_cases():
    """The other matrices and ranges; in the other order."""
    for matrix, rng in OTHER_PAIRS:
        for layout in LAYOUTS:
            for chroma in CHROMAS:
                for w, h in ((5, 3), (17, 4), (64, 3)):
                    yield (f"noise-{w}x{h}-{layout}-{chroma}-{matrix}-{rng}-bgr", noise(w, h, layout, 77 * w + h), w, h, layout,
                           matrix, rng, chroma, "bgr")


def order_cases():
    for layout in LAYOUTS:
        for chroma in CHROMAS:
            for order in ("rgb", "bgr"):
                yield f"noise-33x5-{layout}-{chroma}-{order}", noise(33, 5, layout, 9), 33, 5, layout, "bt601", "tv", chroma, order


def frame_cases():
    for layout in LAYOUTS:
        for chroma in CHROMAS:
            yield f"frame-480x270-{layout}-{chroma}", noise(480, 270, layout, 5), 480, 270, layout, "bt601", "tv", chroma, "bgr"


def extreme_cases():
    combos = np.array(list(itertools.product(LEVELS, repeat=3)), np.uint8).reshape(12, 18, 3)
    near = yuvdec_ref.boundary_triples().reshape(9, 16, 3)
    for layout in LAYOUTS:
        bw, bh = yuvdec_ref.LAYOUTS[layout]
        for chroma in CHROMAS:
            for matrix, rng in yuvdec_ref.PAIRS:
                for name, (a, b, c) in SOLIDS.items():
                    data = pack(np.full((3, 9), a, np.uint8), np.full((-(-3 // bh), -(-9 // bw)), b, np.uint8),
                                np.full((-(-3 // bh), -(-9 // bw)), c, np.uint8), layout)
                    yield f"{name}-{layout}-{chroma}-{matrix}-{rng}", data, 9, 3, layout, matrix, rng, chroma, "rgb"
                data, w, h = blocks(combos, layout)
                yield f"levels-{layout}-{chroma}-{matrix}-{rng}", data, w, h, layout, matrix, rng, chroma, "rgb"
            data, w, h = blocks(near, layout)
            yield f"boundary-{layout}-{chroma}", data, w, h, layout, "bt601", "tv", chroma, "rgb"


def filter_cases():
    """Linear mode on noise at sizes where each wrong form of the filter changes the output
    (tests/test_yuvdec_ref.py asserts that it does)."""
    for layout in LAYOUTS:
        if yuvdec_ref.LAYOUTS[layout][0] == 1:
            continue
        for w, h in FILTER_SIZES:
            yield f"filter-{w}x{h}-{layout}", noise(w, h, layout, 31 * w + h), w, h, layout, "bt601", "tv", "linear", "rgb"


def wrong_forms(layout: str):
    """The wrong forms that exist for a layout: there is no vertical neighbour at 4:2:2."""
    return [f for f in yuvdec_ref.WRONG_FORMS if f != "wrong_side" or yuvdec_ref.LAYOUTS[layout][1] == 2]


def all_cases():
    for layout in LAYOUTS:
        for chroma in CHROMAS:
            yield from size_cases(layout, chroma)
    yield from pair_cases()
    yield from order_cases()
    yield from frame_cases()
    yield from extreme_cases()
    yield from filter_cases()


def want(case) -> np.ndarray:
    _, data, w, h, layout, matrix, rng, chroma, order = case
    return yuvdec_ref.convert_back(data, w, h, layout, matrix, rng, chroma, order)
