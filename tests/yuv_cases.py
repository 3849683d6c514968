"""The frames the YUV conversion is compared on, for the device (tests/test_gpu_yuv.py) and for host_convert
(tests/test_yuv_ref.py): (name, rgb, layout, matrix, range)."""
import numpy as np

from tests import yuv_ref

LAYOUTS = tuple(yuv_ref.LAYOUTS)
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 129, 257)     # around the lane's 8 pixels and the wave's 512
HEIGHTS = (1, 2, 3, 4, 5)
OTHER_PAIRS = [p for p in yuv_ref.PAIRS if p != ("bt601", "tv")]
SOLIDS = {"black": (0, 0, 0), "white": (255, 255, 255), "red": (255, 0, 0), "green": (0, 255, 0), "blue": (0, 0, 255),
          "yellow": (255, 255, 0), "cyan": (0, 255, 255), "magenta": (255, 0, 255)}
# pc chroma that reaches 255.5 and is clamped, with neighbours that are not
PC_CLAMP = np.array([(0, 0, 255), (255, 0, 0), (0, 1, 255), (255, 1, 0), (1, 0, 255), (255, 0, 1), (0, 0, 254), (254, 0, 0)], np.uint8)


def noise(h: int, w: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def size_cases(layout: str):
    for w in WIDTHS:
        for h in HEIGHTS:
            yield f"noise-{w}x{h}-{layout}", noise(h, w, 1000 * w + h), layout, "bt601", "tv"


def pair_cases():
    for matrix, rng in OTHER_PAIRS:
        for layout in LAYOUTS:
            for w in (5, 17, 64):
                for h in (3, 4):
                    yield f"noise-{w}x{h}-{layout}-{matrix}-{rng}", noise(h, w, 77 * w + h), layout, matrix, rng


def frame_cases():
    for layout in LAYOUTS:
        yield f"frame-480x270-{layout}", noise(270, 480, 5), layout, "bt601", "tv"


def extreme_cases():
    for layout in LAYOUTS:
        for matrix, rng in yuv_ref.PAIRS:
            for name, colour in SOLIDS.items():
                yield f"{name}-{layout}-{matrix}-{rng}", np.full((3, 9, 3), colour, np.uint8), layout, matrix, rng
        for matrix in ("bt601", "bt709"):
            clamp = PC_CLAMP.reshape(2, 4, 3)
            yield f"pc-clamp-{layout}-{matrix}", clamp, layout, matrix, "pc"
            yield f"pc-clamp-blocks-{layout}-{matrix}", clamp.repeat(2, axis=0).repeat(2, axis=1), layout, matrix, "pc"
        near = yuv_ref.boundary_triples()
        near = near.reshape(-1, 16, 3)
        yield f"boundary-{layout}", near, layout, "bt601", "tv"
        yield f"boundary-blocks-{layout}", near.repeat(2, axis=0).repeat(2, axis=1), layout, "bt601", "tv"    # a triple a 2x2 block


def all_cases():
    for layout in LAYOUTS:
        yield from size_cases(layout)
    yield from pair_cases()
    yield from frame_cases()
    yield from extreme_cases()
