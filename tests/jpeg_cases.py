"""What the JPEG encoder's tests code and what they expect: the images, the three tables of cases, the fixtures
tests/golden/jpeg_*.npz, jpegopt_*.npz and jpegsub_*.npz (tools/capture_golden_jpeg.py writes them, the tests read them)
and hand-made histograms.  Nothing here is libjpeg's: that is tests/jpeg_ref.py.
"""
from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np

from tests.jpeg_ref import ZIGZAG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the images ------------------------------------------------------------------------------------------------------
def formula_image(height: int, width: int) -> np.ndarray:
    """The one image too large to store: arithmetic only, no generator.  Smooth ramps, a fine texture and hard edges."""
    i, j = np.mgrid[0:height, 0:width].astype(np.int64)
    r = (3 * j + i + ((i * j) >> 5)) & 255
    g = (5 * i + (j >> 1) + 37 * ((i >> 3) & 1) * ((j >> 4) & 1)) & 255
    b = ((i * i + 7 * j) >> 3) + 96 * (((i >> 2) + (j >> 2)) & 1) & 255
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def stored_image(height: int, width: int, seed: int) -> np.ndarray:
    """What a fixture stores: ramps with noise on them, so that blocks have a few coefficients and some runs."""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:height, 0:width]
    base = np.stack([4 * j + i, 255 - 3 * i - j, 2 * i + 2 * j + 40], axis=-1)
    return np.clip(base + rng.integers(-40, 41, (height, width, 3)), 0, 255).astype(np.uint8)


def rng_noise_image(height: int, width: int, seed: int) -> np.ndarray:
    """Uniform noise from numpy's generator: only for pictures whose pixels a fixture stores."""
    return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)


def checkerboard(height: int, width: int) -> np.ndarray:
    """8 x 8 squares of black and white: every block flat, neighbouring DCs 2040 quantisation steps apart at quality 100."""
    i, j = np.mgrid[0:height, 0:width]
    return np.repeat(((((i >> 3) + (j >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)


# ---- directed content: pure integer functions of (height, width, seed), so a fixture stores those, not pixels ---------
def _hash(seed: int, stream: int, n: int) -> np.ndarray:
    """n 64-bit values, splitmix64 of a counter: no generator whose stream a library might change."""
    with np.errstate(over="ignore"):
        z = (np.arange(1, n + 1, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x632BE59BD9B4E019)
             + np.uint64(stream) * np.uint64(0xD6E8FEB86659FD93)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def noise_image(height: int, width: int, seed: int = 11) -> np.ndarray:
    """Uniform noise from the integer hash: no library's generator."""
    return ((_hash(seed, 1, height * width * 3) >> np.uint64(40)) & np.uint64(255)).astype(np.uint8).reshape(height, width, 3)


# 2^14 cos(k pi / 16), k = 0 .. 31, and the DCT's basis vectors in those units (u = 0: 1 / sqrt 2)
_COS = np.array([16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0], np.int64)
_COS = np.concatenate([_COS, -_COS[7::-1]])
_COS = np.concatenate([_COS, _COS[15:0:-1]])
_BASIS = np.array([[11585 if u == 0 else _COS[(2 * x + 1) * u % 32] for x in range(8)] for u in range(8)], np.int64)


def _directed_blocks(by: int, bx: int, seed: int) -> np.ndarray:
    """int64 [by, bx, 8, 8], each block within -128 .. 127: one or two DCT basis functions at zigzag positions drawn
    from 1 .. 63, amplitudes (in units of the unquantised coefficient) from 1 .. 2047 with every size as likely as any
    other, or the sign pattern of the function times 1 .. 127.  Past about 500 the cosine clips towards its sign pattern.
    A block with two functions puts the run between them at the second's disposal: 0 .. 61."""
    n = by * bx
    h = [_hash(seed, stream, n).astype(np.int64) & 0x7FFFFFFF for stream in range(8)]
    out = np.zeros((n, 8, 8), np.int64)
    for b in range(n):
        first = 1 + h[0][b] % 63
        picks = [first]
        if h[1][b] % 3:                                                   # two in three blocks: a second one behind it
            gap = h[2][b] % 62
            picks.append(1 + (first + gap) % 63)
        for i, k in enumerate(picks):
            v, u = divmod(int(ZIGZAG[k]), 8)
            size = 1 + h[3 + i][b] % 11
            amp = (1 << (size - 1)) + (h[3 + i][b] >> 8) % (1 << (size - 1))
            sign = 1 - 2 * ((h[3 + i][b] >> 4) & 1)
            basis = np.outer(_BASIS[v], _BASIS[u])                        # 2^28 cos cos
            if (h[5 + i][b] & 3) == 0:
                out[b] += sign * (1 + (h[5 + i][b] >> 2) % 127) * np.sign(basis) // len(picks)
            else:
                out[b] += (sign * amp * basis + (1 << 29)) >> 30         # amp cu cv cos cos / 4
    return np.clip(out, -128, 127).reshape(by, bx, 8, 8)


def _tile(blocks: np.ndarray, height: int, width: int, step: int) -> np.ndarray:
    """[by, bx, 8, 8] -> a plane [height, width] with every value `step` pixels square."""
    by, bx = blocks.shape[:2]
    plane = blocks.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)
    return np.repeat(np.repeat(plane, step, axis=0), step, axis=1)[:height, :width]


def directed_luma(height: int, width: int, seed: int) -> np.ndarray:
    """A grey image whose luma blocks are `_directed_blocks` on 128: one or two AC coefficients each, anywhere, any size."""
    plane = 128 + _tile(_directed_blocks((height + 7) // 8, (width + 7) // 8, seed), height, width, 1)
    return np.repeat(plane.astype(np.uint8)[..., None], 3, axis=-1)


def directed_chroma(height: int, width: int, seed: int) -> np.ndarray:
    """The same patterns at 2 x 2 pixels on Cb and Cr.  MCUs take turns: constant luma with Cb and Cr following the
    pattern (the inverse of jccolor.c's matrix, clipped to the gamut), and the two saturated pairs blue / yellow
    (Cb 255 / 0) and red / cyan (Cr 255 / 0) on the pattern's sign, which no constant luma reaches."""
    my, mx = (height + 15) // 16, (width + 15) // 16
    cb = _tile(_directed_blocks(my, mx, 2 * seed + 1000), height, width, 2)
    cr = _tile(_directed_blocks(my, mx, 2 * seed + 1001), height, width, 2)
    kind = _tile(np.broadcast_to((_hash(seed, 9, my * mx) % np.uint64(4)).astype(np.int64).reshape(my, mx, 1, 1),
                                 (my, mx, 8, 8)), height, width, 2)
    r = 128 + ((91881 * cr + 32768) >> 16)
    g = 128 - ((22554 * cb + 46802 * cr + 32768) >> 16)
    b = 128 + ((116130 * cb + 32768) >> 16)
    smooth = np.clip(np.stack([r, g, b], axis=-1), 0, 255)
    blue_yellow = np.where((cb >= 0)[..., None], (0, 0, 255), (255, 255, 0))
    red_cyan = np.where((cr >= 0)[..., None], (255, 0, 0), (0, 255, 255))
    kind = kind[..., None]
    return np.where(kind < 2, smooth, np.where(kind == 2, blue_yellow, red_cyan)).astype(np.uint8)


def binary_noise(height: int, width: int, seed: int) -> np.ndarray:
    """Every channel of every pixel 0 or 255: the most bits an MCU gets from anything like a picture."""
    return ((_hash(seed, 0, height * width * 3) >> np.uint64(40)) & np.uint64(1)).astype(np.uint8).reshape(height, width, 3) * 255


def chroma_checker(height: int, width: int) -> np.ndarray:
    """16 x 16 squares, blue and yellow in the left half, red and cyan in the right: every chroma block flat, the Cb
    (left) and Cr (right) DCs of neighbouring MCUs 2040 quantisation steps apart at quality 100, as `checkerboard`'s luma."""
    i, j = np.mgrid[0:height, 0:width]
    odd = ((((i >> 4) + (j >> 4)) & 1) == 1)[..., None]
    left = np.where(odd, (255, 255, 0), (0, 0, 255))
    right = np.where(odd, (0, 255, 255), (255, 0, 0))
    return np.where((j < width // 2)[..., None], left, right).astype(np.uint8)


WIDE_LANE_SEED = 2                           # (with it: ZRL's code has 16 bits, the widest lane 70, luma AC 17 before limiting)


def wide_lane_image(height: int, width: int, seed: int) -> np.ndarray:
    """Grey noise (the integer hash, no library's generator) whose luma block (0, 0) is the DCT's highest basis function
    at full swing: at quality 95 it quantises to the single coefficient at zigzag 63, behind three ZRLs -- the only ZRLs
    of the image, so ZRL gets one of the longest codes of the luma AC table."""
    grey = ((_hash(seed, 0, height * width) >> np.uint64(40)) & np.uint64(255)).astype(np.int64).reshape(height, width)
    x = np.arange(8)
    c = np.cos((2 * x + 1) * 7 * np.pi / 16)
    grey[:8, :8] = np.rint(128 + 127 * np.outer(c, c)).astype(np.int64)
    return np.repeat(grey.astype(np.uint8)[..., None], 3, axis=-1)


# kind -> its maker.  The kinds are what the fixtures name as `content`: "smooth" and "binary" are jpegsub_*.npz's names
# for "formula" and "binary_noise", and their "noise" is the hash's; the generator's noise is stored as pixels only
_SEEDED = {"stored": stored_image, "rng_noise": rng_noise_image, "noise": noise_image, "directed_luma": directed_luma,
           "directed_chroma": directed_chroma, "binary_noise": binary_noise, "binary": binary_noise,
           "wide_lane": wide_lane_image}
_UNSEEDED = {"formula": formula_image, "smooth": formula_image, "checker": checkerboard, "chroma_checker": chroma_checker}


def made_image(kind: str, height: int, width: int, seed=None) -> np.ndarray:
    if kind in _UNSEEDED:
        return _UNSEEDED[kind](height, width)
    return _SEEDED[kind](height, width, int(seed))


# ---- baseline: 4:2:0 with the Annex K tables (tests/golden/jpeg_<name>.npz) -------------------------------------------
# name -> (height, width, content, quality, restart_mcus); content is a kind, or (kind, seed)
BASELINE_CASES = {
    "1x1": (1, 1, "stored", 50, 4),
    "9x7": (9, 7, "stored", 50, 4),
    "16x16": (16, 16, "stored", 50, 4),
    "17x33": (17, 33, "stored", 50, 4),
    "45x61": (45, 61, "stored", 50, 4),
    "24x40": (24, 40, "stored", 50, 4),
    "8x100": (8, 100, "stored", 50, 4),
    "33x47_noise_q100": (33, 47, "rng_noise", 100, 4),
    "33x47_noise_q1": (33, 47, "rng_noise", 1, 4),
    "32x32_checker_q100": (32, 32, "checker", 100, 4),
    "45x61_r1": (45, 61, "stored", 50, 1),
    "45x61_r2": (45, 61, "stored", 50, 2),
    "45x61_r3": (45, 61, "stored", 50, 3),
    "45x61_r8": (45, 61, "stored", 50, 8),              # the library's default interval
    "45x61_r100": (45, 61, "stored", 50, 100),          # more than the 12 MCUs: one interval, no marker
    "270x480_q50": (270, 480, "formula", 50, 4),
    "270x480_q95": (270, 480, "formula", 95, 4),
    # directed content (kind, seed): the seeds and qualities are those at which tests/test_jpeg_ref.py's coverage holds
    "luma_s10_q100": (96, 96, ("directed_luma", 10), 100, 3),
    "luma_s57_q100": (96, 96, ("directed_luma", 57), 100, 5),
    "luma_s19_q99": (96, 96, ("directed_luma", 19), 99, 1),
    "luma_s22_q98": (96, 96, ("directed_luma", 22), 98, 8),
    "luma_s24_q95": (96, 96, ("directed_luma", 24), 95, 2),
    "luma_s0_q50": (96, 96, ("directed_luma", 0), 50, 4),
    "chroma_s14_q100": (96, 96, ("directed_chroma", 14), 100, 3),
    "chroma_s0_q100": (96, 96, ("directed_chroma", 0), 100, 5),
    "chroma_s17_q100": (96, 96, ("directed_chroma", 17), 100, 6),
    "chroma_s44_q99": (96, 96, ("directed_chroma", 44), 99, 1),
    "chroma_s4_q98": (96, 96, ("directed_chroma", 4), 98, 8),
    "chroma_s10_q98": (96, 96, ("directed_chroma", 10), 98, 7),
    "chroma_s44_q65": (96, 96, ("directed_chroma", 44), 65, 2),
    "chroma_s0_q50": (96, 96, ("directed_chroma", 0), 50, 4),
    "32x48_binary_q100": (32, 48, ("binary_noise", 129), 100, 2),      # the fattest MCUs: 600 bytes, ten trips of the flush
    "32x64_chroma_checker_q100": (32, 64, "chroma_checker", 100, 4),   # chroma DC categories 10 and 11
    # interval counts around k_slot_scan's 1024 per trip
    "512x512_r1": (512, 512, "formula", 50, 1),                         # 1024: one full trip
    "16x16400_r1": (16, 16400, "formula", 50, 1),                       # 1025: one element in the second
    "730x725_r1": (730, 725, "formula", 50, 1),                         # 46 x 46 = 2116: three trips, ragged edges
    # the largest sizes libjpeg writes (JPEG_MAX_DIMENSION 65500; tf_jpeg_create admits the format's 65535, which
    # tests/test_gpu_jpeg.py holds to `encode` itself), at the library's default interval
    "1x65500": (1, 65500, "formula", 50, 8),                            # 4094 MCUs in a row, three of four luma blocks dummies
    "65500x1": (65500, 1, "formula", 50, 8),                            # ... in a column
    "40x4099": (40, 4099, "formula", 50, 8),                            # 257 MCUs a row: no power of two
}

# ---- the frame's own tables, 4:2:0 (tests/golden/jpegopt_<name>.npz): as BASELINE_CASES ------------------------------
OWN_TABLES_CASES = {name: case for name, case in BASELINE_CASES.items() if case[0] <= 96 and case[1] <= 96}
OWN_TABLES_CASES["270x480_q95"] = BASELINE_CASES["270x480_q95"]        # luma AC: 17 bits before limiting, 16 after
OWN_TABLES_CASES["224x224_wide_lane"] = (224, 224, ("wide_lane", WIDE_LANE_SEED), 95, 4)   # a lane of more than 64 bits

# ---- the layouts (tests/golden/jpegsub_<name>_s<subsampling>.npz) -----------------------------------------------------
# the grid the restatement is held to Pillow on (tests/test_jpeg_sub_ref.py)
GRID_SIZES = ((1, 1), (8, 8), (7, 9), (9, 17), (16, 16), (17, 33), (23, 41), (8, 15), (8, 16), (8, 17), (40, 72))
GRID_QUALITIES = (10, 50, 90, 100)
GRID_INTERVALS = (1, 3, 8)

# name -> (height, width, kind, seed, quality, restart_mcus, optimize): the device cases, each captured at subsampling 0 and
# 1.  Sizes are (height, width).
LAYOUT_CASES = {
    "1x1": (1, 1, "smooth", 0, 50, 4, False),
    "8x8": (8, 8, "smooth", 0, 50, 4, False),                   # one block; at 4:2:2 the second luma block is a dummy
    "7x9": (7, 9, "smooth", 0, 50, 4, False),                   # both edges replicated, an odd block grid
    "9x17": (9, 17, "smooth", 0, 50, 4, False),
    "8x15": (8, 15, "smooth", 0, 50, 4, False),                 # around the 4:2:2 MCU width
    "8x16": (8, 16, "smooth", 0, 50, 4, False),
    "8x17": (8, 17, "smooth", 0, 50, 4, False),
    "17x33": (17, 33, "smooth", 0, 50, 4, False),
    "23x41_r1": (23, 41, "smooth", 0, 50, 1, False),            # odd MCU counts per interval, intervals that wrap rows,
    "23x41_r3": (23, 41, "smooth", 0, 50, 3, False),            # a short last interval
    "23x41_r5": (23, 41, "smooth", 0, 50, 5, False),
    "40x72_r1": (40, 72, "smooth", 0, 50, 1, False),            # more than 8 intervals: RSTn wraps
    "33x47_noise_q100": (33, 47, "noise", 11, 100, 3, False),   # fat MCUs: the LDS bit buffer, the slot bound
    "33x47_binary_q10": (33, 47, "binary", 129, 10, 3, False),  # long zero runs, ZRLs
    "1x1_opt": (1, 1, "smooth", 0, 50, 4, True),
    "8x8_opt": (8, 8, "smooth", 0, 50, 4, True),
    "7x9_opt": (7, 9, "smooth", 0, 50, 4, True),
    "9x17_opt": (9, 17, "smooth", 0, 50, 4, True),
    "8x15_opt": (8, 15, "smooth", 0, 50, 4, True),
    "8x17_opt": (8, 17, "smooth", 0, 50, 4, True),
    "17x33_opt": (17, 33, "smooth", 0, 50, 4, True),
    "23x41_r3_opt": (23, 41, "smooth", 0, 50, 3, True),
    "33x47_noise_q100_opt": (33, 47, "noise", 11, 100, 3, True),
    "33x47_binary_q10_opt": (33, 47, "binary", 129, 10, 3, True),
}
LAYOUT_CASE_SUBSAMPLINGS = (0, 1)

# a fixture's family is the prefix of its file name
CASES = {"jpeg": BASELINE_CASES, "jpegopt": OWN_TABLES_CASES, "jpegsub": LAYOUT_CASES}


def case_image(family: str, name: str) -> np.ndarray:
    """The picture of a case: what tools/capture_golden_jpeg.py gives Pillow."""
    case = CASES[family][name]
    h, w = case[:2]
    if family == "jpegsub":
        kind, seed = case[2:4]
    elif isinstance(case[2], tuple):
        kind, seed = case[2]
    else:                                                                 # the same picture for every "stored" case of a size
        kind, seed = case[2], {"stored": h * 1000 + w, "rng_noise": 7}.get(case[2])
    return made_image(kind, h, w, seed)


def fixture_path(family: str, name: str, subsampling: int | None = None) -> str:
    return os.path.join(GOLDEN, f"{family}_{name}.npz" if subsampling is None else f"{family}_{name}_s{subsampling}.npz")


class Case(NamedTuple):
    image: np.ndarray
    quality: int
    restart_mcus: int
    subsampling: int
    optimize: bool
    jpeg: bytes                                                           # the file libjpeg wrote


def load_case(path: str) -> Case:
    """A fixture of any family.  It stores its image, or the recipe of it: a kind, a size and a seed (the first fixtures
    name no kind: "formula").  Only jpegsub_*.npz store a layout and whether the tables are the frame's own; for the
    others both follow from the family."""
    family = os.path.basename(path).split("_")[0]
    with np.load(path) as z:
        if "image" in z.files:
            image = z["image"]
        else:
            kind = str(z["content"]) if "content" in z.files else "formula"
            image = made_image(kind, int(z["height"]), int(z["width"]), z["seed"] if "seed" in z.files else None)
        subsampling, optimize = (int(z["subsampling"]), bool(z["optimize"])) if family == "jpegsub" else (2, family == "jpegopt")
        return Case(image, int(z["quality"]), int(z["restart_mcus"]), subsampling, optimize, z["jpeg"].tobytes())


# ---- hand-made histograms ------------------------------------------------------------------------------------------------
def fibonacci_counts(depth: int) -> np.ndarray:
    """256 counts whose `depth` used symbols are 1, 2, 3, 5, 8 ...: every count is above the sum of all before the one
    before it, so with the reserved symbol the code is a comb and its longest size is `depth`.  33 is the shortest
    that libjpeg refuses (its counts sum to 15 million: far below the selection sentinel)."""
    counts = np.zeros(256, np.uint32)
    a, b = 1, 2
    for i in range(depth):
        counts[i] = a
        a, b = b, a + b
    return counts


def limiting_counts() -> np.ndarray:
    """A comb of 24 sizes under 30 symbols that each outweigh it: sizes up to 29, one or two symbols at each above 16,
    so the limiting loop runs for every length from 29 down to 17, and for most more than once."""
    counts = fibonacci_counts(24)
    counts[100:130] = 300000
    return counts


def first_difference(got: bytes, want: bytes) -> str:
    n = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at byte {n}: {got[n:n + 8].hex()} / {want[n:n + 8].hex()}"
