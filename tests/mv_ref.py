"""Numpy restatement of the motion-vector painter (the checker of transflow_amd/motionvectors.py), written from its
specification, and the two generators of vector tables the tests draw from.

The specification: flow = zeros((H, W, 2), float32); for each vector in list order, with `source == -1` required,

    rows    src_y - h // 2 : src_y + h // 2        columns    src_x - w // 2 : src_x + w // 2

as a numpy basic slice of the flow gets the pair (-(motion_x / motion_scale), -(motion_y / motion_scale)), the quotients
being Python's int / int (the correctly rounded float64) and the assignment rounding them to float32.  Nothing here
uses numpy's own slicing for the bounds: `resolve_slice` states the rule, and tests/test_mv_ref.py checks it against
`slice.indices` and against flows the reference itself painted (tests/golden/mv_*.npz).
"""
import numpy as np

FIELDS = ("source", "w", "h", "src_x", "src_y", "motion_x", "motion_y", "motion_scale")
DTYPE = np.dtype([(name, np.int32) for name in FIELDS])


def resolve_slice(a: int, b: int, n: int):
    """The range [lo, hi) that the basic slice a:b selects on an axis of length n (empty when lo >= hi): a negative
    bound counts from the end, then each bound is clamped to [0, n]."""
    def bound(x):
        if x < 0:
            x += n
        return min(max(x, 0), n)
    return bound(a), bound(b)


def check_vector(index: int, v) -> None:
    if int(v["source"]) != -1:
        raise ValueError(f"vector {index} has source {int(v['source'])}, not -1")
    if int(v["motion_scale"]) == 0:
        raise ValueError(f"vector {index} has motion_scale 0")


def rect_and_value(v, width: int, height: int):
    """(i0, i1, j0, j1) after slice resolution and the float32 pair one vector paints."""
    w, h, sx, sy = int(v["w"]), int(v["h"]), int(v["src_x"]), int(v["src_y"])
    i0, i1 = resolve_slice(sy - h // 2, sy + h // 2, height)
    j0, j1 = resolve_slice(sx - w // 2, sx + w // 2, width)
    scale = int(v["motion_scale"])
    dx, dy = int(v["motion_x"]) / scale, int(v["motion_y"]) / scale
    return (i0, i1, j0, j1), (np.float32(-dx), np.float32(-dy))


def rects_and_values(vectors, width: int, height: int):
    n = 0 if vectors is None else len(vectors)
    rects, values = np.zeros((n, 4), np.int32), np.zeros((n, 2), np.float32)
    for k in range(n):
        check_vector(k, vectors[k])
        rects[k], values[k] = rect_and_value(vectors[k], width, height)
    return rects, values


def paint(vectors, width: int, height: int) -> np.ndarray:
    """The flow of one frame: float32 (H, W, 2).  Every rectangle is written through its resolved bounds (0 <= lo < hi
    <= n: nothing is left for numpy's slicing to interpret) in list order, so a later vector overwrites an earlier one."""
    flow = np.zeros((height, width, 2), np.float32)
    if vectors is None:
        return flow
    rects, values = rects_and_values(vectors, width, height)
    for (i0, i1, j0, j1), value in zip(rects.tolist(), values):
        if i0 < i1 and j0 < j1:
            flow[i0:i1, j0:j1] = value
    return flow


def bits(flow: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(flow, dtype=np.float32).view(np.uint32)


def records(rows) -> np.ndarray:
    """Rows (source, w, h, src_x, src_y, motion_x, motion_y, motion_scale) as a table."""
    return np.array([tuple(int(x) for x in r) for r in rows], dtype=DTYPE).reshape(-1)


KNOWN_SIZE = (64, 40)      # width, height
KNOWN_VECTORS = [(-1, 16, 16, 8, 8, 0, -3, 4), (-1, 16, 16, 4, 4, 5, 7, 4), (-1, 16, 16, -10, -10, 1, 1, 3),
                 (-1, 9, 7, 60, 38, -2, 1, 4)]


# ---- generators ----------------------------------------------------------------------------------------------------

def h264_like(width: int, height: int, seed: int, intra: float = 0.1) -> np.ndarray:
    """A P-frame's table as an H.264 decoder exports it: a 16 x 16 macroblock grid (blocks at the right and bottom
    edge reach past the frame, as coded frames are padded), each block absent (intra), whole, or split into 16x8, 8x16,
    8x8 or 4x4 partitions; dst is the partition's centre, motion is in quarter-pel units (motion_scale 4) up to
    +-64 px, and src = dst + motion // 4."""
    rng = np.random.default_rng(seed)
    splits = {0: [(16, 16)], 1: [(16, 8)], 2: [(8, 16)], 3: [(8, 8)], 4: [(4, 4)]}
    rows = []
    for by in range(0, height, 16):
        for bx in range(0, width, 16):
            if rng.random() < intra:
                continue
            pw, ph = splits[int(rng.integers(5))][0]
            base = rng.integers(-256, 257, 2)                      # the block's motion; partitions vary around it
            for oy in range(0, 16, ph):
                for ox in range(0, 16, pw):
                    m = np.clip(base + rng.integers(-8, 9, 2), -256, 256)
                    dst_x, dst_y = bx + ox + pw // 2, by + oy + ph // 2
                    rows.append((-1, pw, ph, dst_x + int(m[0]) // 4, dst_y + int(m[1]) // 4, int(m[0]), int(m[1]), 4))
    return records(rows)


def hostile(width: int, height: int, n: int, seed: int) -> np.ndarray:
    """Vectors that try the semantics: w, h uniform in 0..255, sources up to 300 px outside the frame on every side,
    scales that are not powers of two, motions in +-2^15, one in twenty with motion_x 0, a tenth of the table repeated
    at its end (duplicates); with rectangles this large most early vectors end up fully covered by later ones."""
    rng = np.random.default_rng(seed)
    t = np.zeros(n, DTYPE)
    t["source"] = -1
    t["w"], t["h"] = rng.integers(0, 256, n), rng.integers(0, 256, n)
    t["src_x"], t["src_y"] = rng.integers(-300, width + 301, n), rng.integers(-300, height + 301, n)
    t["motion_x"], t["motion_y"] = rng.integers(-2 ** 15, 2 ** 15 + 1, n), rng.integers(-2 ** 15, 2 ** 15 + 1, n)
    t["motion_scale"] = rng.choice([1, 2, 3, 4, 7, 16], n)
    t["motion_x"][rng.random(n) < 0.05] = 0
    if n >= 10:
        dup = rng.integers(0, n // 2, n // 10)
        t[n - len(dup):] = t[dup]
    return t
