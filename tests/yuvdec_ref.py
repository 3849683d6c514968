"""DESIGN.md section 22 restated for the tests, independently of transflow_amd/yuvdec.py's host_convert_back: the rule that
builds the inverse's integer coefficients (in exact fractions), the chroma expansion by explicit index arrays (and the
named wrong forms of the linear filter), the pixels by plain numpy, `model`, the real-valued equations in float64 clipped
to [0, 255], and a Y4M parser and builder of its own."""
import functools
from fractions import Fraction

import numpy as np

from tests import yuv_ref

LAYOUTS = yuv_ref.LAYOUTS                                   # the chroma block, bw x bh
KR_KB = yuv_ref.KR_KB
PAIRS = yuv_ref.PAIRS
CHROMAS = ("replicate", "linear")
# the linear filter gone wrong in a named way (expand's `wrong`)
WRONG_FORMS = ("bias_swapped", "wrong_side", "unclamped", "replicate")

# the issue's table (cy, rv, gu, gv, bu): what the rule has to give
TABLE = {
    ("bt601", "tv"): (76309, 104597, -25675, -53279, 132201),
    ("bt601", "pc"): (65536, 91881, -22553, -46802, 116130),
    ("bt709", "tv"): (76309, 117489, -13975, -34925, 138438),
    ("bt709", "pc"): (65536, 103206, -12276, -30679, 121609),
}

# why a file is not read, mirrored from transflow_amd/yuvdec.py's REJECT_REASONS
REJECT = ("not_y4m", "bad_header", "interlaced", "chroma", "bad_frame_header")
TAGS = {"C420jpeg": "yuv420p", "C420mpeg2": "yuv420p", "C420paldv": "yuv420p", "C420": "yuv420p", "C422": "yuv422p",
        "C444": "yuv444p"}


class Rejected(Exception):
    def __init__(self, reason: str):
        Exception.__init__(self, reason)
        self.reason = reason


# ---- the coefficients ----------------------------------------------------------------------------------------------------
def inverse_scales(rng: str):
    return (Fraction(255, 219), Fraction(255, 224)) if rng == "tv" else (Fraction(1), Fraction(1))


def real_inverse(matrix: str, rng: str):
    """(cy, rv, gu, gv, bu) as exact fractions."""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    s_y, s_c = inverse_scales(rng)
    return (s_y, 2 * (1 - kr) * s_c, -2 * (1 - kb) * kb / kg * s_c, -2 * (1 - kr) * kr / kg * s_c, 2 * (1 - kb) * s_c)


@functools.lru_cache(maxsize=None)
def rule(matrix: str, rng: str):
    """((cy, rv, gu, gv, bu) as ints with 16 fractional bits, the Y offset)."""
    return tuple(yuv_ref.rint_even(v * 65536) for v in real_inverse(matrix, rng)), (16 if rng == "tv" else 0)


# ---- the planes -----------------------------------------------------------------------------------------------------------
def frame_bytes(w: int, h: int, layout: str) -> int:
    return yuv_ref.frame_bytes(h, w, layout)


def unpack(data, w: int, h: int, layout: str):
    """(Y, U, V) uint8 planes of a frame's bytes, U and V of the chroma size whatever the packing."""
    raw = np.frombuffer(bytes(data), np.uint8)
    bw, bh = LAYOUTS[layout]
    dw, dh = -(-w // bw), -(-h // bh)
    assert raw.size == w * h + 2 * dw * dh
    y = raw[:w * h].reshape(h, w)
    if layout == "nv12":
        pairs = raw[w * h:].reshape(dh, dw, 2)
        return y, pairs[..., 0], pairs[..., 1]
    return y, raw[w * h:w * h + dw * dh].reshape(dh, dw), raw[w * h + dw * dh:].reshape(dh, dw)


def expand(p: np.ndarray, w: int, h: int, layout: str, chroma: str, wrong: str = None) -> np.ndarray:
    """int64 (h, w): the chroma sample at every pixel.  wrong: one of WRONG_FORMS, for the tests that show a case tells
    the right filter from it."""
    bw, bh = LAYOUTS[layout]
    p = p.astype(np.int64)
    dh, dw = p.shape
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    if bw == 1:
        return p[ys, xs]
    r, c = ys // bh, xs // 2
    if chroma == "replicate" or wrong == "replicate":
        return p[r, c]
    assert chroma == "linear"

    def at(rows, cols):
        if wrong == "unclamped":                            # whatever lies beside the plane's row in memory
            return p.reshape(-1)[(rows * dw + cols) % p.size]
        return p[np.clip(rows, 0, dh - 1), np.clip(cols, 0, dw - 1)]

    odd_x = (xs & 1) == 1
    beside = c + np.where(odd_x, 1, -1)                     # the neighbour on the pixel's side
    if bh == 1:
        even_add, odd_add = (2, 1) if wrong == "bias_swapped" else (1, 2)
        return (3 * at(r, c) + at(r, beside) + np.where(odd_x, odd_add, even_add)) >> 2
    odd_y = (ys & 1) == 1
    step = np.where(odd_y, 1, -1)
    other = r + (-step if wrong == "wrong_side" else step)  # below for an odd row, above for an even one
    s_cur = 3 * at(r, c) + at(other, c)
    s_beside = 3 * at(r, beside) + at(other, beside)
    even_add, odd_add = (7, 8) if wrong == "bias_swapped" else (8, 7)
    return (3 * s_cur + s_beside + np.where(odd_x, odd_add, even_add)) >> 4


def pixels(y: np.ndarray, u: np.ndarray, v: np.ndarray, matrix: str, rng: str) -> np.ndarray:
    """uint8 (..., 3) RGB of Y, U', V' at every pixel."""
    (cy, rv, gu, gv, bu), yo = rule(matrix, rng)
    y, u, v = y.astype(np.int64) - yo, u.astype(np.int64) - 128, v.astype(np.int64) - 128
    acc = np.stack([cy * y + rv * v, cy * y + gu * u + gv * v, cy * y + bu * u], axis=-1) + 32768
    assert np.abs(acc).max() < 1 << 31                      # the format's claim: int32 is enough
    return np.clip(acc >> 16, 0, 255).astype(np.uint8)


def convert_back(data, w: int, h: int, layout: str, matrix: str = "bt601", rng: str = "tv", chroma: str = "replicate",
                 order: str = "rgb", wrong: str = None) -> np.ndarray:
    """uint8 (h, w, 3) in `order` of a frame's bytes."""
    y, u, v = unpack(data, w, h, layout)
    rgb = pixels(y, expand(u, w, h, layout, chroma, wrong), expand(v, w, h, layout, chroma, wrong), matrix, rng)
    return np.ascontiguousarray(rgb[..., ::-1]) if order == "bgr" else rgb


def model(yuv: np.ndarray, matrix: str, rng: str) -> np.ndarray:
    """float64 (..., 3) RGB of (..., 3) Y, U, V by the real equations, clipped to [0, 255]."""
    kr, kb = (float(v) for v in KR_KB[matrix])
    kg = 1.0 - kr - kb
    s_y, s_c = (float(v) for v in inverse_scales(rng))
    t = yuv.astype(np.float64)
    luma = s_y * (t[..., 0] - (16.0 if rng == "tv" else 0.0))
    pb, pr = s_c * (t[..., 1] - 128.0), s_c * (t[..., 2] - 128.0)
    red = luma + 2.0 * (1.0 - kr) * pr
    blue = luma + 2.0 * (1.0 - kb) * pb
    green = (luma - kr * red - kb * blue) / kg
    return np.clip(np.stack([red, green, blue], axis=-1), 0.0, 255.0)


@functools.lru_cache(maxsize=None)
def boundary_triples(per_channel: int = 24) -> np.ndarray:
    """(6 * per_channel, 3) uint8 (Y, U, V): for each of R, G and B of bt601 / tv, the triples of the cube whose
    accumulator lies nearest above a rounding boundary (low 16 bits smallest) and nearest below one (largest), among
    those the clamp leaves alone."""
    (cy, rv, gu, gv, bu), yo = rule("bt601", "tv")
    uv = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int64)
    u, v = uv[:, 0] - 128, uv[:, 1] - 128
    chroma_terms = (rv * v, gu * u + gv * v, bu * u)
    best = [[] for _ in range(6)]
    for luma in range(256):
        for i, term in enumerate(chroma_terms):
            acc = cy * (luma - yo) + term + 32768
            inside = (acc >> 16 >= 0) & (acc >> 16 <= 255)
            low = acc & 0xFFFF
            for j, key in ((2 * i, low), (2 * i + 1, 0xFFFF - low)):
                key = np.where(inside, key, 1 << 20)
                idx = np.argpartition(key, per_channel)[:per_channel]
                best[j] += [(int(key[t]), (luma, int(uv[t, 0]), int(uv[t, 1]))) for t in idx]
                best[j] = sorted(best[j])[:per_channel]
    return np.array([t for group in best for _, t in group], np.uint8)


# ---- Y4M ------------------------------------------------------------------------------------------------------------------
def build_y4m(frames, w: int, h: int, tag="C420jpeg", rate="25:1", interlace="p", full=None, frame_params="", extra="") -> bytes:
    """A file of `frames` (bytes each).  tag, interlace: None leaves the field out; full: True / False writes
    XCOLORRANGE; frame_params: text behind FRAME on every frame's line."""
    fields = ["YUV4MPEG2", f"W{w}", f"H{h}", f"F{rate}"]
    if interlace is not None:
        fields.append(f"I{interlace}")
    fields.append("A1:1")
    if tag is not None:
        fields.append(tag)
    if full is not None:
        fields.append("XCOLORRANGE=" + ("FULL" if full else "LIMITED"))
    if extra:
        fields.append(extra)
    out = [(" ".join(fields) + "\n").encode("ascii")]
    for frame in frames:
        out += [("FRAME" + (" " + frame_params if frame_params else "") + "\n").encode("ascii"), bytes(frame)]
    return b"".join(out)


def parse_y4m(data: bytes) -> dict:
    """{width, height, framerate (Fraction), layout, range, siting, header_bytes, offsets, trailing_bytes}; `Rejected`
    with one of REJECT otherwise."""
    data = bytes(data)
    if not (data.startswith(b"YUV4MPEG2 ") or data.startswith(b"YUV4MPEG2\n")):
        raise Rejected("not_y4m")
    line_end = data[:256].find(b"\n")
    if line_end == -1:
        raise Rejected("bad_header")
    seen = {}
    for token in data[9:line_end].decode("latin-1").split():
        seen.setdefault(token[0], []).append(token[1:])
    try:
        width, height = int(seen["W"][-1]), int(seen["H"][-1])
        num, den = seen["F"][-1].split(":")
        if not (seen["W"][-1].isdigit() and seen["H"][-1].isdigit() and num.isdigit() and den.isdigit()):
            raise ValueError
        rate = Fraction(int(num), int(den))
        if width < 1 or height < 1 or rate == 0:
            raise ValueError
    except (KeyError, ValueError, ZeroDivisionError):
        raise Rejected("bad_header") from None
    if "I" in seen and seen["I"][-1] not in ("p", "?"):
        raise Rejected("interlaced")
    tag = "C" + seen["C"][-1] if "C" in seen else None
    if tag is not None and tag not in TAGS:
        raise Rejected("chroma")
    layout = TAGS[tag] if tag else "yuv420p"
    rng = "pc" if "COLORRANGE=FULL" in seen.get("X", []) else "tv"
    size = frame_bytes(width, height, layout)
    at, offsets = line_end + 1, []
    while len(data) - at >= 6 + size:
        head = data[at:at + 80]
        if not (head.startswith(b"FRAME\n") or head.startswith(b"FRAME ")) or b"\n" not in head:
            raise Rejected("bad_frame_header")
        start = at + head.index(b"\n") + 1
        if len(data) - start < size:
            break
        offsets.append(start)
        at = start + size
    return dict(width=width, height=height, framerate=rate, layout=layout, range=rng, siting=tag, header_bytes=line_end + 1,
                offsets=offsets, trailing_bytes=len(data) - at)
