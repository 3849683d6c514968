"""The JPEG decoder's test files, made with Pillow (>= 10.2 for `restart_marker_blocks`): the valid cases whose pixels the
restatement and the device must reproduce, and the malformed ones they must reject with the same reason.  Used by
tests/test_jpegdec_ref.py at test time and by tools/capture_golden_jpegdec.py for tests/golden/jpegdec_*.npz.
"""
from __future__ import annotations

import io

import numpy as np

from . import jpegdec_ref as JR


def image(height: int, width: int, seed: int, kind: str = "scene", grey: bool = False) -> np.ndarray:
    rng = np.random.default_rng(seed)
    shape = (height, width) if grey else (height, width, 3)
    if kind == "noise":
        out = rng.integers(0, 256, shape, dtype=np.uint8)
        # one block of a one-level checkerboard: at quality 100 its only AC coefficient is the last, behind three ZRLs
        yy, xx = np.mgrid[0:8, 0:8]
        board = (127 + ((yy + xx) & 1))[:max(min(height, 16) - 8, 0), :max(min(width, 24) - 16, 0)]    # (what a small image has of it)
        out[8:16, 16:24] = board[..., None] if out.ndim == 3 else board
        return out
    if kind == "flat":
        return np.full(shape, 128, np.uint8)
    yy, xx = np.mgrid[0:height, 0:width]
    if kind == "smooth":                               # grey only: compresses to a few bytes a block
        base = 128 + 60 * np.sin(xx / 23.0) * np.cos(yy / 31.0) + rng.normal(0, 2.5, (height, width))
        return np.clip(base, 0, 255).astype(np.uint8)
    chans = [128 + 100 * np.sin(xx / (3.0 + c) + c) * np.cos(yy / (4.0 + c)) + rng.normal(0, 12, (height, width)) for c in range(3)]
    out = np.clip(np.stack(chans, axis=-1), 0, 255).astype(np.uint8)
    return out[:, :, 0].copy() if grey else out


def encode(array: np.ndarray, quality: int = 90, subsampling: int | None = 2, restart: int = 0, **kw) -> bytes:
    import PIL.Image
    buf = io.BytesIO()
    opts = dict(format="JPEG", quality=quality, **kw)
    if array.ndim == 3:
        opts["subsampling"] = subsampling
    if restart:
        opts["restart_marker_blocks"] = restart
    PIL.Image.fromarray(array).save(buf, **opts)
    return buf.getvalue()


def pillow_pixels(data: bytes) -> np.ndarray:
    import PIL.Image
    return np.array(PIL.Image.open(io.BytesIO(data)).convert("RGB"))


def valid_cases() -> list:
    """[(name, file bytes)]"""
    out = []
    for (w, h) in [(16, 16), (8, 8), (17, 9), (37, 19), (33, 31), (48, 32)]:
        out.append((f"geo_420_{w}x{h}", encode(image(h, w, 10 + w), restart=2)))
    out.append(("geo_422_37x19", encode(image(19, 37, 21), subsampling=1, restart=2)))
    out.append(("geo_444_37x19", encode(image(19, 37, 22), subsampling=0, restart=2)))
    out.append(("geo_grey_37x19", encode(image(19, 37, 23, grey=True), restart=2)))
    for r in (1, 2, 5, 6):
        out.append((f"iv_37x19_r{r}", encode(image(19, 37, 30), restart=r)))
    out.append(("iv_37x19_nodri", encode(image(19, 37, 30))))
    out.append(("iv_160x16_r1", encode(image(16, 160, 31), restart=1)))
    out.append(("iv_512_grey_r1", encode(image(512, 512, 32, "smooth", grey=True), quality=90, restart=1)))
    out.append(("sym_noise_q100", encode(image(48, 64, 40, "noise"), quality=100, restart=2)))
    out.append(("sym_noise_q1", encode(image(48, 64, 41, "noise"), quality=1, restart=2)))
    out.append(("sym_flat", encode(image(32, 48, 0, "flat"), restart=1)))
    out.append(("sym_optimize", encode(image(31, 33, 42), restart=2, optimize=True)))
    out.append(("sym_handmade", _handmade("0" + "00", *HANDMADE_AC)))       # DC 0, EOB: tables of one and four codes
    return out


# ---- the pixel stages' geometry: IDCT to planes, upsampling, colour, the four-pixel store ------------------------------------
GEOMETRY_LAYOUTS = {"grey": None, "444": 0, "422": 1, "420": 2}                    # Pillow's `subsampling`
# widths 1..4: libjpeg replicates the chroma (downsampled_width <= 2); 5: the first fancy one; 7 / 8 / 9 and 16 / 17 / 33:
# either side of the 8- and 16-pixel MCU edges.  Heights 1..3: one or two chroma rows, the context row the same row again.
GEOMETRY_NODRI = ((1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33), (1, 2, 3, 8, 9, 16, 17))     # (widths, heights): the parallel scan
GEOMETRY_DRI1 = ((1, 2, 4, 5, 9, 17, 33), (1, 3, 9, 17))                            # restart interval 1: the serial path
GEOMETRY_MORE = ((4, 4), (3, 5))                                                    # (width, height) without DRI, outside the grid


def geometry_name(layout: str, width: int, height: int, dri: bool) -> str:
    return f"px_{layout}_{width}x{height}" + ("_r1" if dri else "")


def geometry_sizes(dri: bool) -> list:
    """[(width, height)] of one layout's cases."""
    widths, heights = GEOMETRY_DRI1 if dri else GEOMETRY_NODRI
    return [(w, h) for w in widths for h in heights] + ([] if dri else list(GEOMETRY_MORE))


def geometry_cases() -> list:
    """[(name, file bytes)]: noise at quality 95, so that neighbouring chroma samples differ and a wrong upsampling rule,
    context row or plane stride changes pixels."""
    out = []
    for dri in (False, True):
        for n, layout in enumerate(GEOMETRY_LAYOUTS):
            for w, h in geometry_sizes(dri):
                pixels = image(h, w, 7000 + 1000 * n + 40 * h + w, "noise", grey=layout == "grey")
                out.append((geometry_name(layout, w, h, dri),
                            encode(pixels, quality=95, subsampling=GEOMETRY_LAYOUTS[layout], restart=int(dri))))
    return out


# hand-built AC table: codes 00 (EOB), 01 (run 15 size 1: 0xF1), 100 (ZRL), 101 (run 0 size 10: 0x0A); 11x is no code
HANDMADE_AC = ([0, 2, 2] + [0] * 13, [0x00, 0xF1, 0xF0, 0x0A])


# ---- malformed files -------------------------------------------------------------------------------------------------
def _scan_offset(data: bytes) -> int:
    return JR.parse_header(data)["scan_offset"]


def _patch(data: bytes, at: int, value: int) -> bytes:
    b = bytearray(data)
    b[at] = value
    return bytes(b)


def _markers(data: bytes) -> list:
    so = _scan_offset(data)
    return [so + i for i in range(len(data) - so - 1) if data[so + i] == 0xFF and 0xD0 <= data[so + i + 1] <= 0xD7]


def _handmade(scan_bits: str, ac_counts=None, ac_vals=None, dc_vals=(0,), quant: int = 1) -> bytes:
    """An 8 x 8 grey file with hand-built tables: DC code '0' = category dc_vals[0] (a second, '10', if given); the AC
    table as given.  scan_bits: the scan as a string of 0 / 1, padded with ones."""
    ac_counts = ac_counts or [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]        # one code of 2 bits: 00
    ac_vals = ac_vals or [0x00]
    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)
    bits = scan_bits + "1" * (-len(scan_bits) % 8)
    scan = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00")
    return (b"\xff\xd8" + seg(0xDB, [0] + [quant] * 64) + seg(0xC0, [8, 0, 8, 0, 8, 1, 1, 0x11, 0])
            + seg(0xC4, [0x00] + [1, len(dc_vals) - 1] + [0] * 14 + list(dc_vals)) + seg(0xC4, [0x10] + ac_counts + ac_vals)
            + seg(0xDA, [1, 1, 0x00, 0, 63, 0]) + scan + b"\xff\xd9")


def malformed_cases() -> list:
    """[(name, file bytes)]: every one of them is rejected; the reason is the restatement's."""
    out = []
    small = encode(image(9, 17, 50), restart=1)
    for cut in range(0, len(small), 10):
        out.append((f"cut_{cut:04d}", small[:cut]))
    base = encode(image(19, 37, 51), restart=1)          # 6 intervals, 5 markers
    mk = _markers(base)
    out.append(("rst_removed", base[:mk[2]] + base[mk[2] + 2:]))
    swapped = bytearray(base)
    swapped[mk[1] + 1], swapped[mk[2] + 1] = swapped[mk[2] + 1], swapped[mk[1] + 1]
    out.append(("rst_swapped", bytes(swapped)))
    out.append(("rst_duplicated", base[:mk[3]] + base[mk[3]:mk[3] + 2] + base[mk[3]:]))
    out.append(("rst_without_dri", (lambda d, s: d[:s[0]] + d[s[0] + 2 + s[1]:])(base, JR.find_segment(base, 0xDD))))
    out.append(("interval_emptied", base[:mk[1] + 2] + base[mk[2]:]))
    counts, vals = HANDMADE_AC
    out.append(("bad_code", _handmade("0" + "110" + "1" * 24, counts, vals)))
    out.append(("run_past_63", _handmade("0" + ("01" + "1") * 4 + "00", counts, vals)))      # 4 x (run 15, one coefficient)
    out.append(("zrl_past_63", _handmade("0" + "100" * 4 + "00", counts, vals)))
    out.append(("progressive", encode(image(16, 16, 52), progressive=True)))
    sof, _ = JR.find_segment(base, 0xC0)
    out.append(("sof_411", _patch(base, sof + 11, 0x41)))
    out.append(("sof_12bit", _patch(base, sof + 4, 12)))
    out.append(("sof_4_components", _patch(base, sof + 9, 4)))
    dqt, _ = JR.find_segment(base, 0xDB)
    out.append(("dqt_16bit", _patch(base, dqt + 4, 0x10)))
    sos, _ = JR.find_segment(base, 0xDA)
    out.append(("sos_ns_1", _patch(base, sos + 4, 1)))
    return out


def hostile_cases() -> list:
    """[(name, file bytes)]: files the rules take whose coefficients are as large as the rules allow -- what they decode
    to is not pinned; the host check runs them for the sanitizers' sake."""
    counts, vals = HANDMADE_AC
    big = "101" + "0" * 10                                   # run 0, size 10, value -1023
    pos = "101" + "1" * 10                                   # +1023
    out = []
    for name, dc_bits, ac in [("neg", "0" + "0" * 11, big), ("pos", "0" + "1" * 11, pos), ("mixed", "0" + "1" * 11, big + pos)]:
        bits = dc_bits + (ac * 63)[:13 * 63] + ""
        out.append((f"hostile_{name}", _handmade(bits, counts, vals, dc_vals=(11,), quant=255)))
    return out


def stream_images(count: int = 6, height: int = 48, width: int = 64) -> list:
    """A textured scene that drifts by a pixel or two a frame: the clip of the integration tests."""
    rng = np.random.default_rng(60)
    big = rng.integers(0, 256, (height // 4 + 8, width // 4 + 8, 3)).astype(np.float64)
    big = np.kron(big, np.ones((4, 4, 1)))
    for _ in range(2):                                   # soften the blocks' edges
        big = (big + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, (1, 1), (0, 1))) / 4
    return [np.clip(big[8 + i:8 + i + height, 6 + 2 * i:6 + 2 * i + width], 0, 255).astype(np.uint8) for i in range(count)]


def stream_frames() -> list:
    """The clip's frames as JPEG files (4:2:0, quality 90, a restart interval of 2 MCUs), and behind them frame 3 again
    without DRI: the same pixels, a file the provider sends the host's way."""
    images = stream_images()
    return [encode(im, restart=2) for im in images] + [encode(images[3])]
