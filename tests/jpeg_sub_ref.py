"""numpy restatement of libjpeg's baseline encoder for the three chroma layouts transflow_amd/csrc/jpeg.hip writes:
4:4:4, 4:2:2 and 4:2:0 -- Pillow's `save(quality=q, subsampling=s, restart_marker_blocks=r)` with s = 0, 1, 2, and the
same with `optimize=True` (the frame's own Huffman tables), byte for byte (tests/test_jpeg_sub_ref.py holds it to that).

Everything that does not depend on the layout is tests/jpeg_ref.py's and tests/jpeg_optimize_ref.py's, imported and left
alone: colour conversion, the DCT, quantisation, the coder of a block, the bit writer, the table builder.  What the layout
changes is stated here:

  jcmarker.c  write_frame_header   the luma sampling byte of SOF0: 0x11, 0x21, 0x22; chroma stays 0x11
  jcmaster.c  per_scan_setup       the MCU: 8 x 8 pixels, blocks Y Cb Cr; 16 x 8, blocks Y0 Y1 Cb Cr; 16 x 16, Y00 Y01 Y10
                                   Y11 Cb Cr.  The restart interval counts MCUs of the layout's own size
  jccoefct.c  compress_data        the luma grid is ceil(W / 8) x ceil(H / 8), last column and row replicated; a luma block
                                   of an MCU beyond it is a dummy (AC zero, DC of the block before it in the MCU): none at
                                   4:4:4, at 4:2:2 only the second block of the last MCU column when ceil(W / 8) is odd
  jcsample.c  h2v1_downsample      the converted plane replicated right to mcus_x * 16 columns, then
                                   out[x] = (p[2x] + p[2x + 1] + (x & 1)) >> 1 -- the bias 0, 1, 0, 1 along the output row;
                                   rows below the image repeat the last row
  jcsample.c  fullsize_downsample  4:4:4: the converted samples, replicated right and down to whole blocks
  jcsample.c  h2v2_downsample      4:2:0: jpeg_ref.downsample and jpeg_ref.encode's row rule

`encode(..., trace=Trace())` fills a jpeg_ref.Trace: symbols, lane widths, per-MCU bits, the bytes each MCU flushes.
"""
from __future__ import annotations

import numpy as np

from tests import jpeg_optimize_ref, jpeg_ref
from tests.jpeg_ref import Trace  # noqa: F401  (what `encode` fills)

# Pillow's numbering -> (name, luma sampling h, v, the SOF0 byte)
SAMPLINGS = {0: ("4:4:4", 1, 1, 0x11), 1: ("4:2:2", 2, 1, 0x21), 2: ("4:2:0", 2, 2, 0x22)}


def mcu_size(subsampling: int):
    """(height, width) of an MCU in pixels."""
    _, h, v, _ = SAMPLINGS[subsampling]
    return 8 * v, 8 * h


def blocks_per_mcu(subsampling: int) -> int:
    _, h, v, _ = SAMPLINGS[subsampling]
    return h * v + 2


def downsample_h2v1(plane: np.ndarray) -> np.ndarray:
    """h2v1_downsample on a plane of even width."""
    bias = np.arange(plane.shape[1] // 2) & 1
    return (plane[:, 0::2] + plane[:, 1::2] + bias) >> 1


def _patch_sof(head: bytes, subsampling: int) -> bytes:
    """`head` (a header of jpeg_ref's, 4:2:0) with the luma sampling byte of its SOF0 segment set."""
    i = 2
    while head[i + 1] != 0xC0:
        i += 2 + int.from_bytes(head[i + 2:i + 4], "big")
    at = i + 4 + 1 + 2 + 2 + 1 + 1                                        # precision, height, width, count, id
    assert head[at] == 0x22
    return head[:at] + bytes([SAMPLINGS[subsampling][3]]) + head[at + 1:]


def header(height: int, width: int, quality: int, restart_mcus: int, subsampling: int) -> bytes:
    return _patch_sof(jpeg_ref.header(height, width, quality, restart_mcus), subsampling)


def _blocks(rgb: np.ndarray, quality: int, subsampling: int):
    """(mcus_x, mcus_y, a function (my, mx) -> the MCU's (table, component, block) in coding order)."""
    _, h, v, _ = SAMPLINGS[subsampling]
    H, W = rgb.shape[:2]
    mcus_x, mcus_y = -(-W // (8 * h)), -(-H // (8 * v))
    lum_bx, lum_by = (W + 7) // 8, (H + 7) // 8
    y, cb, cr = jpeg_ref.ycc(rgb)
    y = jpeg_ref.pad_bottom(jpeg_ref.pad_right(y, lum_bx * 8), lum_by * 8)
    chroma = []
    for plane in (cb, cr):
        plane = jpeg_ref.pad_right(plane, mcus_x * 8 * h)
        if subsampling == 2:                                              # rows only to an even count, then the downsampled rows
            plane = jpeg_ref.downsample(jpeg_ref.pad_bottom(plane, H + (H & 1)))
        elif subsampling == 1:
            plane = downsample_h2v1(plane)
        chroma.append(jpeg_ref.pad_bottom(plane, mcus_y * 8))
    tl = jpeg_ref.quant_table(jpeg_ref.QUANT_LUMA, quality)
    tc = jpeg_ref.quant_table(jpeg_ref.QUANT_CHROMA, quality)
    cy = jpeg_ref.blocks_quantised(y, tl)
    ccb, ccr = jpeg_ref.blocks_quantised(chroma[0], tc), jpeg_ref.blocks_quantised(chroma[1], tc)

    def mcu(my, mx):
        out, prev = [], None
        for b in range(h * v):
            by, bx = v * my + b // h, h * mx + b % h
            if by < lum_by and bx < lum_bx:
                block = cy[by, bx]
            else:                                                         # jccoefct.c: a dummy block
                block = np.zeros(64, np.int64)
                block[0] = prev[0]
            out.append((0, 0, block))
            prev = block
        out.append((1, 1, ccb[my, mx]))
        out.append((1, 2, ccr[my, mx]))
        return out
    return mcus_x, mcus_y, mcu


def histograms(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1, subsampling: int = 2) -> np.ndarray:
    """uint32 [4][257]: what the gather pass counts (entry 256, the reserved symbol, is 1)."""
    rgb = np.asarray(rgb)
    mcus_x, mcus_y, mcu = _blocks(rgb, quality, subsampling)
    hist = np.zeros((4, 257), np.int64)
    hist[:, 256] = 1
    last, n_mcu = [0, 0, 0], 0
    for my in range(mcus_y):
        for mx in range(mcus_x):
            if n_mcu and n_mcu % restart_mcus == 0:
                last = [0, 0, 0]
            n_mcu += 1
            for table, comp, block in mcu(my, mx):
                jpeg_optimize_ref._count_block(hist[2 * table], hist[2 * table + 1], block, last[comp])
                last[comp] = int(block[0])
    return hist.astype(np.uint32)


def tables(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1, subsampling: int = 2):
    """The four (bits, vals) of the frame, in the DHT segments' order."""
    return [jpeg_optimize_ref.gen_optimal_table(h) for h in histograms(rgb, quality, restart_mcus, subsampling)]


def encode(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1, subsampling: int = 2, optimize: bool = False,
           trace: Trace | None = None) -> bytes:
    """The whole file for a uint8 (H, W, 3) RGB image.  A `trace` is filled with what was coded on the way."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and restart_mcus >= 1
    H, W = rgb.shape[:2]
    if optimize:
        four = tables(rgb, quality, restart_mcus, subsampling)
        head = _patch_sof(jpeg_optimize_ref.header_of(H, W, quality, restart_mcus, four), subsampling)
        dc_l, ac_l, dc_c, ac_c = (jpeg_optimize_ref._Codes(jpeg_ref.huff_codes(*t)) for t in four)
    else:
        head = header(H, W, quality, restart_mcus, subsampling)
        dc_l, ac_l, dc_c, ac_c = (jpeg_ref.huff_codes(*t) for t in (jpeg_ref.DC_LUMA, jpeg_ref.AC_LUMA,
                                                                     jpeg_ref.DC_CHROMA, jpeg_ref.AC_CHROMA))
    mcus_x, mcus_y, mcu = _blocks(rgb, quality, subsampling)
    out = bytearray(head)
    bits, last, n_mcu = jpeg_ref._Bits(), [0, 0, 0], 0
    for my in range(mcus_y):
        for mx in range(mcus_x):
            if n_mcu and n_mcu % restart_mcus == 0:                       # emit_restart (flush_bits ran behind the MCU)
                out += bits.out + bytes([0xFF, 0xD0 + (n_mcu // restart_mcus - 1) % 8])
                bits, last = jpeg_ref._Bits(), [0, 0, 0]
            n_mcu += 1
            bits_before, raw_before = bits.total, len(bits.raw)
            for table, comp, block in mcu(my, mx):
                jpeg_ref._encode_block(bits, block, last[comp], (dc_l, dc_c)[table], (ac_l, ac_c)[table], trace, table)
                last[comp] = int(block[0])
            mcu_bits = bits.total - bits_before
            interval_end = n_mcu % restart_mcus == 0 or n_mcu == mcus_x * mcus_y
            if interval_end:
                bits.flush()
            if trace is not None:
                trace.mcu_bits.append(mcu_bits)
                trace.flushed.append(bytes(bits.raw[raw_before:]))
                trace.interval_end.append(interval_end)
    out += bits.out + b"\xff\xd9"
    if trace is not None:
        trace.data = bytes(out)
    return bytes(out)


def trace(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1, subsampling: int = 2, optimize: bool = False) -> Trace:
    """`encode`, the same code, returning what it coded."""
    t = Trace()
    encode(rgb, quality, restart_mcus, subsampling, optimize, t)
    return t


# ---- the images and the cases -------------------------------------------------------------------------------------------
def smooth_image(height: int, width: int) -> np.ndarray:
    return jpeg_ref.formula_image(height, width)


def noise_image(height: int, width: int, seed: int = 11) -> np.ndarray:
    """Uniform noise from jpeg_ref's integer hash: no library's generator."""
    return ((jpeg_ref._hash(seed, 1, height * width * 3) >> np.uint64(40)) & np.uint64(255)).astype(np.uint8).reshape(height, width, 3)


def made_image(kind: str, height: int, width: int, seed: int = 0) -> np.ndarray:
    if kind == "smooth":
        return smooth_image(height, width)
    if kind == "noise":
        return noise_image(height, width, seed)
    if kind == "binary":
        return jpeg_ref.binary_noise(height, width, seed)
    raise ValueError(kind)


# the grid the restatement is held to Pillow on (tests/test_jpeg_sub_ref.py)
GRID_SIZES = ((1, 1), (8, 8), (7, 9), (9, 17), (16, 16), (17, 33), (23, 41), (8, 15), (8, 16), (8, 17), (40, 72))
GRID_QUALITIES = (10, 50, 90, 100)
GRID_INTERVALS = (1, 3, 8)

# name -> (height, width, kind, seed, quality, restart_mcus, optimize): the device cases, each captured at subsampling 0 and
# 1 (tools/capture_golden_jpeg_sub.py -> tests/golden/jpegsub_<name>_s<subsampling>.npz).  Sizes are (height, width).
CASES = {
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


def case_image(name: str) -> np.ndarray:
    h, w, kind, seed = CASES[name][:4]
    return made_image(kind, h, w, seed)


def fixture_name(name: str, subsampling: int) -> str:
    return f"jpegsub_{name}_s{subsampling}.npz"


def load_case(path: str):
    """(image, quality, restart_mcus, subsampling, optimize, expected file bytes) of a tests/golden/jpegsub_*.npz fixture:
    the fixture stores the image's recipe, not its pixels."""
    with np.load(path) as z:
        image = made_image(str(z["content"]), int(z["height"]), int(z["width"]), int(z["seed"]))
        return (image, int(z["quality"]), int(z["restart_mcus"]), int(z["subsampling"]), bool(z["optimize"]),
                z["jpeg"].tobytes())
