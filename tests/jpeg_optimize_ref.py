"""numpy restatement of libjpeg's `optimize_coding` as transflow_amd/csrc/jpeg.hip runs it in mode 1: the baseline file of
tests/jpeg_ref.py with the frame's own Huffman tables in its four DHT segments -- Pillow's
`save(quality=q, subsampling=2, restart_marker_blocks=r, optimize=True)`, byte for byte (tests/test_jpeg_optimize_ref.py
holds it to that).

  jchuff.c  encode_mcu_gather, htest_one_block   the symbols `encode_one_block` emits, counted; DC prediction restarts
                                                 at every interval, dummy blocks count like any other
  jchuff.c  jpeg_gen_optimal_table               `gen_optimal_table`
  jchuff.c  jpeg_make_c_derived_tbl              jpeg_ref.huff_codes

Everything before the entropy coder is jpeg_ref's (`ycc`, `pad_*`, `downsample`, `blocks_quantised`), and so are the
coder of a block and the bit writer.  The four tables are in the order of the file's DHT segments: DC luma, AC luma,
DC chroma, AC chroma.
"""
from __future__ import annotations

import numpy as np

from tests import jpeg_ref

TABLE_NAMES = ("DC luma", "AC luma", "DC chroma", "AC chroma")
MAX_CLEN = 32                                # jchuff.c: the longest code length the limiting step can repair
SENTINEL = 1000000000                        # jchuff.c: a frequency above it is never selected


class CodeLengthOverflow(ValueError):
    """libjpeg's JERR_HUFF_CLEN_OVERFLOW: a code size above 32."""


def gen_optimal_table(counts):
    """jpeg_gen_optimal_table: 256 (or 257: the last is ignored) frequencies -> (bits[16], vals).  ValueError for a
    histogram without a symbol (libjpeg would run off its array), CodeLengthOverflow for a code size above 32."""
    freq = [int(v) for v in counts][:256]
    assert len(freq) == 256 and min(freq) >= 0
    if not any(freq):
        raise ValueError("a histogram without a symbol")
    freq.append(1)                                                        # the reserved symbol: no real code is all ones
    codesize, others = [0] * 257, [-1] * 257

    def pick(skip):
        c, v = -1, SENTINEL
        for i in range(257):                                              # upward with <=: among equals the largest index
            if freq[i] and freq[i] <= v and i != skip:
                c, v = i, freq[i]
        return c

    while True:
        c1 = pick(-1)
        c2 = pick(c1)
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    if max(codesize) > MAX_CLEN:
        raise CodeLengthOverflow(f"a code size of {max(codesize)}, above {MAX_CLEN}")
    bits = [0] * (MAX_CLEN + 1)
    for size in codesize:
        if size:
            bits[size] += 1
    for i in range(MAX_CLEN, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                                          # the reserved symbol leaves
    vals = [s for size in range(1, MAX_CLEN + 1) for s in range(256) if codesize[s] == size]
    return bits[1:17], vals


def code_sizes_before_limiting(counts) -> int:
    """The longest code size `gen_optimal_table` sees before its limiting step (33 and more: it refuses)."""
    freq = [int(v) for v in counts][:256] + [1]
    depth = {i: 0 for i in range(257) if freq[i]}
    groups = {i: [i] for i in depth}
    live = {i: freq[i] for i in depth}
    while len(live) > 1:
        c1 = min(live, key=lambda i: (live[i], -i))
        v1 = live.pop(c1)
        c2 = min(live, key=lambda i: (live[i], -i))
        v2 = live.pop(c2)
        live[c1] = v1 + v2
        groups[c1] += groups.pop(c2)
        for s in groups[c1]:
            depth[s] += 1
    return max(depth.values())


def _blocks(rgb: np.ndarray, quality: int):
    """(mcus_x, mcus_y, a function (my, mx) -> the MCU's six (table, component, block)) as jpeg_ref.encode has them."""
    H, W = rgb.shape[:2]
    mcus_x, mcus_y = (W + 15) // 16, (H + 15) // 16
    lum_bx, lum_by = (W + 7) // 8, (H + 7) // 8
    y, cb, cr = jpeg_ref.ycc(rgb)
    y = jpeg_ref.pad_bottom(jpeg_ref.pad_right(y, lum_bx * 8), lum_by * 8)
    chroma = []
    for plane in (cb, cr):
        plane = jpeg_ref.pad_bottom(jpeg_ref.pad_right(plane, mcus_x * 16), H + (H & 1))
        chroma.append(jpeg_ref.pad_bottom(jpeg_ref.downsample(plane), mcus_y * 8))
    tl = jpeg_ref.quant_table(jpeg_ref.QUANT_LUMA, quality)
    tc = jpeg_ref.quant_table(jpeg_ref.QUANT_CHROMA, quality)
    cy = jpeg_ref.blocks_quantised(y, tl)
    ccb, ccr = jpeg_ref.blocks_quantised(chroma[0], tc), jpeg_ref.blocks_quantised(chroma[1], tc)

    def mcu(my, mx):
        out, prev = [], None
        for b in range(4):
            by, bx = 2 * my + (b >> 1), 2 * mx + (b & 1)
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


def _count_block(dc_hist, ac_hist, block, last_dc: int) -> None:
    """htest_one_block."""
    dc_hist[int(abs(int(block[0]) - last_dc)).bit_length()] += 1
    prev = 0
    for k in np.flatnonzero(block[1:]) + 1:
        k = int(k)
        run = k - prev - 1
        ac_hist[0xF0] += run >> 4
        ac_hist[((run & 15) << 4) | int(abs(int(block[k]))).bit_length()] += 1
        prev = k
    if prev != 63:
        ac_hist[0x00] += 1


def histograms(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1) -> np.ndarray:
    """uint32 [4][257]: what the gather pass counts (entry 256, the reserved symbol, is 1)."""
    rgb = np.asarray(rgb)
    mcus_x, mcus_y, mcu = _blocks(rgb, quality)
    hist = np.zeros((4, 257), np.int64)
    hist[:, 256] = 1
    last, n_mcu = [0, 0, 0], 0
    for my in range(mcus_y):
        for mx in range(mcus_x):
            if n_mcu and n_mcu % restart_mcus == 0:
                last = [0, 0, 0]
            n_mcu += 1
            for table, comp, block in mcu(my, mx):
                _count_block(hist[2 * table], hist[2 * table + 1], block, last[comp])
                last[comp] = int(block[0])
    return hist.astype(np.uint32)


def tables(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1):
    """The four (bits, vals) of the frame."""
    return [gen_optimal_table(h) for h in histograms(rgb, quality, restart_mcus)]


def header_of(height: int, width: int, quality: int, restart_mcus: int, four_tables) -> bytes:
    """jpeg_ref.header with these four tables in its DHT segments: the order of the segments is unchanged."""
    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)
    fixed = jpeg_ref.header(height, width, quality, restart_mcus)
    annex_k = sum(2 + 2 + 1 + 16 + len(vals) for _, vals in (jpeg_ref.DC_LUMA, jpeg_ref.AC_LUMA, jpeg_ref.DC_CHROMA,
                                                              jpeg_ref.AC_CHROMA))
    tail = 6 + 14                                                         # DRI and SOS
    first = len(fixed) - tail - annex_k
    assert fixed[first:first + 2] == b"\xff\xc4" and fixed[-tail:-tail + 2] == b"\xff\xdd"
    dht = b"".join(seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
                   for tc_th, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), four_tables))
    return fixed[:first] + dht + fixed[-tail:]


def header(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1) -> bytes:
    rgb = np.asarray(rgb)
    return header_of(rgb.shape[0], rgb.shape[1], quality, restart_mcus, tables(rgb, quality, restart_mcus))


class _Codes(dict):
    """symbol -> (code, length).  jpeg_ref's trace asks for ZRL's length in front of every coefficient, also where the
    frame has no ZRL and so no code for it: no bits then."""

    def __missing__(self, symbol):
        if symbol != 0xF0:
            raise KeyError(symbol)
        return (0, 0)


def encode(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1, trace: jpeg_ref.Trace | None = None) -> bytes:
    """The whole optimised file for a uint8 (H, W, 3) RGB image."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and restart_mcus >= 1
    four = tables(rgb, quality, restart_mcus)
    dc_l, ac_l, dc_c, ac_c = (_Codes(jpeg_ref.huff_codes(*t)) for t in four)
    mcus_x, mcus_y, mcu = _blocks(rgb, quality)
    out = bytearray(header_of(rgb.shape[0], rgb.shape[1], quality, restart_mcus, four))
    bits, last, n_mcu = jpeg_ref._Bits(), [0, 0, 0], 0
    for my in range(mcus_y):
        for mx in range(mcus_x):
            if n_mcu and n_mcu % restart_mcus == 0:
                out += bits.out + bytes([0xFF, 0xD0 + (n_mcu // restart_mcus - 1) % 8])
                bits, last = jpeg_ref._Bits(), [0, 0, 0]
            n_mcu += 1
            before = bits.total
            for table, comp, block in mcu(my, mx):
                jpeg_ref._encode_block(bits, block, last[comp], (dc_l, dc_c)[table], (ac_l, ac_c)[table], trace, table)
                last[comp] = int(block[0])
            if trace is not None:
                trace.mcu_bits.append(bits.total - before)
            if n_mcu % restart_mcus == 0 or n_mcu == mcus_x * mcus_y:
                bits.flush()
    out += bits.out + b"\xff\xd9"
    if trace is not None:
        trace.data = bytes(out)
    return bytes(out)


def trace(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1) -> jpeg_ref.Trace:
    t = jpeg_ref.Trace()
    encode(rgb, quality, restart_mcus, t)
    return t


def dht_tables(data: bytes):
    """{tc_th: (bits, vals)} of a file's DHT segments."""
    out, i = {}, 2
    while data[i + 1] != 0xDA:
        n = int.from_bytes(data[i + 2:i + 4], "big")
        if data[i + 1] == 0xC4:
            p = data[i + 4:i + 2 + n]
            out[p[0]] = (list(p[1:17]), list(p[17:]))
        i += 2 + n
    return out


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


# ---- the cases ---------------------------------------------------------------------------------------------------------
WIDE_LANE_SEED = 2                           # (with it: ZRL's code has 16 bits, the widest lane 70, luma AC 17 before limiting)


def wide_lane_image(height: int, width: int, seed: int) -> np.ndarray:
    """Grey noise (jpeg_ref's integer hash, no library's generator) whose luma block (0, 0) is the DCT's highest basis
    function at full swing: at quality 95 it quantises to the single coefficient at zigzag 63, behind three ZRLs -- the
    only ZRLs of the image, so ZRL gets one of the longest codes of the luma AC table."""
    grey = ((jpeg_ref._hash(seed, 0, height * width) >> np.uint64(40)) & np.uint64(255)).astype(np.int64).reshape(height, width)
    x = np.arange(8)
    c = np.cos((2 * x + 1) * 7 * np.pi / 16)
    grey[:8, :8] = np.rint(128 + 127 * np.outer(c, c)).astype(np.int64)
    return np.repeat(grey.astype(np.uint8)[..., None], 3, axis=-1)


# name -> (height, width, content, quality, restart_mcus), as jpeg_ref.CASES
CASES = {name: case for name, case in jpeg_ref.CASES.items() if case[0] <= 96 and case[1] <= 96}
CASES["270x480_q95"] = jpeg_ref.CASES["270x480_q95"]                   # luma AC: 17 bits before limiting, 16 after
CASES["224x224_wide_lane"] = (224, 224, ("wide_lane", WIDE_LANE_SEED), 95, 4)   # a lane of more than 64 bits


def made_image(kind: str, height: int, width: int, seed) -> np.ndarray:
    if kind == "wide_lane":
        return wide_lane_image(height, width, int(seed))
    return jpeg_ref._made_image(kind, height, width, seed)


def case_image(name: str) -> np.ndarray:
    h, w, content, _, _ = CASES[name]
    if isinstance(content, tuple) and content[0] == "wide_lane":
        return wide_lane_image(h, w, content[1])
    return jpeg_ref.case_image(name)


def load_case(path: str):
    """(image, quality, restart_mcus, expected file bytes) of a tests/golden/jpegopt_*.npz fixture."""
    with np.load(path) as z:
        quality, restart = int(z["quality"]), int(z["restart_mcus"])
        if "image" in z.files:
            image = z["image"]
        else:
            image = made_image(str(z["content"]), int(z["height"]), int(z["width"]), z["seed"] if "seed" in z.files else None)
        return image, quality, restart, z["jpeg"].tobytes()
