"""numpy restatement of libjpeg's baseline encoder as transflow_amd/csrc/jpeg.hip runs it: 8-bit YCbCr at 4:4:4, 4:2:2 or
4:2:0, one interleaved scan, jpeg_set_quality's tables, a restart interval counted in MCUs, and for Huffman tables either
Annex K's or the frame's own (libjpeg's `optimize_coding`).

Every rule is libjpeg's integer arithmetic, so `encode()` returns the very file Pillow writes for
`save(quality=q, subsampling=s, restart_marker_blocks=r, optimize=o)` (tests/test_jpeg_ref.py, test_jpeg_sub_ref.py and
test_jpeg_optimize_ref.py hold it to that, byte for byte):

  jccolor.c   rgb_ycc_convert           16-bit fixed point
  jcsample.c  h2v2_downsample           4:2:0: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2 ... along the output row
  jcsample.c  h2v1_downsample           4:2:2: out[x] = (p[2x] + p[2x + 1] + (x & 1)) >> 1 -- the bias 0, 1, 0, 1 along the
                                        output row; rows below the image repeat the last row
  jcsample.c  fullsize_downsample       4:4:4: the converted samples, replicated right and down to whole blocks
  jcprepct.c  pre_process_data          the converted plane replicated right to whole MCUs; at 4:2:0 the input rows
                                        replicated to an even count, the DOWNSAMPLED rows replicated below
  jfdctint.c  jpeg_fdct_islow           CONST_BITS 13, PASS1_BITS 2, on samples - 128
  jcdctmgr.c  forward_DCT               divisor 8 Q[k], rounded half away from zero
  jcmaster.c  per_scan_setup            the MCU: 8 x 8 pixels, blocks Y Cb Cr; 16 x 8, blocks Y0 Y1 Cb Cr; 16 x 16, Y00 Y01 Y10
                                        Y11 Cb Cr.  The restart interval counts MCUs of the layout's own size
  jccoefct.c  compress_data             the luma grid is ceil(W / 8) x ceil(H / 8), last column and row replicated; a luma
                                        block of an MCU beyond it is a dummy (AC zero, DC of the block before it in the MCU):
                                        none at 4:4:4, at 4:2:2 only the second block of the last MCU column when ceil(W / 8)
                                        is odd
  jchuff.c    encode_one_block, emit_restart, flush_bits
  jchuff.c    encode_mcu_gather, htest_one_block   the symbols `encode_one_block` emits, counted; DC prediction restarts at
                                        every interval, dummy blocks count like any other
  jchuff.c    jpeg_gen_optimal_table    `gen_optimal_table`
  jchuff.c    jpeg_make_c_derived_tbl   `huff_codes`
  jcmarker.c  the header                write_frame_header: the luma sampling byte of SOF0 is 0x11, 0x21 or 0x22, chroma
                                        stays 0x11; the four DHT segments carry the tables the scan is coded with

Four tables are always in the order of the file's DHT segments: DC luma, AC luma, DC chroma, AC chroma.
`trace()` is `encode()` with an account of what it coded: symbols, lane widths, MCU sizes, the bytes each MCU flushes.
The images, the case tables and the fixtures' loader are tests/jpeg_cases.py's.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

# Annex K.1 (jcparam.c std_luminance_quant_tbl / std_chrominance_quant_tbl), natural order
QUANT_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
QUANT_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)

# jutils.c jpeg_natural_order: zigzag position -> natural (row-major) index
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
    62, 63], np.int64)

# Annex K.3 (jcparam.c std_huff_tables): bits[1..16], then the values
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
    "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
    "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))


ANNEX_K = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)
TABLE_NAMES = ("DC luma", "AC luma", "DC chroma", "AC chroma")


class Layout(NamedTuple):
    """A chroma layout: the luma sampling factors (chroma's are 1, 1) and the byte SOF0 states them in."""
    name: str
    h: int
    v: int
    sof0: int

    @property
    def mcu_size(self):
        """(height, width) of an MCU in pixels."""
        return 8 * self.v, 8 * self.h


# Pillow's `subsampling` numbers
LAYOUTS = {0: Layout("4:4:4", 1, 1, 0x11), 1: Layout("4:2:2", 2, 1, 0x21), 2: Layout("4:2:0", 2, 2, 0x22)}


def quant_table(base: np.ndarray, quality: int) -> np.ndarray:
    """jpeg_set_quality(q, force_baseline=TRUE): jpeg_quality_scaling, then jpeg_add_quant_table's clamp to 1..255."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base * scale + 50) // 100, 1, 255)


def huff_codes(bits, vals) -> dict:
    """jchuff.c jpeg_make_c_derived_tbl: symbol -> (code, length)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def header(height: int, width: int, quality: int, restart_mcus: int, subsampling: int = 2, tables=ANNEX_K) -> bytes:
    """jcmarker.c write_file_header, write_frame_header, write_scan_header, in libjpeg's order."""
    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for n, base in enumerate((QUANT_LUMA, QUANT_CHROMA)):
        out += seg(0xDB, bytes([n]) + bytes(int(v) for v in quant_table(base, quality)[ZIGZAG]))
    out += seg(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big")
               + bytes([3, 1, LAYOUTS[subsampling].sof0, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), tables):
        out += seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, restart_mcus.to_bytes(2, "big"))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def ycc(rgb: np.ndarray):
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def pad_right(plane: np.ndarray, width: int) -> np.ndarray:
    return np.concatenate([plane, np.repeat(plane[:, -1:], width - plane.shape[1], axis=1)], axis=1)


def pad_bottom(plane: np.ndarray, height: int) -> np.ndarray:
    return np.concatenate([plane, np.repeat(plane[-1:], height - plane.shape[0], axis=0)], axis=0)


def downsample(plane: np.ndarray) -> np.ndarray:
    """h2v2_downsample on a plane of even height and width."""
    bias = 1 + (np.arange(plane.shape[1] // 2) & 1)
    return (plane[0::2, 0::2] + plane[0::2, 1::2] + plane[1::2, 0::2] + plane[1::2, 1::2] + bias) >> 2


def downsample_h2v1(plane: np.ndarray) -> np.ndarray:
    """h2v1_downsample on a plane of even width."""
    bias = np.arange(plane.shape[1] // 2) & 1
    return (plane[:, 0::2] + plane[:, 1::2] + bias) >> 1


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first: bool):
    """One pass of jpeg_fdct_islow over the last axis of d (int64 [..., 8])."""
    CONST_BITS, PASS1_BITS = 13, 2
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    tmp0, tmp7, tmp1, tmp6 = d0 + d7, d0 - d7, d1 + d6, d1 - d6
    tmp2, tmp5, tmp3, tmp4 = d2 + d5, d2 - d5, d3 + d4, d3 - d4
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    out = np.empty_like(d)
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    if first:
        out[..., 0] = (tmp10 + tmp11) << PASS1_BITS
        out[..., 4] = (tmp10 - tmp11) << PASS1_BITS
    else:
        out[..., 0] = _descale(tmp10 + tmp11, PASS1_BITS)
        out[..., 4] = _descale(tmp10 - tmp11, PASS1_BITS)
    z1 = (tmp12 + tmp13) * 4433
    out[..., 2] = _descale(z1 + tmp13 * 6270, n)
    out[..., 6] = _descale(z1 + tmp12 * -15137, n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7] = _descale(tmp4 + z1 + z3, n)
    out[..., 5] = _descale(tmp5 + z2 + z4, n)
    out[..., 3] = _descale(tmp6 + z2 + z3, n)
    out[..., 1] = _descale(tmp7 + z1 + z4, n)
    return out


def blocks_quantised(plane: np.ndarray, table: np.ndarray) -> np.ndarray:
    """plane int64 [8 by, 8 bx] -> quantised coefficients [by, bx, 64] in zigzag order."""
    by, bx = plane.shape[0] // 8, plane.shape[1] // 8
    d = (plane - 128).reshape(by, 8, bx, 8).transpose(0, 2, 1, 3)          # [by, bx, row, col]
    d = _fdct_pass(d, True)                                                # rows
    d = _fdct_pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)   # columns
    q8 = (table * 8).reshape(8, 8)
    c = np.sign(d) * ((np.abs(d) + (q8 >> 1)) // q8)
    return c.reshape(by, bx, 64)[..., ZIGZAG]


class _Bits:
    """jchuff.c emit_bits / flush_bits: MSB first, a 0x00 after every 0xFF.  `raw` is the same bytes before stuffing."""

    def __init__(self):
        self.out, self.raw, self.acc, self.n, self.total = bytearray(), bytearray(), 0, 0, 0

    def put(self, code: int, length: int):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        self.total += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            self.raw.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put(0x7F, 7)
        self.acc = self.n = 0


class Trace:
    """What one `encode` coded.  Index 0 is the luma tables', 1 the chroma tables'."""

    def __init__(self):
        self.ac_symbols = (set(), set())        # run << 4 | size, EOB 0x00 and ZRL 0xF0 included
        self.dc_categories = (set(), set())
        self.zrl_sizes = ({}, {})               # ZRLs in front of one coefficient -> the largest size coded behind so many
        self.widest_lane = [0, 0]               # bits of ZRL codes + symbol code + value bits of one AC coefficient
        self.mcu_bits = []                      # per MCU
        self.flushed = []                       # per MCU: the whole bytes of (carried bits + its bits), unstuffed; the
        #                                         interval's last MCU padded with 1 bits to a byte
        self.interval_end = []                  # per MCU: is it the last of its interval
        self.data = b""                         # the file

    def most_zrls(self, table: int):
        """(the most ZRLs in front of one coefficient, the largest size coded behind that many)."""
        n = max(self.zrl_sizes[table], default=0)
        return n, self.zrl_sizes[table].get(n, 0)

    def merge(self, other: "Trace") -> "Trace":
        for t in range(2):
            self.ac_symbols[t].update(other.ac_symbols[t])
            self.dc_categories[t].update(other.dc_categories[t])
            for n, size in other.zrl_sizes[t].items():
                self.zrl_sizes[t][n] = max(self.zrl_sizes[t].get(n, 0), size)
            self.widest_lane[t] = max(self.widest_lane[t], other.widest_lane[t])
        self.mcu_bits += other.mcu_bits
        self.flushed += other.flushed
        self.interval_end += other.interval_end
        return self


def _encode_block(bits: _Bits, block, last_dc: int, dc_tbl, ac_tbl, trace=None, table: int = 0) -> None:
    def value(v):
        nbits = int(abs(v)).bit_length()
        return nbits, (v - 1 if v < 0 else v) & ((1 << nbits) - 1)
    nbits, extra = value(int(block[0]) - last_dc)
    bits.put(*dc_tbl[nbits])
    bits.put(extra, nbits)
    if trace is not None:
        trace.dc_categories[table].add(nbits)
    prev = 0
    for k in np.flatnonzero(block[1:]) + 1:                               # the coefficients between are the run
        k = int(k)
        run, n_zrl = k - prev - 1, 0
        while run > 15:
            bits.put(*ac_tbl[0xF0])
            run -= 16
            n_zrl += 1
        nbits, extra = value(int(block[k]))
        bits.put(*ac_tbl[(run << 4) | nbits])
        bits.put(extra, nbits)
        prev = k
        if trace is not None:
            trace.ac_symbols[table].add((run << 4) | nbits)
            if n_zrl:
                trace.ac_symbols[table].add(0xF0)
            trace.zrl_sizes[table][n_zrl] = max(trace.zrl_sizes[table].get(n_zrl, 0), nbits)
            lane = n_zrl * ac_tbl[0xF0][1] + ac_tbl[(run << 4) | nbits][1] + nbits
            trace.widest_lane[table] = max(trace.widest_lane[table], lane)
    if prev != 63:
        bits.put(*ac_tbl[0x00])
        if trace is not None:
            trace.ac_symbols[table].add(0x00)


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


class _Codes(dict):
    """symbol -> (code, length).  The trace asks for ZRL's length in front of every coefficient, also where the frame has
    no ZRL and so its own table no code for it: no bits then."""

    def __missing__(self, symbol):
        if symbol != 0xF0:
            raise KeyError(symbol)
        return (0, 0)


def mcus(rgb: np.ndarray, quality: int, subsampling: int = 2):
    """Per MCU in scan order: its (table, component, block) in coding order, blocks quantised and in zigzag order."""
    layout = LAYOUTS[subsampling]
    h, v, (mcu_h, mcu_w) = layout.h, layout.v, layout.mcu_size            # an MCU: h x v luma blocks, then Cb, then Cr
    H, W = rgb.shape[:2]
    mcus_x, mcus_y = -(-W // mcu_w), -(-H // mcu_h)
    lum_bx, lum_by = (W + 7) // 8, (H + 7) // 8                            # the luma block grid; beyond it: dummy blocks
    y, cb, cr = ycc(rgb)
    y = pad_bottom(pad_right(y, lum_bx * 8), lum_by * 8)
    chroma = []
    for plane in (cb, cr):
        plane = pad_right(plane, mcus_x * mcu_w)
        if subsampling == 2:                                              # rows only to an even count, then the downsampled rows
            plane = downsample(pad_bottom(plane, H + (H & 1)))
        elif subsampling == 1:
            plane = downsample_h2v1(plane)
        chroma.append(pad_bottom(plane, mcus_y * 8))
    tl, tc = quant_table(QUANT_LUMA, quality), quant_table(QUANT_CHROMA, quality)
    cy, ccb, ccr = blocks_quantised(y, tl), blocks_quantised(chroma[0], tc), blocks_quantised(chroma[1], tc)
    for my in range(mcus_y):
        for mx in range(mcus_x):
            out, prev = [], None
            for b in range(h * v):
                by, bx = v * my + b // h, h * mx + b % h
                if by < lum_by and bx < lum_bx:
                    block = cy[by, bx]
                else:                                                     # jccoefct.c: a dummy block
                    block = np.zeros(64, np.int64)
                    block[0] = prev[0]
                out.append((0, 0, block))
                prev = block
            out.append((1, 1, ccb[my, mx]))
            out.append((1, 2, ccr[my, mx]))
            yield out


def _walk(rgb: np.ndarray, quality: int, restart_mcus: int, subsampling: int):
    """The scan, as the coder and the gather pass both walk it.  Per MCU: (n of the RSTn in front of it or None, its
    (table, block, the DC its own is predicted from), is it the last of its interval).  Prediction restarts at 0 behind
    every marker."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and restart_mcus >= 1
    every = list(mcus(rgb, quality, subsampling))
    last = [0, 0, 0]
    for n_mcu, mcu in enumerate(every):
        rst = None
        if n_mcu and n_mcu % restart_mcus == 0:
            rst, last = (n_mcu // restart_mcus - 1) % 8, [0, 0, 0]
        coded = []
        for table, comp, block in mcu:
            coded.append((table, block, last[comp]))
            last[comp] = int(block[0])
        yield rst, coded, (n_mcu + 1) % restart_mcus == 0 or n_mcu + 1 == len(every)


def histograms(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1, subsampling: int = 2) -> np.ndarray:
    """uint32 [4][257]: what the gather pass counts (entry 256, the reserved symbol, is 1)."""
    hist = np.zeros((4, 257), np.int64)
    hist[:, 256] = 1
    for _, coded, _ in _walk(rgb, quality, restart_mcus, subsampling):
        for table, block, last_dc in coded:
            _count_block(hist[2 * table], hist[2 * table + 1], block, last_dc)
    return hist.astype(np.uint32)


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


def tables(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1, subsampling: int = 2):
    """The four (bits, vals) of the frame."""
    return [gen_optimal_table(h) for h in histograms(rgb, quality, restart_mcus, subsampling)]


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


def encode(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1, subsampling: int = 2, optimize: bool = False,
           trace: Trace | None = None) -> bytes:
    """The whole file for a uint8 (H, W, 3) RGB image, with Annex K's Huffman tables or (`optimize`) the frame's own.
    A `trace` is filled with what was coded on the way."""
    rgb = np.asarray(rgb)
    four = tables(rgb, quality, restart_mcus, subsampling) if optimize else ANNEX_K
    codes = [_Codes(huff_codes(*t)) for t in four]
    out = bytearray(header(rgb.shape[0], rgb.shape[1], quality, restart_mcus, subsampling, four))
    bits = _Bits()
    for rst, coded, interval_end in _walk(rgb, quality, restart_mcus, subsampling):
        if rst is not None:                                               # emit_restart (flush_bits ran behind the MCU)
            out += bits.out + bytes([0xFF, 0xD0 + rst])
            bits = _Bits()
        bits_before, raw_before = bits.total, len(bits.raw)
        for table, block, last_dc in coded:
            _encode_block(bits, block, last_dc, codes[2 * table], codes[2 * table + 1], trace, table)
        mcu_bits = bits.total - bits_before
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
    encode(rgb, quality, restart_mcus, subsampling, optimize, trace=t)
    return t

