"""numpy restatement of libjpeg's baseline encoder as transflow_amd/csrc/jpeg.hip runs it: 8-bit YCbCr 4:2:0, one
interleaved scan, the Annex K Huffman tables, jpeg_set_quality's tables, a restart interval counted in MCUs.

Every rule is libjpeg's integer arithmetic, so `encode()` returns the very file Pillow writes for
`save(quality=q, subsampling=2, restart_marker_blocks=r)` (tests/test_jpeg_ref.py holds it to that, byte for byte):

  jccolor.c   rgb_ycc_convert           16-bit fixed point
  jcsample.c  h2v2_downsample           (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2 ... along the output row
  jcprepct.c  pre_process_data          input rows replicated to an even count, the DOWNSAMPLED rows replicated below
  jfdctint.c  jpeg_fdct_islow           CONST_BITS 13, PASS1_BITS 2, on samples - 128
  jcdctmgr.c  forward_DCT               divisor 8 Q[k], rounded half away from zero
  jccoefct.c  compress_data             dummy luma blocks: AC zero, DC of the block before them in the MCU
  jchuff.c    encode_one_block, emit_restart, flush_bits
  jcmarker.c  the header

`trace()` is `encode()` with an account of what it coded: symbols, lane widths, MCU sizes, the bytes each MCU flushes.
"""
from __future__ import annotations

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


def header(height: int, width: int, quality: int, restart_mcus: int) -> bytes:
    """jcmarker.c write_file_header, write_frame_header, write_scan_header, in libjpeg's order."""
    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for n, base in enumerate((QUANT_LUMA, QUANT_CHROMA)):
        out += seg(0xDB, bytes([n]) + bytes(int(v) for v in quant_table(base, quality)[ZIGZAG]))
    out += seg(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big")
               + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
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


def encode(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1, trace: Trace | None = None) -> bytes:
    """The whole file for a uint8 (H, W, 3) RGB image.  A `trace` is filled with what was coded on the way."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and restart_mcus >= 1
    H, W = rgb.shape[:2]
    mcus_x, mcus_y = (W + 15) // 16, (H + 15) // 16
    lum_bx, lum_by = (W + 7) // 8, (H + 7) // 8                        # the luma block grid; beyond it: dummy blocks
    y, cb, cr = ycc(rgb)
    y = pad_bottom(pad_right(y, lum_bx * 8), lum_by * 8)
    chroma = []
    for plane in (cb, cr):
        plane = pad_bottom(pad_right(plane, mcus_x * 16), H + (H & 1))    # rows only to an even count ...
        chroma.append(pad_bottom(downsample(plane), mcus_y * 8))          # ... then the downsampled rows
    tl, tc = quant_table(QUANT_LUMA, quality), quant_table(QUANT_CHROMA, quality)
    cy, ccb, ccr = blocks_quantised(y, tl), blocks_quantised(chroma[0], tc), blocks_quantised(chroma[1], tc)
    dc_l, ac_l, dc_c, ac_c = (huff_codes(*t) for t in (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA))
    zero = np.zeros(64, np.int64)
    out = bytearray(header(H, W, quality, restart_mcus))
    bits, last, n_mcu = _Bits(), [0, 0, 0], 0
    for my in range(mcus_y):
        for mx in range(mcus_x):
            if n_mcu and n_mcu % restart_mcus == 0:                       # emit_restart (flush_bits ran behind the MCU)
                out += bits.out + bytes([0xFF, 0xD0 + (n_mcu // restart_mcus - 1) % 8])
                bits, last = _Bits(), [0, 0, 0]
            n_mcu += 1
            bits_before, raw_before = bits.total, len(bits.raw)
            prev = None
            for b in range(4):
                by, bx = 2 * my + (b >> 1), 2 * mx + (b & 1)
                if by < lum_by and bx < lum_bx:
                    block = cy[by, bx]
                else:                                                     # jccoefct.c: a dummy block
                    block = zero.copy()
                    block[0] = prev[0]
                _encode_block(bits, block, last[0], dc_l, ac_l, trace, 0)
                last[0] = int(block[0])
                prev = block
            for c, coef in ((1, ccb), (2, ccr)):
                block = coef[my, mx]
                _encode_block(bits, block, last[c], dc_c, ac_c, trace, 1)
                last[c] = int(block[0])
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


def trace(rgb: np.ndarray, quality: int = 50, restart_mcus: int = 1) -> Trace:
    """`encode`, the same code, returning what it coded."""
    t = Trace()
    encode(rgb, quality, restart_mcus, t)
    return t


# ---- the fixtures' cases (tools/capture_golden_jpeg.py writes them, the tests read them) -----------------------------
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


def noise_image(height: int, width: int, seed: int) -> np.ndarray:
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


# name -> (height, width, content, quality, restart_mcus); content is a kind, or (kind, seed)
CASES = {
    "1x1": (1, 1, "stored", 50, 4),
    "9x7": (9, 7, "stored", 50, 4),
    "16x16": (16, 16, "stored", 50, 4),
    "17x33": (17, 33, "stored", 50, 4),
    "45x61": (45, 61, "stored", 50, 4),
    "24x40": (24, 40, "stored", 50, 4),
    "8x100": (8, 100, "stored", 50, 4),
    "33x47_noise_q100": (33, 47, "noise", 100, 4),
    "33x47_noise_q1": (33, 47, "noise", 1, 4),
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


def case_image(name: str) -> np.ndarray:
    """The picture of a case: what tools/capture_golden_jpeg.py gives Pillow."""
    h, w, content, _, _ = CASES[name]
    kind, seed = content if isinstance(content, tuple) else (content, None)
    if kind == "stored":
        return stored_image(h, w, seed=h * 1000 + w)                     # the same picture for every case of a size
    if kind == "noise":
        return noise_image(h, w, seed=7)
    return _made_image(kind, h, w, seed)


def _made_image(kind: str, height: int, width: int, seed) -> np.ndarray:
    """The content kinds that are pure functions of their parameters: a fixture stores those."""
    if kind in ("directed_luma", "directed_chroma", "binary_noise"):
        return {"directed_luma": directed_luma, "directed_chroma": directed_chroma,
                "binary_noise": binary_noise}[kind](height, width, int(seed))
    return {"checker": checkerboard, "chroma_checker": chroma_checker, "formula": formula_image}[kind](height, width)


def load_case(path: str):
    """(image, quality, restart_mcus, expected file bytes) of a tests/golden/jpeg_*.npz fixture."""
    with np.load(path) as z:
        quality, restart = int(z["quality"]), int(z["restart_mcus"])
        if "image" in z.files:
            image = z["image"]
        else:                                                             # (the first such fixtures name no content)
            kind = str(z["content"]) if "content" in z.files else "formula"
            image = _made_image(kind, int(z["height"]), int(z["width"]), z["seed"] if "seed" in z.files else None)
        return image, quality, restart, z["jpeg"].tobytes()
