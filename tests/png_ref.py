"""The PNG encoder of transflow_amd/csrc/png.hip restated in numpy and plain Python (DESIGN.md section 16 has the rules).

8-bit RGB, colour type 2, no interlace.  Signature, IHDR, an IDAT with the zlib header 78 01, one IDAT per band of
`band_rows` rows, an IDAT with the final stored block 01 00 00 FF FF and the Adler-32 of the filtered stream, IEND.
A band is one dynamic-Huffman block over a literal/length code that is a constant of the library, a distance alphabet of
the single code 0, matches at distance 1 only, and an empty stored block behind it that brings the stream to a byte.

`encode` is the file, `filtered` the stream zlib must return for it, `trace` encode's own account of what it coded.
The image generators use integer arithmetic and no library's random generator.
"""
from __future__ import annotations

import heapq
import math
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
BAND_BYTES = 8192                      # the default band holds at least this much of the filtered stream
TRIP = 64                              # the bytes a wave of the device's coder takes at a time
SCAN_CHUNK = 1024                      # the bands k_slot_scan sums per trip

# RFC 1951 3.2.5: length symbol 257 + k stands for LENGTH_BASE[k] .. with LENGTH_EXTRA[k] extra bits
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


# ---- the constant literal/length code ------------------------------------------------------------------------------------
def weights() -> list:
    w = []
    for v in range(256):
        m = min(v, 256 - v)
        w.append(max(128, 65536 // math.isqrt((m + 1) ** 3)))
    return w + [128] + [512] * 28 + [4096]


def code_lengths() -> list:
    """Two-smallest merge on (weight, order): a leaf's order is its symbol, the k-th internal node's 1000 + k."""
    heap = [(w, s, (s,)) for s, w in enumerate(weights())]
    heapq.heapify(heap)
    depth = [0] * 286
    k = 0
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], 1000 + k, a[2] + b[2]))
        k += 1
    return depth


def canonical_codes(lengths) -> list:
    """RFC 1951 3.2.2."""
    count = [0] * (max(lengths) + 2)
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, next_code = 0, [0] * (max(lengths) + 2)
    for bits in range(1, max(lengths) + 1):
        code = (code + count[bits - 1]) << 1
        next_code[bits] = code
    codes = []
    for n in lengths:
        codes.append(next_code[n] if n else 0)
        next_code[n] += 1 if n else 0
    return codes


LENGTHS = code_lengths()
CODES = canonical_codes(LENGTHS)


def length_symbol(n: int) -> int:
    """The index k of the length symbol 257 + k that codes a match of n bytes."""
    k = 28 if n == 258 else max(i for i in range(28) if LENGTH_BASE[i] <= n)
    return k


def match_bits(n: int) -> int:
    k = length_symbol(n)
    return LENGTHS[257 + k] + LENGTH_EXTRA[k] + 1


def _reversed(code: int, bits: int) -> int:
    return int(format(code, f"0{bits}b")[::-1], 2)


class _Bits:
    """Deflate's bit order: the stream fills bytes from bit 0; Huffman codes go most significant bit first."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value: int, bits: int):
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code: int, bits: int):
        self.put(_reversed(code, bits), bits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def _table_header(bits: _Bits):
    bits.put(0, 1)                      # BFINAL
    bits.put(2, 2)                      # BTYPE 10
    bits.put(29, 5)                     # HLIT: 286 codes
    bits.put(0, 5)                      # HDIST: 1 code
    bits.put(15, 4)                     # HCLEN: 19 lengths
    for s in CLEN_ORDER:
        bits.put(0 if s >= 16 else 4, 3)
    for n in LENGTHS + [1]:             # 4-bit codes for the lengths 0 - 15: the code of a length is the length
        bits.huff(n, 4)


TABLE_BITS = 3 + 14 + 57 + 4 * 287
_HEADER = []


def default_band_rows(height: int, width: int) -> int:
    return min(height, max(1, -(-BAND_BYTES // (3 * width + 1))))


def slot_bytes(band_bytes: int) -> int:
    """The bound on a band's deflate data: the table header, the costliest coding of a byte for
    every byte, end-of-block, the stored block's three bits, the padding and its four bytes; a multiple of 4."""
    per_byte = max(max(LENGTHS[:256]), max(-(-match_bits(n) // n) for n in range(3, 259)))
    bits = TABLE_BITS + band_bytes * per_byte + LENGTHS[256] + 3 + 7 + 32
    return (bits // 8 + 3) & ~3


def file_bound(height: int, width: int, band_rows: int) -> int:
    rows = band_rows if band_rows else default_band_rows(height, width)
    rows = min(rows, height)
    total = 8 + 25 + 14 + 21 + 12
    for first in range(0, height, rows):
        total += 12 + slot_bytes(min(rows, height - first) * (3 * width + 1))
    return total


# ---- filtering -------------------------------------------------------------------------------------------------------------
def _candidates(image: np.ndarray) -> np.ndarray:
    """(5, H, 3 W) uint8: every row filtered with each type; the row above the first is zeros."""
    h, w, _ = image.shape
    cur = image.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(cur)
    a[:, 3:] = cur[:, :-3]
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    c = np.zeros_like(cur)
    c[:, 3:] = b[:, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([cur, cur - a, cur - b, cur - ((a + b) >> 1), cur - paeth]).astype(np.uint8)


def filter_rows(image: np.ndarray):
    """(types (H,), rows (H, 1 + 3 W) uint8): the type with the smallest sum of min(b, 256 - b), ties to the lowest."""
    cand = _candidates(image)
    v = cand.astype(np.int64)
    cost = np.minimum(v, 256 - v).sum(axis=2)                    # (5, H)
    types = np.argmin(cost, axis=0)                              # the first of equal minima
    h = image.shape[0]
    rows = np.empty((h, 1 + cand.shape[2]), np.uint8)
    rows[:, 0] = types
    rows[:, 1:] = cand[types, np.arange(h)]
    return types, rows


def filtered(image: np.ndarray) -> bytes:
    return filter_rows(np.asarray(image))[1].tobytes()


# ---- a band's tokens -------------------------------------------------------------------------------------------------------
def stretches(data: np.ndarray):
    """[(start, n)]: the maximal stretches of bytes equal to their predecessor inside the band."""
    eq = np.zeros(len(data) + 2, bool)
    eq[2:-1] = data[1:] == data[:-1]                              # eq[i + 1]: byte i equals byte i - 1
    edges = np.flatnonzero(eq[1:] != eq[:-1])                     # byte j differs from byte j - 1 in that
    return [(int(s), int(e - s)) for s, e in zip(edges[0::2], edges[1::2])]


def tokens(data: np.ndarray):
    """[(position, kind, value)] in stream order; kind "lit" (value: the byte), "match" (value: the length) or "eob".
    `position` is the band byte whose lane emits the token in the device's coder: a match of 258 where the count
    reaches it, whatever a stretch leaves at the byte behind its end, a literal at itself, end-of-block at len(data)."""
    out = []
    n_bytes = len(data)
    at = 0
    for start, n in stretches(data) + [(n_bytes, 0)]:
        for i in range(at, start):
            out.append((i, "lit", int(data[i])))
        if n == 0:
            break
        done = 0
        while n - done >= 258:
            done += 258
            out.append((start + done - 1, "match", 258))
        rest = n - done
        if rest >= 3:
            out.append((start + n, "match", rest))
        else:
            out.extend((start + n, "lit", int(data[start])) for _ in range(rest))
        at = start + n
    out.append((n_bytes, "eob", 256))
    return out


def token_bits(kind: str, value: int) -> int:
    return match_bits(value) if kind == "match" else LENGTHS[value]


def band_data(data: np.ndarray, toks=None) -> bytes:
    bits = _Bits()
    if not _HEADER:                                               # made once: it is the same for every band
        _table_header(bits)
        assert 8 * len(bits.out) + bits.n == TABLE_BITS
        _HEADER.extend([bytes(bits.out), bits.acc, bits.n])
    bits.out, bits.acc, bits.n = bytearray(_HEADER[0]), _HEADER[1], _HEADER[2]
    for _, kind, value in toks if toks is not None else tokens(data):
        if kind == "match":
            k = length_symbol(value)
            bits.huff(CODES[257 + k], LENGTHS[257 + k])
            bits.put(value - LENGTH_BASE[k], LENGTH_EXTRA[k])
            bits.put(0, 1)                                        # the distance code
        else:
            bits.huff(CODES[value], LENGTHS[value])
    bits.put(0, 3)                                                # an empty stored block: not final, BTYPE 00
    bits.align()
    return bytes(bits.out) + b"\x00\x00\xff\xff"


def chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def adler32(data: bytes) -> int:
    """In blocks whose sums the host combines, as the library does with its rows' sums."""
    s1, s2 = 1, 0
    for first in range(0, len(data), 4099):
        block = np.frombuffer(data[first:first + 4099], np.uint8).astype(np.int64)
        n = len(block)
        s2 = (s2 + n * s1 + int((block * np.arange(n, 0, -1)).sum())) % 65521
        s1 = (s1 + int(block.sum())) % 65521
    return (s2 << 16) | s1


class Trace:
    def __init__(self):
        self.data = b""
        self.filter_types = []          # per row
        self.length_symbols = set()     # 257 ..
        self.runs = []                  # (band, start, n) of every stretch
        self.longest_run = 0
        self.widest_trip = 0            # bits the lanes of one 64-byte trip emit
        self.bands = 0
        self.row_bytes = 0
        self.band_rows = 0
        self.band_bytes = []            # per band

    @property
    def phase_lengths(self):
        """{(the place in its trip where a stretch starts, its length)}."""
        return {(start % TRIP, n) for _, start, n in self.runs}

    @property
    def match_258_lanes(self):
        """The lanes that emit a match of 258: where the count reaches it."""
        return {(start + 258 * j - 1) % TRIP for _, start, n in self.runs for j in range(1, n // 258 + 1)}

    @property
    def pending_literals(self):
        """{(lane, count)}: the one or two literals a stretch leaves, emitted at the lane behind its end."""
        return {((start + n) % TRIP, n % 258) for _, start, n in self.runs if n % 258 in (1, 2)}

    @property
    def ends_at_band_end(self):
        """{(the band's bytes, the stretch's length)} of the stretches whose last byte is their band's last."""
        return {(self.band_bytes[band], n) for band, start, n in self.runs if start + n == self.band_bytes[band]}


def encode(image: np.ndarray, band_rows: int = 0, trace: Trace | None = None) -> bytes:
    image = np.asarray(image)
    h, w, _ = image.shape
    assert image.dtype == np.uint8 and image.shape[2] == 3
    rows = min(h, band_rows if band_rows else default_band_rows(h, w))
    types, lines = filter_rows(image)
    out = bytearray(SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", b"\x78\x01"))
    for band, first in enumerate(range(0, h, rows)):
        data = lines[first:first + rows].reshape(-1)
        toks = tokens(data)
        out += chunk(b"IDAT", band_data(data, toks))
        if trace is not None:
            trips = {}
            for pos, kind, value in toks:
                trips[pos // TRIP] = trips.get(pos // TRIP, 0) + token_bits(kind, value)
                if kind == "match":
                    trace.length_symbols.add(257 + length_symbol(value))
            trace.widest_trip = max(trace.widest_trip, max(trips.values()))
            trace.runs += [(band, s, n) for s, n in stretches(data)]
    stream = lines.tobytes()
    assert adler32(stream) == zlib.adler32(stream)
    out += chunk(b"IDAT", b"\x01\x00\x00\xff\xff" + struct.pack(">I", adler32(stream))) + chunk(b"IEND", b"")
    if trace is not None:
        trace.data = bytes(out)
        trace.filter_types = [int(t) for t in types]
        trace.longest_run = max((n for _, _, n in trace.runs), default=0)
        trace.bands = -(-h // rows)
        trace.row_bytes, trace.band_rows = 1 + 3 * w, rows
        trace.band_bytes = [min(rows, h - first) * (1 + 3 * w) for first in range(0, h, rows)]
    return bytes(out)


def trace(image: np.ndarray, band_rows: int = 0) -> Trace:
    t = Trace()
    encode(image, band_rows, t)
    return t


def chunks(data: bytes):
    """[(kind, payload, crc)] of a file, the signature checked."""
    assert data[:8] == SIGNATURE
    out, at = [], 8
    while at < len(data):
        n = struct.unpack(">I", data[at:at + 4])[0]
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n], struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0]))
        at += 12 + n
    assert at == len(data)
    return out


# ---- images: integer formulas only ------------------------------------------------------------------------------------------
def _hash(seed: int, n: int) -> np.ndarray:
    """n uint32 of a multiply-xorshift hash of (seed, index)."""
    x = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B9) + np.uint64(1)) & np.uint64(0xFFFFFFFF)
    for mul in (0x7FEB352D, 0x846CA68B):
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(mul)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def noise_image(height: int, width: int, seed: int) -> np.ndarray:
    return (_hash(seed, height * width * 3) >> np.uint32(24)).astype(np.uint8).reshape(height, width, 3)


def black_image(height: int, width: int) -> np.ndarray:
    return np.zeros((height, width, 3), np.uint8)


def ramp_image(width: int) -> np.ndarray:
    """1 x W, every channel (-x) mod 256: Sub wins, and behind one literal 255 every byte equals its predecessor."""
    x = (-np.arange(width)) % 256
    return np.repeat(x.astype(np.uint8), 3).reshape(1, width, 3)


def runs_image() -> np.ndarray:
    """One row: for n = 3 .. 258 a byte 1 and n + 1 zeros -- a stretch of exactly n behind two literals -- and a last 1
    that makes the bytes a multiple of three.  None is the filter with the smallest sum (256 ones + 1)."""
    parts = []
    for n in range(3, 259):
        parts.append(np.concatenate([[1], np.zeros(n + 1, np.int64)]))
    row = np.concatenate(parts + [[1]]).astype(np.uint8)
    assert len(row) % 3 == 0
    return row.reshape(1, -1, 3)


def smear_image(height: int, width: int, by: int, bx: int, seed: int) -> np.ndarray:
    """ceil(H / by) x ceil(W / bx) hashed colours, each smeared over by x bx pixels."""
    gy, gx = -(-height // by), -(-width // bx)
    colours = noise_image(gy, gx, seed)
    return np.repeat(np.repeat(colours, by, axis=0), bx, axis=1)[:height, :width].copy()


def edge_image() -> np.ndarray:
    """One row made as runs_image's: stretches of exactly 2, 258, 259, 260, 261 and 516."""
    parts = [np.concatenate([[1], np.zeros(n + 1, np.int64)]) for n in (2, 258, 259, 260, 261, 516)]
    row = np.concatenate(parts + [[1]]).astype(np.uint8)
    assert len(row) % 3 == 0
    return row.reshape(1, -1, 3)


SWEEP = (1, 2, 3, 4, 257, 258, 259, 260, 261, 515, 516, 517, 518, 774)
SWEEP_PARTS = {"a": SWEEP[:8], "b": SWEEP[8:11], "c": SWEEP[11:]}     # a row holds at most 3 * 65535 + 1 bytes


def sweep_image(lengths) -> np.ndarray:
    """One row of bytes 0 and 1 whose filtered stream (None: a 0 and the row) holds, for every n of `lengths` and every
    phase p of 0 .. 63, a stretch of exactly n that starts at a stream position p (mod 64): a 1, a 0 and n more zeros.
    Between them 1 and 0 alternate; where the next phase has the other parity a single 2 takes the place of a 1.  Behind
    a stretch that leaves one or two literals to lane 0 of the next trip, that trip is padded to its end, with a 1 last."""
    s = [0, 1]                                                    # the filter type, the first byte of the row
    for n in lengths:
        for p in range(TRIP):
            start = len(s) + 1 + (p - len(s) - 1) % TRIP          # the first place of phase p with room for the 0 before it
            if (start - 1 - len(s)) % 2:
                s.append(2)
            while len(s) < start:
                s.append(0 if s[-1] else 1)
            assert s[-1] == 0 and s[-2] != 0
            s.extend([0] * n + [1])
            if len(s) % TRIP == 1 and n % 258 in (1, 2):          # lane 0 emits the pending zeros: they are prev_last's,
                s.append(2)                                       # so this trip's last byte is made a 1
                while len(s) % TRIP:
                    s.append(0 if s[-1] else 1)
                assert s[-1] == 1
    while (len(s) - 1) % 3:
        s.append(0 if s[-1] else 1)
    return np.array(s[1:], np.uint8).reshape(1, -1, 3)


def grey_tail_image(height: int, width: int, seed: int) -> np.ndarray:
    """Noise whose row r ends in 1 + r % 3 pixels of the grey 90: whichever filter wins, the row ends in a stretch."""
    image = noise_image(height, width, seed)
    for r in range(height):
        image[r, width - 1 - r % 3:] = 90
    return image


NOISE_SEED = 11

# name: (the image's maker, band_rows)
CASES = {
    "1x1": (lambda: noise_image(1, 1, 1), 0),
    "1x21": (lambda: noise_image(1, 21, 2), 0),
    "1x22": (lambda: noise_image(1, 22, 3), 0),
    "7x1": (lambda: noise_image(7, 1, 4), 0),
    **{f"24x40_noise_b{b}": ((lambda: noise_image(24, 40, NOISE_SEED)), b) for b in (1, 2, 3, 5, 24, 1000)},
    "9x50_black_b3": (lambda: black_image(9, 50), 3),
    "1x6000_ramp": (lambda: ramp_image(6000), 0),
    "1x4099_noise": (lambda: noise_image(1, 4099, 5), 0),
    "runs_3_to_258": (runs_image, 0),
    "1025x1_b1": (lambda: noise_image(1025, 1, 6), 1),
    "2049x2_b1": (lambda: noise_image(2049, 2, 7), 1),
    "40x300_smear": (lambda: smear_image(40, 300, 8, 50, 8), 0),
    "1x523_edges": (edge_image, 0),
    # every stretch length of SWEEP at every place of a trip
    **{f"sweep_{part}": ((lambda part=part: sweep_image(SWEEP_PARTS[part])), 1) for part in SWEEP_PARTS},
    # bands of 256 and 512 bytes: rows of 256 one and two to a band, four rows of 64 in one band
    **{f"4x85_{kind}_b{b}": (maker, b) for b in (1, 2) for kind, maker in
       (("noise", lambda: noise_image(4, 85, 21)), ("black", lambda: black_image(4, 85)),
        ("tail", lambda: grey_tail_image(4, 85, 22)))},
    "4x21_noise_b4": (lambda: noise_image(4, 21, 23), 4),
    "4x21_black_b4": (lambda: black_image(4, 21), 4),
    "4x21_tail_b4": (lambda: grey_tail_image(4, 21, 24), 4),
    # rows of 65524 bytes, more than Adler-32's 65521
    "2x21841_noise_b1": (lambda: noise_image(2, 21841, 25), 1),
    "3x21841_black": (lambda: black_image(3, 21841), 0),
}
# the cases whose image is all noise: the staging bound is asserted on their files
NOISE_CASES = [name for name in CASES if "noise" in name or name in ("1x1", "1x21", "1x22", "7x1", "1025x1_b1", "2049x2_b1")]


def case(name: str):
    maker, band_rows = CASES[name]
    return maker(), band_rows
