"""The flow archive member coder of transflow_amd/csrc/flowzip.hip restated in numpy and plain Python (DESIGN.md section 17
has the rules).

A member's uncompressed stream is S = prefix ‖ data: the `.npy` header numpy.save writes, then the array's C-order bytes.
S is cut into bands of `band_bytes`; a byte is *equal* if it equals the byte `distance` before it inside its band; a
maximal stretch of n equal bytes is a match of 258 while n >= 258, then a match of n if n >= 3, else n literals.  The
literal/length code is built from the tokens of ALL bands (every band brings one end-of-block), by merging the two
smallest on (weight, order); a band whose coded form would not be smaller than its stored form is then stored -- its
counts stay in the histogram, the table is not rebuilt.  The stream ends with 01 00 00 FF FF.

`encode_stream` is the stream, the CRC-32 of S and the code lengths; `trace` its own account of what a case reached;
`round_i64` the round kernel; `zip_records` a walk over an archive's records.  The generators use integer arithmetic
and no library's random generator.
"""
from __future__ import annotations

import heapq
import io
import struct
import zlib

import numpy as np

TRIP = 64                              # the bytes a wave of the device's coder takes at a time
SCAN_CHUNK = 1024                      # the bands k_fz_scan sums per trip
STORED_MAX = 65535

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49]          # RFC 1951 3.2.5, as far as 64
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
END_OF_BLOCK = 256
N_SYMBOLS = 286

_LENGTH_SYMBOL = np.zeros(259, np.int64)                       # n -> k of the length symbol 257 + k
for _k in range(28):
    _LENGTH_SYMBOL[LENGTH_BASE[_k]:] = _k
_LENGTH_SYMBOL[258] = 28


def distance_symbol(distance: int) -> int:
    assert 1 <= distance <= 64
    return max(k for k in range(12) if DIST_BASE[k] <= distance)


def header_bits(distance: int) -> int:
    return 3 + 14 + 3 * 19 + 4 * (N_SYMBOLS + distance_symbol(distance) + 1)


def bound(n: int, band_bytes: int) -> int:
    """N + 5 per stored block + 5."""
    blocks = 0
    for first in range(0, n, band_bytes):
        blocks += -(-min(band_bytes, n - first) // STORED_MAX)
    return n + 5 * blocks + 5


# ---- the code --------------------------------------------------------------------------------------------------------------
def huffman_lengths(weights, first_node: int = 1000) -> list:
    """Two-smallest merge on (weight, order) over the symbols of weight > 0: a leaf's order is its symbol, the k-th
    internal node's 1000 + k.  The others get 0.  (`first_node` = -1000 is the other rule, internal nodes before leaves
    of their weight: the tests use it to show that a case depends on the rule.)"""
    heap = [(int(w), s, (s,)) for s, w in enumerate(weights) if w > 0]
    heapq.heapify(heap)
    depth = [0] * len(weights)
    k = 0
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], first_node + k, a[2] + b[2]))
        k += 1
    return depth


def build_lengths(counts, first_node: int = 1000):
    """(lengths, repairs): while a length exceeds 15 every used weight becomes max(1, w >> 1) and the code is rebuilt."""
    weights = [int(c) for c in counts]
    repairs = 0
    while True:
        lengths = huffman_lengths(weights, first_node)
        if max(lengths) <= 15:
            return lengths, repairs
        weights = [max(1, w >> 1) if w > 0 else 0 for w in weights]
        repairs += 1


def canonical_codes(lengths) -> list:
    """RFC 1951 3.2.2."""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, next_code = 0, [0] * 17
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        next_code[bits] = code
    codes = []
    for n in lengths:
        codes.append(next_code[n] if n else 0)
        next_code[n] += 1 if n else 0
    return codes


def _reversed(code: int, bits: int) -> int:
    return int(format(code, f"0{bits}b")[::-1], 2) if bits else 0


def _pack(values: np.ndarray, nbits: np.ndarray, acc: int = 0, n_acc: int = 0):
    """The bits of `values` (from bit 0, nbits each) behind the n_acc bits of acc: (whole bytes, bits left, their count)."""
    values = np.concatenate([[acc], values]).astype(np.uint64)
    nbits = np.concatenate([[n_acc], nbits]).astype(np.int64)
    total = int(nbits.sum())
    start = np.cumsum(nbits) - nbits
    which = np.repeat(np.arange(len(nbits)), nbits)
    shift = (np.arange(total) - start[which]).astype(np.uint64)
    bits = ((values[which] >> shift) & np.uint64(1)).astype(np.uint8)
    whole = total // 8 * 8
    out = np.packbits(bits[:whole], bitorder="little").tobytes()
    rest = bits[whole:]
    return out, int(sum(int(b) << i for i, b in enumerate(rest))), len(rest)


# ---- a band's tokens -------------------------------------------------------------------------------------------------------
def stretches(band: np.ndarray, distance: int):
    """[(start, n)]: the maximal stretches of bytes equal to the byte `distance` before them inside the band."""
    eq = np.zeros(len(band) + 2, bool)
    if len(band) > distance:
        eq[1 + distance:-1] = band[distance:] == band[:-distance]
    edges = np.flatnonzero(eq[1:] != eq[:-1])
    return [(int(s), int(e - s)) for s, e in zip(edges[0::2], edges[1::2])]


def tokens(band: np.ndarray, distance: int):
    """(position, symbol, length) arrays in stream order: symbol < 256 a literal, 256 end-of-block, 257 + k a match of
    `length` bytes.  `position` is the band byte whose lane emits the token in the device's coder: a match of 258
    where the count reaches it, whatever a stretch leaves at the byte behind its end, a literal at itself."""
    pos, sym, length = [], [], []
    at = 0
    band64 = band.astype(np.int64)

    def literals(first, last, where=None):
        if last > first:
            pos.append(np.arange(first, last) if where is None else np.full(last - first, where))
            sym.append(band64[first:last])
            length.append(np.zeros(last - first, np.int64))

    for start, n in stretches(band, distance):
        literals(at, start)
        done = 0
        while n - done >= 258:
            done += 258
            pos.append([start + done - 1]), sym.append([257 + 28]), length.append([258])
        rest = n - done
        if rest >= 3:
            pos.append([start + n]), sym.append([257 + int(_LENGTH_SYMBOL[rest])]), length.append([rest])
        else:
            literals(start + done, start + n, where=start + n)
        at = start + n
    literals(at, len(band))
    pos.append([len(band)]), sym.append([END_OF_BLOCK]), length.append([0])
    return (np.concatenate(pos).astype(np.int64), np.concatenate(sym).astype(np.int64),
            np.concatenate(length).astype(np.int64))


def stored_bytes(n: int) -> int:
    return n + 5 * -(-n // STORED_MAX)


def stored_band(band: np.ndarray) -> bytes:
    out = bytearray()
    raw = band.tobytes()
    for first in range(0, len(raw), STORED_MAX):
        piece = raw[first:first + STORED_MAX]
        out += struct.pack("<BHH", 0, len(piece), len(piece) ^ 0xFFFF) + piece
    return bytes(out)


class Trace:
    def __init__(self):
        self.stream = b""
        self.crc = 0
        self.lengths = []
        self.n = 0
        self.band_bytes = 0
        self.distance = 0
        self.bands = 0
        self.band_offsets = []          # n_bands + 1: where each band's bytes begin in the stream, and where the last ends
        self.band_coded = []            # per band
        self.stretches = []             # (band, start, n)
        self.repairs = 0                # how often the weights were halved
        self.used_symbols = 0
        self.kraft = 0.0
        self.widest_trip = 0            # bits the lanes of one 64-byte trip emit
        self.cut_by_band = 0            # stretches of the uncut stream that a band's first byte cuts
        self.first_bytes_would_match = 0  # bands after the first whose first D bytes hold one equal to the byte D before

    @property
    def stretch_lengths(self):
        return {n for _, _, n in self.stretches}

    def _coded_stretches(self):
        return [(start, n) for band, start, n in self.stretches if self.band_coded[band]]

    @property
    def phase_lengths(self):
        """{(the place in its trip where a stretch starts, its length)}, over the bands k_fz_emit tokenises."""
        return {(start % TRIP, n) for start, n in self._coded_stretches()}

    @property
    def match_258_lanes(self):
        """The lanes that emit a match of 258: where the count reaches it."""
        return {(start + 258 * j - 1) % TRIP for start, n in self._coded_stretches() for j in range(1, n // 258 + 1)}

    @property
    def pending_literals(self):
        """{(lane, count)}: the one or two literals a stretch leaves, emitted at the lane behind its end."""
        return {((start + n) % TRIP, n % 258) for start, n in self._coded_stretches() if n % 258 in (1, 2)}

    @property
    def ends_at_band_end(self):
        """{(the band's bytes, the stretch's length)} of the stretches whose last byte is a coded band's last."""
        out = set()
        for band, start, n in self.stretches:
            size = min(self.band_bytes, self.n - band * self.band_bytes)
            if self.band_coded[band] and start + n == size:
                out.add((size, n))
        return out

    @property
    def across_trip(self):
        return any(start // TRIP != (start + n - 1) // TRIP for _, start, n in self.stretches)


def encode_stream(prefix: bytes, data: bytes, band_bytes: int, distance: int, trace: Trace | None = None):
    """(the raw deflate stream, zlib.crc32 of S, the 286 code lengths)."""
    assert band_bytes >= 64 and band_bytes % 64 == 0 and 1 <= distance <= 64
    S = np.frombuffer(bytes(prefix) + bytes(data), np.uint8)
    n = len(S)
    assert n >= 1
    bands = [S[first:first + band_bytes] for first in range(0, n, band_bytes)]
    toks = [tokens(band, distance) for band in bands]
    counts = np.zeros(N_SYMBOLS, np.int64)
    for _, sym, _ in toks:
        counts += np.bincount(sym, minlength=N_SYMBOLS)
    lengths, repairs = build_lengths(counts)
    codes = canonical_codes(lengths)
    rev = np.array([_reversed(c, b) for c, b in zip(codes, lengths)], np.int64)
    len_arr = np.array(lengths, np.int64)
    hdist = distance_symbol(distance)
    dist_extra, dist_bits = distance - DIST_BASE[hdist], DIST_EXTRA[hdist]

    head_v = [0, 2, 29, hdist, 15] + [0 if s >= 16 else 4 for s in CLEN_ORDER]
    head_n = [1, 2, 5, 5, 4] + [3] * 19
    for ln in lengths + [0] * hdist + [1]:           # 4-bit codes for the lengths 0 - 15: the code of a length is the length
        head_v.append(_reversed(ln, 4)), head_n.append(4)
    head_bytes, head_acc, head_left = _pack(np.array(head_v), np.array(head_n))
    assert 8 * len(head_bytes) + head_left == header_bits(distance)

    out = bytearray()
    offsets, coded_flags, widest = [], [], 0
    for band, (pos, sym, length) in zip(bands, toks):
        k = np.where(sym > END_OF_BLOCK, sym - 257, 0)
        is_match = sym > END_OF_BLOCK
        lext = np.where(is_match, np.array(LENGTH_EXTRA)[k], 0)
        extra = np.where(is_match, (length - np.array(LENGTH_BASE)[k]) | (dist_extra << (lext + 1)), 0)
        extra_bits = np.where(is_match, lext + 1 + dist_bits, 0)
        nbits = len_arr[sym] + extra_bits
        values = rev[sym] | (extra << len_arr[sym])
        bits = header_bits(distance) + int(nbits.sum())
        coded = (bits + 3 + 7) // 8 + 4
        offsets.append(len(out))
        if coded < stored_bytes(len(band)):
            body, acc, left = _pack(values, nbits, head_acc, head_left)
            body2, _, left2 = _pack(np.array([0]), np.array([3 + (-(left + 3)) % 8]), acc, left)
            assert left2 == 0
            piece = head_bytes + body + body2 + b"\x00\x00\xff\xff"
            assert len(piece) == coded
            out += piece
            coded_flags.append(True)
            widest = max(widest, int(np.bincount(pos // TRIP, weights=nbits).max()))
        else:
            out += stored_band(band)
            coded_flags.append(False)
    offsets.append(len(out))
    out += b"\x01\x00\x00\xff\xff"
    crc = zlib.crc32(S.tobytes())
    if trace is not None:
        trace.stream, trace.crc, trace.lengths = bytes(out), crc, list(lengths)
        trace.n, trace.band_bytes, trace.distance, trace.bands = n, band_bytes, distance, len(bands)
        trace.band_offsets, trace.band_coded = offsets, coded_flags
        trace.stretches = [(b, s, m) for b, band in enumerate(bands) for s, m in stretches(band, distance)]
        trace.repairs, trace.used_symbols = repairs, int((counts > 0).sum())
        trace.kraft = sum(2.0 ** -ln for ln in lengths if ln)
        trace.widest_trip = widest
        for start, m in stretches(S, distance):
            trace.cut_by_band += sum(1 for b in range(1, len(bands)) if start < b * band_bytes < start + m)
        for b in range(1, len(bands)):
            first = b * band_bytes
            head = S[first:first + distance]
            trace.first_bytes_would_match += bool((head == S[first - distance:first - distance + len(head)]).any())
    return bytes(out), crc, list(lengths)


def trace(prefix: bytes, data: bytes, band_bytes: int, distance: int) -> Trace:
    t = Trace()
    encode_stream(prefix, data, band_bytes, distance, t)
    return t


class RefEncoder:
    """The restatement behind the interface DeviceFlowArchiveWriter asks of its encoder (transflow_amd/flowzip.py)."""

    def __init__(self, band_bytes: int = 4096):
        self.band_bytes = band_bytes
        self.calls = []

    def encode_host(self, prefix: bytes, array: np.ndarray, distance: int):
        self.calls.append(("host", array.dtype.str, distance))
        stream, crc, _ = encode_stream(prefix, array.tobytes(), self.band_bytes, distance)
        return stream, crc

    def encode_device(self, prefix: bytes, dev_ptr: int, nbytes: int, distance: int):
        raise AssertionError("the restatement has no device")

    def close(self):
        pass


# ---- the round kernel ------------------------------------------------------------------------------------------------------
def round_i64(x: np.ndarray) -> np.ndarray:
    """numpy.round(x).astype(int) as the kernel states it: half to even in x's type, then the conversion; a value that
    does not fit, or a NaN, gives 0x8000000000000000."""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64)
    r = np.rint(x)
    fits = (r >= x.dtype.type(-2.0 ** 63)) & (r < x.dtype.type(2.0 ** 63))          # (false for NaN)
    out = np.full(x.shape, np.iinfo(np.int64).min, np.int64)
    out[fits] = r[fits].astype(np.int64)
    return out


def round_values(dtype) -> np.ndarray:
    t = np.dtype(dtype).type
    edge = t(2.0 ** 63)
    return np.array([0.5, -0.5, 1.5, -1.5, 2.5, 0.0, -0.0, np.nextafter(edge, t(0)), edge, np.nextafter(edge, t(np.inf)),
                     np.nextafter(-edge, t(0)), -edge, np.nextafter(-edge, t(-np.inf)), np.inf, -np.inf, np.nan,
                     3.4999, -7.5, 1e10, -1e10], dtype)


# ---- the zip records ---------------------------------------------------------------------------------------------------------
def zip_records(data: bytes) -> dict:
    """What an archive holds, by its own records: {"members": [(name, method, crc, csize, usize, offset, zip64)],
    "zip64_end": bool, "entries": n}.  Walks the end record, the ZIP64 end record if the locator is there, and the
    central directory; checks every local header against its central entry."""
    end = data.rfind(b"PK\x05\x06")
    assert end >= 0
    _, _, _, n_disk, n_total, cd_size, cd_offset, _ = struct.unpack("<IHHHHIIH", data[end:end + 22])
    zip64_end = data[end - 20:end - 16] == b"PK\x06\x07"
    if zip64_end:
        _, _, at, _ = struct.unpack("<IIQI", data[end - 20:end])
        assert data[at:at + 4] == b"PK\x06\x06"
        _, _, _, _, _, _, n_disk, n_total, cd_size, cd_offset = struct.unpack("<IQHHIIQQQQ", data[at:at + 56])
    members, at = [], cd_offset
    for _ in range(n_total):
        (sig, _, need, flags, method, _, _, crc, csize, usize, n_name, n_extra, n_comment, _, _, _, offset) = struct.unpack(
            "<IHHHHHHIIIHHHHHII", data[at:at + 46])
        assert sig == 0x02014B50 and flags == 0
        name = data[at + 46:at + 46 + n_name].decode()
        extra = data[at + 46 + n_name:at + 46 + n_name + n_extra]
        zip64 = False
        while extra:
            tag, size = struct.unpack("<HH", extra[:4])
            if tag == 1:
                zip64 = True
                fields = list(struct.unpack("<%dQ" % (size // 8), extra[4:4 + size]))
                if usize == 0xFFFFFFFF:
                    usize = fields.pop(0)
                if csize == 0xFFFFFFFF:
                    csize = fields.pop(0)
                if offset == 0xFFFFFFFF:
                    offset = fields.pop(0)
            extra = extra[4 + size:]
        lsig, _, _, lmethod, _, _, lcrc, _, _, ln_name, ln_extra = struct.unpack("<IHHHHHIIIHH", data[offset:offset + 30])
        assert lsig == 0x04034B50 and lmethod == method and lcrc == crc
        assert data[offset + 30:offset + 30 + ln_name].decode() == name
        members.append((name, method, crc, csize, usize, offset, zip64))
        at += 46 + n_name + n_extra + n_comment
    assert at == cd_offset + cd_size
    return {"members": members, "zip64_end": zip64_end, "entries": n_total}


# ---- inputs: integer formulas only -------------------------------------------------------------------------------------------
def _hash(seed: int, n: int) -> np.ndarray:
    """n uint32 of a multiply-xorshift hash of (seed, index)."""
    x = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B9) + np.uint64(1)) & np.uint64(0xFFFFFFFF)
    for mul in (0x7FEB352D, 0x846CA68B):
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(mul)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def noise_bytes(n: int, seed: int) -> np.ndarray:
    return (_hash(seed, n) >> np.uint32(24)).astype(np.uint8)


def flow_field(height: int, width: int, seed: int, dtype=np.float32) -> np.ndarray:
    """A smooth flow plus noise, (H, W, 2): multiples of 1/8 that vary slowly, plus twelve hashed bits below 1/2."""
    y, x = np.mgrid[0:height, 0:width].astype(np.int64)
    smooth = np.stack([((3 * x + 5 * y) // 7) % 97 - 48, ((2 * y - x) // 5) % 61 - 30], axis=2).astype(np.float64) / 8
    noise = (_hash(seed, height * width * 2) >> np.uint32(20)).astype(np.float64).reshape(height, width, 2) / 8192 - 0.25
    return (smooth + noise).astype(dtype)


def stretch_bytes(lengths, distance: int, seed: int) -> np.ndarray:
    """For every n: `distance` bytes that each differ from the byte `distance` before, n bytes that equal it, and one
    that differs again -- a stretch of exactly n."""
    out = [int(v) for v in noise_bytes(distance, seed)]
    h = [int(v) for v in _hash(seed + 1, (distance + 1) * (len(lengths) + 1))]
    for n in lengths:
        for _ in range(distance):
            out.append((out[-distance] + 1 + h.pop() % 254) & 0xFF)
        for _ in range(n):
            out.append(out[-distance])
        out.append((out[-distance] + 1 + h.pop() % 254) & 0xFF)
    return np.array(out, np.uint8)


def fibonacci_bytes(symbols: int) -> np.ndarray:
    """Byte v occurs L(v + 1) times -- the Lucas numbers 1, 3, 4, 7, 11 ..., Fibonacci's rule without its ties -- in an
    order that steps through the sorted bytes by the golden ratio so that no byte equals its predecessor: the optimal
    code for these counts and one end-of-block is a chain, deeper than 15 bits from 16 symbols on."""
    fib = [1, 3]
    while len(fib) < symbols:
        fib.append(fib[-1] + fib[-2])
    values = np.repeat(np.arange(symbols, dtype=np.uint8), fib)
    n = len(values)
    step = n * 6180339887 // 10000000000
    while np.gcd(step, n) != 1:
        step += 1
    return values[(np.arange(n, dtype=np.int64) * step) % n]


def sweep_bytes(lengths, distance: int, seed: int) -> np.ndarray:
    """For every n of `lengths` and every phase p of 0 .. 63: bytes that each differ from the byte `distance` before
    until the position is p (mod 64), n bytes that equal it, and one that differs -- a stretch of exactly n that starts
    at every place of a trip.  Sixteen byte values, so that a band of nothing but padding is still coded, not stored."""
    out = [int(v) & 15 for v in noise_bytes(distance, seed)]
    h = _hash(seed + 1, len(lengths) * TRIP * (TRIP + 1))
    k = 0
    for n in lengths:
        for p in range(TRIP):
            while len(out) % TRIP != p:
                out.append((out[-distance] + 1 + int(h[k]) % 15) & 15)
                k += 1
            out.extend((out[-distance:] * (n // distance + 1))[:n])
            out.append((out[-distance] + 1 + int(h[k]) % 15) & 15)
            k += 1
    return np.array(out, np.uint8)


def band_end_bytes(length: int, n: int, gap: int, distance: int, seed: int) -> np.ndarray:
    """`length` bytes of four values: bytes that differ from the byte `distance` before, then a stretch of n (none for
    n = 0) that ends `gap` bytes before the last one."""
    assert length - n - gap >= (distance if n else 0)
    out = [int(v) & 3 for v in noise_bytes(distance, seed)][:length]
    h = [int(v) % 3 for v in _hash(seed + 1, length)]
    while len(out) < length - n - gap:
        out.append((out[-distance] + 1 + h.pop()) & 3)
    out.extend((out[-distance:] * (n // distance + 1))[:n])
    while len(out) < length:
        out.append((out[-distance] + 1 + h.pop()) & 3)
    return np.array(out, np.uint8)


BAND_END_STRETCHES = (1, 2, 3, 258, 259)


def band_ends_bytes(band_bytes: int, last: int, last_n: int, last_gap: int, distance: int, seed: int) -> np.ndarray:
    """Bands of exactly `band_bytes`: for each n of BAND_END_STRETCHES one whose stretch of n ends at its last byte, one
    whose stretch ends a byte before, and one without a stretch; then a last band of `last` bytes whose stretch of
    `last_n` ends `last_gap` bytes before its end."""
    bands = [band_end_bytes(band_bytes, n, gap, distance, seed + 10 * i + gap)
             for gap in (0, 1) for i, n in enumerate(BAND_END_STRETCHES)]
    bands.append(band_end_bytes(band_bytes, 0, 0, distance, seed + 100))
    bands.append(band_end_bytes(last, last_n, last_gap, distance, seed + 101))
    return np.concatenate(bands)


def equal_counts_bytes(times: int) -> np.ndarray:
    """The 256 byte values `times` times each, in an order in which no byte equals its predecessor: every merge of the
    code's construction is between equal weights."""
    return np.tile(((np.arange(256) * 167 + 13) % 256).astype(np.uint8), times)


def periodic_bytes(n: int, period: int, seed: int) -> np.ndarray:
    """`period` hashed bytes repeated: with that distance every band is one long stretch behind its first bytes."""
    return np.resize(noise_bytes(period, seed), n)


def npy_prefix(array: np.ndarray) -> bytes:
    buf = io.BytesIO()
    np.save(buf, array)
    raw = buf.getvalue()
    return raw[:len(raw) - array.nbytes]


EDGES = (2, 3, 258, 259, 260, 261, 516)
SWEEP = (1, 2, 3, 4, 257, 258, 259, 260, 261, 515, 516, 517, 518, 774)
SWEEP_DISTANCES = (1, 2, 3, 16, 63, 64)
LAST_BAND = {"end": (2, 0), "before": (3, 1), "none": (0, 0)}          # the last band's stretch and the bytes behind it
SWEEP_BAND = 5007 * 64                 # a multiple of 64 that holds a whole sweep: its phases are the band's
FIBONACCI_DEEP = 20                    # the smallest fibonacci_bytes whose code, in one band, is halved three times

_sweeps = {}


def _sweep(distance: int) -> np.ndarray:
    """sweep_bytes(SWEEP, distance, 50 + distance): made once, never written to."""
    if distance not in _sweeps:
        _sweeps[distance] = sweep_bytes(SWEEP, distance, 50 + distance)
        _sweeps[distance].setflags(write=False)
    return _sweeps[distance]


def every_distance(distance: int) -> np.ndarray:
    """The EDGES stretches at this distance: a few KB, one band of EVERY_DISTANCE_BAND."""
    return stretch_bytes(EDGES, distance, 100 + distance)


EVERY_DISTANCE_BAND = 4096

# name: (the array's maker, band_bytes, distance, whether the stream is numpy.save's bytes or the array's alone)
CASES = {
    "f32_7x9_b64_d1": (lambda: flow_field(7, 9, 1), 64, 1, True),
    "f32_24x40_b1024_d1": (lambda: flow_field(24, 40, 2), 1024, 1, True),
    "f64_7x9_b128_d16": (lambda: flow_field(7, 9, 3, np.float64), 128, 16, True),
    "f64_24x40_b4096_d16": (lambda: flow_field(24, 40, 4, np.float64), 4096, 16, True),
    "i64_33x31_b256_d16": (lambda: round_i64(flow_field(33, 31, 5)), 256, 16, True),
    "i64_33x31_b1024_d8": (lambda: round_i64(flow_field(33, 31, 5)), 1024, 8, True),
    "i64_64x256_b256_d16": (lambda: round_i64(flow_field(64, 256, 6)), 256, 16, True),       # 1025 coded bands
    "f32_128x256_b8192_d1": (lambda: flow_field(128, 256, 7), 8192, 1, True),
    "edges_d1": (lambda: stretch_bytes(EDGES, 1, 8), 65536, 1, True),                        # one band
    "edges_d8_b384": (lambda: stretch_bytes(EDGES, 8, 9), 384, 8, True),
    "edges_d16": (lambda: stretch_bytes(EDGES, 16, 10), 2048, 16, True),
    "edges_d64": (lambda: stretch_bytes(EDGES, 64, 11), 4096, 64, True),
    "periodic_d16_b320": (lambda: periodic_bytes(3000, 16, 12), 320, 16, True),              # bands cut one long stretch
    "fibonacci": (lambda: fibonacci_bytes(16), 4096, 1, False),                              # the length-15 repair
    "noise_beside_zeros": (lambda: np.concatenate([np.zeros(4096 - 128, np.uint8), noise_bytes(4096, 14),
                                                   np.zeros(4096, np.uint8)]), 4096, 1, True),  # coded, stored, coded
    "noise_tail_1": (lambda: noise_bytes(2 * 512 + 1 - 128, 15), 512, 1, True),                    # a last band of one byte
    "stored_block_split": (lambda: noise_bytes(70000, 16), 65536 * 2, 1, True),              # two stored blocks in a band
    "one_byte_b64": (lambda: np.array([7], np.uint8), 64, 1, False),                         # one band, two symbols
    "empty_npy_b64": (lambda: np.zeros(0, np.uint8), 64, 1, True),                           # two bands, both stored
    "noise_1025_bands_b64": (lambda: noise_bytes(1025 * 64 - 128 - 9, 17), 64, 1, True),
    "zeros_2049_bands_b64": (lambda: np.zeros(2049 * 64 - 128, np.uint8), 64, 1, True),
    # every stretch length of SWEEP at every place of a trip, in one band and in bands that cut the stretches
    **{f"sweep_d{d}": ((lambda d=d: _sweep(d)), SWEEP_BAND, d, False) for d in SWEEP_DISTANCES},
    **{f"sweep_d{d}_b4096": ((lambda d=d: _sweep(d)), 4096, d, False) for d in SWEEP_DISTANCES},
    # bands of 64 (mod 256) and of 0 (mod 256) bytes that end in a stretch, a byte behind one, or in none
    **{f"ends_b320_last64_{v}": ((lambda n=n, g=g: band_ends_bytes(320, 64, n, g, 1, 30)), 320, 1, False)
       for v, (n, g) in LAST_BAND.items()},
    **{f"ends_b512_last256_{v}": ((lambda n=n, g=g: band_ends_bytes(512, 256, n, g, 16, 40)), 512, 16, False)
       for v, (n, g) in LAST_BAND.items()},
    "fibonacci_deep": (lambda: fibonacci_bytes(FIBONACCI_DEEP), 65536, 1, False),            # three repairs
    "equal_counts": (lambda: equal_counts_bytes(16), 4096, 1, False),                        # every merge a tie
}


def case(name: str):
    """(prefix, the array, band_bytes, distance)."""
    maker, band_bytes, distance, npy = CASES[name]
    array = np.ascontiguousarray(maker())
    return (npy_prefix(array) if npy else b""), array, band_bytes, distance
