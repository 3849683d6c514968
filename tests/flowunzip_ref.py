"""The band inflater of transflow_amd/csrc/flowunzip.hip restated in plain Python (DESIGN.md section 18 has the rules).

A band is a byte range of a raw deflate stream that must inflate, on its own, to exactly `out_bytes` bytes: RFC 1951
blocks with BFINAL 0 -- stored, fixed, dynamic -- whose matches stay inside the band's own output and whose last block
ends on the range's last bit.  `inflate_band` returns the bytes or the name of the rejection, and a trace of what the
band reached.  `full_flush_stream` makes such bands with zlib (Z_FULL_FLUSH after every band); `BitWriter` and the
`hand_*` / `MALFORMED` makers build what zlib never emits.  `IndexedRefEncoder` is flowzip_ref.RefEncoder with the
`last_band_sizes` an indexing archive writer asks for; `index_field` / `parse_index` restate the archive's extra field.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

from tests import flowzip_ref as R

# the rejections, numbered as transflow_amd/csrc/flowunzip_common.h numbers them
REJECTS = ("ok", "bfinal", "btype", "stored_len", "bad_code", "repeat_first", "repeat_past", "bad_symbol", "distance",
           "overrun", "short", "exhausted")
REJECT_NUMBER = {name: k for k, name in enumerate(REJECTS)}

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
            6145, 8193, 12289, 16385, 24577]
DST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
INDEX_ID = 0x4654


class Rejected(Exception):
    pass


class BandTrace:
    def __init__(self):
        self.block_types = []               # per block: 0 stored, 1 fixed, 2 dynamic
        self.repeat_codes = set()           # of 16, 17, 18
        self.max_distance = 0
        self.overlapping = 0                # matches with distance < length
        self.match_at_start_distance = 0    # matches whose distance is every byte the band has produced
        self.max_code_length = 0
        self.single_distance_code = 0       # dynamic blocks whose distance code has one symbol
        self.longest_match = 0

    @property
    def coded_blocks(self):
        return sum(1 for t in self.block_types if t)

    @property
    def stored_blocks(self):
        return sum(1 for t in self.block_types if t == 0)


class _Code:
    """A canonical code: {(length, code): symbol}; `left` as puff counts it (0 complete, > 0 incomplete, < 0 over)."""

    def __init__(self, lengths):
        self.count = [0] * 16
        for n in lengths:
            self.count[n] += 1
        self.n = len(lengths)
        self.empty = self.count[0] == self.n
        self.left = 0
        self.table = {}
        if self.empty:
            return
        left = 1
        for bits in range(1, 16):
            left = (left << 1) - self.count[bits]
            if left < 0:
                self.left = left
                return
        self.left = left
        codes = R.canonical_codes(list(lengths))
        self.table = {(n, c): s for s, (n, c) in enumerate(zip(lengths, codes)) if n}
        self.longest = max(lengths)


class _Bits:
    def __init__(self, data: bytes):
        self.data, self.at, self.total = data, 0, 8 * len(data)

    def take(self, n: int) -> int:
        if self.total - self.at < n:
            raise Rejected("exhausted")
        p = self.at >> 3
        v = (int.from_bytes(self.data[p:p + 4], "little") >> (self.at & 7)) & ((1 << n) - 1)
        self.at += n
        return v

    def symbol(self, code: _Code) -> int:
        """Bit by bit, the first bit the code's most significant: exhausted where the range ends inside the code, bad_code
        after 15 bits that are no code."""
        p = self.at >> 3
        bits = int.from_bytes(self.data[p:p + 4], "little") >> (self.at & 7)
        left = self.total - self.at
        c = 0
        table = code.table
        for n in range(1, 16):
            if n > left:
                raise Rejected("exhausted")
            c = (c << 1) | (bits & 1)
            bits >>= 1
            s = table.get((n, c))
            if s is not None:
                self.at += n
                return s
        raise Rejected("bad_code")


def _dynamic(b: _Bits, trace: BandTrace):
    v = b.take(14)
    nlen, ndist, ncode = (v & 31) + 257, ((v >> 5) & 31) + 1, (v >> 10) + 4
    if nlen > 286 or ndist > 30:
        raise Rejected("bad_symbol")
    cl = [0] * 19
    for i in range(ncode):
        cl[CL_ORDER[i]] = b.take(3)
    clc = _Code(cl)
    if clc.empty or clc.left != 0:
        raise Rejected("bad_code")
    lengths = []
    total = nlen + ndist
    while len(lengths) < total:
        s = b.symbol(clc)
        if s < 16:
            lengths.append(s)
            continue
        trace.repeat_codes.add(s)
        if s == 16:
            if not lengths:
                raise Rejected("repeat_first")
            value, repeat = lengths[-1], 3 + b.take(2)
        elif s == 17:
            value, repeat = 0, 3 + b.take(3)
        else:
            value, repeat = 0, 11 + b.take(7)
        if len(lengths) + repeat > total:
            raise Rejected("repeat_past")
        lengths += [value] * repeat
    if lengths[256] == 0:
        raise Rejected("bad_code")
    dist = _Code(lengths[nlen:])
    if dist.left < 0 or (dist.left > 0 and not (dist.count[1] == 1 and dist.count[0] == ndist - 1)):
        raise Rejected("bad_code")
    lit = _Code(lengths[:nlen])
    if lit.left != 0:
        raise Rejected("bad_code")
    trace.max_code_length = max(trace.max_code_length, max(lengths))
    if dist.count[1] == 1 and dist.count[0] == ndist - 1:
        trace.single_distance_code += 1
    return lit, dist


_FIXED = None


def inflate_band(stream: bytes, first: int, size: int, out_bytes: int):
    """(the band's bytes or None, the rejection's name or None, BandTrace) for bytes [first, first + size) of `stream`."""
    global _FIXED
    b = _Bits(bytes(stream[first:first + size]))
    out = bytearray()
    trace = BandTrace()
    try:
        while b.at != b.total:
            v = b.take(3)
            if v & 1:
                raise Rejected("bfinal")
            kind = v >> 1
            if kind == 3:
                raise Rejected("btype")
            trace.block_types.append(kind)
            if kind == 0:
                b.at = (b.at + 7) & ~7
                n, inv = b.take(16), b.take(16)
                if n != (~inv & 0xFFFF):
                    raise Rejected("stored_len")
                src = b.at >> 3
                if n > size - src:
                    raise Rejected("exhausted")
                if n > out_bytes - len(out):
                    raise Rejected("overrun")
                out += b.data[src:src + n]
                b.at += 8 * n
                continue
            if kind == 1:
                if _FIXED is None:
                    _FIXED = (_Code(FIXED_LITLEN), _Code(FIXED_DIST))
                lit, dist = _FIXED
            else:
                lit, dist = _dynamic(b, trace)
            while True:
                s = b.symbol(lit)
                if s < 256:
                    if len(out) >= out_bytes:
                        raise Rejected("overrun")
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s >= 286:
                    raise Rejected("bad_symbol")
                n = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
                s = b.symbol(dist)
                if s >= 30:
                    raise Rejected("bad_symbol")
                d = DST_BASE[s] + b.take(DST_EXTRA[s])
                if d > len(out):
                    raise Rejected("distance")
                if n > out_bytes - len(out):
                    raise Rejected("overrun")
                trace.max_distance = max(trace.max_distance, d)
                trace.longest_match = max(trace.longest_match, n)
                trace.overlapping += d < n
                trace.match_at_start_distance += d == len(out)
                if d >= n:
                    out += out[len(out) - d:len(out) - d + n]
                else:
                    piece = bytes(out[-d:])
                    out += (piece * (n // d + 1))[:n]
        if len(out) != out_bytes:
            raise Rejected("short")
    except Rejected as e:
        return None, str(e), trace
    return bytes(out), None, trace


def offsets_of(sizes) -> list:
    out = [0]
    for n in sizes:
        out.append(out[-1] + int(n))
    return out


def inflate_member(stream: bytes, sizes, band_bytes: int, usize: int):
    """(S or None, the first rejected band or None, its reason, [BandTrace])."""
    at, out, traces = 0, [], []
    for band, n in enumerate(sizes):
        want = min(band_bytes, usize - band * band_bytes)
        data, reason, trace = inflate_band(stream, at, int(n), want)
        traces.append(trace)
        if data is None:
            return None, band, reason, traces
        out.append(data)
        at += int(n)
    return b"".join(out), None, None, traces


def tail_ok(tail: bytes) -> bool:
    """What the host asks of the bytes behind the last band: a final block that holds nothing."""
    d = zlib.decompressobj(-15)
    try:
        return d.decompress(bytes(tail)) == b"" and d.eof and d.unused_data == b""
    except zlib.error:
        return False


def zlib_accepts(band: bytes, out_bytes: int):
    """The band's bytes if zlib inflates it to out_bytes bytes, sees no final block in it and finds the stream, behind
    it, at a block boundary on a byte boundary (an empty final block parses there); else None."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(band))
        if d.eof or len(out) != out_bytes:
            return None
        more = d.decompress(b"\x01\x00\x00\xff\xff")
    except zlib.error:
        return None
    return out if (d.eof and more == b"" and d.unused_data == b"") else None


# ---- bands made by zlib ----------------------------------------------------------------------------------------------------
def full_flush_stream(data: bytes, band_bytes: int, level: int, strategy: int):
    """(stream, band sizes, tail): every band compressed and then flushed with Z_FULL_FLUSH -- to a byte boundary, behind an
    empty stored block, the dictionary forgotten -- and the final block zlib ends with."""
    data = bytes(data)
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    pieces = []
    for first in range(0, len(data), band_bytes):
        pieces.append(c.compress(data[first:first + band_bytes]) + c.flush(zlib.Z_FULL_FLUSH))
    tail = c.flush(zlib.Z_FINISH)
    return b"".join(pieces) + tail, [len(p) for p in pieces], tail


LEVELS = (0, 1, 6, 9)
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE}
BANDS = (64, 1024, 4096, 65536)
_data = {}


def matrix_data(name: str) -> bytes:
    """The full-flush matrix's inputs, made once."""
    if name not in _data:
        makers = {
            "flow_f32": lambda: _npy(R.flow_field(33, 31, 21)),
            "flow_i64": lambda: _npy(R.round_i64(R.flow_field(33, 31, 21))),
            "zeros": lambda: bytes(70000),
            "noise": lambda: R.noise_bytes(70000, 22).tobytes(),
            "periodic": lambda: R.periodic_bytes(70000, 32000, 23).tobytes(),
        }
        _data[name] = makers[name]()
    return _data[name]


DATA = ("flow_f32", "flow_i64", "zeros", "noise", "periodic")


def _npy(array: np.ndarray) -> bytes:
    return R.npy_prefix(array) + np.ascontiguousarray(array).tobytes()


# ---- bands made by hand ------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, value: int, n: int):
        """n bits, the value's least significant first (header fields, extra bits)."""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        return self

    def code(self, code: int, n: int):
        """A Huffman code of n bits, its most significant bit first."""
        for i in range(n - 1, -1, -1):
            self.bits((code >> i) & 1, 1)
        return self

    def align(self):
        self.n = (self.n + 7) & ~7
        return self

    def raw(self, data: bytes):
        assert self.n % 8 == 0
        for v in data:
            self.bits(v, 8)
        return self

    def end_band(self):
        """The empty stored block that brings a band to a byte boundary."""
        return self.bits(0, 3).align().raw(b"\x00\x00\xff\xff")

    def bytes(self) -> bytes:
        return self.acc.to_bytes((self.n + 7) // 8, "little")


_FIXED_CODES = R.canonical_codes(FIXED_LITLEN)


def fixed_symbol(w: BitWriter, sym: int):
    return w.code(_FIXED_CODES[sym], FIXED_LITLEN[sym])


def fixed_match(w: BitWriter, length: int, distance: int, length_symbol=None, distance_symbol=None):
    k = max(i for i in range(29) if LEN_BASE[i] <= length) if length != 258 else 28
    fixed_symbol(w, 257 + k if length_symbol is None else length_symbol)
    w.bits(length - LEN_BASE[k], LEN_EXTRA[k])
    j = max(i for i in range(30) if DST_BASE[i] <= distance)
    w.code(j if distance_symbol is None else distance_symbol, 5)
    return w.bits(distance - DST_BASE[j], DST_EXTRA[j])


def fixed_block(w: BitWriter, tokens, final: int = 0, end: bool = True):
    """tokens: ints (literals) and (length, distance) pairs."""
    w.bits(final, 1).bits(1, 2)
    for t in tokens:
        if isinstance(t, tuple):
            fixed_match(w, *t)
        else:
            fixed_symbol(w, t)
    if end:
        fixed_symbol(w, 256)
    return w


def dynamic_header(w: BitWriter, nlen: int, ndist: int, cl_lengths, symbols, final: int = 0):
    """A dynamic block's header: the code-length code's 19 lengths, then `symbols`: (symbol, extra value) pairs coded with
    it (extra bits: 2 / 3 / 7 for 16 / 17 / 18, none below)."""
    w.bits(final, 1).bits(2, 2).bits(nlen - 257, 5).bits(ndist - 1, 5)
    ncode = max(4, max(i for i in range(19) if cl_lengths[CL_ORDER[i]]) + 1)
    w.bits(ncode - 4, 4)
    for i in range(ncode):
        w.bits(cl_lengths[CL_ORDER[i]], 3)
    codes = R.canonical_codes(list(cl_lengths))
    for sym, extra in symbols:
        w.code(codes[sym], cl_lengths[sym])
        w.bits(extra, {16: 2, 17: 3, 18: 7}.get(sym, 0))
    return w


def plain_dynamic_header(w: BitWriter, litlen, dist):
    """The header for these lengths, every length coded by itself with a 4-bit code (no repeat codes)."""
    cl = [4] * 16 + [0] * 3
    return dynamic_header(w, len(litlen), len(dist), cl, [(n, 0) for n in list(litlen) + list(dist)])


def _literals(n: int, seed: int) -> list:
    return [int(v) for v in R.noise_bytes(n, seed)]


def _expand(tokens) -> bytes:
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out)


def _one_band(tokens):
    return fixed_block(BitWriter(), tokens).end_band().bytes(), _expand(tokens)


_made = {}


def hand_valid() -> dict:
    """name -> (stream, band sizes, band_bytes, S): members zlib never emits.  Made once."""
    if "valid" not in _made:
        _made["valid"] = _hand_valid()
    return _made["valid"]


def _hand_valid() -> dict:
    out = {}
    # a match at distance exactly 32768, which is also every byte the band has produced
    tokens = _literals(32768, 31) + [(10, 32768), 5, (258, 32768), (7, 32000)]
    band, S = _one_band(tokens)
    out["distance_32768"] = (band, [len(band)], 65536, S)
    # a match whose distance equals the bytes produced so far, in a second band (what lies before is another band's)
    a, Sa = _one_band(_literals(64, 32))
    b, Sb = _one_band(_literals(5, 33) + [(5, 5), 9, (11, 11), (30, 3)])
    out["distance_is_produced"] = (a + b, [len(a), len(b)], 64, Sa + Sb)
    # a match of 258 at distance 1 right after the first literal; a band of one byte behind it
    a, Sa = _one_band([77, (258, 1), (258, 1), (258, 1), (249, 1)])
    b, Sb = _one_band([3])
    out["run_258_d1"] = (a + b, [len(a), len(b)], 1024, Sa + Sb)
    # a dynamic block whose distance code has one symbol (of one bit), a two-symbol-plus-end literal code
    litlen = [0] * 257
    litlen[65], litlen[66], litlen[256] = 1, 2, 3
    litlen += [0] * 7 + [3]                  # 264: a match of 10
    w = plain_dynamic_header(BitWriter(), litlen, [0, 0, 1])       # distance symbol 2: distance 3
    codes = R.canonical_codes(litlen)
    S = bytearray()
    for sym in (65, 66, 65, 264, 66, 264, 256):
        w.code(codes[sym], litlen[sym])
        if sym == 264:
            w.bits(0, 1)                     # the distance code's only code, 0
            for _ in range(10):
                S.append(S[-3])
        elif sym < 256:
            S.append(sym)
    band = w.end_band().bytes()
    out["single_distance_code"] = (band, [len(band)], 64, bytes(S))
    # two fixed blocks and a stored one in a band; the second block's matches reach into the first's bytes
    w = fixed_block(BitWriter(), _literals(40, 34))
    fixed_block(w, [(20, 40), (3, 1)])
    w.bits(0, 3).align().raw(struct.pack("<HH", 7, 7 ^ 0xFFFF) + bytes(range(7)))
    S = _expand(_literals(40, 34) + [(20, 40), (3, 1)]) + bytes(range(7))
    band = w.end_band().bytes()
    out["three_blocks"] = (band, [len(band)], 128, S)
    # fixed, fixed, dynamic, fixed, an empty fixed block, fixed: a decoder that keeps its fixed tables between fixed blocks
    # has to notice that a dynamic block took them
    first, second, third = _literals(20, 35), _literals(9, 36) + [(12, 25)], _literals(15, 37) + [(30, 50)]
    w = fixed_block(fixed_block(BitWriter(), first), second)
    plain_dynamic_header(w, litlen, [0, 0, 1])
    middle = bytearray()
    for sym in (66, 65, 65, 264, 256):
        w.code(codes[sym], litlen[sym])
        if sym == 264:
            w.bits(0, 1)
            middle += bytes(10)                  # placeholders: the bytes are copied below, from the member so far
        elif sym < 256:
            middle.append(sym)
    S = bytearray(_expand(first + second)) + middle[:3]
    for _ in range(10):
        S.append(S[-3])
    fixed_block(w, third)
    fixed_block(w, [])
    fixed_block(w, [200, 201])
    for t in third + [200, 201]:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                S.append(S[-t[1]])
        else:
            S.append(t)
    band = w.end_band().bytes()
    out["fixed_dynamic_fixed"] = (band, [len(band)], 128, bytes(S))
    return out


def _bad_member(bad: bytes, want: int = 64):
    """A member of three bands of 64 bytes, the middle one `bad`: (stream, sizes, band_bytes, usize, the bad band)."""
    a, _ = _one_band(_literals(64, 41))
    c, _ = _one_band(_literals(want, 42))
    return a + bad + c, [len(a), len(bad), len(c)], 64, 128 + want, 1


def malformed() -> dict:
    """name -> ((stream, band sizes, band_bytes, usize, the first bad band), the reason): at least one per rejection.
    Made once."""
    if "malformed" not in _made:
        _made["malformed"] = _malformed()
    return _made["malformed"]


def _malformed() -> dict:
    lits = _literals(64, 43)
    out = {}

    def add(name, reason, band):
        out[name] = (_bad_member(band), reason)

    add("bfinal_fixed", "bfinal", fixed_block(BitWriter(), lits, final=1).bytes())
    add("bfinal_stored_tail", "bfinal", fixed_block(BitWriter(), lits).bits(1, 3).align().raw(b"\x00\x00\xff\xff").bytes())
    add("btype_3", "btype", BitWriter().bits(0, 1).bits(3, 2).align().raw(bytes(70)).bytes())
    add("stored_len", "stored_len", BitWriter().bits(0, 3).align().raw(struct.pack("<HH", 64, 64) + bytes(lits)).end_band().bytes())
    over = [0] * 257
    over[0], over[1], over[256] = 1, 1, 1
    add("oversubscribed", "bad_code", plain_dynamic_header(BitWriter(), over, [1, 1]).align().raw(bytes(20)).bytes())
    inc = [0] * 257
    inc[0], inc[256] = 1, 2
    add("incomplete_literals", "bad_code", plain_dynamic_header(BitWriter(), inc, [1, 1]).align().raw(bytes(20)).bytes())
    good = [0] * 257
    good[0], good[256] = 1, 1
    add("incomplete_distances", "bad_code", plain_dynamic_header(BitWriter(), good, [2, 2]).align().raw(bytes(20)).bytes())
    add("incomplete_code_lengths", "bad_code",
        dynamic_header(BitWriter(), 257, 1, [0] * 18 + [1], []).align().raw(bytes(20)).bytes())
    no_end = [0] * 257
    no_end[0], no_end[1] = 1, 1
    add("no_end_of_block", "bad_code", plain_dynamic_header(BitWriter(), no_end, [1, 1]).align().raw(bytes(20)).bytes())
    cl = [0] * 19
    cl[16], cl[0], cl[1] = 1, 2, 2
    add("repeat_16_first", "repeat_first", dynamic_header(BitWriter(), 257, 1, cl, [(16, 0)]).align().raw(bytes(20)).bytes())
    cl = [0] * 19
    cl[18], cl[0], cl[1] = 1, 2, 2
    add("repeat_18_past", "repeat_past",
        dynamic_header(BitWriter(), 257, 1, cl, [(18, 127), (18, 127)]).align().raw(bytes(20)).bytes())
    cl = [0] * 19
    cl[16], cl[17], cl[1] = 1, 2, 2
    add("repeat_16_past", "repeat_past",
        dynamic_header(BitWriter(), 257, 1, cl, [(1, 0)] + [(16, 3)] * 42 + [(16, 3)]).align().raw(bytes(20)).bytes())
    add("too_many_lengths", "bad_symbol", BitWriter().bits(0, 1).bits(2, 2).bits(30, 5).bits(0, 5).bits(0, 4).align()
        .raw(bytes(20)).bytes())
    add("literal_286", "bad_symbol", fixed_symbol(fixed_block(BitWriter(), lits[:10], end=False), 286).align().raw(bytes(8)).bytes())
    add("literal_287", "bad_symbol", fixed_symbol(fixed_block(BitWriter(), lits[:10], end=False), 287).align().raw(bytes(8)).bytes())
    w = fixed_block(BitWriter(), lits[:40], end=False)
    add("distance_30", "bad_symbol", fixed_match(w, 3, 1, distance_symbol=30).align().raw(bytes(8)).bytes())
    w = fixed_block(BitWriter(), lits[:40], end=False)
    add("distance_31", "bad_symbol", fixed_match(w, 3, 1, distance_symbol=31).align().raw(bytes(8)).bytes())
    # the bad access would point before the band's first output byte: into the band before it
    add("distance_before_band", "distance", fixed_block(BitWriter(), [lits[0], (63, 2)]).end_band().bytes())
    add("distance_first_token", "distance", fixed_block(BitWriter(), [(64, 1)]).end_band().bytes())
    add("distance_32768_of_40", "distance", fixed_block(BitWriter(), lits[:40] + [(24, 32768)]).end_band().bytes())
    add("overrun_literal", "overrun", fixed_block(BitWriter(), lits + [1]).end_band().bytes())
    add("overrun_match", "overrun", fixed_block(BitWriter(), lits[:60] + [(5, 1)]).end_band().bytes())
    add("overrun_match_258", "overrun", fixed_block(BitWriter(), lits[:63] + [(258, 63)]).end_band().bytes())
    add("overrun_stored", "overrun",
        BitWriter().bits(0, 3).align().raw(struct.pack("<HH", 65, 65 ^ 0xFFFF) + bytes(lits) + b"\x01").end_band().bytes())
    add("short", "short", fixed_block(BitWriter(), lits[:63]).end_band().bytes())
    add("short_empty", "short", BitWriter().end_band().bytes())
    out["short_no_bytes"] = (_bad_member(b""), "short")
    # the range ends inside a block: the decoder's next access would be past the band's last compressed byte, where the
    # next band's bytes lie
    whole = fixed_block(BitWriter(), lits).end_band().bytes()
    add("exhausted_in_literals", "exhausted", whole[:40])
    add("exhausted_no_end_block", "exhausted", fixed_block(BitWriter(), lits).bytes())
    add("exhausted_in_stored_header", "exhausted", whole[:-2])
    add("exhausted_stored_bytes", "exhausted",
        BitWriter().bits(0, 3).align().raw(struct.pack("<HH", 64, 64 ^ 0xFFFF) + bytes(lits[:50])).bytes())
    add("exhausted_in_dynamic_header", "exhausted", plain_dynamic_header(BitWriter(), good, [1, 1]).bytes()[:60])
    # a bad last band, and a bad first band
    a, _ = _one_band(_literals(64, 44))
    b = fixed_block(BitWriter(), [9, (2 + 3, 2)]).end_band().bytes()
    out["distance_last_band_of_6"] = ((a + b, [len(a), len(b)], 64, 70, 1), "distance")
    c, _ = _one_band(_literals(64, 45))
    bad = fixed_block(BitWriter(), lits[:63]).end_band().bytes()
    out["short_first_band"] = ((bad + c, [len(bad), len(c)], 64, 128, 0), "short")
    return out


def corpus_lines(cases) -> list:
    """The host check program's input: `name out_bytes hex` per band of every member of `cases` (name -> (stream, sizes,
    band_bytes, usize))."""
    lines = []
    for name, (stream, sizes, band_bytes, usize) in cases.items():
        offs = offsets_of(sizes)
        for band, n in enumerate(sizes):
            want = min(band_bytes, usize - band * band_bytes)
            piece = bytes(stream[offs[band]:offs[band] + n])
            lines.append("%s/%d %d %s" % (name, band, want, piece.hex() or "-"))
    return lines


# ---- the archive's band index ------------------------------------------------------------------------------------------------
def index_field(prefix_len: int, band_bytes: int, sizes) -> bytes:
    """The extra field: header ID 0x4654, then version 1, flags 0, prefix_len, band_bytes, one size per band."""
    payload = struct.pack("<BBHI", 1, 0, prefix_len, band_bytes) + b"".join(struct.pack("<I", int(n)) for n in sizes)
    return struct.pack("<HH", INDEX_ID, len(payload)) + payload


def parse_index(extra: bytes, usize: int):
    """(prefix_len, band_bytes, [sizes]) from a central-directory entry's extra fields, or None."""
    extra = bytes(extra)
    while len(extra) >= 4:
        tag, size = struct.unpack("<HH", extra[:4])
        body = extra[4:4 + size]
        extra = extra[4 + size:]
        if tag != INDEX_ID or len(body) < 8:
            continue
        version, _flags, prefix_len, band_bytes = struct.unpack("<BBHI", body[:8])
        if version != 1 or band_bytes == 0 or len(body) != 8 + 4 * -(-usize // band_bytes):
            return None
        return prefix_len, band_bytes, list(struct.unpack("<%dI" % ((len(body) - 8) // 4), body[8:]))
    return None


class StoredEncoder:
    """An encoder that stores every band (one stored block each, band_bytes <= 65535): quick members of many bands."""

    def __init__(self, band_bytes: int = 64):
        assert band_bytes <= R.STORED_MAX
        self.band_bytes = band_bytes
        self._sizes = None

    def encode_host(self, prefix: bytes, array: np.ndarray, distance: int):
        S = bytes(prefix) + array.tobytes()
        pieces = []
        for first in range(0, len(S), self.band_bytes):
            piece = S[first:first + self.band_bytes]
            pieces.append(struct.pack("<BHH", 0, len(piece), len(piece) ^ 0xFFFF) + piece)
        self._sizes = [len(p) for p in pieces]
        return b"".join(pieces) + b"\x01\x00\x00\xff\xff", zlib.crc32(S)

    def last_band_sizes(self) -> list:
        return list(self._sizes)

    def close(self):
        pass


class IndexedRefEncoder(R.RefEncoder):
    """flowzip_ref.RefEncoder that remembers where its bands begin: whole indexed archives without a GPU."""

    def __init__(self, band_bytes: int = 4096):
        R.RefEncoder.__init__(self, band_bytes)
        self._sizes = None

    def encode_host(self, prefix: bytes, array: np.ndarray, distance: int):
        self.calls.append(("host", array.dtype.str, distance))
        t = R.trace(prefix, array.tobytes(), self.band_bytes, distance)
        self._sizes = [b - a for a, b in zip(t.band_offsets[:-1], t.band_offsets[1:])]
        return t.stream, t.crc

    def last_band_sizes(self) -> list:
        if self._sizes is None:
            raise RuntimeError("nothing has been encoded")
        return list(self._sizes)
