"""The banded-PNG decoder of transflow_amd/csrc/pngdec.hip restated in plain Python and numpy (DESIGN.md section 20 has
the rules).

An indexed file is what PngEncoder(index=True) writes: 8-bit RGB, IHDR, the ancillary chunk tfBX (version 1, flags 0, 0,
band_rows, n_bands), an IDAT with a two-byte zlib header, one IDAT per band of `band_rows` rows, an IDAT with an empty
final block and the Adler-32, IEND.  `walk` sorts a file into indexed / not for the device / rejected with the names of
pngdec_common.h; `decode` is the whole decoder -- chunk CRCs, every band inflated alone with tests/flowunzip_ref.py's
machine, the filter types, the Adler-32, the unfilter -- and `Trace` its account of what the rows reached.  `build` makes
indexed files with zlib (Z_FULL_FLUSH at every band's end) and *forced* per-row filter types: the independent oracle on
the way in.  `with_index` puts the index into a file of tests/png_ref.encode.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

from tests import flowunzip_ref as U
from tests import png_ref as P

# the rejections, numbered as transflow_amd/csrc/pngdec_common.h numbers them
REJECT_NUMBER = {"ok": 0, "signature": 1, "truncated": 2, "ihdr": 3, "size": 4, "index": 5, "zlib_header": 6, "tail": 7,
                 "no_iend": 8, "idat_order": 9, "chunk_crc": 10, "adler": 11, "filter_type": 12}
R_BAND = 16
REJECT_NUMBER.update({"band_" + name: R_BAND + k for k, name in enumerate(U.REJECTS) if k})
REJECT_NAME = {v: k for k, v in REJECT_NUMBER.items()}
WHY_NOT = ("indexed", "no_index", "format", "interlaced", "version")
MAX_DIM = (1 << 24) - 1
MAX_STREAM = 1 << 31
MARCH_ROWS = 64                         # the rows the unfilter kernel marches together
RING_BYTES = 32768
INDEX_TYPE = b"tfBX"


class Rejected(Exception):
    def __init__(self, reason: str, where: int | None = None):
        Exception.__init__(self, reason if where is None else f"{reason} at {where}")
        self.reason, self.where = reason, where

    @property
    def word(self) -> int:
        return REJECT_NUMBER[self.reason] | ((self.where or 0) << 8)


class Layout:
    """What `walk` found: the fields of tf_pngdec_info, `bands` [(offset, size)], `first_band_chunk`, `adler`."""

    def __init__(self):
        self.width = self.height = self.band_rows = self.n_bands = 0
        self.indexed, self.why_not = False, "indexed"
        self.bands, self.first_band_chunk, self.adler, self.n_chunks = [], 0, 0, 0

    @property
    def max_band_bytes(self) -> int:
        return max((n for _, n in self.bands), default=0)


# ---- the format --------------------------------------------------------------------------------------------------------
def index_chunk(band_rows: int, n_bands: int, version: int = 1, flags: int = 0) -> bytes:
    return P.chunk(INDEX_TYPE, struct.pack(">BBHII", version, flags, 0, band_rows, n_bands))


def with_index(data: bytes, band_rows: int, n_bands: int | None = None) -> bytes:
    """A file of png_ref.encode with the index between IHDR and the first IDAT."""
    assert data[12:16] == b"IHDR"
    height = struct.unpack(">I", data[20:24])[0]
    if n_bands is None:
        n_bands = -(-height // band_rows)
    return data[:33] + index_chunk(band_rows, n_bands) + data[33:]


def zlib_header_ok(cmf: int, flg: int) -> bool:
    return (cmf & 15) == 8 and (cmf >> 4) <= 7 and not (flg & 0x20) and ((cmf << 8) | flg) % 31 == 0


def walk(data: bytes, max_width: int = MAX_DIM, max_height: int = MAX_DIM) -> Layout:
    """pngdec_common.h's walk: the Layout, or Rejected."""
    data = bytes(data)
    n = len(data)
    if n < 8 or data[:8] != P.SIGNATURE:
        raise Rejected("signature")
    at, chunks = 8, []                  # (type, offset of the length field, payload length)
    idat_closed = ended = False
    while at < n:
        if n - at < 12:
            raise Rejected("truncated")
        size = struct.unpack(">I", data[at:at + 4])[0]
        if size > n - at - 12:
            raise Rejected("truncated")
        kind = data[at + 4:at + 8]
        if (not chunks and (kind != b"IHDR" or size != 13)) or (chunks and kind == b"IHDR"):
            raise Rejected("ihdr")
        if kind == b"IDAT":
            if idat_closed:
                raise Rejected("idat_order")
        else:
            idat_closed = idat_closed or any(k == b"IDAT" for k, _, _ in chunks)
            if kind == b"IEND":
                if size != 0 or at + 12 != n:
                    raise Rejected("no_iend")
                ended = True
        chunks.append((kind, at, size))
        at += 12 + size
    if not ended:
        raise Rejected("no_iend")
    idats = [i for i, (k, _, _) in enumerate(chunks) if k == b"IDAT"]
    if not idats:
        raise Rejected("idat_order")
    out = Layout()
    out.n_chunks = len(chunks)
    width, height, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", data[16:29])
    combos = {0: (1, 2, 4, 8, 16), 3: (1, 2, 4, 8), 2: (8, 16), 4: (8, 16), 6: (8, 16)}
    if depth not in combos.get(colour, ()) or compression or filt or interlace > 1 or width > 0x7FFFFFFF or height > 0x7FFFFFFF:
        raise Rejected("ihdr")
    if width == 0 or height == 0:
        raise Rejected("size")
    out.width, out.height = width, height
    index = [i for i, (k, _, _) in enumerate(chunks) if k == INDEX_TYPE]
    if depth != 8 or colour != 2:
        out.why_not = "format"
    elif interlace:
        out.why_not = "interlaced"
    elif not index:
        out.why_not = "no_index"
    if out.why_not != "indexed":
        return out
    if len(index) > 1 or index[0] > idats[0]:
        raise Rejected("index")
    _, index_at, index_size = chunks[index[0]]
    payload = data[index_at + 8:index_at + 8 + index_size]
    if index_size >= 1 and payload[0] != 1:
        out.why_not = "version"
        return out
    if index_size != 12 or payload[1:4] != b"\0\0\0":
        raise Rejected("index")
    if width > min(max_width, MAX_DIM) or height > min(max_height, MAX_DIM) or (1 + 3 * width) * height > MAX_STREAM:
        raise Rejected("size")
    band_rows, n_bands = struct.unpack(">II", payload[4:])
    if band_rows == 0 or band_rows > height or n_bands != -(-height // band_rows) or len(idats) != n_bands + 2:
        raise Rejected("index")
    out.band_rows, out.n_bands = band_rows, n_bands
    _, first_at, first_size = chunks[idats[0]]
    if first_size != 2 or not zlib_header_ok(data[first_at + 8], data[first_at + 9]):
        raise Rejected("zlib_header")
    out.first_band_chunk = idats[0] + 1
    out.bands = [(chunks[i][1] + 8, chunks[i][2]) for i in idats[1:-1]]
    _, tail_at, tail_size = chunks[idats[-1]]
    if tail_size < 5 or not U.tail_ok(data[tail_at + 8:tail_at + 8 + tail_size - 4]):
        raise Rejected("tail")
    out.adler = struct.unpack(">I", data[tail_at + 4 + tail_size:tail_at + 8 + tail_size])[0]
    out.indexed = True
    return out


# ---- filters -----------------------------------------------------------------------------------------------------------
def paeth(a: int, b: int, c: int) -> int:
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def filter_rows(image: np.ndarray, types) -> np.ndarray:
    """(H, 1 + 3 W) uint8: row y filtered with types[y]; a type above 4 is written as it is over a row filtered with
    None (what a corrupt file holds)."""
    cand = P._candidates(np.asarray(image))
    h = image.shape[0]
    rows = np.empty((h, 1 + cand.shape[2]), np.uint8)
    for y in range(h):
        rows[y, 0] = types[y]
        rows[y, 1:] = cand[types[y] if types[y] <= 4 else 0, y]
    return rows


class Trace:
    """What the unfilter of one or more files reached."""

    def __init__(self):
        self.types = set()                  # every row's type
        self.row0_types = set()
        self.band_first_types = set()       # of bands behind the first
        self.paeth_picks = set()            # "a", "b", "c"
        self.paeth_ties = set()             # "pa=pb", "pb=pc", "pa=pc", "all"
        self.average_overflow = False       # a + b >= 256
        self.sub_wrap = self.up_wrap = False
        self.segments = set()               # the lengths of the segments
        self.max_band_bytes = 0
        self.max_distance = 0
        self.stored_bands = 0
        self.shapes = set()                 # (H, W)

    def merge(self, other: "Trace"):
        for name, value in vars(other).items():
            mine = getattr(self, name)
            if isinstance(mine, set):
                mine |= value
            elif isinstance(mine, bool):
                setattr(self, name, mine or value)
            elif name == "stored_bands":
                self.stored_bands += value
            else:
                setattr(self, name, max(mine, value))


def segment_lengths(types) -> list:
    """Rows are cut at row 0 and at every None or Sub row."""
    starts = [y for y, t in enumerate(types) if y == 0 or t < 2] + [len(types)]
    return [b - a for a, b in zip(starts, starts[1:])]


def unfilter(rows: np.ndarray, trace: Trace | None = None) -> np.ndarray:
    """(H, 3 W) uint8 from the filtered rows (H, 1 + 3 W); the types are 0 - 4."""
    h, n = rows.shape[0], rows.shape[1] - 1
    out = np.zeros((h, n), np.uint8)
    above = np.zeros(n, np.int64)
    for y in range(h):
        t = int(rows[y, 0])
        x = rows[y, 1:].astype(np.int64)
        if t == 0:
            cur = x
        elif t == 2:
            cur = (x + above) & 255
            if trace is not None and bool(((x + above) > 255).any()):
                trace.up_wrap = True
        elif t == 1:
            cur = x.copy()
            for c in range(3):
                cur[c::3] = np.cumsum(x[c::3]) & 255
            if trace is not None and n > 3 and bool(((x[3:] + cur[:-3]) > 255).any()):
                trace.sub_wrap = True
        else:
            cur = [0] * n
            xs, bs = x.tolist(), above.tolist()
            for i in range(n):
                a = cur[i - 3] if i >= 3 else 0
                b = bs[i]
                c = bs[i - 3] if i >= 3 else 0
                if t == 3:
                    pred = (a + b) >> 1
                    if trace is not None and a + b >= 256:
                        trace.average_overflow = True
                else:
                    pred = paeth(a, b, c)
                    if trace is not None:
                        p = a + b - c
                        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                        trace.paeth_picks.add("a" if (pa <= pb and pa <= pc) else ("b" if pb <= pc else "c"))
                        if pa == pb == pc:
                            trace.paeth_ties.add("all")
                        else:
                            for name, same in (("pa=pb", pa == pb), ("pb=pc", pb == pc), ("pa=pc", pa == pc)):
                                if same:
                                    trace.paeth_ties.add(name)
                cur[i] = (xs[i] + pred) & 255
            cur = np.array(cur, np.int64)
        out[y] = cur
        above = cur
    return out


def decode(data: bytes, trace: Trace | None = None, max_width: int = MAX_DIM, max_height: int = MAX_DIM) -> np.ndarray:
    """The pixels (H, W, 3) RGB of an indexed file, or Rejected: the walk, the CRCs of the chunks that are no band, the
    bands' CRCs, the bands (each inflated alone; the lowest rejected band), the filter types (the lowest bad row), the
    Adler-32 -- the order in which tf_pngdec_decode_dev reports."""
    data = bytes(data)
    lay = walk(data, max_width, max_height)
    if not lay.indexed:
        raise ValueError("not for the device: " + lay.why_not)
    band_chunks = range(lay.first_band_chunk, lay.first_band_chunk + lay.n_bands)
    bad = [i for i, (kind, payload, crc) in enumerate(P.chunks(data)) if zlib.crc32(kind + payload) != crc]
    for group in ([i for i in bad if i not in band_chunks], [i for i in bad if i in band_chunks]):
        if group:
            raise Rejected("chunk_crc", group[0])
    row_len = 1 + 3 * lay.width
    parts = []
    for band, (off, size) in enumerate(lay.bands):
        want = min(lay.band_rows, lay.height - band * lay.band_rows) * row_len
        out, reason, btrace = U.inflate_band(data, off, size, want)
        if out is None:
            raise Rejected("band_" + reason, band)
        parts.append(out)
        if trace is not None:
            trace.max_band_bytes = max(trace.max_band_bytes, want)
            trace.max_distance = max(trace.max_distance, btrace.max_distance)
            trace.stored_bands += len(btrace.block_types) > 1 and all(t == 0 for t in btrace.block_types)
    stream = b"".join(parts)
    rows = np.frombuffer(stream, np.uint8).reshape(lay.height, row_len)
    types = rows[:, 0]
    if (types > 4).any():
        raise Rejected("filter_type", int(np.flatnonzero(types > 4)[0]))
    if zlib.adler32(stream) != lay.adler:
        raise Rejected("adler")
    if trace is not None:
        kinds = [int(t) for t in types]
        trace.types |= set(kinds)
        trace.row0_types.add(kinds[0])
        trace.band_first_types |= {kinds[y] for y in range(lay.band_rows, lay.height, lay.band_rows)}
        trace.segments |= set(segment_lengths(kinds))
        trace.shapes.add((lay.height, lay.width))
    return unfilter(rows, trace).reshape(lay.height, lay.width, 3)


# ---- the builder -------------------------------------------------------------------------------------------------------
def build(image: np.ndarray, band_rows: int, filters=None, level: int = 6, header: bytes = b"\x78\x9c",
          strategy: int = zlib.Z_DEFAULT_STRATEGY, bands: dict | None = None, tail: bytes | None = None,
          index: bytes | None = None, adler: int | None = None, flush: dict | None = None) -> bytes:
    """An indexed file of `image` (H, W, 3) uint8 made with zlib: row y filtered with filters[y] (an int: every row;
    None: png_ref's choice), every band compressed and flushed with Z_FULL_FLUSH.  For the malformed corpus: `bands`
    {band: its compressed bytes instead}, `flush` {band: another flush mode}, `tail`, `index` (the whole chunk) and
    `adler` replace what is right."""
    image = np.asarray(image)
    h, w, _ = image.shape
    if filters is None:
        types = [int(t) for t in P.filter_rows(image)[0]]
    else:
        types = [int(filters)] * h if isinstance(filters, int) else [int(t) for t in filters]
    rows = filter_rows(image, types)
    n_bands = -(-h // band_rows)
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out = bytearray(P.SIGNATURE + P.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))
    out += index_chunk(band_rows, n_bands) if index is None else index
    out += P.chunk(b"IDAT", header)
    for band in range(n_bands):
        raw = rows[band * band_rows:(band + 1) * band_rows].tobytes()
        coded = c.compress(raw) + c.flush((flush or {}).get(band, zlib.Z_FULL_FLUSH))
        out += P.chunk(b"IDAT", (bands or {}).get(band, coded))
    last = c.flush(zlib.Z_FINISH) if tail is None else tail
    check = zlib.adler32(rows.tobytes()) if adler is None else adler
    out += P.chunk(b"IDAT", last + struct.pack(">I", check)) + P.chunk(b"IEND", b"")
    return bytes(out)


def rechunk(data: bytes, edit) -> bytes:
    """The file with its chunk list [(kind, payload)] passed through `edit`, CRCs made anew."""
    chunks = [(kind, payload) for kind, payload, _ in P.chunks(data)]
    return P.SIGNATURE + b"".join(P.chunk(kind, payload) for kind, payload in edit(chunks))


def adam7(image: np.ndarray) -> bytes:
    """An interlaced 8-bit RGB PNG of `image` (every row filter None): a file that is not for the device."""
    h, w, _ = image.shape
    passes = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))
    raw = bytearray()
    for x0, y0, dx, dy in passes:
        sub = image[y0::dy, x0::dx]
        if sub.size:
            for row in sub:
                raw += b"\0" + row.tobytes()
    return (P.SIGNATURE + P.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 1)) + P.chunk(b"IDAT", zlib.compress(bytes(raw)))
            + P.chunk(b"IEND", b""))
