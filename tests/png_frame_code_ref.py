"""The PNG encoder's mode "frame" (tf_png_set_code, transflow_amd/csrc/png.hip) restated over tests/png_ref.py and
tests/flowzip_ref.py ("The frame's own code").

Layout, bands, filtering, tokens, the distance code, the Adler-32, the band index and the chunk CRCs are png_ref's.  Two
things differ.  The literal/length code is built from the tokens of ALL bands of the frame -- a match of n counts as
symbol 257 + length_symbol(n), every band brings one end-of-block -- by flowzip_ref.build_lengths; an unused symbol has
length 0; every coded band carries the same 1222-bit table header.  And a band whose coded form would not be smaller than
its stored form is stored: flowzip_ref.stored_band, nothing behind it.

`encode` is the file, `trace` encode's own account of what it coded.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

from tests import flowzip_ref as Z
from tests import png_ref as P
from tests import pngdec_ref as D

N_SYMBOLS = 286
TABLE_BITS = P.TABLE_BITS


def symbol(kind: str, value: int) -> int:
    return 257 + P.length_symbol(value) if kind == "match" else value


def histogram(toks) -> np.ndarray:
    """The 286 counts of one band's tokens."""
    return np.bincount([symbol(kind, value) for _, kind, value in toks], minlength=N_SYMBOLS).astype(np.int64)


def cost(lengths) -> np.ndarray:
    """The bits one occurrence of a symbol takes: a match's extra bits and its distance bit included."""
    return np.array([n + (P.LENGTH_EXTRA[s - 257] + 1 if s > 256 else 0) for s, n in enumerate(lengths)], np.int64)


def coded_bytes(token_bits: int) -> int:
    """The header, the tokens, the three bits of the empty stored block, the padding, its four bytes."""
    return -(-(TABLE_BITS + token_bits + 3) // 8) + 4


def _header(lengths):
    bits = P._Bits()
    for value, n in ((0, 1), (2, 2), (29, 5), (0, 5), (15, 4)):       # BFINAL, BTYPE 10, HLIT, HDIST, HCLEN
        bits.put(value, n)
    for s in P.CLEN_ORDER:
        bits.put(0 if s >= 16 else 4, 3)
    for n in list(lengths) + [1]:                                     # the code of a length is the length
        bits.huff(n, 4)
    assert 8 * len(bits.out) + bits.n == TABLE_BITS
    return bytes(bits.out), bits.acc, bits.n


def coded_band(toks, lengths, codes, header) -> bytes:
    bits = P._Bits()
    bits.out, bits.acc, bits.n = bytearray(header[0]), header[1], header[2]
    for _, kind, value in toks:
        s = symbol(kind, value)
        assert lengths[s]
        bits.huff(codes[s], lengths[s])
        if kind == "match":
            k = s - 257
            bits.put(value - P.LENGTH_BASE[k], P.LENGTH_EXTRA[k])
            bits.put(0, 1)                                            # the distance code
    bits.put(0, 3)                                                    # an empty stored block: not final, BTYPE 00
    bits.align()
    return bytes(bits.out) + b"\x00\x00\xff\xff"


class Trace:
    def __init__(self):
        self.data = b""
        self.histogram = []             # 286 counts over all bands
        self.lengths = []               # 286
        self.repairs = 0
        self.bands = 0
        self.band_rows = 0
        self.row_bytes = 0
        self.band_bytes = []            # per band: the bytes of the filtered stream it holds
        self.band_stored = []           # per band
        self.band_sizes = []            # per band: the bytes of its deflate data
        self.filter_types = []
        self.matches = 0                # match tokens over all bands

    @property
    def stored_blocks(self):
        """The stored blocks of each stored band."""
        return [-(-n // Z.STORED_MAX) for n, stored in zip(self.band_bytes, self.band_stored) if stored]


def encode(image: np.ndarray, band_rows: int = 0, index: bool = False, trace: Trace | None = None) -> bytes:
    image = np.asarray(image)
    h, w, _ = image.shape
    assert image.dtype == np.uint8 and image.shape[2] == 3
    rows = min(h, band_rows if band_rows else P.default_band_rows(h, w))
    types, lines = P.filter_rows(image)
    bands = [lines[first:first + rows].reshape(-1) for first in range(0, h, rows)]
    toks = [P.tokens(band) for band in bands]
    counts = [histogram(t) for t in toks]
    total = np.sum(counts, axis=0)
    lengths, repairs = Z.build_lengths(total)
    codes = Z.canonical_codes(lengths)
    header = _header(lengths)
    bits = cost(lengths)
    out = bytearray(P.SIGNATURE + P.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))
    if index:
        out += D.index_chunk(rows, len(bands))
    out += P.chunk(b"IDAT", b"\x78\x01")
    stored, sizes = [], []
    for band, t, c in zip(bands, toks, counts):
        coded = coded_bytes(int((c * bits).sum()))
        if coded < Z.stored_bytes(len(band)):
            data = coded_band(t, lengths, codes, header)
            assert len(data) == coded
        else:
            data = Z.stored_band(band)
        stored.append(coded >= Z.stored_bytes(len(band)))
        sizes.append(len(data))
        out += P.chunk(b"IDAT", data)
    stream = lines.tobytes()
    out += P.chunk(b"IDAT", b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(stream))) + P.chunk(b"IEND", b"")
    if trace is not None:
        trace.data = bytes(out)
        trace.histogram, trace.lengths, trace.repairs = [int(v) for v in total], list(lengths), repairs
        trace.bands, trace.band_rows, trace.row_bytes = len(bands), rows, 1 + 3 * w
        trace.band_bytes = [len(band) for band in bands]
        trace.band_stored, trace.band_sizes = stored, sizes
        trace.filter_types = [int(v) for v in types]
        trace.matches = int(total[257:].sum())
    return bytes(out)


def trace(image: np.ndarray, band_rows: int = 0, index: bool = False) -> Trace:
    t = Trace()
    encode(image, band_rows, index, t)
    return t


# ---- images: integer formulas only ------------------------------------------------------------------------------------------
def striped_image(height: int, width: int, seed: int) -> np.ndarray:
    """Rows of noise alternating with flat rows of the grey 90."""
    image = P.noise_image(height, width, seed)
    image[1::2] = 90
    return image


def fibonacci_image(symbols: int = 22, seed: int = 31) -> np.ndarray:
    """One row whose byte value v of 1 .. symbols occurs F(v) times (1, 1, 2, 3, 5 ...) in an order shuffled by a hash,
    cut to whole pixels.  Whatever filter wins, the counts of what is coded fall off like the values' do, and the
    optimal code for such counts is a chain: with this seed it is deeper than 15 bits (the tests assert that from the
    trace, not from this text)."""
    fib = [1, 1]
    while len(fib) < symbols:
        fib.append(fib[-1] + fib[-2])
    values = np.repeat(np.arange(1, symbols + 1, dtype=np.uint8), fib)
    values = values[np.argsort(P._hash(seed, len(values)), kind="stable")]
    return values[:len(values) // 3 * 3].reshape(1, -1, 3)


# name: (the image's maker, band_rows) -- png_ref's cases and three of this mode's own
CASES = {
    **P.CASES,
    "8x700_stripes_b1": (lambda: striped_image(8, 700, 41), 1),            # coded and stored bands under one code
    "2x21841_noise_b2": (lambda: P.noise_image(2, 21841, 25), 2),          # a band of 131 048 bytes: two stored blocks
    "1x15455_fibonacci": (fibonacci_image, 0),                             # the code is repaired to 15 bits
}
# the small cases: their files are pinned under tests/golden/ (tools/capture_golden_png_frame_code.py)
GOLDEN_CASES = [name for name in CASES if not (name.startswith("sweep_") or "21841" in name or name.startswith("2049"))]


def case(name: str):
    maker, band_rows = CASES[name]
    return maker(), band_rows
