"""Hand-built JPEG files for the device decoders ("Hand-built scans"): a builder that writes a
baseline file from tables and per-block symbols, a model of the serial reader's window that says where a file makes it
refill, and the case families of tests/test_jpegdec_sweep_ref.py (CPU) and tests/test_gpu_jpegdec_sweep.py (device).
It generalises jpegdec_cases._handmade and jpegdec_par_cases.handmade_big.  Pure Python and numpy, deterministic; the
one file read is the Pillow-written fixture whose DHT segments give the Annex K tables (standard_tables).

A block is (DC difference, [(run, value), ...]): value 0 with run 15 is a ZRL; EOB is written unless the last coefficient
sits at k = 63.  A block may also be a string of raw bits.  `at({k: value})` turns zigzag positions into runs.
"""
from __future__ import annotations

import os
from collections import namedtuple

import numpy as np

from . import jpegdec_ref as JR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# jpegdec_common.h
WINDOW_BYTES = 1024
BLOCK_MARGIN = 2 * 216 + 16
FAST_BITS = 9


# ---- tables ----------------------------------------------------------------------------------------------------------------
def canonical(table) -> dict:
    """{symbol: (length, code)} of a (counts, vals) table."""
    counts, vals = table
    out, code, p = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[vals[p]] = (length, code)
            code, p = code + 1, p + 1
        code <<= 1
    return out


def ladder_ac(longest: int = 0x01):
    """One code per length 1..16: 0 (EOB), 10 (run 1 size 1), 110 (run 2 size 1), ..., and `longest` under
    1111111111111110."""
    return [1] * 16, [0x00] + [(r << 4) | 1 for r in range(1, 15)] + [longest]


LADDER_DC = ([1] * 12 + [0] * 4, list(range(12)))          # categories 0..11 under codes of 1..12 bits


def seam_ac():
    """The FAST_BITS seam: EOB under 00, the 160 symbols (run 0..15, size 1..10) under 60 codes of 9 bits and 100 of
    10, ZRL under a code of 11."""
    syms = [(r << 4) | s for s in range(1, 11) for r in range(16)]
    return [0, 1, 0, 0, 0, 0, 0, 0, 60, 100, 1, 0, 0, 0, 0, 0], [0x00] + syms + [0xF0]


def tables_of(data: bytes) -> dict:
    """{(class, id): (counts, vals)} of a file's DHT segments."""
    out, at = {}, 2
    while data[at + 1] != 0xDA:
        length = int.from_bytes(data[at + 2:at + 4], "big")
        if data[at + 1] == 0xC4:
            p, k = data[at + 4:at + 2 + length], 0
            while k < len(p):
                counts = list(p[k + 1:k + 17])
                out[(p[k] >> 4, p[k] & 15)] = (counts, list(p[k + 17:k + 17 + sum(counts)]))
                k += 17 + sum(counts)
        at += 2 + length
    return out


_STANDARD = []


def standard_tables() -> dict:
    """Annex K's tables as Pillow writes them: the DHT segments of a fixture file, not typed in.
    {"dc_luma", "ac_luma", "dc_chroma", "ac_chroma"}."""
    if not _STANDARD:
        z = np.load(os.path.join(GOLDEN, "jpegdec_valid.npz"))
        t = tables_of(z["geo_420_37x19.file"].tobytes())
        _STANDARD.append({"dc_luma": t[(0, 0)], "ac_luma": t[(1, 0)], "dc_chroma": t[(0, 1)], "ac_chroma": t[(1, 1)]})
        assert sum(t[(1, 0)][0]) == 162 and t[(1, 0)][0][15] == 125 and sum(t[(0, 0)][0]) == 12
    return _STANDARD[0]


# ---- the builder -----------------------------------------------------------------------------------------------------------
Built = namedtuple("Built", "data ops")
# ops: per interval, per block, [(kind, code length, value bits)], kind "d" or "a" (None for a block of raw bits)


def at(coefs: dict) -> list:
    """{zigzag position: value} -> [(run, value)] with the ZRLs the runs need."""
    out, k = [], 1
    for pos in sorted(coefs):
        run = pos - k
        out += [(15, 0)] * (run // 16) + [(run % 16, coefs[pos])]
        k = pos + 1
    return out


def _magnitude(value: int):
    s = abs(value).bit_length()
    return s, format(value if value > 0 else value + (1 << s) - 1, f"0{s}b") if s else ""


def _block_bits(block, dc: dict, ac: dict):
    if isinstance(block, str):
        return block, None
    diff, pairs = block
    s, vbits = _magnitude(diff)
    length, code = dc[s]
    bits, ops, k = [format(code, f"0{length}b"), vbits], [("d", length, s)], 1
    for run, value in pairs:
        s, vbits = _magnitude(value)
        assert s or run == 15, "value 0 is for ZRL"
        length, code = ac[(run << 4) | s]
        bits += [format(code, f"0{length}b"), vbits]
        ops.append(("a", length, s))
        k += run + 1
    assert k <= 64, "the block's runs pass coefficient 63"
    if k < 64:
        length, code = ac[0x00]
        bits.append(format(code, f"0{length}b"))
        ops.append(("a", length, 0))
    return "".join(bits), ops


def _seg(marker: int, payload, fill: int = 0) -> bytes:
    return b"\xff" * fill + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def build(blocks, size, colour: bool = False, dc=None, ac=None, quant=1, restart: int = 0, width=None, height=None,
          merge_dht: bool = False, merge_dqt: bool = False, extra: bytes = b"", fill: int = 0, sampling=(2, 2)) -> Built:
    """A baseline file.  size: (across, down) in MCUs -- 8 x 8 blocks of a grey file, 16 x 16 pixels of 6 blocks (4 luma,
    Cb, Cr) of a 4:2:0 one; width / height: the picture's, where it ends inside the last MCUs.  blocks: all of them in
    scan order.  sampling: a colour file's luma factors -- (2, 2), (2, 1) for 4:2:2 (16 x 8 pixels of 4 blocks: 2 luma,
    Cb, Cr) or (1, 1) for 4:4:4 (8 x 8 pixels of 3 blocks).  dc, ac: a (counts, vals) table, or one per component; quant:
    a number or 64 of them by zigzag position, or one such per component.  Equal tables share an id.  restart: the interval in MCUs (0: no DRI).  merge_dht,
    merge_dqt: one segment for all tables of the kind; extra: bytes put in front of SOS; fill: FF bytes in front of every
    marker of the header."""
    ncomp = 3 if colour else 1
    assert sampling in ((1, 1), (2, 1), (2, 2)), sampling
    hs, vs = sampling if colour else (1, 1)
    luma = hs * vs
    per_mcu = luma + 2 if colour else 1
    n_mcus = size[0] * size[1]
    assert len(blocks) == n_mcus * per_mcu, (len(blocks), n_mcus * per_mcu)
    each = lambda v, single: [v] * ncomp if single(v) else list(v)
    dcs = each(dc, lambda v: isinstance(v, tuple))
    acs = each(ac, lambda v: isinstance(v, tuple))
    quants = each(quant, lambda v: np.ndim(v) == 0 or len(v) == 64)
    quants = [[int(q)] * 64 if np.ndim(q) == 0 else [int(v) for v in q] for q in quants]

    def ids(items):
        distinct = []
        for item in items:
            if item not in distinct:
                distinct.append(item)
        return distinct, [distinct.index(item) for item in items]

    q_tabs, q_ids = ids(quants)
    dc_tabs, dc_ids = ids(dcs)
    ac_tabs, ac_ids = ids(acs)
    mw, mh = 8 * hs, 8 * vs
    w, h = width or size[0] * mw, height or size[1] * mh
    assert -(-w // mw) == size[0] and -(-h // mh) == size[1]
    out = b"\xff\xd8"
    dqts = [[i] + q for i, q in enumerate(q_tabs)]
    out += _seg(0xDB, sum(dqts, []), fill) if merge_dqt else b"".join(_seg(0xDB, p, fill) for p in dqts)
    comps = [[c + 1, ((hs << 4 | vs) if c == 0 else 0x11), q_ids[c]] for c in range(ncomp)]
    out += _seg(0xC0, [8, *h.to_bytes(2, "big"), *w.to_bytes(2, "big"), ncomp] + sum(comps, []), fill)
    dhts = [[i] + list(t[0]) + list(t[1]) for i, t in enumerate(dc_tabs)] + [[0x10 | i] + list(t[0]) + list(t[1]) for i, t in enumerate(ac_tabs)]
    out += _seg(0xC4, sum(dhts, []), fill) if merge_dht else b"".join(_seg(0xC4, p, fill) for p in dhts)
    if restart:
        out += _seg(0xDD, restart.to_bytes(2, "big"), fill)
    out += extra
    out += _seg(0xDA, [ncomp] + sum([[c + 1, (dc_ids[c] << 4) | ac_ids[c]] for c in range(ncomp)], []) + [0, 63, 0], fill)
    dc_codes, ac_codes = [canonical(t) for t in dcs], [canonical(t) for t in acs]
    per = restart or n_mcus
    ops = []
    for iv, first in enumerate(range(0, n_mcus, per)):
        bits, iv_ops = [], []
        for m in range(first, min(first + per, n_mcus)):
            for blk in range(per_mcu):
                c = 0 if blk < luma else blk - luma + 1
                b, o = _block_bits(blocks[m * per_mcu + blk], dc_codes[c], ac_codes[c])
                bits.append(b)
                iv_ops.append(o)
        bits = "".join(bits)
        bits += "1" * (-len(bits) % 8)
        if iv:
            out += bytes([0xFF, 0xD0 + ((iv - 1) & 7)])
        out += int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00") if bits else b""
        ops.append(iv_ops)
    return Built(out + b"\xff\xd9", ops)


def intervals_of(data: bytes) -> list:
    hd = JR.parse_header(data)
    return JR.split_intervals(data[hd["scan_offset"]:], hd["intervals"] - 1)


# ---- what a file's symbols are, and where the serial reader's window moves ---------------------------------------------------
def symbol_phases(built: Built) -> set:
    """{(kind, code length, bit phase)}: the position modulo 8, in the interval's bits without stuffing, at which each
    code of the file begins."""
    out = set()
    for blocks in built.ops:
        pos = 0
        for ops in blocks:
            assert ops is not None, "a block of raw bits has no symbols to follow"
            for kind, length, s in ops:
                out.add((kind, length, pos & 7))
                pos += length + s
    return out


Refill = namedtuple("Refill", "interval block next cnt tail behind head")


def refills(built: Built, margin: int = BLOCK_MARGIN):
    """The serial reader's window over a file (need_refill, refill_range and fill of jpegdec_common.h): every refill as
    (interval, block within it, next, bits in buf, the window's last two bytes, the byte behind them or None, the
    window's first two bytes), and the number of symbols the window could not feed (none unless `margin` is too small).  For
    asserting what a file covers; never for expected pixels."""
    out, starved = [], 0
    for iv, (chunk, blocks) in enumerate(zip(intervals_of(built.data), built.ops)):
        size, nxt, cnt, base, wlen = len(chunk), 0, 0, 0, 0

        def fill():
            nonlocal nxt, cnt
            while cnt <= 56 and nxt < size and nxt - base < wlen:
                if chunk[nxt] == 0xFF:
                    if nxt + 1 - base >= wlen or chunk[nxt + 1] != 0:
                        break
                    nxt += 1
                cnt, nxt = cnt + 8, nxt + 1

        for blk, ops in enumerate(blocks):
            assert ops is not None, "a block of raw bits has no symbols to follow"
            if base + wlen < size and nxt + margin > base + wlen:
                base, wlen = nxt, min(size - nxt, WINDOW_BYTES)
                end = base + wlen
                out.append(Refill(iv, blk, nxt, cnt, bytes(chunk[max(end - 2, base):end]), chunk[end] if end < size else None, bytes(chunk[base:base + 2])))
            for _, length, s in ops:
                for need, floor in ((length, 16), (s, s)):
                    if cnt < floor:
                        fill()
                    starved += cnt < need
                    cnt -= min(need, cnt)
    return out, starved


# ---- the case families -----------------------------------------------------------------------------------------------------
# Every family: [(name, Built)].  A..B, D..F are pinned by Pillow (tests/test_jpegdec_sweep_ref.py holds the restatement
# equal to it on each of them); C by the restatement alone.
BIG_SIGNS = 0x5A3C96E1F00F17D3          # the signs of a long block's 63 coefficients, rotated from block to block


def long_block(i: int = 0, diff: int = 0, value: int = 1) -> tuple:
    """DC `diff` and 63 coefficients of +-value under the run-0 code: with ladder_ac, 17 bits each for value 1."""
    signs = [(BIG_SIGNS >> ((k * 7 + i * 11) % 64)) & 1 for k in range(63)]
    return diff, [(0, value if s else -value) for s in signs]


SHORT = (0, [])                         # DC 0, EOB: two bits under the ladder tables


def _rows(blocks: list, across: int, pad=SHORT):
    """The blocks padded to whole rows of `across`: (blocks, (across, down))."""
    down = -(-len(blocks) // across)
    return blocks + [pad] * (across * down - len(blocks)), (across, down)


def _dc_walk(categories, pred: int = 0):
    """Differences of the given categories, each of the sign that keeps the prediction inside +-2047, and one more that
    brings it back to 0."""
    diffs = []
    for n, s in enumerate(categories):
        mag = 0 if s == 0 else ((1 << s) - 1 if n & 1 else 1 << (s - 1))
        diff = -mag if pred > 0 else mag
        diffs.append(diff)
        pred += diff
    return diffs + [-pred]


def family_a() -> list:
    """Code lengths by phases."""
    out = []
    # every ladder code at every bit phase: blocks of ladder symbols with coefficients +-1; at each step the symbol is one
    # that has not yet begun at the current phase, where there is one (the DC categories' value bits shift the phase)
    rng = np.random.default_rng(2024)
    want = {("a", length, ph) for length in range(1, 17) for ph in range(8)} | {("d", length, ph) for length in range(1, 13) for ph in range(8)}
    blocks, pred, seen, pos = [], 0, set(), 0
    ladder = ladder_ac()
    while not want <= seen:
        assert len(blocks) < 200
        new = [s for s in range(12) if ("d", s + 1, pos & 7) not in seen]
        s = new[0] if new else int(rng.integers(0, 12))
        mag = 0 if s == 0 else int(rng.integers(1 << (s - 1), 1 << s))
        diff = -mag if pred > 0 else mag
        pred += diff
        seen.add(("d", s + 1, pos & 7))
        pos += 2 * s + 1
        pairs, k = [], 1
        while k < 64:
            fits = [length for length in range(1, 17) if k + (0 if length == 16 else length - 1) <= 63]
            new = [length for length in fits if ("a", length, pos & 7) not in seen]
            length = new[int(rng.integers(0, len(new)))] if new else fits[int(rng.integers(0, len(fits)))]
            seen.add(("a", length, pos & 7))
            pos += length + (length > 1)
            if length == 1:
                break
            run = 0 if length == 16 else length - 1
            pairs.append((run, 1 if rng.integers(0, 2) else -1))
            k += run + 1
        blocks.append((diff, pairs))
    padded, size = _rows(blocks, 8, pad=(0, []))
    out.append(("a_ladder_phases", build(padded, size, dc=LADDER_DC, ac=ladder)))
    std = standard_tables()
    for name, dc, ac in (("a_standard_all_symbols", std["dc_luma"], std["ac_luma"]), ("a_seam_9_10", LADDER_DC, seam_ac())):
        padded, size = _rows(all_symbol_blocks(), 8)
        out.append((name, build(padded, size, dc=dc, ac=ac)))
    return out


SAMPLE_BUDGET = 370     # |sample - 128| a block may reach: within the 384 up to which wrapping (libjpeg's C) is clamping (its SIMD)


def all_symbol_blocks() -> list:
    """Blocks that between them use the 160 (run, size) symbols, ZRL, EOB and the twelve DC categories.  A coefficient is
    the smallest of its size, signs alternate, and a block takes symbols only while |DC| / 8 + sum |AC| / 4 stays under
    SAMPLE_BUDGET (the largest basis amplitudes), so no sample leaves the range where wrapping and clamping agree."""
    blocks = []
    for diff in _dc_walk(list(range(12)) + [11, 10, 9]):                # the DC categories, with a +-1 or two beside them
        blocks.append((diff, [(0, 1), (2, -1)]))
    symbols = [(r, s) for s in range(10, 0, -1) for r in range(16)]
    pairs, k, load, sign = [], 1, 0.0, 1
    while symbols:
        for i, (r, s) in enumerate(symbols):                             # the first that still fits this block
            mag = 1 << (s - 1)
            if k + r <= 63 and load + mag / 4 <= SAMPLE_BUDGET:
                pairs.append((r, sign * mag))
                k, load, sign = k + r + 1, load + mag / 4, -sign
                del symbols[i]
                break
        else:
            blocks.append((0, pairs))
            pairs, k, load = [], 1, 0.0
    blocks.append((0, pairs))
    blocks.append((0, [(15, 0)] * 3 + [(14, 1)]))                        # ZRL ZRL ZRL, then run 14 lands on k = 63: no EOB
    blocks.append((0, [(15, 0)] * 2 + [(14, -1), (15, 1)]))              # a run-15 symbol lands on k = 63
    blocks.append((0, [(0, 1 if k & 1 else -1) for k in range(63)]))     # 63 coefficients, no EOB
    blocks.append((0, [(15, 0), (0, 2)]))
    return blocks


def family_b() -> list:
    """The refill sweep: long ladder blocks (about 200 bytes each, half of them stuffed) behind a varying number of
    2-bit blocks, in one interval and in intervals of 5, 7 and 11 blocks."""
    out = []
    ladder = ladder_ac()
    for shorts, odd in B_FRONTS:
        blocks = [SHORT] * shorts + [ODD] * odd + [long_block(i + shorts) for i in range(B_LONG)]
        padded, size = _rows(blocks, 8)
        out.append((f"b_nodri_s{shorts:02d}_o{odd}", build(padded, size, dc=LADDER_DC, ac=ladder)))
    for restart in B_RESTARTS:
        blocks = [long_block(i + restart) for i in range(B_DRI_LONG)]
        out.append((f"b_dri_{restart:02d}", build(blocks, (8, B_DRI_LONG // 8), dc=LADDER_DC, ac=ladder, restart=restart)))
    return out


ODD = (0, [(1, 1)])                     # DC 0, run 1 size 1, EOB: five bits, so that the long blocks begin at odd phases too
B_FRONTS = ((0, 0), (1, 0), (2, 0), (3, 0), (7, 0), (12, 0), (19, 0),
            (0, 1), (1, 1), (2, 1), (3, 1), (5, 1), (9, 1), (15, 1))
B_LONG = 24
B_RESTARTS = (5, 7, 11)
B_DRI_LONG = 24


def family_c() -> list:
    """The margin: blocks of 63 coefficients of +1023 under the 16-bit code, 26 bits with one zero, about 400 bytes after
    stuffing; shorter blocks between them so that they begin at many distances from the window's end."""
    ladder = ladder_ac(0x0A)
    heavy = (0, [(0, 1023)] * 63)
    blocks = []
    for i in range(10):
        blocks += [heavy, (0, [(0, 1023)] * (5 + 6 * i))]
    blocks += [heavy, heavy, (2047, [(0, 1023)] * 63), (-2047, [(0, -1023)] * 63)]
    assert len(blocks) == 24
    return [("c_margin_nodri", build(blocks, (8, 3), dc=LADDER_DC, ac=ladder)),
            ("c_margin_dri2", build(blocks, (8, 3), dc=LADDER_DC, ac=ladder, restart=2))]


def family_d() -> list:
    """Coefficient edges."""
    std = standard_tables()
    dc, ac = std["dc_luma"], std["ac_luma"]
    out = []
    # the prediction walks 0 -> +1023 -> -1024 -> +1023 ..., then +2047 and -2047 alone
    diffs = [1023, -2047, 2047, -2047, 2047, -1023, 2047, -2047, -2047, 2047, 0, -2047, 2047, 2047, -2047, 0]
    for name, tabs in (("d_dc_walk", (dc, ac)), ("d_dc_walk_ladder", (LADDER_DC, ladder_ac()))):
        out.append((name, build([(d, []) for d in diffs], (8, 2), dc=tabs[0], ac=tabs[1])))
    out.append(("d_dc_walk_dri1", build([(d, []) for d in (2047, -2047, 1024, -1024, 2047, -2047, 1023, -1023)], (8, 1), dc=dc, ac=ac, restart=1)))
    # category 10 alone at each of the 63 positions
    blocks = [(0, at({k: v})) for k in range(1, 64) for v in (1023, -1023, 512, -512)]
    padded, size = _rows(blocks, 18)
    out.append(("d_ac10_positions", build(padded, size, dc=dc, ac=ac)))
    # the ends of every category, AC (at two positions) and DC
    blocks = [(0, at({k: v})) for s in range(1, 11) for k in (1, 37) for v in ((1 << (s - 1)), -(1 << (s - 1)), (1 << s) - 1, 1 - (1 << s))]
    for s in range(1, 12):
        for v in ((1 << (s - 1)), -(1 << (s - 1)), (1 << s) - 1, 1 - (1 << s)):
            blocks += [(v, [(0, 1)]), (-v, [])]
    padded, size = _rows(blocks, 16)
    out.append(("d_category_edges", build(padded, size, dc=dc, ac=ac)))
    # quantiser 255 with small values
    blocks = [(d, at({k: v})) for d, k, v in [(0, 1, 1), (0, 2, -1), (1, 63, 1), (-1, 9, 2), (8, 5, -2), (-8, 1, 1), (-8, 20, -1), (8, 44, 2),
                                              (3, 1, 3), (-3, 8, -3), (5, 2, 1), (-5, 3, -1), (0, 62, 4), (0, 4, -4), (2, 6, 1), (-2, 7, -1)]]
    out.append(("d_quant_255", build(blocks, (8, 2), dc=dc, ac=ac, quant=255)))
    return out


def family_e() -> list:
    """Colour: 4:2:0, 37 x 19 (3 x 2 MCUs, both edges inside an MCU), luma on the ladder tables, chroma on the standard
    ones, a quantiser table per component; without DRI and with DRI 1."""
    std = standard_tables()
    blocks = []
    for m in range(6):
        blocks += [long_block(4 * m + i, diff=(3 if (m + i) & 1 else -3)) for i in range(4)]
        blocks += [(2 * m - 5, at({1: 2, 2: -1, 9: 1})), (4 - m, at({1: -1, 3: 1, 63: 1}))]
    kw = dict(colour=True, width=37, height=19, dc=[LADDER_DC, std["dc_chroma"], std["dc_chroma"]],
              ac=[ladder_ac(), std["ac_chroma"], std["ac_chroma"]], quant=[1, 2, 3])
    return [("e_420_nodri", build(blocks, (3, 2), **kw)), ("e_420_dri1", build(blocks, (3, 2), restart=1, **kw))]


def family_f() -> list:
    """Segment forms the header walker takes: 4:2:0, 16 x 16, one MCU."""
    std = standard_tables()
    blocks = [(5, at({1: 3})), (-2, at({2: -2})), (1, []), (0, at({63: 1})), (4, at({1: 1})), (-4, at({8: -1}))]
    kw = dict(colour=True, dc=[std["dc_luma"], std["dc_chroma"], std["dc_chroma"]], ac=[std["ac_luma"], std["ac_chroma"], std["ac_chroma"]],
              quant=[2, 3, 3])
    unused = _seg(0xDB, [3] + [7] * 64) + _seg(0xC4, [0x13] + ladder_ac()[0] + ladder_ac()[1]) + _seg(0xC4, [0x03] + LADDER_DC[0] + LADDER_DC[1])
    com_app = _seg(0xFE, b"hand-built") + _seg(0xE5, bytes(range(40))) + _seg(0xEF, b"\xff\xd9\xff\x00")
    return [("f_plain", build(blocks, (1, 1), **kw)),
            ("f_dht_in_one_segment", build(blocks, (1, 1), merge_dht=True, **kw)),
            ("f_dqt_in_one_segment", build(blocks, (1, 1), merge_dqt=True, **kw)),
            ("f_unused_tables", build(blocks, (1, 1), extra=unused, **kw)),
            ("f_com_and_app", build(blocks, (1, 1), extra=com_app, **kw)),
            ("f_fill_bytes", build(blocks, (1, 1), fill=2, **kw)),
            ("f_dri_past_the_end", build(blocks, (1, 1), restart=9, **kw)),
            ("f_dht_cut_short", build(blocks, (1, 1), extra=_seg(0xC4, [0x02] + [0] * 10), **kw))]      # rejected: bad_dht


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e, "f": family_f}
RESTATEMENT_ONLY = ("c",)


def all_cases() -> list:
    """[(name, Built)], every family, in order."""
    return [case for key in FAMILIES for case in FAMILIES[key]()]


SUBS = (16, 64, 128)                    # the subsequence sizes whose entry rows the fixture keeps: forced small, the default, forced large


def family_of(name: str) -> str:
    return name[0]


# ---- the pixel stages: colour, MCU order, the IDCT's basis -------------------------------------------------------------------
# Families G..I are not part of all_cases() / jpegdec_sweep.npz: tests/golden/jpegdec_geometry.npz keeps them with
# Pillow's pixels (tools/capture_golden_jpegdec.py); tests/test_jpegdec_sweep_ref.py holds the restatement equal to Pillow on
# each of them and tests/test_gpu_jpegdec_geometry.py the device to both.
def flat_blocks(samples, components, restart_blocks: int = 0) -> list:
    """DC-only blocks at quantiser 8, where a block's 64 samples are 128 + DC: the DC differences that give the blocks, in
    scan order, the flat sample values `samples` (0..255).  components: each block's component; restart_blocks: the
    predictions start over every so many blocks."""
    out, pred = [], [0, 0, 0]
    for i, (v, c) in enumerate(zip(samples, components)):
        if restart_blocks and i % restart_blocks == 0:
            pred = [0, 0, 0]
        out.append((int(v) - 128 - pred[c], []))
        pred[c] = int(v) - 128
    return out


LATTICE_Y = (0, 1, 16, 127, 128, 235, 254, 255)
LATTICE_C = (0, 1, 16, 64, 127, 128, 129, 192, 240, 254, 255)
LATTICE_SIZE = (44, 22)                 # 968 MCUs of 8 x 8: 352 x 176 pixels


def lattice() -> list:
    """[(Y, Cb, Cr)] of the colour lattice's MCUs, in scan order."""
    return [(y, cb, cr) for y in LATTICE_Y for cb in LATTICE_C for cr in LATTICE_C]


def _standard_colour() -> dict:
    std = standard_tables()
    return dict(colour=True, dc=[std["dc_luma"], std["dc_chroma"], std["dc_chroma"]], ac=[std["ac_luma"], std["ac_chroma"], std["ac_chroma"]],
                quant=8)


def family_g() -> list:
    """The colour lattice: 4:4:4, one flat MCU per (Y, Cb, Cr), so every pixel of it is that triple through jdcolor.c's
    tables -- each channel's clamp at 0 and at 255, and the rounding either side of Cb, Cr = 128."""
    samples = [v for triple in lattice() for v in triple]
    assert len(samples) == 3 * LATTICE_SIZE[0] * LATTICE_SIZE[1]
    return [("g_lattice_444", build(flat_blocks(samples, [0, 1, 2] * (len(samples) // 3)), LATTICE_SIZE, sampling=(1, 1), **_standard_colour()))]


H_SIZE = (6, 4)                         # MCUs: 24 of them


def order_samples(sampling, size=H_SIZE) -> list:
    """The flat sample values of family H's blocks in scan order: every luma block of an MCU another value (and another
    from MCU to MCU), Cb 0 / 255 in a checkerboard of MCUs and Cr its opposite, so that a chroma block's neighbour is the
    largest step away, across and down."""
    luma = sampling[0] * sampling[1]
    out = []
    for my in range(size[1]):
        for mx in range(size[0]):
            m = my * size[0] + mx
            out += [(29 * m + 67 * i + 11) % 256 for i in range(luma)]
            out += [255 * ((mx + my) & 1), 255 * ((mx + my + 1) & 1)]
    return out


def family_h() -> list:
    """MCU order of 4:2:2 and 4:2:0: flat blocks, see order_samples; the picture ends one pixel and fifteen pixels into
    the last MCU across (and inside the last MCU down); without DRI, and at 16k + 1 with an interval of 5 MCUs (which
    does not divide a row's 6)."""
    out = []
    for tag, sampling in (("422", (2, 1)), ("420", (2, 2))):
        per_mcu = sampling[0] * sampling[1] + 2
        comps = ([0] * (per_mcu - 2) + [1, 2]) * (H_SIZE[0] * H_SIZE[1])
        samples = order_samples(sampling)
        height = 8 * sampling[1] * (H_SIZE[1] - 1) + 3
        for width in (16 * (H_SIZE[0] - 1) + 1, 16 * (H_SIZE[0] - 1) + 15):
            kw = dict(sampling=sampling, width=width, height=height, **_standard_colour())
            out.append((f"h_order_{tag}_{width}x{height}", build(flat_blocks(samples, comps), H_SIZE, **kw)))
            if width % 16 == 1:
                out.append((f"h_order_{tag}_{width}x{height}_dri5", build(flat_blocks(samples, comps, 5 * per_mcu), H_SIZE, restart=5, **kw)))
    return out


BASIS_SIZE = (16, 16)                   # 256 blocks: 128 x 128 pixels
BASIS_QUANT = list(range(1, 65))        # by zigzag position


def basis_blocks() -> list:
    """[(zigzag position, coefficient as coded)] of family I's blocks in scan order: each position alone, at +-1 and at
    +- the largest value whose dequantised amplitude (|DC| / 8, |AC| / 4 bound a sample's distance from 128) stays within
    SAMPLE_BUDGET, and within category 10 (for DC too: from +1023 to -1023 is a difference of category 11, the last)."""
    out = []
    for k in range(64):
        top = min(SAMPLE_BUDGET * (8 if k == 0 else 4) // BASIS_QUANT[k], 1023)
        out += [(k, 1), (k, -1), (k, top), (k, -top)]
    return out


def family_i() -> list:
    """The IDCT's basis: a grey file, one coefficient a block, the quantiser 1..64 by zigzag position."""
    std = standard_tables()
    blocks, pred = [], 0
    for k, v in basis_blocks():
        dc = v if k == 0 else 0
        blocks.append((dc - pred, [] if k == 0 else at({k: v})))
        pred = dc
    return [("i_idct_basis", build(blocks, BASIS_SIZE, dc=std["dc_luma"], ac=std["ac_luma"], quant=BASIS_QUANT))]


PIXEL_FAMILIES = {"g": family_g, "h": family_h, "i": family_i}


def pixel_cases() -> list:
    """[(name, Built)] of families G, H and I."""
    return [case for key in PIXEL_FAMILIES for case in PIXEL_FAMILIES[key]()]
