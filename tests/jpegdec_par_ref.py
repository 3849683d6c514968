"""The device JPEG decoder's parallel path for scans without restart markers, restated in Python
(transflow_amd/csrc/jpegdec_par_common.h, jpegdec.hip; DESIGN.md section 19, "scans without restart markers"): the grid
of subsequences, the bit window, the lane that decodes leniently (synchronisation) or strictly (write), the fixed point
of the entries and the exclusive sums.  Headers, tables and the serial truth are tests/jpegdec_ref.py's.

A state is (position, block within the MCU, k): the position a bit index into the scan's bytes without the EOI, stuffed
bytes included, never inside the 00 of an FF 00 pair.  The lenient rules, as the header pins them:
    16 bits that match no code            skip one bit
    a run past coefficient 63             the symbol is consumed, its value bits are not; the block ends
    an AC symbol that is no symbol        the block ends
    a category above 11 (DC) or 10 (AC)   the value bits of the largest legal category are taken
    fewer bits left than a symbol needs   the lane ends at the end of the data, (block, k) as they were
"""
from __future__ import annotations

import numpy as np

from . import jpegdec_ref as JR

REASON_BITS = 5
_LUTS = {}


def _lut(table: dict) -> list:
    """By the next 16 bits: (length << 8) | symbol, or 0."""
    key = id(table)
    if key not in _LUTS:
        lut = [0] * 65536
        for (length, code), sym in table.items():
            first = code << (16 - length)
            lut[first:first + (1 << (16 - length))] = [(length << 8) | sym] * (1 << (16 - length))
        _LUTS[key] = (table, lut)
    return _LUTS[key][1]


def _extend(v: int, s: int) -> int:
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


class ParScan:
    """A file whose header the device takes and whose marker scan passes, cut into subsequences of `sub_bytes`."""

    def __init__(self, data: bytes, sub_bytes: int):
        hd = JR.parse_header(data)
        scan = data[hd["scan_offset"]:]
        JR.split_intervals(scan, hd["intervals"] - 1)                 # the marker scan's verdict first
        assert hd["restart_mcus"] == 0, "the parallel path is for files without DRI"
        self.hd, self.S = hd, sub_bytes
        self.size = len(scan) - 2
        self.data = scan[:self.size] + bytes(16)                       # zeros behind the data
        self.total_bits = 8 * self.size
        self.n_subs = max(1, -(-self.size // sub_bytes))
        self.blocks = hd["blocks_per_mcu"]
        self.luma = 1 if hd["components"] == 1 else hd["h_samp"] * hd["v_samp"]
        self.total_blocks = hd["n_mcus"] * self.blocks
        self.dc = [_lut(hd["tables"][min(c, hd["components"] - 1) if hd["components"] == 3 else 0][0]) for c in range(3)]
        self.ac = [_lut(hd["tables"][min(c, hd["components"] - 1) if hd["components"] == 3 else 0][1]) for c in range(3)]
        self.quant = [hd["tables"][c if hd["components"] == 3 else 0][2] for c in range(3)]

    # ---- the bit window: par_window, par_peek, par_advance ----
    def _window(self, pos: int):
        base = pos >> 3
        raw = self.data[base:base + 8]
        if self.size - base < 8:
            raw = self.data[base:max(base, self.size)] + bytes(8)
            raw = raw[:8]
        stuffed = 0
        if b"\xff\x00" in raw:
            out = bytearray()
            for t in range(8):
                if t and raw[t - 1] == 0xFF and raw[t] == 0:
                    stuffed |= 1 << t
                else:
                    out.append(raw[t])
            raw = bytes(out) + bytes(8 - len(out))
        return int.from_bytes(raw, "big"), stuffed, base

    @staticmethod
    def _advance(win, pos: int, n: int) -> int:
        _, stuffed, base = win
        bit = (pos & 7) + n
        j = bit >> 3
        u = j
        if stuffed:
            for _ in range(4):
                u = j + bin(stuffed & ((2 << u) - 1)).count("1")
        return (base + u) * 8 + (bit & 7)

    def guess(self, i: int):
        at = i * self.S
        if i and at < self.size and self.data[at] == 0 and self.data[at - 1] == 0xFF:
            at += 1
        return (at * 8, 0, 0)

    def lane(self, i: int, entry, strict: bool = False, first_block: int = 0, pred=(0, 0, 0), coef=None):
        """par_lane: (exit state, blocks begun, DC sums mod 2^32, fault name or None)."""
        end = min((i + 1) * self.S, self.size) * 8
        p, b, k = entry
        n_begin, sums, fault = 0, [0, 0, 0], None
        cur = first_block - 1
        dcv = [((v + 2 ** 31) % 2 ** 32) - 2 ** 31 for v in pred]
        done = strict and k > 0 and not 0 <= cur < self.total_blocks
        trips = 0
        while trips <= 8 * self.S and p < end and not done:
            trips += 1
            c = 0 if b < self.luma else b - self.luma + 1
            if strict and k == 0 and first_block + n_begin >= self.total_blocks:
                break
            win = self._window(p)
            o = p & 7
            e = (self.dc if k == 0 else self.ac)[c][(win[0] >> (48 - o)) & 0xFFFF]
            if not e:
                if self._advance(win, p, 16) > self.total_bits:
                    fault, p = "exhausted", self.total_bits
                    break
                if strict:
                    fault = "bad_code"
                    break
                p = self._advance(win, p, 1)
                continue
            length, sym = e >> 8, e & 255
            behind = self._advance(win, p, length)
            if behind > self.total_bits:
                fault, p = "exhausted", self.total_bits
                break
            ends, k_at = False, 0
            if k == 0:
                s = sym
                if s > 11:
                    if strict:
                        fault = "category"
                        break
                    s = 11
            else:
                r, s = sym >> 4, sym & 15
                if s:
                    k_at = k + r
                    if k_at > 63:
                        if strict:
                            fault = "run_past_63"
                            break
                        s, ends = 0, True
                    elif s > 10:
                        if strict:
                            fault = "category"
                            break
                        s = 10
                elif r == 15:
                    k_at = k + 15
                    if k_at > 63:
                        if strict:
                            fault = "run_past_63"
                            break
                        ends = True
                elif r == 0:
                    ends = True
                else:
                    if strict:
                        fault = "bad_symbol"
                        break
                    ends = True
            nxt, value = behind, 0
            if s:
                if o + length + s < 32:
                    v = (win[0] >> (64 - o - length - s)) & ((1 << s) - 1)
                    nxt = self._advance(win, p, length + s)
                else:
                    w2 = self._window(behind)
                    v = (w2[0] >> (64 - (behind & 7) - s)) & ((1 << s) - 1)
                    nxt = self._advance(w2, behind, s)
                if nxt > self.total_bits:
                    fault, p = "exhausted", self.total_bits
                    break
                value = _extend(v, s)
            p = nxt
            if k == 0:
                cur = first_block + n_begin
                n_begin += 1
                sums[c] = (sums[c] + value) % 2 ** 32
                if strict:
                    dcv[c] = ((dcv[c] + value + 2 ** 31) % 2 ** 32) - 2 ** 31
                    if not -2047 <= dcv[c] <= 2047:
                        fault = "dc_range"
                        break
                    if cur < self.total_blocks:
                        coef[cur, 0] = dcv[c]
                k = 1
            elif not ends:
                if strict and s and 0 <= cur < self.total_blocks:
                    coef[cur, JR.ZIGZAG[k_at]] = value
                k = k_at + 1
                ends = k > 63
            if ends:
                k, b = 0, (b + 1 if b + 1 < self.blocks else 0)
        if strict and fault is None and p >= self.total_bits and k > 0 and 0 <= cur < self.total_blocks:
            fault = "exhausted"
        return (p, b, k), n_begin, sums, (fault if strict else None)

    # ---- the serial lenient decode and the fixed point ----
    def serial_entries(self) -> list:
        """The state of the serial lenient decode at the first symbol boundary at or behind every subsequence's start."""
        out = [(0, 0, 0)]
        for i in range(self.n_subs - 1):
            out.append(self.lane(i, out[-1])[0])
        return out

    def fixed_point(self):
        """(entries, lane results, rounds): every lane decodes from a guess, hands its exit on, and decodes again
        while its entry changes.  A lane's result depends on its entry alone, so it is computed once per entry."""
        entries = [(0, 0, 0)] + [self.guess(i) for i in range(1, self.n_subs)]
        memo = {}

        def run(i):
            key = (i, entries[i])
            if key not in memo:
                memo[key] = self.lane(i, entries[i])
            return memo[key]

        results = [run(i) for i in range(self.n_subs)]
        changed = set(range(self.n_subs))
        rounds = 1
        while True:
            nxt = set()
            for i in sorted(changed):
                if i + 1 < self.n_subs and results[i][0] != entries[i + 1]:
                    nxt.add(i + 1)
            if not nxt:
                return entries, results, rounds
            for i in sorted(nxt, reverse=True):                        # all hand-offs of a round use the last round's exits
                entries[i] = results[i - 1][0]
            for i in nxt:
                results[i] = run(i)
            changed = nxt
            rounds += 1

    def sums(self, results):
        """The exclusive sums: per subsequence (first block, three DC predictions mod 2^32), and the blocks begun in all."""
        rows, acc = [], [0, 0, 0, 0]
        for _, n_begin, dcs, _ in results:
            rows.append(tuple(acc))
            acc = [(acc[0] + n_begin) % 2 ** 32] + [(acc[1 + c] + dcs[c]) % 2 ** 32 for c in range(3)]
        return rows, acc[0]

    def decode(self):
        """(coefficients (total_blocks, 64) undequantised in natural order, verdict name, entries, sums' rows, rounds)."""
        entries, results, rounds = self.fixed_point()
        rows, begun = self.sums(results)
        coef = np.zeros((self.total_blocks, 64), np.int64)
        faults = []
        for i in range(self.n_subs):
            fault = self.lane(i, entries[i], True, rows[i][0], rows[i][1:], coef)[3]
            if fault:
                faults.append((i << REASON_BITS) | JR.R[fault])
        if begun < self.total_blocks:
            faults.append((self.n_subs << REASON_BITS) | JR.R["exhausted"])
        verdict = JR.REJECT[min(faults) & ((1 << REASON_BITS) - 1)] if faults else "ok"
        return coef, verdict, entries, rows, rounds

    def dequantised(self, coef: np.ndarray) -> np.ndarray:
        """(n_mcus, blocks, 64) as tests/jpegdec_ref.py's decode_coefficients gives them."""
        out = coef.reshape(self.hd["n_mcus"], self.blocks, 64).copy()
        unzig = np.zeros(64, np.int64)
        unzig[JR.ZIGZAG] = np.arange(64)
        for blk in range(self.blocks):
            c = 0 if blk < self.luma else blk - self.luma + 1
            out[:, blk] *= np.asarray(self.quant[c], np.int64)[unzig]
        return out


def entry_rows(data: bytes, sub_bytes: int) -> np.ndarray:
    """uint32 (subsequences, 8): tf_jpegdec_par_entries' rows from the serial decode -- the position's low and high word,
    the block within the MCU, k, the first block's number and the three DC predictions."""
    ps = ParScan(data, sub_bytes)
    entries = ps.serial_entries()
    results = [ps.lane(i, entries[i]) for i in range(ps.n_subs)]
    rows, _ = ps.sums(results)
    out = np.zeros((ps.n_subs, 8), np.uint32)
    for i, ((p, b, k), row) in enumerate(zip(entries, rows)):
        out[i] = [p & 0xFFFFFFFF, p >> 32, b, k, row[0], row[1], row[2], row[3]]
    return out


def verdict(data: bytes, sub_bytes: int) -> str:
    """The reject name the device gives the file in scan mode 1."""
    try:
        hd = JR.parse_header(data)
        if hd["restart_mcus"]:
            return JR.verdict(data)
        return ParScan(data, sub_bytes).decode()[1]
    except JR.Rejected as e:
        return e.reason
