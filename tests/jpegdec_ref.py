"""The device JPEG decoder's rules, restated in numpy (transflow_amd/csrc/jpegdec_common.h, jpegdec.hip; DESIGN.md
section 19): which files are taken, why the others are rejected, and libjpeg's arithmetic for the pixels -- jdhuff.c's
decoding, jidctint.c's islow IDCT, jdsample.c's upsampling (fancy, or replicating for a frame up to 4 pixels wide) with
jdmainct.c's edge rows, jdcolor.c's tables.
tests/test_jpegdec_ref.py holds it equal to Pillow; the GPU tests and tools/jpegdec_host_check.cpp are held equal to it.
"""
from __future__ import annotations

import zlib

import numpy as np

# jpegdec_common.h's Reject, name for name
REJECT = ["ok", "not_jpeg", "truncated", "bad_segment", "progressive", "arithmetic", "sof_kind", "precision", "components",
          "sampling", "multi_scan", "dnl", "adobe_transform", "dqt_16bit", "missing_table", "bad_dht", "no_eoi",
          "stray_marker", "rst_count", "rst_order", "bad_code", "bad_symbol", "run_past_63", "category", "dc_range",
          "exhausted"]
R = {name: i for i, name in enumerate(REJECT)}

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Rejected(Exception):
    def __init__(self, reason: str):
        Exception.__init__(self, reason)
        self.reason = reason


def build_huff(counts, vals, is_dc: bool) -> dict:
    """{(length, code): symbol}; Rejected("bad_dht") as build_huff of jpegdec_common.h."""
    total = sum(counts)
    if total > 256 or total > len(vals):
        raise Rejected("bad_dht")
    if is_dc and any(v > 15 for v in vals[:total]):
        raise Rejected("bad_dht")
    table, code, p = {}, 0, 0
    for length in range(1, 17):
        n = counts[length - 1]
        if n and code + n >= (1 << length):         # a code that does not fit, or all ones
            raise Rejected("bad_dht")
        for k in range(n):
            table[(length, code + k)] = vals[p + k]
        p += n
        code = (code + n) << 1
    return table


def parse_header(data: bytes) -> dict:
    """The segments up to SOS (parse_header of jpegdec_common.h, check for check)."""
    n = len(data)
    if n < 2:
        raise Rejected("truncated" if n == 0 or data[0] == 0xFF else "not_jpeg")
    if data[0] != 0xFF or data[1] != 0xD8:
        raise Rejected("not_jpeg")
    q, dc, ac = {}, {}, {}
    sof = None
    restart = 0
    at = 2
    while True:
        if n - at < 2:
            raise Rejected("truncated")
        if data[at] != 0xFF:
            raise Rejected("bad_segment")
        marker = data[at + 1]
        if marker == 0xFF:
            at += 1
            continue
        at += 2
        if marker == 0xD9:
            raise Rejected("truncated")
        if marker in (0xD8, 0x01, 0x00) or 0xD0 <= marker <= 0xD7:
            raise Rejected("bad_segment")
        if n - at < 2:
            raise Rejected("truncated")
        length = int.from_bytes(data[at:at + 2], "big")
        if length < 2:
            raise Rejected("bad_segment")
        if n - at < length:
            raise Rejected("truncated")
        p = data[at + 2:at + length]
        m = len(p)
        at += length
        if 0xC0 <= marker <= 0xCF and marker not in (0xC4, 0xC8, 0xCC):
            if marker == 0xC2:
                raise Rejected("progressive")
            if marker >= 0xC9:
                raise Rejected("arithmetic")
            if marker != 0xC0:
                raise Rejected("sof_kind")
            if sof is not None or m < 6:
                raise Rejected("bad_segment")
            if p[0] != 8:
                raise Rejected("precision")
            height, width, ncomp = int.from_bytes(p[1:3], "big"), int.from_bytes(p[3:5], "big"), p[5]
            if ncomp not in (1, 3):
                raise Rejected("components")
            if m != 6 + 3 * ncomp:
                raise Rejected("bad_segment")
            if height == 0:
                raise Rejected("dnl")
            if width == 0:
                raise Rejected("bad_segment")
            comps = []
            for c in range(ncomp):
                cid, hv, tq = p[6 + 3 * c], p[7 + 3 * c], p[8 + 3 * c]
                hs, vs = hv >> 4, hv & 15
                if tq > 3:
                    raise Rejected("bad_segment")
                if c == 0:
                    ok = (hs, vs) == (1, 1) if ncomp == 1 else (hs, vs) in ((2, 2), (2, 1), (1, 1))
                    if not ok:
                        raise Rejected("sampling")
                elif (hs, vs) != (1, 1):
                    raise Rejected("sampling")
                comps.append((cid, hs, vs, tq))
            sof = dict(width=width, height=height, components=ncomp, h_samp=comps[0][1], v_samp=comps[0][2], comps=comps)
        elif marker == 0xCC:
            raise Rejected("arithmetic")
        elif marker == 0xC4:
            k = 0
            while k < m:
                if m - k < 17:
                    raise Rejected("bad_dht")
                tc, th = p[k] >> 4, p[k] & 15
                if tc > 1 or th > 3:
                    raise Rejected("bad_dht")
                counts = list(p[k + 1:k + 17])
                (ac if tc else dc)[th] = build_huff(counts, list(p[k + 17:]), tc == 0)
                k += 17 + sum(counts)
        elif marker == 0xDB:
            k = 0
            while k < m:
                pq, tq = p[k] >> 4, p[k] & 15
                if pq == 1:
                    raise Rejected("dqt_16bit")
                if pq > 1 or tq > 3 or m - k < 65:
                    raise Rejected("bad_segment")
                q[tq] = np.array(list(p[k + 1:k + 65]), np.int64)       # by zigzag position
                k += 65
        elif marker == 0xDD:
            if m != 2:
                raise Rejected("bad_segment")
            restart = int.from_bytes(p, "big")
        elif marker == 0xDC:
            raise Rejected("dnl")
        elif marker == 0xEE:
            if m >= 12 and p[:5] == b"Adobe" and p[11] != 1:
                raise Rejected("adobe_transform")
        elif marker == 0xDA:
            if sof is None or m < 1:
                raise Rejected("bad_segment")
            ns = p[0]
            if ns != sof["components"]:
                raise Rejected("multi_scan")
            if m != 4 + 2 * ns:
                raise Rejected("bad_segment")
            tables = []
            for c in range(ns):
                if p[1 + 2 * c] != sof["comps"][c][0]:
                    raise Rejected("multi_scan")
                td, ta = p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15
                if td > 3 or ta > 3:
                    raise Rejected("bad_segment")
                tq = sof["comps"][c][3]
                if td not in dc or ta not in ac or tq not in q:
                    raise Rejected("missing_table")
                tables.append((dc[td], ac[ta], q[tq]))
            if p[1 + 2 * ns] != 0 or p[2 + 2 * ns] != 63 or p[3 + 2 * ns] != 0:
                raise Rejected("multi_scan")
            hd = dict(sof)
            hd["restart_mcus"] = restart
            hd["tables"] = tables
            hd["scan_offset"] = at
            mw, mh = 8 * hd["h_samp"], 8 * hd["v_samp"]
            hd["mcus_x"], hd["mcus_y"] = -(-hd["width"] // mw), -(-hd["height"] // mh)
            hd["n_mcus"] = hd["mcus_x"] * hd["mcus_y"]
            hd["blocks_per_mcu"] = 1 if ns == 1 else hd["h_samp"] * hd["v_samp"] + 2
            hd["intervals"] = -(-hd["n_mcus"] // restart) if restart else 1
            return hd
        elif 0xE0 <= marker <= 0xEF or marker == 0xFE:
            pass
        else:
            raise Rejected("bad_segment")


def probe(data: bytes) -> dict:
    """tf_jpegdec_probe: the geometry, or {"reject": name}."""
    try:
        hd = parse_header(data)
    except Rejected as e:
        return {"reject": e.reason}
    out = {k: hd[k] for k in ("width", "height", "components", "h_samp", "v_samp", "restart_mcus", "intervals")}
    out["reject"] = "ok"
    return out


def split_intervals(scan: bytes, expected_markers: int) -> list:
    """The marker scan: the intervals' byte strings, or Rejected with the lowest-numbered fault."""
    n = len(scan)
    faults = set()
    if n < 2 or scan[-2:] != b"\xff\xd9":
        faults.add("no_eoi")
    markers = []
    i = scan.find(b"\xff")
    while i >= 0:
        if i + 1 >= n:
            faults.add("stray_marker")
        else:
            v = scan[i + 1]
            if 0xD0 <= v <= 0xD7:
                if v != 0xD0 + (len(markers) & 7):
                    faults.add("rst_order")
                markers.append(i)
            elif v != 0 and not (i + 2 == n and v == 0xD9):
                faults.add("stray_marker")
        i = scan.find(b"\xff", i + 1)
    if len(markers) != expected_markers:
        faults.add("rst_count")
    if faults:
        raise Rejected(min(faults, key=lambda name: R[name]))
    edges = [0] + [m + 2 for m in markers]
    ends = markers + [n - 2]
    return [scan[a:b] for a, b in zip(edges, ends)]


class _Bits:
    """An interval's bits: FF 00 is FF (the marker scan left no other FF pair)."""

    def __init__(self, data: bytes):
        raw = data.replace(b"\xff\x00", b"\xff")
        if data.endswith(b"\xff") and not data.endswith(b"\xff\x00"):
            raw = raw[:-1]
        self.value = int.from_bytes(raw, "big") if raw else 0
        self.left = 8 * len(raw)

    def peek16(self) -> int:
        if self.left >= 16:
            return (self.value >> (self.left - 16)) & 0xFFFF
        return (self.value << (16 - self.left)) & 0xFFFF

    def take(self, nbits: int) -> int:
        if self.left < nbits:
            raise Rejected("exhausted")
        self.left -= nbits
        return (self.value >> self.left) & ((1 << nbits) - 1)

    def symbol(self, table: dict) -> int:
        bits = self.peek16()
        for length in range(1, 17):
            sym = table.get((length, bits >> (16 - length)))
            if sym is not None:
                if length > self.left:
                    raise Rejected("exhausted")
                self.left -= length
                return sym
        raise Rejected("exhausted" if self.left < 16 else "bad_code")


def _extend(v: int, s: int) -> int:
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v               # HUFF_EXTEND


def decode_block(bits: _Bits, dc: dict, ac: dict, quant, last_dc: int, trace=None):
    """(the new prediction, 64 dequantised coefficients in natural order): decode_block of jpegdec_common.h."""
    coef = np.zeros(64, np.int64)
    s = bits.symbol(dc)
    if s > 11:
        raise Rejected("category")
    diff = _extend(bits.take(s), s) if s else 0
    last_dc += diff
    if not -2047 <= last_dc <= 2047:
        raise Rejected("dc_range")
    coef[0] = last_dc * int(quant[0])
    if trace is not None:
        trace.setdefault("dc_sizes", set()).add(s)
    k = 1
    while k < 64:
        sym = bits.symbol(ac)
        r, s = sym >> 4, sym & 15
        if trace is not None:
            trace.setdefault("ac_symbols", []).append(sym)
        if s:
            k += r
            if k > 63:
                raise Rejected("run_past_63")
            if s > 10:
                raise Rejected("category")
            coef[ZIGZAG[k]] = _extend(bits.take(s), s) * int(quant[k])
        elif r == 15:
            k += 15
            if k > 63:
                raise Rejected("run_past_63")
        elif r == 0:
            break
        else:
            raise Rejected("bad_symbol")
        k += 1
    return last_dc, coef


# ---- jidctint.c jpeg_idct_islow ------------------------------------------------------------------------------------
def _idct_pass(v, shift: int):
    """One pass along the last axis of (..., 8) int64."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (v[..., i] for i in range(8))
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 + i6 * -15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    s1, s2, s3, s4 = i7 + i1, i5 + i3, i7 + i3, i5 + i1
    z5 = (s3 + s4) * 9633
    o0, o1, o2, o3 = i7 * 2446, i5 * 16819, i3 * 25172, i1 * 12299
    z1, z2, z3, z4 = s1 * -7373, s2 * -20995, s3 * -16069 + z5, s4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    half = 1 << (shift - 1)
    out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return np.stack([(x + half) >> shift for x in out], axis=-1)


def idct_islow(coef: np.ndarray) -> np.ndarray:
    """(..., 64) dequantised coefficients in natural order -> (..., 8, 8) uint8 samples."""
    c = coef.reshape(coef.shape[:-1] + (8, 8)).astype(np.int64)
    ws = np.swapaxes(_idct_pass(np.swapaxes(c, -1, -2), 11), -1, -2)   # columns: CONST_BITS - PASS1_BITS
    x = _idct_pass(ws, 18) & 1023                                       # rows: CONST_BITS + PASS1_BITS + 3
    return np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896))).astype(np.uint8)


# ---- jdsample.c ----------------------------------------------------------------------------------------------------
def _h2v1(p: np.ndarray, dw: int, width: int) -> np.ndarray:
    """p: (rows, >= max(dw, 2)) int64 -> (rows, width)."""
    x = np.arange(width)
    c = x >> 1
    odd = (x & 1) == 1
    cur, prev, nxt = p[:, c], p[:, np.maximum(c - 1, 0)], p[:, np.minimum(c + 1, p.shape[1] - 1)]
    mid = np.where(odd, (cur * 3 + nxt + 2) >> 2, (cur * 3 + prev + 1) >> 2)
    last = np.where(odd, cur, (cur * 3 + prev + 1) >> 2)
    first = np.where(odd, (cur * 3 + nxt + 2) >> 2, cur)
    return np.where(c == 0, first, np.where(c == dw - 1, last, mid))


def _h2v2(p: np.ndarray, dw: int, dh: int, width: int, height: int) -> np.ndarray:
    y = np.arange(height)
    row = y >> 1
    other = np.where(y & 1, np.minimum(row + 1, dh - 1), np.maximum(row - 1, 0))    # jdmainct.c: the edge rows repeat
    s = p[row] * 3 + p[other]                                                       # the column sums, per output row
    x = np.arange(width)
    c = x >> 1
    odd = (x & 1) == 1
    cur, prev, nxt = s[:, c], s[:, np.maximum(c - 1, 0)], s[:, np.minimum(c + 1, s.shape[1] - 1)]
    mid = np.where(odd, (cur * 3 + nxt + 7) >> 4, (cur * 3 + prev + 8) >> 4)
    last = np.where(odd, (cur * 4 + 7) >> 4, (cur * 3 + prev + 8) >> 4)
    first = np.where(odd, (cur * 3 + nxt + 7) >> 4, (cur * 4 + 8) >> 4)
    return np.where(c == 0, first, np.where(c == dw - 1, last, mid))


def _replicated(p: np.ndarray, vs: int, width: int, height: int) -> np.ndarray:
    """h2v1_upsample / h2v2_upsample: every chroma sample is the pixel's own, no neighbour and no context row."""
    return p[(np.arange(height) >> (vs - 1))[:, None], (np.arange(width) >> 1)[None, :]]


def _upsampled(p: np.ndarray, hs: int, vs: int, width: int, height: int, narrow_rule: bool = True) -> np.ndarray:
    """A chroma plane of whole MCUs at the picture's size, as jinit_upsampler chooses: the fancy filters only where the
    component's downsampled_width = ceil(W / 2) is above 2, replication otherwise.  narrow_rule=False blends at every
    width: not libjpeg's pixels for W <= 4, kept for the test that shows the corpus tells the two apart."""
    dw, dh = (width + 1) // 2, (height + 1) // 2
    if hs == 1:
        return p[:height, :width]
    if narrow_rule and dw <= 2:
        return _replicated(p, vs, width, height)
    return _h2v1(p[:height], dw, width) if vs == 1 else _h2v2(p, dw, dh, width, height)


def _colour(y, cb, cr):
    """jdcolor.c ycc_rgb_convert with build_ycc_rgb_table's tables (SCALEBITS 16)."""
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode_coefficients(data: bytes, trace=None):
    """(header, (n_mcus, blocks, 64) int64 dequantised coefficients); Rejected otherwise."""
    hd = parse_header(data)
    scan = data[hd["scan_offset"]:]
    if trace is not None:
        trace["ff00"] = scan.count(b"\xff\x00")
    intervals = split_intervals(scan, hd["intervals"] - 1)
    nb = hd["blocks_per_mcu"]
    luma = 1 if hd["components"] == 1 else hd["h_samp"] * hd["v_samp"]
    per = hd["restart_mcus"] or hd["n_mcus"]
    coefs = np.zeros((hd["n_mcus"], nb, 64), np.int64)
    for iv, chunk in enumerate(intervals):
        bits = _Bits(chunk)
        last = [0, 0, 0]
        for m in range(iv * per, min((iv + 1) * per, hd["n_mcus"])):
            for blk in range(nb):
                c = 0 if blk < luma else blk - luma + 1
                dc, ac, q = hd["tables"][c]
                last[c], coefs[m, blk] = decode_block(bits, dc, ac, q, last[c], trace)
    return hd, coefs


def coefficients_crc(coefs: np.ndarray) -> int:
    """CRC-32 of the coefficients as little-endian int32 in decoding order: what tools/jpegdec_host_check prints."""
    return zlib.crc32(coefs.astype("<i4").tobytes()) & 0xFFFFFFFF


def decode(data: bytes, order: str = "rgb", trace=None) -> np.ndarray:
    """uint8 (H, W, 3): the pixels of PIL.Image.open(...).convert("RGB"); Rejected for a file the device does not take."""
    return _decode(data, order, trace)


def _decode_blending_at_every_width(data: bytes) -> np.ndarray:
    """decode() without jinit_upsampler's choice (see _upsampled): for tests/test_jpegdec_ref.py only."""
    return _decode(data, "rgb", None, narrow_rule=False)


def _decode(data: bytes, order: str, trace, narrow_rule: bool = True) -> np.ndarray:
    hd, coefs = decode_coefficients(data, trace)
    W, H, hs, vs = hd["width"], hd["height"], hd["h_samp"], hd["v_samp"]
    mx, my = hd["mcus_x"], hd["mcus_y"]
    samples = idct_islow(coefs).astype(np.int64)                        # (n_mcus, blocks, 8, 8)
    luma = 1 if hd["components"] == 1 else hs * vs
    # the planes of whole MCUs: an MCU's luma blocks are vs rows of hs blocks
    yb = samples[:, :luma].reshape(my, mx, vs, hs, 8, 8)
    yp = yb.transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8)
    y = yp[:H, :W]
    if hd["components"] == 1:
        out = np.stack([y, y, y], axis=-1).astype(np.uint8)
    else:
        planes = [samples[:, luma + i].reshape(my, mx, 8, 8).transpose(0, 2, 1, 3).reshape(my * 8, mx * 8) for i in range(2)]
        cb, cr = (_upsampled(p, hs, vs, W, H, narrow_rule) for p in planes)
        out = _colour(y, cb, cr)
    return out[:, :, ::-1].copy() if order == "bgr" else out


def verdict(data: bytes) -> str:
    """The reject name the device gives the file ("ok" for a file it takes)."""
    try:
        decode_coefficients(data)
    except Rejected as e:
        return e.reason
    return "ok"


# ---- test files ------------------------------------------------------------------------------------------------------
def find_segment(data: bytes, marker: int, start: int = 2):
    """(offset of the FF, length field) of the first segment with `marker` before SOS, or None."""
    at = start
    while at + 4 <= len(data):
        m = data[at + 1]
        length = int.from_bytes(data[at + 2:at + 4], "big")
        if m == marker:
            return at, length
        if m == 0xDA:
            return None
        at += 2 + length
    return None


def index_stream(data: bytes) -> list:
    """(offset, size) of every JPEG file of a raw MJPEG stream: the segments by their lengths to SOS, then the next
    FF D9 (which cannot occur inside a scan)."""
    out, at, n = [], 0, len(data)
    while True:
        at = data.find(b"\xff\xd8", at)
        if at < 0:
            return out
        p = at + 2
        while p + 4 <= n and data[p] == 0xFF and data[p + 1] != 0xDA:
            p += 2 + int.from_bytes(data[p + 2:p + 4], "big")
        if p + 4 > n or data[p] != 0xFF:
            return out
        end = data.find(b"\xff\xd9", p + 2 + int.from_bytes(data[p + 2:p + 4], "big"))
        if end < 0:
            return out
        out.append((at, end + 2 - at))
        at = end + 2
