"""The corpus of the banded-PNG decoder: valid indexed files from both builders -- tests/png_ref's
restatement of the device encoder with the index put in, and zlib full-flush files with forced filter types
(tests/pngdec_ref.build) -- files that are well formed but not for the device, and malformed and hostile files with the
reason each must be rejected for.  Everything is made by this repository's own code, zlib and Pillow, once per process.
"""
from __future__ import annotations

import io
import struct
import zlib

import numpy as np

from tests import flowunzip_ref as U
from tests import png_ref as P
from tests import pngdec_ref as D

MARCH = D.MARCH_ROWS


def plan_random(height: int, seed: int) -> list:
    return [int(v) % 5 for v in P._hash(seed, height)]


def ties_image() -> np.ndarray:
    """8 x 12: flat areas (every Paeth distance equal: a = b = c), steps along x and along y (pa = pb, pb = pc,
    pa = pc in turn) and pairs that add up beyond 255 for Average."""
    image = np.zeros((8, 12, 3), np.uint8)
    image[:, :] = 200
    image[2:5, 3:9] = (250, 10, 130)
    image[5:, :6] = (10, 250, 128)
    image[1, :] = np.arange(12, dtype=np.uint8)[:, None] * 20
    image[6, 6:] = (255, 255, 1)
    image[3:7, 9, 0] = (60, 100, 140, 180)
    image[3:7, 10, 0] = (100, 140, 180, 220)
    image[3:7, 11, 1] = (90, 60, 30, 0)
    return image


def far_match_file() -> tuple:
    """700 x 17, band_rows 16, every row None: band 0 is 33616 bytes, more than the 32 KB ring, coded by hand as a stored
    block of its first 32600 bytes and a fixed block that begins with a match of 258 at distance 32600 (zlib never
    reaches back more than 32506)."""
    h, w, rows = 17, 700, 16
    image = P.noise_image(h, w, 91)
    stream = D.filter_rows(image, [0] * h)
    flat = stream[:rows].reshape(-1).copy()
    flat[32600:32858] = flat[0:258]
    stream[:rows] = flat.reshape(rows, -1)
    image = np.ascontiguousarray(stream[:, 1:]).reshape(h, w, 3)
    wr = U.BitWriter()
    wr.bits(0, 3).align().bits(32600, 16).bits(32600 ^ 0xFFFF, 16).raw(flat[:32600].tobytes())
    U.fixed_block(wr, [(258, 32600)] + [int(v) for v in flat[32858:]])
    band0 = wr.end_band().bytes()
    return D.build(image, rows, filters=0, bands={0: band0}), image


_made = {}


def _valid() -> dict:
    out = {}

    def zl(name, image, band_rows, filters, **kw):
        out["zlib." + name] = (D.build(image, band_rows, filters=filters, **kw), image)

    # geometry: widths where 3 W + 1 takes every residue mod 4, the trip edge, the window's edge
    for k, w in enumerate((1, 2, 3, 4, 21, 22, 85, 86, 341, 342)):
        zl(f"{w}x5_random_b2", P.noise_image(5, w, 30 + k), 2, plan_random(5, 60 + k))
    zl("700x33_random_b16", P.noise_image(33, 700, 41), 16, plan_random(33, 71))
    out["hand.700x17_far_b16"] = far_match_file()
    # heights around the rows the unfilter kernel marches together, all Paeth: one segment
    for h, rows in ((1, 1), (2, 2), (MARCH - 1, 1), (MARCH, MARCH), (MARCH + 1, 2), (2 * MARCH + 1, 7)):
        zl(f"5x{h}_paeth_b{rows}", P.noise_image(h, 5, 80 + h), rows, 4)
    zl(f"3x{2 * MARCH + 1}_average_b{MARCH}", P.noise_image(2 * MARCH + 1, 3, 95), MARCH, 3)
    # filter plans on noise and on the crafted image
    noise = P.noise_image(24, 40, 11)
    for t, name in enumerate(("none", "sub", "up", "average", "paeth")):
        zl(f"40x24_{name}_b5", noise, 5, t)
        zl(f"12x8_ties_{name}_b3", ties_image(), 3, t)
    zl("40x24_none_paeth_b5", noise, 5, [0, 4] * 12)
    zl("40x24_none_then_paeth_b5", noise, 5, [0] + [4] * 23)
    zl("40x24_random_b5", noise, 5, plan_random(24, 5))
    zl("40x24_random_b24", noise, 24, plan_random(24, 6))
    zl("40x24_chosen_b1", noise, 1, None)
    # what zlib's levels and headers make of a band: stored blocks, fixed codes, other headers
    zl("40x24_stored_b5", noise, 5, plan_random(24, 7), level=0, header=b"\x78\x01")
    zl("40x24_fixed_b5", P.smear_image(24, 40, 4, 8, 3), 5, plan_random(24, 8), level=9, strategy=zlib.Z_FIXED, header=b"\x78\xda")
    zl("300x40_smear_b7", P.smear_image(40, 300, 8, 50, 8), 7, None, level=9, header=b"\x48\x0d")
    # the device encoder's files, as tests/png_ref restates them, with the index put in
    for name in ("1x1", "1x21", "1x22", "7x1", "24x40_noise_b1", "24x40_noise_b5", "24x40_noise_b1000", "9x50_black_b3",
                 "40x300_smear", "4x85_tail_b2", "4x21_noise_b4"):
        image, band_rows = P.case(name)
        rows = min(image.shape[0], band_rows if band_rows else P.default_band_rows(*image.shape[:2]))
        out["enc." + name] = (D.with_index(P.encode(image, band_rows), rows), image)
    return out


def _pillow_png(image: np.ndarray, mode=None, **kw) -> bytes:
    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(image, mode).save(buf, format="PNG", **kw)
    return buf.getvalue()


def _host() -> dict:
    """name -> (file, why_not): well-formed files that are not for the device."""
    noise = P.noise_image(9, 14, 17)
    out = {"pillow_rgb": (_pillow_png(noise), "no_index"),
           "encoder_without_index": (P.encode(noise, 2), "no_index"),
           "rgba": (_pillow_png(np.dstack([noise, noise[:, :, :1]])), "format"),
           "grey16": (_pillow_png((noise[:, :, 0].astype(np.uint16) * 257)), "format"),
           "interlaced": (D.adam7(noise), "interlaced")}
    future = D.build(noise, 2, filters=1)
    out["index_version_2"] = (D.rechunk(future, lambda c: [(k, b"\x02" + p[1:]) if k == D.INDEX_TYPE else (k, p) for k, p in c]), "version")
    return out


def _bound() -> dict:
    """name -> (file, image): indexed files that ask more of the device than an untrusted file may (the Python side
    sends them the host's way): a band of more than 1 MiB, a band of four bytes behind 250 empty stored blocks."""
    black = P.black_image(500, 700)
    tiny = P.noise_image(2, 1, 5)
    rows = D.filter_rows(tiny, [0, 0])
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    padded = b"\x00\x00\x00\xff\xff" * 250 + c.compress(rows[0].tobytes()) + c.flush(zlib.Z_FULL_FLUSH)
    return {"band_over_1mib": (D.build(black, 500, filters=2), black),
            "band_of_many_blocks": (D.build(tiny, 1, filters=0, bands={0: padded}), tiny)}


def _flip_crc(data: bytes, chunk: int) -> bytes:
    at = 8
    for _ in range(chunk):
        at += 12 + struct.unpack(">I", data[at:at + 4])[0]
    end = at + 12 + struct.unpack(">I", data[at:at + 4])[0]
    return data[:end - 1] + bytes([data[end - 1] ^ 0x10]) + data[end:]


def _raw_band(data: bytes, final: bool = False, flush=zlib.Z_FULL_FLUSH) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush(zlib.Z_FINISH if final else flush)


def _malformed() -> dict:
    """name -> (file, reason, where or None, whether `walk` alone finds it)."""
    image = P.noise_image(12, 10, 51)
    plan = plan_random(12, 52)
    good = D.build(image, 5, filters=plan)            # chunks: IHDR, tfBX, IDAT header, 3 bands (2 - 4 ... ), tail, IEND
    rows = D.filter_rows(image, plan)
    out = {}

    def probe(name, data, reason):
        out[name] = (bytes(data), reason, None, True)

    def device(name, data, reason, where=None):
        out[name] = (bytes(data), reason, where, False)

    def edit(fn):
        return D.rechunk(good, fn)

    probe("signature", b"\x89PNX" + good[4:], "signature")
    probe("empty", b"", "signature")
    probe("truncated_in_band", good[:150], "truncated")
    probe("truncated_in_crc", good[:-2], "truncated")
    probe("length_beyond_file", good[:8] + struct.pack(">I", 0x7FFFFFF0) + good[12:], "truncated")
    probe("no_ihdr", edit(lambda c: c[1:]), "ihdr")
    probe("ihdr_of_12", edit(lambda c: [(c[0][0], c[0][1][:12])] + c[1:]), "ihdr")
    probe("ihdr_depth_3", edit(lambda c: [(c[0][0], c[0][1][:8] + b"\x03" + c[0][1][9:])] + c[1:]), "ihdr")
    probe("ihdr_interlace_2", edit(lambda c: [(c[0][0], c[0][1][:12] + b"\x02")] + c[1:]), "ihdr")
    probe("zero_width", edit(lambda c: [(c[0][0], struct.pack(">I", 0) + c[0][1][4:])] + c[1:]), "size")
    probe("width_2_to_24", edit(lambda c: [(c[0][0], struct.pack(">I", 1 << 24) + c[0][1][4:])] + c[1:]), "size")
    probe("beyond_2_to_31_bytes", edit(lambda c: [(c[0][0], struct.pack(">II", 1 << 20, 1 << 20) + c[0][1][8:])] + c[1:]), "size")
    probe("index_one_band_more", D.build(image, 5, filters=plan, index=D.index_chunk(5, 4)), "index")
    probe("index_one_band_fewer", D.build(image, 5, filters=plan, index=D.index_chunk(5, 2)), "index")
    probe("index_band_rows_0", D.build(image, 5, filters=plan, index=D.index_chunk(0, 3)), "index")
    probe("index_flags", D.build(image, 5, filters=plan, index=D.index_chunk(5, 3, flags=1)), "index")
    probe("index_of_8_bytes", edit(lambda c: [(k, p[:8]) if k == D.INDEX_TYPE else (k, p) for k, p in c]), "index")
    probe("index_twice", edit(lambda c: c[:2] + [c[1]] + c[2:]), "index")
    probe("index_behind_idat", edit(lambda c: [c[0]] + c[2:-1] + [c[1], c[-1]]), "index")
    probe("an_idat_missing", edit(lambda c: c[:4] + c[5:]), "index")
    probe("zlib_header_check_bits", edit(lambda c: c[:2] + [(b"IDAT", b"\x78\x02")] + c[3:]), "zlib_header")
    probe("zlib_header_dictionary", edit(lambda c: c[:2] + [(b"IDAT", b"\x78\xbb")] + c[3:]), "zlib_header")
    probe("zlib_header_method_7", edit(lambda c: c[:2] + [(b"IDAT", b"\x77\x05")] + c[3:]), "zlib_header")
    probe("zlib_header_window_64k", edit(lambda c: c[:2] + [(b"IDAT", b"\x88\x1c")] + c[3:]), "zlib_header")
    probe("zlib_header_of_3_bytes", edit(lambda c: c[:2] + [(b"IDAT", b"\x78\x9c\x00")] + c[3:]), "zlib_header")
    probe("tail_not_final", D.build(image, 5, filters=plan, tail=b"\x00\x00\x00\xff\xff"), "tail")
    probe("tail_with_data", D.build(image, 5, filters=plan, tail=b"\x01\x01\x00\xfe\xff\x2a"), "tail")
    probe("tail_with_more_behind", D.build(image, 5, filters=plan, tail=b"\x03\x00\x00"), "tail")
    probe("tail_of_4_bytes", edit(lambda c: c[:-2] + [(b"IDAT", c[-2][1][-4:])] + c[-1:]), "tail")
    probe("no_iend", edit(lambda c: c[:-1]), "no_iend")
    probe("iend_with_payload", edit(lambda c: c[:-1] + [(b"IEND", b"\0")]), "no_iend")
    probe("data_behind_iend", good + b"\0", "no_iend")
    probe("chunk_behind_iend", good + P.chunk(b"tEXt", b"a\0b"), "no_iend")
    probe("idats_not_consecutive", edit(lambda c: c[:4] + [(b"tEXt", b"a\0b")] + c[4:]), "idat_order")
    probe("no_idat", edit(lambda c: [x for x in c if x[0] != b"IDAT"]), "idat_order")

    device("crc_of_band_1", _flip_crc(good, 4), "chunk_crc", 4)
    device("crc_of_ihdr", _flip_crc(good, 0), "chunk_crc", 0)
    device("crc_of_tail", _flip_crc(good, 6), "chunk_crc", 6)
    device("adler", D.build(image, 5, filters=plan, adler=zlib.adler32(rows.tobytes()) ^ 0x100), "adler")
    for row in (0, 6, 11):
        device(f"filter_5_row_{row}", D.build(image, 5, filters=plan[:row] + [5] + plan[row + 1:]), "filter_type", row)
    device("band_1_short", D.build(image, 5, filters=plan, bands={1: _raw_band(rows[5:9].tobytes())}), "band_short", 1)
    device("band_1_over", D.build(image, 5, filters=plan, bands={1: _raw_band(rows[5:11].tobytes())}), "band_overrun", 1)
    device("band_2_bfinal", D.build(image, 5, filters=plan, bands={2: _raw_band(rows[10:].tobytes(), final=True)}), "band_bfinal", 2)
    # an index whose band_rows agrees with the height and the count but not with the bands: only the bands can tell
    device("index_other_band_rows", D.build(image, 5, filters=plan, index=D.index_chunk(4, 3)), "band_overrun", 0)
    device("band_0_empty", D.build(image, 5, filters=plan, bands={0: b""}), "band_short", 0)
    device("band_0_cut", D.build(image, 5, filters=plan, bands={0: _raw_band(rows[:5].tobytes())[:40]}), "band_exhausted", 0)
    # a band that reaches back into the band before it: two bands of the same bytes, the first flushed with Z_SYNC_FLUSH
    flat = np.repeat(P.noise_image(1, 10, 53), 4, axis=0)
    device("band_1_distance", D.build(flat, 2, filters=0, flush={0: zlib.Z_SYNC_FLUSH}), "band_distance", 1)
    return out


def valid() -> dict:
    """name -> (file, image)."""
    if "valid" not in _made:
        _made["valid"] = _valid()
    return _made["valid"]


def host() -> dict:
    if "host" not in _made:
        _made["host"] = _host()
    return _made["host"]


def bound() -> dict:
    if "bound" not in _made:
        _made["bound"] = _bound()
    return _made["bound"]


def malformed() -> dict:
    if "malformed" not in _made:
        _made["malformed"] = _malformed()
    return _made["malformed"]
