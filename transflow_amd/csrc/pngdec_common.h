// Banded PNG frames decoded on the device (pngdec.hip): the part that decides what a file is and what is in bounds --
// the chunk walk, the band index, the zlib header and tail, the small chunks' CRCs, the unfilter arithmetic -- as
// host/device inline functions over plain memory.  tf_pngdec_probe and tf_pngdec_decode_dev run the walk on the host;
// tools/pngdec_host_check.cpp runs all of it on the CPU under the sanitizers (DESIGN.md section 20;
// tests/pngdec_ref.py is the Python statement of the same rules, with the same names).
//
// An indexed file is what PngEncoder(index=True) writes: 8-bit RGB, colour type 2, not interlaced;
// IHDR, the ancillary chunk tfBX (version 1, flags 0, 0, band_rows, n_bands; big-endian), an IDAT that holds the two
// bytes of a zlib header, n_bands IDATs that each hold one band -- non-final deflate blocks that end on a byte and
// inflate, on their own, to the band's rows of the filtered stream -- an IDAT with an empty final block and the
// Adler-32, IEND.  The walk verifies exactly that; the bands themselves are verified where they are inflated
// (flowunzip_common.h's machine, one wave per band).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "crc32_common.h"
#include "flowunzip_common.h"

#define PD_HD FU_HD

namespace tf {
namespace pngdec {

// why a file was rejected (0: it was not); the names are tests/pngdec_ref.py's.  A reject word is reason | where << 8:
// `where` is the chunk (R_CHUNK_CRC; IHDR is chunk 0), the row (R_FILTER_TYPE) or the band (R_BAND + ...), else 0.
enum Reject : uint32_t {
    R_OK = 0,
    R_SIGNATURE = 1,   // not the eight bytes of a PNG
    R_TRUNCATED = 2,   // a chunk that is cut short or reaches beyond the file
    R_IHDR = 3,        // IHDR missing, not 13 bytes, or with values the specification does not allow
    R_SIZE = 4,        // a zero dimension; a dimension beyond MAX_DIM or the handle; more than 2^31 filtered bytes
    R_INDEX = 5,       // tfBX misplaced, twice, of a wrong size, or at odds with the height or with the IDATs
    R_ZLIB_HEADER = 6, // the first IDAT is not a valid two-byte zlib header (CM 8, window <= 32 K, no dictionary)
    R_TAIL = 7,        // the last IDAT is not an empty final block that ends the stream, and four bytes
    R_NO_IEND = 8,     // no IEND, IEND with a payload, or bytes behind it
    R_IDAT_ORDER = 9,  // IDATs that are not consecutive, or none
    R_CHUNK_CRC = 10,  // a chunk whose CRC-32 differs
    R_ADLER = 11,      // the filtered stream's Adler-32 differs from the trailer
    R_FILTER_TYPE = 12, // a row whose filter type is not 0 - 4
    R_BAND = 16,       // R_BAND + flowunzip::Reject: why a band is no valid band
    R_COUNT = R_BAND + flowunzip::R_EXHAUSTED + 1,
};

// why a well-formed file is not for the device (0: it is)
enum NotDevice : uint32_t { N_INDEXED = 0, N_NO_INDEX = 1, N_FORMAT = 2, N_INTERLACED = 3, N_VERSION = 4 };

constexpr uint32_t MAX_DIM = (1u << 24) - 1;        // a row or band number fits a reject word's 24 bits
constexpr uint64_t MAX_STREAM = 1ull << 31;         // filtered bytes
constexpr uint32_t INDEX_BYTES = 12;
constexpr uint32_t MARCH_ROWS = 64;                 // the rows the unfilter kernel marches together: a wave's lanes

PD_HD uint32_t make_reject(uint32_t reason, uint32_t where) { return reason | (where << 8); }

PD_HD const char *reject_name(uint32_t reject)
{
    switch (reject & 0xFFu) {
    case R_OK: return "ok";
    case R_SIGNATURE: return "signature";
    case R_TRUNCATED: return "truncated";
    case R_IHDR: return "ihdr";
    case R_SIZE: return "size";
    case R_INDEX: return "index";
    case R_ZLIB_HEADER: return "zlib_header";
    case R_TAIL: return "tail";
    case R_NO_IEND: return "no_iend";
    case R_IDAT_ORDER: return "idat_order";
    case R_CHUNK_CRC: return "chunk_crc";
    case R_ADLER: return "adler";
    case R_FILTER_TYPE: return "filter_type";
    case R_BAND + flowunzip::R_BFINAL: return "band_bfinal";
    case R_BAND + flowunzip::R_BTYPE: return "band_btype";
    case R_BAND + flowunzip::R_STORED_LEN: return "band_stored_len";
    case R_BAND + flowunzip::R_BAD_CODE: return "band_bad_code";
    case R_BAND + flowunzip::R_REPEAT_FIRST: return "band_repeat_first";
    case R_BAND + flowunzip::R_REPEAT_PAST: return "band_repeat_past";
    case R_BAND + flowunzip::R_BAD_SYMBOL: return "band_bad_symbol";
    case R_BAND + flowunzip::R_DISTANCE: return "band_distance";
    case R_BAND + flowunzip::R_OVERRUN: return "band_overrun";
    case R_BAND + flowunzip::R_SHORT: return "band_short";
    case R_BAND + flowunzip::R_EXHAUSTED: return "band_exhausted";
    default: return "unknown";
    }
}

// what the walk found.  Offsets are from the file's first byte; a file is at most 2^32 - 1 bytes.
struct Layout {
    uint32_t width, height;
    uint32_t band_rows, n_bands;
    uint32_t indexed, why_not;
    uint32_t n_chunks;         // IEND included
    uint32_t first_band_chunk; // the chunk number of band 0's IDAT
    uint32_t first_band_at;    // where that chunk begins (its length field)
    uint32_t max_band_bytes;   // the largest band's compressed bytes
    uint32_t adler;            // the trailer
};

PD_HD uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

PD_HD bool is_type(const uint8_t *p, const char *name) { return p[0] == (uint8_t)name[0] && p[1] == (uint8_t)name[1] && p[2] == (uint8_t)name[2] && p[3] == (uint8_t)name[3]; }

PD_HD uint64_t row_bytes(uint32_t width) { return 1 + 3 * (uint64_t)width; }

// the rows of band b, and its bytes of the filtered stream (b < n_bands, band_rows >= 1)
PD_HD uint32_t band_row_count(const Layout &l, uint32_t b)
{
    const uint64_t first = (uint64_t)b * l.band_rows;
    return (uint32_t)(l.height - first < l.band_rows ? l.height - first : l.band_rows);
}

// A zlib stream's first two bytes (RFC 1950): CM 8, a window of at most 32 K, no preset dictionary, FCHECK right.
PD_HD bool zlib_header_ok(uint32_t cmf, uint32_t flg)
{
    return (cmf & 15u) == 8 && (cmf >> 4) <= 7 && (flg & 0x20u) == 0 && ((cmf << 8) | flg) % 31 == 0;
}

// The deflate data behind the last band: one final block that makes no byte and ends in the data's last byte
// (what zlib.decompressobj(-15) takes to its end with nothing made and nothing left over).
PD_HD bool empty_final_block(const uint8_t *p, uint32_t size, flowunzip::Code &lit, flowunzip::Code &dist, uint8_t *lengths)
{
    using namespace flowunzip;
    Bits b;
    b.win = p, b.win_base = 0, b.win_len = size, b.size = size, b.next = 0, b.buf = 0, b.cnt = 0;
    uint32_t v = 0, sym = 0;
    if (!take(b, 3, v) || !(v & 1u))
        return false;
    const uint32_t type = v >> 1;
    if (type == 0) {
        uint32_t len = 0, src = 0;
        if (read_stored(b, len, src) != flowunzip::R_OK || len != 0)
            return false;
        return src == size;
    }
    if (type == 1)
        build_fixed(lit, dist, lengths);
    else if (type != 2 || read_dynamic(b, lit, dist, lengths) != flowunzip::R_OK)
        return false;
    if (decode(b, lit, sym) != flowunzip::R_OK || sym != 256)
        return false;
    return (bits_consumed(b) + 7) / 8 == size;
}

// ---- the walk --------------------------------------------------------------------------------------------------------
// Fills `l`; returns R_OK for an indexed file and for one that is not for the device (l.indexed says which), else the
// reason.  max_width / max_height: the caller's bounds (MAX_DIM at the most).  band_offsets / band_sizes: where each
// band's compressed bytes begin and how many they are, for the first `capacity` bands (null with capacity 0).
// Every length is compared with what the file has left before it is used; no sum can pass 2^64.
PD_HD uint32_t walk(const uint8_t *file, size_t n, uint32_t max_width, uint32_t max_height, Layout &l, uint32_t *band_offsets,
                    uint32_t *band_sizes, size_t capacity, flowunzip::Code &lit, flowunzip::Code &dist, uint8_t *lengths)
{
    l.width = l.height = l.band_rows = l.n_bands = l.indexed = l.why_not = 0;
    l.n_chunks = l.first_band_chunk = l.first_band_at = l.max_band_bytes = l.adler = 0;
    if (n < 8 || file[0] != 0x89 || file[1] != 'P' || file[2] != 'N' || file[3] != 'G' || file[4] != '\r' || file[5] != '\n' ||
        file[6] != 0x1A || file[7] != '\n')
        return R_SIGNATURE;
    if (n > 0xFFFFFFFFull)
        return R_SIZE;
    size_t at = 8;
    uint32_t chunk = 0, n_idat = 0, first_idat_chunk = 0, n_index = 0;
    size_t first_idat_at = 0, last_idat_at = 0, index_at = 0;
    bool idat_closed = false, index_late = false, index_size_ok = false, ended = false;
    while (at < n) {
        if (n - at < 12)
            return R_TRUNCATED;
        const uint32_t len = be32(file + at);
        if (len > n - at - 12)
            return R_TRUNCATED;
        const uint8_t *type = file + at + 4;
        if (chunk == 0 && (!is_type(type, "IHDR") || len != 13))
            return R_IHDR;
        if (chunk != 0 && is_type(type, "IHDR"))
            return R_IHDR;
        if (is_type(type, "IDAT")) {
            if (idat_closed)
                return R_IDAT_ORDER;
            if (n_idat == 0)
                first_idat_chunk = chunk, first_idat_at = at;
            last_idat_at = at;
            n_idat++;
        } else {
            if (n_idat)
                idat_closed = true;
            if (is_type(type, "tfBX")) {
                n_index++;
                index_late = index_late || n_idat != 0;
                index_size_ok = len == INDEX_BYTES;
                index_at = at;
            } else if (is_type(type, "IEND")) {
                if (len != 0 || at + 12 != n)
                    return R_NO_IEND;
                ended = true;
            }
        }
        at += 12 + (size_t)len;
        chunk++;
        if (chunk == 0xFFFFFFFFu)
            return R_TRUNCATED; // (never: such a file has more than 2^32 bytes)
    }
    if (!ended)
        return R_NO_IEND;
    if (n_idat == 0)
        return R_IDAT_ORDER;
    l.n_chunks = chunk;
    // ---- IHDR
    const uint8_t *ihdr = file + 16;
    const uint32_t width = be32(ihdr), height = be32(ihdr + 4);
    const uint32_t depth = ihdr[8], colour = ihdr[9], compression = ihdr[10], filter = ihdr[11], interlace = ihdr[12];
    bool combo = false; // the specification's table of colour types and depths
    if (colour == 0)
        combo = depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
    else if (colour == 3)
        combo = depth == 1 || depth == 2 || depth == 4 || depth == 8;
    else if (colour == 2 || colour == 4 || colour == 6)
        combo = depth == 8 || depth == 16;
    if (!combo || compression != 0 || filter != 0 || interlace > 1 || width > 0x7FFFFFFFu || height > 0x7FFFFFFFu)
        return R_IHDR;
    if (width == 0 || height == 0)
        return R_SIZE;
    l.width = width, l.height = height;
    // ---- is it for the device at all
    if (depth != 8 || colour != 2) {
        l.why_not = N_FORMAT;
        return R_OK;
    }
    if (interlace) {
        l.why_not = N_INTERLACED;
        return R_OK;
    }
    if (n_index == 0) {
        l.why_not = N_NO_INDEX;
        return R_OK;
    }
    if (n_index > 1 || index_late)
        return R_INDEX;
    const uint8_t *index = file + index_at + 8; // (the chunk's payload lies inside the file: the walk checked)
    if (be32(file + index_at) >= 1 && index[0] != 1) {
        l.why_not = N_VERSION;
        return R_OK;
    }
    if (!index_size_ok || index[1] != 0 || index[2] != 0 || index[3] != 0)
        return R_INDEX;
    // ---- the size, then the index against it and against the IDATs
    if (width > max_width || height > max_height || width > MAX_DIM || height > MAX_DIM || row_bytes(width) * height > MAX_STREAM)
        return R_SIZE;
    const uint32_t band_rows = be32(index + 4), n_bands = be32(index + 8);
    if (band_rows == 0 || band_rows > height || n_bands != (height + band_rows - 1) / band_rows) // (height + band_rows < 2^25)
        return R_INDEX;
    if ((uint64_t)n_idat != (uint64_t)n_bands + 2)
        return R_INDEX;
    l.band_rows = band_rows, l.n_bands = n_bands;
    // ---- the zlib header, the bands, the tail
    if (be32(file + first_idat_at) != 2 || !zlib_header_ok(file[first_idat_at + 8], file[first_idat_at + 9]))
        return R_ZLIB_HEADER;
    at = first_idat_at + 14;
    l.first_band_chunk = first_idat_chunk + 1, l.first_band_at = (uint32_t)at;
    for (uint32_t b = 0; b < n_bands; b++) { // (consecutive IDATs inside the file: the walk above has been over them)
        const uint32_t len = be32(file + at);
        if (b < capacity)
            band_offsets[b] = (uint32_t)(at + 8), band_sizes[b] = len;
        l.max_band_bytes = len > l.max_band_bytes ? len : l.max_band_bytes;
        at += 12 + (size_t)len;
    }
    if (at != last_idat_at)
        return R_INDEX; // (never: the counts agree)
    const uint32_t tail = be32(file + at);
    if (tail < 5 || !empty_final_block(file + at + 8, tail - 4, lit, dist, lengths))
        return R_TAIL;
    l.adler = be32(file + at + 8 + (tail - 4));
    l.indexed = 1;
    return R_OK;
}

// The CRC-32 of every chunk that is no band (IHDR, tfBX, ancillary chunks, the first and the last IDAT, IEND), on the
// host: a reject word with the first chunk that differs, or R_OK.  For a file `walk` has been over.  The named chunks
// are a few dozen bytes; an ancillary chunk is taken here too, however long it is (the encoder writes none; DESIGN.md
// section 20 says what that costs).
PD_HD uint32_t check_small_crcs(const uint8_t *file, size_t n, const Layout &l, const Crc32Consts &consts)
{
    size_t at = 8;
    for (uint32_t chunk = 0; chunk < l.n_chunks && n - at >= 12; chunk++) {
        const uint32_t len = be32(file + at);
        if (len > n - at - 12)
            break; // (never)
        const bool band = l.indexed && chunk >= l.first_band_chunk && chunk - l.first_band_chunk < l.n_bands;
        if (!band && crc32_bytes(consts, file + at + 4, (size_t)len + 4) != be32(file + at + 8 + len))
            return make_reject(R_CHUNK_CRC, chunk);
        at += 12 + (size_t)len;
    }
    return R_OK;
}

// ---- unfilter ----------------------------------------------------------------------------------------------------------
PD_HD int paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the byte a filtered byte x stands for: a left, b above, c above-left (type 0 - 4)
PD_HD uint32_t unfilter_byte(uint32_t type, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : (uint32_t)paeth((int)a, (int)b, (int)c);
    return (x + pred) & 0xFFu;
}

// Adler-32 of the rows' sums: a row of L bytes moves s2 by L s1 + its weighted sum (png.hip's recurrence)
PD_HD uint32_t adler_of_rows(const uint32_t *rowsums, uint32_t height, uint64_t row_len)
{
    uint64_t s1 = 1, s2 = 0;
    for (uint32_t r = 0; r < height; r++) {
        s2 = (s2 + (row_len % 65521) * s1 + rowsums[2 * (size_t)r + 1]) % 65521;
        s1 = (s1 + rowsums[2 * (size_t)r]) % 65521;
    }
    return (uint32_t)((s2 << 16) | s1);
}

} // namespace pngdec
} // namespace tf
