// The JPEG decoder's shared core (transflow_amd/csrc/jpegdec_common.h) run on the CPU: the segment walker, the table
// builder, the bit reader, the per-block step and the IDCT the device runs, with the wave's share of the work (the
// marker scan, the window refill) done by plain loops that make the same range checks.  Built with
// -fsanitize=address,undefined and run over valid and malformed files, it shows that no file makes the shared code read
// or write outside what it owns, or compute anything undefined.  Every buffer here is a heap
// allocation of exactly the size the decoder is entitled to, so that the sanitizer sees any access beyond it.
//
//   jpegdec_host_check CORPUS
//
// CORPUS: one case per line, `name hex-of-the-file` (`-` for no bytes).  Prints one line per case:
// `name verdict crc32`, the verdict being the Reject number (0: decoded whole), the CRC-32 that of the dequantised
// coefficients as little-endian int32, block by block in decoding order (0 for a rejected file).
#include "../transflow_amd/csrc/crc32_common.h"
#include "../transflow_amd/csrc/jpegdec_common.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace tf::jpegdec;

static volatile uint32_t g_sink; // the samples go here: the IDCT is run for the sanitizer's eyes

// the marker scan over scan[0, n): the markers' positions, or the lowest-numbered fault
static uint32_t marker_scan(const uint8_t *scan, size_t n, uint32_t expected, std::vector<uint32_t> &markers)
{
    uint32_t fault = 0xFFFFFFFFu;
    auto note = [&](uint32_t r) { fault = r < fault ? r : fault; };
    if (n < 2 || scan[n - 2] != 0xFF || scan[n - 1] != 0xD9)
        note(R_NO_EOI);
    for (size_t i = 0; i < n; i++) {
        if (scan[i] != 0xFF)
            continue;
        if (i + 1 >= n) {
            note(R_STRAY_MARKER);
            continue;
        }
        const uint32_t kind = pair_kind(scan[i + 1]);
        if (kind == P_RST) {
            if (scan[i + 1] != 0xD0 + (markers.size() & 7))
                note(R_RST_ORDER);
            markers.push_back((uint32_t)i);
        } else if (kind == P_STRAY && !(i + 2 == n && scan[i + 1] == 0xD9)) {
            note(R_STRAY_MARKER);
        }
    }
    if (markers.size() != expected)
        note(R_RST_COUNT);
    return fault == 0xFFFFFFFFu ? (uint32_t)R_OK : fault;
}

// one interval: its MCUs' coefficients appended to `coefs`
static uint32_t decode_interval(const Header &hd, const uint8_t *src, uint32_t size, int first, int last, std::vector<int32_t> &coefs)
{
    uint8_t *win = (uint8_t *)malloc(WINDOW_BYTES);
    int32_t *coef = (int32_t *)malloc(64 * sizeof(int32_t)), *ws = (int32_t *)malloc(64 * sizeof(int32_t));
    memset(win, 0xA5, WINDOW_BYTES);
    Bits b;
    start(b, win, size);
    int last_dc[3] = {0, 0, 0};
    const int luma = hd.components == 1 ? 1 : hd.h_samp * hd.v_samp;
    uint32_t rc = R_OK;
    for (int m = first; m < last && rc == R_OK; m++)
        for (int blk = 0; blk < hd.blocks_per_mcu && rc == R_OK; blk++) {
            if (need_refill(b, BLOCK_MARGIN)) {
                uint32_t at = 0, len = 0;
                refill_range(b, &at, &len);
                for (uint32_t i = 0; i < len && i < WINDOW_BYTES; i++)
                    win[i] = at + i < size ? src[at + i] : 0;
            }
            memset(coef, 0, 64 * sizeof(int32_t));
            const int c = blk < luma ? 0 : blk - luma + 1;
            rc = decode_block(b, hd.dc[c], hd.ac[c], hd.quant[c], last_dc[c], coef);
            if (rc != R_OK)
                break;
            coefs.insert(coefs.end(), coef, coef + 64);
            uint8_t px[8];
            for (int col = 0; col < 8; col++)
                idct_column(coef, col, ws);
            for (int row = 0; row < 8; row++) {
                idct_row(ws, row, px);
                g_sink = g_sink + px[row];
            }
        }
    free(win), free(coef), free(ws);
    return rc;
}

static uint32_t decode_file(const uint8_t *file, size_t n, std::vector<int32_t> &coefs)
{
    Header *hd = (Header *)malloc(sizeof(Header));
    Raw *raw = (Raw *)malloc(sizeof(Raw));
    memset(hd, 0, sizeof(Header)), memset(raw, 0, sizeof(Raw));
    uint32_t rc = parse_header(file, n, *hd, *raw);
    if (rc == R_OK) {
        // the scan in a block of its own: an index past it is an index past the allocation
        const size_t scan_bytes = n - hd->scan_offset;
        uint8_t *scan = (uint8_t *)malloc(scan_bytes ? scan_bytes : 1);
        memcpy(scan, file + hd->scan_offset, scan_bytes);
        std::vector<uint32_t> markers;
        rc = marker_scan(scan, scan_bytes, (uint32_t)hd->intervals - 1, markers);
        const int per = hd->restart_mcus ? hd->restart_mcus : hd->n_mcus;
        for (int iv = 0; iv < hd->intervals && rc == R_OK; iv++) {
            uint32_t from = iv == 0 ? 0 : markers[(size_t)iv - 1] + 2;
            uint32_t to = iv + 1 == hd->intervals ? (uint32_t)scan_bytes - 2 : markers[(size_t)iv];
            to = to < scan_bytes ? to : (uint32_t)scan_bytes, from = from < to ? from : to;
            // the interval in a block of its own too
            uint8_t *part = (uint8_t *)malloc(to - from ? to - from : 1);
            memcpy(part, scan + from, to - from);
            const long first = (long)iv * per, last = first + per < hd->n_mcus ? first + per : hd->n_mcus;
            rc = decode_interval(*hd, part, to - from, (int)first, (int)last, coefs);
            free(part);
        }
        free(scan);
    }
    free(hd), free(raw);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s CORPUS\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    tf::Crc32Consts consts;
    tf::make_crc32_consts(consts);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream fields(line);
        std::string name, hex;
        if (!(fields >> name >> hex))
            continue;
        if (hex == "-")
            hex.clear();
        const size_t size = hex.size() / 2;
        uint8_t *file = (uint8_t *)malloc(size ? size : 1);
        for (size_t i = 0; i < size; i++)
            file[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
        std::vector<int32_t> coefs;
        const uint32_t verdict = decode_file(file, size, coefs);
        uint32_t crc = 0;
        if (verdict == R_OK) {
            std::vector<uint8_t> bytes(coefs.size() * 4);
            for (size_t i = 0; i < coefs.size(); i++)
                for (int k = 0; k < 4; k++)
                    bytes[4 * i + k] = (uint8_t)((uint32_t)coefs[i] >> (8 * k));
            crc = tf::crc32_bytes(consts, bytes.data(), bytes.size());
        }
        printf("%s %u %u\n", name.c_str(), verdict, crc);
        free(file);
    }
    return 0;
}
