// The JPEG decoder's parallel path for scans without restart markers (transflow_amd/csrc/jpegdec_par_common.h) run on
// the CPU: the lanes of the device one after another, round after round, with the hand-offs, the exclusive sums and the
// strict write the kernels do.  Built with -fsanitize=address,undefined and run over valid, malformed and hostile files,
// it shows that no file makes the shared code read or write outside what it owns, or compute anything undefined
// (DESIGN.md section 19).  The scan, the entries and the coefficients are heap allocations of exactly the size the
// decoder is entitled to, so that the sanitizer sees any access beyond them.
//
//   jpegdec_par_host_check CORPUS SUB_BYTES
//
// CORPUS: one case per line, `name hex-of-the-file` (`-` for no bytes).  Prints one line per case:
// `name verdict crc32 rounds`, the verdict being the Reject number (0: decoded whole), the CRC-32 that of the dequantised
// coefficients as little-endian int32, block by block in decoding order (0 for a rejected file), rounds the trips to the
// fixed point.  A file with a restart interval is not this path's: its line is `name - 0 0`.
#include "../transflow_amd/csrc/crc32_common.h"
#include "../transflow_amd/csrc/jpegdec_par_common.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace tf::jpegdec;

// the marker scan of a file without DRI: the lowest-numbered fault
static uint32_t marker_scan(const uint8_t *scan, size_t n)
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
        if (kind == P_RST)
            note(R_RST_COUNT);
        else if (kind == P_STRAY && !(i + 2 == n && scan[i + 1] == 0xD9))
            note(R_STRAY_MARKER);
    }
    return fault == 0xFFFFFFFFu ? (uint32_t)R_OK : fault;
}

static uint32_t decode_scan(const Header &hd, const uint8_t *scan_all, size_t scan_bytes, uint32_t sub_bytes, std::vector<int32_t> &dequantised,
                            uint32_t &rounds)
{
    ParGeom g;
    g.size = (uint32_t)scan_bytes - 2;
    g.sub_bytes = sub_bytes;
    g.n_subs = par_subs(g.size, sub_bytes);
    g.blocks = (uint32_t)hd.blocks_per_mcu, g.luma_blocks = hd.components == 1 ? 1u : (uint32_t)(hd.h_samp * hd.v_samp);
    g.total_blocks = (uint32_t)hd.n_mcus * g.blocks;
    // what the lanes are entitled to: the scan without its EOI, one entry and one result per subsequence, the picture's blocks
    uint8_t *scan = (uint8_t *)malloc(g.size ? g.size : 1);
    memcpy(scan, scan_all, g.size);
    uint64_t *entries = (uint64_t *)malloc(g.n_subs * sizeof(uint64_t));
    ParLane *lanes = (ParLane *)malloc(g.n_subs * sizeof(ParLane));
    int16_t *coef = (int16_t *)calloc((size_t)g.total_blocks * 64, sizeof(int16_t));
    Huff dc[3], ac[3];
    for (int c = 0; c < 3; c++)
        dc[c] = hd.dc[c < hd.components ? c : 0], ac[c] = hd.ac[c < hd.components ? c : 0];
    for (uint32_t i = 0; i < g.n_subs; i++)
        entries[i] = i == 0 ? par_pack(0, 0, 0) : par_guess(scan, g.size, sub_bytes, i);
    std::vector<uint8_t> changed(g.n_subs, 1);
    rounds = 0;
    for (uint32_t round = 0; round < g.n_subs; round++) { // entry r is exact after round r
        for (uint32_t i = 0; i < g.n_subs; i++)
            if (changed[i])
                par_lane<false>(ParBytes{scan}, g, dc, ac, i, entries[i], 0u, nullptr, nullptr, lanes[i]);
        bool any = false;
        for (uint32_t i = g.n_subs; i-- > 1;) { // every hand-off of a round takes the exit of that round
            changed[i] = lanes[i - 1].exit != entries[i];
            entries[i] = lanes[i - 1].exit;
            any |= changed[i] != 0;
        }
        changed[0] = 0;
        rounds++;
        if (!any)
            break;
    }
    uint32_t first_block = 0, pred[3] = {0, 0, 0};
    uint32_t status = PAR_NO_FAULT;
    for (uint32_t i = 0; i < g.n_subs; i++) {
        ParLane out;
        par_lane<true>(ParBytes{scan}, g, dc, ac, i, entries[i], first_block, pred, coef, out);
        if (out.fault != R_OK) {
            const uint32_t word = (i << PAR_REASON_BITS) | out.fault;
            status = word < status ? word : status;
        }
        first_block += lanes[i].n_begin;
        for (int c = 0; c < 3; c++)
            pred[c] += lanes[i].dc_sum[c];
    }
    if (status == PAR_NO_FAULT && first_block < g.total_blocks)
        status = (g.n_subs << PAR_REASON_BITS) | (uint32_t)R_EXHAUSTED;
    const uint32_t verdict = status == PAR_NO_FAULT ? (uint32_t)R_OK : status & ((1u << PAR_REASON_BITS) - 1);
    if (verdict == R_OK)
        for (uint32_t j = 0; j < g.total_blocks; j++) {
            const uint32_t blk = j % g.blocks, c = blk < g.luma_blocks ? 0u : blk - g.luma_blocks + 1u;
            int32_t natural[64];
            for (int k = 0; k < 64; k++)
                natural[ZIGZAG[k]] = (int32_t)coef[(size_t)j * 64 + ZIGZAG[k]] * (int32_t)hd.quant[c < (uint32_t)hd.components ? c : 0][k];
            dequantised.insert(dequantised.end(), natural, natural + 64);
        }
    free(scan), free(entries), free(lanes), free(coef);
    return verdict;
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s CORPUS SUB_BYTES\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    const uint32_t sub_bytes = (uint32_t)strtoul(argv[2], nullptr, 10);
    if (!in || sub_bytes < PAR_MIN_SUB || sub_bytes > PAR_MAX_SUB) {
        fprintf(stderr, "cannot read %s, or SUB_BYTES is not %u to %u\n", argv[1], PAR_MIN_SUB, PAR_MAX_SUB);
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
        Header *hd = (Header *)malloc(sizeof(Header));
        Raw *raw = (Raw *)malloc(sizeof(Raw));
        memset(hd, 0, sizeof(Header)), memset(raw, 0, sizeof(Raw));
        uint32_t verdict = parse_header(file, size, *hd, *raw), rounds = 0, crc = 0;
        if (verdict == R_OK && hd->restart_mcus) {
            printf("%s - 0 0\n", name.c_str());
        } else {
            std::vector<int32_t> coefs;
            if (verdict == R_OK) {
                const size_t scan_bytes = size - hd->scan_offset;
                verdict = scan_bytes < 2 ? (uint32_t)R_NO_EOI : marker_scan(file + hd->scan_offset, scan_bytes);
                if (verdict == R_OK)
                    verdict = decode_scan(*hd, file + hd->scan_offset, scan_bytes, sub_bytes, coefs, rounds);
            }
            if (verdict == R_OK) {
                std::vector<uint8_t> bytes(coefs.size() * 4);
                for (size_t i = 0; i < coefs.size(); i++)
                    for (int k = 0; k < 4; k++)
                        bytes[4 * i + k] = (uint8_t)((uint32_t)coefs[i] >> (8 * k));
                crc = tf::crc32_bytes(consts, bytes.data(), bytes.size());
            }
            printf("%s %u %u %u\n", name.c_str(), verdict, crc, rounds);
        }
        free(hd), free(raw), free(file);
    }
    return 0;
}
