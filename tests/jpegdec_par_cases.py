"""The test files of the JPEG decoder's parallel path for scans without restart markers: Pillow-written files without DRI,
and malformed ones built by hand so that each fault sits where it is wanted.  Used by
tools/capture_golden_jpegdec_par.py for tests/golden/jpegdec_par_*.npz."""
from __future__ import annotations

import numpy as np

from . import jpegdec_cases as JC

# the sizes the GPU tests force (jd_par_sub_bytes, jd_par_group_subs): a work-group's share of the scan is SUB * GROUP bytes
SUBS = (16, 128)
GROUP = 64


def gradient(height: int, width: int) -> np.ndarray:
    """Smooth and bright at the bottom: the DC prediction is far from 0 through most of the scan."""
    yy, xx = np.mgrid[0:height, 0:width]
    rng = np.random.default_rng(70)
    base = 20 + 220 * (yy / max(height - 1, 1)) ** 0.5 + 10 * np.sin(xx / 9.0) + rng.normal(0, 6, (height, width))
    return np.clip(np.stack([base, base * 0.9 + 10, 255 - base * 0.5], axis=-1), 0, 255).astype(np.uint8)


def valid_cases() -> list:
    """[(name, file bytes)], none with a restart interval."""
    out = []
    for w, h in [(37, 19), (64, 48)]:
        out.append((f"geo_420_{w}x{h}", JC.encode(JC.image(h, w, 80 + w))))
        out.append((f"geo_422_{w}x{h}", JC.encode(JC.image(h, w, 81 + w), subsampling=1)))
        out.append((f"geo_444_{w}x{h}", JC.encode(JC.image(h, w, 82 + w), subsampling=0)))
        out.append((f"geo_grey_{w}x{h}", JC.encode(JC.image(h, w, 83 + w, grey=True))))
    out.append(("short_grey_8x8", JC.encode(JC.image(8, 8, 84, grey=True), quality=50)))      # 12 bytes of scan
    out.append(("flat_128", JC.encode(JC.image(128, 128, 0, "flat"))))
    out.append(("noise_128_q100", JC.encode(JC.image(128, 128, 85, "noise"), quality=100)))
    out.append(("scene_256_q90", JC.encode(JC.image(256, 256, 86))))
    out.append(("scene_256_q90_optimize", JC.encode(JC.image(256, 256, 86), optimize=True)))
    out.append(("gradient_160x120", JC.encode(gradient(120, 160), quality=95)))
    base = JC.encode(JC.image(48, 64, 87))
    rng = np.random.default_rng(88)
    tail = bytes(int(v) for v in rng.integers(0, 255, 700))            # no FF: the marker scan has nothing to say
    out.append(("garbage_behind_the_last_mcu", base[:-2] + tail + b"\xff\xd9"))
    return out


# ---- hand-built grey files of many long blocks ---------------------------------------------------------------------------
# DC codes: 0 (category 0), 10 (category 11), 110 (category 12: a fault)
BIG_DC = ([1, 1, 1] + [0] * 13, [0, 11, 12])
# AC codes: 00 (EOB), 01 (run 15 size 1), 100 (ZRL), 101 (run 0 size 10), 110 (run 3 size 0: no symbol),
# 1110 (run 0 size 11: a category fault); 1111 begins no code
BIG_AC = ([0, 2, 3, 1] + [0] * 12, [0x00, 0xF1, 0xF0, 0x0A, 0x30, 0x0B])
BIG_SIDE = 19                                                          # blocks a side: 152 x 152 pixels, 361 blocks


def _good_block(rng) -> str:
    """DC 0, fifteen coefficients of ten value bits, EOB: 198 bits."""
    bits = "0"
    for _ in range(15):
        bits += "101" + format(int(rng.integers(0, 1024)), "010b")
    return bits + "00"


def handmade_big(faults: dict | None = None, cut_block: int | None = None, drop_from: int | None = None) -> bytes:
    """A 152 x 152 grey file of 361 blocks of 198 bits (8.9 KB of scan).  faults: {block: bits that replace it}.
    cut_block: the scan ends in the middle of that block.  drop_from: the scan ends in front of that block."""
    rng = np.random.default_rng(90)
    n = BIG_SIDE * BIG_SIDE
    blocks = [_good_block(rng) for _ in range(n)]
    for at, bits in (faults or {}).items():
        blocks[at] = bits
    if cut_block is not None:
        blocks = blocks[:cut_block] + [blocks[cut_block][:97]]
    if drop_from is not None:
        blocks = blocks[:drop_from]
    bits = "".join(blocks)
    bits += "1" * (-len(bits) % 8)
    scan = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00")

    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)

    side = (8 * BIG_SIDE).to_bytes(2, "big")
    return (b"\xff\xd8" + seg(0xDB, [0] + [1] * 64) + seg(0xC0, [8, *side, *side, 1, 1, 0x11, 0])
            + seg(0xC4, [0x00] + BIG_DC[0] + BIG_DC[1]) + seg(0xC4, [0x10] + BIG_AC[0] + BIG_AC[1])
            + seg(0xDA, [1, 1, 0x00, 0, 63, 0]) + scan + b"\xff\xd9")


LATE = 345          # a block behind byte 8192 of the scan (198 bits a block, more with stuffing): behind the first work-group
FAULT_BITS = {
    "bad_code": "0" + "1111" + "0" * 20,
    "bad_symbol": "0" + "110" + "00",
    "run_past_63": "0" + ("01" + "1") * 4 + "00",
    "category": "0" + "1110" + "0" * 11 + "00",
    "dc_category": "110" + "0" * 12 + "00",
    "dc_range": "10" + "1" * 11 + "00",           # + 2047, and again in the block behind it
}


def malformed_cases() -> list:
    """[(name, file bytes, the reason it was built for)]"""
    out = []
    for name, bits in FAULT_BITS.items():
        faults = {LATE: bits}
        if name == "dc_range":
            faults[LATE + 1] = bits
        reason = "category" if name == "dc_category" else name
        out.append((name, handmade_big(faults), reason))
    out.append(("exhausted_cut", handmade_big(cut_block=LATE), "exhausted"))
    out.append(("exhausted_short", handmade_big(drop_from=LATE), "exhausted"))
    out.append(("two_faults", handmade_big({LATE: FAULT_BITS["bad_symbol"], LATE + 9: FAULT_BITS["bad_code"]}), "bad_symbol"))
    good = handmade_big()
    so = JC._scan_offset(good)
    at = so + 8500
    while good[at - 1] == 0xFF or good[at] == 0xFF:                    # not into an FF 00 pair
        at += 1
    out.append(("rst_without_dri", good[:at] + b"\xff\xd0" + good[at:], "rst_count"))
    return out


def hostile_cases() -> list:
    """[(name, file bytes)]: files whose verdict nothing pins -- random bytes as a scan under real tables, so that the
    lenient decoder meets every kind of fault; the host check runs them for the sanitizers' sake."""
    out = []
    base = JC.encode(JC.image(48, 64, 91))
    so = JC._scan_offset(base)
    for seed in range(4):
        rng = np.random.default_rng(92 + seed)
        body = bytes(int(v) for v in rng.integers(0, 256, 900)).replace(b"\xff", b"\xff\x00")
        out.append((f"hostile_random_{seed}", base[:so] + body + b"\xff\xd9"))
    out.append(("hostile_empty_scan", base[:so] + b"\xff\xd9"))
    out.append(("hostile_ones", base[:so] + b"\xfe" * 600 + b"\xff\xd9"))
    out.append(("hostile_handmade_ones", handmade_big({3: "0" + "1111" * 200})))
    return out
