#!/usr/bin/env python3
"""Writes tests/golden/jpegdec_par_valid.npz and jpegdec_par_malformed.npz from tests/jpegdec_par_cases.py (Pillow, no
`restart_marker_blocks`): every valid file with Pillow's pixels of it and the serial decoder's state at every
subsequence boundary (tests/jpegdec_par_ref.py's entry_rows, for subsequences of 16 and of 128 bytes); every malformed
file with the reject number tests/jpegdec_ref.py gives it; the hostile files as they are.  Asserts that each file holds
what it was chosen for.  tests/test_jpegdec_par_ref.py holds the restatement and the shared core to these files,
tests/test_gpu_jpegdec_par.py the device.

    python tools/capture_golden_jpegdec_par.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import jpegdec_cases as JC  # noqa: E402
from tests import jpegdec_par_cases as PC  # noqa: E402
from tests import jpegdec_par_ref as PR  # noqa: E402
from tests import jpegdec_ref as JR  # noqa: E402


def check_valid(name: str, data: bytes) -> None:
    hd = JR.parse_header(data)
    assert hd["restart_mcus"] == 0, name
    size = len(data) - hd["scan_offset"] - 2
    if name.startswith("geo_"):
        assert (hd["width"], hd["height"]) in ((37, 19), (64, 48)), name   # 37 x 19: no edge is a whole MCU's
    if name.startswith("short_"):
        assert size < min(PC.SUBS), (name, size)
    if name.startswith("flat_"):
        ps = PR.ParScan(data, 16)
        begun = [ps.lane(i, e)[1] for i, e in enumerate(ps.serial_entries())]
        assert max(begun) >= 3 * ps.blocks, (name, max(begun))          # many whole MCUs inside one subsequence
    if name.startswith("noise_"):
        scan = data[hd["scan_offset"]:-2]
        for sub in PC.SUBS:
            ps = PR.ParScan(data, sub)
            _, results, rounds = ps.fixed_point()
            print(f"  {name}: S = {sub}: {ps.n_subs} subsequences, {rounds} rounds (resynchronisation over {rounds * sub} bytes)")
            assert rounds > PC.GROUP, (name, sub, rounds)               # the distance crosses a work-group's share
            if sub == 16:
                assert rounds >= 3 * PC.GROUP, (name, rounds)           # several of them
                assert any(r[1] == 0 for r in results), name            # a subsequence in which no block begins
                assert any(scan[i - 1] == 0xFF and scan[i] == 0 for i in range(sub, len(scan), sub)), name  # FF | 00
    if name.startswith("gradient_"):
        rows = PR.entry_rows(data, 16)
        far = np.abs(rows[:: PC.GROUP, 5].astype(np.int32))
        assert far.max() >= 200, (name, far.max())                      # a luma prediction far from 0 at group boundaries
    if name.startswith("garbage_"):
        assert JR.verdict(data) == "ok", name
        ps = PR.ParScan(data, 16)
        entries = ps.serial_entries()
        rows, begun = ps.sums([ps.lane(i, e) for i, e in enumerate(entries)])
        assert begun > ps.total_blocks, name
        ps.total_blocks = begun + 1                                     # as if the garbage's blocks were the picture's
        coef = np.zeros((ps.total_blocks, 64), np.int64)
        strict = [ps.lane(i, e, True, rows[i][0], rows[i][1:], coef)[3] for i, e in enumerate(entries)]
        assert any(strict), name                                        # a strict decoder rejects what follows the last MCU


def main() -> None:
    golden = os.path.join(ROOT, "tests", "golden")
    cases = PC.valid_cases()
    valid = {"names": np.array([name for name, _ in cases])}
    for name, data in cases:
        pixels = JC.pillow_pixels(data)
        assert np.array_equal(JR.decode(data), pixels), name
        check_valid(name, data)
        valid[name + ".file"] = np.frombuffer(data, np.uint8)
        twin = name[:-len("_optimize")] if name.endswith("_optimize") else None
        if twin is not None and np.array_equal(valid[twin + ".rgb"], pixels):      # other tables, the same pixels: kept once
            valid[name + ".rgb_of"] = np.array(twin)
        else:
            valid[name + ".rgb"] = pixels
        for sub in PC.SUBS:
            valid[f"{name}.entries{sub}"] = PR.entry_rows(data, sub)
        print(f"  {name}: {len(data)} bytes")
    path = os.path.join(golden, "jpegdec_par_valid.npz")
    np.savez_compressed(path, **valid)
    print(f"valid: {len(cases)} files, fixture {os.path.getsize(path)} bytes")
    cases = PC.malformed_cases()
    hostile = PC.hostile_cases()
    malformed = {"names": np.array([name for name, _, _ in cases]), "hostile_names": np.array([name for name, _ in hostile])}
    for name, data, built_for in cases:
        reason = JR.verdict(data)
        assert reason == built_for, (name, reason, built_for)
        hd = JR.parse_header(data)
        assert hd["restart_mcus"] == 0 and len(data) - hd["scan_offset"] > max(PC.SUBS) * PC.GROUP, name  # behind the first work-group
        malformed[name + ".file"] = np.frombuffer(data, np.uint8)
        malformed[name + ".reject"] = np.int64(JR.R[reason])
    for name, data in hostile:
        malformed[name + ".file"] = np.frombuffer(data, np.uint8)
    path = os.path.join(golden, "jpegdec_par_malformed.npz")
    np.savez_compressed(path, **malformed)
    print(f"malformed: {len(cases)} files, hostile: {len(hostile)}, fixture {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
