#!/usr/bin/env python3
"""Writes tests/golden/flowunzip_valid.npz and tests/golden/flowunzip_malformed.npz from the Python restatement of the
band inflater (tests/flowunzip_ref.py): the hand-built members zlib never emits (stream, band sizes, band size, the
member's bytes) and the malformed ones (stream, band sizes, and the verdict: band size, member size, the first bad band,
the rejection's number).  tests/test_flowunzip_ref.py holds the restatement to these files; tests/test_gpu_flowunzip.py
holds the device to the restatement.

    python tools/capture_golden_flowunzip.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import flowunzip_ref as U  # noqa: E402


def main() -> None:
    golden = os.path.join(ROOT, "tests", "golden")
    valid = {"names": np.array(sorted(U.hand_valid()))}
    for name, (stream, sizes, band_bytes, member) in U.hand_valid().items():
        S, bad, reason, _ = U.inflate_member(stream, sizes, band_bytes, len(member))
        assert S == member and bad is None, (name, bad, reason)
        valid[name + ".stream"] = np.frombuffer(stream, np.uint8)
        valid[name + ".sizes"] = np.array(sizes, np.int64)
        valid[name + ".band_bytes"] = np.int64(band_bytes)
        valid[name + ".member"] = np.frombuffer(member, np.uint8)
    path = os.path.join(golden, "flowunzip_valid.npz")
    np.savez_compressed(path, **valid)
    print(f"valid: {len(U.hand_valid())} members, file {os.path.getsize(path)}")
    malformed = {"names": np.array(sorted(U.malformed()))}
    for name, ((stream, sizes, band_bytes, usize, bad), reason) in U.malformed().items():
        verdict = U.inflate_member(stream, sizes, band_bytes, usize)
        assert verdict[0] is None and verdict[1:3] == (bad, reason), (name, verdict[1:3])
        malformed[name + ".stream"] = np.frombuffer(stream, np.uint8)
        malformed[name + ".sizes"] = np.array(sizes, np.int64)
        malformed[name + ".verdict"] = np.array([band_bytes, usize, bad, U.REJECT_NUMBER[reason]], np.int64)
    path = os.path.join(golden, "flowunzip_malformed.npz")
    np.savez_compressed(path, **malformed)
    print(f"malformed: {len(U.malformed())} members, file {os.path.getsize(path)}")


if __name__ == "__main__":
    main()
