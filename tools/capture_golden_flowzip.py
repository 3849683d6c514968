#!/usr/bin/env python3
"""Writes tests/golden/flowzip_<case>.npz from the numpy restatement of the flow archive member coder
(tests/flowzip_ref.py): the member's uncompressed bytes, the restatement's deflate stream, its CRC-32 and the code
lengths, with the band size and the distance the case was coded at.  tests/test_flowzip_ref.py holds the restatement to
these files; tests/test_gpu_flowzip.py holds the device to the restatement.  flowzip_every_distance.npz holds the streams
of R.every_distance(D) for D = 1 .. 64, one behind the other, with their ends, CRCs and lengths.

    python tools/capture_golden_flowzip.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import flowzip_ref as R  # noqa: E402


def main() -> None:
    golden = os.path.join(ROOT, "tests", "golden")
    for name in R.CASES:
        prefix, array, band_bytes, distance = R.case(name)
        member = prefix + array.tobytes()
        stream, crc, lengths = R.encode_stream(prefix, array.tobytes(), band_bytes, distance)
        path = os.path.join(golden, f"flowzip_{name}.npz")
        np.savez_compressed(path, member=np.frombuffer(member, np.uint8), stream=np.frombuffer(stream, np.uint8),
                            lengths=np.array(lengths, np.uint8), crc=np.uint32(crc), band_bytes=np.int64(band_bytes),
                            distance=np.int64(distance), prefix_len=np.int64(len(prefix)))
        print(f"{name}: {len(member)} bytes -> {len(stream)}, file {os.path.getsize(path)}")
    streams, crcs, sizes = [], [], []
    for distance in range(1, 65):
        member = R.every_distance(distance).tobytes()
        stream, crc, _ = R.encode_stream(b"", member, R.EVERY_DISTANCE_BAND, distance)
        streams.append(stream), crcs.append(crc), sizes.append(len(member))
    path = os.path.join(golden, "flowzip_every_distance.npz")
    np.savez_compressed(path, streams=np.frombuffer(b"".join(streams), np.uint8), ends=np.cumsum([len(s) for s in streams]),
                        crcs=np.array(crcs, np.uint32), sizes=np.array(sizes, np.int64),
                        band_bytes=np.int64(R.EVERY_DISTANCE_BAND))
    print(f"every_distance: {sum(sizes)} bytes -> {sum(len(s) for s in streams)}, file {os.path.getsize(path)}")


if __name__ == "__main__":
    main()
