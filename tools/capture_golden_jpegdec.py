#!/usr/bin/env python3
"""Writes tests/golden/jpegdec_valid.npz, jpegdec_malformed.npz, jpegdec_stream.npz and jpegdec_geometry.npz from
tests/jpegdec_cases.py (Pillow >= 10.2): every valid file with Pillow's pixels of it (`PIL.Image.open(...).convert("RGB")`:
libjpeg's), every malformed file with the reject number the restatement (tests/jpegdec_ref.py) gives it, the frames of the
MJPEG stream of the integration tests, and the pixel stages' corpus -- the small frames of `geometry_cases` -- with
Pillow's pixels (tests/test_gpu_jpegdec_geometry.py holds the device to them).  The fixtures hold the pixels, so the Pillow of the machine that runs the GPU tests
does not matter.  tests/test_jpegdec_ref.py holds the restatement to these files; tests/test_gpu_jpegdec.py the device.

    python tools/capture_golden_jpegdec.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import jpegdec_cases as JC  # noqa: E402
from tests import jpegdec_ref as JR  # noqa: E402


def main() -> None:
    golden = os.path.join(ROOT, "tests", "golden")
    cases = JC.valid_cases()
    valid = {"names": np.array([name for name, _ in cases])}
    for name, data in cases:
        pixels = JC.pillow_pixels(data)
        assert np.array_equal(JR.decode(data), pixels), name
        valid[name + ".file"] = np.frombuffer(data, np.uint8)
        valid[name + ".rgb"] = pixels
    path = os.path.join(golden, "jpegdec_valid.npz")
    np.savez_compressed(path, **valid)
    print(f"valid: {len(cases)} files, fixture {os.path.getsize(path)} bytes")
    cases = JC.malformed_cases()
    malformed = {"names": np.array([name for name, _ in cases])}
    for name, data in cases:
        reason = JR.verdict(data)
        assert reason != "ok", name
        malformed[name + ".file"] = np.frombuffer(data, np.uint8)
        malformed[name + ".reject"] = np.int64(JR.R[reason])
    path = os.path.join(golden, "jpegdec_malformed.npz")
    np.savez_compressed(path, **malformed)
    print(f"malformed: {len(cases)} files, fixture {os.path.getsize(path)} bytes")
    frames = JC.stream_frames()
    stream = {"count": np.int64(len(frames))}
    for i, data in enumerate(frames):
        stream[f"{i}.file"] = np.frombuffer(data, np.uint8)
        stream[f"{i}.rgb"] = JC.pillow_pixels(data)
    path = os.path.join(golden, "jpegdec_stream.npz")
    np.savez_compressed(path, **stream)
    print(f"stream: {len(frames)} frames, fixture {os.path.getsize(path)} bytes")
    cases = JC.geometry_cases()
    geometry = {"names": np.array([name for name, _ in cases])}
    for name, data in cases:
        pixels = JC.pillow_pixels(data)
        assert np.array_equal(JR.decode(data), pixels), name
        geometry[name + ".file"] = np.frombuffer(data, np.uint8)
        geometry[name + ".rgb"] = pixels
    path = os.path.join(golden, "jpegdec_geometry.npz")
    np.savez_compressed(path, **geometry)
    print(f"geometry: {len(cases)} files, fixture {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
