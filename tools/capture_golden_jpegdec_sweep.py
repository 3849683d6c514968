#!/usr/bin/env python3
"""Writes tests/golden/jpegdec_sweep.npz from tests/jpegdec_sweep.py: every hand-built file with the reject number and
the pixels tests/jpegdec_ref.py gives it and, for an accepted file without DRI, the serial decoder's state at every
subsequence boundary (tests/jpegdec_par_ref.py's entry_rows for subsequences of 16, 64 and 128 bytes).  Where Pillow is
importable, asserts that its pixels are the restatement's on every family but the one pinned by the restatement alone.
tests/test_jpegdec_sweep_ref.py holds the fixture to the builder and the restatement, and asserts what each family
covers; tests/test_gpu_jpegdec_sweep.py holds the device to the fixture.  With Pillow, also writes
tests/golden/jpegdec_sweep_pixels.npz: the families of the pixel stages (colour lattice, MCU order, IDCT basis;
`pixel_cases`) with Pillow's pixels, which tests/test_gpu_jpegdec_geometry.py holds the device to.

    python tools/capture_golden_jpegdec_sweep.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import jpegdec_par_ref as PR  # noqa: E402
from tests import jpegdec_ref as JR  # noqa: E402
from tests import jpegdec_sweep as SW  # noqa: E402


def main() -> None:
    try:
        from tests.jpegdec_cases import pillow_pixels
        import PIL  # noqa: F401
    except ImportError:
        pillow_pixels = None
    cases = SW.all_cases()
    out = {"names": np.array([name for name, _ in cases])}
    for name, built in cases:
        data = built.data
        reason = JR.verdict(data)
        out[name + ".file"] = np.frombuffer(data, np.uint8)
        out[name + ".reject"] = np.int64(JR.R[reason])
        if reason != "ok":
            print(f"  {name}: {len(data)} bytes, {reason}")
            continue
        pixels = JR.decode(data)
        if pillow_pixels is not None and SW.family_of(name) not in SW.RESTATEMENT_ONLY:
            assert np.array_equal(pixels, pillow_pixels(data)), name
        out[name + ".rgb"] = pixels
        if JR.parse_header(data)["restart_mcus"] == 0:
            for sub in SW.SUBS:
                out[f"{name}.entries{sub}"] = PR.entry_rows(data, sub)
        print(f"  {name}: {len(data)} bytes, {pixels.shape[1]} x {pixels.shape[0]}")
    path = os.path.join(ROOT, "tests", "golden", "jpegdec_sweep.npz")
    np.savez_compressed(path, **out)
    print(f"{len(cases)} files, fixture {os.path.getsize(path)} bytes")
    if pillow_pixels is None:
        print("no Pillow here: jpegdec_sweep_pixels.npz holds its pixels and is left as it is")
        return
    cases = SW.pixel_cases()
    out = {"names": np.array([name for name, _ in cases])}
    for name, built in cases:
        pixels = pillow_pixels(built.data)
        assert np.array_equal(JR.decode(built.data), pixels), name
        out[name + ".file"] = np.frombuffer(built.data, np.uint8)
        out[name + ".rgb"] = pixels
        print(f"  {name}: {len(built.data)} bytes, {pixels.shape[1]} x {pixels.shape[0]}")
    path = os.path.join(ROOT, "tests", "golden", "jpegdec_sweep_pixels.npz")
    np.savez_compressed(path, **out)
    print(f"{len(cases)} files of the pixel stages' families, fixture {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
