#!/usr/bin/env python3
"""Generate tests/golden/jpegsub_*.npz by RUNNING libjpeg at 4:4:4 and 4:2:2 through Pillow.

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_jpeg_sub.py

Needs a Pillow whose JPEG plugin takes `restart_marker_blocks` (10.2 or later).  A fixture holds the recipe of its image
(size, content kind, seed: tests/jpeg_sub_ref.py makes it with integer arithmetic and no library's generator), the
quality, `restart_mcus`, the subsampling, whether the file carries its own Huffman tables, and the bytes of the file that
`Image.save(format="JPEG", quality=q, subsampling=s, restart_marker_blocks=r, optimize=o)` wrote: data only.  The cases
are tests/jpeg_sub_ref.py's CASES, each at subsampling 0 and 1; every fixture is checked against the restatement as it is
written.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import jpeg_sub_ref  # noqa: E402
from transflow_amd.jpeg import pillow_encode  # noqa: E402


def main():
    for name, (h, w, kind, seed, quality, restart, optimize) in jpeg_sub_ref.CASES.items():
        image = jpeg_sub_ref.case_image(name)
        for sub in (0, 1):
            data = pillow_encode(image, quality, restart, optimize=optimize, subsampling=sub)
            same = jpeg_sub_ref.encode(image, quality, restart, sub, optimize) == data
            path = os.path.join(OUT, jpeg_sub_ref.fixture_name(name, sub))
            np.savez_compressed(path, height=np.int32(h), width=np.int32(w), content=np.str_(kind), seed=np.int64(seed),
                                quality=np.int32(quality), restart_mcus=np.int32(restart), subsampling=np.int32(sub),
                                optimize=np.bool_(optimize), jpeg=np.frombuffer(data, np.uint8))
            print(f"{os.path.basename(path)}: {h}x{w} q{quality} r{restart} s{sub}{' optimize' if optimize else ''} -> "
                  f"{len(data)} bytes, {os.path.getsize(path)} on disk, restatement {'equal' if same else 'DIFFERS'}")
            if not same:
                raise SystemExit(f"{name}: tests/jpeg_sub_ref.py does not reproduce Pillow's file")


if __name__ == "__main__":
    main()
