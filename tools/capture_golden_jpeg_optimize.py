#!/usr/bin/env python3
"""Generate tests/golden/jpegopt_*.npz by RUNNING libjpeg's optimize_coding through Pillow.

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_jpeg_optimize.py

Needs a Pillow whose JPEG plugin takes `restart_marker_blocks` (10.2 or later).  A fixture holds the image (uint8
(H, W, 3), at most 61 x 45), the quality, `restart_mcus`, and the bytes of the file that
`Image.save(format="JPEG", quality=q, subsampling=2, restart_marker_blocks=r, optimize=True)` wrote: data only.  Every
other case stores its size, its content kind and its seed instead of its pixels (tests/jpeg_ref.py and
tests/jpeg_optimize_ref.py make them with integer arithmetic and no library's generator).  The cases are
tests/jpeg_optimize_ref.py's CASES; every fixture is checked against the restatement as it is written.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import jpeg_optimize_ref  # noqa: E402
from transflow_amd.jpeg import pillow_encode  # noqa: E402


def main():
    for name, (h, w, content, quality, restart) in jpeg_optimize_ref.CASES.items():
        kind, seed = content if isinstance(content, tuple) else (content, None)
        image = jpeg_optimize_ref.case_image(name)
        data = pillow_encode(image, quality, restart, optimize=True)
        same = jpeg_optimize_ref.encode(image, quality, restart) == data
        fields = dict(quality=np.int32(quality), restart_mcus=np.int32(restart), jpeg=np.frombuffer(data, np.uint8))
        if kind in ("stored", "noise", "checker"):
            assert h * w <= 61 * 45, (h, w)
            fields.update(image=image)
        else:
            fields.update(height=np.int32(h), width=np.int32(w), content=np.str_(kind))
            if seed is not None:
                fields.update(seed=np.int64(seed))
        path = os.path.join(OUT, f"jpegopt_{name}.npz")
        np.savez_compressed(path, **fields)
        print(f"{os.path.basename(path)}: {h}x{w} q{quality} r{restart} -> {len(data)} bytes, "
              f"{os.path.getsize(path)} on disk, restatement {'equal' if same else 'DIFFERS'}")
        if not same:
            raise SystemExit(f"{name}: tests/jpeg_optimize_ref.py does not reproduce Pillow's file")


if __name__ == "__main__":
    main()
