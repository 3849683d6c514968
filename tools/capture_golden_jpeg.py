#!/usr/bin/env python3
"""Generate tests/golden/jpeg_*.npz by RUNNING libjpeg through Pillow.

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_jpeg.py

Needs a Pillow whose JPEG plugin takes `restart_marker_blocks` (10.2 or later).  A fixture holds the image (uint8
(H, W, 3), at most 61 x 45), the quality, `restart_mcus`, and the bytes of the file that
`Image.save(format="JPEG", quality=q, subsampling=2, restart_marker_blocks=r)` wrote: data only.  The one larger case
(270 x 480) stores its size instead of its pixels: tests/jpeg_ref.py's formula_image makes them, arithmetic with no
generator.  The cases are tests/jpeg_ref.py's CASES; every fixture is checked against the restatement as it is written.
"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import jpeg_ref  # noqa: E402


def pillow_file(image: np.ndarray, quality: int, restart_mcus: int) -> bytes:
    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(image).save(buf, format="JPEG", quality=quality, subsampling=2, restart_marker_blocks=restart_mcus)
    return buf.getvalue()


def main():
    for n, (name, (h, w, content, quality, restart)) in enumerate(jpeg_ref.CASES.items()):
        if content == "stored":
            image = jpeg_ref.stored_image(h, w, seed=h * 1000 + w)      # the same picture for every case of a size
        elif content == "noise":
            image = jpeg_ref.noise_image(h, w, seed=7)
        elif content == "checker":
            image = jpeg_ref.checkerboard(h, w)
        else:
            image = jpeg_ref.formula_image(h, w)
        data = pillow_file(image, quality, restart)
        same = jpeg_ref.encode(image, quality, restart) == data
        fields = dict(quality=np.int32(quality), restart_mcus=np.int32(restart), jpeg=np.frombuffer(data, np.uint8))
        if content == "formula":
            fields.update(height=np.int32(h), width=np.int32(w))
        else:
            assert h * w <= 61 * 45, (h, w)
            fields.update(image=image)
        path = os.path.join(OUT, f"jpeg_{name}.npz")
        np.savez_compressed(path, **fields)
        print(f"{os.path.basename(path)}: {h}x{w} q{quality} r{restart} -> {len(data)} bytes, "
              f"{os.path.getsize(path)} on disk, restatement {'equal' if same else 'DIFFERS'}")
        if not same:
            raise SystemExit(f"{name}: tests/jpeg_ref.py does not reproduce Pillow's file")


if __name__ == "__main__":
    main()
