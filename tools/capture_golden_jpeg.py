#!/usr/bin/env python3
"""Generate tests/golden/jpeg_*.npz by RUNNING libjpeg through Pillow.

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_jpeg.py

Needs a Pillow whose JPEG plugin takes `restart_marker_blocks` (10.2 or later).  A fixture holds the image (uint8
(H, W, 3), at most 61 x 45), the quality, `restart_mcus`, and the bytes of the file that
`Image.save(format="JPEG", quality=q, subsampling=2, restart_marker_blocks=r)` wrote: data only.  Every other case
stores its size, its content kind and its seed instead of its pixels: tests/jpeg_ref.py makes them with integer
arithmetic and no library's generator (formula_image, directed_luma, directed_chroma, binary_noise, chroma_checker).
The cases are tests/jpeg_ref.py's CASES; every fixture is checked against the restatement as it is written.
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
    for name, (h, w, content, quality, restart) in jpeg_ref.CASES.items():
        kind, seed = content if isinstance(content, tuple) else (content, None)
        image = jpeg_ref.case_image(name)
        data = pillow_file(image, quality, restart)
        same = jpeg_ref.encode(image, quality, restart) == data
        fields = dict(quality=np.int32(quality), restart_mcus=np.int32(restart), jpeg=np.frombuffer(data, np.uint8))
        if kind == "formula" and (h, w) == (270, 480):
            fields.update(height=np.int32(h), width=np.int32(w))         # as they were first written
        elif kind in ("stored", "noise", "checker"):
            assert h * w <= 61 * 45, (h, w)
            fields.update(image=image)
        else:
            fields.update(height=np.int32(h), width=np.int32(w), content=np.str_(kind))
            if seed is not None:
                fields.update(seed=np.int64(seed))
        path = os.path.join(OUT, f"jpeg_{name}.npz")
        np.savez_compressed(path, **fields)
        print(f"{os.path.basename(path)}: {h}x{w} q{quality} r{restart} -> {len(data)} bytes, "
              f"{os.path.getsize(path)} on disk, restatement {'equal' if same else 'DIFFERS'}")
        if not same:
            raise SystemExit(f"{name}: tests/jpeg_ref.py does not reproduce Pillow's file")


if __name__ == "__main__":
    main()
