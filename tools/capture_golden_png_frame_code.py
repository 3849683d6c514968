#!/usr/bin/env python3
"""Generate tests/golden/png_fc_*.npz from tests/png_frame_code_ref.py: a regression pin of the PNG encoder's mode
"frame" ("The frame's own code").

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_png_frame_code.py

Every case of png_frame_code_ref.GOLDEN_CASES gets png_fc_<name>.npz: its name, size and `band_rows` -- the images are
formulas of the restatements, so no pixels are stored -- the bytes of the restatement's file, the code's lengths, the
repair count, and per band its bytes and whether it is stored.  Before a file is written Pillow must decode it to the
image and zlib must inflate its IDAT data to the filtered rows.
"""
import io
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import png_frame_code_ref as F  # noqa: E402
from tests import png_ref  # noqa: E402


def main():
    import PIL.Image
    for name in F.GOLDEN_CASES:
        image, band_rows = F.case(name)
        t = F.trace(image, band_rows)
        with PIL.Image.open(io.BytesIO(t.data)) as im:
            if not (np.asarray(im.convert("RGB")) == image).all():
                raise SystemExit(f"{name}: Pillow does not decode the file to the image")
        idat = b"".join(p for k, p, _ in png_ref.chunks(t.data) if k == b"IDAT")
        if zlib.decompress(idat) != png_ref.filtered(image):
            raise SystemExit(f"{name}: zlib does not return the filtered rows")
        path = os.path.join(OUT, f"png_fc_{name}.npz")
        np.savez_compressed(path, name=np.str_(name), height=np.int32(image.shape[0]), width=np.int32(image.shape[1]),
                            band_rows=np.int32(band_rows), png=np.frombuffer(t.data, np.uint8),
                            lengths=np.array(t.lengths, np.uint8), repairs=np.int32(t.repairs),
                            band_sizes=np.array(t.band_sizes, np.uint32), band_stored=np.array(t.band_stored, bool))
        print(f"{os.path.basename(path)}: {image.shape[0]}x{image.shape[1]} band_rows {band_rows} -> {len(t.data)} bytes, "
              f"{os.path.getsize(path)} on disk")


if __name__ == "__main__":
    main()
