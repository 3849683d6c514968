#!/usr/bin/env python3
"""Generate tests/golden/png_*.npz from tests/png_ref.py: a regression pin of the PNG format.

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_png.py

png_code_lengths.npz holds the literal/length code (lengths and canonical codes of the 286 symbols).  Every case of
png_ref.CASES gets png_case_<name>.npz: its name, size and `band_rows` -- the images are formulas of tests/png_ref.py,
so no pixels are stored -- and the bytes of the restatement's file.  Before a file is written Pillow must decode it to
the image and zlib must inflate its IDAT data to the filtered rows.
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

from tests import png_ref  # noqa: E402


def main():
    import PIL.Image
    np.savez_compressed(os.path.join(OUT, "png_code_lengths.npz"), lengths=np.array(png_ref.LENGTHS, np.uint8),
                        codes=np.array(png_ref.CODES, np.uint16))
    for name in png_ref.CASES:
        image, band_rows = png_ref.case(name)
        data = png_ref.encode(image, band_rows)
        with PIL.Image.open(io.BytesIO(data)) as im:
            if not (np.asarray(im.convert("RGB")) == image).all():
                raise SystemExit(f"{name}: Pillow does not decode the file to the image")
        idat = b"".join(p for k, p, _ in png_ref.chunks(data) if k == b"IDAT")
        if zlib.decompress(idat) != png_ref.filtered(image):
            raise SystemExit(f"{name}: zlib does not return the filtered rows")
        path = os.path.join(OUT, f"png_case_{name}.npz")
        np.savez_compressed(path, name=np.str_(name), height=np.int32(image.shape[0]), width=np.int32(image.shape[1]),
                            band_rows=np.int32(band_rows), png=np.frombuffer(data, np.uint8))
        print(f"{os.path.basename(path)}: {image.shape[0]}x{image.shape[1]} band_rows {band_rows} -> {len(data)} bytes, "
              f"{os.path.getsize(path)} on disk")


if __name__ == "__main__":
    main()
