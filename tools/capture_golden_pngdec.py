"""Records tests/golden/pngdec_corpus.npz: a few indexed PNG files of the corpus (tests/pngdec_cases.py) -- made by this
repository's own code, zlib and Pillow -- and the pixels they decode to, so that the decoders are held to files that do
not move with the zlib that builds the corpus.

    python -m tools.capture_golden_pngdec
"""
import io
import os
import sys

import numpy as np
import PIL.Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import pngdec_cases as K  # noqa: E402
from tests import pngdec_ref as D  # noqa: E402

NAMES = ("zlib.1x5_random_b2", "zlib.22x5_random_b2", "zlib.86x5_random_b2", "zlib.5x65_paeth_b2", "zlib.12x8_ties_paeth_b3",
         "zlib.12x8_ties_average_b3", "zlib.40x24_random_b5", "zlib.40x24_stored_b5", "zlib.40x24_fixed_b5", "enc.24x40_noise_b5",
         "enc.9x50_black_b3", "enc.7x1")


def main():
    out = {"names": np.array(NAMES)}
    for i, name in enumerate(NAMES):
        data, image = K.valid()[name]
        assert (D.decode(data) == image).all()
        assert (np.array(PIL.Image.open(io.BytesIO(data)).convert("RGB")) == image).all()
        out[f"file_{i}"] = np.frombuffer(data, np.uint8)
        out[f"image_{i}"] = image
    path = os.path.join(ROOT, "tests", "golden", "pngdec_corpus.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
