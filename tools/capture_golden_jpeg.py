#!/usr/bin/env python3
"""Generate a family of the JPEG encoder's fixtures by RUNNING libjpeg through Pillow.

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_jpeg.py {jpeg,jpegopt,jpegsub} [OUT_DIR]

  jpeg     tests/golden/jpeg_<name>.npz                  4:2:0, the Annex K tables
  jpegopt  tests/golden/jpegopt_<name>.npz               4:2:0, the frame's own tables (libjpeg's optimize_coding)
  jpegsub  tests/golden/jpegsub_<name>_s<0 or 1>.npz     4:4:4 and 4:2:2, either tables

Needs a Pillow whose JPEG plugin takes `restart_marker_blocks` (10.2 or later).  A fixture holds the quality,
`restart_mcus`, and the bytes of the file that
`Image.save(format="JPEG", quality=q, subsampling=s, restart_marker_blocks=r, optimize=o)` wrote: data only.  A jpeg or
jpegopt fixture of a picture that numpy's generator has a part in holds the image (uint8 (H, W, 3), at most 61 x 45);
every other stores its size, its content kind and its seed instead of its pixels: tests/jpeg_cases.py makes them with
integer arithmetic and no library's generator.  A jpegsub fixture always stores the recipe, and the subsampling and
whether the file carries its own Huffman tables besides.  The cases are tests/jpeg_cases.py's tables; every fixture is
checked against the restatement, tests/jpeg_ref.py, as it is written.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import jpeg_cases, jpeg_ref  # noqa: E402
from transflow_amd.jpeg import pillow_encode  # noqa: E402


def fields_420(family, case, image):
    """The schema of jpeg_*.npz and jpegopt_*.npz."""
    h, w, content = case[:3]
    kind, seed = content if isinstance(content, tuple) else (content, None)
    if family == "jpeg" and kind == "formula" and (h, w) == (270, 480):
        fields = dict(height=np.int32(h), width=np.int32(w))              # as they were first written
    elif kind in ("stored", "rng_noise", "checker"):
        assert h * w <= 61 * 45, (h, w)
        fields = dict(image=image)
    else:
        fields = dict(height=np.int32(h), width=np.int32(w), content=np.str_(kind))
        if seed is not None:
            fields.update(seed=np.int64(seed))
    return fields


def main(family, out):
    for name, case in jpeg_cases.CASES[family].items():
        image = jpeg_cases.case_image(family, name)
        quality, restart = case[-3:-1] if family == "jpegsub" else case[3:]
        optimize = case[-1] if family == "jpegsub" else family == "jpegopt"
        for sub in jpeg_cases.LAYOUT_CASE_SUBSAMPLINGS if family == "jpegsub" else (None,):
            layout = 2 if sub is None else sub
            data = pillow_encode(image, quality, restart, optimize=optimize, subsampling=layout)
            if family == "jpegsub":
                fields = dict(height=np.int32(case[0]), width=np.int32(case[1]), content=np.str_(case[2]),
                              seed=np.int64(case[3]), subsampling=np.int32(sub), optimize=np.bool_(optimize))
            else:
                fields = fields_420(family, case, image)
            path = os.path.join(out, os.path.basename(jpeg_cases.fixture_path(family, name, sub)))
            np.savez_compressed(path, quality=np.int32(quality), restart_mcus=np.int32(restart),
                                jpeg=np.frombuffer(data, np.uint8), **fields)
            same = jpeg_ref.encode(image, quality, restart, layout, optimize) == data
            print(f"{os.path.basename(path)}: {image.shape[0]}x{image.shape[1]} q{quality} r{restart} s{layout}"
                  f"{' optimize' if optimize else ''} -> {len(data)} bytes, {os.path.getsize(path)} on disk, "
                  f"restatement {'equal' if same else 'DIFFERS'}")
            if not same:
                raise SystemExit(f"{name}: tests/jpeg_ref.py does not reproduce Pillow's file")


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3) or sys.argv[1] not in jpeg_cases.CASES:
        raise SystemExit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) == 3 else jpeg_cases.GOLDEN)
