#!/usr/bin/env python3
"""Generate tests/golden/yuvdec_<layout>.npz from tests/yuvdec_ref.py: a regression pin of the conversion back from YUV
 against later edits of the restatement itself.  The project's own data: nothing else is involved.

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_yuvdec.py

Each file holds the small cases of one layout: `names`, `matrices`, `ranges`, `chromas`, and per case i its input
`planes_<i>` (the frame's bytes), `size_<i>` (width, height) and the restatement's RGB pixels `out_<i>` (uint8 (H, W, 3)).
Before a file is written the table of coefficients must be the one DESIGN.md states and every grey must come out grey.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import yuvdec_cases, yuvdec_ref  # noqa: E402


def small_cases(layout):
    """The odd and even sizes up to two lanes wide in all four matrix / range pairs and both chroma modes, and the
    extremes."""
    for matrix, rng in yuvdec_ref.PAIRS:
        for chroma in yuvdec_ref.CHROMAS:
            for w in (1, 2, 3, 5, 8, 17):
                for h in (1, 2, 3, 5):
                    yield f"noise-{w}x{h}-{matrix}-{rng}-{chroma}", yuvdec_cases.noise(w, h, layout, 100 * w + h), w, h, matrix, rng, chroma
    for name, data, w, h, case_layout, matrix, rng, chroma, _ in yuvdec_cases.extreme_cases():
        if case_layout == layout:
            yield name, data, w, h, matrix, rng, chroma


def main():
    for pair, table in yuvdec_ref.TABLE.items():
        if yuvdec_ref.rule(*pair)[0] != table:
            raise SystemExit(f"{pair}: the rule does not give the table")
        levels = np.arange(256, dtype=np.uint8)
        grey = yuvdec_ref.pixels(levels, np.full(256, 128, np.uint8), np.full(256, 128, np.uint8), *pair)
        if not ((grey[:, 0] == grey[:, 1]).all() and (grey[:, 1] == grey[:, 2]).all()):
            raise SystemExit(f"{pair}: a grey has colour")
    for layout in yuvdec_cases.LAYOUTS:
        arrays, names, matrices, ranges, chromas = {}, [], [], [], []
        for i, (name, data, w, h, matrix, rng, chroma) in enumerate(small_cases(layout)):
            names.append(name), matrices.append(matrix), ranges.append(rng), chromas.append(chroma)
            arrays[f"planes_{i}"] = data
            arrays[f"size_{i}"] = np.array([w, h], np.int32)
            arrays[f"out_{i}"] = yuvdec_ref.convert_back(data, w, h, layout, matrix, rng, chroma)
        path = os.path.join(OUT, f"yuvdec_{layout}.npz")
        np.savez_compressed(path, names=np.array(names), matrices=np.array(matrices), ranges=np.array(ranges),
                            chromas=np.array(chromas), **arrays)
        print(f"{os.path.basename(path)}: {len(names)} cases, {os.path.getsize(path)} bytes on disk")


if __name__ == "__main__":
    main()
