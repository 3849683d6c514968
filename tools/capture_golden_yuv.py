#!/usr/bin/env python3
"""Generate tests/golden/yuv_<layout>.npz from tests/yuv_ref.py: a regression pin of the YUV format (DESIGN.md section
21) against later edits of the restatement itself.

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_yuv.py

Each file holds the small cases of one layout: `names`, `matrices`, `ranges`, and per case i its input `rgb_<i>`
(uint8 (H, W, 3)) and the restatement's frame `out_<i>` (the layout's bytes).  Before a file is written the table of
coefficients must be the one DESIGN.md states and every grey must come out with neutral chroma.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import yuv_cases, yuv_ref  # noqa: E402


def small_cases(layout):
    """The odd and even sizes up to two lanes wide in all four matrix / range pairs, and the extremes."""
    for matrix, rng in yuv_ref.PAIRS:
        for w in (1, 2, 3, 5, 8, 17):
            for h in (1, 2, 3):
                yield f"noise-{w}x{h}-{matrix}-{rng}", yuv_cases.noise(h, w, 100 * w + h), matrix, rng
    for name, rgb, case_layout, matrix, rng in yuv_cases.extreme_cases():
        if case_layout == layout and not name.startswith("boundary-blocks"):
            yield name, rgb, matrix, rng


def main():
    for pair, table in yuv_ref.TABLE.items():
        if [list(r) for r in yuv_ref.rule(*pair)[0]] != table:
            raise SystemExit(f"{pair}: the rule does not give the table")
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    for layout in yuv_cases.LAYOUTS:
        for matrix, rng in yuv_ref.PAIRS:
            _, u, v = yuv_ref.planes(grey, layout, matrix, rng)
            if not ((u == 128).all() and (v == 128).all()):
                raise SystemExit(f"{layout} {matrix} {rng}: a grey has colour")
        arrays, names, matrices, ranges = {}, [], [], []
        for i, (name, rgb, matrix, rng) in enumerate(small_cases(layout)):
            names.append(name), matrices.append(matrix), ranges.append(rng)
            arrays[f"rgb_{i}"] = rgb
            arrays[f"out_{i}"] = np.frombuffer(yuv_ref.convert(rgb, layout, matrix, rng), np.uint8)
        path = os.path.join(OUT, f"yuv_{layout}.npz")
        np.savez_compressed(path, names=np.array(names), matrices=np.array(matrices), ranges=np.array(ranges), **arrays)
        print(f"{os.path.basename(path)}: {len(names)} cases, {os.path.getsize(path)} bytes on disk")


if __name__ == "__main__":
    main()
