#!/usr/bin/env python3
"""Pin the Lucas-Kanade restatement (tests/lk_ref.py) to a real OpenCV.  Stand-alone: needs numpy and cv2 only.

    python tools/pin_lk_with_cv2.py [OUT_DIR]      # default tests/golden

Writes lk_cv2_<cv2 version>.npz: for seeded frame pairs and point sets, cv2.calcOpticalFlowPyrLK's nextPts with the
reference's call (winSize=(w, w), maxLevel=L, default criteria, flags 0; nextPts given as the output array, written
in place).  tests/test_lk_ref.py::test_pin_files_match_restatement compares the restatement with every case bit for
bit; the cases are chosen to decide the points the restatement lists as [VERIFY]:

- windows 3 .. 31 odd and even (the 4- and 8-column SIMD chunks and their scalar tails: the summation order);
- sizes where the pyramid stops early, and frames smaller than the window (the level count, the pads);
- points off the grid (fractional weights, cvRound ties), near and beyond the borders (bounds tests, zero-padded
  derivatives), on flat patches (the minEig / FLT_EPSILON test);
- large motion, including out of the frame (the lost-point paths, nextPts as last written).
"""
import os
import sys

import cv2
import numpy as np


def textured(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    v = np.zeros((h, w))
    for _ in range(6):
        fx, fy, ph = rng.uniform(0.004, 0.08), rng.uniform(0.004, 0.08), rng.uniform(0, 2 * np.pi)
        v += rng.uniform(0.4, 1.0) * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph)
    a = np.clip(np.rint(128 + 20 * v + rng.normal(0, 5, (h, w))), 0, 255).astype(np.uint8)
    return a


def cases():
    rng = np.random.default_rng(1)
    out = []
    for k, win in enumerate((3, 4, 5, 7, 8, 9, 11, 12, 15, 16, 21, 24, 31)):
        h, w = int(rng.integers(40, 130)), int(rng.integers(40, 170))
        a = textured(h, w, 10 + k)
        dy, dx = int(rng.integers(-4, 5)), int(rng.integers(-4, 5))
        b = np.roll(a, (dy, dx), (0, 1))
        b = np.clip(b.astype(np.int16) + rng.integers(-3, 4, b.shape), 0, 255).astype(np.uint8)
        n = 400
        pts = np.stack([rng.uniform(-win, w + win, n), rng.uniform(-win, h + win, n)], 1).astype(np.float32)
        pts[:100] = np.round(pts[:100])
        pts[100:150] = np.round(pts[100:150] * 2) / 2          # half-pixel points: cvRound ties
        out.append((a, b, pts, win, int(rng.integers(0, 6))))
    a = textured(9, 11, 40)
    out.append((a, np.roll(a, 1, 1), np.stack(np.meshgrid(np.arange(11), np.arange(9)), -1).reshape(-1, 2)
                .astype(np.float32), 15, 3))
    flat = np.full((50, 60), 120, np.uint8)
    flat[20:30, 25:35] = 160
    out.append((flat, np.roll(flat, 2, 0), np.stack(np.meshgrid(np.arange(60), np.arange(50)), -1).reshape(-1, 2)
                .astype(np.float32), 9, 2))
    a = textured(80, 100, 41)
    out.append((a, np.roll(a, (-12, 20), (0, 1)), np.stack(np.meshgrid(np.arange(100), np.arange(80)), -1)
                .reshape(-1, 2).astype(np.float32), 15, 2))
    return out


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tests", "golden")
    arrays = {}
    cs = cases()
    for k, (a, b, pts, win, levels) in enumerate(cs):
        p0 = pts.reshape(-1, 1, 2).copy()
        p1 = p0.copy()
        cv2.calcOpticalFlowPyrLK(a, b, p0, p1, winSize=(win, win), maxLevel=levels)
        p = f"c{k}_"
        arrays.update({p + "prev": a, p + "next": b, p + "pts": pts, p + "win": np.int64(win),
                       p + "levels": np.int64(levels), p + "next_pts": p1.reshape(-1, 2)})
    arrays["n_cases"] = np.int64(len(cs))
    arrays["cv2_version"] = np.bytes_(cv2.__version__)
    arrays["cv2_build"] = np.bytes_(cv2.getBuildInformation())
    path = os.path.join(out_dir, f"lk_cv2_{cv2.__version__}.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
