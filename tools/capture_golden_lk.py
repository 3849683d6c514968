#!/usr/bin/env python3
"""Generate tests/golden/lk_*.npz by RUNNING the reference's Lucas-Kanade function.

Run in the build container only (the reference package does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_lk.py

OpenCV is not installed there.  The one OpenCV call of the function, cv2.calcOpticalFlowPyrLK(prev, next, p0, p1,
winSize=(w, w), maxLevel=L), is served by a stub put into sys.modules BEFORE the reference is imported: the numpy
restatement tests/lk_ref.py, writing nextPts IN PLACE into p1 as OpenCV's Python bindings do (the reference ignores
the return value and reads p1).  Every other line -- the point grid, the copy, the subtraction, numpy.kron, the crop
and the dtype -- is the reference's own code.  Each fixture holds the frames, the parameters and the flow.
"""
import os
import sys
import types

import numpy as np

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import lk_ref  # noqa: E402
from tests.helpers import synth_pair  # noqa: E402


def _install_cv2_stub():
    def calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts, winSize=(21, 21), maxLevel=3, criteria=None,
                             flags=0, minEigThreshold=1e-4, **kwargs):
        if criteria is not None or flags or minEigThreshold != 1e-4 or kwargs or winSize[0] != winSize[1]:
            raise NotImplementedError("the stub serves the default criteria, flags and threshold, square windows")
        p0 = np.asarray(prevPts)
        assert p0.dtype == np.float32 and nextPts.dtype == np.float32 and nextPts.flags.c_contiguous
        out = lk_ref.calc_pyr_lk(prevImg, nextImg, p0.reshape(-1, 2), int(winSize[0]), int(maxLevel))
        nextPts.reshape(-1, 2)[...] = out          # in place, as the bindings write into a matching array
        n = len(out)
        return nextPts, np.ones((n, 1), np.uint8), np.zeros((n, 1), np.float32)

    stub = types.ModuleType("cv2")
    stub.calcOpticalFlowPyrLK = calcOpticalFlowPyrLK
    sys.modules["cv2"] = stub


def reference_function():
    """The reference's function, imported with the cv2 stub in place."""
    _install_cv2_stub()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from transflow.flow.methods.lukas_kanade import calc_optical_flow_lukas_kanade
    return calc_optical_flow_lukas_kanade


def _textured(h, w, seed):
    return synth_pair(h, w, seed=seed, shift=(2.5, 1.5), noise=4.0)


def cases():
    """(name, prev, next, win, max_level, step)"""
    out = []
    a, b = _textured(45, 61, 31)
    out += [("45x61_w3_l0_s1", a, b, 3, 0, 1), ("45x61_w4_l2_s1", a, b, 4, 2, 1), ("45x61_w21_l2_s1", a, b, 21, 2, 1)]
    a, b = _textured(48, 64, 32)
    out.append(("48x64_w15_l2_s1", a, b, 15, 2, 1))
    a, b = _textured(120, 160, 33)
    out.append(("120x160_w15_l5_s1", a, b, 15, 5, 1))               # the pyramid stops at level 2
    a, b = _textured(75, 101, 34)
    out += [("75x101_w15_l2_s4", a, b, 15, 2, 4), ("75x101_w15_l2_s16", a, b, 15, 2, 16),
            ("75x101_w4_l0_s4", a, b, 4, 0, 4)]
    a, b = _textured(9, 11, 35)
    out.append(("9x11_w15_l2_s1", a, b, 15, 2, 1))                  # a frame smaller than the window
    flat = np.full((40, 50), 97, np.uint8)
    out.append(("40x50_flat_w15_l2_s1", flat, flat.copy(), 15, 2, 1))
    a, _ = _textured(60, 80, 36)
    out.append(("60x80_same_w9_l2_s1", a, a.copy(), 9, 2, 1))
    moved = np.roll(a, (-9, 14), (0, 1))                             # motion that leaves the frame
    moved[:, :14] = 0
    out.append(("60x80_leave_w9_l1_s1", a, moved, 9, 1, 1))
    return out


def main():
    fn = reference_function()
    os.makedirs(OUT, exist_ok=True)
    for (name, a, b, win, levels, step) in cases():
        flow = fn(a, b, win, levels, step)
        assert flow.dtype == np.float32 and flow.shape == a.shape + (2,)
        path = os.path.join(OUT, f"lk_{name}.npz")
        np.savez_compressed(path, prev=a, next=b, win_size=np.int64(win), max_level=np.int64(levels),
                            step=np.int64(step), flow=flow)
        print(f"{name}: max |flow| {np.abs(flow).max():.3f}, {os.path.getsize(path)} B")


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
