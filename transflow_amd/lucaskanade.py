"""Lucas-Kanade handle: thin object over the tf_lk_* entry points of libtfhip.so.

`LucasKanade.calc(prev, next, win_size, max_level, step)` has the signature and the result of transflow's
calc_optical_flow_lukas_kanade (transflow/flow/methods/lukas_kanade.py): cv2.calcOpticalFlowPyrLK over the grid
arange(0, W, step) x arange(0, H, step) with the default criteria, flow = nextPts - p0 whatever the status,
block-replicated to step x step and cropped, float32 [H][W][2].  It equals the numpy restatement of OpenCV's
lkpyramid.cpp in tests/lk_ref.py bit for bit; that restatement is not yet pinned against a real OpenCV.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

MAX_LEVELS = 20      # TF_LK_MAX_LEVELS
TRACE_CODES = ("done", "lost_prev", "lost_eig", "lost_next")


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def level_sizes(width: int, height: int, win_size: int, max_level: int):
    """[(w, h)] of the pyramid levels buildOpticalFlowPyramid keeps for this window and maxLevel."""
    sizes = [(width, height)]
    w, h = width, height
    for _ in range(max_level):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win_size or h <= win_size:
            break
        sizes.append((w, h))
    return sizes


class LucasKanade:
    def __init__(self, width: int, height: int, frame_slots: int = 2, max_pairs: int = 1, device: int | None = None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        if device is not None:
            check(self._lib.tf_init(int(device)))
        self.width, self.height = int(width), int(height)
        self.frame_slots, self.max_pairs = int(frame_slots), int(max_pairs)
        check(self._lib.tf_lk_create(C.byref(self._h), self.width, self.height, self.frame_slots, self.max_pairs))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tf_lk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _grey(self, frame) -> np.ndarray:
        a = np.asarray(frame)
        if a.dtype != np.uint8 or a.shape != (self.height, self.width):
            raise ValueError(f"expected uint8 grey frame {(self.height, self.width)}, got {a.dtype} {a.shape}")
        if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
            a = np.ascontiguousarray(a)
        return a

    # -- frames ------------------------------------------------------------------------------
    def set_frame(self, slot: int, frame) -> None:
        a = self._grey(frame)
        check(self._lib.tf_lk_set_frame(self._h, int(slot), _ptr(a), a.strides[0]))

    def set_frame_bgr(self, slot: int, frame) -> None:
        """cv.py:461-466 on the device: a decoded BGR frame of any size -> nearest-neighbour resize -> grey."""
        a = np.asarray(frame)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError(f"expected a uint8 BGR frame (H, W, 3), got {a.dtype} {a.shape}")
        if a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
            a = np.ascontiguousarray(a)
        check(self._lib.tf_lk_set_frame_bgr(self._h, int(slot), _ptr(a), a.shape[1], a.shape[0], a.strides[0]))

    # -- calls ---------------------------------------------------------------------------------
    def calc_slots(self, prev_slots, next_slots, win_size=15, max_level=2, step=1, stats=False) -> None:
        """One call over len(prev_slots) pairs; flows stay on the device (get_flow, flow_ptr)."""
        n = len(prev_slots)
        if n != len(next_slots) or n < 1:
            raise ValueError("prev_slots and next_slots must be non-empty and of the same length")
        ps, ns = (C.c_int * n)(*map(int, prev_slots)), (C.c_int * n)(*map(int, next_slots))
        check(self._lib.tf_lk_calc_slots(self._h, int(win_size), int(max_level), int(step), n, ps, ns, int(bool(stats))))

    def calc(self, prev, nxt, win_size=15, max_level=2, step=1) -> np.ndarray:
        """calc_optical_flow_lukas_kanade(prev, next, win_size, max_level, step): a new float32 array."""
        self.set_frame(0, prev)
        self.set_frame(1, nxt)
        self.calc_slots([0], [1], win_size=win_size, max_level=max_level, step=step)
        return self.get_flow(0)

    def get_flow(self, pair: int) -> np.ndarray:
        out = np.empty((self.height, self.width, 2), np.float32)
        check(self._lib.tf_lk_get_flow(self._h, int(pair), _ptr(out)))
        return out

    def flow_ptr(self, pair: int) -> int:
        p = C.c_void_p()
        check(self._lib.tf_lk_flow_ptr(self._h, int(pair), C.byref(p)))
        return p.value

    def last_stats(self, pair: int = 0) -> list:
        """Of the last call made with stats=True: [(sum, max)] of the steps run per point, one entry per level."""
        n = C.c_int()
        buf = (C.c_ulonglong * (2 * MAX_LEVELS))()
        check(self._lib.tf_lk_stats(self._h, int(pair), C.byref(n), buf))
        return [(int(buf[2 * l]), int(buf[2 * l + 1])) for l in range(n.value)]

    # -- stage entry points (tests) ----------------------------------------------------------------
    def stage_pyramid(self, slot: int, win_size: int, max_level: int, level: int) -> np.ndarray:
        """A level of the slot's pyramid, padded by win_size (reflect-101): uint8 [h + 2 win][w + 2 win]."""
        w, h = level_sizes(self.width, self.height, win_size, max_level)[level]
        out = np.empty((h + 2 * win_size, w + 2 * win_size), np.uint8)
        check(self._lib.tf_lk_stage_pyramid(self._h, int(slot), int(win_size), int(max_level), int(level), _ptr(out)))
        return out

    def stage_scharr(self, slot: int, win_size: int, max_level: int, level: int) -> np.ndarray:
        """The Scharr derivatives of a level of the slot's pyramid, zero-padded: int16 [h + 2 win][w + 2 win][2]."""
        w, h = level_sizes(self.width, self.height, win_size, max_level)[level]
        out = np.empty((h + 2 * win_size, w + 2 * win_size, 2), np.int16)
        check(self._lib.tf_lk_stage_scharr(self._h, int(slot), int(win_size), int(max_level), int(level), _ptr(out)))
        return out

    def stage_trace(self, prev_slot: int, next_slot: int, win_size: int, max_level: int, x: float, y: float):
        """One point through every level: [levels][4] float32 {nextPts.x, nextPts.y, steps, code} (index = level)."""
        n = len(level_sizes(self.width, self.height, win_size, max_level))
        out = np.zeros((MAX_LEVELS, 4), np.float32)
        check(self._lib.tf_lk_stage_trace(self._h, int(prev_slot), int(next_slot), int(win_size), int(max_level),
                                          float(x), float(y), _ptr(out)))
        return out[:n]
