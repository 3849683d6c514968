"""Horn-Schunck handle: thin object over the tf_hs_* entry points of libtfhip.so.

`HornSchunck.calc(prev, next, flow, alpha, max_iters, decay, delta)` has the signature and the result, bit for bit, of
transflow's calc_optical_flow_horn_schunck (transflow/flow/methods/horn_schunck.py), as CvFlowSource calls it
(transflow/flow/sources/cv.py:491-500).  `flow=None` runs the float64 chain, an initial flow the float32 one.

The convergence test `numpy.linalg.norm(u - prev, 2) < delta` is decided on the device when the library can do so
with a safety margin; when it cannot (the spectral norm within 1e-3 of delta, or a NaN or an infinity in u - prev) the
pair waits, and this module evaluates the reference's own expression on the downloaded difference -- so a NaN raises
numpy's LinAlgError, as the reference does.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import TfHsParams, check

STATS_KEYS = ("iterations", "bounds", "power", "gram", "host")


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


class HornSchunck:
    def __init__(self, width: int, height: int, frame_slots: int = 2, max_pairs: int = 1, device: int | None = None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        if device is not None:
            check(self._lib.tf_init(int(device)))
        self.width, self.height = int(width), int(height)
        self.frame_slots, self.max_pairs = int(frame_slots), int(max_pairs)
        check(self._lib.tf_hs_create(C.byref(self._h), self.width, self.height, self.frame_slots, self.max_pairs))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tf_hs_destroy(self._h)
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

    # -- frames and initial flows ------------------------------------------------------
    def set_frame(self, slot: int, frame) -> None:
        a = self._grey(frame)
        check(self._lib.tf_hs_set_frame(self._h, int(slot), _ptr(a), a.strides[0]))

    def set_frame_bgr(self, slot: int, frame) -> None:
        """cv.py:461-466 on the device: a decoded BGR frame of any size -> nearest-neighbour resize -> grey."""
        a = np.asarray(frame)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError(f"expected a uint8 BGR frame (H, W, 3), got {a.dtype} {a.shape}")
        if a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
            a = np.ascontiguousarray(a)
        check(self._lib.tf_hs_set_frame_bgr(self._h, int(slot), _ptr(a), a.shape[1], a.shape[0], a.strides[0]))

    def set_initial_flow(self, pair: int, flow) -> None:
        """The initial flow of `pair` for the next calc_slots (None: the float64 chain from zeros)."""
        if flow is None:
            check(self._lib.tf_hs_set_initial_flow(self._h, int(pair), None))
            return
        f = np.ascontiguousarray(flow, dtype=np.float32)
        if f.shape != (self.height, self.width, 2):
            raise ValueError(f"initial flow shape {f.shape} != {(self.height, self.width, 2)}")
        check(self._lib.tf_hs_set_initial_flow(self._h, int(pair), _ptr(f)))

    def set_initial_flow_dev(self, pair: int, flow_dev: int | None) -> None:
        """The same from a device address (float32 [H][W][2], 8-byte aligned; None: the float64 chain).  Borrowed, not
        copied: the next calc_slots reads it once, in stream order, and nothing waits on the host."""
        check(self._lib.tf_hs_set_initial_flow_dev(self._h, int(pair), C.c_void_p(flow_dev) if flow_dev else None))

    # -- calls ----------------------------------------------------------------------------
    @staticmethod
    def params(alpha=1, max_iters=3, decay=0, delta=1) -> TfHsParams:
        return TfHsParams(float(alpha ** 2), float(decay), int(max_iters), 0.0 if delta is None else float(delta),
                          0 if delta is None else 1)

    def calc_slots(self, prev_slots, next_slots, alpha=1, max_iters=3, decay=0, delta=1) -> None:
        """One call over len(prev_slots) pairs; each pair's initial flow is what set_initial_flow gave it (or none).
        Pairs the device cannot decide are decided here, with the reference's expression."""
        n = len(prev_slots)
        if n != len(next_slots) or n < 1:
            raise ValueError("prev_slots and next_slots must be non-empty and of the same length")
        prm = self.params(alpha, max_iters, decay, delta)
        ps, ns = (C.c_int * n)(*map(int, prev_slots)), (C.c_int * n)(*map(int, next_slots))
        check(self._lib.tf_hs_calc_slots(self._h, C.byref(prm), n, ps, ns))
        self._host_decisions(delta)

    def _host_decisions(self, delta) -> None:
        waiting = (C.c_int * self.max_pairs)()
        nw = C.c_int()
        buf = None
        while True:
            check(self._lib.tf_hs_waiting(self._h, waiting, C.byref(nw)))
            if nw.value == 0:
                return
            for pair in list(waiting[:nw.value]):
                if buf is None:
                    buf = np.empty(self.height * self.width, np.float64)
                is64 = C.c_int()
                check(self._lib.tf_hs_delta_download(self._h, pair, _ptr(buf), C.byref(is64)))
                du = (buf if is64.value else buf.view(np.float32)[:buf.size]).reshape(self.height, self.width)
                converged = bool(np.linalg.norm(du, 2) < delta)    # horn_schunck.py:43; NaN raises LinAlgError
                check(self._lib.tf_hs_resolve(self._h, pair, int(converged)))
            check(self._lib.tf_hs_resume(self._h))

    def calc(self, prev, nxt, flow=None, alpha=1, max_iters=3, decay=0, delta=1) -> np.ndarray:
        """calc_optical_flow_horn_schunck(prev, next, flow, alpha, max_iters, decay, delta): a new float32 array."""
        self.set_frame(0, prev)
        self.set_frame(1, nxt)
        self.set_initial_flow(0, flow)
        self.calc_slots([0], [1], alpha=alpha, max_iters=max_iters, decay=decay, delta=delta)
        return self.get_flow(0)

    def get_flow(self, pair: int) -> np.ndarray:
        out = np.empty((self.height, self.width, 2), np.float32)
        check(self._lib.tf_hs_get_flow(self._h, int(pair), _ptr(out)))
        return out

    def flow_ptr(self, pair: int) -> int:
        p = C.c_void_p()
        check(self._lib.tf_hs_flow_ptr(self._h, int(pair), C.byref(p)))
        return p.value

    def last_stats(self, pair: int = 0) -> dict:
        """Of the last call: iterations run, and how many convergence decisions each stage made."""
        s = (C.c_int * 5)()
        check(self._lib.tf_hs_stats(self._h, int(pair), s))
        return dict(zip(STATS_KEYS, list(s)))

    # -- stage entry points (tests) ---------------------------------------------------------
    def stage_derivatives(self, prev, nxt, alpha=1):
        """ex, ey, et, den (float32 [H][W] each) of the prepare kernel."""
        p, n = np.ascontiguousarray(self._grey(prev)), np.ascontiguousarray(self._grey(nxt))
        out = np.empty((self.height, self.width, 4), np.float32)
        check(self._lib.tf_hs_stage_derivatives(self._h, _ptr(p), _ptr(n), float(alpha ** 2), _ptr(out)))
        return out[..., 0], out[..., 1], out[..., 2], out[..., 3]

    def last_bounds(self, pair: int = 0):
        """F, U, L of `pair`'s most recent convergence check in the last call, from the iteration kernel's partial sums.
        ValueError when the call made none (delta None, or no iteration)."""
        out = (C.c_double * 3)()
        check(self._lib.tf_hs_stage_last_bounds(self._h, int(pair), out))
        return tuple(out)


def stage_norm_test(field: np.ndarray, delta: float):
    """The device's stages of `numpy.linalg.norm(field, 2) < delta` -> (decision, stage): decision 1 / 0, or -1 when only
    the host can tell; stage 0 bounds, 1 power iteration, 2 Gram certificate, 3 host."""
    f = np.ascontiguousarray(field)
    if f.dtype not in (np.float32, np.float64) or f.ndim != 2:
        raise ValueError("a 2-D float32 or float64 field")
    dec, st = C.c_int(), C.c_int()
    check(_lib.load().tf_hs_stage_norm_test(_ptr(f), f.shape[1], f.shape[0], int(f.dtype == np.float64), float(delta),
                                            C.byref(dec), C.byref(st)))
    return dec.value, st.value


POWER_STEPS = 8


def stage_norm_values(u_new: np.ndarray, u_old: np.ndarray | None = None) -> dict:
    """Every stage of the test without early exit, on du = u_new - u_old in the fields' dtype (u_old None: zeros):
    {"F", "U", "L", "power": the 2 * POWER_STEPS lower bounds in the device's order, "gram": the bounds of k = 1, 2, 4},
    float64."""
    f = np.ascontiguousarray(u_new)
    if f.dtype not in (np.float32, np.float64) or f.ndim != 2:
        raise ValueError("a 2-D float32 or float64 field")
    o = None
    if u_old is not None:
        o = np.ascontiguousarray(u_old)
        if o.dtype != f.dtype or o.shape != f.shape:
            raise ValueError("u_old must have u_new's dtype and shape")
    out = (C.c_double * (3 + 2 * POWER_STEPS + 3))()
    check(_lib.load().tf_hs_stage_norm_values(_ptr(f), None if o is None else _ptr(o), f.shape[1], f.shape[0],
                                              int(f.dtype == np.float64), out))
    v = np.array(out)
    return {"F": v[0], "U": v[1], "L": v[2], "power": v[3:3 + 2 * POWER_STEPS], "gram": v[3 + 2 * POWER_STEPS:]}
