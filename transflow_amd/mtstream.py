"""numpy's legacy global random stream, drawn on the device (tf_mt_* of libtfhip.so).

The reference's layers all call `numpy.random.random` (compositor/layers/reference.py:59): one global MT19937 stream per
process.  `Mt19937Stream` is that stream's device side, one per process: it adopts the global state, draws the fields
where the remap kernels read them -- the doubles `numpy.random.random` would have returned, bit for bit -- and `sync()`
writes the position it has reached back into numpy, so that the host goes on drawing what the reference's process would
draw next."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

KEY_WORDS = 624


def _same_state(a, b) -> bool:
    return (a is not None and b is not None and a[0] == b[0] and int(a[2]) == int(b[2]) and int(a[3]) == int(b[3])
            and float(a[4]) == float(b[4]) and np.array_equal(a[1], b[1]))


class Mt19937:
    """One tf_mt handle: a stream of its own (tests, benchmarks).  The compositor uses Mt19937Stream."""

    def __init__(self):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        check(self._lib.tf_mt_create(C.byref(self._h)))

    def set_state(self, key, pos: int) -> None:
        key = np.ascontiguousarray(key, dtype=np.uint32)
        if key.shape != (KEY_WORDS,):
            raise ValueError(f"an MT19937 key has {KEY_WORDS} words, not {key.shape}")
        check(self._lib.tf_mt_set_state(self._h, C.c_void_p(key.ctypes.data), int(pos)))

    def get_state(self):
        """(key, 0): an equivalent state of the stream's position, for numpy.random.set_state / RandomState.set_state."""
        key = np.empty(KEY_WORDS, np.uint32)
        pos = C.c_int()
        check(self._lib.tf_mt_get_state(self._h, C.c_void_p(key.ctypes.data), C.byref(pos)))
        return key, pos.value

    def random_sample_dev(self, out_dev: int, n: int) -> None:
        """The stream's next n doubles into device memory at out_dev, queued on this thread's stream."""
        check(self._lib.tf_mt_random_sample_dev(self._h, C.c_void_p(out_dev), int(n)))

    def info(self) -> dict:
        g, s, ms = C.c_int(), C.c_int(), C.c_float()
        check(self._lib.tf_mt_info(self._h, C.byref(g), C.byref(s), C.byref(ms)))
        return {"segments": g.value, "segment_words": s.value, "bootstrap_ms": ms.value}

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tf_mt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mt19937Stream:
    """numpy's global stream on the device.  `field(n)` hands out the next n doubles as a device address; the global
    state is adopted at the first draw and again whenever it is not the one last adopted or written (someone seeded, or
    drew on the host)."""

    _instance = None

    @classmethod
    def instance(cls) -> "Mt19937Stream":
        if cls._instance is None:
            cls._instance = cls()
        return cls._instance

    @classmethod
    def sync_active(cls) -> None:
        """sync() of the process's stream if there is one: before anything draws from numpy's stream on the host."""
        if cls._instance is not None:
            cls._instance.sync()

    def __init__(self):
        self._mt = Mt19937()
        self._mark = None       # numpy's state tuple as last adopted or written
        self._ahead = False     # the device has drawn past the global state
        self._fields = {}       # n -> ([DevBuffer, DevBuffer], next index)

    def _adopt(self, state) -> None:
        if state[0] != "MT19937":
            raise ValueError(f"numpy's global stream is {state[0]}, not MT19937")
        self._mt.set_state(state[1], int(state[2]))
        self._mark = state
        self._ahead = False

    def field(self, n: int) -> int:
        """The device address of the stream's next n doubles (numpy.random.random of n values).  Two buffers per size
        take turns, and the draw is queued on the stream the layers' kernels run on: a field stays as it is until the
        draw after the next one of its size."""
        from .device import DevBuffer
        n = int(n)
        state = np.random.get_state()
        if not _same_state(state, self._mark):
            self._adopt(state)
        bufs, turn = self._fields.get(n, (None, 0))
        if bufs is None:
            bufs = [DevBuffer(8 * n), DevBuffer(8 * n)]
        self._fields[n] = (bufs, turn ^ 1)
        self._mt.random_sample_dev(bufs[turn].ptr, n)
        self._ahead = True
        return bufs[turn].ptr

    def sync(self) -> None:
        """Writes the stream's position into numpy's global state (the 2.5 KB state comes down; has_gauss and
        cached_gaussian pass through untouched): the host then draws what the reference's process would draw next."""
        if not self._ahead:
            return
        state = np.random.get_state()
        if not _same_state(state, self._mark):   # someone seeded since the last draw: that state is the newer one
            self._ahead = False
            return
        key, pos = self._mt.get_state()
        np.random.set_state(("MT19937", key, pos, state[3], state[4]))
        self._mark = np.random.get_state()
        self._ahead = False

    def info(self) -> dict:
        return self._mt.info()

    def close(self) -> None:
        for bufs, _ in self._fields.values():
            for b in bufs:
                b.close()
        self._fields = {}
        self._mt.close()
        if Mt19937Stream._instance is self:
            Mt19937Stream._instance = None
