"""tf_flow_convolve_post_process_dev: the convolution kernel of FlowSource.post_process and what follows it in the
convolution's type (source.py:344-362), out of place and without the intermediate array; and tf_flow_narrow_dev, the
float64 flow rounded in double for the compositor's layers.  The tail on every case of tests/conv_tail_cases.py, in all
three directions, as bit patterns: against the oracle (post_process_with_kernel; conv_tail_cases.expected says how a NaN
that reaches FORWARD's integer conversion is pinned), and independently against tf_flow_convolve_dev followed by
tf_flow_post_process_dev.  `dst` sits between two 64 KB guard zones and `src` is read back."""
import ctypes as C

import numpy as np
import pytest

from tests import conv_tail_cases as T
from tests.flow_ops_cases import same_bits

pytestmark = pytest.mark.gpu

GUARD = 64 * 1024
POISON = 0xA5


class _Device:
    def __init__(self):
        from transflow_amd import _lib
        from transflow_amd.device import DevBuffer
        self.lib, self.check, self.DevBuffer = _lib.load(), _lib.check, DevBuffer

    def tail(self, flow, kernel, direction, winner=True):
        """(dst, src read back, guards intact) of the new entry."""
        h, w, _ = flow.shape
        rt = np.result_type(np.float32, kernel.dtype)
        k = np.ascontiguousarray(kernel, dtype=rt)
        n = h * w * 2 * rt.itemsize
        src, kb = self.DevBuffer.from_array(flow), self.DevBuffer.from_array(k)
        room = self.DevBuffer.from_array(np.full(2 * GUARD + n, POISON, np.uint8))
        win = self.DevBuffer(max(4, 4 * h * w))
        p = C.c_void_p
        try:
            self.check(self.lib.tf_flow_convolve_post_process_dev(
                p(src.ptr), p(kb.ptr), k.shape[0], k.shape[1], int(rt == np.float64), p(room.ptr + GUARD), w, h, direction,
                p(win.ptr) if winner else None))
            whole = room.download((2 * GUARD + n,), np.uint8)
            back = src.download(flow.shape, np.float32)
        finally:
            for b in (src, kb, room, win):
                b.close()
        guards = bool((whole[:GUARD] == POISON).all() and (whole[GUARD + n:] == POISON).all())
        return whole[GUARD:GUARD + n].view(rt).reshape(h, w, 2), back, guards

    def two_entries(self, flow, kernel, direction):
        """tf_flow_convolve_dev, then tf_flow_post_process_dev in place."""
        from transflow_amd.flowops import convolve_post_process
        return convolve_post_process(flow, kernel, None if direction < 0 else direction)


@pytest.fixture(scope="module")
def dev():
    return _Device()


@pytest.mark.parametrize("case", T.tail_cases(), ids=lambda c: c["name"])
def test_tail_matches_the_oracle_and_the_two_entries(dev, case):
    flow, kernel = T.tail_inputs(case)
    for d in T.DIRECTIONS:
        got, back, guards = dev.tail(flow, kernel, d)
        assert guards, f"{case['name']}, direction {d}: a guard zone was written"
        assert same_bits(back, flow), f"{case['name']}, direction {d}: src was written"
        exp = T.expected(case, d)
        assert got.dtype == exp.dtype
        wrong = np.flatnonzero((got.view(np.uint8).reshape(-1, got.itemsize) != exp.view(np.uint8).reshape(-1, got.itemsize)).any(axis=1))
        print(f"{case['name']} direction {d}: {wrong.size} of {got.size} values differ from the oracle")
        assert wrong.size == 0, f"{case['name']}, direction {d}: first at {wrong[:4]}"
        assert same_bits(got, dev.two_entries(flow, kernel, d)), f"{case['name']}, direction {d}: not the two entries' bits"


def test_tail_refuses_what_it_cannot_do(dev):
    from transflow_amd import _lib
    w, h = 5, 3
    a, b, k, win = (dev.DevBuffer(16 * w * h) for _ in range(4))
    p = C.c_void_p
    entry = dev.lib.tf_flow_convolve_post_process_dev
    try:
        for args in ((p(a.ptr), p(k.ptr), 1, 1, 0, p(a.ptr), w, h, 1, None),             # in place
                     (None, p(k.ptr), 1, 1, 0, p(b.ptr), w, h, 1, None),                 # no source
                     (p(a.ptr), None, 1, 1, 0, p(b.ptr), w, h, 1, None),                 # no kernel
                     (p(a.ptr), p(k.ptr), 1, 1, 0, None, w, h, 1, None),                 # no destination
                     (p(a.ptr), p(k.ptr), 1, 1, 0, p(b.ptr), w, h, 0, None),             # FORWARD without a winner map
                     (p(a.ptr), p(k.ptr), 1, 1, 0, p(b.ptr), w, h, 0, p(b.ptr)),         # the winner map over dst
                     (p(a.ptr), p(k.ptr), 0, 3, 0, p(b.ptr), w, h, 1, None),             # kh * kw == 0
                     (p(a.ptr), p(k.ptr), 3, 0, 1, p(b.ptr), w, h, 1, None),
                     (p(a.ptr), p(k.ptr), 1, 1, 0, p(b.ptr), w, h, 2, p(win.ptr)),       # no such direction
                     (p(a.ptr), p(k.ptr), 1, 1, 1, p(b.ptr + 8), w, h, 1, None)):        # a float64 dst that is not 16-byte aligned
            with pytest.raises(ValueError):
                _lib.check(entry(*args))
        _lib.check(entry(None, None, 1, 1, 0, None, 0, 7, 1, None))                       # an empty image: nothing to do
    finally:
        for buf in (a, b, k, win):
            buf.close()


@pytest.mark.parametrize("offset", [0, 8])
@pytest.mark.parametrize("count", T.NARROW_COUNTS)
def test_narrow_matches_numpy(dev, count, offset):
    a = T.narrow_input(count)
    src = dev.DevBuffer(8 * count + 16)
    room = dev.DevBuffer.from_array(np.full(2 * GUARD + 4 * count + 16, POISON, np.uint8))
    p = C.c_void_p
    try:
        dev.check(dev.lib.tf_dev_upload(p(src.ptr + offset), p(a.ctypes.data), a.nbytes))
        for mode in (0, 1):
            dev.check(dev.lib.tf_flow_narrow_dev(p(src.ptr + offset), p(room.ptr + GUARD + offset), count, mode))
            whole = room.download((2 * GUARD + 4 * count + 16,), np.uint8)
            got = whole[GUARD + offset:GUARD + offset + 4 * count].view(np.float32)
            with np.errstate(invalid="ignore"):
                exp = T.narrow_form(a, mode)
            nan = np.isnan(exp)
            assert (np.isnan(got) == nan).all(), (count, offset, mode)
            assert (np.signbit(got[nan]) == np.signbit(exp[nan])).all(), (count, offset, mode)
            assert same_bits(np.where(nan, 0, got).astype(np.float32), np.where(nan, 0, exp).astype(np.float32)), (count, offset, mode)
            assert (whole[:GUARD + offset] == POISON).all() and (whole[GUARD + offset + 4 * count:] == POISON).all()
        with pytest.raises(ValueError):
            dev.check(dev.lib.tf_flow_narrow_dev(p(src.ptr), p(room.ptr + GUARD), count, 2))
    finally:
        src.close()
        room.close()
