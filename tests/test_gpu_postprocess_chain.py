"""tf_flow_post_process_chain_dev: FlowSource.post_process out of place, on a flow that sits in a method handle's own
buffer, leaving the reference's `prev_flow` -- the next call's initial flow -- in a third buffer.  `dst` against the
oracle's post-process behind its filter and mask pre-steps (what tests/test_gpu_postprocess.py compares the in-place
entry with), `chain` against the pre-steps WITHOUT the mask multiply where a mask is set (numpy.multiply makes a new
array, source.py:342-343) and against `dst` where none is, `src` against itself: all three as bit patterns."""
import ctypes as C

import numpy as np
import pytest

from oracle import remap_ref as R

pytestmark = pytest.mark.gpu

# (H, W): one pixel; an odd width below one wave; odd both ways, an odd pixel count; a width past one wave; several
# work-groups of 256 lanes
SHAPES = [(1, 1), (3, 5), (37, 53), (60, 84), (64, 256)]
DIRECTIONS = {"forward": R.FORWARD, "backward": R.BACKWARD, "none": -1}
OPS = {"no filters": [], "weak": [("scale", 1.5), ("threshold", 0.75), ("clip", 4.0)],
       "float64": [("scale", np.float64(-0.5)), ("threshold", np.float64(0.4)), ("clip", np.float64(2.5))]}
POISON = np.float32(-77.25)      # what dst and chain hold before the call


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _flow(h, w, seed=61):
    """Both zeros, values a quarter of a pixel on either side of each of a pixel's four clip bounds (-j, W - 1 - j,
    -i, H - 1 - i), vectors far outside the frame, and a tenth of the pixels all pointing at the middle one."""
    rng = np.random.default_rng(seed)
    f = rng.normal(0, 3, (h, w, 2)).astype(np.float32)
    ii, jj = np.mgrid[0:h, 0:w]
    pick = rng.random((h, w))
    f[pick < 0.15] = np.float32(-0.0)
    f[(pick >= 0.15) & (pick < 0.25)] = np.float32(0.0)
    far = (pick >= 0.25) & (pick < 0.3)
    f[far] = rng.choice(np.array([-1e3, 1e3, 2.5, -2.5], np.float32), (int(far.sum()), 2))
    edge = (pick >= 0.3) & (pick < 0.55)
    kind = rng.integers(0, 8, (h, w))
    side = np.where(kind % 2 == 0, -0.25, 0.25).astype(np.float32)
    bound_x = np.where(kind % 4 < 2, -jj, w - 1 - jj).astype(np.float32) + side
    bound_y = np.where(kind % 4 < 2, -ii, h - 1 - ii).astype(np.float32) + side
    on_x = edge & (kind < 4)
    on_y = edge & (kind >= 4)
    f[..., 0][on_x] = bound_x[on_x]
    f[..., 1][on_y] = bound_y[on_y]
    crowd = pick >= 0.9
    f[..., 0][crowd] = (w // 2 - jj)[crowd]
    f[..., 1][crowd] = (h // 2 - ii)[crowd]
    return f


def _mask(h, w):
    rng = np.random.default_rng(62)
    m = rng.random((h, w)).astype(np.float32)
    m[rng.random((h, w)) < 0.3] = 0
    return m


class _Buffers:
    """src (at `offset` bytes into its allocation: 8 makes the 16-byte accesses impossible, as the second pair of a
    handle with an odd pixel count does), dst, chain, winner and the mask on the device."""

    def __init__(self, h, w, offset):
        from transflow_amd import _lib
        from transflow_amd.device import DevBuffer
        self.lib, self.check = _lib.load(), _lib.check
        self.h, self.w, self.n = h, w, 8 * h * w
        self.src_buf, self.dst, self.chain = DevBuffer(self.n + 16), DevBuffer(self.n), DevBuffer(self.n)
        self.src = self.src_buf.ptr + offset
        self.winner = DevBuffer(4 * h * w)
        self.mask = DevBuffer.from_array(_mask(h, w))
        self.poison = np.full((h, w, 2), POISON)

    def run(self, raw, direction, ops, masked, with_chain=True):
        from transflow_amd.flowops import flow_ops_array
        arr, n = flow_ops_array(ops)
        self.check(self.lib.tf_dev_upload(C.c_void_p(self.src), C.c_void_p(raw.ctypes.data), raw.nbytes))
        self.dst.upload(self.poison)
        self.chain.upload(self.poison)
        self.check(self.lib.tf_flow_post_process_chain_dev(
            C.c_void_p(self.src), C.c_void_p(self.dst.ptr), C.c_void_p(self.chain.ptr) if with_chain else None, self.w,
            self.h, direction, n, arr, C.c_void_p(self.mask.ptr) if masked else None, C.c_void_p(self.winner.ptr)))
        src = np.empty_like(raw)
        self.check(self.lib.tf_dev_download(C.c_void_p(src.ctypes.data), C.c_void_p(self.src), raw.nbytes))
        shape = (self.h, self.w, 2)
        return src, self.dst.download(shape, np.float32), self.chain.download(shape, np.float32)

    def close(self):
        for b in (self.src_buf, self.dst, self.chain, self.winner, self.mask):
            b.close()


_EXPECTED = {}


def _expected(h, w, direction, ops_name, masked):
    """(dst, chain) of the oracle, computed once per case."""
    key = (h, w, direction, ops_name, masked)
    if key not in _EXPECTED:
        filtered = R.pre_steps(_flow(h, w), OPS[ops_name], None)
        pre = R.pre_steps(filtered, (), _mask(h, w)) if masked else filtered.copy()
        dst = pre if direction < 0 else R.post_process(pre, direction)
        _EXPECTED[key] = (dst, filtered if masked else dst)
    return _EXPECTED[key]


@pytest.mark.parametrize("offset", [0, 8])
@pytest.mark.parametrize("h,w", SHAPES)
def test_chain_entry_matches_the_oracle(h, w, offset):
    raw = _flow(h, w)
    bufs = _Buffers(h, w, offset)
    try:
        for dname, direction in DIRECTIONS.items():
            for ops_name, ops in OPS.items():
                for masked in (False, True):
                    what = f"{dname}, {ops_name}, mask {masked}"
                    exp_dst, exp_chain = _expected(h, w, direction, ops_name, masked)
                    src, dst, chain = bufs.run(raw, direction, ops, masked)
                    np.testing.assert_array_equal(_bits(src), _bits(raw), err_msg=f"src, {what}")
                    np.testing.assert_array_equal(_bits(dst), _bits(exp_dst), err_msg=f"dst, {what}")
                    np.testing.assert_array_equal(_bits(chain), _bits(exp_chain), err_msg=f"chain, {what}")
                    # without a chain buffer: the same dst, and nothing is written where the chain would be
                    src, dst, chain = bufs.run(raw, direction, ops, masked, with_chain=False)
                    np.testing.assert_array_equal(_bits(dst), _bits(exp_dst), err_msg=f"dst alone, {what}")
                    assert (chain == POISON).all(), f"chain written without being given, {what}"
    finally:
        bufs.close()


@pytest.mark.parametrize("h,w", SHAPES)
def test_chain_entry_equals_the_in_place_entry(h, w):
    """dst holds exactly the bits tf_flow_post_process_ex_dev leaves in place."""
    from transflow_amd.flowops import PostProcess
    raw = _flow(h, w)
    bufs, pp = _Buffers(h, w, 0), PostProcess(w, h)
    try:
        for dname, direction in DIRECTIONS.items():
            for ops_name, ops in OPS.items():
                for masked in (False, True):
                    pp._flow.upload(raw)
                    pp.post_process_ex(0, None if direction < 0 else direction, ops, bufs.mask.ptr if masked else None)
                    exp = pp._flow.download(raw.shape, np.float32)
                    _, dst, _ = bufs.run(raw, direction, ops, masked)
                    np.testing.assert_array_equal(_bits(dst), _bits(exp), err_msg=f"{dname}, {ops_name}, mask {masked}")
    finally:
        bufs.close()
        pp.close()


@pytest.mark.parametrize("h,w", [(37, 53), (60, 84)])
def test_chain_is_the_output_unless_a_mask_comes_between(h, w):
    raw = _flow(h, w)
    mask = _mask(h, w)
    bufs = _Buffers(h, w, 0)
    try:
        for dname, direction in DIRECTIONS.items():
            for ops_name, ops in OPS.items():
                _, dst, chain = bufs.run(raw, direction, ops, False)
                np.testing.assert_array_equal(_bits(chain), _bits(dst), err_msg=f"no mask, {dname}, {ops_name}")
                _, dst, chain = bufs.run(raw, direction, ops, True)
                filtered = R.pre_steps(raw.copy(), ops, None)
                np.testing.assert_array_equal(_bits(chain), _bits(filtered), err_msg=f"mask, {dname}, {ops_name}")
                if direction == R.FORWARD:
                    continue                                  # (dst is the inverted field: other pixels' vectors)
                hidden = (mask == 0)[..., None] & (filtered != 0)
                assert hidden.any()
                assert (dst[hidden] == 0).all() and (chain[hidden] != 0).all(), f"{dname}, {ops_name}"
                assert (_bits(dst)[hidden] != _bits(chain)[hidden]).all()
    finally:
        bufs.close()


def test_chain_entry_refuses_what_it_cannot_do():
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer
    from transflow_amd.flowops import flow_ops_array
    lib = _lib.load()
    w, h = 5, 3
    a, b, c = DevBuffer(8 * w * h), DevBuffer(8 * w * h), DevBuffer(8 * w * h)
    arr, _ = flow_ops_array([])
    p = C.c_void_p
    try:
        for args in ((p(a.ptr), p(a.ptr), None, w, h, 1, 0, arr, None, None),          # in place
                     (p(a.ptr), p(b.ptr), p(b.ptr), w, h, 1, 0, arr, None, None),      # chain over dst
                     (p(a.ptr), p(b.ptr), None, w, h, 0, 0, arr, None, None),          # FORWARD without a winner map
                     (p(a.ptr), p(b.ptr), None, w, h, 2, 0, arr, None, p(c.ptr)),      # no such direction
                     (p(a.ptr), p(b.ptr), None, w, h, 1, 9, arr, None, None),          # too many filters
                     (p(a.ptr + 4), p(b.ptr), None, w, h, 1, 0, arr, None, None)):     # a flow that is not 8-byte aligned
            with pytest.raises(ValueError):
                _lib.check(lib.tf_flow_post_process_chain_dev(*args))
    finally:
        for buf in (a, b, c):
            buf.close()
