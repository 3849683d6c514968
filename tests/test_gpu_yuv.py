"""tf_yuv_* on the GPU against the numpy restatement of DESIGN.md section 21 (tests/yuv_ref.py), byte for byte: from a
host array (tf_yuv_convert) and from a resident frame (tf_yuv_convert_dev), at every alignment of input and output, with
nothing written outside the frame's bytes, and through the compositor."""
import numpy as np
import pytest

from tests import yuv_cases, yuv_ref

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def _first_difference(got: bytes, want: bytes) -> str:
    n = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at byte {n}: {got[n:n + 8].hex()} / {want[n:n + 8].hex()}"


class _At:
    """A frame at a device address, as FrameEncoder takes a CompImage."""

    def __init__(self, ptr, height, width):
        self.ptr, self.height, self.width = ptr, height, width

    def image_ptr(self):
        return self.ptr


def _check(cases):
    """Every case through both entry points."""
    from transflow_amd.pixmap import DevicePixmap
    from transflow_amd.yuv import YuvEncoder
    for name, rgb, layout, matrix, rng in cases:
        want = yuv_ref.convert(rgb, layout, matrix, rng)
        enc = YuvEncoder(rgb.shape[0], rgb.shape[1], layout, matrix, rng)
        try:
            assert enc.nbytes == len(want), name
            got = enc.encode(rgb)
            assert got == want, f"{name}, from the host: " + _first_difference(got, want)
            frame = enc.frame(DevicePixmap.from_host(np.array(rgb)))
            assert frame.tobytes() == want, f"{name}, resident: " + _first_difference(frame.tobytes(), want)
            assert (frame.shape, frame.layout, frame.matrix, frame.range) == (rgb.shape, layout, matrix, rng)
        finally:
            enc.close()


@pytest.mark.parametrize("layout", yuv_cases.LAYOUTS)
def test_sizes_around_the_lanes_and_the_waves_width(layout):
    _check(yuv_cases.size_cases(layout))


def test_the_other_matrices_and_ranges():
    _check(yuv_cases.pair_cases())


def test_a_frame_of_many_blocks():
    _check(yuv_cases.frame_cases())


def test_extremes_rounding_boundaries_and_clamped_chroma():
    _check(yuv_cases.extreme_cases())


@pytest.mark.parametrize("width", [5, 7, 64])
def test_every_alignment_of_the_input(width):
    """W = 5 and 7: the rows begin at every alignment in turn; and the whole frame 1, 2 and 3 bytes into an allocation."""
    from transflow_amd.device import DevBuffer
    from transflow_amd.yuv import YuvEncoder
    h = 6
    rgb = yuv_cases.noise(h, width, 31 + width)
    for layout in yuv_cases.LAYOUTS:
        want = yuv_ref.convert(rgb, layout)
        enc = YuvEncoder(h, width, layout)
        try:
            for offset in (0, 1, 2, 3):
                buf = DevBuffer.from_array(np.concatenate([np.zeros(offset, np.uint8), rgb.reshape(-1), np.zeros(8, np.uint8)]))
                got = enc.encode(_At(buf.ptr + offset, h, width))
                buf.close()
                assert got == want, f"{layout}, {offset} bytes in: " + _first_difference(got, want)
        finally:
            enc.close()


@pytest.mark.parametrize("layout", yuv_cases.LAYOUTS)
@pytest.mark.parametrize("width,height", [(1, 1), (3, 3), (17, 5), (65, 3)])
def test_nothing_is_written_outside_the_frames_bytes(layout, width, height):
    from transflow_amd.device import DevBuffer, sync
    from transflow_amd.pixmap import DevicePixmap
    from transflow_amd.yuv import YuvEncoder, frame_bytes
    rgb = yuv_cases.noise(height, width, 7)
    want = yuv_ref.convert(rgb, layout)
    n = frame_bytes(height, width, layout)
    assert n == len(want)
    enc = YuvEncoder(height, width, layout)
    pixmap = DevicePixmap.from_host(np.array(rgb))
    try:
        for before in (256, 257, 258, 259):                                 # the planes at every alignment too
            buf = DevBuffer.from_array(np.full(before + n + 256, CANARY, np.uint8))
            enc.convert_to_dev(pixmap, buf.ptr + before)
            sync()
            got = buf.download((before + n + 256,), np.uint8)
            buf.close()
            assert got[before:before + n].tobytes() == want, _first_difference(got[before:before + n].tobytes(), want)
            assert (got[:before] == CANARY).all() and (got[before + n:] == CANARY).all(), f"written outside, planes {before} bytes in"
    finally:
        enc.close()


def test_bad_arguments_are_refused_and_nothing_is_written():
    import ctypes as C

    from transflow_amd import _lib
    from transflow_amd.yuv import YuvEncoder
    lib = _lib.load()
    h = C.c_void_p()
    for args in ((0, 8, 2, 0, 0), (8, 70000, 2, 0, 0), (8, 8, 4, 0, 0), (8, 8, 2, 2, 0), (8, 8, 2, 0, 2)):
        assert lib.tf_yuv_create(C.byref(h), *args) == _lib.TF_ERR_ARG and not h.value
    rgb = yuv_cases.noise(4, 6, 2)
    enc = YuvEncoder(4, 6)
    try:
        out = np.full(enc.nbytes - 1, CANARY, np.uint8)
        with pytest.raises(ValueError):
            enc.encode_into(rgb, out)
        assert enc.last_needed == enc.nbytes and (out == CANARY).all()
        with pytest.raises(ValueError):
            enc.encode(yuv_cases.noise(4, 7, 2))
    finally:
        enc.close()


# ---- through the compositor --------------------------------------------------------------------------------------------
H, W, FRAMES = 21, 37, 3


class _HostSource:
    def __init__(self, array, introduction_mask):
        self.array, self.introduction_mask, self.counter = array, introduction_mask, -1

    def next(self, timeout=1):
        self.counter += 1
        return self.array

    @property
    def frame_number(self):
        return self.counter


def _render_all(**options):
    from oracle import remap_ref as OR
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    rng = np.random.default_rng(1)
    comp = HipCompositor.from_args(H, W, [LayerConfig(0, classname="moveref")], background_color="#204060", **options)
    comp.set_sources({0: [_HostSource(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), np.ones((H, W), bool))]})
    flows = np.random.default_rng(4)
    out = []
    try:
        for _ in range(FRAMES):
            comp.update(OR.post_process(flows.normal(0, 2.5, (H, W, 2)).astype(np.float32), OR.BACKWARD))
            frame = comp.render()
            out.append(frame if options else np.array(frame))               # (a raw frame is the pool's array: copy)
    finally:
        comp.close()
    return out


def test_compositor_returns_the_planes_of_its_plain_render():
    from transflow_amd.yuv import YuvFrame
    plain = _render_all()
    assert (plain[0] != plain[-1]).any()
    for layout in yuv_cases.LAYOUTS:
        frames = _render_all(yuv_frames=layout, yuv_matrix="bt709" if layout == "nv12" else None)
        matrix = "bt709" if layout == "nv12" else "bt601"
        for t, (frame, raw) in enumerate(zip(frames, plain)):
            assert isinstance(frame, YuvFrame) and frame.shape == (H, W, 3)
            assert (frame.layout, frame.matrix, frame.range) == (layout, matrix, "tv")
            want = yuv_ref.convert(raw, layout, matrix, "tv")
            assert frame.tobytes() == want, f"{layout}, frame {t}: " + _first_difference(frame.tobytes(), want)
    for a, b in zip(_render_all(), plain):                                  # the default compositor renders what it rendered
        np.testing.assert_array_equal(a, b)
