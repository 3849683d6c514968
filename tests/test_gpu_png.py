"""tf_png_* on the GPU against the numpy restatement of its format (tests/png_ref.py), whole files byte for byte, and --
independently of the restatement -- against Pillow's decoder: the file holds the frame's pixels exactly."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

from tests import png_ref

pytestmark = pytest.mark.gpu

_wanted = {}


def _case(name):
    """(image, band_rows, the restatement's file): made once and left as they are."""
    if name not in _wanted:
        image, band_rows = png_ref.case(name)
        image.setflags(write=False)
        _wanted[name] = (image, band_rows, png_ref.encode(image, band_rows))
    return _wanted[name]


def _first_difference(got: bytes, want: bytes) -> str:
    n = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at byte {n}: {got[n:n + 8].hex()} / {want[n:n + 8].hex()}"


def _decode(data: bytes) -> np.ndarray:
    import PIL.Image
    with PIL.Image.open(io.BytesIO(data)) as im:
        assert im.mode == "RGB"
        return np.asarray(im)


@pytest.mark.parametrize("name", list(png_ref.CASES))
def test_encoder_writes_the_restatements_file_and_pillow_reads_the_pixels(name):
    from transflow_amd.png import PngEncoder
    image, band_rows, want = _case(name)
    enc = PngEncoder(image.shape[0], image.shape[1], band_rows or None)
    try:
        assert enc.band_rows == min(image.shape[0], band_rows or png_ref.default_band_rows(*image.shape[:2]))
        got = enc.encode(image)
    finally:
        enc.close()
    np.testing.assert_array_equal(_decode(got), image)                    # whatever the restatement says
    chunks = png_ref.chunks(got)
    assert all(crc == zlib.crc32(kind + payload) for kind, payload, crc in chunks)
    idat = b"".join(payload for kind, payload, _ in chunks if kind == b"IDAT")
    assert len(zlib.decompress(idat)) == image.shape[0] * (3 * image.shape[1] + 1)      # zlib checks the Adler-32
    assert got == want, _first_difference(got, want)
    if name in png_ref.NOISE_CASES:                                        # staging is sized by the bound: no file exceeds it
        bound = png_ref.file_bound(image.shape[0], image.shape[1], band_rows)
        print(f"{name}: {len(got)} bytes, bound {bound}")
        assert len(got) <= bound


def test_one_encoder_keeps_no_state_between_images():
    """Noise, then a flat image whose bands are a few bytes behind the table header, then the noise again: bits left in
    the LDS buffer or the staging slots would show in the second file."""
    from transflow_amd.png import PngEncoder
    a, band_rows, want_a = _case("24x40_noise_b5")
    b = np.empty((24, 40, 3), np.uint8)
    b[:] = (90, 160, 30)
    want_b = png_ref.encode(b, band_rows)
    assert len(want_b) < len(want_a) // 3
    enc = PngEncoder(24, 40, band_rows)
    try:
        assert enc.encode(a) == want_a
        assert enc.encode(b) == want_b
        assert enc.encode(a) == want_a
    finally:
        enc.close()


def test_device_inputs_give_the_host_arrays_bytes():
    from transflow_amd.pixmap import DevicePixmap
    from transflow_amd.png import PngEncoder, PngFrame
    from transflow_amd.remap import CompImage
    image, band_rows, want = _case("24x40_noise_b3")
    enc = PngEncoder(24, 40, band_rows)
    pixmap = DevicePixmap.from_host(np.array(image))
    comp = CompImage(24, 40, (10, 200, 90))
    try:
        assert enc.encode(pixmap) == want
        comp.begin()
        flat = np.empty((24, 40, 3), np.uint8)
        flat[:] = (10, 200, 90)
        assert enc.encode(comp) == png_ref.encode(flat, band_rows)
        frame = enc.frame(pixmap)
        assert isinstance(frame, PngFrame) and frame.data == want
        assert (frame.shape, frame.band_rows) == ((24, 40, 3), band_rows)
        np.testing.assert_array_equal(frame.decode(), image)
        with pytest.raises(ValueError):
            enc.encode(np.zeros((24, 39, 3), np.uint8))
    finally:
        enc.close()
        pixmap.close()
        comp.close()


def test_bad_arguments_are_refused():
    from transflow_amd.png import PngEncoder
    for args in ((0, 8), (8, 0), (8, 8, -1), (70000, 8), (8, 70000)):
        with pytest.raises(ValueError):
            PngEncoder(*args)


@pytest.mark.parametrize("name", ["24x40_noise_b5", "2049x2_b1", "4x85_tail_b1"])
def test_a_buffer_one_byte_short_is_refused_and_left_alone(name):
    """2049 bands: the same contract where k_png_pack's offsets come from the second and third trips of k_slot_scan.
    Bands of 256 bytes: where end-of-block's lane is alone in its block of trips."""
    from transflow_amd.png import PngEncoder
    image, band_rows, want = _case(name)
    enc = PngEncoder(image.shape[0], image.shape[1], band_rows)
    try:
        guard = 64
        buf = np.full(len(want) + guard, 0xA5, np.uint8)
        with pytest.raises(ValueError):
            enc.encode_into(image, buf[:len(want) - 1])
        assert enc.last_needed == len(want)                                # the library says what it takes
        assert (buf == 0xA5).all()                                         # nothing written, within or beyond
        for capacity in (0, 10, 47, 52, len(want) // 2, len(want) - 33):
            with pytest.raises(ValueError):
                enc.encode_into(image, buf[:capacity])
            assert enc.last_needed == len(want) and (buf == 0xA5).all()
        exact = buf[:len(want)]
        assert enc.encode_into(image, exact) == len(want)
        assert exact.tobytes() == want and (buf[len(want):] == 0xA5).all()
    finally:
        enc.close()


def test_a_file_larger_than_the_encoders_buffer_is_packed_again_not_encoded_again():
    from transflow_amd import _lib
    from transflow_amd.png import PngEncoder
    lib = _lib.load()
    image, band_rows, want = _case("24x40_noise_b5")
    enc = PngEncoder(24, 40, band_rows)
    try:
        n = C.c_size_t()
        small = np.zeros(700, np.uint8)
        rc = lib.tf_png_copy_last(enc._h, C.c_void_p(small.ctypes.data), small.nbytes, C.byref(n))
        assert rc == _lib.TF_ERR_STATE                                     # nothing encoded yet
        enc._out = small                                                   # far too small
        _lib.profile(True, "png_")
        try:
            assert enc.encode(image) == want
            report = _lib.profile_report()
        finally:
            _lib.profile(False)
        assert report["png_filter"][0] == 1 and report["png_deflate"][0] == 1 and report["png_pack"][0] == 2
        assert enc._out.nbytes == len(want) and (small == 0).all()
        with pytest.raises(ValueError):                                    # a wrong shape is not mistaken for a short buffer
            enc.encode(np.zeros((24, 41, 3), np.uint8))
    finally:
        enc.close()


@pytest.mark.parametrize("code, launches", [
    ("fixed", {"png_filter": 1, "png_deflate": 1, "png_scan": 1, "png_pack": 1}),
    ("frame", {"png_filter": 1, "png_count": 1, "png_total": 1, "png_table": 1, "png_deflate": 1, "png_scan": 1, "png_pack": 1}),
])
def test_an_encode_and_a_copy_last_launch_what_they_always_did(code, launches):
    """Every label and count of one encode into a buffer that is large enough, and of one tf_png_copy_last: a single
    pack.  Then tf_png_set_index: the head of that file is gone, and there is nothing to copy again."""
    from transflow_amd import _lib
    from transflow_amd.png import PngEncoder
    image = np.random.default_rng(7).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    enc = PngEncoder(16, 16, 5, code=code)
    try:
        out, again, n = np.zeros(1 << 12, np.uint8), np.full(1 << 12, 0xA5, np.uint8), C.c_size_t()
        _lib.profile(True, "png_")
        try:
            size = enc.encode_into(image, out)
            encode = {label: count for label, (count, _) in _lib.profile_report().items()}
            _lib.profile(True, "png_")                                    # (resets the counts)
            _lib.check(enc._lib.tf_png_copy_last(enc._h, C.c_void_p(again.ctypes.data), again.nbytes, C.byref(n)))
            copy = {label: count for label, (count, _) in _lib.profile_report().items()}
        finally:
            _lib.profile(False)
        assert encode == launches
        assert copy == {"png_pack": 1}
        assert n.value == size and again[:size].tobytes() == out[:size].tobytes()
        np.testing.assert_array_equal(_decode(out[:size].tobytes()), image)
        again[:] = 0xA5
        _lib.check(enc._lib.tf_png_set_index(enc._h, 1))
        rc = enc._lib.tf_png_copy_last(enc._h, C.c_void_p(again.ctypes.data), again.nbytes, C.byref(n))
        assert rc == _lib.TF_ERR_STATE and n.value == 0 and (again == 0xA5).all()
        indexed = enc.encode_into(image, again)                           # the next encode has the new head
        assert indexed > size and b"tfBX" in again[:indexed].tobytes()
    finally:
        enc.close()


def test_abi_reports_the_needed_size():
    """tf_png_encode_dev itself: TF_ERR_ARG and *n_bytes for a short buffer, device pointer in."""
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer
    lib = _lib.load()
    image, band_rows, want = _case("24x40_noise_b2")
    h = C.c_void_p()
    _lib.check(lib.tf_png_create(C.byref(h), 24, 40, band_rows))
    dev = DevBuffer.from_array(np.array(image))
    try:
        out = np.full(len(want) + 16, 0x5A, np.uint8)
        n = C.c_size_t()
        rc = lib.tf_png_encode_dev(h, C.c_void_p(dev.ptr), C.c_void_p(out.ctypes.data), len(want) - 1, C.byref(n))
        assert rc == _lib.TF_ERR_ARG and n.value == len(want) and (out == 0x5A).all()
        rc = lib.tf_png_encode_dev(h, C.c_void_p(dev.ptr), C.c_void_p(out.ctypes.data), out.nbytes, C.byref(n))
        assert rc == _lib.TF_OK and out[:n.value].tobytes() == want and (out[n.value:] == 0x5A).all()
    finally:
        lib.tf_png_destroy(h)
        dev.close()


# ---- the compositor returns the file ------------------------------------------------------------------------------------
H, W, FRAMES = 48, 64, 3


class _HostSource:
    def __init__(self, array, introduction_mask):
        self.array, self.introduction_mask, self.counter = array, introduction_mask, -1

    def next(self, timeout=1):
        self.counter += 1
        return self.array

    @property
    def frame_number(self):
        return self.counter


def _flows(seed, device):
    from oracle import remap_ref as OR
    rng = np.random.default_rng(seed)
    flows = [OR.post_process((rng.normal(0, 2.5, (H, W, 2))).astype(np.float32), OR.BACKWARD) for _ in range(FRAMES)]
    if not device:
        return flows
    from transflow_amd.device import DevBuffer
    from transflow_amd.deviceflow import DeviceFlow, _Event
    out = []
    for f in flows:
        buf = DevBuffer.from_array(f)
        ev = _Event()
        ev.record()
        flow = DeviceFlow(f.shape, buf.ptr, ev, owner=buf)
        flow.in_frame = True                 # clipped by post_process: the one-launch step may take it
        out.append(flow)
    return out


def _render_all(layers, device_flows, png_frames, deferred=None):
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    rng = np.random.default_rng(1)
    comp = HipCompositor.from_args(H, W, [LayerConfig(i, classname=c) for i, c in enumerate(layers)],
                                   background_color="#204060", png_frames=png_frames)
    masks = [np.ones((H, W), bool), np.zeros((H, W), bool)]
    masks[1][H // 3:, 5:W // 2] = True
    comp.set_sources({i: [_HostSource(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), masks[i])] for i in range(len(layers))})
    out = []
    try:
        for flow in _flows(4, device_flows):
            comp.update(flow)
            if deferred is not None:
                deferred.append(comp.layers[0]._deferred is not None)
            frame = comp.render()
            out.append(frame if png_frames else np.array(frame))           # (a raw frame is the pool's array: copy)
    finally:
        comp.close()
    return out


@pytest.mark.parametrize("layers,device_flows", [(["moveref", "sum"], False), (["moveref"], True)],
                         ids=["two_layers", "deferred_single_layer"])
def test_compositor_returns_the_file_of_its_plain_render(layers, device_flows):
    from transflow_amd.png import PngFrame
    deferred = []
    plain = _render_all(layers, device_flows, False)
    files = _render_all(layers, device_flows, True, deferred)
    assert deferred == [device_flows] * FRAMES                             # the one-launch path is the one under test
    assert (plain[0] != plain[-1]).any()
    for t, (frame, raw) in enumerate(zip(files, plain)):
        assert isinstance(frame, PngFrame) and frame.shape == (H, W, 3)
        assert frame.band_rows == png_ref.default_band_rows(H, W)
        np.testing.assert_array_equal(frame.decode(), raw, err_msg=f"frame {t}")
        want = png_ref.encode(raw)
        assert frame.data == want, f"frame {t}: " + _first_difference(frame.data, want)
