"""tf_yuvdec_* on the GPU against the numpy restatement of DESIGN.md section 22 (tests/yuvdec_ref.py), byte for byte: from a
host frame (tf_yuvdec_convert) and from resident planes (tf_yuvdec_convert_dev), at every alignment of input and output,
with nothing written outside the frame's bytes, back from the YUV encoder on the device, and through a flow source and
a pixmap source over a Y4M file."""
import numpy as np
import pytest

from tests import yuv_cases, yuv_ref, yuvdec_cases as K, yuvdec_ref as D

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def _first_difference(got: np.ndarray, want: np.ndarray) -> str:
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    at = np.argwhere(got != want)
    return f"{len(at)} bytes differ, the first at (y, x, c) = {tuple(at[0])}: {got[tuple(at[0])]} / {want[tuple(at[0])]}"


@pytest.fixture(scope="module")
def decoder():
    from transflow_amd.yuvdec import YuvDecoder
    dec = YuvDecoder(520, 300)
    yield dec
    dec.close()


def _check(dec, cases):
    """Every case through both entry points."""
    from transflow_amd.device import DevBuffer
    n = 0
    for case in cases:
        name, data, w, h, layout, matrix, rng, chroma, order = case
        want = K.want(case)
        pixmap = dec.decode(data, w, h, layout, matrix, rng, chroma, order)
        got = np.asarray(pixmap)
        assert pixmap.shape == (h, w, 3) and (got == want).all(), f"{name}, from the host: " + _first_difference(got, want)
        pixmap.close()
        planes = DevBuffer.from_array(data)
        pixmap = dec.decode_dev(planes.ptr, data.nbytes, w, h, layout, matrix, rng, chroma, order)
        got = np.asarray(pixmap)
        assert (got == want).all(), f"{name}, resident: " + _first_difference(got, want)
        pixmap.close(), planes.close()
        n += 1
    assert n


@pytest.mark.parametrize("chroma", K.CHROMAS)
@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_sizes_around_the_lanes_and_the_waves_width(decoder, layout, chroma):
    _check(decoder, K.size_cases(layout, chroma))


def test_the_other_matrices_and_ranges_in_the_other_order(decoder):
    _check(decoder, K.pair_cases())


def test_both_orders(decoder):
    _check(decoder, K.order_cases())


def test_a_frame_of_many_blocks(decoder):
    _check(decoder, K.frame_cases())


def test_extremes_level_combinations_and_rounding_boundaries(decoder):
    _check(decoder, K.extreme_cases())


def test_the_linear_filter_and_none_of_its_wrong_forms(decoder):
    _check(decoder, K.filter_cases())


def test_frames_queued_back_to_back_do_not_share_the_staging_buffer(decoder):
    """Nothing waits between the calls: the second frame must not reach the staging buffer before the first has left."""
    cases = [(f"queued-{k}", K.noise(480, 270, "yuv420p", 90 + k), 480, 270, "yuv420p", "bt601", "tv", "linear", "bgr") for k in range(4)]
    pixmaps = [decoder.decode(c[1], *c[2:]) for c in cases]
    for case, pixmap in zip(cases, pixmaps):
        got, want = np.asarray(pixmap), K.want(case)
        assert (got == want).all(), f"{case[0]}: " + _first_difference(got, want)
        pixmap.close()


@pytest.mark.parametrize("width", [5, 7, 64])
def test_every_alignment_of_the_input(decoder, width):
    """W = 5 and 7: the rows begin at every alignment in turn; and the planes 1, 2 and 3 bytes into an allocation."""
    from transflow_amd.device import DevBuffer
    h = 6
    for layout in K.LAYOUTS:
        for chroma in K.CHROMAS:
            case = ("", K.noise(width, h, layout, 31 + width), width, h, layout, "bt601", "tv", chroma, "rgb")
            want = K.want(case)
            for offset in (0, 1, 2, 3):
                buf = DevBuffer.from_array(np.concatenate([np.zeros(offset, np.uint8), case[1], np.zeros(8, np.uint8)]))
                pixmap = decoder.decode_dev(buf.ptr + offset, case[1].nbytes, width, h, layout, chroma=chroma, order="rgb")
                got = np.asarray(pixmap)
                pixmap.close(), buf.close()
                assert (got == want).all(), f"{layout}, {chroma}, {offset} bytes in: " + _first_difference(got, want)


@pytest.mark.parametrize("chroma", K.CHROMAS)
@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("width,height", [(1, 1), (3, 3), (8, 2), (17, 5), (65, 3)])
def test_nothing_is_written_outside_the_frames_bytes(decoder, layout, chroma, width, height):
    from transflow_amd.device import DevBuffer, sync
    case = ("", K.noise(width, height, layout, 7), width, height, layout, "bt601", "tv", chroma, "bgr")
    want = K.want(case).reshape(-1)
    n = 3 * width * height
    planes = DevBuffer.from_array(case[1])
    try:
        for before in (256, 257, 258, 259):                                 # the output at every alignment too
            buf = DevBuffer.from_array(np.full(before + n + 256, CANARY, np.uint8))
            for entry in ("host", "resident"):
                if entry == "host":
                    decoder.convert_into(case[1], width, height, layout, buf.ptr + before, chroma=chroma)
                else:
                    decoder.convert_dev_into(planes.ptr, case[1].nbytes, width, height, layout, buf.ptr + before, chroma=chroma)
                sync()
                got = buf.download((before + n + 256,), np.uint8)
                assert (got[before:before + n] == want).all(), f"{entry}, the output {before} bytes in"
                assert (got[:before] == CANARY).all() and (got[before + n:] == CANARY).all(), f"{entry}: written outside, {before} bytes in"
            buf.close()
    finally:
        planes.close()


@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_back_from_the_encoders_planes_on_the_device(layout):
    """RGB -> tf_yuv_convert_to_dev -> tf_yuvdec_convert_dev, nothing coming down in between: the CPU round trip."""
    from transflow_amd.device import DevBuffer
    from transflow_amd.pixmap import DevicePixmap
    from transflow_amd.yuv import YuvEncoder
    from transflow_amd.yuvdec import YuvDecoder
    h, w = 37, 61
    rgb = yuv_cases.noise(h, w, 12)
    enc, dec = YuvEncoder(h, w, layout, "bt709", "pc"), YuvDecoder(w, h)
    planes = DevBuffer(enc.nbytes)
    try:
        enc.convert_to_dev(DevicePixmap.from_host(np.array(rgb)), planes.ptr)
        for chroma in K.CHROMAS:
            pixmap = dec.decode_dev(planes.ptr, enc.nbytes, w, h, layout, "bt709", "pc", chroma, "rgb")
            got = np.asarray(pixmap)
            want = D.convert_back(yuv_ref.convert(rgb, layout, "bt709", "pc"), w, h, layout, "bt709", "pc", chroma)
            assert (got == want).all(), f"{chroma}: " + _first_difference(got, want)
            if layout == "yuv444p":
                assert np.abs(got.astype(int) - rgb).max() <= 1         # section 22's bound for both pc pairs
            pixmap.close()
    finally:
        enc.close(), dec.close(), planes.close()


def test_bad_arguments_are_refused_and_nothing_is_written():
    import ctypes as C

    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer, sync
    from transflow_amd.yuvdec import YuvDecoder
    lib = _lib.load()
    h = C.c_void_p()
    for args in ((0, 8), (8, 0), (70000, 8), (8, 70000)):
        assert lib.tf_yuvdec_create(C.byref(h), *args) == _lib.TF_ERR_ARG and not h.value
    assert lib.tf_yuvdec_create(None, 8, 8) == _lib.TF_ERR_ARG
    w, height = 6, 4
    data = K.noise(w, height, "yuv420p", 2)
    dec = YuvDecoder(8, 4)
    out = DevBuffer.from_array(np.full(3 * 8 * 4 + 64, CANARY, np.uint8))
    planes = DevBuffer.from_array(data)
    good = dict(nbytes=data.nbytes, width=w, height=height, layout=2, matrix=0, range=0, chroma=0, order=1)
    try:
        for change in (dict(layout=4), dict(layout=-1), dict(matrix=2), dict(range=2), dict(chroma=2), dict(chroma=-1), dict(order=2),
                       dict(width=9, nbytes=9 * 4 + 2 * 5 * 2), dict(height=5, nbytes=6 * 5 + 2 * 3 * 3), dict(width=0), dict(height=0),
                       dict(nbytes=data.nbytes - 1), dict(nbytes=data.nbytes + 1), dict(layout=0)):
            a = {**good, **change}
            tail = (a["width"], a["height"], a["layout"], a["matrix"], a["range"], a["chroma"], C.c_void_p(out.ptr), a["order"])
            assert lib.tf_yuvdec_convert(dec._h, C.c_void_p(data.ctypes.data), a["nbytes"], *tail) == _lib.TF_ERR_ARG, change
            assert lib.tf_yuvdec_convert_dev(dec._h, C.c_void_p(planes.ptr), a["nbytes"], *tail) == _lib.TF_ERR_ARG, change
        tail = (w, height, 2, 0, 0, 0, C.c_void_p(out.ptr), 1)
        assert lib.tf_yuvdec_convert(None, C.c_void_p(data.ctypes.data), data.nbytes, *tail) == _lib.TF_ERR_ARG
        assert lib.tf_yuvdec_convert(dec._h, None, data.nbytes, *tail) == _lib.TF_ERR_ARG
        assert lib.tf_yuvdec_convert_dev(dec._h, C.c_void_p(planes.ptr), data.nbytes, w, height, 2, 0, 0, 0, None, 1) == _lib.TF_ERR_ARG
        sync()
        assert (out.download((3 * 8 * 4 + 64,), np.uint8) == CANARY).all()
        with pytest.raises(ValueError):
            dec.decode(data, 9, 4, "yuv420p")
        with pytest.raises(ValueError):
            dec.decode(data[:-1], w, height, "yuv420p")
        np.testing.assert_array_equal(np.asarray(dec.decode(data, w, height, "yuv420p")), D.convert_back(data, w, height, "yuv420p", order="bgr"))
    finally:
        dec.close(), out.close(), planes.close()


# ---- a Y4M clip under a flow source and a pixmap source -------------------------------------------------------------------
W, H, FRAMES = 64, 48, 4


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """(path, the frames' bytes): a coarse pattern that moves two pixels a frame, as yuv420p planes in a Y4M file."""
    coarse = np.random.default_rng(21).integers(0, 256, (H // 4, W // 4, 3), dtype=np.uint8).repeat(4, axis=0).repeat(4, axis=1)
    frames = [yuv_ref.convert(np.roll(coarse, (k, 2 * k), axis=(0, 1)), "yuv420p") for k in range(FRAMES)]
    path = tmp_path_factory.mktemp("yuvdec") / "clip.y4m"
    path.write_bytes(D.build_y4m(frames, W, H, tag="C420mpeg2", frame_params="Ip"))
    return str(path), frames


def _flows(provider, **kw):
    from transflow_amd.flow import HipFlowSource
    with HipFlowSource.from_args(provider, direction="backward", **kw) as source:
        return [np.array(f, copy=True) for f in source]


@pytest.mark.parametrize("chroma", K.CHROMAS)
def test_farneback_flows_are_those_of_the_host_arrays(clip, chroma):
    from transflow_amd.flow import ArrayFrameProvider
    from transflow_amd.yuvdec import Y4mFrameProvider
    path, frames = clip
    want = _flows(ArrayFrameProvider([D.convert_back(f, W, H, "yuv420p", chroma=chroma, order="bgr") for f in frames], 25.0))
    provider = Y4mFrameProvider(path, chroma=chroma)
    assert (provider.width, provider.height, provider.frame_count, provider.siting) == (W, H, FRAMES, "C420mpeg2")
    got = _flows(provider)
    assert len(got) == len(want) == FRAMES - 1 and any(np.abs(w).max() > 0 for w in want)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()


def test_pixmap_source_yields_the_restatements_rgb_and_loops(clip):
    from transflow_amd.pixmap import DevicePixmap, HipPixmapSource, HipY4mPixmapSource
    path, frames = clip
    rgb = [D.convert_back(f, W, H, "yuv420p", "bt709", "tv", "linear") for f in frames]
    with HipY4mPixmapSource(path, seek=1, repeat=2, matrix="bt709", chroma="linear") as source:
        assert (source.width, source.height, source.framerate, source.length) == (W, H, 25, 2 * FRAMES)
        got = list(source)
    assert len(got) == 2 * (FRAMES - 1) and all(isinstance(g, DevicePixmap) and g._host is None for g in got)
    for g, w in zip(got, rgb[1:] + rgb[1:]):
        np.testing.assert_array_equal(np.asarray(g), w)
    with HipPixmapSource.from_args(path, (W, H), seek_time=0.08, y4m_inputs=True) as source:      # 2 frames at 25 frames/s
        assert isinstance(source, HipY4mPixmapSource) and source.seek == 2 and source.length == FRAMES - 2
        got = list(source)
    assert len(got) == FRAMES - 2
    for g, f in zip(got, frames[2:]):
        np.testing.assert_array_equal(np.asarray(g), D.convert_back(f, W, H, "yuv420p"))
