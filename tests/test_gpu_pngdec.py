"""Banded PNG frames decoded on the device (transflow_amd/pngdec.py, csrc/pngdec.hip): every valid
case of the corpus (tests/pngdec_cases.py) bit for bit the restatement's and Pillow's pixels in both orders, the device
encoder's own indexed files, the round trip through HipFramesOutput and a Farnebäck flow source, the pixmap source, every
malformed and hostile case rejected for its reason with the destination's surroundings intact, and the host's way for
files that are not for the device.

The unfilter kernel marches MARCH = 64 rows together (a wave's lanes): the corpus has heights MARCH - 1, MARCH, MARCH + 1
and 2 * MARCH + 1.  The inputs here are ones the host-checked core (tests/test_pngdec_ref.py) accepts or rejects
cleanly; none is there to provoke a fault."""
import ctypes as C
import io

import numpy as np
import PIL.Image
import pytest

from tests import png_ref as P
from tests import pngdec_cases as K
from tests import pngdec_ref as D

pytestmark = pytest.mark.gpu

MARCH = 64
assert D.MARCH_ROWS == MARCH


def pillow(data: bytes) -> np.ndarray:
    return np.array(PIL.Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.fixture(scope="module")
def decoder():
    from transflow_amd.pngdec import PngDecoder
    dec = PngDecoder(700, 260)
    yield dec
    dec.close()


# ---- correctness -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.valid()))
def test_decode_is_the_restatements_and_pillows_pixels(decoder, name):
    data, image = K.valid()[name]
    want = D.decode(data)
    np.testing.assert_array_equal(want, image)
    np.testing.assert_array_equal(pillow(data), image)
    rgb = decoder.decode(data)
    assert rgb._host is None and rgb.shape == image.shape
    np.testing.assert_array_equal(np.asarray(rgb), want)
    np.testing.assert_array_equal(np.asarray(decoder.decode(data, "bgr")), want[:, :, ::-1])
    assert decoder.fallbacks == 0


def test_golden_files_decode_to_their_pixels(decoder):
    import os
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pngdec_corpus.npz"))
    for i, name in enumerate(golden["names"]):
        np.testing.assert_array_equal(np.asarray(decoder.decode(golden[f"file_{i}"].tobytes())), golden[f"image_{i}"], err_msg=str(name))


ENCODER_CASES = [(1, 1, None), (1, 7, 1), (2, 5, 2), (3, 22, None), (4, 86, 1), (21, MARCH - 1, 5), (85, MARCH, MARCH),
                 (341, MARCH + 1, 7), (342, 2 * MARCH + 1, None), (700, 33, 16), (300, 40, None)]


@pytest.mark.parametrize("w,h,band_rows", ENCODER_CASES)
def test_the_device_encoders_indexed_files_come_back(decoder, w, h, band_rows):
    """PngEncoder(index=True): the restatement's file with the index put in, and through PngDecoder the image again; the
    images are noise and a smeared one whose rows take the other filter types."""
    from transflow_amd.png import PngEncoder
    from transflow_amd.pngdec import probe
    for image in (P.noise_image(h, w, 7 * w + h), P.smear_image(h, w, 3, 5, w + h)):
        enc = PngEncoder(h, w, band_rows, index=True)
        try:
            data = enc.encode(image)
            plain = P.encode(image, band_rows or 0)
            assert data == D.with_index(plain, enc.band_rows)
            info = probe(data)
            assert info.indexed and info.band_rows == enc.band_rows and info.within_bound
            np.testing.assert_array_equal(np.asarray(decoder.decode(data, info=info)), image)
            np.testing.assert_array_equal(np.asarray(decoder.decode(data, "bgr")), image[:, :, ::-1])
        finally:
            enc.close()
    # the default stays the parent's bytes
    enc = PngEncoder(h, w, band_rows)
    try:
        assert enc.encode(image) == plain
    finally:
        enc.close()


def test_a_rendered_frame_round_trips_on_the_device(decoder):
    from transflow_amd.pixmap import DevicePixmap
    from transflow_amd.png import PngEncoder
    y, x = np.mgrid[0:120, 0:200]
    frame = np.stack([(x * 3 + y) % 256, (x ^ y) % 256, np.where((x // 20 + y // 15) % 2, 240, 16)], axis=2).astype(np.uint8)
    frame[40:80, 50:150] = (32, 64, 96)
    enc = PngEncoder(120, 200, index=True)
    try:
        data = enc.encode(DevicePixmap.from_host(frame))
    finally:
        enc.close()
    assert len(set(P.filter_rows(frame)[0].tolist())) >= 2                     # more than one filter type is in it
    np.testing.assert_array_equal(np.asarray(decoder.decode(data)), frame)


# ---- the round trip through the outputs and the sources ----------------------------------------------------------------
H, W, FRAMES = 48, 64, 4


class _HostSource:
    def __init__(self, array, introduction_mask):
        self.array, self.introduction_mask, self.counter = array, introduction_mask, -1

    def next(self, timeout=1):
        self.counter += 1
        return self.array

    @property
    def frame_number(self):
        return self.counter


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    """(the template, the frames): FRAMES rendered frames written by HipFramesOutput from an indexed compositor."""
    from oracle import remap_ref as OR
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    from transflow_amd.output import HipFramesOutput
    from transflow_amd.png import PngFrame
    rng = np.random.default_rng(1)
    template = str(tmp_path_factory.mktemp("pngseq") / "%05d.png")
    comp = HipCompositor.from_args(H, W, [LayerConfig(0, classname="moveref")], background_color="#204060", png_frames="indexed")
    y, x = np.mgrid[0:H, 0:W]
    picture = np.stack([(x * 4) % 256, (y * 5) % 256, ((x // 8 + y // 8) % 2) * 200], axis=2).astype(np.uint8)
    comp.set_sources({0: [_HostSource(picture, np.ones((H, W), bool))]})
    frames = []
    try:
        with HipFramesOutput(template, W, H, initial_counter=1) as out:
            for _ in range(FRAMES):
                comp.update(OR.post_process(rng.normal(0, 2.5, (H, W, 2)).astype(np.float32), OR.BACKWARD))
                frame = comp.render()
                assert isinstance(frame, PngFrame)
                frames.append(frame.decode())
                out.feed(frame)
    finally:
        comp.close()
    assert (frames[0] != frames[-1]).any()
    return template, frames


def test_written_sequence_is_read_back_on_the_device(sequence):
    from transflow_amd.pixmap import DevicePixmap
    from transflow_amd.pngdec import PngSequenceFrameProvider, probe
    template, frames = sequence
    with open(template % 1, "rb") as f:
        assert probe(f.read()).indexed
    p = PngSequenceFrameProvider(template, framerate=30.0)
    assert (p.width, p.height, p.frame_count, p.framerate) == (W, H, FRAMES, 30.0)
    for want in frames:
        frame = p.read()
        assert isinstance(frame, DevicePixmap) and frame._host is None
        np.testing.assert_array_equal(np.asarray(frame), want[:, :, ::-1])
    assert p.read() is None and p.fallbacks == 0
    p.seek_start()
    np.testing.assert_array_equal(np.asarray(p.read("rgb")), frames[0])
    import pickle
    q = pickle.loads(pickle.dumps(p))                   # the handle stays behind
    assert q._decoder is None and q.fallbacks == 0 and q.pos == 1
    np.testing.assert_array_equal(np.asarray(q.read("rgb")), frames[1])
    q.release()
    p.release()
    host = PngSequenceFrameProvider(template, device_decode=False)
    np.testing.assert_array_equal(np.asarray(host.read()), frames[0][:, :, ::-1])
    assert host.fallbacks == 1


def _flows(provider, **kw):
    from transflow_amd.flow import HipFlowSource
    with HipFlowSource.from_args(provider, direction="backward", **kw) as source:
        return [np.array(f, copy=True) for f in source]


def test_farneback_flows_are_those_of_the_host_arrays(sequence):
    from transflow_amd.flow import ArrayFrameProvider
    from transflow_amd.pngdec import PngSequenceFrameProvider
    template, frames = sequence
    want = _flows(ArrayFrameProvider([np.ascontiguousarray(f[:, :, ::-1]) for f in frames], 25.0))
    provider = PngSequenceFrameProvider(template)
    got = _flows(provider)
    assert len(got) == len(want) == FRAMES - 1
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert provider.fallbacks == 0


def test_a_provider_grows_its_decoder_for_a_larger_frame():
    from transflow_amd.pngdec import PngSequenceFrameProvider
    small, large = K.valid()["zlib.40x24_random_b5"], K.valid()["zlib.300x40_smear_b7"]
    p = PngSequenceFrameProvider([small[0], large[0], small[0]])
    for _, image in (small, large, small):
        np.testing.assert_array_equal(np.asarray(p.read("rgb")), image)
    assert (p._decoder.max_width, p._decoder.max_height) == (300, 40) and p.fallbacks == 0
    p.release()


def _reference_loop(frames, seek, repeat):
    """pixmap/cv.py:24-62 over a list of frames: rewind, seek, the repeat loop."""
    pos, loop_index, out = (seek or 0), 1, []
    while True:
        if pos < len(frames):
            out.append(frames[pos])
            pos += 1
            continue
        if repeat == 0 or loop_index < repeat:
            loop_index += 1
            pos = seek or 0
            continue
        return out


def test_pixmap_source_loops_as_the_reference_does(sequence, tmp_path):
    from transflow_amd.pixmap import DevicePixmap, HipPixmapSource, HipPngSequencePixmapSource
    template, frames = sequence
    overlay = np.zeros((H, W, 4), np.uint8)
    overlay[5:9, 10:20] = (200, 10, 30, 255)
    alteration = str(tmp_path / "overlay.png")
    PIL.Image.fromarray(overlay).save(alteration)
    want = []
    for frame in _reference_loop(frames, 1, 2):
        a = frame.copy()
        a[5:9, 10:20] = (200, 10, 30)
        want.append(a)
    with HipPngSequencePixmapSource(template, seek=1, alteration_path=alteration, repeat=2) as source:
        assert (source.width, source.height, source.framerate, source.length) == (W, H, 25, 2 * FRAMES)
        got = list(source)
    assert len(got) == len(want) == 2 * (FRAMES - 1) and all(isinstance(g, DevicePixmap) for g in got)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(np.asarray(g), w)
    with HipPngSequencePixmapSource(template, seek_time=0.08) as source:          # 2 frames at 25 frames/s
        assert source.seek == 2 and source.length == FRAMES - 2
        got = list(source)
    assert len(got) == FRAMES - 2 and all(g._host is None for g in got)
    for g, w in zip(got, frames[2:]):
        np.testing.assert_array_equal(np.asarray(g), w)
    routed = HipPixmapSource.from_args(template, (W, H), seek=1, repeat=3)
    assert isinstance(routed, HipPngSequencePixmapSource) and (routed.seek, routed.repeat) == (1, 3)
    with pytest.raises(NotImplementedError):
        HipPixmapSource.from_args(str(tmp_path / "missing_%05d.png"), (W, H))


# ---- rejection ---------------------------------------------------------------------------------------------------------
GUARD = 3          # rows of the destination's width in front of and behind it


def _decode_between_guards(data: bytes, width: int, height: int, max_w: int = 700, max_h: int = 260):
    """tf_pngdec_decode_dev into the middle of a buffer filled with 0x5A: (status, reject word, the pixels, whether the
    guard rows are intact)."""
    from transflow_amd import _lib
    from transflow_amd.pixmap import _dev_alloc, _dev_download, _dev_upload
    lib = _lib.load()
    row = 3 * width
    total = (height + 2 * GUARD) * row
    buf = _dev_alloc(total)
    h = C.c_void_p()
    _lib.check(lib.tf_pngdec_create(C.byref(h), max_w, max_h, max(len(data), 1) + 64))
    try:
        _dev_upload(buf, np.full(max(4, total), 0x5A, np.uint8))
        reject = C.c_uint32()
        rc = lib.tf_pngdec_decode_dev(h, data, len(data), C.c_void_p(buf.ptr + GUARD * row), 0, C.byref(reject))
        out = _dev_download(buf, (max(4, total),))[:total]
    finally:
        lib.tf_pngdec_destroy(h)
        buf.close()
    intact = bool((out[:GUARD * row] == 0x5A).all() and (out[(GUARD + height) * row:] == 0x5A).all())
    return rc, reject.value, out[GUARD * row:(GUARD + height) * row].reshape(height, width, 3), intact


@pytest.mark.parametrize("name", sorted(K.malformed()))
def test_malformed_and_hostile_files_are_rejected_for_their_reason(decoder, name):
    from transflow_amd import _lib
    from transflow_amd.pngdec import PngRejected
    data, reason, where, at_walk = K.malformed()[name]
    with pytest.raises(PngRejected) as err:
        decoder.decode_or_host(data)
    assert (err.value.reason, err.value.where) == (reason, where)
    assert decoder.fallbacks == 0                       # corrupt data is not masked by the host's way
    if not at_walk:
        lay = D.walk(data)
        rc, word, _, intact = _decode_between_guards(data, lay.width, lay.height)
        assert rc == _lib.TF_ERR_STATE and word == D.REJECT_NUMBER[reason] | ((where or 0) << 8)
        assert intact


def test_nothing_is_written_around_the_destination():
    from transflow_amd import _lib
    for name in ("zlib.3x5_random_b2", "zlib.22x5_random_b2", "zlib.5x65_paeth_b2", "zlib.341x5_random_b2"):
        data, image = K.valid()[name]
        rc, word, pixels, intact = _decode_between_guards(data, image.shape[1], image.shape[0])
        assert (rc, word) == (_lib.TF_OK, 0) and intact, name
        np.testing.assert_array_equal(pixels, image)


def test_inconsistent_arguments_are_refused_before_anything_runs():
    from transflow_amd import _lib
    from transflow_amd.pngdec import PngDecoder
    data, image = K.valid()["zlib.40x24_random_b5"]
    rc, word, _, intact = _decode_between_guards(data, 40, 24, max_w=39, max_h=24)     # beyond the handle: `size`
    assert rc == _lib.TF_ERR_STATE and word == D.REJECT_NUMBER["size"] and intact
    rc, word, _, intact = _decode_between_guards(K.host()["pillow_rgb"][0], 14, 9)     # not for the device
    assert rc == _lib.TF_ERR_ARG and word == 0 and intact
    small = PngDecoder(39, 24)
    try:
        with pytest.raises(ValueError):
            small.decode(data)
        with pytest.raises(ValueError):
            small.decode(K.host()["rgba"][0])
    finally:
        small.close()


def test_a_rejected_frame_of_a_sequence_names_the_frame():
    from transflow_amd.pngdec import PngRejected, PngSequenceFrameProvider
    good = K.valid()["zlib.40x24_random_b5"][0]
    image = P.noise_image(24, 40, 11)
    bad = D.build(image, 5, filters=[0] * 10 + [5] + [0] * 13)
    p = PngSequenceFrameProvider([good, good, bad])
    assert p.read() is not None and p.read() is not None
    with pytest.raises(PngRejected) as err:
        p.read()
    assert (err.value.reason, err.value.where, err.value.frame) == ("filter_type", 10, 2)
    assert p.fallbacks == 0
    p.release()


# ---- the host's way ----------------------------------------------------------------------------------------------------
def test_files_not_for_the_device_go_the_hosts_way():
    from transflow_amd.pngdec import PngDecoder
    dec = PngDecoder(700, 500)
    try:
        files = [v[0] for v in K.host().values()] + [v[0] for v in K.bound().values()]
        for n, data in enumerate(files, 1):
            for order in ("rgb", "bgr"):
                got = np.asarray(dec.decode_or_host(data, order))
                want = pillow(data)
                np.testing.assert_array_equal(got, want if order == "rgb" else want[:, :, ::-1])
            assert dec.fallbacks == 2 * n
        for data, _ in K.bound().values():          # `decode` itself gives the device nothing beyond the bound
            with pytest.raises(ValueError, match="beyond the bound"):
                dec.decode(data)
    finally:
        dec.close()
