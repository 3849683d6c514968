"""What MjpegFrameProvider and PngSequenceFrameProvider share (transflow_amd/framecodec.py: CompressedFrameProvider) and
where they differ, without a device: a provider's constructor reads headers only, a frame that goes the host's way is
Pillow's, and `DevicePixmap.from_host` is replaced by the identity so that such a frame stays on the host."""
import io
import pickle

import numpy as np
import PIL.Image
import pytest

from transflow_amd import jpegdec, pngdec
from transflow_amd.framecodec import pillow_decode
from transflow_amd.pixmap import DevicePixmap

W, H = 40, 24


def _image(k: int) -> PIL.Image.Image:
    return PIL.Image.fromarray(np.random.default_rng(k).integers(0, 256, (H, W, 3), dtype=np.uint8))


def _file(kind: str, k: int, **options) -> bytes:
    out = io.BytesIO()
    _image(k).save(out, {"jpeg": "JPEG", "png": "PNG"}[kind], **options)
    return out.getvalue()


PROVIDER = {"jpeg": jpegdec.MjpegFrameProvider, "png": pngdec.PngSequenceFrameProvider}
EXT = {"jpeg": "jpg", "png": "png"}
EMPTY = {"jpeg": "the MJPEG source holds no frame", "png": "the PNG sequence holds no frame"}
KINDS = ("jpeg", "png")


@pytest.fixture(autouse=True)
def host_pixmaps(monkeypatch):
    monkeypatch.setattr(DevicePixmap, "from_host", classmethod(lambda cls, array: array))


class FakeDecoder:
    """Stands where a provider's DECODER is: no handle, `decode_or_host` says which decoder got the frame."""

    made = []

    def __init__(self, max_width, max_height, device=None):
        self.max_width, self.max_height, self.fallbacks, self.closed = max_width, max_height, 0, False
        FakeDecoder.made.append(self)

    def decode_or_host(self, raw, order, info):
        assert not self.closed
        return self, order, (info.width, info.height)

    def close(self):
        self.closed = True


@pytest.fixture
def fake_decoder(monkeypatch):
    FakeDecoder.made = []
    for provider in PROVIDER.values():
        monkeypatch.setattr(provider, "DECODER", FakeDecoder)
    return FakeDecoder


@pytest.mark.parametrize("kind", KINDS)
def test_a_pattern_lists_the_same_frames_from_0_and_from_1(kind, tmp_path):
    files = [_file(kind, k) for k in range(3)]
    got = []
    for first in (0, 1):
        folder = tmp_path / f"from{first}"
        folder.mkdir()
        for k, data in enumerate(files):
            (folder / f"{first + k:03d}.{EXT[kind]}").write_bytes(data)
        (folder / f"{first + 4:03d}.{EXT[kind]}").write_bytes(files[0])          # behind a gap: not part of the sequence
        p = PROVIDER[kind](str(folder / f"%03d.{EXT[kind]}"), device_decode=False)
        assert (p.frame_count, p.width, p.height) == (3, W, H)
        got.append([p.read("rgb") for _ in range(3)])
        assert p.fallbacks == 3
    for a, b, data in zip(got[0], got[1], files):
        np.testing.assert_array_equal(a, pillow_decode(data))
        np.testing.assert_array_equal(b, pillow_decode(data))


@pytest.mark.parametrize("kind", KINDS)
def test_a_pattern_without_its_first_frame_is_no_file(kind, tmp_path):
    (tmp_path / f"002.{EXT[kind]}").write_bytes(_file(kind, 0))
    with pytest.raises(FileNotFoundError):
        PROVIDER[kind](str(tmp_path / f"%03d.{EXT[kind]}"))


@pytest.mark.parametrize("kind", KINDS)
def test_an_empty_source_is_refused_in_the_providers_own_words(kind):
    with pytest.raises(ValueError) as err:
        PROVIDER[kind]([])
    assert str(err.value) == EMPTY[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_read_ends_with_none_and_seek_start_rewinds(kind):
    files = [_file(kind, k) for k in range(2)]
    p = PROVIDER[kind](files, framerate=30, size=(80, 48), device_decode=False)
    assert (p.framerate, p.width, p.height, p.frame_count, p.pos) == (30.0, 80, 48, 2, 0)
    first = p.read()
    np.testing.assert_array_equal(first, pillow_decode(files[0], "bgr"))         # BGR unless asked otherwise
    assert p.read() is not None and p.pos == 2
    assert p.read() is None and p.read() is None and p.pos == 2
    p.seek_start()
    assert p.pos == 0
    np.testing.assert_array_equal(p.read(), first)
    p.release()
    assert p.fallbacks == 3


@pytest.mark.parametrize("kind", KINDS)
def test_pickling_drops_the_decoder_and_keeps_the_count(kind, fake_decoder):
    files = [_file(kind, k) for k in range(3)]
    p = PROVIDER[kind](files, device_decode=False)
    p.read(), p.read()
    p._decoder = fake_decoder(W, H)
    p._decoder.fallbacks = 5
    assert p.fallbacks == 7
    q = pickle.loads(pickle.dumps(p))
    assert q._decoder is None and q.fallbacks == 7 and q.pos == 2
    assert p._decoder is not None and not p._decoder.closed                     # the original keeps its own
    np.testing.assert_array_equal(q.read("rgb"), pillow_decode(files[2]))
    assert q.fallbacks == 8
    p.release()
    assert p._decoder is None and p.fallbacks == 7 and fake_decoder.made[0].closed


def test_a_mapped_stream_file_is_indexed_read_and_pickled_without_its_mapping(tmp_path):
    files = [_file("jpeg", k) for k in range(3)]
    path = tmp_path / "clip.mjpeg"
    path.write_bytes(b"".join(files))
    p = jpegdec.MjpegFrameProvider(str(path), device_decode=False)
    assert (p.frame_count, p.width, p.height) == (3, W, H)
    np.testing.assert_array_equal(p.read("rgb"), pillow_decode(files[0]))
    assert p._data is not None
    q = pickle.loads(pickle.dumps(p))
    assert q._data is None and q.pos == 1 and q.fallbacks == 1
    np.testing.assert_array_equal(q.read("rgb"), pillow_decode(files[1]))
    for provider in (p, q):
        provider.release()
        assert provider._data is None
    np.testing.assert_array_equal(p.read("rgb"), pillow_decode(files[1]))        # a released provider maps the file again
    p.release()


# ---- where the two differ --------------------------------------------------------------------------------------------------
def test_mjpeg_a_first_frame_the_device_does_not_take_gives_its_size_by_pillow():
    progressive = _file("jpeg", 0, progressive=True)
    with pytest.raises(jpegdec.JpegRejected):
        jpegdec.probe(progressive)
    p = jpegdec.MjpegFrameProvider([progressive])
    assert (p.width, p.height) == (W, H)


def test_png_a_malformed_first_frame_is_rejected_as_frame_0():
    with pytest.raises(pngdec.PngRejected) as err:
        pngdec.PngSequenceFrameProvider([_file("png", 0)[:40]])
    assert err.value.frame == 0 and err.value.reason == pngdec.reject_name(2)


def test_mjpeg_without_device_decode_no_header_is_looked_at(monkeypatch):
    files = [_file("jpeg", 0), _file("jpeg", 1, progressive=True)]
    p = jpegdec.MjpegFrameProvider(files, device_decode=False)

    def no_probe(data):
        raise AssertionError("probed")
    monkeypatch.setattr(jpegdec, "probe", no_probe)
    for data in files:
        np.testing.assert_array_equal(p.read("rgb"), pillow_decode(data))
    assert p.fallbacks == 2 and p._decoder is None


def test_png_without_device_decode_a_malformed_frame_still_raises_with_its_number():
    files = [_file("png", 0), _file("png", 1)[:-20], _file("png", 2)]
    p = pngdec.PngSequenceFrameProvider(files, device_decode=False)
    np.testing.assert_array_equal(p.read("rgb"), pillow_decode(files[0]))
    with pytest.raises(pngdec.PngRejected) as err:
        p.read()
    assert err.value.frame == 1 and p.pos == 1 and p.fallbacks == 1              # Pillow never saw it
    assert p.decode_frame(2, "rgb") is not None and p.fallbacks == 2


def test_mjpeg_a_frame_the_device_does_not_take_goes_to_pillow_and_is_counted(fake_decoder):
    files = [_file("jpeg", 0, progressive=True), _file("jpeg", 1, progressive=True)]
    p = jpegdec.MjpegFrameProvider(files, require_restart=False)
    for data in files:
        np.testing.assert_array_equal(p.read("rgb"), pillow_decode(data))
    assert p.fallbacks == 2 and fake_decoder.made == []


def test_png_a_frame_of_another_kind_goes_to_pillow_and_is_counted(fake_decoder):
    files = [_file("png", 0), _file("png", 1)]
    assert not pngdec.probe(files[0]).indexed
    p = pngdec.PngSequenceFrameProvider(files)
    for data in files:
        np.testing.assert_array_equal(p.read("rgb"), pillow_decode(data))
    assert p.fallbacks == 2 and fake_decoder.made == []


def test_mjpeg_require_restart_keeps_a_frame_without_restart_intervals_on_the_host(fake_decoder):
    data = _file("jpeg", 0)
    assert jpegdec.probe(data).restart_mcus == 0
    p = jpegdec.MjpegFrameProvider([data, data])
    np.testing.assert_array_equal(p.read("rgb"), pillow_decode(data))
    assert p.fallbacks == 1 and fake_decoder.made == []
    p.require_restart = False
    decoder, order, size = p.read()
    assert decoder is fake_decoder.made[0] and order == "bgr" and size == (W, H) and p.fallbacks == 1


@pytest.mark.parametrize("kind", KINDS)
def test_a_larger_frame_closes_the_decoder_at_once_and_carries_its_count(kind, fake_decoder):
    if kind == "jpeg":
        out = io.BytesIO()
        PIL.Image.new("RGB", (64, 16)).save(out, "JPEG")
        files, sizes = [_file("jpeg", 0), out.getvalue(), _file("jpeg", 1)], [(W, H), (64, 16), (W, H)]
        p = jpegdec.MjpegFrameProvider(files, require_restart=False)
    else:
        from tests import pngdec_cases as K
        names = ("zlib.40x24_random_b5", "zlib.300x40_smear_b7", "zlib.40x24_none_b5")
        files, sizes = [K.valid()[name][0] for name in names], [(40, 24), (300, 40), (40, 24)]
        p = pngdec.PngSequenceFrameProvider(files)
    first = p.read()
    assert first[0] is fake_decoder.made[0] and first[2] == sizes[0]
    assert (first[0].max_width, first[0].max_height) == sizes[0]
    first[0].fallbacks = 4
    second = p.read()
    assert first[0].closed and second[0] is fake_decoder.made[1] and second[2] == sizes[1]
    room = (max(sizes[0][0], sizes[1][0]), max(sizes[0][1], sizes[1][1]))
    assert (second[0].max_width, second[0].max_height) == room                   # never smaller than the one before
    assert p.fallbacks == 4
    assert p.read()[0] is second[0] and len(fake_decoder.made) == 2              # a smaller frame keeps the handle
