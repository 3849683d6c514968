"""tf_png's mode "frame" on the GPU (tf_png_set_code, transflow_amd/csrc/png.hip: k_png_count, k_png_table and the stored
path of k_png_deflate) against its restatement (tests/png_frame_code_ref.py): whole files byte for byte from host and
device inputs, the code and the bands' account, the way back to the fixed code, the files through the device's decoder,
and the compositor's option."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from tests import png_frame_code_ref as F
from tests import png_ref as P
from tests import pngdec_ref as D
from tests.test_gpu_png import H, W, _decode, _first_difference, _flows, _HostSource

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_wanted = {}


def _case(name):
    """(image, band_rows, the restatement's trace): made once and left as they are."""
    if name not in _wanted:
        image, band_rows = F.case(name)
        image.setflags(write=False)
        _wanted[name] = (image, band_rows, F.trace(image, band_rows))
    return _wanted[name]


@pytest.mark.parametrize("name", list(F.CASES))
def test_encoder_writes_the_restatements_file_code_and_bands(name):
    """From tf_png_encode (a host array) and tf_png_encode_dev (a DevicePixmap); tf_png_copy_last returns it again."""
    from transflow_amd import _lib
    from transflow_amd.pixmap import DevicePixmap
    from transflow_amd.png import PngEncoder
    image, band_rows, t = _case(name)
    enc = PngEncoder(image.shape[0], image.shape[1], band_rows or None, code="frame")
    pixmap = DevicePixmap.from_host(np.array(image))
    try:
        assert enc.band_rows == t.band_rows
        with pytest.raises(_lib.TfError):                                  # TF_ERR_STATE before an encode in this mode
            enc.last_code()
        with pytest.raises(_lib.TfError):
            enc.last_bands()
        got = enc.encode(image)
        assert got == t.data, _first_difference(got, t.data)
        np.testing.assert_array_equal(_decode(got), image)                 # whatever the restatement says
        assert enc.last_code() == (t.lengths, t.repairs)
        assert enc.last_bands() == (t.band_sizes, t.band_stored)
        from_device = enc.encode(pixmap)
        assert from_device == t.data, _first_difference(from_device, t.data)
        again = np.empty(len(t.data), np.uint8)
        n = C.c_size_t()
        _lib.check(enc._lib.tf_png_copy_last(enc._h, C.c_void_p(again.ctypes.data), again.nbytes, C.byref(n)))
        assert n.value == len(t.data) and again.tobytes() == t.data
    finally:
        enc.close()
        pixmap.close()


def test_golden_files_are_the_devices():
    from transflow_amd.png import PngEncoder
    fixtures = sorted(glob.glob(os.path.join(GOLDEN, "png_fc_*.npz")))
    assert len(fixtures) == len(F.GOLDEN_CASES)
    for path in fixtures:
        with np.load(path) as z:
            image, band_rows, _ = _case(str(z["name"]))
            enc = PngEncoder(image.shape[0], image.shape[1], band_rows or None, code="frame")
            try:
                assert enc.encode(image) == z["png"].tobytes(), str(z["name"])
            finally:
                enc.close()


@pytest.mark.parametrize("name", ["8x700_stripes_b1", "40x300_smear", "24x40_noise_b5"])
def test_a_handle_switched_to_the_fixed_code_and_back_writes_each_modes_bytes(name):
    from transflow_amd import _lib
    from transflow_amd.png import PngEncoder
    image, band_rows, t = _case(name)
    fixed = P.encode(image, band_rows)
    assert fixed != t.data
    enc = PngEncoder(image.shape[0], image.shape[1], band_rows or None, code="frame")
    try:
        assert enc.encode(image) == t.data
        enc.set_code("fixed")
        assert enc.last_code() == (t.lengths, t.repairs)                   # the last encode's, until the next
        got = enc.encode(image)
        assert got == fixed, _first_difference(got, fixed)
        with pytest.raises(_lib.TfError):                                  # that one had no code of its own
            enc.last_code()
        with pytest.raises(_lib.TfError):
            enc.last_bands()
        enc.set_code("frame")
        assert enc.encode(image) == t.data
        assert enc.last_bands() == (t.band_sizes, t.band_stored)
        with pytest.raises(ValueError):
            enc.set_code("best")
        with pytest.raises(ValueError):
            _lib.check(enc._lib.tf_png_set_code(enc._h, 2))
        assert enc.encode(image) == t.data                                 # a refused mode changes nothing
    finally:
        enc.close()
    with pytest.raises(ValueError):
        PngEncoder(8, 8, code="best")


def test_last_bands_reports_the_count_it_has_no_room_for():
    from transflow_amd import _lib
    from transflow_amd.png import PngEncoder
    image, band_rows, t = _case("8x700_stripes_b1")
    enc = PngEncoder(8, 700, band_rows, code="frame")
    try:
        enc.encode(image)
        sizes, stored, n = (C.c_uint32 * 8)(*([7] * 8)), (C.c_uint8 * 8)(*([7] * 8)), C.c_size_t()
        assert enc._lib.tf_png_last_bands(enc._h, sizes, stored, 7, C.byref(n)) == _lib.TF_ERR_ARG
        assert n.value == 8 and list(sizes) == [7] * 8 and list(stored) == [7] * 8
        assert enc._lib.tf_png_last_bands(enc._h, None, None, 0, C.byref(n)) == _lib.TF_ERR_ARG and n.value == 8
    finally:
        enc.close()


@pytest.mark.parametrize("name", list(F.CASES))
def test_indexed_files_come_back_through_the_devices_decoder(name):
    from transflow_amd.png import PngEncoder
    from transflow_amd.pngdec import PngDecoder, probe
    image, band_rows, t = _case(name)
    enc = PngEncoder(image.shape[0], image.shape[1], band_rows or None, index=True, code="frame")
    dec = PngDecoder(image.shape[1], image.shape[0])
    try:
        data = enc.encode(image)
        assert data == D.with_index(t.data, t.band_rows)
        info = probe(data)
        assert info.indexed and info.band_rows == t.band_rows
        np.testing.assert_array_equal(np.asarray(dec.decode(data, info=info)), image)
        assert dec.fallbacks == 0
    finally:
        enc.close()
        dec.close()


def _render(png_frames, png_code="fixed"):
    """tests/test_gpu_png.py's two-layer clip through a compositor with these options."""
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    rng = np.random.default_rng(1)
    comp = HipCompositor.from_args(H, W, [LayerConfig(i, classname=c) for i, c in enumerate(("moveref", "sum"))],
                                   background_color="#204060", png_frames=png_frames, png_code=png_code)
    masks = [np.ones((H, W), bool), np.zeros((H, W), bool)]
    masks[1][H // 3:, 5:W // 2] = True
    comp.set_sources({i: [_HostSource(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), masks[i])] for i in range(2)})
    out = []
    try:
        for flow in _flows(4, False):
            comp.update(flow)
            frame = comp.render()
            out.append(frame if png_frames else np.array(frame))
    finally:
        comp.close()
    return out


def test_compositor_returns_the_frame_coded_indexed_file_of_its_plain_render():
    from transflow_amd.png import PngFrame
    from transflow_amd.pngdec import PngDecoder
    plain = _render(False)
    files = _render("indexed", "frame")
    assert (plain[0] != plain[-1]).any()
    dec = PngDecoder(W, H)
    try:
        for t, (frame, raw) in enumerate(zip(files, plain)):
            assert isinstance(frame, PngFrame) and frame.shape == (H, W, 3)
            want = F.encode(raw, 0, index=True)
            assert frame.data == want, f"frame {t}: " + _first_difference(frame.data, want)
            assert len(frame.data) <= len(D.with_index(P.encode(raw), frame.band_rows))
            np.testing.assert_array_equal(np.asarray(dec.decode(frame.data)), raw, err_msg=f"frame {t}")
            np.testing.assert_array_equal(frame.decode(), raw, err_msg=f"frame {t}")
    finally:
        dec.close()
