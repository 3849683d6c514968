"""The device JPEG decoder's pixel stages (transflow_amd/csrc/jpegdec.hip) -- coefficients to planes
through the IDCT, chroma upsampling, YCbCr to RGB / BGR, k_jd_colour's four-pixels-a-lane store -- at the sizes where they
can go wrong: frames of 1 to 4 pixels' width, where libjpeg replicates the chroma instead of filtering it, the first
filtered width, either side of the 8- and 16-pixel MCU edges, one to three rows, pixel counts that are no multiple of 4;
grey, 4:4:4, 4:2:2 and 4:2:0, through the serial kernel (with and without a restart interval) and the parallel scan.
The expected pixels are Pillow's, kept in tests/golden/jpegdec_geometry.npz (tests/jpegdec_cases.geometry_cases) and, for
the hand-built colour lattice, MCU-order and IDCT-basis files of tests/jpegdec_sweep.py, in jpegdec_sweep_pixels.npz;
tests/test_jpegdec_ref.py and tests/test_jpegdec_sweep_ref.py hold the restatement equal to them on the CPU.  Every decode
through the C ABI writes into a buffer filled with 0xA5 whose bytes in front of and behind the output are checked."""
import os

import numpy as np
import pytest

from tests import jpegdec_cases as JC
from tests import jpegdec_par_ref as PR
from tests import jpegdec_ref as JR
from tests import jpegdec_sweep as SW
from tests.test_gpu_jpegdec import Handle
from tests.test_gpu_jpegdec_par import ParHandle, sizes  # noqa: F401  (sizes: the fixture that forces the parallel path's sizes)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GEO = np.load(os.path.join(GOLDEN, "jpegdec_geometry.npz"))
BUILT = np.load(os.path.join(GOLDEN, "jpegdec_sweep_pixels.npz"))
LAYOUTS = list(JC.GEOMETRY_LAYOUTS)
# scan: (the files have a restart interval of 1 MCU, the handle's scan mode, the parallel path's forced subsequence size)
SCANS = {"dri1_serial": (True, 0, 0), "nodri_one_wave": (False, 0, 0), "nodri_parallel": (False, 1, 0), "nodri_parallel_sub16": (False, 1, 16)}
SIDE = 64
DEFAULT_SUB = 64                                                        # the parallel path's subsequence size when none is forced


def _case(layout, w, h, dri, z=GEO):
    name = JC.geometry_name(layout, w, h, dri)
    return name, z[name + ".file"].tobytes(), z[name + ".rgb"]


def _exact(handle, name, data, rgb, order=0, shift=0, what=""):
    rc, reject, got = handle.decode(data, rgb.shape, order, shift)
    assert rc == handle.ok, name
    assert reject == 0, f"{name}: rejected as {JR.REJECT[reject] if reject < len(JR.REJECT) else reject}"
    np.testing.assert_array_equal(got, rgb[:, :, ::-1] if order else rgb, err_msg=f"{name} order {order} shift {shift} {what}")


@pytest.fixture(scope="module")
def handles():
    """One guarded handle per scan mode, for frames up to 64 x 64."""
    made = {mode: ParHandle(mode=mode, max_w=SIDE, max_h=SIDE, max_file=1 << 16) for mode in (0, 1)}
    yield made
    for h in made.values():
        h.close()


def test_the_fixture_is_the_corpus():
    names = [str(n) for n in GEO["names"]]
    assert names == [JC.geometry_name(layout, w, h, dri) for dri in (False, True) for layout in LAYOUTS for w, h in JC.geometry_sizes(dri)]
    assert len(names) == 4 * (11 * 7 + 2 + 7 * 4)
    assert [str(n) for n in BUILT["names"]] == [name for name, _ in SW.pixel_cases()]


@pytest.mark.parametrize("scan", list(SCANS))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_size_decodes_to_libjpegs_pixels(handles, sizes, layout, scan):
    """reject == 0 and the fixture's pixels, in RGB and in BGR, the guards intact.  The files without DRI take the
    parallel path on the handle in scan mode 1 (one subsequence at the default size, up to a hundred at 16 bytes) and the
    one wave of the serial kernel in mode 0, which is what JpegDecoder does with them by default."""
    dri, mode, sub = SCANS[scan]
    if sub:
        sizes(sub)
    handle = handles[mode]
    before = handle.stats()
    for w, h in JC.geometry_sizes(dri):
        name, data, rgb = _case(layout, w, h, dri)
        _exact(handle, name, data, rgb)
        _exact(handle, name, data, rgb, order=1)
        if mode == 1 and not dri:
            assert handle.stats()[0] == PR.ParScan(data, sub or DEFAULT_SUB).n_subs, name      # it took the parallel path
    if mode == 0 or dri:
        assert handle.stats() == before                                 # the parallel path was not taken


@pytest.mark.parametrize("dri", (False, True), ids=("nodri_parallel", "dri1_serial"))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_an_output_that_is_not_dword_aligned(handles, layout, dri):
    """Shifts of 1, 2 and 3 bytes for every frame of at most 16 pixels or of a pixel count that is no multiple of 4: the
    byte stores of every lane, and of the last lane's one to three pixels.  1 x 1 is three bytes between the guards."""
    chosen = [(w, h) for w, h in JC.geometry_sizes(dri) if w * h <= 16 or (w * h) % 4]
    assert (1, 1) in chosen and len(chosen) >= 15 and {(w * h) % 4 for w, h in chosen} == {0, 1, 2, 3}
    for w, h in chosen:
        name, data, rgb = _case(layout, w, h, dri)
        for shift in (1, 2, 3):
            _exact(handles[1], name, data, rgb, order=shift & 1, shift=shift)


OTHER_LAYOUT = {"grey": 0, "444": 1, "422": 2, "420": 0}                 # JpegEncoder's subsampling of the frame decoded in between


@pytest.fixture(scope="module")
def big_frames():
    """{subsampling: (file, the restatement's pixels)}: 64 x 64 noise at quality 95 from the device encoder."""
    from transflow_amd.jpeg import JpegEncoder
    image = np.random.default_rng(64).integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8)
    out = {}
    for sub in (0, 1, 2):
        enc = JpegEncoder(SIDE, SIDE, 95, subsampling=sub)
        try:
            data = enc.encode(image)
        finally:
            enc.close()
        out[sub] = (data, JR.decode(data))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
def test_small_frames_behind_a_large_one_of_another_layout(handles, big_frames, layout):
    """Stale planes: a 64 x 64 noise frame of another sampling fills the handle's planes before every frame up to 9 pixels
    wide, and the small frame is still the fixture's.  Up to W = 4 nothing but chroma column x >> 1 may be read (the old
    first-column rule read column 1, which at downsampled_width = 1 is the padded block's, and beyond it the frame before);
    from W = 5 the neighbour columns are the frame's own samples."""
    data_big, rgb_big = big_frames[OTHER_LAYOUT[layout]]
    handle = handles[1]
    _exact(handle, "the 64 x 64 frame", data_big, rgb_big)
    count = 0
    for dri in (False, True):
        for w, h in JC.geometry_sizes(dri):
            if w > 9:
                continue
            rc, reject, _ = handle.decode(data_big, rgb_big.shape)
            assert rc == handle.ok and reject == 0
            name, data, rgb = _case(layout, w, h, dri)
            _exact(handle, name, data, rgb, what="behind a 64 x 64 frame")
            count += 1
    assert count == 8 * 7 + 2 + 5 * 4


@pytest.mark.parametrize("layout", LAYOUTS)
def test_handles_of_exactly_the_frames_size(layout):
    """tf_jpegdec_create(w, h): the planes of whole MCUs of every sampling, the blocks and the intervals fit a handle made
    for just this frame, with a restart interval (where the corpus has the size with one) and without, in both scan modes."""
    for w, h in ((1, 1), (4, 4), (5, 3), (17, 9), (33, 17)):
        for mode in (0, 1):
            handle = ParHandle(mode=1, max_w=w, max_h=h, max_file=1 << 13) if mode else Handle(max_w=w, max_h=h, max_file=1 << 13)
            try:
                for dri in (False, True):
                    if (w, h) in JC.geometry_sizes(dri):
                        name, data, rgb = _case(layout, w, h, dri)
                        _exact(handle, name, data, rgb, order=mode, what=f"on a {w} x {h} handle")
            finally:
                handle.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_jpeg_decoder_class_on_frames_up_to_4_pixels_wide(layout):
    from transflow_amd.jpegdec import JpegDecoder
    for parallel in (False, True):
        dec = JpegDecoder(8, 8, parallel_scan=parallel)
        try:
            for w, h in ((4, 4), (3, 5)):
                name, data, rgb = _case(layout, w, h, False)
                for order in ("rgb", "bgr"):
                    pixels = dec.decode(data, order)
                    np.testing.assert_array_equal(np.asarray(pixels), rgb if order == "rgb" else rgb[:, :, ::-1], err_msg=name)
                    pixels.close()
                pixels = dec.decode_or_host(data)
                np.testing.assert_array_equal(np.asarray(pixels), rgb, err_msg=name)
                pixels.close()
            assert dec.fallbacks == 0
        finally:
            dec.close()


@pytest.mark.parametrize("sub", (0, 1, 2), ids=("444", "422", "420"))
def test_the_device_encoders_small_files_round_trip(sub):
    """JpegEncoder's own files of 1 x 1 to 5 x 3 through JpegDecoder: the pixels libjpeg decodes them to (Pillow's here,
    and the restatement's, which needs no libjpeg)."""
    from transflow_amd.framecodec import pillow_decode
    from transflow_amd.jpeg import JpegEncoder
    from transflow_amd.jpegdec import JpegDecoder, probe
    rng = np.random.default_rng(90 + sub)
    for w, h in ((1, 1), (2, 2), (3, 5), (4, 4), (5, 3)):
        image = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        enc = JpegEncoder(h, w, 95, subsampling=sub)
        dec = JpegDecoder(w, h)
        try:
            data = enc.encode(image)
            info = probe(data)
            assert (info.width, info.height, info.h_samp, info.v_samp) == (w, h, 2 - (sub == 0), 1 + (sub == 2))
            pixels = dec.decode(data)
            got = np.asarray(pixels).copy()
            pixels.close()
            np.testing.assert_array_equal(got, JR.decode(data), err_msg=f"{w} x {h}")
            np.testing.assert_array_equal(got, pillow_decode(data), err_msg=f"{w} x {h}")
            assert dec.fallbacks == 0
        finally:
            enc.close()
            dec.close()


# ---- hand-built files: colour, MCU order, the IDCT's basis ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    """Handles for the 352 x 176 lattice, one per scan mode."""
    made = {mode: ParHandle(mode=mode, max_w=352, max_h=176, max_file=1 << 16) for mode in (0, 1)}
    yield made
    for h in made.values():
        h.close()


def _built(name):
    data, rgb = BUILT[name + ".file"].tobytes(), BUILT[name + ".rgb"]
    assert data == dict(SW.pixel_cases())[name].data
    return data, rgb


@pytest.mark.parametrize("mode", (0, 1), ids=("serial", "parallel"))
def test_the_colour_lattice(wide, mode):
    """968 flat MCUs, one per (Y, Cb, Cr) of the lattice: Pillow's pixels and the restatement's, RGB and BGR.  A difference
    names the triple."""
    data, rgb = _built("g_lattice_444")
    np.testing.assert_array_equal(JR.decode(data), rgb)
    triples = SW.lattice()
    for order in (0, 1):
        rc, reject, got = wide[mode].decode(data, rgb.shape, order)
        assert rc == wide[mode].ok and reject == 0
        want = rgb[:, :, ::-1] if order else rgb
        if not np.array_equal(got, want):
            y, x = np.argwhere((got != want).any(axis=2))[0]
            m = (y // 8) * SW.LATTICE_SIZE[0] + x // 8
            raise AssertionError(f"order {order}: (Y, Cb, Cr) = {triples[m]} at ({x}, {y}) is {got[y, x].tolist()}, not {want[y, x].tolist()}")


@pytest.mark.parametrize("mode", (0, 1), ids=("serial", "parallel"))
def test_mcu_order_of_422_and_420(wide, mode):
    """Every luma block of an MCU another grey, chroma blocks 0 / 255 in a checkerboard, the picture ending 1 and 15 pixels
    into the last MCU: a swapped block order, a wrong plane stride or a wrong rounding term of the fancy filters shows."""
    names = [str(n) for n in BUILT["names"] if str(n)[0] == "h"]
    assert len(names) == 6
    for name in names:
        data, rgb = _built(name)
        np.testing.assert_array_equal(JR.decode(data), rgb, err_msg=name)
        for order in (0, 1):
            _exact(wide[mode], name, data, rgb, order=order)
        _exact(wide[mode], name, data, rgb, shift=3)


@pytest.mark.parametrize("mode", (0, 1), ids=("serial", "parallel"))
def test_the_idct_basis(wide, mode):
    """Each of the 64 coefficients alone, at +-1 and at +- the largest amplitude inside the range where libjpeg's IDCTs
    agree.  A difference names the coefficient."""
    data, rgb = _built("i_idct_basis")
    np.testing.assert_array_equal(JR.decode(data), rgb)
    rc, reject, got = wide[mode].decode(data, rgb.shape)
    assert rc == wide[mode].ok and reject == 0
    for i, (k, v) in enumerate(SW.basis_blocks()):
        by, bx = divmod(i, SW.BASIS_SIZE[0])
        a, b = (p[8 * by:8 * by + 8, 8 * bx:8 * bx + 8, 0] for p in (got, rgb))
        assert np.array_equal(a, b), f"zigzag position {k} (natural {int(JR.ZIGZAG[k])}), coefficient {v} x quantiser {SW.BASIS_QUANT[k]}:\n{a}\nnot\n{b}"
    np.testing.assert_array_equal(got, rgb)
