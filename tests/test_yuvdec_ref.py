"""DESIGN.md section 22 on the CPU: the rule and its table, the bound against the real equations, the round trip through
section 21, the linear filter against libjpeg's formulas and its named wrong forms, host_convert_back against the
restatement on every GPU case, the Y4M reader, the providers and the drop-in's routing.  No GPU."""
import pickle
from fractions import Fraction

import numpy as np
import pytest

from tests import jpegdec_ref, yuv_cases, yuv_ref, yuvdec_cases as K, yuvdec_ref as D
from transflow_amd import yuvdec


# ---- the rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,rng", D.PAIRS)
def test_the_table_is_the_rule_in_fractions_and_the_librarys(matrix, rng):
    coef, offset = D.rule(matrix, rng)
    assert coef == D.TABLE[(matrix, rng)]
    assert offset == (16 if rng == "tv" else 0)
    assert tuple(int(v) for v in yuvdec.coefficients(matrix, rng)) == coef
    for value, real in zip(coef, D.real_inverse(matrix, rng)):
        assert abs(Fraction(value) - real * 65536) <= Fraction(1, 2)


def test_bad_names_are_refused_by_the_library_and_by_python():
    import ctypes as C

    from transflow_amd import _lib
    out = (C.c_int32 * 5)()
    lib = _lib.load()
    for matrix, rng in ((2, 0), (0, 2), (-1, 0)):
        assert lib.tf_yuvdec_coefficients(matrix, rng, out) == _lib.TF_ERR_ARG
    assert lib.tf_yuvdec_coefficients(0, 0, None) == _lib.TF_ERR_ARG
    data = K.noise(4, 2, "yuv420p", 1)
    for kw in (dict(layout="yuv411p"), dict(matrix="bt2020"), dict(range="jpeg"), dict(chroma="cubic"), dict(order="gbr")):
        with pytest.raises(ValueError):
            yuvdec.host_convert_back(data, 4, 2, **{"layout": "yuv420p", **kw})
    with pytest.raises(ValueError):
        yuvdec.host_convert_back(data[:-1], 4, 2, "yuv420p")


@pytest.mark.parametrize("matrix,rng", D.PAIRS)
def test_greys_are_grey_and_pc_greys_the_identity(matrix, rng):
    levels = np.arange(256, dtype=np.uint8)
    grey = D.pixels(levels, np.full(256, 128, np.uint8), np.full(256, 128, np.uint8), matrix, rng)
    assert (grey[:, 0] == grey[:, 1]).all() and (grey[:, 1] == grey[:, 2]).all()
    if rng == "pc":
        np.testing.assert_array_equal(grey[:, 0], levels)
    else:
        assert grey[16, 0] == 0 and grey[235, 0] == 255 and (grey[:16] == 0).all() and (grey[235:] == 255).all()


def _cube_slices():
    uv = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.uint8)
    for luma in range(256):
        yield np.concatenate([np.full((65536, 1), luma, np.uint8), uv], axis=1)


def _worst(triples: np.ndarray, matrix: str, rng: str) -> float:
    got = D.pixels(triples[:, 0], triples[:, 1], triples[:, 2], matrix, rng)
    return float(np.abs(got - D.model(triples, matrix, rng)).max())


def test_every_output_is_within_0_51_of_the_real_equations():
    """One rounding costs 0.5, the coefficients' errors at most 495 * 2^-17 (|y| <= 239, |u|, |v| <= 128, each
    coefficient off by at most 2^-17): 0.504.  The whole cube for bt601 / tv, two million seeded triples for the others."""
    worst = max(_worst(triples, "bt601", "tv") for triples in _cube_slices())
    print(f"bt601 tv, the cube: {worst:.4f}")
    assert worst <= 0.51
    for k, (matrix, rng) in enumerate(yuv_cases.OTHER_PAIRS):
        triples = np.random.default_rng(40 + k).integers(0, 256, (2_000_000, 3), dtype=np.uint8)
        worst = _worst(triples, matrix, rng)
        print(f"{matrix} {rng}: {worst:.4f}")
        assert worst <= 0.51


@pytest.mark.parametrize("matrix,rng,bound", [("bt601", "tv", (1, 1, 2)), ("bt709", "tv", (2, 1, 2)), ("bt601", "pc", (1, 1, 1)),
                                               ("bt709", "pc", (1, 1, 1))])
def test_the_round_trip_through_section_21(matrix, rng, bound):
    """RGB -> yuv444p -> back: the forward bound of 0.51 a sample pushed through the linear inverse, and the inverse's own
    0.51."""
    cy, rv, gu, gv, bu = D.rule(matrix, rng)[0]
    derived = tuple(int((total * 0.51) / 65536 + 0.51) for total in (abs(cy) + abs(rv), abs(cy) + abs(gu) + abs(gv), abs(cy) + abs(bu)))
    assert derived == bound
    rgb = np.random.default_rng(8).integers(0, 256, (1000, 2000, 3), dtype=np.uint8)
    y, u, v = yuv_ref.planes(rgb, "yuv444p", matrix, rng)
    back = D.pixels(y, u, v, matrix, rng)
    worst = np.abs(back.astype(np.int64) - rgb).reshape(-1, 3).max(axis=0)
    print(f"{matrix} {rng}: {tuple(int(v) for v in worst)}")
    assert (worst <= np.array(bound)).all(), worst


# ---- the chroma filters ---------------------------------------------------------------------------------------------------
def test_the_clamped_linear_filter_is_libjpegs_at_every_small_size():
    rng = np.random.default_rng(3)
    for w in range(1, 10):
        for h in range(1, 6):
            dw, dh = (w + 1) // 2, (h + 1) // 2
            p = rng.integers(0, 256, (dh, dw)).astype(np.int64)
            got = D.expand(p, w, h, "yuv420p", "linear")
            np.testing.assert_array_equal(got, jpegdec_ref._h2v2(p, dw, dh, w, h), err_msg=f"{w}x{h}")
            assert got.min() >= 0 and got.max() <= 255
            p = rng.integers(0, 256, (h, dw)).astype(np.int64)
            got = D.expand(p, w, h, "yuv422p", "linear")
            np.testing.assert_array_equal(got, jpegdec_ref._h2v1(p, dw, w), err_msg=f"{w}x{h}")
            assert got.min() >= 0 and got.max() <= 255


def test_the_modes_are_one_at_444_and_replication_inverts_the_block():
    data = K.noise(7, 5, "yuv444p", 2)
    np.testing.assert_array_equal(D.convert_back(data, 7, 5, "yuv444p", chroma="linear"), D.convert_back(data, 7, 5, "yuv444p"))
    _, u, _ = D.unpack(K.noise(7, 5, "yuv420p", 2), 7, 5, "yuv420p")
    full = D.expand(u, 7, 5, "yuv420p", "replicate")
    for y in range(5):
        for x in range(7):
            assert full[y, x] == u[y >> 1, x >> 1]
    assert (D.expand(np.full((3, 4), 77), 7, 5, "yuv420p", "linear") == 77).all()        # a flat plane stays flat


def test_the_filter_cases_tell_the_filter_from_every_wrong_form():
    cases = list(K.filter_cases())
    assert {c[4] for c in cases} == {"yuv422p", "yuv420p", "nv12"}
    for case in cases:
        name, data, w, h, layout = case[:5]
        right = K.want(case)
        for wrong in K.wrong_forms(layout):
            other = D.convert_back(data, w, h, layout, chroma="linear", wrong=wrong)
            assert (other != right).any(), f"{name}: {wrong} gives the same pixels"
    assert "wrong_side" in K.wrong_forms("nv12") and "wrong_side" not in K.wrong_forms("yuv422p")


# ---- host_convert_back ----------------------------------------------------------------------------------------------------
def test_host_convert_back_is_the_restatement_on_every_gpu_case():
    n = 0
    for case in K.all_cases():
        name, data, w, h, layout, matrix, rng, chroma, order = case
        got = yuvdec.host_convert_back(data, w, h, layout, matrix, rng, chroma, order)
        assert got.dtype == np.uint8 and got.shape == (h, w, 3)
        np.testing.assert_array_equal(got, K.want(case), err_msg=name)
        n += 1
    assert n > 900
    assert len(K.SIZES) == len(yuv_cases.WIDTHS) * len(yuv_cases.HEIGHTS) + 6


def test_the_extremes_reach_both_clamps_and_the_boundaries_are_near():
    near = D.boundary_triples()
    assert near.shape == (144, 3)
    (cy, rv, gu, gv, bu), yo = D.rule("bt601", "tv")
    t = near.astype(np.int64) - (yo, 128, 128)
    accs = (cy * t[:, 0] + rv * t[:, 2], cy * t[:, 0] + gu * t[:, 1] + gv * t[:, 2], cy * t[:, 0] + bu * t[:, 1])
    for i, acc in enumerate(accs):
        low = (acc[48 * i:48 * i + 48] + 32768) & 0xFFFF
        assert (low[:24] < 64).all() and (low[24:] > 65535 - 64).all(), i
    case = next(c for c in K.extreme_cases() if c[0] == "levels-yuv444p-replicate-bt601-tv")
    out = K.want(case)
    assert (out == 0).any() and (out == 255).any()


# ---- Y4M ------------------------------------------------------------------------------------------------------------------
W, H, FRAMES = 6, 4, 3


def _frames(layout="yuv420p", n=FRAMES):
    return [K.noise(W, H, layout, 50 + k).tobytes() for k in range(n)]


def _reason(data) -> str:
    with pytest.raises(D.Rejected) as ref:
        D.parse_y4m(data)
    with pytest.raises(yuvdec.YuvRejected) as got:
        yuvdec.Y4mFrameProvider(data, device_decode=False)
    assert got.value.reason == ref.value.reason
    return got.value.reason


def test_the_reject_reasons_are_one_list():
    assert tuple(yuvdec.REJECT_REASONS) == tuple(D.REJECT)
    assert yuvdec.Y4M_TAGS == D.TAGS


@pytest.mark.parametrize("tag,layout", [(None, "yuv420p")] + sorted(D.TAGS.items()))
def test_every_accepted_tag(tag, layout):
    frames = _frames(layout)
    data = D.build_y4m(frames, W, H, tag=tag, rate="30000:1001", full=True)
    info = yuvdec.probe_y4m(data)
    ref = D.parse_y4m(data)
    assert (info.width, info.height, info.framerate, info.layout, info.range, info.siting, info.header_bytes) == \
        (W, H, Fraction(30000, 1001), layout, "pc", tag, ref["header_bytes"])
    assert (ref["layout"], ref["range"], ref["siting"], ref["framerate"]) == (layout, "pc", tag, Fraction(30000, 1001))
    offsets, trailing = yuvdec.index_y4m(data, info)
    assert offsets == ref["offsets"] and len(offsets) == FRAMES and trailing == ref["trailing_bytes"] == 0
    for at, frame in zip(offsets, frames):
        assert data[at:at + len(frame)] == frame
    assert yuvdec.probe_y4m(D.build_y4m(frames, W, H, tag=tag, full=False)).range == "tv"
    assert yuvdec.probe_y4m(D.build_y4m(frames, W, H, tag=tag, interlace="?")).range == "tv"
    assert yuvdec.probe_y4m(D.build_y4m(frames, W, H, tag=tag, interlace=None)).layout == layout


def test_every_reject_reason_from_a_hand_built_header():
    frames = _frames()
    good = D.build_y4m(frames, W, H)
    seen = set()
    for data, reason in [
        (b"RIFF" + good, "not_y4m"), (b"", "not_y4m"), (b"YUV4MPEG1 W6 H4 F25:1\n", "not_y4m"), (b"YUV4MPEG2W6 H4 F25:1\n", "not_y4m"),
        (b"YUV4MPEG2 H4 F25:1 Ip\n" + frames[0], "bad_header"), (b"YUV4MPEG2 W6 F25:1\n", "bad_header"),
        (b"YUV4MPEG2 W6 H4 Ip\n", "bad_header"), (b"YUV4MPEG2 Wsix H4 F25:1\n", "bad_header"),
        (b"YUV4MPEG2 W6 H4 F25\n", "bad_header"), (b"YUV4MPEG2 W6 H4 F25:x\n", "bad_header"),
        (b"YUV4MPEG2 W6 H4 F25:0\n", "bad_header"), (b"YUV4MPEG2 W0 H4 F25:1\n", "bad_header"),
        (b"YUV4MPEG2 W6 H4 F25:1 X" + b"a" * 300 + b"\n", "bad_header"), (b"YUV4MPEG2 W6 H4 F25:1", "bad_header"),
        (D.build_y4m(frames, W, H, interlace="t"), "interlaced"), (D.build_y4m(frames, W, H, interlace="b"), "interlaced"),
        (D.build_y4m(frames, W, H, interlace="m"), "interlaced"),
        (D.build_y4m(frames, W, H, tag="Cmono"), "chroma"), (D.build_y4m(frames, W, H, tag="C411"), "chroma"),
        (D.build_y4m(frames, W, H, tag="C444alpha"), "chroma"), (D.build_y4m(frames, W, H, tag="C420p10"), "chroma"),
        (D.build_y4m(frames, W, H, tag="C422p10"), "chroma"),
        (good.replace(b"FRAME\n", b"FRAMF\n", 1), "bad_frame_header"), (good.replace(b"FRAME\n", b"FRAMES\n", 1), "bad_frame_header"),
        (D.build_y4m(frames, W, H, frame_params="X" + "a" * 90), "bad_frame_header"),
        (good[:-len(frames[-1]) - 6] + b"frame\n" + frames[-1], "bad_frame_header"),
    ]:
        assert _reason(data) == reason, data[:60]
        seen.add(reason)
    assert seen == set(D.REJECT)


def test_frame_parameters_and_a_trailing_partial_frame():
    frames = _frames()
    data = D.build_y4m(frames, W, H, frame_params="Ip XSOMETHING=1")
    p = yuvdec.Y4mFrameProvider(data, device_decode=False)
    assert (p.frame_count, p.trailing_bytes) == (FRAMES, 0)
    assert [p._get(k).tobytes() for k in range(FRAMES)] == frames
    for cut in (1, 10, len(frames[-1]) - 1, len(frames[-1]) + 3):
        short = yuvdec.Y4mFrameProvider(data[:-cut], device_decode=False)
        ref = D.parse_y4m(data[:-cut])
        assert short.frame_count == FRAMES - 1 == len(ref["offsets"])
        assert short.trailing_bytes == ref["trailing_bytes"] > 0
    with pytest.raises(ValueError):
        yuvdec.Y4mFrameProvider(D.build_y4m([], W, H), device_decode=False)
    with pytest.raises(ValueError):
        yuvdec.Y4mFrameProvider(D.build_y4m(frames[:1], W, H)[:-1], device_decode=False)      # one partial frame: none


@pytest.mark.parametrize("layout", ["yuv420p", "yuv422p", "yuv444p"])
def test_a_file_of_the_y4m_outputs_parses_back_to_its_planes(layout, tmp_path):
    from transflow_amd.output import HipY4mOutput
    from transflow_amd.yuv import host_convert
    rgbs = [yuv_cases.noise(5, 7, 60 + k) for k in range(3)]
    path = str(tmp_path / "clip.y4m")
    with HipY4mOutput(path, 7, 5, 30000 / 1001, layout, "bt709", "pc", replace=True) as out:
        for rgb in rgbs:
            out.feed(host_convert(rgb, layout, "bt709", "pc"))
    p = yuvdec.Y4mFrameProvider(path, matrix="bt709", device_decode=False)
    assert (p.width, p.height, p.frame_count, p.layout, p.range, p.trailing_bytes) == (7, 5, 3, layout, "pc", 0)
    assert p.framerate == pytest.approx(30000 / 1001) and p.siting == {"yuv420p": "C420jpeg", "yuv422p": "C422", "yuv444p": "C444"}[layout]
    for k, rgb in enumerate(rgbs):
        assert p._get(k).tobytes() == yuv_ref.convert(rgb, layout, "bt709", "pc")
        np.testing.assert_array_equal(p.read("rgb"), D.convert_back(yuv_ref.convert(rgb, layout, "bt709", "pc"), 7, 5, layout, "bt709", "pc"))
    assert p.read() is None
    p.release()


def test_provider_positions_seek_start_and_the_pickle(tmp_path):
    frames = _frames("yuv422p", 4)
    path = tmp_path / "clip.y4m"
    path.write_bytes(D.build_y4m(frames, W, H, tag="C422", rate="24:1"))
    want = [D.convert_back(f, W, H, "yuv422p", "bt709", "tv", "linear", "bgr") for f in frames]
    p = yuvdec.Y4mFrameProvider(str(path), matrix="bt709", chroma="linear", device_decode=False)
    assert (p.width, p.height, p.framerate, p.frame_count, p.pos) == (W, H, 24.0, 4, 0)
    np.testing.assert_array_equal(p.read(), want[0])
    np.testing.assert_array_equal(p.read("rgb"), want[1][:, :, ::-1])
    assert p.pos == 2
    q = pickle.loads(pickle.dumps(p))                       # the mapping stays behind
    assert "_data" not in p.__getstate__() and q._decoder is None and q.pos == 2
    np.testing.assert_array_equal(q.read(), want[2])
    np.testing.assert_array_equal(q.read(), want[3])
    assert q.read() is None and q.pos == 4
    q.seek_start()
    np.testing.assert_array_equal(q.read(), want[0])
    q.release(), p.release()
    assert yuvdec.Y4mFrameProvider(str(path), size=(12, 8), range="pc", device_decode=False).range == "pc"
    sized = yuvdec.Y4mFrameProvider(str(path), size=(12, 8), device_decode=False)
    assert (sized.width, sized.height, sized.range) == (12, 8, "tv")
    for bad in (dict(matrix="bt2020"), dict(range="jpeg"), dict(chroma="cubic")):
        with pytest.raises(ValueError):
            yuvdec.Y4mFrameProvider(str(path), device_decode=False, **bad)


@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_raw_yuv_files(layout, tmp_path):
    frames = [K.noise(7, 5, layout, 70 + k).tobytes() for k in range(3)]
    path = tmp_path / "clip.yuv"
    path.write_bytes(b"".join(frames) + b"\x01\x02\x03")
    p = yuvdec.RawYuvFrameProvider(str(path), 7, 5, layout, framerate=50, matrix="bt709", range="pc", device_decode=False)
    assert (p.width, p.height, p.framerate, p.frame_count, p.trailing_bytes) == (7, 5, 50.0, 3, 3)
    for frame in frames:
        np.testing.assert_array_equal(p.read(), D.convert_back(frame, 7, 5, layout, "bt709", "pc", order="bgr"))
    assert p.read() is None
    again = pickle.loads(pickle.dumps(p))
    again.seek_start()
    np.testing.assert_array_equal(again.read("rgb"), D.convert_back(frames[0], 7, 5, layout, "bt709", "pc"))
    with pytest.raises(ValueError):
        yuvdec.RawYuvFrameProvider(str(path), 700, 500, layout, device_decode=False)


# ---- routing (no GPU call: a provider's constructor walks headers only) ------------------------------------------------------
def test_dropin_routes_y4m_files_only_on_request(tmp_path):
    from transflow_amd import dropin
    from transflow_amd.flow import HipFlowSource
    from transflow_amd.pixmap import HipPixmapSource, HipY4mPixmapSource
    path = str(tmp_path / "clip.y4m")
    with open(path, "wb") as f:
        f.write(D.build_y4m(_frames(), W, H, full=True))
    assert yuvdec.is_y4m(path)
    for other in (str(tmp_path / "missing.y4m"), "clip.mp4", str(tmp_path), 3):
        assert not yuvdec.is_y4m(other)

    def flow_holder(**options):
        class Ref:
            from_args = dropin._flow_from_args(lambda *a, **k: "the reference's", **options)
        return Ref

    builder = flow_holder(yuv_inputs=True, yuv_input_matrix="bt709").from_args(path)
    provider = builder.provider_arg
    assert isinstance(builder, HipFlowSource.Builder) and isinstance(provider, yuvdec.Y4mFrameProvider)
    assert (provider.width, provider.height, provider.frame_count) == (W, H, FRAMES)
    assert (provider.matrix, provider.range, provider.chroma, provider.siting) == ("bt709", "pc", "replicate", "C420jpeg")
    assert flow_holder(yuv_inputs="linear").from_args(path, size=(12, 8)).provider_arg.chroma == "linear"
    assert flow_holder(yuv_inputs="linear").from_args(path, size=(12, 8)).provider_arg.width == 12
    assert flow_holder().from_args(path).provider_arg == path                         # without it: a path for cv2, as before
    assert flow_holder(mjpeg_inputs=True, png_inputs=True).from_args(path).provider_arg == path
    assert flow_holder(yuv_inputs=True).from_args("clip.mp4").provider_arg == "clip.mp4"
    assert flow_holder(yuv_inputs=True).from_args(path, use_mvs=True) == "the reference's"   # motion vectors are not this file's

    def pixmap_holder(**options):
        class Ref:
            from_args = dropin._pixmap_from_args(lambda *a, **k: "the reference's", **options)
        return Ref

    routed = pixmap_holder(stills=False, yuv_inputs="linear", yuv_input_matrix="bt709").from_args(path, (W, H), seek=1, repeat=2)
    assert isinstance(routed, HipY4mPixmapSource)
    assert (routed.seek, routed.repeat, routed.matrix, routed.chroma, routed.range) == (1, 2, "bt709", "linear", None)
    assert pixmap_holder(stills=False, yuv_inputs=True).from_args(path, (W, H)).chroma == "replicate"
    assert pixmap_holder(stills=False).from_args(path, (W, H)) == "the reference's"
    assert pixmap_holder(stills=False, mjpeg_inputs=True, png_inputs=True).from_args(path, (W, H)) == "the reference's"
    assert pixmap_holder(stills=False, yuv_inputs=True).from_args("clip.mp4", (W, H)) == "the reference's"
    with pytest.raises(NotImplementedError):                                          # the class's own factory: opt-in too
        HipPixmapSource.from_args(path, (W, H))
    assert isinstance(HipPixmapSource.from_args(path, (W, H), y4m_inputs=True), HipY4mPixmapSource)


@pytest.mark.parametrize("options", [dict(yuv_inputs="cubic"), dict(yuv_inputs="replicate"), dict(yuv_inputs=1), dict(yuv_inputs=None),
                                     dict(yuv_inputs=True, yuv_input_matrix="bt2020"), dict(yuv_input_matrix=None)])
def test_dropin_refuses_other_values(options):
    from transflow_amd import dropin
    with pytest.raises(ValueError):
        dropin.install(**options)
