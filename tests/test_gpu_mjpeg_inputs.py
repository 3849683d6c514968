"""MJPEG inputs decoded on the device (transflow_amd/jpegdec.py, pixmap.py): an MjpegFrameProvider under a HipFlowSource
gives the flows of the same frames as decoded arrays, bit for bit; HipMjpegPixmapSource loops, seeks and repeats as the
reference's CvPixmapSource does and feeds a layer what host arrays feed it; and the routing is opt-in.  The clip and
Pillow's decode of every frame are tests/golden/jpegdec_stream.npz."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STREAM = np.load(os.path.join(GOLDEN, "jpegdec_stream.npz"))
FILES = [STREAM[f"{i}.file"].tobytes() for i in range(6)]
RGB = [STREAM[f"{i}.rgb"] for i in range(6)]
BGR = [np.ascontiguousarray(a[:, :, ::-1]) for a in RGB]
NODRI3 = STREAM["6.file"].tobytes()                  # frame 3 again, without a restart interval: the same pixels


def _flows(provider, **kw):
    from transflow_amd.flow import HipFlowSource
    with HipFlowSource.from_args(provider, direction="backward", **kw) as source:
        return [np.array(f, copy=True) for f in source]


def _array_provider():
    from transflow_amd.flow import ArrayFrameProvider
    return ArrayFrameProvider(BGR, 25.0)


def _same(got, want, n):
    assert len(got) == len(want) == n
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()


@pytest.fixture(scope="module")
def stream_path(tmp_path_factory):
    path = tmp_path_factory.mktemp("mjpeg") / "clip.mjpeg"
    path.write_bytes(b"".join(FILES))
    return str(path)


def test_provider_reads_the_stream(stream_path):
    from transflow_amd.jpegdec import MjpegFrameProvider
    from transflow_amd.pixmap import DevicePixmap
    p = MjpegFrameProvider(stream_path, framerate=30.0)
    assert (p.width, p.height, p.frame_count, p.framerate) == (64, 48, 6, 30.0)
    for want in BGR:
        frame = p.read()
        assert isinstance(frame, DevicePixmap) and frame._host is None
        np.testing.assert_array_equal(np.asarray(frame), want)
    assert p.read() is None and p.fallbacks == 0
    p.seek_start()
    np.testing.assert_array_equal(np.asarray(p.read()), BGR[0])
    p.release()


def test_farneback_flows_are_those_of_the_decoded_arrays(stream_path):
    from transflow_amd.config import FlowConfig
    from transflow_amd.jpegdec import MjpegFrameProvider
    want = _flows(_array_provider())
    assert any(np.abs(w).max() > 0.5 for w in want)                      # the clip moves
    provider = MjpegFrameProvider(stream_path)
    _same(_flows(provider), want, 5)
    assert provider.fallbacks == 0
    _same(_flows(MjpegFrameProvider(FILES), repeat=2), _flows(_array_provider(), repeat=2), 10)      # a rewind in between
    _same(_flows(MjpegFrameProvider(FILES), cv_config=FlowConfig(hip_batch=2)), want, 5)
    _same(_flows(MjpegFrameProvider(FILES), cv_config=FlowConfig(hip_prefetch=1)), want, 5)


def test_frames_reach_farneback_without_a_host_copy():
    from transflow_amd.flow import HipFlowSource
    from transflow_amd.jpegdec import MjpegFrameProvider
    seen = []

    class Watching(MjpegFrameProvider):
        def read(self, order="bgr"):
            frame = MjpegFrameProvider.read(self, order)
            if frame is not None:
                seen.append(frame)
            return frame

    with HipFlowSource.from_args(Watching(FILES), direction="backward") as source:
        assert len(list(source)) == 5
    assert len(seen) == 6 and all(f._host is None for f in seen)


def test_horn_schunck_takes_the_host_branch():
    from transflow_amd.config import HornSchunckConfig
    from transflow_amd.jpegdec import MjpegFrameProvider
    cfg = HornSchunckConfig(hs_iterations=5)
    _same(_flows(MjpegFrameProvider(FILES), cv_config=cfg), _flows(_array_provider(), cv_config=cfg), 5)


def test_a_frame_without_dri_goes_the_hosts_way():
    from transflow_amd.jpegdec import MjpegFrameProvider
    files = FILES[:3] + [NODRI3] + FILES[4:]
    provider = MjpegFrameProvider(files)
    _same(_flows(provider), _flows(_array_provider()), 5)
    assert provider.fallbacks == 1
    on_device = MjpegFrameProvider(files, require_restart=False)             # one wave decodes the whole frame
    _same(_flows(on_device), _flows(_array_provider()), 5)
    assert on_device.fallbacks == 0


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


def test_pixmap_source_loops_as_the_reference_does(stream_path, tmp_path):
    import PIL.Image

    from transflow_amd.pixmap import DevicePixmap, HipMjpegPixmapSource
    overlay = np.zeros((48, 64, 4), np.uint8)
    overlay[5:9, 10:20] = (200, 10, 30, 255)
    overlay[40, 3] = (1, 2, 3, 9)
    alteration = str(tmp_path / "overlay.png")
    PIL.Image.fromarray(overlay).save(alteration)
    want = []
    for frame in _reference_loop(RGB, 2, 2):
        a = frame.copy()
        a[5:9, 10:20] = (200, 10, 30)
        a[40, 3] = (1, 2, 3)
        want.append(a)
    with HipMjpegPixmapSource(stream_path, seek=2, alteration_path=alteration, repeat=2) as source:
        assert (source.width, source.height, source.framerate, source.length) == (64, 48, 25, 12)
        got = list(source)
    assert len(got) == len(want) == 8 and all(isinstance(g, DevicePixmap) for g in got)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(np.asarray(g), w)
    with HipMjpegPixmapSource(stream_path, seek_time=0.08) as source:        # 2 frames at 25 frames/s
        assert source.seek == 2 and source.length == 4
        got = list(source)
    assert len(got) == 4 and all(g._host is None for g in got)
    for g, w in zip(got, RGB[2:]):
        np.testing.assert_array_equal(np.asarray(g), w)


def test_a_layer_fed_device_frames_equals_one_fed_host_arrays(stream_path):
    from transflow_amd.pixmap import HipMjpegPixmapSource, HipPixmapInterface
    from transflow_amd.remap import CompImage, RemapLayer
    h, w = 48, 64
    rng = np.random.default_rng(3)
    from oracle import remap_ref as OR
    flows = [OR.post_process((rng.random((h, w, 2)) * 6 - 3).astype(np.float32), OR.BACKWARD) for _ in range(4)]   # clipped to the frame
    us = [rng.random((h, w)) for _ in range(4)]

    def run(frames):
        layer = RemapLayer(h, w, reset_mode="random", reset_random_factor=0.1)
        layer.set_sources([np.ones((h, w), np.uint8)])
        comp = CompImage(h, w, (255, 255, 255))
        out = []
        for flow, u, frame in zip(flows, us, frames):
            layer.update(flow, u)
            layer.gather(0, frame)
            comp.begin()
            layer.render(comp)
            out.append(comp.download().copy())
        return out, layer.get_state()[0].copy()

    with HipMjpegPixmapSource(stream_path) as source:
        itf = HipPixmapInterface(source, np.ones((h, w), bool))
        got, state = run(itf.next() for _ in range(4))
        assert itf.frame_number == 3
    want, want_state = run(RGB[:4])
    np.testing.assert_array_equal(state, want_state)
    for g, e in zip(got, want):
        np.testing.assert_array_equal(g, e)
    assert any((a != b).any() for a, b in zip(want, want[1:]))


def test_routing_is_by_extension_and_existence(stream_path, tmp_path):
    from transflow_amd.pixmap import HipMjpegPixmapSource, HipPixmapSource
    source = HipPixmapSource.from_args(stream_path, (64, 48), seek=1, repeat=3)
    assert isinstance(source, HipMjpegPixmapSource) and (source.seek, source.repeat) == (1, 3)
    for video in ("clip.mp4", "gradient2", str(tmp_path / "missing.png"), str(tmp_path / "missing.mjpeg")):
        with pytest.raises(NotImplementedError):
            HipPixmapSource.from_args(video, (8, 6))
