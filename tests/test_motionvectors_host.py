"""Host side of the motion-vector flow source (transflow_amd/motionvectors.py): record conversion, the builder's
arithmetic, the PyAV provider against a stub `av` module (PyAV is not installed where this suite runs), and the routing
through HipFlowSource.from_args and the drop-in.  No GPU call is made."""
import os
import sys
import types

import numpy as np
import pytest

from tests import mv_ref
from transflow_amd.flow import FlowSource, HipFlowSource


def _mv():
    from transflow_amd import motionvectors
    return motionvectors


# what PyAV's MotionVectors.to_ndarray() returns: libavutil's AVMotionVector, field for field
AV_DTYPE = np.dtype([("source", "int32"), ("w", "uint8"), ("h", "uint8"), ("src_x", "int16"), ("src_y", "int16"),
                     ("dst_x", "int16"), ("dst_y", "int16"), ("flags", "uint64"), ("motion_x", "int32"),
                     ("motion_y", "int32"), ("motion_scale", "uint16")], align=True)


def _av_table(table):
    out = np.zeros(len(table), AV_DTYPE)
    for name in mv_ref.FIELDS:
        out[name] = table[name]
    return out


def test_records_from_structured_arrays_and_from_objects_agree():
    mv = _mv()
    table = mv_ref.h264_like(160, 120, seed=7)
    assert mv.MV_DTYPE == mv_ref.DTYPE and mv.MV_DTYPE.itemsize == 32
    from transflow_amd._lib import TfMvVector
    import ctypes
    assert ctypes.sizeof(TfMvVector) == 32 and [f[0] for f in TfMvVector._fields_] == list(mv.MV_DTYPE.names)
    a = mv.vectors_to_records(_av_table(table))
    b = mv.vectors_to_records([types.SimpleNamespace(**{n: int(r[n]) for n in mv_ref.FIELDS}, dst_x=0) for r in table])
    c = mv.vectors_to_records(table)
    for got in (a, b, c):
        assert got.dtype == mv.MV_DTYPE and got.flags.c_contiguous and got.shape == (len(table),)
        assert got.tobytes() == table.tobytes()
    assert mv.vectors_to_records(None).shape == (0,) and mv.vectors_to_records([]).shape == (0,)
    with pytest.raises(ValueError, match="motion_scale"):
        mv.vectors_to_records(np.zeros(3, np.dtype([(n, "int32") for n in mv_ref.FIELDS[:-1]])))


def _provider(n=10, w=64, h=40, fps=25.0):
    mv = _mv()
    tables = [mv_ref.h264_like(w, h, seed=i) if i % 4 != 3 else None for i in range(n)]
    return mv.ArrayVectorProvider(tables, w, h, fps), tables


def test_builder_arithmetic():
    """Length, seek, repeat and base_length = frames - 1 (av.py:37), as FlowSource.Builder does them for any source."""
    mv = _mv()
    p, _ = _provider(10)
    b = HipFlowSource.from_args(p, use_mvs=True, direction="forward")
    b.build()
    assert (b.width, b.height, b.framerate, b.base_length, b.length) == (64, 40, 25.0, 9, 9)
    assert (b.start_frame, b.end_frame) == (0, 9) and b.direction is FlowSource.Direction.FORWARD
    b = mv.MotionVectorFlowSource.Builder(p, seek_time=0.2, duration_time=0.12, repeat=3)
    b.build()
    assert (b.start_frame, b.end_frame, b.length) == (5, 8, 9)
    assert b.direction is FlowSource.Direction.BACKWARD           # the builder's default, as the reference's
    with b as source:                                             # builds the source: the constructor's rewind reads
        assert isinstance(source, mv.MotionVectorFlowSource)      # start_frame + 1 tables (av.py:55-59), no GPU call
        assert p.pos == 6 and source.input_frame_index == 5 and len(source) == 9
        assert source._mv is None and source._pp is None
        source.rewind()
        assert p.pos == 6
    p2, _ = _provider(3)
    with mv.MotionVectorFlowSource.Builder(p2, seek_time=0.08) as source:      # start frame 2: the last table is skipped
        with pytest.raises(StopIteration):
            p2.read()


def test_from_args_routes_use_mvs_here():
    mv = _mv()
    p, _ = _provider(4)
    b = HipFlowSource.from_args(p, use_mvs=True)
    assert isinstance(b, mv.MotionVectorFlowSource.Builder) and b.provider_arg is p and b.avformat is None
    b = HipFlowSource.from_args("h264::clip.mp4", use_mvs=True, flow_filters="scale=2", repeat=2, lock_expr="0.1,0.1")
    assert isinstance(b, mv.MotionVectorFlowSource.Builder)
    assert (b.provider_arg, b.avformat, b.flow_filters_string, b.repeat) == ("clip.mp4", "h264", "scale=2", 2)
    from transflow_amd.archive import ArchiveFlowSource
    assert isinstance(HipFlowSource.from_args("x.flow.zip", use_mvs=True), ArchiveFlowSource.Builder)   # source.py:397


class _StubAv:
    """A stand-in for the `av` package: what AvVectorProvider touches, recording what it is asked."""

    def __init__(self, frames, framerate=24, count=None):
        self.log = []
        stub = self

        class Context:
            options = None
        Context.framerate = framerate

        class Container:
            def __init__(self):
                self.streams = types.SimpleNamespace(video=[types.SimpleNamespace(
                    codec_context=Context(), frames=len(frames) if count is None else count)])

            def decode(self, video=None):
                stub.log.append(("decode", video))
                return iter(frames)

            def seek(self, offset):
                stub.log.append(("seek", offset))

            def close(self):
                stub.log.append(("close",))

        def open_(file=None, format=None):
            stub.log.append(("open", file, format))
            stub.container = Container()
            return stub.container
        self.av = types.ModuleType("av")
        self.av.container = types.ModuleType("av.container")
        self.av.container.open = open_

    def __enter__(self):
        self.saved = {k: sys.modules.get(k) for k in ("av", "av.container")}
        sys.modules.update({"av": self.av, "av.container": self.av.container})
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


class _SideData(list):
    def __init__(self, table):
        super().__init__(types.SimpleNamespace(**{n: int(r[n]) for n in mv_ref.FIELDS}) for r in table)
        self.table = table


class _SideDataArray(_SideData):
    def to_ndarray(self):
        return _av_table(self.table)


def test_av_provider_against_a_stub_av():
    mv = _mv()
    t0, t1 = mv_ref.h264_like(64, 48, 1), mv_ref.h264_like(64, 48, 2)
    frames = [types.SimpleNamespace(width=64, height=48, side_data={}),
              types.SimpleNamespace(width=64, height=48, side_data={"MOTION_VECTORS": _SideData(t0)}),
              types.SimpleNamespace(width=64, height=48, side_data={"MOTION_VECTORS": _SideDataArray(t1)})]
    with _StubAv(frames) as stub:
        p = mv.AvVectorProvider("clip.mp4", "h264")
        assert stub.log[:2] == [("open", "clip.mp4", "h264"), ("decode", 0)]
        assert stub.container.streams.video[0].codec_context.options == {"flags2": "+export_mvs"}
        assert (p.width, p.height, p.framerate, p.frame_count) == (64, 48, 24.0, 3)
        p.seek_start()
        assert stub.log[2:] == [("seek", 0), ("decode", 0)]
        assert p.read() is None                                        # a frame without side data
        assert mv.vectors_to_records(p.read()).tobytes() == t0.tobytes()     # objects to iterate
        got = p.read()
        assert isinstance(got, np.ndarray) and mv.vectors_to_records(got).tobytes() == t1.tobytes()
        with pytest.raises(StopIteration):
            p.read()
        p.seek_start()
        assert p.read() is None
        with HipFlowSource.from_args("h264::clip.mp4", use_mvs=True) as source:
            assert (source.width, source.height, source.framerate, len(source)) == (64, 48, 24.0, 2)
            assert isinstance(source.provider, mv.AvVectorProvider)
        assert stub.log[-1] == ("close",)
    with _StubAv(frames, framerate=None) as stub:
        assert mv.AvVectorProvider("clip.mp4").framerate == 30.0       # av.py:35-36: the builder's default stays


def test_missing_pyav_is_an_import_error_when_the_provider_is_built():
    try:
        import av  # noqa: F401
        pytest.skip("PyAV is installed here")
    except ImportError:
        pass
    mv = _mv()                                                         # importing the module needed no PyAV
    with pytest.raises(ImportError):
        mv.AvVectorProvider("clip.mp4")
    with pytest.raises(ImportError):
        HipFlowSource.from_args("clip.mp4", use_mvs=True).build()


@pytest.mark.skipif(not os.path.isdir("/root/reference/transflow"), reason="reference tree not present")
def test_dropin_routes_motion_vectors_only_when_asked():
    """dropin.install(motion_vectors=True) serves use_mvs requests; a plain install() leaves them to the reference's
    AvFlowSource (imported here over a stub `av`)."""
    mv = _mv()
    with _StubAv([]) as stub:
        stub.av.container.InputContainer = type("InputContainer", (), {})
        sys.path.insert(0, "/root/reference")
        try:
            from transflow.flow.sources.source import FlowSource as RefFlowSource

            from transflow_amd import dropin
            dropin.install(compositor=False, motion_vectors=True)
            try:
                b = RefFlowSource.from_args("h264::clip.mp4", use_mvs=True, direction=RefFlowSource.Direction.FORWARD)
                assert isinstance(b, mv.MotionVectorFlowSource.Builder)
                assert (b.provider_arg, b.avformat, b.direction) == ("clip.mp4", "h264", FlowSource.Direction.FORWARD)
                assert isinstance(RefFlowSource.from_args("clip.mp4"), HipFlowSource.Builder)
            finally:
                dropin.uninstall()
            dropin.install(compositor=False)
            try:
                b = RefFlowSource.from_args("clip.mp4", use_mvs=True)
                from transflow.flow.sources.av import AvFlowSource
                assert isinstance(b, AvFlowSource.Builder) and not isinstance(b, FlowSource.Builder)
            finally:
                dropin.uninstall()
        finally:
            sys.path.remove("/root/reference")
            for m in [m for m in sys.modules if m == "transflow" or m.startswith("transflow.")]:
                del sys.modules[m]
