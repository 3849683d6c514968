"""tf_flowzip_* and tf_flow_round_i64_dev on the GPU against the numpy restatement (tests/flowzip_ref.py): streams, CRCs
and code lengths byte for byte, and -- independently of the restatement -- zlib, zipfile and numpy.load return the
arrays from what the device wrote.  Band sizes and distances are always given: the library's defaults can move."""
import ctypes as C
import io
import sys
import types
import zipfile
import zlib

import numpy as np
import pytest

from tests import flowzip_ref as R

pytestmark = pytest.mark.gpu

_wanted = {}


def _case(name):
    """(prefix, array, band_bytes, distance, the restatement's stream, CRC, lengths): made once, left as they are."""
    if name not in _wanted:
        prefix, array, band_bytes, distance = R.case(name)
        array.setflags(write=False)
        _wanted[name] = (prefix, array, band_bytes, distance) + R.encode_stream(prefix, array.tobytes(), band_bytes, distance)
    return _wanted[name]


def _first_difference(got: bytes, want: bytes) -> str:
    n = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at byte {n}: {got[n:n + 8].hex()} / {want[n:n + 8].hex()}"


@pytest.mark.parametrize("name", list(R.CASES))
def test_device_writes_the_restatements_stream_and_zlib_inflates_the_member(name):
    from transflow_amd.flowzip import FlowZipEncoder
    prefix, array, band_bytes, distance, want, want_crc, want_lengths = _case(name)
    member = prefix + array.tobytes()
    enc = FlowZipEncoder(band_bytes)
    try:
        got, crc = enc.encode_host(prefix, array, distance)
        lengths = enc.last_lengths()
        again, crc_again = enc.encode_host(prefix, array, distance)
        assert enc.band_bytes == band_bytes
    finally:
        enc.close()
    d = zlib.decompressobj(-15)                                            # whatever the restatement says
    assert d.decompress(got) == member and d.eof and d.unused_data == b""
    assert crc == zlib.crc32(member)
    assert len(got) <= R.bound(len(member), band_bytes)
    assert got == want, _first_difference(got, want)
    assert crc == want_crc and lengths == want_lengths
    assert again == got and crc_again == crc                               # integer counts: the same table every time


def test_every_distance_codes_its_symbol_and_extra_bits():
    """The EDGES stretches at each distance of 1 .. 64 through one encoder: all 12 distance symbols, every value of their
    extra bits in the match entries, and the header's HDIST."""
    from transflow_amd.flowzip import FlowZipEncoder
    enc = FlowZipEncoder(R.EVERY_DISTANCE_BAND)
    try:
        for distance in range(1, 65):
            array = R.every_distance(distance)
            member = array.tobytes()
            want, want_crc, want_lengths = R.encode_stream(b"", member, R.EVERY_DISTANCE_BAND, distance)
            got, crc = enc.encode_host(b"", array, distance)
            d = zlib.decompressobj(-15)                                    # whatever the restatement says
            assert d.decompress(got) == member and d.eof and d.unused_data == b"", distance
            assert crc == zlib.crc32(member), distance
            assert got == want, f"distance {distance}: " + _first_difference(got, want)
            assert crc == want_crc and enc.last_lengths() == want_lengths, distance
    finally:
        enc.close()


def test_one_encoder_keeps_no_state_between_members():
    """A member of many coded bands, a short one at another distance, the first again: counts, tables or stream bytes left
    in the handle would show.  Then a member whose code is halved three times, one that needs no repair, the first again:
    weights, ranks or parents left from the repair passes would show."""
    from transflow_amd.flowzip import FlowZipEncoder
    a, b = _case("i64_33x31_b256_d16"), _case("f64_7x9_b128_d16")
    enc = FlowZipEncoder(256)
    try:
        want_b = R.encode_stream(b[0], b[1].tobytes(), 256, 8)
        assert enc.encode_host(a[0], a[1], 16) == (a[4], a[5])
        assert enc.encode_host(b[0], b[1], 8) == want_b[:2]
        assert enc.last_lengths() == want_b[2]
        assert enc.encode_host(a[0], a[1], 16) == (a[4], a[5])
    finally:
        enc.close()
    deep, plain = _case("fibonacci_deep"), _case("edges_d1")
    assert deep[2] == plain[2] == 65536 and deep[3] == plain[3] == 1
    enc = FlowZipEncoder(65536)
    try:
        for prefix, array, _, distance, want, want_crc, want_lengths in (deep, plain, deep):
            assert enc.encode_host(prefix, array, distance) == (want, want_crc)
            assert enc.last_lengths() == want_lengths
    finally:
        enc.close()


@pytest.mark.parametrize("name", ["i64_33x31_b256_d16", "zeros_2049_bands_b64", "ends_b512_last256_end"])
def test_a_buffer_one_byte_short_is_refused_and_left_alone(name):
    """2049 bands: the same contract where the offsets come from the second and third trips of k_fz_scan.  A last band of
    256 bytes: where end-of-block's lane is alone in its block of trips."""
    from transflow_amd import _lib
    lib = _lib.load()
    prefix, array, band_bytes, distance, want, want_crc, _ = _case(name)
    h = C.c_void_p()
    _lib.check(lib.tf_flowzip_create(C.byref(h), len(prefix) + array.nbytes, band_bytes))
    try:
        buf = np.full(len(want) + 64, 0xA5, np.uint8)
        n, crc = C.c_size_t(), C.c_uint32()
        rc = lib.tf_flowzip_copy_last(h, C.c_void_p(buf.ctypes.data), buf.nbytes, C.byref(n))
        assert rc == _lib.TF_ERR_STATE                                     # nothing encoded yet
        for capacity in (len(want) - 1, 0, 10, len(want) // 2):
            rc = lib.tf_flowzip_encode(h, prefix, len(prefix), C.c_void_p(array.ctypes.data), array.nbytes, distance,
                                       C.c_void_p(buf.ctypes.data), capacity, C.byref(n), C.byref(crc))
            assert rc == _lib.TF_ERR_ARG and n.value == len(want)          # the library says what it takes
            assert (buf == 0xA5).all()                                     # nothing written, within or beyond
        rc = lib.tf_flowzip_copy_last(h, C.c_void_p(buf.ctypes.data), len(want) - 1, C.byref(n))
        assert rc == _lib.TF_ERR_ARG and n.value == len(want) and (buf == 0xA5).all()
        _lib.check(lib.tf_flowzip_copy_last(h, C.c_void_p(buf.ctypes.data), len(want), C.byref(n)))
        assert n.value == len(want) and buf[:n.value].tobytes() == want and (buf[n.value:] == 0xA5).all()
    finally:
        lib.tf_flowzip_destroy(h)


def test_bad_arguments_are_refused():
    from transflow_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.tf_flowzip_default_band_bytes() % 64 == 0 and lib.tf_flowzip_default_band_bytes() >= 64
    for size, band in ((0, 64), (100, 32), (100, 96), (100, -64), ((1 << 31) + 1, 64)):
        assert lib.tf_flowzip_create(C.byref(h), size, band) == _lib.TF_ERR_ARG and not h.value
    _lib.check(lib.tf_flowzip_create(C.byref(h), 1000, 0))
    try:
        assert lib.tf_flowzip_band_bytes(h) == lib.tf_flowzip_default_band_bytes()
        data = np.zeros(1000, np.uint8)
        out = np.zeros(2000, np.uint8)
        n, crc = C.c_size_t(), C.c_uint32()

        def encode(prefix_len, nbytes, distance):
            return lib.tf_flowzip_encode(h, bytes(4096), prefix_len, C.c_void_p(data.ctypes.data), nbytes, distance,
                                         C.c_void_p(out.ctypes.data), out.nbytes, C.byref(n), C.byref(crc))
        for args in ((32, 100, 1), (100, 100, 1), (64, 937, 1), (0, 0, 1), (64, 100, 0), (64, 100, 65)):
            assert encode(*args) == _lib.TF_ERR_ARG, args
        assert encode(64, 936, 64) == _lib.TF_OK
        assert zlib.decompressobj(-15).decompress(out[:n.value].tobytes()) == bytes(1000)
    finally:
        lib.tf_flowzip_destroy(h)


# ---- rounding --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_round_kernel_is_numpys(dtype):
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer
    lib = _lib.load()
    field = (R.flow_field(37, 41, 21, np.float64) * 37.3).astype(dtype).reshape(-1)
    values = np.concatenate([R.round_values(dtype), field])
    with np.errstate(invalid="ignore"):
        want = np.round(values).astype(int)
    src, dst = DevBuffer.from_array(values), DevBuffer(values.size * 8)
    try:
        _lib.check(lib.tf_flow_round_i64_dev(C.c_void_p(src.ptr), values.size, int(dtype is np.float64), C.c_void_p(dst.ptr)))
        got = dst.download(values.shape, np.int64)
    finally:
        src.close()
        dst.close()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, R.round_i64(values))


# ---- whole archives --------------------------------------------------------------------------------------------------------
META = {"path": "clip.mp4", "width": 40, "height": 24, "framerate": 25.0, "direction": 1, "seek_time": None}


def _device_flow(array):
    from transflow_amd.device import DevBuffer
    from transflow_amd.deviceflow import DeviceFlow, _Event
    buf = DevBuffer.from_array(array)
    ev = _Event()
    ev.record()
    return DeviceFlow(array.shape, buf.ptr, ev, owner=buf)


def _members(path):
    with zipfile.ZipFile(path) as zf:
        assert zf.testzip() is None
        names = zf.namelist()
        assert names[0] == "meta.json" and names[1:] == ["%09d.npy" % i for i in range(len(names) - 1)]
        return [np.load(io.BytesIO(zf.read(n))) for n in names[1:]]


def test_writer_puts_device_and_host_arrays_into_an_archive_numpy_reads(tmp_path):
    from transflow_amd.archive import DeviceFlowArchiveWriter
    f32 = R.flow_field(24, 40, 31)
    nan = f32.copy()
    nan.view(np.uint32)[0, :4, 0] = [0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001]
    flow, flow2 = _device_flow(f32), _device_flow(nan)
    host = [R.round_i64(f32), R.flow_field(24, 40, 32, np.float64), f32.astype(np.float16), f32[:, ::2]]
    path = tmp_path / "a.flow.zip"
    with DeviceFlowArchiveWriter(str(path), band_bytes=1024) as w:
        w.write_meta(META)
        w.write_array(flow)
        w.write_array(flow, rounded=True)
        w.write_array(flow2)
        for a in host:
            w.write_array(a)
    assert flow._host is None and flow2._host is None                      # neither came down
    want = [f32, np.round(f32).astype(int), nan] + host
    got = _members(path)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b).tobytes(), f"member {i}"
    with zipfile.ZipFile(path) as zf:                                      # the device's members are the restatement's
        stream, crc, _ = R.encode_stream(R.npy_prefix(f32), f32.tobytes(), 1024, 1)
        info = zf.getinfo("000000000.npy")
        assert (info.CRC, info.compress_size, info.file_size) == (crc, len(stream), 128 + f32.nbytes)
        raw = path.read_bytes()
        at = info.header_offset + 30 + len(info.filename)
        assert raw[at:at + len(stream)] == stream


def test_a_flow_from_a_flow_source_is_written_where_it_is(tmp_path):
    from tests.helpers import synth_pair
    from transflow_amd.archive import DeviceFlowArchiveWriter
    from transflow_amd.config import FlowConfig
    from transflow_amd.deviceflow import DeviceFlow
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    a, b = synth_pair(48, 64, seed=3)
    frames = [np.repeat(g[:, :, None], 3, axis=2) for g in (a, b, a)]
    path = tmp_path / "b.flow.zip"
    kept = []
    with DeviceFlowArchiveWriter(str(path), band_bytes=2048) as w, HipFlowSource.from_args(
            ArrayFrameProvider(frames, 25.0), direction="backward", cv_config=FlowConfig(hip_device_flows=True)) as source:
        w.write_meta(META)
        for flow in source:
            assert isinstance(flow, DeviceFlow)
            w.write_array(flow)
            assert flow._host is None
            kept.append(flow)
    got = _members(path)
    assert len(got) == len(kept) == 2
    for a, flow in zip(got, kept):
        assert a.dtype == np.float32 and a.tobytes() == np.asarray(flow).tobytes()
    assert np.abs(got[0]).max() > 0


class _Pipeline:
    """What transflow/pipeline.py:363-377 and 505-506 do with their flow output, around whatever NumpyOutput is."""

    def __init__(self, module, path, round_flow):
        self.round_flow = round_flow
        self.flow_output = module.NumpyOutput(path, True)
        self.flow_output.write_meta(META)

    def export(self, flow):
        self.flow_output.write_array(np.round(flow).astype(int) if self.round_flow else flow)


def test_dropin_exports_flows_that_never_come_down(tmp_path, monkeypatch):
    """install(device_flow_export=True) puts the writer where the pipeline finds NumpyOutput and turns the round switch
    on; the pipeline's own expressions then give the members the host writer would have held.  (The pipeline module here
    is a stand-in with the one name install() replaces: the test needs no installed transflow.)"""
    from transflow_amd import archive, deviceflow, dropin
    from transflow_amd.flowzip import DeviceInt64Flow, RoundedFlow
    package, module = types.ModuleType("transflow"), types.ModuleType("transflow.pipeline")
    package.pipeline, module.NumpyOutput = module, archive.NumpyOutput
    package.__path__ = []
    monkeypatch.setitem(sys.modules, "transflow", package)
    monkeypatch.setitem(sys.modules, "transflow.pipeline", module)
    f32 = R.flow_field(24, 40, 33) * np.float32(3)
    flow, other = _device_flow(f32), _device_flow(f32)                     # `other` is the one that may come down
    assert type(np.round(other)) is np.ndarray                             # off: as before
    dropin.install(flow=False, compositor=False, device_flow_export=True)
    try:
        assert module.NumpyOutput is archive.DeviceFlowArchiveWriter and deviceflow.DEVICE_ROUND
        rounded = np.round(flow)
        assert isinstance(rounded, RoundedFlow) and isinstance(rounded.astype(int), DeviceInt64Flow)
        assert isinstance(np.around(flow), RoundedFlow)
        assert type(np.round(other, 1)) is np.ndarray and type(np.round(other, out=np.empty_like(f32))) is np.ndarray
        for round_flow in (False, True):
            p = _Pipeline(module, str(tmp_path / f"{round_flow}.flow.zip"), round_flow)
            p.export(flow)
            p.flow_output.close()
            assert flow._host is None                                      # nothing brought down
            host = archive.FlowArchiveWriter(str(tmp_path / f"{round_flow}.host.flow.zip"), True)
            host.write_meta(META)
            host.write_array(np.round(f32).astype(int) if round_flow else f32)
            host.close()
            ours, theirs = _members(p.flow_output.path), _members(host.path)
            assert len(ours) == len(theirs) == 1 and ours[0].dtype == theirs[0].dtype
            assert ours[0].tobytes() == theirs[0].tobytes()
        np.testing.assert_array_equal(np.asarray(np.round(flow)), np.round(f32))   # any other use: numpy's values
        np.testing.assert_array_equal(np.round(flow) + 1, np.round(f32) + 1)
    finally:
        dropin.uninstall()
    assert module.NumpyOutput is archive.NumpyOutput and deviceflow.DEVICE_ROUND is False
    assert type(np.round(flow)) is np.ndarray
    np.testing.assert_array_equal(np.round(flow), np.round(f32))
