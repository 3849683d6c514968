"""The device's band inflater (transflow_amd/csrc/flowunzip.hip) held to the Python restatement
(tests/flowunzip_ref.py): the encoder's own bands, zlib's full-flush bands, hand-built bands, the malformed corpus (which
tests/test_flowunzip_ref.py runs through the decoder's shared core on the CPU, under the sanitizers, first); the encoder's
band sizes; the int64 -> float32 conversion; and ArchiveFlowSource(device_inflate=True) against the host's source."""
import ctypes as C
import sys
import types
import zipfile
import zlib

import numpy as np
import pytest

from tests import flowunzip_ref as U
from tests import flowzip_ref as R
from tests.test_flowunzip_ref import MALFORMED, flush_member, ref_member

pytestmark = pytest.mark.gpu

GPU_BANDS = (64, 4096, 65536)
GUARD = 256


@pytest.fixture(scope="module")
def decoder():
    from transflow_amd.flowunzip import FlowUnzipDecoder
    d = FlowUnzipDecoder()
    yield d
    d.close()


def _decode_both_ways(decoder, S, stream, sizes, band_bytes, splits):
    want_crc = zlib.crc32(S)
    for split in splits:
        for _ in range(2):                                   # twice: the handle keeps nothing of a member
            head, data, crc = decoder.decode(stream, sizes, band_bytes, len(S), split)
            assert len(head) == split and len(data) == len(S) - split
            assert head == S[:split], "the head differs"
            if data != S[split:]:
                at = next(i for i, (a, b) in enumerate(zip(data, S[split:])) if a != b)
                raise AssertionError(f"split {split}: first difference at byte {split + at} (band {(split + at) // band_bytes})")
            assert crc == want_crc


def _splits(usize, prefix_len):
    return sorted({0} | {s for s in (prefix_len or 64,) if s <= usize})


@pytest.mark.parametrize("name", list(R.CASES))
def test_device_inflates_the_encoders_members(decoder, name):
    S, stream, sizes, band_bytes, crc = ref_member(name)
    prefix = R.case(name)[0]
    _decode_both_ways(decoder, S, stream, sizes, band_bytes, _splits(len(S), len(prefix)))


@pytest.mark.parametrize("data,level,strategy,band_bytes",
                         [(d, lv, st, bb) for d in U.DATA for lv in U.LEVELS for st in U.STRATEGIES for bb in GPU_BANDS])
def test_device_inflates_zlibs_full_flush_bands(decoder, data, level, strategy, band_bytes):
    S, stream, sizes, _, tail = flush_member(data, level, strategy, band_bytes)
    assert U.tail_ok(stream[sum(sizes):])
    _decode_both_ways(decoder, S, stream, sizes, band_bytes, _splits(len(S), 128))


@pytest.mark.parametrize("name", list(U.hand_valid()))
def test_device_inflates_the_hand_built_bands(decoder, name):
    stream, sizes, band_bytes, S = U.hand_valid()[name]
    _decode_both_ways(decoder, S, stream, sizes, band_bytes, _splits(len(S), 64))


def _guarded(nbytes):
    from transflow_amd.device import DevBuffer
    buf = DevBuffer(GUARD + nbytes + GUARD)
    buf.upload(np.full(GUARD + nbytes + GUARD, 0xA5, np.uint8))
    return buf


def _guards_untouched(buf, nbytes):
    got = buf.download((GUARD + nbytes + GUARD,), np.uint8)
    return bool((got[:GUARD] == 0xA5).all() and (got[GUARD + nbytes:] == 0xA5).all()), got[GUARD:GUARD + nbytes]


@pytest.mark.parametrize("name", list(MALFORMED))
def test_device_rejects_the_malformed_bands_and_touches_nothing_else(decoder, name):
    from transflow_amd.flowunzip import BandRejected
    (stream, sizes, band_bytes, usize, bad), reason = MALFORMED[name]
    assert U.inflate_member(stream, sizes, band_bytes, usize)[1:3] == (bad, reason)
    for split in (0, 64):
        buf = _guarded(usize - split)
        with pytest.raises(BandRejected) as e:
            decoder.decode_device(stream, sizes, band_bytes, usize, split, buf.ptr + GUARD)
        assert e.value.band == bad
        assert "reason %d" % U.REJECT_NUMBER[reason] in str(e.value)
        assert _guards_untouched(buf, usize - split)[0]
        buf.close()
    # the handle is as good as before
    stream, sizes, band_bytes, S = U.hand_valid()["three_blocks"]
    buf = _guarded(len(S))
    head, crc = decoder.decode_device(stream, sizes, band_bytes, len(S), 0, buf.ptr + GUARD)
    clean, got = _guards_untouched(buf, len(S))
    assert clean and got.tobytes() == S and crc == zlib.crc32(S) and head == b""
    buf.close()


def test_valid_members_stay_inside_their_buffer(decoder):
    for name in ("noise_tail_1", "f32_7x9_b64_d1", "stored_block_split"):
        S, stream, sizes, band_bytes, crc = ref_member(name)
        for split in (0, 128):
            buf = _guarded(len(S) - split)
            head, got_crc = decoder.decode_device(stream, sizes, band_bytes, len(S), split, buf.ptr + GUARD)
            clean, got = _guards_untouched(buf, len(S) - split)
            assert clean and head == S[:split] and got.tobytes() == S[split:] and got_crc == crc
            buf.close()


def test_inconsistent_sizes_are_refused_before_anything_is_launched(decoder):
    S, stream, sizes, band_bytes, crc = ref_member("f32_24x40_b1024_d1")
    ok = dict(stream=stream, band_sizes=sizes, band_bytes=band_bytes, usize=len(S), split=128)
    decoder.decode(**ok)
    for change in (dict(split=32), dict(split=4096 + 64), dict(band_bytes=1000), dict(band_sizes=sizes[:-1]),
                   dict(band_sizes=sizes + [1]), dict(band_sizes=sizes[:-1] + [sizes[-1] + 6]), dict(usize=len(S) + 1024),
                   dict(band_bytes=0)):
        with pytest.raises(ValueError) as e:
            decoder.decode(**dict(ok, **change))
        assert not hasattr(e.value, "band"), change                  # TF_ERR_ARG, not a rejected band
    head, data, got = decoder.decode(**ok)
    assert head + data == S and got == crc


# ---- the encoder's band sizes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype,band_bytes", [((7, 9, 2), np.float32, 64), ((128, 256, 2), np.float32, 8192),
                                                    ((33, 31, 2), np.int64, 256)])
def test_round_trip_on_the_device(decoder, shape, dtype, band_bytes):
    from transflow_amd import _lib
    from transflow_amd.flowzip import DISTANCES, FlowZipEncoder, npy_prefix
    field = R.flow_field(shape[0], shape[1], 61)
    array = field if dtype == np.float32 else R.round_i64(field)
    prefix = npy_prefix(array.shape, array.dtype)
    enc = FlowZipEncoder(band_bytes)
    with pytest.raises(_lib.TfError):
        enc._handle(len(prefix) + array.nbytes)
        enc.last_band_sizes()                                        # TF_ERR_STATE before the first encode
    stream, crc = enc.encode_host(prefix, array, DISTANCES[array.dtype])
    sizes = enc.last_band_sizes()
    S = prefix + array.tobytes()
    t = R.trace(prefix, array.tobytes(), band_bytes, DISTANCES[array.dtype])
    assert sizes == [b - a for a, b in zip(t.band_offsets[:-1], t.band_offsets[1:])]
    assert len(sizes) == -(-len(S) // band_bytes) and sum(sizes) + 5 == len(stream)
    assert U.tail_ok(stream[sum(sizes):])
    n = C.c_size_t()
    small = (C.c_uint32 * len(sizes))()
    rc = enc._lib.tf_flowzip_last_band_sizes(enc._h, small, len(sizes) - 1, C.byref(n))       # too small by one
    assert rc == _lib.TF_ERR_ARG and n.value == len(sizes)
    _decode_both_ways(decoder, S, stream, sizes, band_bytes, [0, len(prefix)])
    enc.close()


def test_i64_to_f32_is_numpys_astype():
    from transflow_amd.device import DevBuffer, sync
    from transflow_amd.flowunzip import i64_to_f32_dev
    big = [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 53 + 1, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 40 + 2 ** 16, 2 ** 40 + 3 * 2 ** 16, 2 ** 62 + 2 ** 38]
    values = np.array([0, 1, -1] + big + [-v for v in big] + [np.iinfo(np.int64).max, np.iinfo(np.int64).min]
                      + list(R.round_i64(R.flow_field(9, 7, 62) * np.float32(1e6)).ravel()), np.int64)
    want = values.astype(np.float32)
    src, dst = DevBuffer.from_array(values), DevBuffer(4 * values.size)
    i64_to_f32_dev(src.ptr, values.size, dst.ptr)
    sync()
    got = dst.download(values.shape, np.float32)
    assert got.tobytes() == want.tobytes()
    assert want[3] == 2.0 ** 24 and want[4] == 2.0 ** 24 + 4                 # the ties went to even
    i64_to_f32_dev(0, 0, 0)                                                  # no values: nothing to do, and no error


# ---- the source ----------------------------------------------------------------------------------------------------------------
H, W = 24, 40


def _meta(direction):
    return {"path": "clip.mp4", "width": W, "height": H, "framerate": 25.0, "direction": direction, "seek_time": None}


def _frames(rounded):
    flows = [R.flow_field(H, W, 70 + i) * np.float32(2.5) for i in range(3)]
    return [R.round_i64(f) for f in flows] if rounded else flows


_archives = {}


def _archive(tmp_path_factory, rounded, direction, kind="indexed"):
    """An archive of three frames: `indexed` through DeviceFlowArchiveWriter(index=True), `one_missing` with the second
    member's index left out, `plain` by FlowArchiveWriter (zlib's members), `flipped` indexed with one compressed byte of
    the second member changed."""
    from transflow_amd.archive import DeviceFlowArchiveWriter, FlowArchiveWriter, member_span
    from transflow_amd.flowzip import FlowZipEncoder
    key = (rounded, direction, kind)
    if key in _archives:
        return _archives[key]
    path = str(tmp_path_factory.mktemp("flowunzip") / ("%s_%d_%d.flow.zip" % (kind, rounded, direction)))
    if kind == "plain":
        writer = FlowArchiveWriter(path)
    else:
        encoder = FlowZipEncoder(1024, views=True)
        writer = DeviceFlowArchiveWriter(path, encoder=_SomeIndexes(encoder, {1}) if kind == "one_missing" else encoder, index=True)
    with writer as w:
        w.write_meta(_meta(direction))
        for a in _frames(rounded):
            w.write_array(a)
    with zipfile.ZipFile(path) as zf:
        indexed = [bool(zf.getinfo("%09d.npy" % i).extra) for i in range(3)]
        assert indexed == {"plain": [False] * 3, "one_missing": [True, False, True]}.get(kind, [True] * 3)
        if kind == "flipped":
            with open(path, "rb") as f:
                offset, csize = member_span(f, zf.getinfo("%09d.npy" % 1))
    if kind == "flipped":
        data = bytearray(open(path, "rb").read())
        data[offset + csize // 2] ^= 0x10
        open(path, "wb").write(bytes(data))
    _archives[key] = path
    return path


class _SomeIndexes:
    """An encoder that has no last_band_sizes for the members of `without`."""

    def __init__(self, encoder, without):
        self._encoder, self._without, self._n = encoder, without, 0

    band_bytes = property(lambda self: self._encoder.band_bytes)

    def encode_host(self, *args):
        self._n += 1
        return self._encoder.encode_host(*args)

    @property
    def last_band_sizes(self):
        if self._n - 1 in self._without:
            raise AttributeError("last_band_sizes")
        return self._encoder.last_band_sizes

    def close(self):
        self._encoder.close()


def _drain(source):
    """The source's flows, up to the KeyError of the first missing member: that is how an archive ends."""
    flows = []
    with pytest.raises(KeyError):
        for _ in range(100):
            flows.append(next(source))
    return flows


def _replay(path, filters=None, mask=None, lock_skip=None, **kwargs):
    """(Like the reference's, the archive builder does no arithmetic on its arguments: filters, mask and lock are given
    to the source as objects.)"""
    from transflow_amd.archive import ArchiveFlowSource
    from transflow_amd.flow import FlowFilter
    builder = ArchiveFlowSource.Builder(path, **kwargs)
    builder.build()
    builder.mask = mask
    builder.flow_filters = [FlowFilter.from_string(part) for part in filters.split(";")] if filters else []
    builder.lock_expr_skip = lock_skip
    source = builder.cls(*builder.args(), **builder.kwargs())
    source.validate()
    try:
        flows = _drain(source)
        kinds = [type(f).__name__ for f in flows]
        hosts = [getattr(f, "_host", "ndarray") for f in flows]
        return [np.array(np.asarray(f), copy=True) for f in flows], kinds, hosts
    finally:
        source.close()


MASK = (np.arange(H * W, dtype=np.float32).reshape(H, W, 1) % 7) / np.float32(7)


@pytest.mark.parametrize("rounded", [False, True])
@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("filters,mask", [(None, None), ("scale=1.5+t", MASK)])
def test_resident_replay_is_the_hosts(tmp_path_factory, rounded, direction, filters, mask):
    path = _archive(tmp_path_factory, rounded, direction)
    want, kinds, _ = _replay(path, filters, mask)
    assert len(want) == 3 and kinds == ["ndarray"] * 3
    want = [w.astype(np.float32) for w in want]
    for device_flows in (False, True):
        got, kinds, hosts = _replay(path, filters, mask, device_inflate=True, device_flows=device_flows)
        assert len(got) == 3
        if device_flows:
            assert kinds == ["DeviceFlow"] * 3 and hosts == [None] * 3       # they never came down before they were asked for
        else:
            assert kinds == ["ndarray"] * 3
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.dtype == np.float32 and a.shape == (H, W, 2)
            assert a.tobytes() == b.tobytes(), f"frame {i}"
    assert any(np.abs(w).max() > 0 for w in want)


@pytest.mark.parametrize("rounded", [False, True])
@pytest.mark.parametrize("kind", ["one_missing", "plain"])
def test_members_without_an_index_go_the_hosts_way(tmp_path_factory, rounded, kind):
    path = _archive(tmp_path_factory, rounded, 1, kind)
    want, _, _ = _replay(path)
    got, kinds, _ = _replay(path, device_inflate=True)
    assert kinds == ["ndarray"] * 3 and len(got) == 3
    for a, b in zip(got, want):
        assert a.astype(np.float32).tobytes() == b.astype(np.float32).tobytes()
    if not rounded:
        assert [a.dtype for a in got] == [np.float32] * 3


def test_resident_replay_falls_back_while_the_raw_flow_is_needed_on_the_host(tmp_path_factory):
    path = _archive(tmp_path_factory, False, 1)
    want, _, _ = _replay(path, lock_skip=lambda t: t > 100, lock_mode="skip")
    got, kinds, _ = _replay(path, lock_skip=lambda t: t > 100, lock_mode="skip", device_inflate=True, device_flows=True)
    assert kinds == ["ndarray"] * 3
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()


def test_a_flipped_byte_is_a_bad_zip_file(tmp_path_factory):
    path = _archive(tmp_path_factory, False, 1, "flipped")
    with pytest.raises(zipfile.BadZipFile) as e:
        _replay(path, device_inflate=True)
    assert "000000001.npy" in str(e.value)
    with pytest.raises((zipfile.BadZipFile, zlib.error)):          # and so it is for the host
        _replay(path)


def test_the_archive_ends_with_the_first_missing_member(tmp_path_factory):
    from transflow_amd.archive import ArchiveFlowSource
    path = _archive(tmp_path_factory, False, 1)
    builder = ArchiveFlowSource.Builder(path, device_inflate=True)
    builder.build()
    source = builder.cls(*builder.args(), **builder.kwargs())
    try:
        assert source.length is None
        for _ in range(3):
            next(source)
        with pytest.raises(KeyError):
            next(source)
    finally:
        source.close()


def test_dropin_switch_builds_this_source(tmp_path_factory, monkeypatch):
    """install(device_flow_replay=True): the builder the reference's FlowSource.from_args returns for a `.flow.zip` path is
    ArchiveFlowSource's with device_inflate on.  (The reference here is a stand-in with the one class install() patches.)"""
    from transflow_amd import archive, dropin
    names = ["transflow", "transflow.flow", "transflow.flow.sources", "transflow.flow.sources.source", "transflow.pipeline"]
    modules = {n: types.ModuleType(n) for n in names}
    for n in names[:-2]:
        modules[n].__path__ = []

    class FlowSource:
        @classmethod
        def from_args(cls, flow_path, **kwargs):
            return "the reference's"

    modules["transflow.flow.sources.source"].FlowSource = FlowSource
    modules["transflow.pipeline"].NumpyOutput = archive.NumpyOutput
    for n, m in modules.items():
        monkeypatch.setitem(sys.modules, n, m)
    path = _archive(tmp_path_factory, False, 1)
    dropin.install(compositor=False, device_flow_replay=True, device_flow_export="indexed")
    try:
        builder = FlowSource.from_args(path, direction="backward")
        assert isinstance(builder, archive.ArchiveFlowSource.Builder) and builder.device_inflate is True
        assert not builder.device_flows
        with builder as source:
            assert isinstance(source, archive.ArchiveFlowSource) and source.device_inflate
            flows = [np.array(f, copy=True) for f in _drain(source)]
        want, _, _ = _replay(path)
        assert [f.tobytes() for f in flows] == [w.tobytes() for w in want]
        out = str(tmp_path_factory.mktemp("export") / "x.flow.zip")
        writer = modules["transflow.pipeline"].NumpyOutput(out, True)
        assert isinstance(writer, archive.DeviceFlowArchiveWriter) and writer._index
        writer.write_meta(_meta(1))
        writer.write_array(_frames(False)[0])
        writer.close()
        with zipfile.ZipFile(out) as zf:
            assert archive.read_member_index(zf.getinfo("%09d.npy" % 0)) is not None
    finally:
        dropin.uninstall()
    assert FlowSource.from_args(path) == "the reference's"
    dropin.install(compositor=False)
    try:
        assert FlowSource.from_args(path, direction="backward").device_inflate is False
    finally:
        dropin.uninstall()


def test_plain_export_switch_still_writes_no_index(tmp_path_factory, monkeypatch):
    from transflow_amd import archive, dropin
    package, module = types.ModuleType("transflow"), types.ModuleType("transflow.pipeline")
    package.pipeline, module.NumpyOutput = module, archive.NumpyOutput
    package.__path__ = []
    monkeypatch.setitem(sys.modules, "transflow", package)
    monkeypatch.setitem(sys.modules, "transflow.pipeline", module)
    dropin.install(flow=False, compositor=False, device_flow_export=True)
    try:
        assert module.NumpyOutput is archive.DeviceFlowArchiveWriter
        out = str(tmp_path_factory.mktemp("export") / "y.flow.zip")
        with module.NumpyOutput(out, True) as w:
            w.write_meta(_meta(1))
            w.write_array(_frames(False)[0])
        with zipfile.ZipFile(out) as zf:
            assert zf.getinfo("%09d.npy" % 0).extra == b""
    finally:
        dropin.uninstall()
