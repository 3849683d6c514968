"""The numpy restatement of the flow archive member coder (tests/flowzip_ref.py) against zlib's
inflater, numpy.save, zipfile and numpy.load; what its cases reach, by its own trace; the archives
DeviceFlowArchiveWriter writes with the restatement as its encoder.  No GPU: tests/test_gpu_flowzip.py holds the device's
bytes to the restatement's."""
import io
import os
import zipfile
import zlib

import numpy as np
import pytest

from tests import flowzip_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_traces = {}


def _trace(name):
    """(S, the case's trace): made once and left as they are."""
    if name not in _traces:
        prefix, array, band_bytes, distance = R.case(name)
        _traces[name] = (prefix + array.tobytes(), R.trace(prefix, array.tobytes(), band_bytes, distance))
    return _traces[name]


@pytest.mark.parametrize("name", list(R.CASES))
def test_stream_inflates_to_the_member_within_the_bound(name):
    S, t = _trace(name)
    d = zlib.decompressobj(-15)
    assert d.decompress(t.stream) == S and d.eof and d.unused_data == b""
    assert t.crc == zlib.crc32(S)
    assert len(t.stream) <= R.bound(len(S), t.band_bytes)
    assert t.stream.endswith(b"\x01\x00\x00\xff\xff")
    assert t.bands == -(-len(S) // t.band_bytes) and len(t.band_offsets) == t.bands + 1


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_coded_band_inflates_on_its_own(name):
    S, t = _trace(name)
    for b in range(t.bands):
        piece = t.stream[t.band_offsets[b]:t.band_offsets[b + 1]]
        want = S[b * t.band_bytes:(b + 1) * t.band_bytes]
        if t.band_coded[b]:
            assert piece[0] & 7 == 0b100                      # BFINAL 0, BTYPE 10
            assert piece.endswith(b"\x00\x00\xff\xff")
            assert len(piece) < R.stored_bytes(len(want))
        else:
            assert piece[0] == 0 and len(piece) == R.stored_bytes(len(want))
        assert zlib.decompressobj(-15).decompress(piece) == want, f"band {b}"


@pytest.mark.parametrize("name", [n for n in R.CASES if R.CASES[n][3]])
def test_prefix_and_data_are_numpy_saves_bytes(name):
    prefix, array, _, _ = R.case(name)
    buf = io.BytesIO()
    np.save(buf, array)
    assert prefix + array.tobytes() == buf.getvalue()
    assert len(prefix) % 64 == 0
    from transflow_amd.flowzip import npy_prefix
    assert npy_prefix(array.shape, array.dtype) == prefix


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_code_is_complete_and_within_15_bits(name):
    _, t = _trace(name)
    assert t.kraft == 1.0 and max(t.lengths) <= 15 and len(t.lengths) == 286
    assert t.lengths[256] > 0                                   # end-of-block is always used
    assert sum(1 for n in t.lengths if n) == t.used_symbols >= 2


def test_cases_reach_what_the_kernels_can_get_wrong():
    traces = {name: _trace(name)[1] for name in R.CASES}
    assert {1, 8, 16} <= {t.distance for t in traces.values()}
    for name in ("edges_d1", "edges_d16", "edges_d64"):         # the exact stretches, in one coded band
        assert set(R.EDGES) <= traces[name].stretch_lengths and traces[name].band_coded == [True], name
        assert traces[name].across_trip
    assert traces["edges_d8_b384"].cut_by_band >= 1 and all(traces["edges_d8_b384"].band_coded)
    assert traces["periodic_d16_b320"].cut_by_band >= 1 and all(traces["periodic_d16_b320"].band_coded)
    assert traces["periodic_d16_b320"].first_bytes_would_match >= 1
    assert traces["fibonacci"].repairs >= 1 and all(traces["fibonacci"].band_coded)
    assert max(R.huffman_lengths(np.bincount(R.fibonacci_bytes(16)).tolist() + [2])) > 15      # what the repair mends
    assert max(traces["i64_64x256_b256_d16"].lengths) == 15                                     # and a code that needs none
    assert traces["one_byte_b64"].used_symbols == 2 and traces["one_byte_b64"].lengths[7] == 1
    assert traces["noise_beside_zeros"].band_coded == [True, False, True]
    for name in ("empty_npy_b64", "noise_tail_1", "stored_block_split"):
        assert not any(traces[name].band_coded), name
    t = traces["noise_tail_1"]
    assert t.n % 64 != 0 and t.n - (t.bands - 1) * t.band_bytes == 1
    assert traces["f32_7x9_b64_d1"].n % 64 != 0
    assert traces["stored_block_split"].n > 65535 and traces["stored_block_split"].bands == 1
    at_64 = {t.bands for t in traces.values() if t.band_bytes == 64}
    assert {1, 2, 1025, 2049} <= at_64
    assert traces["i64_64x256_b256_d16"].bands == 1025 and sum(traces["i64_64x256_b256_d16"].band_coded) > 1000
    assert max(t.widest_trip for t in traces.values()) <= 64 * 45      # what 64 lanes can emit in a trip


def test_merge_order_decides_between_equal_weights():
    """(weight, order): leaves before internal nodes of the same weight, lower symbols first."""
    assert R.huffman_lengths([1, 1, 1, 1]) == [2, 2, 2, 2]
    assert R.huffman_lengths([1, 1, 2, 0]) == [2, 2, 1, 0]
    assert R.huffman_lengths([2, 1, 1, 2]) == [2, 2, 2, 2]      # the leaf 0 (2, 0) goes before the node (2, 1000)
    lengths, repairs = R.build_lengths([1, 1] + [0] * 284)
    assert lengths[:2] == [1, 1] and repairs == 0


# ---- the sweeps: what the new cases reach (these are the conditions of the GPU tests) --------------------------------------
def test_sweep_puts_every_length_at_every_phase_in_coded_bands():
    """Per distance: every (phase, length) pair exactly once and nothing else, in one coded band whose phases are the
    stream's; a match of 258 from each of the 64 lanes; one and two pending literals at lane 0 and at lane 1, where they
    are the trip before's bytes.  Cut into bands of 4096 every band is still coded: k_fz_emit tokenises all of them."""
    pairs = {(p, n) for n in R.SWEEP for p in range(R.TRIP)}
    assert R.SWEEP_BAND % 64 == 0
    for d in R.SWEEP_DISTANCES:
        _, t = _trace(f"sweep_d{d}")
        assert t.band_bytes == R.SWEEP_BAND >= t.n and t.bands == 1 and t.band_coded == [True], d
        assert sorted((start % R.TRIP, n) for _, start, n in t.stretches) == sorted(pairs), d
        assert t.phase_lengths == pairs and t.match_258_lanes == set(range(64)), d
        assert {(0, 1), (0, 2), (1, 1), (1, 2)} <= t.pending_literals, d
        S, cut = _trace(f"sweep_d{d}_b4096")
        assert S == _trace(f"sweep_d{d}")[0] and cut.band_bytes == 4096 and cut.bands == -(-len(S) // 4096)
        assert all(cut.band_coded), d
        assert cut.cut_by_band >= 20 and cut.match_258_lanes == set(range(64)), d
        assert {(0, 1), (0, 2), (1, 1), (1, 2)} <= cut.pending_literals, d
    assert set(R.SWEEP_DISTANCES) == {1, 2, 3, 16, 63, 64}
    assert R.SWEEP == (1, 2, 3, 4, 257, 258, 259, 260, 261, 515, 516, 517, 518, 774)


def test_pending_literals_at_lane_0_differ_from_this_trips():
    """A coder that took lane 0's pending literals from its own trip's lane 63 and 62 would go unnoticed where those
    bytes are equal: at every distance some stretch that ends at a trip's last byte has them different."""
    for d in R.SWEEP_DISTANCES:
        S, t = _trace(f"sweep_d{d}")
        found = 0
        for _, start, n in t.stretches:
            end = start + n
            if end % R.TRIP == 0 and n % 258 in (1, 2) and end + R.TRIP <= len(S):
                found += S[end - 1] != S[end + R.TRIP - 1]
        assert found >= 1, d


def test_every_distance_reaches_every_distance_symbol():
    assert {R.distance_symbol(d) for d in range(1, 65)} == set(range(12))
    extra = set()
    for d in range(1, 65):
        member = R.every_distance(d).tobytes()
        assert len(member) <= R.EVERY_DISTANCE_BAND
        t = R.trace(b"", member, R.EVERY_DISTANCE_BAND, d)
        assert t.band_coded == [True] and set(R.EDGES) <= t.stretch_lengths, d
        assert zlib.decompressobj(-15).decompress(t.stream) == member, d
        hdist = (int.from_bytes(t.stream[:4], "little") >> 8) & 31        # behind BFINAL, BTYPE and HLIT
        assert hdist == R.distance_symbol(d), d
        extra.add((hdist, d - R.DIST_BASE[hdist]))
    assert len(extra) == 64 and max(e for _, e in extra) == 15            # every value of every symbol's extra bits


def test_golden_every_distance_streams_are_the_restatements():
    with np.load(os.path.join(GOLDEN, "flowzip_every_distance.npz")) as z:
        streams, ends = z["streams"].tobytes(), [0] + list(z["ends"])
        assert int(z["band_bytes"]) == R.EVERY_DISTANCE_BAND and len(ends) == 65
        for d in range(1, 65):
            member = R.every_distance(d).tobytes()
            stream, crc, _ = R.encode_stream(b"", member, R.EVERY_DISTANCE_BAND, d)
            assert streams[ends[d - 1]:ends[d]] == stream, d
            assert int(z["crcs"][d - 1]) == crc and int(z["sizes"][d - 1]) == len(member)


def test_band_end_cases_end_stretches_at_and_before_the_last_byte():
    """Bands of 320 (64 mod 256) and 512 (0 mod 256) bytes, all coded: a stretch of each of 1, 2, 3, 258 and 259 that
    ends at the band's last byte -- end-of-block's lane then emits what it left -- one that ends a byte before, and a
    band with no stretch.  The last band of 256 is coded too; one of 64 never is (the table header alone is 154 bytes),
    so there it is k_fz_count whose end-of-block lane is alone in its trip."""
    for band_bytes, last, d in ((320, 64, 1), (512, 256, 16)):
        streams = set()
        for variant, (last_n, last_gap) in R.LAST_BAND.items():
            S, t = _trace(f"ends_b{band_bytes}_last{last}_{variant}")
            streams.add(t.stream)
            assert (t.band_bytes, t.distance, t.bands) == (band_bytes, d, 12) and t.n == 11 * band_bytes + last
            assert all(t.band_coded[:11]) and t.band_coded[11] == (last == 256)
            behind = {}                                                   # bytes behind a band's stretch: its lengths
            for band, start, n in t.stretches:
                size = min(band_bytes, t.n - band * band_bytes)
                behind.setdefault(size - start - n, set()).add((size, n))
            assert {(band_bytes, n) for n in R.BAND_END_STRETCHES} <= behind[0]
            assert {(band_bytes, n) for n in R.BAND_END_STRETCHES} <= behind[1]
            assert {(band_bytes, n) for n in R.BAND_END_STRETCHES} <= t.ends_at_band_end
            assert [n for band, _, n in t.stretches if band == 10] == []
            in_last = [(start, n) for band, start, n in t.stretches if band == 11]
            assert in_last == ([(last - last_n - last_gap, last_n)] if last_n else []), variant
            if last == 256 and variant == "end":
                assert (256, 2) in t.ends_at_band_end
        assert len(streams) == 3
    assert 320 % 64 == 0 and 320 % 256 and 512 % 256 == 0


def test_deep_fibonacci_needs_three_repairs_and_the_tie_rule():
    """FIBONACCI_DEEP is the smallest fibonacci_bytes(k) whose code, in one band, is halved three times; on those passes
    equal weights meet, and the other tie rule (internal node before leaf) would give other lengths."""
    for k in range(16, R.FIBONACCI_DEEP + 1):
        counts = np.bincount(R.fibonacci_bytes(k), minlength=R.N_SYMBOLS)
        for start, n in R.stretches(R.fibonacci_bytes(k), 1):             # a stretch of one or two is literals
            assert n <= 2
        counts[R.END_OF_BLOCK] = 1
        assert (R.build_lengths(counts)[1] >= 3) == (k == R.FIBONACCI_DEEP), k
    S, t = _trace("fibonacci_deep")
    assert t.repairs == 3 and t.band_coded == [True] and 10000 < len(S) < 100000 and max(t.lengths) <= 15
    assert _trace("edges_d1")[1].repairs == 0 and _trace("edges_d1")[1].band_bytes == t.band_bytes   # its neighbour on the GPU
    counts = np.bincount(np.frombuffer(S, np.uint8), minlength=R.N_SYMBOLS)
    counts[R.END_OF_BLOCK] = 1
    assert R.build_lengths(counts)[0] == t.lengths
    other, other_repairs = R.build_lengths(counts, first_node=-1000)
    assert other_repairs == 3 and other != t.lengths
    weights = [int(c) for c in counts]
    for _ in range(2):                                                     # the second pass alone already depends on it
        weights = [max(1, w >> 1) if w else 0 for w in weights]
    assert R.huffman_lengths(weights) != R.huffman_lengths(weights, first_node=-1000)


def test_equal_counts_are_all_ties():
    S, t = _trace("equal_counts")
    assert np.bincount(np.frombuffer(S, np.uint8)).tolist() == [16] * 256 and t.stretches == [] and t.repairs == 0
    assert sorted(set(t.lengths[:256])) == [8, 9] and t.lengths[256] == 9
    assert t.lengths[:256] == sorted(t.lengths[:256], reverse=True)        # lower symbols merge first and sink deeper
    assert t.band_coded == [False]                                         # 8 bits a byte: the table is what is compared


@pytest.mark.parametrize("name", list(R.CASES))
def test_golden_streams_are_the_restatements(name):
    """tools/capture_golden_flowzip.py wrote these from the restatement: a change of either shows here."""
    S, t = _trace(name)
    with np.load(os.path.join(GOLDEN, f"flowzip_{name}.npz")) as z:
        assert z["member"].tobytes() == S
        assert z["stream"].tobytes() == t.stream
        assert list(z["lengths"]) == t.lengths
        assert int(z["crc"]) == t.crc and int(z["band_bytes"]) == t.band_bytes and int(z["distance"]) == t.distance


# ---- rounding --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_round_restatement_is_numpys(dtype):
    values = R.round_values(dtype)
    with np.errstate(invalid="ignore"):
        want = np.round(values).astype(int)
    got = R.round_i64(values)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, want)
    assert got[0] == 0 and got[2] == 2 and got[4] == 2 and got[3] == -2          # half to even
    assert (got[-7:-4] == np.iinfo(np.int64).min).all()                            # +-inf, NaN
    field = (R.flow_field(40, 50, 21, np.float64) * 37.3).astype(dtype)
    np.testing.assert_array_equal(R.round_i64(field), np.round(field).astype(int))


# ---- whole archives --------------------------------------------------------------------------------------------------------
META = {"path": "clip.mp4", "width": 40, "height": 24, "framerate": 25.0, "direction": 1, "seek_time": None}


def _arrays():
    f32 = R.flow_field(24, 40, 31)
    nan = f32.copy()
    nan.view(np.uint32)[0, :4, 0] = [0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001]     # NaN payloads
    return [f32, R.round_i64(f32), R.flow_field(24, 40, 32, np.float64), nan,
            f32.astype(np.float16), f32[:, ::2], np.float32(1.5)]                         # the last three: the host's path


def _write(path, **kwargs):
    from transflow_amd.archive import DeviceFlowArchiveWriter
    enc = R.RefEncoder(1024)
    with DeviceFlowArchiveWriter(str(path), encoder=enc, **kwargs) as w:
        w.write_meta(META)
        for a in _arrays():
            w.write_array(a)
        assert w.index == len(_arrays())
    return enc


def _check_archive(path):
    from transflow_amd.archive import read_archive_frame, read_archive_meta
    with zipfile.ZipFile(path) as zf:
        assert zf.testzip() is None
        assert zf.namelist() == ["meta.json"] + ["%09d.npy" % i for i in range(len(_arrays()))]
        assert read_archive_meta(zf) == META
        for i, want in enumerate(_arrays()):
            got = read_archive_frame(zf, i)
            assert got.dtype == want.dtype and got.shape == want.shape
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), f"member {i}"
            buf = io.BytesIO()
            np.save(buf, want)
            assert zf.read("%09d.npy" % i) == buf.getvalue()
            assert zf.getinfo("%09d.npy" % i).compress_type == zipfile.ZIP_DEFLATED


def test_writer_with_the_restatement_writes_an_archive_zipfile_reads(tmp_path):
    path = tmp_path / "a.flow.zip"
    enc = _write(path)
    assert enc.calls == [("host", "<f4", 1), ("host", "<i8", 16), ("host", "<f8", 16), ("host", "<f4", 1)]
    _check_archive(path)
    records = R.zip_records(path.read_bytes())
    assert not records["zip64_end"] and not any(m[6] for m in records["members"])
    assert records["entries"] == 1 + len(_arrays())


def test_writer_writes_zip64_records_once_they_are_needed(tmp_path, monkeypatch):
    from transflow_amd import archive
    monkeypatch.setattr(archive, "ZIP64_LIMIT", 3000)
    monkeypatch.setattr(archive, "ZIP64_COUNT_LIMIT", 4)
    path = tmp_path / "b.flow.zip"
    _write(path)
    _check_archive(path)
    records = R.zip_records(path.read_bytes())
    assert records["zip64_end"] and records["entries"] == 1 + len(_arrays())
    members = records["members"]
    assert not members[0][6] and all(m[6] for m in members[2:])           # meta.json is small and first
    with zipfile.ZipFile(path) as zf:
        for info, m in zip(zf.infolist(), members):
            assert (info.filename, info.CRC, info.compress_size, info.file_size, info.header_offset) == m[:1] + m[2:6]


def test_writer_never_overwrites_unless_told_to(tmp_path):
    from transflow_amd.archive import DeviceFlowArchiveWriter
    path = tmp_path / "c.flow.zip"
    for want in ("c.flow.zip", "c.000.flow.zip", "c.001.flow.zip"):
        with DeviceFlowArchiveWriter(str(path), encoder=R.RefEncoder()) as w:
            w.write_meta(META)
        assert os.path.basename(w.path) == want
    with DeviceFlowArchiveWriter(str(path), replace=True, encoder=R.RefEncoder()) as w:
        assert w.path == str(path)


def test_archive_flow_source_reads_the_archive(tmp_path):
    from transflow_amd.archive import ArchiveFlowSource, DeviceFlowArchiveWriter, read_archive_frame
    path = tmp_path / "d.flow.zip"
    flows = [R.flow_field(24, 40, 40 + i) for i in range(3)]
    with DeviceFlowArchiveWriter(str(path), encoder=R.RefEncoder(512)) as w:
        w.write_meta(META)
        for f in flows:
            w.write_array(f)
    builder = ArchiveFlowSource.Builder(str(path))
    builder.build()
    try:
        assert (builder.width, builder.height, builder.framerate, builder.base_length) == (40, 24, 25.0, 3)
        assert builder.direction.value == 1
        for i, f in enumerate(flows):
            assert read_archive_frame(builder.archive, i).tobytes() == f.tobytes()
        with pytest.raises(KeyError):
            read_archive_frame(builder.archive, 3)
    finally:
        builder.archive.close()


@pytest.mark.skipif(not os.path.isdir("/root/reference/transflow"), reason="reference tree not present")
def test_the_references_archive_source_reads_the_archive(tmp_path):
    import sys
    sys.path.insert(0, "/root/reference")
    try:
        ref = pytest.importorskip("transflow.flow.sources.archive")
        _reference_reads(ref, tmp_path)
    finally:
        sys.path.remove("/root/reference")
        for m in [m for m in sys.modules if m == "transflow" or m.startswith("transflow.")]:
            del sys.modules[m]


def _reference_reads(ref, tmp_path):
    from transflow_amd.archive import DeviceFlowArchiveWriter
    path = tmp_path / "e.flow.zip"
    flows = [R.flow_field(24, 40, 50 + i) for i in range(2)]
    with DeviceFlowArchiveWriter(str(path), encoder=R.RefEncoder(512)) as w:
        w.write_meta(META)
        for f in flows:
            w.write_array(f)
    builder = ref.ArchiveFlowSource.Builder(str(path))
    builder.build()
    try:
        assert (builder.width, builder.height, builder.framerate) == (40, 24, 25.0)
        for i, f in enumerate(flows):
            got = np.load(io.BytesIO(builder.archive.read("%09d.npy" % i)))
            assert got.tobytes() == f.tobytes()
    finally:
        builder.archive.close()


def test_round_switch_is_off_by_default():
    from transflow_amd import deviceflow
    assert deviceflow.DEVICE_ROUND is False
