"""The Python restatement of the band inflater (tests/flowunzip_ref.py) against zlib, band by band;
what its cases reach, by its own trace; the band index in archives written without a GPU; and the decoder's shared
host/device core (transflow_amd/csrc/flowunzip_common.h) run on the CPU under the sanitizers, verdict by verdict, and the
codecs' shared CRC-32 (crc32_common.h) likewise.  No GPU: tests/test_gpu_flowunzip.py holds the device to the restatement."""
import io
import os
import shutil
import struct
import subprocess
import time
import zipfile
import zlib

import numpy as np
import pytest

from tests import flowunzip_ref as U
from tests import flowzip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

_members = {}


def ref_member(name):
    """(S, stream, band sizes, band_bytes, crc) of a flowzip_ref case: made once and left as it is."""
    if name not in _members:
        prefix, array, band_bytes, distance = R.case(name)
        t = R.trace(prefix, array.tobytes(), band_bytes, distance)
        sizes = [b - a for a, b in zip(t.band_offsets[:-1], t.band_offsets[1:])]
        _members[name] = (prefix + array.tobytes(), t.stream, sizes, band_bytes, t.crc)
    return _members[name]


def flush_member(data, level, strategy, band_bytes):
    key = (data, level, strategy, band_bytes)
    if key not in _members:
        S = U.matrix_data(data)
        stream, sizes, tail = U.full_flush_stream(S, band_bytes, level, U.STRATEGIES[strategy])
        _members[key] = (S, stream, sizes, band_bytes, tail)
    return _members[key]


_inflated = {}


def _inflate(stream, first, size, want):
    """U.inflate_band of a stream that one of the makers above keeps: computed once."""
    key = (id(stream), first, size, want)
    if key not in _inflated:
        _inflated[key] = U.inflate_band(stream, first, size, want)
    return _inflated[key]


MATRIX = [(d, lv, st, bb) for d in U.DATA for lv in U.LEVELS for st in U.STRATEGIES for bb in U.BANDS]
_traces = []          # every BandTrace the valid cases made, for test_cases_reach_...
_band_counts = set()
_facts = set()


def _check_member(S, stream, sizes, band_bytes):
    """The restatement returns zlib's bytes band by band; the traces are kept."""
    offs = U.offsets_of(sizes)
    assert len(sizes) == -(-len(S) // band_bytes)
    pieces = []
    for band, n in enumerate(sizes):
        want = min(band_bytes, len(S) - band * band_bytes)
        data, reason, trace = _inflate(stream, offs[band], n, want)
        assert reason is None, (band, reason)
        assert data == U.zlib_accepts(stream[offs[band]:offs[band] + n], want), band
        assert data == S[band * band_bytes:band * band_bytes + want], band
        pieces.append(data)
        _traces.append(trace)
        if trace.block_types == [0, 0, 0]:
            _facts.add("stored band of two blocks")        # two with bytes, and the empty one a flush ends with
        if trace.block_types == [0, 0] and want > 65535:
            _facts.add("stored band of two blocks")
        if want == 1 and band == len(sizes) - 1:
            _facts.add("last band of one byte")
    assert zlib.crc32(b"".join(pieces)) == zlib.crc32(S)
    _band_counts.add(len(sizes))
    if len(S) % 64:
        _facts.add("usize no multiple of 64")
    return offs[-1]


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_inflates_the_encoders_bands(name):
    S, stream, sizes, band_bytes, crc = ref_member(name)
    used = _check_member(S, stream, sizes, band_bytes)
    assert stream[used:] == b"\x01\x00\x00\xff\xff" and U.tail_ok(stream[used:])
    assert crc == zlib.crc32(S)


@pytest.mark.parametrize("data,level,strategy,band_bytes", MATRIX)
def test_restatement_inflates_zlibs_full_flush_bands(data, level, strategy, band_bytes):
    S, stream, sizes, _, tail = flush_member(data, level, strategy, band_bytes)
    used = _check_member(S, stream, sizes, band_bytes)
    assert stream[used:] == tail and tail in (b"\x03\x00", b"\x01\x00\x00\xff\xff") and U.tail_ok(tail)
    assert zlib.decompressobj(-15).decompress(stream) == S


@pytest.mark.parametrize("name", list(U.hand_valid()))
def test_restatement_inflates_the_hand_built_bands(name):
    stream, sizes, band_bytes, S = U.hand_valid()[name]
    _check_member(S, stream, sizes, band_bytes)


def test_cases_reach_what_the_kernel_can_get_wrong():
    """Runs behind the tests above (pytest keeps a file's order) and reads the traces they left."""
    if len(_traces) < 1000:
        for name in R.CASES:
            test_restatement_inflates_the_encoders_bands(name)
        for case in MATRIX:
            test_restatement_inflates_zlibs_full_flush_bands(*case)
        for name in U.hand_valid():
            test_restatement_inflates_the_hand_built_bands(name)
    kinds = set()
    for t in _traces:
        kinds |= set(t.block_types)
    assert kinds == {0, 1, 2}
    assert any(t.coded_blocks > 1 for t in _traces)                     # a band of more than one coded block
    repeats = set()
    for t in _traces:
        repeats |= t.repeat_codes
    assert repeats == {16, 17, 18}
    assert max(t.max_code_length for t in _traces) == 15
    S, stream, sizes, band_bytes, _ = flush_member("periodic", 6, "default", 65536)
    far = [U.inflate_band(stream, o, n, min(band_bytes, len(S) - b * band_bytes))[2].max_distance
           for b, (o, n) in enumerate(zip(U.offsets_of(sizes), sizes))]
    assert max(far) >= 32000                                            # from zlib
    stream, sizes, band_bytes, S = U.hand_valid()["distance_32768"]
    trace = U.inflate_band(stream, 0, sizes[0], len(S))[2]
    assert trace.max_distance == 32768 and trace.match_at_start_distance >= 1
    stream, sizes, band_bytes, S = U.hand_valid()["distance_is_produced"]
    assert U.inflate_band(stream, sizes[0], sizes[1], len(S) - band_bytes)[2].match_at_start_distance == 2
    stream, sizes, band_bytes, S = U.hand_valid()["run_258_d1"]
    trace = U.inflate_band(stream, 0, sizes[0], band_bytes)[2]
    assert trace.longest_match == 258 and trace.overlapping == 4 and trace.max_distance == 1
    stream, sizes, band_bytes, S = U.hand_valid()["single_distance_code"]
    assert U.inflate_band(stream, 0, sizes[0], len(S))[2].single_distance_code == 1
    assert any(t.single_distance_code for t in _traces[:2000])           # the encoder's own coded bands too
    assert any(t.overlapping for t in _traces)
    assert {"stored band of two blocks", "last band of one byte", "usize no multiple of 64"} <= _facts
    assert {1, 2, 1025} <= _band_counts


MALFORMED = U.malformed()


@pytest.mark.parametrize("name", list(MALFORMED))
def test_malformed_bands_are_refused_by_zlib_and_named_by_the_restatement(name):
    (stream, sizes, band_bytes, usize, bad), reason = MALFORMED[name]
    offs = U.offsets_of(sizes)
    for band, n in enumerate(sizes):
        want = min(band_bytes, usize - band * band_bytes)
        data, why, _ = U.inflate_band(stream, offs[band], n, want)
        accepted = U.zlib_accepts(stream[offs[band]:offs[band] + n], want)
        if band == bad:
            assert data is None and why == reason
            assert accepted is None
        else:
            assert why is None and data == accepted
    assert U.inflate_member(stream, sizes, band_bytes, usize)[1:3] == (bad, reason)


def test_every_rejection_has_a_case_and_the_two_that_point_outside():
    reasons = {reason for _, reason in MALFORMED.values()}
    assert reasons == set(U.REJECTS) - {"ok"}
    # the distance case's source lies before the band's first output byte, where the band before it put its bytes;
    # the exhausted cases stop where the next band's compressed bytes begin
    (stream, sizes, band_bytes, usize, bad), reason = MALFORMED["distance_before_band"]
    assert bad == 1 and sizes[0] > 0 and reason == "distance"
    (stream, sizes, band_bytes, usize, bad), reason = MALFORMED["exhausted_in_literals"]
    assert bad == 1 and sizes[2] > 0 and reason == "exhausted"
    offs = U.offsets_of(sizes)
    longer = U.inflate_band(stream, offs[1], sizes[1] + sizes[2], 64)       # with the next band's bytes in reach it goes on
    assert longer[1] != "exhausted"


# ---- goldens -----------------------------------------------------------------------------------------------------------------
def test_golden_bands_are_the_restatements():
    """tools/capture_golden_flowunzip.py wrote these from the restatement: a change of either shows here."""
    with np.load(os.path.join(GOLDEN, "flowunzip_valid.npz")) as z:
        assert sorted(str(n) for n in z["names"]) == sorted(U.hand_valid())
        for name, (stream, sizes, band_bytes, S) in U.hand_valid().items():
            assert z[name + ".stream"].tobytes() == stream and z[name + ".member"].tobytes() == S
            assert list(z[name + ".sizes"]) == sizes and int(z[name + ".band_bytes"]) == band_bytes
    with np.load(os.path.join(GOLDEN, "flowunzip_malformed.npz")) as z:
        assert sorted(str(n) for n in z["names"]) == sorted(MALFORMED)
        for name, ((stream, sizes, band_bytes, usize, bad), reason) in MALFORMED.items():
            assert z[name + ".stream"].tobytes() == stream and list(z[name + ".sizes"]) == sizes
            assert [int(v) for v in z[name + ".verdict"]] == [band_bytes, usize, bad, U.REJECT_NUMBER[reason]]


# ---- the shared core on the CPU, under the sanitizers ----------------------------------------------------------------------------
def _corpus():
    cases = {}
    for name, (stream, sizes, band_bytes, S) in U.hand_valid().items():
        cases["hand." + name] = (stream, sizes, band_bytes, len(S))
    for name, ((stream, sizes, band_bytes, usize, _), _) in MALFORMED.items():
        cases["bad." + name] = (stream, sizes, band_bytes, usize)
    for name in R.CASES:
        S, stream, sizes, band_bytes, _ = ref_member(name)
        cases["ref." + name] = (stream, sizes, band_bytes, len(S))
    for data, level, strategy, band_bytes in MATRIX:
        S, stream, sizes, _, _ = flush_member(data, level, strategy, band_bytes)
        cases["zlib.%s.%d.%s.%d" % (data, level, strategy, band_bytes)] = (stream, sizes, band_bytes, len(S))
    return cases


def _run_host_check(tmp_path, source_name, corpus_lines):
    """tools/<source_name> built with the sanitizers by the first host compiler whose program runs, and run over the
    corpus: its output, after no sanitizer report."""
    source = os.path.join(ROOT, "tools", source_name)
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    program = None
    for compiler in ("g++", "clang++", "c++"):
        if shutil.which(compiler) is None:
            continue
        out = str(tmp_path / ("check_" + compiler.replace("+", "x")))
        built = subprocess.run([compiler, *flags, source, "-o", out], capture_output=True, text=True)
        probe = built.returncode == 0 and subprocess.run([out], capture_output=True, text=True)
        if probe and probe.returncode == 2 and "usage" in probe.stderr:
            program = out
            break
    if program is None:
        pytest.skip("no host compiler here builds a program that runs with -fsanitize=address,undefined")
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(corpus_lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([program, str(corpus)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    return run.stdout


def test_host_check_program(tmp_path):
    """tools/flowunzip_host_check.cpp -- the machine the device's lane 0 runs, with every buffer a heap block of the size
    the decoder is entitled to -- over the whole valid and malformed corpus: no sanitizer report, and every verdict and
    CRC-32 the restatement's."""
    cases = _corpus()
    stdout = _run_host_check(tmp_path, "flowunzip_host_check.cpp", U.corpus_lines(cases))
    got = {}
    for line in stdout.splitlines():
        name, verdict, crc = line.split()
        got[name] = (int(verdict), int(crc))
    want = {}
    for name, (stream, sizes, band_bytes, usize) in cases.items():
        offs = U.offsets_of(sizes)
        for band, n in enumerate(sizes):
            data, reason, _ = _inflate(stream, offs[band], n, min(band_bytes, usize - band * band_bytes))
            want["%s/%d" % (name, band)] = (0, zlib.crc32(data)) if data is not None else (U.REJECT_NUMBER[reason], 0)
    assert len(got) == len(want)
    wrong = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
    assert not wrong, sorted(wrong.items())[:10]


CRC_LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, *range(252, 261), 4095, 4096, 4097, 65535, 65539]


def test_crc32_host_check_program(tmp_path):
    """tools/crc32_host_check.cpp -- the CRC-32 the device codecs share (transflow_amd/csrc/crc32_common.h), a wave's lanes
    done by a loop -- over random and all-zero messages of the lengths where the slices change shape: no sanitizer
    report, and the table's value, the 64 plain slices', the 64 whole-dword slices' and the two bands' all zlib's."""
    rng = np.random.default_rng(20)
    cases = {}
    for n in CRC_LENGTHS:
        cases["random.%d" % n] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        cases["zeros.%d" % n] = bytes(n)
    stdout = _run_host_check(tmp_path, "crc32_host_check.cpp", ["%s %s" % (name, data.hex() or "-") for name, data in cases.items()])
    got = {}
    for line in stdout.splitlines():
        name, *values = line.split()
        got[name] = [int(v) for v in values]
    want = {name: [zlib.crc32(data)] * 4 for name, data in cases.items()}
    assert len(got) == len(want)
    wrong = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
    assert not wrong, sorted(wrong.items())[:10]


# ---- indexed archives ----------------------------------------------------------------------------------------------------------
META = {"path": "clip.mp4", "width": 40, "height": 24, "framerate": 25.0, "direction": 1, "seek_time": None}


def _arrays():
    f32 = R.flow_field(24, 40, 31)
    return [f32, R.round_i64(f32), R.flow_field(24, 40, 32, np.float64), f32.astype(np.float16), f32[:, ::2]]


def _write(path, encoder, **kwargs):
    from transflow_amd.archive import DeviceFlowArchiveWriter
    with DeviceFlowArchiveWriter(str(path), encoder=encoder, **kwargs) as w:
        w.write_meta(META)
        for a in _arrays():
            w.write_array(a)


def _check_reads(path):
    from transflow_amd.archive import read_archive_frame, read_archive_meta
    with zipfile.ZipFile(path) as zf:
        assert zf.testzip() is None
        assert read_archive_meta(zf) == META
        for i, want in enumerate(_arrays()):
            got = read_archive_frame(zf, i)
            assert got.dtype == want.dtype and got.shape == want.shape
            assert got.tobytes() == np.ascontiguousarray(want).tobytes()
            buf = io.BytesIO()
            np.save(buf, want)
            assert zf.read("%09d.npy" % i) == buf.getvalue()
            assert np.load(io.BytesIO(zf.read("%09d.npy" % i))).tobytes() == np.ascontiguousarray(want).tobytes()


def test_indexed_archive_reads_as_before_and_carries_the_sizes(tmp_path):
    from transflow_amd.archive import member_span, read_member_index
    path = tmp_path / "a.flow.zip"
    enc = U.IndexedRefEncoder(1024)
    _write(path, enc, index=True)
    _check_reads(path)
    records = R.zip_records(path.read_bytes())
    assert not records["zip64_end"] and records["entries"] == 1 + len(_arrays())
    with zipfile.ZipFile(path) as zf, open(path, "rb") as f:
        assert U.parse_index(zf.getinfo("meta.json").extra, zf.getinfo("meta.json").file_size) is None
        assert read_member_index(zf.getinfo("meta.json")) is None
        for i, a in enumerate(_arrays()):
            info = zf.getinfo("%09d.npy" % i)
            parsed = U.parse_index(info.extra, info.file_size)
            if i >= 3:                                     # the host's path: float16, not contiguous
                assert parsed is None and info.extra == b"" and read_member_index(info) is None
                continue
            prefix = R.npy_prefix(a)
            t = R.trace(prefix, a.tobytes(), 1024, {4: 1, 8: 16}[a.itemsize])
            sizes = [q - p for p, q in zip(t.band_offsets[:-1], t.band_offsets[1:])]
            assert parsed == (len(prefix), 1024, sizes)
            assert info.extra == U.index_field(len(prefix), 1024, sizes)
            mine = read_member_index(info)
            assert (mine[0], mine[1], list(mine[2])) == parsed
            offset, csize = member_span(f, info)
            f.seek(offset)
            stream = f.read(csize)
            assert stream == t.stream and sum(sizes) + 5 == csize
            S, bad, reason, _ = U.inflate_member(stream, sizes, 1024, info.file_size)
            assert bad is None and S == prefix + a.tobytes() and zlib.crc32(S) == info.CRC
            # the local header carries no extra field
            f.seek(info.header_offset)
            assert struct.unpack("<HH", f.read(30)[26:]) == (len(info.filename), 0)


def test_index_is_off_by_default_and_then_no_byte_differs(tmp_path, monkeypatch):
    from transflow_amd import archive
    monkeypatch.setattr(time, "localtime", lambda *a: time.struct_time((2024, 5, 6, 7, 8, 10, 0, 127, 0)))
    _write(tmp_path / "plain.flow.zip", R.RefEncoder(1024))
    _write(tmp_path / "off.flow.zip", U.IndexedRefEncoder(1024))
    _write(tmp_path / "false.flow.zip", U.IndexedRefEncoder(1024), index=False)
    _write(tmp_path / "no_sizes.flow.zip", R.RefEncoder(1024), index=True)      # an encoder without last_band_sizes
    _write(tmp_path / "on.flow.zip", U.IndexedRefEncoder(1024), index=True)
    plain = (tmp_path / "plain.flow.zip").read_bytes()
    for other in ("off", "false", "no_sizes"):
        assert (tmp_path / (other + ".flow.zip")).read_bytes() == plain
    on = (tmp_path / "on.flow.zip").read_bytes()
    assert on != plain and on[:on.find(b"PK\x01\x02")] == plain[:plain.find(b"PK\x01\x02")]     # up to the directory
    assert archive.INDEX_ID == U.INDEX_ID == 0x4654


def test_an_index_that_would_not_fit_is_left_out(tmp_path):
    from transflow_amd.archive import DeviceFlowArchiveWriter, read_member_index
    path = tmp_path / "big.flow.zip"
    small, large = R.flow_field(24, 40, 33), R.flow_field(512, 512, 34)       # 122 and 32770 bands of 64 bytes
    with DeviceFlowArchiveWriter(str(path), encoder=U.StoredEncoder(64), index=True) as w:
        w.write_meta(dict(META, width=512, height=512))
        w.write_array(small)
        w.write_array(large)
    with zipfile.ZipFile(path) as zf:
        assert zf.testzip() is None
        a, b = zf.getinfo("%09d.npy" % 0), zf.getinfo("%09d.npy" % 1)
        assert len(a.extra) == 4 + 8 + 4 * 122 and read_member_index(a) is not None
        assert 4 + 8 + 4 * -(-b.file_size // 64) > 65535 and b.extra == b"" and read_member_index(b) is None
        assert np.load(io.BytesIO(zf.read(b.filename))).tobytes() == large.tobytes()
        assert np.load(io.BytesIO(zf.read(a.filename))).tobytes() == small.tobytes()


def test_zip64_field_comes_first(tmp_path, monkeypatch):
    from transflow_amd import archive
    monkeypatch.setattr(archive, "ZIP64_LIMIT", 3000)
    monkeypatch.setattr(archive, "ZIP64_COUNT_LIMIT", 4)
    path = tmp_path / "b.flow.zip"
    _write(path, U.IndexedRefEncoder(1024), index=True)
    _check_reads(path)
    data = path.read_bytes()
    records = R.zip_records(data)
    assert records["zip64_end"] and all(m[6] for m in records["members"][2:])
    with zipfile.ZipFile(path) as zf:
        for i in range(3):
            info = zf.getinfo("%09d.npy" % i)
            # zipfile strips the ZIP64 field it has used from `extra`: read the entry's own bytes
            at = data.find(b"PK\x01\x02" + b"\x2d\x00\x2d\x00", 0)
            entries = []
            while at >= 0:
                n_name, n_extra = struct.unpack("<HH", data[at + 28:at + 32])
                entries.append((data[at + 46:at + 46 + n_name].decode(), data[at + 46 + n_name:at + 46 + n_name + n_extra]))
                at = data.find(b"PK\x01\x02" + b"\x2d\x00\x2d\x00", at + 46)
            extra = dict(entries)[info.filename]
            tag, size = struct.unpack("<HH", extra[:4])
            assert tag == 1 and struct.unpack("<HH", extra[4 + size:8 + size])[0] == U.INDEX_ID
            assert U.parse_index(extra, info.file_size) is not None
            assert archive.read_member_index(info) is not None


def test_parse_index_refuses_what_it_must():
    from transflow_amd.archive import read_member_index
    sizes = [10, 20, 30]
    good = U.index_field(128, 64, sizes)
    info = zipfile.ZipInfo("x.npy")
    info.file_size = 150

    def both(extra, usize=150):
        info.extra, info.file_size = extra, usize
        mine = read_member_index(info)
        theirs = U.parse_index(extra, usize)
        assert (mine is None) == (theirs is None)
        return theirs

    assert both(good) == (128, 64, sizes)
    assert both(struct.pack("<HH", 0x7075, 3) + b"abc" + good) == (128, 64, sizes)        # behind another field
    assert both(b"") is None
    assert both(good, 200) is None and both(good, 128) is None                             # another band count
    assert both(good[:4] + b"\x02" + good[5:]) is None                                      # another version
    assert both(good[:-4]) is None                                                          # cut short


def _source_flows(path, **kwargs):
    from transflow_amd.archive import ArchiveFlowSource, read_archive_frame
    builder = ArchiveFlowSource.Builder(str(path), **kwargs)
    builder.build()
    try:
        return [read_archive_frame(builder.archive, i) for i in range(builder.base_length)]
    finally:
        builder.archive.close()


def test_host_archive_source_reads_an_indexed_archive(tmp_path):
    """The source itself, not only its archive: next() is the host's read and needs no device."""
    from transflow_amd.archive import ArchiveFlowSource
    path = tmp_path / "d.flow.zip"
    _write(path, U.IndexedRefEncoder(512), index=True)
    for got, want in zip(_source_flows(path), _arrays()):
        assert got.dtype == want.dtype and got.tobytes() == np.ascontiguousarray(want).tobytes()
    builder = ArchiveFlowSource.Builder(str(path))
    builder.build()
    source = builder.cls(*builder.args(), **builder.kwargs())
    try:
        source.validate()
        assert source.device_inflate is False
        for want in _arrays():
            got = source.next()
            source.input_frame_index += 1
            assert got.dtype == want.dtype and got.shape == want.shape
            assert got.tobytes() == np.ascontiguousarray(want).tobytes()
        with pytest.raises(KeyError):
            source.next()
    finally:
        source.archive.close()
    builder = ArchiveFlowSource.Builder(str(path), device_inflate=True, device_flows=True)
    assert builder.kwargs()["device_inflate"] is True and builder.kwargs()["device_flows"] is True
    assert ArchiveFlowSource.Builder(str(path)).kwargs()["device_inflate"] is False


def _source_over(path, **kwargs):
    from transflow_amd.archive import ArchiveFlowSource
    builder = ArchiveFlowSource.Builder(str(path), **kwargs)
    builder.build()
    return builder.cls(*builder.args(), **builder.kwargs())


def test_source_takes_only_indexes_the_device_may_be_given(tmp_path):
    """An index is untrusted.  One whose band size the decoder does not take (no multiple of 64, above the source's
    limit), or whose bands are larger than any sensible coder makes them, is not an index the source uses: the member
    goes the host's way, where zlib reads it.  (Nothing here touches a device.)"""
    from transflow_amd import archive
    path = tmp_path / "f.flow.zip"
    flow = R.flow_field(24, 40, 35)
    with archive.DeviceFlowArchiveWriter(str(path), encoder=U.IndexedRefEncoder(1024), index=True) as w:
        w.write_meta(META)
        w.write_array(flow)
    with zipfile.ZipFile(path) as zf:
        prefix_len, band_bytes, sizes = archive.read_member_index(zf.getinfo("%09d.npy" % 0))
    sizes = [int(v) for v in sizes]

    class Lying(U.IndexedRefEncoder):
        """The restatement's stream under an index that says something else."""

        def __init__(self, says_band_bytes, says_sizes):
            U.IndexedRefEncoder.__init__(self, 1024)
            self._says = (says_band_bytes, says_sizes)

        def encode_host(self, *args):
            out = U.IndexedRefEncoder.encode_host(self, *args)
            self.band_bytes = self._says[0]
            return out

        def last_band_sizes(self):
            return list(self._says[1])

    def verdict(says_band_bytes, says_sizes):
        other = tmp_path / "g.flow.zip"
        with archive.DeviceFlowArchiveWriter(str(other), replace=True, encoder=Lying(says_band_bytes, says_sizes), index=True) as w:
            w.write_meta(META)
            w.write_array(flow)
        source = _source_over(other, device_inflate=True)
        try:
            info = source.archive.getinfo("%09d.npy" % 0)
            assert archive.read_member_index(info) is not None             # the field itself is well formed
            got = source._indexed(info)
            assert source.next().tobytes() == flow.tobytes()               # the host reads the member either way
            return got
        finally:
            source.archive.close()

    taken = verdict(1024, sizes)
    assert taken is not None and taken[:2] == (prefix_len, 1024) and list(taken[2]) == sizes
    assert 128 + flow.nbytes == 7808 and -(-7808 // 1000) == len(sizes)       # the same count: the field's length agrees
    assert verdict(1000, sizes) is None                                        # no multiple of 64
    assert verdict(1024, [sizes[0], 2 * 1024 + 1025] + sizes[2:]) is None      # a band of more than twice its bytes and 1024
    assert verdict(1024, [sizes[0], 2 * 1024 + 1024] + sizes[2:]) is not None
    assert archive.MAX_DEVICE_BAND_BYTES == 1 << 20
    assert verdict(2 * archive.MAX_DEVICE_BAND_BYTES, [sum(sizes)]) is None    # one band of 2 MiB: above the limit
    assert verdict(8192, [sum(sizes)]) is not None


def test_the_references_archive_source_reads_an_indexed_archive(tmp_path):
    ref = pytest.importorskip("transflow.flow.sources.archive")
    path = tmp_path / "e.flow.zip"
    _write(path, U.IndexedRefEncoder(512), index=True)
    builder = ref.ArchiveFlowSource.Builder(str(path))
    builder.build()
    try:
        assert (builder.width, builder.height, builder.framerate) == (40, 24, 25.0)
        for i, want in enumerate(_arrays()):
            got = np.load(io.BytesIO(builder.archive.read("%09d.npy" % i)))
            assert got.tobytes() == np.ascontiguousarray(want).tobytes()
    finally:
        builder.archive.close()
