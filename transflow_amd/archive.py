"""`.flow.zip` flow archives -- the on-disk flow format either side of the path.

The format, as the reference's files lay it out (written by transflow/output/zip.py:6-28 and
output/numpy.py:6-14 from pipeline.py:363-377, 505-506; read by flow/sources/archive.py:10-51): a
deflated zip with one member `meta.json` ({"path", "width", "height", "framerate", "direction",
"seek_time"}) followed by one `.npy` member per frame named by its nine-digit index.  This module is
an independent reader / writer of that layout: `FlowArchiveWriter`, `read_archive_meta`,
`read_archive_frame`, and `ArchiveFlowSource`, whose frames go through FlowSource.post_process on the
GPU like any other flow.  tests/test_host_mirror.py checks that archives written here are
byte-identical to the reference's and that each implementation reads the other's.
"""
from __future__ import annotations

import io
import json
import os
import re
import struct
import time
import zipfile
import zlib

import numpy as np

from .flow import FlowSource

META_MEMBER = "meta.json"


def frame_member(index: int) -> str:
    return "%09d.npy" % index


def unique_path(path: str) -> str:
    """`path` if nothing is there yet, otherwise the first free `<stem>.NNN<ext>`; a `.flow` / `.map`
    before the extension belongs to the extension (`a.flow.zip` -> `a.000.flow.zip`), and a stem that
    already ends in a counter continues from it (utils.find_unique_path's naming, utils.py:147-160)."""
    if not os.path.isfile(path):
        return path
    stem, ext = os.path.splitext(path)
    for tag in (".flow", ".map"):
        if stem.endswith(tag):
            stem, ext = stem[:-len(tag)], tag + ext
            break
    counter = re.search(r"\.(\d{3})$", stem)
    n = 0
    if counter:
        stem, n = stem[:counter.start()], int(counter.group(1)) + 1
    while True:
        candidate = f"{stem}.{n:03d}{ext}"
        if not os.path.isfile(candidate):
            return candidate
        n += 1


def flow_export_meta(flow_path, width: int, height: int, framerate, direction, seek_time=None) -> dict:
    """The six fields pipeline.py:370-377 stores with an exported flow."""
    return dict(path=flow_path, width=width, height=height, framerate=framerate,
                direction=FlowSource.Direction.from_arg(direction).value, seek_time=seek_time)


class FlowArchiveWriter:
    """Appends frames to a new archive.  `replace=False` never overwrites: it picks `unique_path(path)`."""

    def __init__(self, path: str, replace: bool = False):
        self.path = path if replace else unique_path(path)
        self._zip = zipfile.ZipFile(self.path, mode="w", compression=zipfile.ZIP_DEFLATED)
        self.index = 0

    def _put(self, member: str, payload: bytes) -> None:
        with self._zip.open(member, mode="w") as f:
            f.write(payload)

    def write_meta(self, meta: dict) -> None:
        if meta:
            self._put(META_MEMBER, json.dumps(meta).encode())

    def write_array(self, array: np.ndarray) -> None:
        buf = io.BytesIO()
        np.save(buf, array)
        self._put(frame_member(self.index), buf.getvalue())
        self.index += 1

    def close(self) -> None:
        self._zip.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


NumpyOutput = FlowArchiveWriter      # the name the reference's pipeline uses for this role (output/numpy.py)


# A size or an offset at or above ZIP64_LIMIT, or an entry count at or above ZIP64_COUNT_LIMIT, is written in the ZIP64
# records (the values the format itself sets; a test lowers them to see those records written on a small archive).
ZIP64_LIMIT = 0xFFFFFFFF
ZIP64_COUNT_LIMIT = 0xFFFF


def _deflate(payload: bytes) -> bytes:
    """A raw deflate stream at zlib's default level: what zipfile writes into a ZIP_DEFLATED member."""
    c = zlib.compressobj(zlib.Z_DEFAULT_COMPRESSION, zlib.DEFLATED, -15)
    return c.compress(payload) + c.flush()


# ---- the band index: an extra field of a member's central-directory entry ------------------------
# header ID 0x4654, then `<BBHI`: version 1, flags 0, prefix_len (the `.npy` header's bytes), band_bytes; then one `<I` per
# band, ceil(usize / band_bytes) of them: the band's compressed bytes.  What follows the last band in the member is the
# final block 01 00 00 FF FF; it is not indexed.
INDEX_ID = 0x4654
INDEX_VERSION = 1
# What the source gives the device (an archive is untrusted, and the decoder rebuilds its tables for every block, however
# little the block holds -- DESIGN.md section 18, Bounds): bands of at most this many bytes, whose compressed bytes are at
# most twice their own and 1024 more.  Every coder's bands are far inside that; any other member is read by the host.
MAX_DEVICE_BAND_BYTES = 1 << 20


def index_field(prefix_len: int, band_bytes: int, sizes) -> bytes:
    payload = struct.pack("<BBHI", INDEX_VERSION, 0, prefix_len, band_bytes) + struct.pack("<%dI" % len(sizes), *sizes)
    return struct.pack("<HH", INDEX_ID, len(payload)) + payload


def read_member_index(info: zipfile.ZipInfo):
    """(prefix_len, band_bytes, the bands' compressed sizes as a uint32 array) from the member's band index; None if it
    has none, if the version is not 1, or if the field's length disagrees with ceil(file_size / band_bytes)."""
    extra = info.extra
    at = 0
    while at + 4 <= len(extra):
        tag, size = struct.unpack_from("<HH", extra, at)
        body = extra[at + 4:at + 4 + size]
        at += 4 + size
        if tag != INDEX_ID:
            continue
        if len(body) < 8 or len(body) != size:
            return None
        version, _flags, prefix_len, band_bytes = struct.unpack_from("<BBHI", body)
        if version != INDEX_VERSION or band_bytes == 0 or len(body) != 8 + 4 * -(-info.file_size // band_bytes):
            return None
        return prefix_len, band_bytes, np.frombuffer(body, np.uint32, offset=8)
    return None


def member_span(file, info: zipfile.ZipInfo):
    """(offset, bytes) of the member's compressed bytes in `file`, by its local header."""
    file.seek(info.header_offset)
    header = file.read(30)
    if len(header) != 30 or header[:4] != b"PK\x03\x04":
        raise zipfile.BadZipFile(f"Bad magic number for file header of {info.filename!r}")
    n_name, n_extra = struct.unpack_from("<HH", header, 26)
    return info.header_offset + 30 + n_name + n_extra, info.compress_size


class DeviceFlowArchiveWriter:
    """FlowArchiveWriter's surface over members that are deflated on the device (transflow_amd/flowzip.py, DESIGN.md
    section 17): the same layout -- `meta.json`, then one `.npy` member per frame -- and the same arrays back from
    `numpy.load`, but not the same compressed bytes.  `zipfile` cannot take a member that is deflated already, so the
    records are written here: a local header and the member's stream per entry, the central directory and the end
    record on close(), the ZIP64 records once an offset, a size or the entry count needs them.

    write_array(a):
      * a DeviceFlow whose device copy is current is encoded where it is -- it never comes down (`flow._host` stays
        None) -- and so is the device int64 array `numpy.round(flow).astype(int)` is under deviceflow.DEVICE_ROUND;
      * a C-contiguous float32 / float64 / int64 ndarray is uploaded and encoded on the device;
      * anything else is written as FlowArchiveWriter writes it: numpy.save, zlib on the host.
    write_array(flow, rounded=True) rounds on the device first (numpy.round(flow).astype(int)).
    `encoder`: the object that makes the streams (flowzip.FlowZipEncoder by default, made on first use).
    `index`: every member the encoder makes gets a band index -- the compressed size of each of its bands, in an extra
    field (header ID 0x4654) of its central-directory entry, from the encoder's `last_band_sizes()` -- with which
    `ArchiveFlowSource(device_inflate=True)` inflates the bands side by side on the device.
    Readers that do not know the field skip it; without `index` not a byte differs from what was written before."""

    def __init__(self, path: str, replace: bool = False, encoder=None, band_bytes: int | None = None, index: bool = False):
        self.path = path if replace else unique_path(path)
        self._file = open(self.path, "wb")
        self._encoder, self._band_bytes = encoder, band_bytes
        self._index = bool(index)
        self._entries = []          # (name, time, date, crc, csize, usize, offset, the band index's extra field)
        self._at = 0
        self.index = 0

    # ---- the records
    def _put(self, member: str, stream: bytes, crc: int, usize: int, index: bytes = b"") -> None:
        name = member.encode()
        t = time.localtime()
        dos_time, dos_date = t[3] << 11 | t[4] << 5 | t[5] // 2, (max(t[0], 1980) - 1980) << 9 | t[1] << 5 | t[2]
        csize, offset = len(stream), self._at
        big = csize >= ZIP64_LIMIT or usize >= ZIP64_LIMIT
        extra = struct.pack("<HHQQ", 1, 16, usize, csize) if big else b""
        self._file.write(struct.pack("<IHHHHHIIIHH", 0x04034B50, 45 if big else 20, 0, 8, dos_time, dos_date, crc,
                                     0xFFFFFFFF if big else csize, 0xFFFFFFFF if big else usize, len(name), len(extra)))
        self._file.write(name + extra)
        self._file.write(stream)
        self._at += 30 + len(name) + len(extra) + csize
        self._entries.append((name, dos_time, dos_date, crc, csize, usize, offset, index))

    def _put_host(self, member: str, payload: bytes) -> None:
        self._put(member, _deflate(payload), zlib.crc32(payload), len(payload))

    def _end(self) -> None:
        cd_offset = self._at
        for name, dos_time, dos_date, crc, csize, usize, offset, index in self._entries:
            # the fields that do not fit their 32 bits go into the ZIP64 extra field, in this order
            wide = [v for v in (usize, csize, offset) if v >= ZIP64_LIMIT]
            usize, csize, offset = (0xFFFFFFFF if v >= ZIP64_LIMIT else v for v in (usize, csize, offset))
            extra = struct.pack("<HH%dQ" % len(wide), 1, 8 * len(wide), *wide) if wide else b""
            if len(extra) + len(index) <= 0xFFFF:      # the ZIP64 field first; an index that does not fit is left out
                extra += index
            version = 45 if wide else 20
            record = struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, version, version, 0, 8, dos_time, dos_date, crc, csize, usize,
                                 len(name), len(extra), 0, 0, 0, 0o600 << 16, offset)
            self._file.write(record + name + extra)
            self._at += len(record) + len(name) + len(extra)
        cd_size, n = self._at - cd_offset, len(self._entries)
        if n >= ZIP64_COUNT_LIMIT or cd_offset >= ZIP64_LIMIT or cd_size >= ZIP64_LIMIT:
            self._file.write(struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 45, 45, 0, 0, n, n, cd_size, cd_offset))
            self._file.write(struct.pack("<IIQI", 0x07064B50, 0, self._at, 1))
            n = 0xFFFF if n >= ZIP64_COUNT_LIMIT else n
            cd_size = 0xFFFFFFFF if cd_size >= ZIP64_LIMIT else cd_size
            cd_offset = 0xFFFFFFFF if cd_offset >= ZIP64_LIMIT else cd_offset
        self._file.write(struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, n, n, cd_size, cd_offset, 0))

    # ---- FlowArchiveWriter's surface
    def write_meta(self, meta: dict) -> None:
        if meta:
            self._put_host(META_MEMBER, json.dumps(meta).encode())

    def _get_encoder(self):
        if self._encoder is None:
            from .flowzip import FlowZipEncoder
            self._encoder = FlowZipEncoder(self._band_bytes, views=True)
        return self._encoder

    def _index_field(self, prefix: bytes) -> bytes:
        """The band index of the member the encoder has just made, or nothing."""
        encoder = self._encoder
        if not self._index or not hasattr(encoder, "last_band_sizes"):
            return b""
        sizes = encoder.last_band_sizes()
        if 4 + 8 + 4 * len(sizes) > 0xFFFF:            # an entry's extra fields have 65535 bytes: this member has no index
            return b""
        return index_field(len(prefix), int(encoder.band_bytes), sizes)

    def write_array(self, array, rounded: bool = False) -> None:
        from .deviceflow import DeviceFlow
        from .flowzip import DISTANCES, DeviceInt64Flow, npy_prefix, round_i64_dev
        member = frame_member(self.index)
        if rounded:
            if isinstance(array, DeviceFlow) and not array.on_host and array.dtype == np.float32:
                array = round_i64_dev(array)      # (a float64 flow comes down: numpy's own round, as DEVICE_ROUND does)
            else:
                array = np.round(array).astype(int)
        if isinstance(array, (DeviceFlow, DeviceInt64Flow)) and not array.on_host:
            prefix = npy_prefix(array.shape, array.dtype)
            array.wait_on_stream()
            stream, crc = self._get_encoder().encode_device(prefix, array.dev_ptr, array.nbytes, DISTANCES[array.dtype])
            if isinstance(array, DeviceFlow):
                array.mark_used()           # (the encoder has waited for its kernels; the ring's next writer need not)
            self._put(member, stream, crc, len(prefix) + array.nbytes, self._index_field(prefix))
        elif (isinstance(array, np.ndarray) and array.flags.c_contiguous and array.dtype in DISTANCES
              and array.dtype.isnative and array.ndim >= 1):
            prefix = npy_prefix(array.shape, array.dtype)
            stream, crc = self._get_encoder().encode_host(prefix, array, DISTANCES[array.dtype])
            self._put(member, stream, crc, len(prefix) + array.nbytes, self._index_field(prefix))
        else:
            buf = io.BytesIO()
            np.save(buf, array)
            self._put_host(member, buf.getvalue())
        self.index += 1

    def close(self) -> None:
        if self._file is not None:
            self._end()
            self._file.close()
            self._file = None
        if self._encoder is not None and hasattr(self._encoder, "close"):
            self._encoder.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_archive_meta(zf: zipfile.ZipFile) -> dict:
    return json.loads(zf.read(META_MEMBER).decode())


def read_archive_frame(zf: zipfile.ZipFile, index: int) -> np.ndarray:
    """Frame `index`; a missing member is zipfile's KeyError -- that is how an archive ends."""
    return np.load(io.BytesIO(zf.read(frame_member(index))))


class ArchiveFlowSource(FlowSource):
    """Flows replayed from an archive.  Like the reference's (archive.py:22-31) its builder takes
    geometry, frame rate and direction from meta.json and does no timing arithmetic at all: no seek,
    duration or repeat for archives, `length` stays None, and iteration ends with the KeyError of the
    first missing frame (which the pipeline's source process logs and stops on, pipeline.py:90-97)."""

    class Builder(FlowSource.Builder):
        def __init__(self, path: str, device_inflate: bool = False, device_flows=False, device: int | None = None, **kwargs):
            FlowSource.Builder.__init__(self, **kwargs)
            self.path, self.archive = path, None
            self.device_inflate, self.device_flows, self.device = device_inflate, device_flows, device

        cls = property(lambda self: ArchiveFlowSource)

        def build(self):
            self.archive = zipfile.ZipFile(self.path)
            meta = read_archive_meta(self.archive)
            self.width, self.height, self.framerate = meta["width"], meta["height"], meta["framerate"]
            # archives from before the field existed hold forward flows (archive.py:26-27)
            self.direction = FlowSource.Direction(meta.get("direction", FlowSource.Direction.FORWARD.value))
            self.base_length = len(self.archive.namelist()) - 1

        def args(self):
            return [self.archive] + FlowSource.Builder.args(self)

        def kwargs(self):
            kw = FlowSource.Builder.kwargs(self)
            kw.update(device_inflate=self.device_inflate, device_flows=self.device_flows, device=self.device)
            return kw

    def __init__(self, archive: zipfile.ZipFile, *args, device_inflate: bool = False, device_flows=False,
                 device: int | None = None, **kwargs):
        """device_inflate: members that carry a band index (DeviceFlowArchiveWriter(index=True)) and hold a float32 or
        int64 (H, W, 2) array are read from the file into page-locked memory, inflated on the device straight into the
        post-processing handle's flow (transflow_amd/flowunzip.py) and post-processed there, where
        the resident tail applies (FlowSource._resident_ok); only the final flow comes down, or none with `device_flows`
        (True or "ipc": the source yields DeviceFlows, as MotionVectorFlowSource does).  The `.npy` header and the CRC-32
        are checked: a member the device rejects, or whose CRC differs, raises zipfile.BadZipFile.  Every other member --
        no index, another dtype or shape -- goes the host's way as before.
        A rounded (int64) member comes out of the resident path as the float32 flow `member.astype(numpy.float32)`
        post-processed like any flow (exact for every vector a frame can hold); the host path keeps returning the
        integer array the reference returns."""
        self.archive = archive
        self.device_inflate, self.device_flows, self.device = bool(device_inflate), device_flows, device
        self._unzip = self._i64 = None
        FlowSource.__init__(self, *args, **kwargs)

    def validate(self):
        FlowSource.validate(self)
        if not isinstance(self.archive, zipfile.ZipFile):
            raise ValueError(f"Attribute archive has incorrect type {type(self.archive)}")

    def next(self):
        return read_archive_frame(self.archive, self.input_frame_index)

    # ---- resident form of one iteration (FlowSource's resident tail): an indexed member never exists on the host
    def _indexed(self, info: zipfile.ZipInfo):
        """(prefix_len, band_bytes, sizes, dtype) if the member is one the device inflates, else None."""
        if info.compress_type != zipfile.ZIP_DEFLATED or info.flag_bits & 1:
            return None
        index = read_member_index(info)
        if index is None:
            return None
        band_bytes, sizes = index[1], index[2]
        if band_bytes % 64 or band_bytes > MAX_DEVICE_BAND_BYTES or int(sizes.max()) > 2 * band_bytes + 1024:
            return None
        from .flowzip import npy_prefix
        shape = (self.height, self.width, 2)
        for dtype in (np.float32, np.int64):
            prefix = npy_prefix(shape, dtype)
            n = len(prefix) + int(np.prod(shape)) * np.dtype(dtype).itemsize
            if index[0] == len(prefix) and info.file_size == n and len(prefix) % 64 == 0 and len(prefix) <= 4096:
                return (*index, np.dtype(dtype))
        return None

    def _inflate_resident(self, info: zipfile.ZipInfo, index) -> None:
        """The member's array into _post_handle().flow_ptr(0), as float32."""
        from .flowunzip import BandRejected, FlowUnzipDecoder, i64_to_f32_dev
        from .flowzip import npy_prefix
        prefix_len, band_bytes, sizes, dtype = index
        if self._unzip is None:
            self._unzip = FlowUnzipDecoder()
        file = self.archive.fp
        offset, csize = member_span(file, info)
        staged = self._unzip.staging(csize)
        file.seek(offset)
        if file.readinto(memoryview(staged)) != csize:
            raise zipfile.BadZipFile(f"{info.filename}: the archive ends inside the member")
        used = int(sizes.sum(dtype=np.uint64))
        tail = bytes(staged[used:]) if used <= csize else None
        d = zlib.decompressobj(-15)
        try:
            tail_ok = tail is not None and d.decompress(tail) == b"" and d.eof and not d.unused_data
        except zlib.error:
            tail_ok = False
        if not tail_ok:
            raise zipfile.BadZipFile(f"{info.filename}: the band index does not fit the member's stream")
        n_values = self.height * self.width * 2
        target = self._post_handle().flow_ptr(0)
        if dtype == np.int64:
            if self._i64 is None:
                from .device import DevBuffer
                self._i64 = DevBuffer(n_values * 8)
            target = self._i64.ptr
        try:
            head, crc = self._unzip.decode_device(staged, sizes, band_bytes, info.file_size, prefix_len, target)
        except BandRejected as e:
            raise zipfile.BadZipFile(f"{info.filename}: band {e.band} is no valid deflate band") from e
        if head != npy_prefix((self.height, self.width, 2), dtype):
            raise zipfile.BadZipFile(f"{info.filename}: not the header of a {dtype} array of {self.height} x {self.width} x 2")
        if crc != info.CRC:
            raise zipfile.BadZipFile(f"Bad CRC-32 for file {info.filename!r} (inflated on the device, all bands accepted)")
        if dtype == np.int64:
            i64_to_f32_dev(self._i64.ptr, n_values, self._post_handle().flow_ptr(0))

    def read_next_flow(self):
        if not (self.device_inflate and self._resident_ok()):
            return FlowSource.read_next_flow(self)
        if self.input_frame_index == self.end_frame:
            self.rewind()
        info = self.archive.getinfo(frame_member(self.input_frame_index))     # KeyError: that is how an archive ends
        index = self._indexed(info)
        if index is None:
            return FlowSource.read_next_flow(self)
        self._inflate_resident(info, index)
        self.input_frame_index += 1
        return self._take_output(self.device_flows, 4)

    def _resident_flow(self):
        return self._pp, 0

    def _download(self, pp, pair, out):
        import ctypes as C

        from . import _lib
        _lib.check(_lib.load().tf_dev_download(C.c_void_p(out.ctypes.data), C.c_void_p(pp.flow_ptr(pair)), out.nbytes))

    def close(self):
        self.archive.close()
        if self._unzip is not None:
            self._unzip.close()
            self._unzip = None
        if self._i64 is not None:
            self._i64.close()
            self._i64 = None
        FlowSource.close(self)
