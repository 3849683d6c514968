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
    `encoder`: the object that makes the streams (flowzip.FlowZipEncoder by default, made on first use)."""

    def __init__(self, path: str, replace: bool = False, encoder=None, band_bytes: int | None = None):
        self.path = path if replace else unique_path(path)
        self._file = open(self.path, "wb")
        self._encoder, self._band_bytes = encoder, band_bytes
        self._entries = []          # (name, time, date, crc, csize, usize, offset)
        self._at = 0
        self.index = 0

    # ---- the records
    def _put(self, member: str, stream: bytes, crc: int, usize: int) -> None:
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
        self._entries.append((name, dos_time, dos_date, crc, csize, usize, offset))

    def _put_host(self, member: str, payload: bytes) -> None:
        self._put(member, _deflate(payload), zlib.crc32(payload), len(payload))

    def _end(self) -> None:
        cd_offset = self._at
        for name, dos_time, dos_date, crc, csize, usize, offset in self._entries:
            # the fields that do not fit their 32 bits go into the ZIP64 extra field, in this order
            wide = [v for v in (usize, csize, offset) if v >= ZIP64_LIMIT]
            usize, csize, offset = (0xFFFFFFFF if v >= ZIP64_LIMIT else v for v in (usize, csize, offset))
            extra = struct.pack("<HH%dQ" % len(wide), 1, 8 * len(wide), *wide) if wide else b""
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

    def write_array(self, array, rounded: bool = False) -> None:
        from .deviceflow import DeviceFlow
        from .flowzip import DISTANCES, DeviceInt64Flow, npy_prefix, round_i64_dev
        member = frame_member(self.index)
        if rounded:
            if isinstance(array, DeviceFlow) and not array.on_host:
                array = round_i64_dev(array)
            else:
                array = np.round(array).astype(int)
        if isinstance(array, (DeviceFlow, DeviceInt64Flow)) and not array.on_host:
            prefix = npy_prefix(array.shape, array.dtype)
            array.wait_on_stream()
            stream, crc = self._get_encoder().encode_device(prefix, array.dev_ptr, array.nbytes, DISTANCES[array.dtype])
            if isinstance(array, DeviceFlow):
                array.mark_used()           # (the encoder has waited for its kernels; the ring's next writer need not)
            self._put(member, stream, crc, len(prefix) + array.nbytes)
        elif (isinstance(array, np.ndarray) and array.flags.c_contiguous and array.dtype in DISTANCES
              and array.dtype.isnative and array.ndim >= 1):
            prefix = npy_prefix(array.shape, array.dtype)
            stream, crc = self._get_encoder().encode_host(prefix, array, DISTANCES[array.dtype])
            self._put(member, stream, crc, len(prefix) + array.nbytes)
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
        def __init__(self, path: str, **kwargs):
            FlowSource.Builder.__init__(self, **kwargs)
            self.path, self.archive = path, None

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

    def __init__(self, archive: zipfile.ZipFile, *args, **kwargs):
        self.archive = archive
        FlowSource.__init__(self, *args, **kwargs)

    def validate(self):
        FlowSource.validate(self)
        if not isinstance(self.archive, zipfile.ZipFile):
            raise ValueError(f"Attribute archive has incorrect type {type(self.archive)}")

    def next(self):
        return read_archive_frame(self.archive, self.input_frame_index)

    def close(self):
        self.archive.close()
        FlowSource.close(self)
