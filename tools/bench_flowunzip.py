#!/usr/bin/env python3
"""What replaying an exported flow costs up to the flow being in device memory, ready for post_process: the host's inflate
and upload against the device inflater, at 4K and 1080p, on a float32 Farnebäck flow of the
bench's clip and on its rounded form (int64), exported indexed at the default band.

  (a) the host's path, as ArchiveFlowSource.next() and post_process_host_ex do it: read_archive_frame (zipfile.read,
      numpy.load; one CPU thread inflates the member) and the upload of the array (the rounded form's astype(float32)
      first, as post_process does): host clock, each part apart.
  (b) the resident replay, as ArchiveFlowSource(device_inflate=True) does it (the file read into the decoder's page-locked
      buffer, FlowUnzipDecoder.decode_device into the flow's place, the rounded form's i64_to_f32_dev): host clock around
      the whole; and its parts apart -- the file read into the page-locked buffer (host clock), the upload of the compressed bytes
      (a copy of that size from page-locked memory, host clock around copy and wait), the kernels from the library's own
      event profiler in a pass of their own.
  check the flow in flow_ptr(0) is the member's array (as float32), bit for bit.

    python tools/bench_flowunzip.py [--out profiles/flowunzip_bench.json] [--csv profiles/flowunzip_kernel_stats.csv]

Prints one JSON object (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from bench_flowzip import clip_flow  # noqa: E402
from bench_jpeg import spread  # noqa: E402
from transflow_amd import _lib  # noqa: E402
from transflow_amd.archive import DeviceFlowArchiveWriter, member_span, read_archive_frame, read_member_index  # noqa: E402
from transflow_amd.device import DevBuffer, sync  # noqa: E402
from transflow_amd.flowunzip import FlowUnzipDecoder, i64_to_f32_dev  # noqa: E402
from transflow_amd.flowzip import default_band_bytes, npy_prefix  # noqa: E402

SIZES = {"4k": (2160, 3840), "1080p": (1080, 1920)}
KERNELS = ("fu_inflate", "fu_crc", "fu_finish", "fu_i64_f32")


def write_archive(path, array, h, w):
    with DeviceFlowArchiveWriter(path, True, index=True) as writer:
        writer.write_meta({"path": "clip", "width": w, "height": h, "framerate": 25.0, "direction": 1, "seek_time": None})
        writer.write_array(array)


def host_path(path, reps):
    inflate, convert, upload = [], [], []
    with zipfile.ZipFile(path) as zf:
        first = read_archive_frame(zf, 0)
        dev = DevBuffer(first.size * 4)
        for _ in range(reps):
            t0 = time.perf_counter()
            array = read_archive_frame(zf, 0)
            t1 = time.perf_counter()
            flow = array if array.dtype == np.float32 else array.astype(np.float32)
            t2 = time.perf_counter()
            dev.upload(flow)
            sync()
            t3 = time.perf_counter()
            inflate.append((t1 - t0) * 1e3), convert.append((t2 - t1) * 1e3), upload.append((t3 - t2) * 1e3)
        dev.close()
    parts = {"read_archive_frame_ms": spread(inflate), "astype_float32_ms": spread(convert), "upload_ms": spread(upload)}
    parts["per_frame_ms"] = {"median_ms": sum(v["median_ms"] for v in parts.values()), "note": "the medians added"}
    return parts


def device_path(path, want, reps):
    """What ArchiveFlowSource(device_inflate=True) does for an indexed member, through the same public pieces: the band
    index and the member's place in the file (archive.read_member_index, member_span), the read into the decoder's
    page-locked buffer, FlowUnzipDecoder.decode_device and, for an int64 member, i64_to_f32_dev."""
    dtype = want.dtype
    prefix = npy_prefix(want.shape, dtype)
    decoder = FlowUnzipDecoder()
    flow = DevBuffer(want.size * 4)                                  # where post_process would find the flow
    wide = DevBuffer(want.size * 8) if dtype == np.int64 else None
    with zipfile.ZipFile(path) as zf, open(path, "rb") as file:
        info = zf.getinfo("%09d.npy" % 0)
        prefix_len, band_bytes, sizes = read_member_index(info)
        offset, csize = member_span(file, info)
        assert prefix_len == len(prefix) and int(sizes.sum()) + 5 == csize

        def read():
            staged = decoder.staging(csize)
            file.seek(offset)
            assert file.readinto(memoryview(staged)) == csize
            return staged

        def inflate(staged):
            head, crc = decoder.decode_device(staged, sizes, band_bytes, info.file_size, prefix_len, wide.ptr if wide else flow.ptr)
            assert head == prefix and crc == info.CRC
            if wide:
                i64_to_f32_dev(wide.ptr, want.size, flow.ptr)

        inflate(read())                                              # makes the handle; not timed
        sync()
        got = flow.download(want.shape, np.float32)
        whole, reads, up = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            inflate(read())
            sync()
            whole.append((time.perf_counter() - t0) * 1e3)
        scratch = DevBuffer(csize)
        for _ in range(reps):
            t0 = time.perf_counter()
            staged = read()
            t1 = time.perf_counter()
            _lib.check(_lib.load().tf_dev_upload(C.c_void_p(scratch.ptr), C.c_void_p(staged.ctypes.data), csize))
            sync()
            t2 = time.perf_counter()
            reads.append((t1 - t0) * 1e3), up.append((t2 - t1) * 1e3)
        scratch.close()
        staged = read()
        _lib.profile(True, "fu_")
        for _ in range(reps):
            inflate(staged)
        sync()
        report = _lib.profile_report()
        _lib.profile(False)
    decoder.close()
    kernels = {k: {"launches": report[k][0], "ms_per_launch": report[k][1] / report[k][0]} for k in KERNELS if k in report}
    return {"band_bytes": int(band_bytes), "bands": int(len(sizes)), "member_bytes": int(csize), "raw_bytes": int(info.file_size),
            "per_frame_ms": spread(whole), "file_read_ms": spread(reads), "upload_compressed_ms": spread(up), "kernels": kernels,
            "kernels_ms": sum(v["ms_per_launch"] for v in kernels.values()),
            "flow_is_the_members": bool(got.tobytes() == want.astype(np.float32).tobytes())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--csv")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sizes", default="4k,1080p")
    args = ap.parse_args()
    result = {"tool": "bench_flowunzip", "host": bench.host_description(), "default_band_bytes": default_band_bytes(), "sizes": {}}
    rows = []
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:    # no disk in the timings
        for name in args.sizes.split(","):
            h, w = SIZES[name]
            flow = clip_flow(h, w)
            entry = {"height": h, "width": w}
            for form, array in (("float32", flow), ("rounded_int64", np.round(flow).astype(int))):
                path = os.path.join(tmp, f"{name}_{form}.flow.zip")
                write_archive(path, array, h, w)
                with zipfile.ZipFile(path) as zf:
                    assert read_member_index(zf.getinfo("%09d.npy" % 0)) is not None
                run = {"device": device_path(path, array, args.reps), "host": host_path(path, args.host_reps)}
                run["host_over_device"] = run["host"]["per_frame_ms"]["median_ms"] / run["device"]["per_frame_ms"]["median_ms"]
                entry[form] = run
                for k, v in run["device"]["kernels"].items():
                    rows.append((name, form, k, v["launches"], v["ms_per_launch"]))
                os.unlink(path)
            result["sizes"][name] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.csv:
        with open(args.csv, "w") as f:
            f.write("size,form,kernel,launches,ms_per_launch\n")
            for row in rows:
                f.write("%s,%s,%s,%d,%.6f\n" % row)


if __name__ == "__main__":
    main()
