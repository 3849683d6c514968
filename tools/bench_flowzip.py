#!/usr/bin/env python3
"""What an exported flow costs: the download and host deflate the flow export needs without the device coder, against
DeviceFlowArchiveWriter.write_array of a resident flow, at 4K and 1080p, on a float32 Farnebäck flow of the bench's clip
and on its rounded form (numpy.round(flow).astype(int), int64).

  time   (a) host path: tf_dev_download into a page-locked array, (for the rounded form) numpy.round(flow).astype(int),
             and FlowArchiveWriter.write_array (numpy.save + zlib level 6 on one thread): host clock, each part apart.
         (b) device path: DeviceFlowArchiveWriter.write_array(resident flow[, rounded=True]) into an archive in a
             memory-backed directory: host clock around `--reps` calls, median of `--rounds` windows; per kernel from the library's own event
             profiler, in a pass of its own.
  size   the member's bytes beside the raw `.npy` bytes and beside zlib level 6 on the same bytes (the host writer's
         member).
  bands  the encoder alone (FlowZipEncoder.encode_device) at band_bytes 8, 16, 32 and 64 KB on the 4K flows: time and size;
         and the member's bytes at the distances 1, 2, 4, 8 and 16.
  check  numpy.load returns the flow from the device-written archive, bit for bit.

    python tools/bench_flowzip.py [--out profiles/flowzip_bench.json] [--csv profiles/flowzip_kernel_stats.csv]

Prints one JSON object (and writes it to --out)."""
import argparse
import ctypes as C
import io
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
from bench_jpeg import spread  # noqa: E402
from transflow_amd import _lib  # noqa: E402
from transflow_amd.archive import DeviceFlowArchiveWriter, FlowArchiveWriter  # noqa: E402
from transflow_amd.device import DevBuffer, pinned_empty, sync  # noqa: E402
from transflow_amd.deviceflow import DeviceFlow, _Event  # noqa: E402
from transflow_amd.farneback import Farneback  # noqa: E402
from transflow_amd.flowzip import DISTANCES, FlowZipEncoder, default_band_bytes, npy_prefix, round_i64_dev  # noqa: E402

SIZES = {"4k": (2160, 3840), "1080p": (1080, 1920)}
KERNELS = ("fz_round", "fz_count", "fz_table", "fz_sizes", "fz_scan", "fz_emit")
BANDS = (8192, 16384, 32768, 65536)
DISTANCE_SWEEP = (1, 2, 4, 8, 16)


def clip_flow(h, w):
    """The flow between two frames of the bench's clip, as the flagship path computes it."""
    clip = bench.ClipSynth(h, w, 8, 0)
    fb = Farneback(w, h, device=0)
    return np.ascontiguousarray(fb.calc(clip.frame(1), clip.frame(0)), dtype=np.float32)


def device_flow(array):
    buf = DevBuffer.from_array(array)
    ev = _Event()
    ev.record()
    return DeviceFlow(array.shape, buf.ptr, ev, owner=buf)


def member_of(path, index=0):
    with zipfile.ZipFile(path) as zf:
        info = zf.getinfo("%09d.npy" % index)
        return info.compress_size, info.file_size, np.load(io.BytesIO(zf.read(info)))


def host_path(flow, rounded, reps, tmp):
    pinned = pinned_empty(flow.shape, np.float32)
    down, rnd, deflate = [], [], []
    path = os.path.join(tmp, "host.flow.zip")
    for _ in range(reps):
        t0 = time.perf_counter()
        _lib.check(_lib.load().tf_dev_download(C.c_void_p(pinned.ctypes.data), C.c_void_p(flow.dev_ptr), pinned.nbytes))
        t1 = time.perf_counter()
        array = np.round(pinned).astype(int) if rounded else pinned
        t2 = time.perf_counter()
        with FlowArchiveWriter(path, True) as w:
            w.write_array(array)
        t3 = time.perf_counter()
        down.append((t1 - t0) * 1e3), rnd.append((t2 - t1) * 1e3), deflate.append((t3 - t2) * 1e3)
    csize, usize, _ = member_of(path)
    os.unlink(path)
    return {"download_ms": spread(down), "host_round_ms": spread(rnd), "save_and_zlib6_ms": spread(deflate),
            "per_frame_ms": {"median_ms": spread(down)["median_ms"] + spread(rnd)["median_ms"] + spread(deflate)["median_ms"],
                             "note": "the medians added"},
            "member_bytes": csize, "raw_bytes": usize}


def device_path(flow, rounded, reps, rounds, tmp, want):
    """A new archive per window (each holds 1 + reps members): the first write makes the encoder's handle and is not timed."""
    path = os.path.join(tmp, "device.flow.zip")
    wall = []
    for _ in range(rounds):
        with DeviceFlowArchiveWriter(path, True) as w:
            w.write_array(flow, rounded=rounded)
            t0 = time.perf_counter()
            for _ in range(reps):
                w.write_array(flow, rounded=rounded)
            wall.append((time.perf_counter() - t0) * 1e3 / reps)
    with DeviceFlowArchiveWriter(path, True) as w:
        w.write_array(flow, rounded=rounded)
        _lib.profile(True, "fz_")
        for _ in range(reps):
            w.write_array(flow, rounded=rounded)
        sync()
        report = _lib.profile_report()
        _lib.profile(False)
        band = w._encoder.band_bytes
    csize, usize, back = member_of(path, 1)
    os.unlink(path)
    kernels = {k: {"launches": report[k][0], "ms_per_launch": report[k][1] / report[k][0]} for k in KERNELS if k in report}
    return {"band_bytes": band, "per_frame_ms": spread(wall), "kernels": kernels, "member_bytes": csize, "raw_bytes": usize,
            "numpy_loads_the_flow": bool(back.dtype == want.dtype and back.tobytes() == want.tobytes()),
            "flow_stayed_on_the_device": flow._host is None}


def band_sweep(ptr, nbytes, shape, dtype, reps):
    out = {}
    prefix = npy_prefix(shape, dtype)
    for band in BANDS:
        enc = FlowZipEncoder(band, views=True)               # the stream in the encoder's page-locked buffer, as the writer takes it
        try:
            stream, _ = enc.encode_device(prefix, ptr, nbytes, DISTANCES[np.dtype(dtype)])
            size = len(stream)
            times = []
            for _ in range(reps):
                t0 = time.perf_counter()
                enc.encode_device(prefix, ptr, nbytes, DISTANCES[np.dtype(dtype)])
                times.append((time.perf_counter() - t0) * 1e3)
            _lib.profile(True, "fz_")
            for _ in range(reps):
                enc.encode_device(prefix, ptr, nbytes, DISTANCES[np.dtype(dtype)])
            sync()
            report = _lib.profile_report()
            _lib.profile(False)
            out[str(band)] = {"encode_ms": spread(times), "member_bytes": size,
                              "kernels_ms": sum(report[k][1] / report[k][0] for k in KERNELS if k in report)}
        finally:
            enc.close()
    return out


def distance_sweep(ptr, nbytes, shape, dtype, reps):
    """The member's bytes at the default band for the distances a 4- or 8-byte element suggests."""
    out = {}
    prefix = npy_prefix(shape, dtype)
    enc = FlowZipEncoder(views=True)
    try:
        for distance in DISTANCE_SWEEP:
            stream, _ = enc.encode_device(prefix, ptr, nbytes, distance)
            out[str(distance)] = {"member_bytes": len(stream)}
    finally:
        enc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--csv")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--sizes", default="4k,1080p")
    args = ap.parse_args()
    result = {"tool": "bench_flowzip", "host": bench.host_description(), "default_band_bytes": default_band_bytes(),
              "distances": {str(k): v for k, v in DISTANCES.items()}, "sizes": {}}
    rows = []
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:    # no disk in the timings
        for name in args.sizes.split(","):
            h, w = SIZES[name]
            host_flow = clip_flow(h, w)
            flow = device_flow(host_flow)
            entry = {"height": h, "width": w}
            for form, rounded in (("float32", False), ("rounded_int64", True)):
                want = np.round(host_flow).astype(int) if rounded else host_flow
                run = {"device": device_path(flow, rounded, args.reps, args.rounds, tmp, want),
                       "host": host_path(flow, rounded, args.host_reps, tmp)}
                run["host_over_device"] = run["host"]["per_frame_ms"]["median_ms"] / run["device"]["per_frame_ms"]["median_ms"]
                run["device_over_zlib6_bytes"] = run["device"]["member_bytes"] / run["host"]["member_bytes"]
                entry[form] = run
                for k, v in run["device"]["kernels"].items():
                    rows.append((name, form, k, v["launches"], v["ms_per_launch"]))
            if name == "4k":
                rounded = round_i64_dev(flow)
                entry["band_sweep"] = {
                    "float32": band_sweep(flow.dev_ptr, flow.nbytes, flow.shape, np.float32, args.reps),
                    "rounded_int64": band_sweep(rounded.dev_ptr, rounded.nbytes, rounded.shape, np.int64, args.reps)}
                entry["distance_sweep"] = {
                    "float32": distance_sweep(flow.dev_ptr, flow.nbytes, flow.shape, np.float32, args.reps),
                    "rounded_int64": distance_sweep(rounded.dev_ptr, rounded.nbytes, rounded.shape, np.int64, args.reps)}
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
