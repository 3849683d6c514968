#!/usr/bin/env python3
"""What a compressed frame costs: the download and host encode a JPEG output needs without the device encoder, against
tf_jpeg_encode_dev, at 4K and 1080p, on a rendered frame of the bench's clip.

The frame: three frames of bench.py's ClipSynth as the pixmap's R, G, B, moved by the clip's own displacement field
through a moveref layer and painted into a compositor image -- it stays on the device, as pipeline frames do.

  (a) host path      comp.download() into a page-locked array + Pillow's libjpeg at the same quality, subsampling and
                     restart interval (the stand-in for cv2.imencode): host clock, median of `--host-reps` frames,
                     download and encode also apart.
  (b) device path    JpegEncoder.encode_into(comp): host clock around `--reps` calls (each ends in a synchronise and has
                     the file in host memory), median of `--rounds` windows; device events around the same calls; and
                     per kernel, from the library's own event profiler, in a pass of its own.

(b) is swept over restart intervals.  The library's default is the fastest interval whose file is within 2 % of the
smallest file of the sweep (restart markers are the only size cost); the tool prints which one that is.  Every file is
compared with Pillow's, byte for byte.

    python tools/bench_jpeg.py [--out profiles/jpeg_bench.json] [--csv profiles/jpeg_kernel_stats.csv]

Prints one JSON object (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from transflow_amd import _lib  # noqa: E402
from transflow_amd.device import pinned_empty, sync  # noqa: E402
from transflow_amd.jpeg import JpegEncoder, pillow_encode  # noqa: E402
from transflow_amd.remap import CompImage, RemapLayer  # noqa: E402

SIZES = {"4k": (2160, 3840), "1080p": (1080, 1920)}
KERNELS = ("jpeg_encode", "jpeg_scan", "jpeg_pack")


def rendered_frame(h, w, seed=0):
    """A CompImage holding one rendered frame (and the layer that painted it, to keep it alive)."""
    clip = bench.ClipSynth(h, w, 8, seed)
    pixmap = np.stack([clip.frame(0), clip.frame(3), clip.frame(6)], axis=-1)
    flow = np.empty((h, w, 2), np.float32)
    flow[..., 0] = clip.u[:, None]
    flow[..., 1] = clip.v[None, :]
    yy, xx = np.mgrid[0:h, 0:w]
    flow[..., 0] = np.clip(xx + np.rint(flow[..., 0]), 0, w - 1) - xx      # stays in the frame (post_process's clip)
    flow[..., 1] = np.clip(yy + np.rint(flow[..., 1]), 0, h - 1) - yy
    layer = RemapLayer(h, w)
    layer.set_sources([np.ones((h, w), np.uint8)])
    comp = CompImage(h, w, (255, 255, 255))
    layer.update(flow)
    layer.gather(0, pixmap)
    comp.begin()
    layer.render(comp)
    sync()
    return comp, layer


class Events:
    def __init__(self):
        self.lib = _lib.load()
        self.a, self.b = C.c_void_p(), C.c_void_p()
        _lib.check(self.lib.tf_event_create(C.byref(self.a)))
        _lib.check(self.lib.tf_event_create(C.byref(self.b)))

    def start(self):
        _lib.check(self.lib.tf_event_record(self.a))

    def stop_ms(self):
        _lib.check(self.lib.tf_event_record(self.b))
        _lib.check(self.lib.tf_event_synchronize(self.b))
        ms = C.c_float()
        _lib.check(self.lib.tf_event_elapsed_ms(self.a, self.b, C.byref(ms)))
        return ms.value


def spread(values):
    return {"median_ms": statistics.median(values), "min_ms": min(values), "max_ms": max(values), "n": len(values)}


def host_path(comp, pinned, quality, restart, reps):
    down, enc, both = [], [], []
    data = b""
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        frame = comp.download(pinned)
        t1 = time.perf_counter()
        data = pillow_encode(frame, quality, restart)
        t2 = time.perf_counter()
        down.append((t1 - t0) * 1e3), enc.append((t2 - t1) * 1e3), both.append((t2 - t0) * 1e3)
    return {"download_ms": spread(down[1:]), "pillow_encode_ms": spread(enc[1:]), "per_frame_ms": spread(both[1:]),
            "bytes": len(data)}, data


def device_path(comp, h, w, quality, restart, reps, rounds, events):
    enc = JpegEncoder(h, w, quality, restart)
    out = np.empty(h * w * 3 // 2, np.uint8)
    try:
        n = enc.encode_into(comp, out)                       # warm-up, and the file to compare
        data = out[:n].tobytes()
        wall, dev = [], []
        for _ in range(rounds):
            events.start()
            t0 = time.perf_counter()
            for _ in range(reps):
                enc.encode_into(comp, out)
            wall.append((time.perf_counter() - t0) * 1e3 / reps)
            dev.append(events.stop_ms() / reps)
        _lib.profile(True, "jpeg_")
        for _ in range(reps):
            enc.encode_into(comp, out)
        sync()
        report = _lib.profile_report()
        _lib.profile(False)
        kernels = {k: {"launches": report[k][0], "ms_per_launch": report[k][1] / report[k][0]} for k in KERNELS if k in report}
    finally:
        enc.close()
    return {"restart_mcus": restart, "bytes": len(data), "per_frame_ms": spread(wall),
            "per_frame_device_events_ms": spread(dev), "kernels": kernels}, data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--csv")
    ap.add_argument("--quality", type=int, default=50)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--sizes", default="4k,1080p")
    ap.add_argument("--intervals", default="1,2,4,8,16,row")
    args = ap.parse_args()
    events = Events()
    result = {"tool": "bench_jpeg", "quality": args.quality, "host": bench.host_description(), "sizes": {}}
    rows = []
    for name in args.sizes.split(","):
        h, w = SIZES[name]
        comp, layer = rendered_frame(h, w)
        pinned = pinned_empty((h, w, 3), np.uint8)
        entry = {"height": h, "width": w, "raw_bytes": h * w * 3, "device": []}
        intervals = [(w + 15) // 16 if v == "row" else int(v) for v in args.intervals.split(",")]
        for restart in intervals:
            run, data = device_path(comp, h, w, args.quality, restart, args.reps, args.rounds, events)
            run["equals_pillow"] = data == pillow_encode(comp.download(pinned), args.quality, restart)
            entry["device"].append(run)
            for k, v in run["kernels"].items():
                rows.append((name, restart, k, v["launches"], v["ms_per_launch"]))
        smallest = min(r["bytes"] for r in entry["device"])
        eligible = [r for r in entry["device"] if r["bytes"] <= 1.02 * smallest]
        best = min(eligible, key=lambda r: r["per_frame_ms"]["median_ms"])
        entry["default_rule"] = {"smallest_bytes": smallest, "within_2_percent": [r["restart_mcus"] for r in eligible],
                                 "fastest_of_them": best["restart_mcus"]}
        library = JpegEncoder(h, w, args.quality)
        entry["library_default_restart_mcus"] = library.restart_mcus
        library.close()
        entry["host"], _ = host_path(comp, pinned, args.quality, library.restart_mcus, args.host_reps)
        dflt = next((r for r in entry["device"] if r["restart_mcus"] == library.restart_mcus), best)
        entry["device_beats_host"] = dflt["per_frame_ms"]["median_ms"] < entry["host"]["per_frame_ms"]["median_ms"]
        entry["host_over_device"] = entry["host"]["per_frame_ms"]["median_ms"] / dflt["per_frame_ms"]["median_ms"]
        result["sizes"][name] = entry
        layer.close()
        comp.close()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.csv:
        with open(args.csv, "w") as f:
            f.write("size,restart_mcus,kernel,launches,ms_per_launch\n")
            for row in rows:
                f.write("%s,%d,%s,%d,%.6f\n" % row)


if __name__ == "__main__":
    main()
