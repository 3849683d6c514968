#!/usr/bin/env python3
"""What a frame on its way to a video encoder costs: the download of the RGB frame against the conversion to planes on
the device and the download of those, at 4K and 1080p, on a rendered frame of the bench's clip (tools/bench_jpeg.py makes
it).  Medians over `--rounds` windows of `--reps` calls, each call ending in a synchronise with its bytes in page-locked
host memory.

  (a) the parent's way: comp.download() of the uint8 (H, W, 3) frame.
  (b) tf_yuv_convert_dev for each layout: the kernel and the download of the planes; host clock and device events.
  (c) the kernel alone, from the library's event profiler in a pass of its own: the bytes it must move (3 a pixel in,
      1.5 to 3 out) over its time, as a share of the HBM copy rate the other sections use.
  check  the planes are the numpy restatement's (tests/yuv_ref.py), byte for byte.

The pipe and ffmpeg behind it are not measured.

    python tools/bench_yuv.py [--out profiles/yuv_bench.json]

Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from bench_jpeg import Events, rendered_frame, spread  # noqa: E402
from tests import yuv_ref  # noqa: E402
from transflow_amd import _lib  # noqa: E402
from transflow_amd.device import pinned_empty, sync  # noqa: E402
from transflow_amd.yuv import LAYOUTS, YuvEncoder  # noqa: E402

SIZES = {"4k": (2160, 3840), "1080p": (1080, 1920)}
HBM_BYTES_PER_S = 6.29e12          # the measured copy rate of the MI355X's HBM3E (8.0 TB/s on paper)


def windows(call, reps, rounds, events):
    call()                                                   # warm-up
    wall, dev = [], []
    for _ in range(rounds):
        events.start()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        wall.append((time.perf_counter() - t0) * 1e3 / reps)
        dev.append(events.stop_ms() / reps)
    return {"per_frame_ms": spread(wall), "per_frame_device_events_ms": spread(dev)}


def layout_path(comp, frame, h, w, layout, args, events):
    enc = YuvEncoder(h, w, layout)
    out = pinned_empty((enc.nbytes,), np.uint8)
    try:
        run = windows(lambda: enc.encode_into(comp, out), args.reps, args.rounds, events)
        run["bytes"] = enc.nbytes
        run["equals_the_restatement"] = out.tobytes() == yuv_ref.convert(frame, layout)
        label = "yuv_" + layout[3:] if layout.startswith("yuv") else "yuv_" + layout
        _lib.profile(True, label)
        for _ in range(args.reps):
            enc.encode_into(comp, out)
        sync()
        report = _lib.profile_report()
        _lib.profile(False)
        launches, ms = report[label]
        moved = h * w * 3 + enc.nbytes
        run["kernel"] = {"label": label, "launches": launches, "ms_per_launch": ms / launches, "bytes": moved,
                         "share_of_hbm_rate": moved / (ms / launches * 1e-3) / HBM_BYTES_PER_S}
    finally:
        enc.close()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="4k,1080p")
    args = ap.parse_args()
    events = Events()
    result = {"tool": "bench_yuv", "host": bench.host_description(), "hbm_bytes_per_s": HBM_BYTES_PER_S, "reps": args.reps,
              "rounds": args.rounds, "sizes": {}}
    for name in args.sizes.split(","):
        h, w = SIZES[name]
        pinned = pinned_empty((h, w, 3), np.uint8)
        comp, layer = rendered_frame(h, w)
        entry = {"height": h, "width": w}
        entry["rgb_download"] = dict(windows(lambda: comp.download(pinned), args.reps, args.rounds, events), bytes=h * w * 3)
        frame = np.array(comp.download(pinned))
        entry["layouts"] = {layout: layout_path(comp, frame, h, w, layout, args, events) for layout in LAYOUTS}
        rgb_ms = entry["rgb_download"]["per_frame_ms"]["median_ms"]
        for run in entry["layouts"].values():
            run["over_rgb_download"] = run["per_frame_ms"]["median_ms"] / rgb_ms
        layer.close()
        comp.close()
        result["sizes"][name] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
