#!/usr/bin/env python3
"""What a frame of a Y4M or raw .yuv file costs on its way onto the card, at 4K and 1080p, on planes of noise (the
kernel's time does not depend on the values).  Medians over `--rounds` windows of `--reps` calls, each call ending in a
synchronise.

  (a) the parent's way to get such a frame onto the card: DevicePixmap.from_host of the uint8 (H, W, 3) BGR array, from
      pageable memory.
  (b) tf_yuvdec_convert from pageable memory for each layout and chroma mode: the copy into the staging buffer, the
      upload of the planes and the kernel; host clock and device events.
  (c) the kernel alone, from the library's event profiler in a pass of its own: the bytes it must move (1.5 to 3 a pixel
      in, 3 out) over its time, as a share of the HBM copy rate the other sections use.
  check  the pixels are the numpy restatement's (tests/yuvdec_ref.py), byte for byte.

Reading the file and whatever follows the frame are not measured.

    python tools/bench_yuvdec.py [--out profiles/yuvdec_bench.json]

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
from bench_jpeg import Events, spread  # noqa: E402
from tests import yuvdec_cases, yuvdec_ref  # noqa: E402
from transflow_amd import _lib  # noqa: E402
from transflow_amd.device import sync  # noqa: E402
from transflow_amd.pixmap import DevicePixmap, _dev_alloc, _dev_download  # noqa: E402
from transflow_amd.yuvdec import CHROMAS, LAYOUTS, YuvDecoder  # noqa: E402

SIZES = {"4k": (2160, 3840), "1080p": (1080, 1920)}
HBM_BYTES_PER_S = 6.29e12          # the measured copy rate of the MI355X's HBM3E (8.0 TB/s on paper)
LABELS = {"yuv444p": "yuvdec_444p", "yuv422p": "yuvdec_422p", "yuv420p": "yuvdec_420p", "nv12": "yuvdec_nv12"}


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


def from_host(bgr):
    pixmap = DevicePixmap.from_host(bgr)
    sync()
    pixmap.close()


def layout_path(dec, out, h, w, layout, chroma, args, events):
    planes = yuvdec_cases.noise(w, h, layout, 3)

    def call():
        dec.convert_into(planes, w, h, layout, out.ptr, chroma=chroma)
        sync()

    run = windows(call, args.reps, args.rounds, events)
    run["bytes"] = int(planes.nbytes)
    got = _dev_download(out, (h, w, 3))
    run["equals_the_restatement"] = bool((got == yuvdec_ref.convert_back(planes, w, h, layout, chroma=chroma, order="bgr")).all())
    label = LABELS[layout] + ("_linear" if chroma == "linear" else "")
    _lib.profile(True, label)
    for _ in range(args.reps):
        call()
    report = _lib.profile_report()
    _lib.profile(False)
    launches, ms = report[label]
    moved = planes.nbytes + 3 * h * w
    run["kernel"] = {"label": label, "launches": launches, "ms_per_launch": ms / launches, "bytes": moved,
                     "share_of_hbm_rate": moved / (ms / launches * 1e-3) / HBM_BYTES_PER_S}
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="4k,1080p")
    args = ap.parse_args()
    events = Events()
    result = {"tool": "bench_yuvdec", "host": bench.host_description(), "hbm_bytes_per_s": HBM_BYTES_PER_S, "reps": args.reps,
              "rounds": args.rounds, "sizes": {}}
    for name in args.sizes.split(","):
        h, w = SIZES[name]
        bgr = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
        entry = {"height": h, "width": w}
        entry["bgr_from_host"] = dict(windows(lambda: from_host(bgr), args.reps, args.rounds, events), bytes=h * w * 3)
        dec, out = YuvDecoder(w, h), _dev_alloc(3 * h * w)
        entry["layouts"] = {f"{layout}/{chroma}": layout_path(dec, out, h, w, layout, chroma, args, events)
                            for layout in LAYOUTS for chroma in CHROMAS}
        base = entry["bgr_from_host"]["per_frame_ms"]["median_ms"]
        for run in entry["layouts"].values():
            run["over_bgr_from_host"] = run["per_frame_ms"]["median_ms"] / base
        dec.close(), out.close()
        result["sizes"][name] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
