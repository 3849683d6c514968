#!/usr/bin/env python3
"""What the frame's own literal/length code (PngEncoder(code="frame")) costs and saves against the
library's fixed code, at 4K and 1080p, on a rendered frame of the bench's clip (tools/bench_jpeg.py makes it) and on
seeded noise.

  time   both modes on one resident frame, in one process, alternating window by window: `--rounds` windows of `--reps`
         calls of encode_into each (every call ends in a synchronise and has the file in host memory), host clock and
         device events, median and spread per mode; per kernel from the library's own event profiler, in a pass of its
         own per mode.
  size   both files against the raw frame, zlib level 1 with Z_RLE on Sub-filtered rows and Pillow's compress_level=1
         file (tools/bench_png.py's columns); the stored bands, the repairs and the longest code of the frame's own.
  check  Pillow decodes the frame-coded file to the frame's pixels.

    python tools/bench_png_frame_code.py [--out profiles/png_frame_code_bench.json] [--csv profiles/png_frame_code_kernel_stats.csv]

Prints one JSON object (and writes it to --out)."""
import argparse
import io
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
from bench_png import SIZES, opencv_default_size  # noqa: E402
from tests import png_ref  # noqa: E402
from transflow_amd import _lib  # noqa: E402
from transflow_amd.device import pinned_empty, sync  # noqa: E402
from transflow_amd.pixmap import DevicePixmap  # noqa: E402
from transflow_amd.png import PngEncoder, pillow_encode_png  # noqa: E402

MODES = ("fixed", "frame")
KERNELS = ("png_filter", "png_count", "png_total", "png_table", "png_deflate", "png_scan", "png_pack")


def measure(source, frame, h, w, args, events):
    encoders = {mode: PngEncoder(h, w, code=mode) for mode in MODES}
    out = np.empty(png_ref.file_bound(h, w, 0), np.uint8)
    run = {mode: {"wall": [], "dev": []} for mode in MODES}
    try:
        files = {}
        for mode, enc in encoders.items():                   # warm-up, and the files to compare
            files[mode] = out[:enc.encode_into(source, out)].tobytes()
        for _ in range(args.rounds):
            for mode, enc in encoders.items():
                events.start()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    enc.encode_into(source, out)
                run[mode]["wall"].append((time.perf_counter() - t0) * 1e3 / args.reps)
                run[mode]["dev"].append(events.stop_ms() / args.reps)
        result = {}
        for mode, enc in encoders.items():
            _lib.profile(True, "png_")
            for _ in range(args.reps):
                enc.encode_into(source, out)
            sync()
            report = _lib.profile_report()
            _lib.profile(False)
            kernels = {k: {"launches": report[k][0], "ms_per_launch": report[k][1] / report[k][0]} for k in KERNELS if k in report}
            result[mode] = {"bytes": len(files[mode]), "per_frame_ms": spread(run[mode]["wall"]),
                            "per_frame_device_events_ms": spread(run[mode]["dev"]), "kernels": kernels,
                            "kernels_ms_sum": sum(v["ms_per_launch"] for v in kernels.values())}
        enc = encoders["frame"]
        lengths, repairs = enc.last_code()
        sizes, stored = enc.last_bands()
        result["frame"].update(bands=len(sizes), stored_bands=sum(stored), repairs=repairs, longest_code=max(lengths),
                               used_symbols=sum(1 for n in lengths if n))
    finally:
        for enc in encoders.values():
            enc.close()
    import PIL.Image
    with PIL.Image.open(io.BytesIO(files["frame"])) as im:
        result["frame"]["pillow_decodes_to_the_frame"] = bool((np.asarray(im.convert("RGB")) == frame).all())
    bound = png_ref.file_bound(h, w, 0)
    result["frame"]["within_bound"] = len(files["frame"]) <= bound
    rle = opencv_default_size(frame) + 57                    # + signature, IHDR, one IDAT's 12 bytes, IEND
    pillow = len(pillow_encode_png(frame))
    fixed, own = len(files["fixed"]), len(files["frame"])
    result["sizes"] = {"raw_bytes": h * w * 3, "fixed_bytes": fixed, "frame_bytes": own, "zlib_level1_rle_sub_bytes": rle,
                       "pillow_level1_bytes": pillow, "frame_over_fixed": own / fixed, "frame_over_raw": own / (h * w * 3),
                       "frame_over_zlib_rle": own / rle, "frame_over_pillow_level1": own / pillow,
                       "fixed_over_zlib_rle": fixed / rle, "fixed_over_pillow_level1": fixed / pillow}
    result["frame_over_fixed_ms"] = result["frame"]["per_frame_ms"]["median_ms"] / result["fixed"]["per_frame_ms"]["median_ms"]
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--csv")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="4k,1080p")
    args = ap.parse_args()
    events = Events()
    result = {"tool": "bench_png_frame_code", "host": bench.host_description(), "reps": args.reps, "rounds": args.rounds, "sizes": {}}
    rows = []
    for name in args.sizes.split(","):
        h, w = SIZES[name]
        entry = {"height": h, "width": w}
        pinned = pinned_empty((h, w, 3), np.uint8)
        comp, layer = rendered_frame(h, w)
        entry["rendered"] = measure(comp, np.array(comp.download(pinned)), h, w, args, events)
        layer.close()
        comp.close()
        noise = png_ref.noise_image(h, w, 1)
        pixmap = DevicePixmap.from_host(noise)
        entry["noise"] = measure(pixmap, noise, h, w, args, events)
        pixmap.close()
        for content in ("rendered", "noise"):
            for mode in MODES:
                for k, v in entry[content][mode]["kernels"].items():
                    rows.append((name, content, mode, k, v["launches"], v["ms_per_launch"]))
        result["sizes"][name] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.csv:
        with open(args.csv, "w") as f:
            f.write("size,content,code,kernel,launches,ms_per_launch\n")
            for row in rows:
                f.write("%s,%s,%s,%s,%d,%.6f\n" % row)


if __name__ == "__main__":
    main()
