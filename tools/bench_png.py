#!/usr/bin/env python3
"""What a lossless compressed frame costs: the download and host encode a frame-sequence output needs without the
device encoder, against tf_png_encode_dev, at 4K and 1080p, on a rendered frame of the bench's clip (tools/bench_jpeg.py
makes it) and on seeded noise.

  time   (a) host path: comp.download() into a page-locked array + Pillow's PNG encode at compress_level=1 (the stand-in
             for cv2.imwrite, which is not installed): host clock, median of `--host-reps` frames, both also apart.
         (b) device path: PngEncoder.encode_into(resident frame): host clock around `--reps` calls (each ends in a
             synchronise and has the file in host memory), median of `--rounds` windows; device events around the same
             calls; per kernel from the library's own event profiler, in a pass of its own.  For the slowest kernel:
             the bytes it must move (computed from the shapes) over its time, as a share of the HBM rate.
  size   the device's file against zlib level 1 with Z_RLE on Sub-filtered rows (OpenCV's default settings restated with
         zlib) and against Pillow's compress_level=1 file, as ratios; and against the staging bound, which no file may
         exceed.
  check  Pillow decodes the device's file to the frame's pixels.

    python tools/bench_png.py [--out profiles/png_bench.json] [--csv profiles/png_kernel_stats.csv]

Prints one JSON object (and writes it to --out)."""
import argparse
import io
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from bench_jpeg import Events, rendered_frame, spread  # noqa: E402
from tests import png_ref  # noqa: E402
from transflow_amd import _lib  # noqa: E402
from transflow_amd.device import pinned_empty, sync  # noqa: E402
from transflow_amd.pixmap import DevicePixmap  # noqa: E402
from transflow_amd.png import PngEncoder, pillow_encode_png  # noqa: E402

SIZES = {"4k": (2160, 3840), "1080p": (1080, 1920)}
KERNELS = ("png_filter", "png_deflate", "png_scan", "png_pack")
HBM_BYTES_PER_S = 6.29e12          # the measured copy rate of the MI355X's HBM3E (8.0 TB/s on paper)


def opencv_default_size(frame: np.ndarray) -> int:
    """The bytes of the zlib stream OpenCV's defaults make: every row Sub-filtered, level 1, Z_RLE."""
    h, w, _ = frame.shape
    rows = np.zeros((h, 1 + 3 * w), np.uint8)
    rows[:, 0] = 1
    flat = frame.reshape(h, 3 * w)
    rows[:, 1:4] = flat[:, :3]
    rows[:, 4:] = flat[:, 3:] - flat[:, :-3]
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return len(c.compress(rows.tobytes()) + c.flush())


def kernel_bytes(h, w, file_bytes):
    """What each kernel must read and write at the least."""
    raw, stream = h * w * 3, h * (3 * w + 1)
    return {"png_filter": raw + stream, "png_deflate": stream + file_bytes, "png_scan": 0, "png_pack": 2 * file_bytes}


def device_path(source, h, w, reps, rounds, events):
    enc = PngEncoder(h, w)
    out = np.empty(png_ref.file_bound(h, w, 0), np.uint8)
    try:
        n = enc.encode_into(source, out)                     # warm-up, and the file to compare
        data = out[:n].tobytes()
        wall, dev = [], []
        for _ in range(rounds):
            events.start()
            t0 = time.perf_counter()
            for _ in range(reps):
                enc.encode_into(source, out)
            wall.append((time.perf_counter() - t0) * 1e3 / reps)
            dev.append(events.stop_ms() / reps)
        _lib.profile(True, "png_")
        for _ in range(reps):
            enc.encode_into(source, out)
        sync()
        report = _lib.profile_report()
        _lib.profile(False)
        need = kernel_bytes(h, w, len(data))
        kernels = {}
        for k in KERNELS:
            if k in report:
                ms = report[k][1] / report[k][0]
                kernels[k] = {"launches": report[k][0], "ms_per_launch": ms, "bytes": need[k],
                              "share_of_hbm_rate": need[k] / (ms * 1e-3) / HBM_BYTES_PER_S if ms > 0 else None}
        band_rows = enc.band_rows
    finally:
        enc.close()
    slowest = max(kernels, key=lambda k: kernels[k]["ms_per_launch"]) if kernels else None
    return {"band_rows": band_rows, "bytes": len(data), "per_frame_ms": spread(wall), "per_frame_device_events_ms": spread(dev),
            "kernels": kernels, "slowest_kernel": slowest}, data


def host_path(download, reps):
    down, enc, both = [], [], []
    data = b""
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        frame = download()
        t1 = time.perf_counter()
        data = pillow_encode_png(frame)
        t2 = time.perf_counter()
        down.append((t1 - t0) * 1e3), enc.append((t2 - t1) * 1e3), both.append((t2 - t0) * 1e3)
    return {"download_ms": spread(down[1:]), "pillow_level1_encode_ms": spread(enc[1:]), "per_frame_ms": spread(both[1:]),
            "bytes": len(data)}


def measure(source, download, h, w, args, events):
    run, data = device_path(source, h, w, args.reps, args.rounds, events)
    frame = np.array(download())
    import PIL.Image
    with PIL.Image.open(io.BytesIO(data)) as im:
        run["pillow_decodes_to_the_frame"] = bool((np.asarray(im.convert("RGB")) == frame).all())
    bound = png_ref.file_bound(h, w, 0)
    run["bound_bytes"], run["within_bound"] = bound, len(data) <= bound
    host = host_path(download, args.host_reps)
    rle = opencv_default_size(frame) + 57                    # + signature, IHDR, one IDAT's 12 bytes, IEND
    sizes = {"raw_bytes": h * w * 3, "device_bytes": len(data), "zlib_level1_rle_sub_bytes": rle, "pillow_level1_bytes": host["bytes"],
             "device_over_zlib_rle": len(data) / rle, "device_over_pillow_level1": len(data) / host["bytes"]}
    return {"device": run, "host": host, "sizes": sizes,
            "host_over_device": host["per_frame_ms"]["median_ms"] / run["per_frame_ms"]["median_ms"],
            "download_over_device": host["download_ms"]["median_ms"] / run["per_frame_ms"]["median_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--csv")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sizes", default="4k,1080p")
    args = ap.parse_args()
    events = Events()
    result = {"tool": "bench_png", "host": bench.host_description(), "hbm_bytes_per_s": HBM_BYTES_PER_S, "sizes": {}}
    rows = []
    for name in args.sizes.split(","):
        h, w = SIZES[name]
        entry = {"height": h, "width": w}
        pinned = pinned_empty((h, w, 3), np.uint8)
        comp, layer = rendered_frame(h, w)
        entry["rendered"] = measure(comp, lambda: comp.download(pinned), h, w, args, events)
        layer.close()
        comp.close()
        noise = png_ref.noise_image(h, w, 1)
        pixmap = DevicePixmap.from_host(noise)

        entry["noise"] = measure(pixmap, lambda: noise, h, w, args, events)
        # (a DevicePixmap keeps its host copy, so its download cannot be timed: the rendered frame's is the same bytes)
        host, ref = entry["noise"]["host"], entry["rendered"]["host"]
        host["download_ms"] = dict(ref["download_ms"], note="the rendered frame's: the same bytes")
        total = host["download_ms"]["median_ms"] + host["pillow_level1_encode_ms"]["median_ms"]
        host["per_frame_ms"] = {"median_ms": total, "note": "the two medians added"}
        device_ms = entry["noise"]["device"]["per_frame_ms"]["median_ms"]
        entry["noise"]["host_over_device"] = total / device_ms
        entry["noise"]["download_over_device"] = host["download_ms"]["median_ms"] / device_ms
        pixmap.close()
        for content in ("rendered", "noise"):
            for k, v in entry[content]["device"]["kernels"].items():
                rows.append((name, content, k, v["launches"], v["ms_per_launch"], v["bytes"]))
        result["sizes"][name] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.csv:
        with open(args.csv, "w") as f:
            f.write("size,content,kernel,launches,ms_per_launch,bytes\n")
            for row in rows:
                f.write("%s,%s,%s,%d,%.6f,%d\n" % row)


if __name__ == "__main__":
    main()
