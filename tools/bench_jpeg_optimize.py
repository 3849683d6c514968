#!/usr/bin/env python3
"""What the frame's own Huffman tables (JpegEncoder(optimize=True)) cost and save against the
Annex K tables, at 4K and 1080p, quality 50 and 90, on the rendered frame of the bench's clip (tools/bench_jpeg.py makes
it), at the library's default restart interval.

  time   both modes on one resident frame, in one process, alternating window by window: `--rounds` windows of `--reps`
         calls of encode_into each (every call ends in a synchronise and has the file in host memory), host clock and
         device events, median and spread per mode; per kernel from the library's own event profiler, in a pass of its
         own per mode.  k_jpeg_tables is measured in both its forms: the wave reductions the library runs, and one lane
         per table (TF_JPEG_TABLES_ONE_LANE=1), in an encoder of its own.
  size   both files, and what the four DHT segments take in each.
  check  the optimised file is Pillow's `optimize=True` file, byte for byte, and the default file Pillow's default.

    python tools/bench_jpeg_optimize.py [--out profiles/jpeg_optimize_bench.json]

Prints one JSON object (and writes it to --out).  For profiles/jpeg_optimize_kernel_stats.csv the tool is run under
`rocprofv3 --kernel-trace --stats` in a run of its own, with `--reps 10 --rounds 1`."""
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
from bench_jpeg import SIZES, Events, rendered_frame, spread  # noqa: E402
from transflow_amd import _lib  # noqa: E402
from transflow_amd.device import pinned_empty, sync  # noqa: E402
from transflow_amd.jpeg import JpegEncoder, pillow_encode  # noqa: E402

MODES = ("annex_k", "own")
KERNELS = ("jpeg_encode", "jpeg_gather", "jpeg_tables", "jpeg_emit", "jpeg_scan", "jpeg_pack")


def kernels_of(enc, comp, out, reps):
    _lib.profile(True, "jpeg_")
    for _ in range(reps):
        enc.encode_into(comp, out)
    sync()
    report = _lib.profile_report()
    _lib.profile(False)
    return {k: {"launches": report[k][0], "ms_per_launch": report[k][1] / report[k][0]} for k in KERNELS if k in report}


def dht_bytes(data: bytes) -> int:
    total, i = 0, 2
    while data[i + 1] != 0xDA:
        n = int.from_bytes(data[i + 2:i + 4], "big")
        total += 2 + n if data[i + 1] == 0xC4 else 0
        i += 2 + n
    return total


def measure(comp, frame, h, w, quality, args, events):
    encoders = {"annex_k": JpegEncoder(h, w, quality), "own": JpegEncoder(h, w, quality, optimize=True)}
    out = np.empty(h * w * 3 // 2, np.uint8)
    run = {mode: {"wall": [], "dev": []} for mode in MODES}
    result = {"quality": quality, "restart_mcus": encoders["own"].restart_mcus}
    try:
        files = {mode: out[:enc.encode_into(comp, out)].tobytes() for mode, enc in encoders.items()}   # warm-up, and the files
        for _ in range(args.rounds):
            for mode, enc in encoders.items():
                events.start()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    enc.encode_into(comp, out)
                run[mode]["wall"].append((time.perf_counter() - t0) * 1e3 / args.reps)
                run[mode]["dev"].append(events.stop_ms() / args.reps)
        for mode, enc in encoders.items():
            kernels = kernels_of(enc, comp, out, args.reps)
            result[mode] = {"bytes": len(files[mode]), "dht_bytes": dht_bytes(files[mode]), "per_frame_ms": spread(run[mode]["wall"]),
                            "per_frame_device_events_ms": spread(run[mode]["dev"]), "kernels": kernels,
                            "kernels_ms_sum": sum(v["ms_per_launch"] for v in kernels.values())}
        tables = encoders["own"].last_tables()
        result["own"]["symbols"] = [len(vals) for _, vals in tables]
        result["own"]["longest_code"] = [max(i + 1 for i, n in enumerate(bits) if n) for bits, _ in tables]
    finally:
        for enc in encoders.values():
            enc.close()
    os.environ["TF_JPEG_TABLES_ONE_LANE"] = "1"                # read when a handle first needs the mode's buffers
    try:
        enc = JpegEncoder(h, w, quality, optimize=True)
        try:
            same = out[:enc.encode_into(comp, out)].tobytes() == files["own"]
            one_lane = kernels_of(enc, comp, out, args.reps)["jpeg_tables"]
        finally:
            enc.close()
    finally:
        del os.environ["TF_JPEG_TABLES_ONE_LANE"]
    result["tables_kernel"] = {"wave_reductions_ms": result["own"]["kernels"]["jpeg_tables"]["ms_per_launch"],
                               "one_lane_per_table_ms": one_lane["ms_per_launch"], "one_lane_writes_the_same_file": same}
    restart = result["restart_mcus"]
    result["own"]["equals_pillow_optimize"] = files["own"] == pillow_encode(frame, quality, restart, optimize=True)
    result["annex_k"]["equals_pillow"] = files["annex_k"] == pillow_encode(frame, quality, restart)
    a, b = result["annex_k"], result["own"]
    result["own_over_annex_k_bytes"] = b["bytes"] / a["bytes"]
    result["bytes_saved"] = a["bytes"] - b["bytes"]
    result["own_over_annex_k_ms"] = b["per_frame_ms"]["median_ms"] / a["per_frame_ms"]["median_ms"]
    result["own_minus_annex_k_ms"] = b["per_frame_ms"]["median_ms"] - a["per_frame_ms"]["median_ms"]
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="4k,1080p")
    ap.add_argument("--qualities", default="50,90")
    args = ap.parse_args()
    events = Events()
    result = {"tool": "bench_jpeg_optimize", "host": bench.host_description(), "reps": args.reps, "rounds": args.rounds,
              "gather_form": "per-wave LDS histogram, non-zero counters added to the frame's with atomics (the per-interval "
                             "rows and column sums were not built)", "sizes": {}}
    for name in args.sizes.split(","):
        h, w = SIZES[name]
        comp, layer = rendered_frame(h, w)
        frame = np.array(comp.download(pinned_empty((h, w, 3), np.uint8)))
        entry = {"height": h, "width": w, "raw_bytes": h * w * 3}
        for quality in (int(q) for q in args.qualities.split(",")):
            entry[f"q{quality}"] = measure(comp, frame, h, w, quality, args, events)
        result["sizes"][name] = entry
        layer.close()
        comp.close()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
