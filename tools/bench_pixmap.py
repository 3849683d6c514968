#!/usr/bin/env python3
"""What making a gradient pixmap costs: tf_pixmap_gradient_dev on the GPU, the vectorised numpy restatement
(tests/px_ref.py) on the host, and the reference's per-pixel Python loop.

The device figure is a host clock around `reps` launches that end in a synchronise, after a warm-up, and the median
of `rounds` such windows.  The host figures are this machine's CPU.  The reference's loop (still.py:156-163) is timed
as tests/px_ref.py restates it, statement for statement, at 64 x 96 -- 6144 pixels take a fraction of a second -- and
its time at 1080p and 4K is that rate times the pixel count: a PROJECTION, marked as one in the output; nobody waits
four minutes for it here.  The whole source (`HipGradientPixmapSource.__enter__`: tree, allocation, launch, event) is
timed too, and the colour fill.

    python tools/bench_pixmap.py [--out profiles/pixmap_bench.json] [--seed 0] [--reps 20] [--rounds 5] [--no-host]

Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import px_ref  # noqa: E402
from transflow_amd import pixmap as P  # noqa: E402
from transflow_amd.device import DevBuffer, sync  # noqa: E402

SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}


def device_ms(call, reps, rounds):
    call()
    sync()
    windows = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        sync()
        windows.append((time.perf_counter() - t0) * 1e3 / reps)
    return {"median_ms": statistics.median(windows), "min_ms": min(windows), "max_ms": max(windows), "reps": reps, "rounds": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host comparisons (for a profiler run)")
    args = ap.parse_args()
    tree = px_ref.gradient_tree(args.seed)
    nodes = px_ref.flatten(tree)
    result = {"tool": "bench_pixmap", "seed": args.seed, "tree_nodes": len(nodes), "sizes": {}}
    if not args.no_host:
        t0 = time.perf_counter()
        small = px_ref.gradient_loop(tree, 64, 96)
        loop_s = time.perf_counter() - t0
        assert np.array_equal(small, px_ref.gradient_from_tree(tree, 64, 96))
        result["python_loop_64x96"] = {"seconds": loop_s, "us_per_pixel": loop_s / (64 * 96) * 1e6,
                                       "what": "the reference's per-pixel loop as tests/px_ref.py restates it, this machine's CPU"}
    for name, (h, w) in SIZES.items():
        buf = DevBuffer(h * w * 3)
        entry = {"height": h, "width": w}
        entry["gradient_kernel"] = device_ms(lambda: P._dev_gradient(buf, w, h, nodes), args.reps, args.rounds)
        entry["fill_kernel"] = device_ms(lambda: P._dev_fill(buf, h * w, (16, 32, 48)), args.reps, args.rounds)
        P._dev_gradient(buf, w, h, nodes)
        got = buf.download((h, w, 3), np.uint8)
        buf.close()
        enters = []
        for _ in range(3):
            t0 = time.perf_counter()
            with P.HipGradientPixmapSource(w, h, args.seed) as s:
                next(s).wait_on_stream()
                sync()
                enters.append((time.perf_counter() - t0) * 1e3)
        entry["source_enter_ms"] = {"median_ms": statistics.median(enters), "all_ms": enters}
        if not args.no_host:
            t0 = time.perf_counter()
            want = px_ref.gradient_from_tree(tree, h, w)
            entry["numpy_restatement_ms"] = (time.perf_counter() - t0) * 1e3
            entry["bit_identical_to_restatement"] = bool(np.array_equal(got, want))
            entry["python_loop_projected_s"] = result["python_loop_64x96"]["us_per_pixel"] * 1e-6 * h * w
            entry["python_loop_projected_from"] = "64x96 rate x pixel count (not run at this size)"
        result["sizes"][name] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
