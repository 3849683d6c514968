#!/usr/bin/env python3
"""What the chroma layouts of the device JPEG encoder cost: 4:4:4, 4:2:2 and 4:2:0 (JpegEncoder(subsampling=0 / 1 / 2)) on
the rendered frame of tools/bench_jpeg.py, at 4K and 1080p, quality 50 and 90 -- per layout at the library's default
restart interval (16, 12, 8 MCUs: 48 blocks each) and at half and twice that, so that the two defaults nobody tuned have
numbers beside them.  Per run: ms per frame (host clock around `--reps` calls of encode_into, each of which ends with
the file in host memory; median of `--rounds` windows; device events around the same calls), the kernels per launch
from the library's event profiler, the file's size, and whether the file equals Pillow's, byte for byte.

Every (size, quality) is a step: a child process of this tool with a time limit of its own (`--step-timeout` seconds);
the first step that fails or runs out of time ends the run, and nothing more is started on the GPU.  This process never
opens the GPU.

    python tools/bench_jpeg_subsampling.py [--out profiles/jpeg_subsampling_bench.json]
        [--ab-parent A.json B.json --ab-branch C.json D.json]

--ab-parent / --ab-branch: the outputs of `python tools/bench_jpeg.py --sizes 4k --intervals 8` in the parent's
checkout and in this tree, two runs each on one box: the four 4K default (4:2:0) times go into the result, with the
verdict -- the branch's slower run may exceed the parent's slower run by no more than the spread between the parent's two.

    rocprofv3 --kernel-trace --stats ... -- python tools/bench_jpeg_subsampling.py --step 4k 50 --reps 10 --rounds 1
is the profiler's view of the kernels, a run of its own (profiles/jpeg_subsampling_kernel_stats.csv).

Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: "4:4:4", 1: "4:2:2", 2: "4:2:0"}
KERNELS = ("jpeg_encode", "jpeg_scan", "jpeg_pack")


def step(size, quality, reps, rounds):
    """One (size, quality) on the GPU: every layout at half, once and twice its default interval."""
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_jpeg
    from transflow_amd import _lib
    from transflow_amd.device import pinned_empty, sync
    from transflow_amd.jpeg import JpegEncoder, pillow_encode
    h, w = bench_jpeg.SIZES[size]
    comp, layer = bench_jpeg.rendered_frame(h, w)
    frame = comp.download(pinned_empty((h, w, 3), np.uint8)).copy()
    events = bench_jpeg.Events()
    out = np.empty(h * w * 3, np.uint8)
    runs = []
    for sub in (0, 1, 2):
        default = int(_lib.load().tf_jpeg_default_restart_mcus_for(sub))
        for restart in (default // 2, default, default * 2):
            enc = JpegEncoder(h, w, quality, restart, subsampling=sub)
            try:
                n = enc.encode_into(comp, out)                   # warm-up, and the file to compare
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
            finally:
                enc.close()
            runs.append({"subsampling": sub, "layout": NAMES[sub], "restart_mcus": restart, "is_default": restart == default,
                         "bytes": len(data), "encode_ms": bench_jpeg.spread(wall), "encode_device_events_ms": bench_jpeg.spread(dev),
                         "kernels_ms_per_launch": {k: report[k][1] / report[k][0] for k in KERNELS if k in report},
                         "equals_pillow": data == pillow_encode(frame, quality, restart, subsampling=sub)})
    layer.close()
    comp.close()
    return {"size": size, "height": h, "width": w, "quality": quality, "raw_bytes": h * w * 3, "runs": runs}


def four_k_default_ms(path):
    with open(path) as f:
        entry = json.load(f)["sizes"]["4k"]
    run = next(r for r in entry["device"] if r["restart_mcus"] == entry["library_default_restart_mcus"])
    return run["per_frame_ms"]["median_ms"]


def parent_comparison(parent_files, branch_files):
    parent, branch = [four_k_default_ms(p) for p in parent_files], [four_k_default_ms(p) for p in branch_files]
    spread = max(parent) - min(parent)
    return {"what": "tools/bench_jpeg.py --sizes 4k --intervals 8, per_frame_ms median, parent and branch alternating on one box",
            "parent_ms": parent, "branch_ms": branch, "parent_spread_ms": spread,
            "branch_over_parent_ms": max(branch) - max(parent),
            "not_slower": max(branch) - max(parent) <= spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sizes", default="4k,1080p")
    ap.add_argument("--qualities", default="50,90")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=float, default=150.0)
    ap.add_argument("--step", nargs=2, metavar=("SIZE", "QUALITY"), help="run one step in this process and print its JSON")
    ap.add_argument("--ab-parent", nargs=2)
    ap.add_argument("--ab-branch", nargs=2)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args.step[0], int(args.step[1]), args.reps, args.rounds)))
        return 0
    result = {"tool": "bench_jpeg_subsampling", "reps": args.reps, "rounds": args.rounds, "steps": []}
    status = 0
    for size in args.sizes.split(","):
        for quality in args.qualities.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", size, quality, "--reps", str(args.reps),
                   "--rounds", str(args.rounds)]
            try:
                done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                result["stopped"] = f"step {size} q{quality} ran past {args.step_timeout} s"
                status = 124
                break
            if done.returncode != 0:
                result["stopped"] = f"step {size} q{quality} ended with status {done.returncode}"
                status = 1
                break
            result["steps"].append(json.loads(done.stdout.decode().strip().splitlines()[-1]))
        if status:
            break
    if not status:
        sys.path.insert(0, ROOT)
        import bench
        result["host"] = bench.host_description()
    if args.ab_parent and args.ab_branch:
        result["parent_comparison_420"] = parent_comparison(args.ab_parent, args.ab_branch)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
