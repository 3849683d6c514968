#!/usr/bin/env python3
"""What a JPEG frame WITHOUT restart markers costs up to its pixels being in device memory ("scans
without restart markers"): the frames of tools/bench_jpegdec.py (4K and 1080p, quality 90, 4:2:0) written without DRI,
and a quality-100 noise frame at 1080p as the slow case.

  mode1    JpegDecoder(parallel_scan=True).decode: host clock around call and wait (medians after a warm-up), the
           kernels apart from the library's event profiler in a pass of its own, and tf_jpegdec_par_stats.
  mode0    the same file through the one-wave path (k_jd_entropy, which this path leaves as it was).
  pillow   Pillow's decode to an RGB array on one core of this machine, and the upload of that array.
  sweep    mode1 at the 4K and the noise frame over subsequence sizes, group sizes and the scan read through the cache or
           from LDS (jd_par_sub_bytes, jd_par_group_subs, jd_par_staged).
  flow     frames/s of a Farnebäck HipFlowSource over an MjpegFrameProvider of a clip without DRI: parallel_scan=True
           against the default route such a clip takes (Pillow on the host, the pixels uploaded).
Every leg runs in a process of its own.

    python tools/bench_jpegdec_par.py [--out profiles/jpegdec_par_bench.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_jpegdec_par.py --kernels-only      (a run of its own)

Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_jpegdec import SIZES, encode, pillow_decode, scene  # noqa: E402

KERNELS = ("jd_count", "jd_scan", "jd_markers", "jd_par_init", "jd_par_sync", "jd_par_scan", "jd_par_write", "jd_par_idct", "jd_entropy", "jd_colour")
FRAMES = {"4k": ("4k", "scene"), "1080p": ("1080p", "scene"), "1080p_noise_q100": ("1080p", "noise")}


def frame_file(name, shift=0):
    size, kind = FRAMES[name]
    h, w = SIZES[size]
    if kind == "scene":
        return encode(scene(h, w, shift), 0)
    import io

    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(np.random.default_rng(11).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(buf, format="JPEG", quality=100, subsampling=2)
    return buf.getvalue()


def spread(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "runs": len(v)}


def decode_leg(name, mode, sub, group, reps, warmup, staged=0):
    from transflow_amd import _lib
    from transflow_amd.device import sync
    from transflow_amd.jpegdec import JpegDecoder, probe
    data = frame_file(name)
    info = probe(data)
    assert info.restart_mcus == 0
    _lib.set_option("jd_par_sub_bytes", sub)
    _lib.set_option("jd_par_group_subs", group)
    _lib.set_option("jd_par_staged", staged)
    dec = JpegDecoder(info.width, info.height, parallel_scan=bool(mode))
    pix = dec.decode(data)
    same = bool(np.array_equal(np.asarray(pix), pillow_decode(data)))
    pix.close()
    for _ in range(warmup):
        dec.decode(data).close()
    sync()
    whole = []
    for _ in range(reps):
        t0 = time.perf_counter()
        pix = dec.decode(data)
        sync()
        whole.append((time.perf_counter() - t0) * 1e3)
        pix.close()
    _lib.profile(True, "jd_")
    for _ in range(reps):
        dec.decode(data).close()
    sync()
    report = _lib.profile_report()
    _lib.profile(False)
    kernels = {k: {"launches_per_decode": report[k][0] / reps, "ms_per_decode": report[k][1] / reps} for k in KERNELS if k in report}
    out = {"frame": name, "mode": mode, "file_bytes": len(data), "per_frame_ms": spread(whole), "kernels": kernels,
           "kernels_ms": sum(v["ms_per_decode"] for v in kernels.values()), "pixels_are_pillows": same}
    if mode:
        out["stats"] = dec.par_stats()
        out["sub_bytes"], out["group_subs"], out["staged"] = sub or "default", group or "default", staged
    dec.close()
    return out


def pillow_leg(name, reps):
    from transflow_amd.device import DevBuffer, sync
    data = frame_file(name)
    array = pillow_decode(data)
    dev = DevBuffer(array.nbytes)
    dev.upload(array)
    decode_ms, upload_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        array = pillow_decode(data)
        t1 = time.perf_counter()
        dev.upload(array)
        sync()
        decode_ms.append((t1 - t0) * 1e3), upload_ms.append((time.perf_counter() - t1) * 1e3)
    dev.close()
    return {"frame": name, "pillow_decode_ms": spread(decode_ms), "upload_raw_ms": spread(upload_ms)}


def flow_leg(name, parallel, frames, batch):
    from transflow_amd.config import FlowConfig
    from transflow_amd.device import sync
    from transflow_amd.flow import HipFlowSource
    from transflow_amd.jpegdec import MjpegFrameProvider
    files = [frame_file(name, 3 * i) for i in range(frames)]
    provider = MjpegFrameProvider(files, parallel_scan=parallel)
    cfg = FlowConfig(hip_device_flows=True, hip_batch=batch)
    with HipFlowSource.from_args(provider, direction="backward", cv_config=cfg) as source:
        next(source)
        t0 = time.perf_counter()
        n = sum(1 for _ in source)
        sync()
        rate = n / (time.perf_counter() - t0)
    return {"frame": name, "parallel_scan": parallel, "frames_per_s": rate, "fallbacks": provider.fallbacks, "frames": frames, "batch": batch}


def child(*leg):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", json.dumps(leg)], capture_output=True, text=True, timeout=420)
    if out.returncode != 0:
        raise RuntimeError(f"leg {leg} failed: {out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def kernels_only(reps):
    """For a profiler around this process: mode-1 decodes of the 4K frame at the default sizes, nothing else."""
    from transflow_amd.device import sync
    from transflow_amd.jpegdec import JpegDecoder
    h, w = SIZES["4k"]
    data = frame_file("4k")
    dec = JpegDecoder(w, h, parallel_scan=True)
    for _ in range(reps):
        dec.decode(data).close()
    sync()
    dec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", default="4k,1080p,1080p_noise_q100")
    ap.add_argument("--sweep-subs", default="32,64,128,256,512")
    ap.add_argument("--sweep-groups", default="64,128,256")
    ap.add_argument("--flow-frames", type=int, default=13)
    ap.add_argument("--flow-batch", type=int, default=4)
    ap.add_argument("--flow-rounds", type=int, default=3)
    ap.add_argument("--no-mode0", action="store_true")
    ap.add_argument("--leg", help="(a child of this tool) one leg as JSON; prints its result")
    ap.add_argument("--kernels-only", action="store_true", help="only mode-1 decodes, for a profiler around this process")
    args = ap.parse_args()
    if args.leg:
        kind, *rest = json.loads(args.leg)
        print(json.dumps({"decode": decode_leg, "pillow": pillow_leg, "flow": flow_leg}[kind](*rest)))
        return
    if args.kernels_only:
        kernels_only(args.reps)
        return
    import bench
    result = {"tool": "bench_jpegdec_par", "host": bench.host_description(), "quality": 90, "sampling": "4:2:0", "restart_interval": None,
              "frames": {}}
    for name in args.frames.split(","):
        entry = {"mode1": child("decode", name, 1, 0, 0, args.reps, args.warmup), "pillow": child("pillow", name, 5)}
        if not args.no_mode0:
            entry["mode0"] = child("decode", name, 0, 0, 0, 2, 0)
            entry["mode0_over_mode1"] = entry["mode0"]["per_frame_ms"]["median_ms"] / entry["mode1"]["per_frame_ms"]["median_ms"]
        entry["pillow_over_mode1"] = entry["pillow"]["pillow_decode_ms"]["median_ms"] / entry["mode1"]["per_frame_ms"]["median_ms"]
        result["frames"][name] = entry
        print(name, "mode1", entry["mode1"]["per_frame_ms"]["median_ms"], "pillow", entry["pillow"]["pillow_decode_ms"]["median_ms"], file=sys.stderr, flush=True)
    sweep = []
    for sub in (int(v) for v in args.sweep_subs.split(",") if v):
        for group in (int(v) for v in args.sweep_groups.split(",")):
            for name, staged in (("4k", 0), ("1080p_noise_q100", 0), ("4k", 1), ("1080p_noise_q100", 1)):
                if staged and (sub & (sub - 1) or group * (sub + 4) + 16 > 48 * 1024):
                    continue                                             # the library reads through the cache there
                run = child("decode", name, 1, sub, group, args.reps, args.warmup, staged)
                sweep.append({"frame": name, "sub_bytes": sub, "group_subs": group, "staged": staged, "median_ms": run["per_frame_ms"]["median_ms"],
                              "kernels_ms": run["kernels_ms"], "sync_ms": run["kernels"]["jd_par_sync"]["ms_per_decode"],
                              "write_ms": run["kernels"]["jd_par_write"]["ms_per_decode"], "stats": run["stats"]})
                print(sweep[-1], file=sys.stderr, flush=True)
    result["sweep"] = sweep
    if args.flow_frames > 1:
        rates = {True: [], False: []}
        for _ in range(args.flow_rounds):
            for parallel in (True, False):
                rates[parallel].append(child("flow", "4k", parallel, args.flow_frames, args.flow_batch))
        result["flow_source_4k"] = {"parallel_scan_frames_per_s": float(np.median([r["frames_per_s"] for r in rates[True]])),
                                    "host_route_frames_per_s": float(np.median([r["frames_per_s"] for r in rates[False]])),
                                    "parallel_scan_runs": rates[True], "host_route_runs": rates[False]}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
