#!/usr/bin/env python3
"""What a decoded frame costs up to its pixels being in device memory: the device JPEG decoder
against Pillow (libjpeg-turbo) on this machine's CPU, at 4K and 1080p, quality 90, 4:2:0, with restart intervals of 1, 8,
one MCU row, and none.

  device   JpegDecoder.decode of the file (header walk, the scan's upload, the kernels, the status): host clock around
           call and wait; and the kernels apart, from the library's own event profiler in a pass of its own.
  host     Pillow's decode of the same file to an RGB array (one CPU thread), and the upload of that array.
  check    the device's pixels are Pillow's, bit for bit.
  flow     frames/s of a Farnebäck HipFlowSource (hip_device_flows, hip_batch) over an MjpegFrameProvider of the clip,
           against the same clip as decoded arrays through ArrayFrameProvider, at the interval of 8.  Each leg runs in
           a process of its own, the two in turn, --flow-rounds times.  With --array-tree DIR the array leg runs the
           package of the built checkout at DIR -- the commit before the decoder (tools/bench_host_path.py's method:
           the frames are decoded arrays in host memory, whose upload and grey conversion are in the measured time).

    python tools/bench_jpegdec.py [--out profiles/jpegdec_bench.json] [--csv profiles/jpegdec_events.csv]
                                  [--array-tree DIR]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_jpegdec.py --kernels-only --sizes 4k    (kernel times, a run of its own)

Prints one JSON object (and writes it to --out)."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

# the tree whose package runs: this one, or for a flow leg the checkout --array-tree names (it has no decoder)
ROOT = os.environ.get("TF_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = {"4k": (2160, 3840), "1080p": (1080, 1920)}
KERNELS = ("jd_count", "jd_scan", "jd_markers", "jd_entropy", "jd_colour")


def scene(h, w, shift=0):
    """A frame with structure at every scale, so that the file has a video frame's size (about 0.25 byte a pixel)."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    xx = xx + shift
    chans = [128 + 70 * np.sin(xx / (37.0 + 9 * c)) * np.cos(yy / (29.0 + 5 * c)) + 30 * np.sin((xx + 2 * yy) / (5.0 + c)) for c in range(3)]
    return np.clip(np.stack(chans, -1) + rng.normal(0, 4, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(image, restart):
    import PIL.Image
    buf = io.BytesIO()
    opts = dict(format="JPEG", quality=90, subsampling=2)
    if restart:
        opts["restart_marker_blocks"] = restart
    PIL.Image.fromarray(image).save(buf, **opts)
    return buf.getvalue()


def pillow_decode(data, order="rgb"):
    import PIL.Image
    rgb = np.array(PIL.Image.open(io.BytesIO(data)).convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1]) if order == "bgr" else rgb


def measure(data, reps, host_reps):
    from bench_jpeg import spread
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer, sync
    from transflow_amd.jpegdec import JpegDecoder, probe
    info = probe(data)
    dec = JpegDecoder(info.width, info.height)
    pix = dec.decode(data)
    same = bool(np.array_equal(np.asarray(pix), pillow_decode(data)))
    pix.close()
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
    dec.close()
    kernels = {k: {"launches": report[k][0], "ms_per_launch": report[k][1] / report[k][0]} for k in KERNELS if k in report}
    decode_ms, upload_ms = [], []
    dev = DevBuffer(info.width * info.height * 3)
    for _ in range(host_reps):
        t0 = time.perf_counter()
        array = pillow_decode(data)
        t1 = time.perf_counter()
        dev.upload(array)
        sync()
        t2 = time.perf_counter()
        decode_ms.append((t1 - t0) * 1e3), upload_ms.append((t2 - t1) * 1e3)
    dev.close()
    out = {"file_bytes": len(data), "intervals": info.intervals, "device_per_frame_ms": spread(whole), "kernels": kernels,
           "kernels_ms": sum(v["ms_per_launch"] for v in kernels.values()), "pillow_decode_ms": spread(decode_ms),
           "upload_raw_ms": spread(upload_ms), "pixels_are_pillows": same}
    out["device_frames_per_s"] = 1e3 / out["device_per_frame_ms"]["median_ms"]
    out["pillow_over_device"] = out["pillow_decode_ms"]["median_ms"] / out["device_per_frame_ms"]["median_ms"]
    return out


def flow_leg(leg, h, w, frames, batch):
    """One leg in this process: frames/s of the flow source over the clip, the first flow (the handles) not timed."""
    from transflow_amd.config import FlowConfig
    from transflow_amd.device import sync
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    files = [encode(scene(h, w, 3 * i), 8) for i in range(frames)]
    if leg == "mjpeg":
        from transflow_amd.jpegdec import MjpegFrameProvider
        provider = MjpegFrameProvider(files)
    else:
        provider = ArrayFrameProvider([pillow_decode(f, "bgr") for f in files], 25.0)
    cfg = FlowConfig(hip_device_flows=True, hip_batch=batch)
    with HipFlowSource.from_args(provider, direction="backward", cv_config=cfg) as source:
        next(source)
        t0 = time.perf_counter()
        n = sum(1 for _ in source)
        sync()
        return n / (time.perf_counter() - t0)


def flow_rates(size, frames, batch, rounds, array_tree):
    """Both legs in child processes, in turn."""
    import subprocess
    rates = {"mjpeg": [], "array": []}
    for _ in range(rounds):
        for leg in ("mjpeg", "array"):
            env = dict(os.environ)
            cwd = None
            if leg == "array" and array_tree:
                env["TF_BENCH_TREE"] = cwd = os.path.abspath(array_tree)
            cmd = [sys.executable, os.path.abspath(__file__), "--flow-leg", leg, "--sizes", size, "--flow-frames", str(frames),
                   "--flow-batch", str(batch)]
            out = subprocess.run(cmd, env=env, cwd=cwd, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                raise RuntimeError(f"the {leg} leg failed: {out.stderr[-2000:]}")
            rates[leg].append(float(out.stdout.strip().splitlines()[-1]))
    med = lambda v: float(np.median(v))
    return {"mjpeg_provider_frames_per_s": med(rates["mjpeg"]), "array_provider_frames_per_s": med(rates["array"]),
            "mjpeg_provider_runs": rates["mjpeg"], "array_provider_runs": rates["array"],
            "array_provider_tree": "the commit before the decoder" if array_tree else "this commit", "frames": frames, "batch": batch}


def kernels_only(sizes, reps):
    """For a profiler around this process: the decodes at the encoder's default interval of 8, nothing else."""
    from transflow_amd.device import sync
    from transflow_amd.jpegdec import JpegDecoder
    for name in sizes:
        h, w = SIZES[name]
        data = encode(scene(h, w), 8)
        dec = JpegDecoder(w, h)
        for _ in range(reps):
            dec.decode(data).close()
        sync()
        dec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--csv")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sizes", default="4k,1080p")
    ap.add_argument("--flow-frames", type=int, default=17)
    ap.add_argument("--flow-batch", type=int, default=4)
    ap.add_argument("--flow-rounds", type=int, default=3)
    ap.add_argument("--array-tree", help="a built checkout of the commit before the decoder: its package runs the array leg")
    ap.add_argument("--flow-leg", choices=("mjpeg", "array"), help="(a child of this tool) one leg; prints its frames/s")
    ap.add_argument("--kernels-only", action="store_true", help="only the decodes, for a profiler around this process")
    args = ap.parse_args()
    if args.flow_leg:
        h, w = SIZES[args.sizes]
        print(flow_leg(args.flow_leg, h, w, args.flow_frames, args.flow_batch))
        return
    if args.kernels_only:
        kernels_only(args.sizes.split(","), args.reps)
        return
    import bench
    result = {"tool": "bench_jpegdec", "host": bench.host_description(), "quality": 90, "sampling": "4:2:0", "sizes": {}}
    rows = []
    for name in args.sizes.split(","):
        h, w = SIZES[name]
        image = scene(h, w)
        entry = {"height": h, "width": w, "intervals": {}}
        for label, restart in (("1", 1), ("8", 8), ("mcu_row", (w + 15) // 16), ("none", 0)):
            run = measure(encode(image, restart), args.reps if restart else max(2, args.reps // 5), args.host_reps)
            entry["intervals"][label] = run
            for k, v in run["kernels"].items():
                rows.append((name, label, k, v["launches"], v["ms_per_launch"]))
        if args.flow_frames > 1:
            entry["flow_source"] = flow_rates(name, args.flow_frames, args.flow_batch, args.flow_rounds, args.array_tree)
        result["sizes"][name] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.csv:
        with open(args.csv, "w") as f:
            f.write("size,interval,kernel,launches,ms_per_launch\n")
            for row in rows:
                f.write("%s,%s,%s,%d,%.6f\n" % row)


if __name__ == "__main__":
    main()
