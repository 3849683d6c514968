#!/usr/bin/env python3
"""What a random reset's field costs, drawn on the device from numpy's stream (rng="mt19937", transflow_amd/mtstream.py)
and on the host (rng="numpy"), at 1080p and 4K on one GPU.

  (a) the device field: tf_mt_random_sample_dev of H * W doubles, the fill and jump kernels together, by device events
      over windows of `--reps` draws after a warm-up; the two kernels apart from the library's event profiler in a pass of
      its own; the one-time bootstrap (tf_mt_info) apart.  The first field is compared with RandomState's, every double.
  (b) the host route, same run, same box: numpy.random.random((H, W)) by the host clock, and the float64 field's upload
      from pageable memory as tf_remap_update does it (a queued copy and a synchronise).  Their sum is the comparand.
  (c) a compositor of one moveref layer with random reset over DeviceFlows: frames/s of update() + render() with rng
      "numpy", "mt19937" and "device" ("device" is another generator: what parity with numpy costs).
  (d) the mt_segments sweep behind the default.

    python tools/bench_mt_reset.py [--out profiles/mt_reset_bench.json]

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
from transflow_amd import _lib  # noqa: E402
from transflow_amd.compositor import HipCompositor  # noqa: E402
from transflow_amd.config import LayerConfig  # noqa: E402
from transflow_amd.device import DevBuffer, sync  # noqa: E402
from transflow_amd.deviceflow import DeviceFlow  # noqa: E402
from transflow_amd.mtstream import Mt19937, Mt19937Stream  # noqa: E402

SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}
SWEEP = [0, 64, 128, 256, 512, 1024, 2048, 4096]


def device_windows(mt, out, n, reps, rounds, events):
    dev = []
    for _ in range(rounds):
        events.start()
        for _ in range(reps):
            mt.random_sample_dev(out.ptr, n)
        dev.append(events.stop_ms() / reps)
    return spread(dev)


def device_field(h, w, args, events):
    n = h * w
    out = DevBuffer(8 * n)
    mt = Mt19937()
    rs = np.random.RandomState(1)
    mt.set_state(*rs.get_state()[1:3])
    mt.random_sample_dev(out.ptr, n)                        # the bootstrap and the first field
    same = bool((out.download((n,), np.uint64) == rs.random_sample(n).view(np.uint64)).all())
    info = mt.info()
    for _ in range(3):
        mt.random_sample_dev(out.ptr, n)
    sync()
    # the stream is still numpy's after draws from jumped states
    key, pos = mt.get_state()
    fresh = np.random.RandomState(0)
    fresh.set_state(("MT19937", key, pos))
    for _ in range(3):
        rs.random_sample(n)
    still = bool((fresh.random_sample(1000) == rs.random_sample(1000)).all())
    run = {"segments": info["segments"], "segment_words": info["segment_words"], "bootstrap_ms": info["bootstrap_ms"],
           "first_field_equals_numpy": same, "state_after_four_fields_equals_numpy": still,
           "per_field_device_events_ms": device_windows(mt, out, n, args.reps, args.rounds, events)}
    _lib.profile(True, "mt_")
    for _ in range(args.reps):
        mt.random_sample_dev(out.ptr, n)
    sync()
    report = _lib.profile_report()
    _lib.profile(False)
    run["kernels"] = {label: {"launches": cnt, "ms_per_launch": ms / cnt} for label, (cnt, ms) in report.items() if cnt}
    sweep = {}
    for g in SWEEP:
        _lib.set_option("mt_segments", g)
        mt.random_sample_dev(out.ptr, n)                    # re-derives the segments' states
        mt.random_sample_dev(out.ptr, n)
        sync()
        sweep[str(g)] = dict(device_windows(mt, out, n, args.reps, 3, events), segments=mt.info()["segments"],
                             bootstrap_ms=mt.info()["bootstrap_ms"])
    _lib.set_option("mt_segments", 0)
    run["mt_segments_sweep"] = sweep
    mt.close(), out.close()
    return run


def host_route(h, w, args):
    out = DevBuffer(8 * h * w)
    draw, up = [], []
    for _ in range(args.host_reps + 1):
        t0 = time.perf_counter()
        u = np.random.random((h, w))
        t1 = time.perf_counter()
        out.upload(u)                                       # queued from pageable memory, then a synchronise
        t2 = time.perf_counter()
        draw.append((t1 - t0) * 1e3), up.append((t2 - t1) * 1e3)
    out.close()
    both = [a + b for a, b in zip(draw[1:], up[1:])]
    return {"numpy_random_ms": spread(draw[1:]), "field_upload_ms": spread(up[1:]), "per_field_ms": spread(both), "bytes": 8 * h * w}


def compositor_rate(h, w, rng, frames):
    gen = np.random.default_rng(3)
    flow = np.clip(gen.normal(0, 2, (h, w, 2)), -3, 3).astype(np.float32)
    flow[:4], flow[-4:], flow[:, :4], flow[:, -4:] = 0, 0, 0, 0          # no rounded vector leaves the frame
    pix = gen.integers(0, 256, (h, w, 3), dtype=np.uint8)

    class Source:
        introduction_mask = np.ones((h, w), bool)

        def next(self, timeout=1):
            return pix

    buf = DevBuffer.from_array(flow)
    dflow = DeviceFlow(flow.shape, buf.ptr, None, owner=buf)
    dflow.in_frame = True
    comp = HipCompositor.from_args(h, w, [LayerConfig(0, reset_mode="random", reset_random_factor=0.05)], rng=rng)
    comp.set_sources({0: [Source()]})
    np.random.seed(2)
    for _ in range(3):
        comp.update(dflow)
        comp.render()
    sync()
    t0 = time.perf_counter()
    for _ in range(frames):
        comp.update(dflow)
        comp.render()
    sync()
    dt = time.perf_counter() - t0
    comp.close(), buf.close()
    return {"frames": frames, "frames_per_s": frames / dt, "ms_per_frame": dt * 1e3 / frames}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=8)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--sizes", default="1080p,4k")
    args = ap.parse_args()
    events = Events()
    result = {"tool": "bench_mt_reset", "host": bench.host_description(), "reps": args.reps, "rounds": args.rounds, "sizes": {}}
    for name in args.sizes.split(","):
        h, w = SIZES[name]
        entry = {"height": h, "width": w, "device_field": device_field(h, w, args, events), "host_route": host_route(h, w, args)}
        entry["device_over_host"] = (entry["device_field"]["per_field_device_events_ms"]["median_ms"]
                                     / entry["host_route"]["per_field_ms"]["median_ms"])
        entry["compositor"] = {rng: compositor_rate(h, w, rng, args.frames) for rng in ("numpy", "mt19937", "device")}
        result["sizes"][name] = entry
    if Mt19937Stream._instance is not None:
        Mt19937Stream._instance.close()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
