#!/usr/bin/env python3
"""Motion-vector painter throughput on the GPU: prints one JSON line.

For 1080p and 4K, H.264-like vector tables (tests/mv_ref.py h264_like; a different table every frame, records
pre-converted):
- frames per second of MotionVectors.rasterize_into (host slice resolution + table upload + the two kernels, the flow
  left in device memory), the stream drained once at the end;
- HIP-event times per kernel (the library's profiler, in a separate pass so that its events do not slow the timed one);
- vectors per frame, painting rectangles, and the overlap factor (pixel writes of the paint / H*W);
- the resolve kernel's bytes (4 B winner read + 8 B flow store per pixel + 4 B winner reset per painted pixel) and the
  fraction of 8 TB/s it reaches; the paint kernel's achieved atomic bytes per second (4 B per pixel write);
- the flow source end to end (MotionVectorFlowSource over an ArrayVectorProvider, scale filter, backward): frames per
  second with host arrays and with device_flows;
- as CPU baseline, tests/mv_ref.py's painter (numpy slice assignments, as the reference's loop) on the same tables on
  this host.

Usage on the GPU box:  python tools/bench_mv.py [--quick] [--profile-only SIZE]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import mv_ref  # noqa: E402
from transflow_amd import _lib  # noqa: E402
from transflow_amd.device import DevBuffer  # noqa: E402
from transflow_amd.motionvectors import (ArrayVectorProvider, MotionVectorFlowSource, MotionVectors,  # noqa: E402
                                         stage_resolve_rects, vectors_to_records)

PEAK = 8e12   # HBM3E, bytes per second
SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}
N_TABLES = 4


def sync():
    _lib.check(_lib.load().tf_sync())


def table_stats(tables, w, h):
    vectors, painting, writes, covered = [], [], [], []
    for t in tables:
        rects, _ = stage_resolve_rects(w, h, t)
        rh, rw = np.maximum(rects[:, 1] - rects[:, 0], 0), np.maximum(rects[:, 3] - rects[:, 2], 0)
        area = rh.astype(np.int64) * rw
        vectors.append(len(t))
        painting.append(int(np.count_nonzero(area)))
        writes.append(int(area.sum()))
        covered.append(int(np.count_nonzero(mv_ref.bits(mv_ref.paint(t, w, h)).reshape(-1, 2).any(axis=1))))
    return dict(vectors_per_frame=round(statistics.mean(vectors), 1), painting_rects_per_frame=round(statistics.mean(painting), 1),
                pixel_writes_per_frame=round(statistics.mean(writes), 1),
                overlap_factor=round(statistics.mean(writes) / (w * h), 4),
                # pixels whose value has a bit set (a zero motion paints -0.0): those whose winner word is written back
                painted_fraction=round(statistics.mean(covered) / (w * h), 4),
                table_bytes_per_frame=round(statistics.mean(vectors) * 32, 1))


def rasterize_rate(mv, recs, out, frames, warmup):
    for i in range(warmup):
        mv.rasterize_into(recs[i % len(recs)], out.ptr)
    sync()
    t0 = time.perf_counter()
    for i in range(frames):
        mv.rasterize_into(recs[i % len(recs)], out.ptr)
    sync()
    dt = time.perf_counter() - t0
    return dict(frames_per_s=round(frames / dt, 1), ms_per_frame=round(1e3 * dt / frames, 4), frames=frames)


def kernel_profile(mv, recs, out, frames, stats, w, h):
    sync()
    _lib.profile(True)
    for i in range(frames):
        mv.rasterize_into(recs[i % len(recs)], out.ptr)
    sync()
    rep = _lib.profile_report()
    _lib.profile(False)
    res = {}
    for name, (count, ms) in sorted(rep.items()):
        e = dict(launches=count, ms_total=round(ms, 4), ms_per_launch=round(ms / count, 5))
        s = ms / count * 1e-3
        if name == "mv_resolve":
            b = (12 + 4 * stats["painted_fraction"]) * w * h
            e.update(bytes_per_launch=round(b), tb_per_s=round(b / s / 1e12, 3), fraction_of_8tbs=round(b / s / PEAK, 3))
        if name == "mv_paint":
            b = 4 * stats["pixel_writes_per_frame"]
            e.update(atomic_bytes_per_launch=round(b), atomic_tb_per_s=round(b / s / 1e12, 3))
        res[name] = e
    return res


def source_rate(tables, w, h, device_flows, frames):
    repeat = max(1, frames // (len(tables) - 1))
    builder = MotionVectorFlowSource.Builder(ArrayVectorProvider(tables, w, h, 30.0), device_flows=device_flows,
                                             direction="backward", flow_filters="scale=2", repeat=repeat)
    with builder as source:
        it = iter(source)
        keep = next(it)                      # the first flow makes the handles
        sync()
        n = 0
        t0 = time.perf_counter()
        for flow in it:
            keep = flow
            n += 1
        sync()
        dt = time.perf_counter() - t0
        del keep, flow
    return dict(frames_per_s=round(n / dt, 1), ms_per_frame=round(1e3 * dt / n, 4), frames=n)


def main():
    quick = "--quick" in sys.argv
    only = sys.argv[sys.argv.index("--profile-only") + 1] if "--profile-only" in sys.argv else None
    frames, warmup = (40, 8) if quick else (400, 20)
    results = {}
    for name, (w, h) in SIZES.items():
        if only and name != only:
            continue
        tables = [mv_ref.h264_like(w, h, seed=70 + i) for i in range(N_TABLES)]
        recs = [vectors_to_records(t) for t in tables]
        stats = table_stats(tables, w, h)
        mv = MotionVectors(w, h)
        out = DevBuffer(w * h * 8)
        r = dict(tables=stats)
        if only:
            rasterize_rate(mv, recs, out, 8, 2)
        else:
            r["rasterize_into"] = rasterize_rate(mv, recs, out, frames, warmup)
        r["kernels"] = kernel_profile(mv, recs, out, 8 if only else 40, stats, w, h)
        mv.close()
        out.close()
        if not only:
            r["source_host_arrays"] = source_rate(tables, w, h, False, frames // 4)
            r["source_device_flows"] = source_rate(tables, w, h, True, frames // 4)
            t0 = time.perf_counter()
            for t in tables[:2]:
                mv_ref.paint(t, w, h)
            cpu = (time.perf_counter() - t0) / 2
            r["cpu_baseline"] = dict(s_per_frame=round(cpu, 4), frames_per_s=round(1 / cpu, 2))
            r["gpu_over_cpu"] = round(r["rasterize_into"]["frames_per_s"] * cpu, 1)
        results[name] = r
    line = dict(metric="mv_rasterize_frames_per_s_4k", unit="frames/s", higher_is_better=True,
                value=results.get("4k", {}).get("rasterize_into", {}).get("frames_per_s"), results=results,
                peak_bytes_per_s=PEAK, cpu_threads=os.environ.get("OMP_NUM_THREADS"))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
