#!/usr/bin/env python3
"""Lucas-Kanade throughput on the GPU: prints one JSON line.

- ms per pair at 1080p and 4K, for lk_step 1, 4 and 16 (window 15, maxLevel 2: the reference's defaults and its two
  shipped configs), for batches of 1, 8 and 32 pairs per tf_lk_calc_slots call.  The time is the whole call: every
  frame was uploaded just before (so its pyramid and derivatives are built inside the call), the flows stay on the
  device;
- HIP-event times per kernel (the library's profiler, in a separate pass so that its events do not slow the timed one);
- the mean and max number of steps (iterations) per point at each level, from a pass with the counters on;
- a CPU figure: the numpy restatement (tests/lk_ref.py) on a small frame -- numpy, not OpenCV.

Usage on the GPU box:  python tools/bench_lk.py [--quick]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lk_ref  # noqa: E402
from tests.helpers import synth_pair  # noqa: E402
from transflow_amd import _lib  # noqa: E402
from transflow_amd.lucaskanade import LucasKanade  # noqa: E402

SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}
WIN, LEVELS = 15, 2


def sync():
    _lib.check(_lib.load().tf_sync())


def frames_for(w, h, n):
    a, b = synth_pair(h, w, seed=11, shift=(4.0, 3.0), noise=4.0)
    return [a if i % 2 == 0 else b for i in range(n)]


def run_case(lk, frames, batch, step, reps, warmup):
    times = []
    for r in range(warmup + reps):
        for s in range(batch + 1):
            lk.set_frame(s, frames[s])          # fresh frames: the call builds every pyramid it needs
        sync()
        t0 = time.perf_counter()
        lk.calc_slots(list(range(batch)), list(range(1, batch + 1)), WIN, LEVELS, step)
        sync()
        if r >= warmup:
            times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    return dict(ms_per_call=round(1e3 * med, 3), ms_per_pair=round(1e3 * med / batch, 3),
                ms_min_per_pair=round(1e3 * min(times) / batch, 3), reps=reps)


def kernel_profile(lk, frames, batch, step):
    for s in range(batch + 1):
        lk.set_frame(s, frames[s])
    sync()
    _lib.profile(True)
    lk.calc_slots(list(range(batch)), list(range(1, batch + 1)), WIN, LEVELS, step)
    sync()
    rep = _lib.profile_report()
    _lib.profile(False)
    return {name: dict(launches=c, ms_total=round(ms, 4), ms_per_launch=round(ms / c, 4))
            for name, (c, ms) in sorted(rep.items())}


def iteration_stats(lk, frames, step, w, h):
    lk.set_frame(0, frames[0])
    lk.set_frame(1, frames[1])
    lk.calc_slots([0], [1], WIN, LEVELS, step, stats=True)
    n = len(range(0, w, step)) * len(range(0, h, step))
    return [dict(level=l, mean=round(s / n, 4), max=m) for l, (s, m) in enumerate(lk.last_stats(0))]


def cpu_figure():
    h, w = 120, 160
    a, b = synth_pair(h, w, seed=11, shift=(4.0, 3.0), noise=4.0)
    t0 = time.perf_counter()
    lk_ref.lukas_kanade(a, b, WIN, LEVELS, 1)
    return dict(impl="numpy restatement tests/lk_ref.py (not OpenCV)", size=f"{w}x{h}", step=1,
                ms_per_pair=round(1e3 * (time.perf_counter() - t0), 1))


def main():
    quick = "--quick" in sys.argv
    batches = (1, 8) if quick else (1, 8, 32)
    out = dict(bench="lucas_kanade", win_size=WIN, max_level=LEVELS, results={}, kernels={}, iterations={})
    for name, (w, h) in SIZES.items():
        lk = LucasKanade(w, h, frame_slots=max(batches) + 1, max_pairs=max(batches), device=0)
        frames = frames_for(w, h, max(batches) + 1)
        for step in (1, 4, 16):
            for batch in batches:
                reps = 3 if batch * w * h / step ** 2 > 8 * 3840 * 2160 else 5
                out["results"][f"{name}_step{step}_b{batch}"] = run_case(lk, frames, batch, step, reps, 1)
            out["kernels"][f"{name}_step{step}_b8"] = kernel_profile(lk, frames, 8, step)
            out["iterations"][f"{name}_step{step}"] = iteration_stats(lk, frames, step, w, h)
        lk.close()
    out["cpu"] = cpu_figure()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
