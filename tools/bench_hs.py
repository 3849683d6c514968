#!/usr/bin/env python3
"""Horn-Schunck throughput on the GPU: prints one JSON line.

- pairs per second at 1080p and 4K, for batches of 1, 8 and 32 pairs per tf_hs_calc_slots call, with delta None (every
  call runs hs_iterations iterations) and delta 1 (the convergence test runs after every iteration).  Pairs run the
  float32 chain (every pair of a flow source but its first), 3 iterations (the shipped horn-schunck.json).  The time is
  the call alone: frames and initial flows are on the device before the clock starts;
- HIP-event times per kernel (the library's profiler, in a separate pass so that its events do not slow the timed one);
- a bytes-per-pixel model of each kernel and the fraction of 8 TB/s it reaches;
- how many convergence decisions each stage of the spectral-norm test made;
- a CPU baseline: the numpy restatement of the reference's function (tests/hs_ref.py), per pair, on this host.

Usage on the GPU box:  python tools/bench_hs.py [--quick]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hs_ref  # noqa: E402
from tests.helpers import synth_pair  # noqa: E402
from transflow_amd import _lib  # noqa: E402
from transflow_amd.hornschunck import STATS_KEYS, HornSchunck  # noqa: E402

PEAK = 8e12   # HBM3E, bytes per second
# HBM bytes per pixel and launch (reads + writes; neighbours' lines are taken as cache hits)
BYTES_PER_PX = {
    "hs_prepare": 2 + 16,              # two uint8 frames in, {ex, ey, et, den} float32 out
    "hs_iterate_f32": 16 + 8 + 8,      # {ex, ey, et, den}, u and v in, u and v out
    "hs_iterate_f64": 16 + 16 + 16,
    "hs_init": 8 + 8,                  # the initial flow in, u and v out
    "hs_output": 8 + 8,                # u, v (float32 chain) in, the flow out
}
SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}
ITERS = 3


def sync():
    _lib.check(_lib.load().tf_sync())


def run_case(hs, frames, init, batch, delta, reps, warmup):
    stages = dict.fromkeys(STATS_KEYS, 0)
    times = []
    for r in range(warmup + reps):
        for p in range(batch):
            hs.set_initial_flow(p, init)
        sync()
        t0 = time.perf_counter()
        hs.calc_slots(list(range(batch)), list(range(1, batch + 1)), alpha=1, max_iters=ITERS, decay=0.95, delta=delta)
        sync()
        dt = time.perf_counter() - t0
        if r >= warmup:
            times.append(dt)
            for p in range(batch):
                for k, v in hs.last_stats(p).items():
                    stages[k] += v
    med = statistics.median(times)
    return dict(pairs_per_s=round(batch / med, 2), ms_per_call=round(1e3 * med, 3), ms_per_pair=round(1e3 * med / batch, 4),
                ms_min=round(1e3 * min(times), 3), reps=reps), stages


def kernel_profile(hs, init, batch, delta, w, h):
    for p in range(batch):
        hs.set_initial_flow(p, init)
    sync()
    _lib.profile(True)
    hs.calc_slots(list(range(batch)), list(range(1, batch + 1)), alpha=1, max_iters=ITERS, decay=0.95, delta=delta)
    sync()
    rep = _lib.profile_report()
    _lib.profile(False)
    out = {}
    for name, (count, ms) in sorted(rep.items()):
        e = dict(launches=count, ms_total=round(ms, 4), ms_per_launch=round(ms / count, 4))
        if name in BYTES_PER_PX:
            pairs = batch if name not in ("hs_init", "hs_output") else 1   # (init and output run once per pair)
            gb = BYTES_PER_PX[name] * w * h * pairs
            e["bytes_per_launch"] = gb
            e["tb_per_s"] = round(gb / (ms / count * 1e-3) / 1e12, 3)
            e["fraction_of_8tbs"] = round(gb / (ms / count * 1e-3) / PEAK, 3)
        out[name] = e
    return out


def main():
    quick = "--quick" in sys.argv
    reps, warmup = (3, 1) if quick else (7, 2)
    results, kernels, stages_all = {}, {}, {}
    for name, (w, h) in SIZES.items():
        a, b = synth_pair(h, w, seed=3, shift=(2.5, 1.5), noise=5.0)
        init = np.random.default_rng(4).normal(0, 1.0, (h, w, 2)).astype(np.float32)
        for batch in (1, 8, 32):
            hs = HornSchunck(w, h, frame_slots=batch + 1, max_pairs=batch)
            for s in range(batch + 1):
                hs.set_frame(s, a if s % 2 == 0 else b)
            for delta in (None, 1):
                key = f"{name}_b{batch}_delta{'None' if delta is None else delta}"
                results[key], stages_all[key] = run_case(hs, None, init, batch, delta, reps, warmup)
                if batch == 8 or (batch == 1 and name == "4k"):
                    kernels[key] = kernel_profile(hs, init, batch, delta, w, h)
            hs.close()
    # CPU baseline: the restatement (bit-identical to the reference's function) on this host
    cpu = {}
    for name, delta in (("1080p", 1), ("1080p", None), ("4k", None)):
        w, h = SIZES[name]
        a, b = synth_pair(h, w, seed=3, shift=(2.5, 1.5), noise=5.0)
        init = np.random.default_rng(4).normal(0, 1.0, (h, w, 2)).astype(np.float32)
        t0 = time.perf_counter()
        hs_ref.horn_schunck(a, b, init, 1, ITERS, 0.95, delta)
        cpu[f"{name}_delta{delta}"] = dict(s_per_pair=round(time.perf_counter() - t0, 3))
    cpu["4k_delta1"] = "not measured (about 3 s per iteration of numpy's SVD)"
    line = dict(metric="hs_pairs_per_s_4k_b8_delta1", value=results["4k_b8_delta1"]["pairs_per_s"], unit="pairs/s",
                higher_is_better=True, iterations=ITERS, chain="float32", results=results, kernels=kernels,
                bytes_per_px=BYTES_PER_PX, peak_bytes_per_s=PEAK, decisions=stages_all, cpu_baseline=cpu,
                cpu_threads=os.environ.get("OMP_NUM_THREADS"))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
