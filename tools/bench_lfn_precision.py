#!/usr/bin/env python3
"""LiteFlowNet's precision modes against each other on the GPU: prints one JSON line (profiles/lfn_precision_bench.json).

One handle per size (854x480, 1080p, 4K); for calls of 1 and 4 pairs the legs f32, bf16, bf16x3 and f32 again run in
turn, round after round, so that every mode sees the same clocks and the same neighbours; the second f32 leg measures
the run-to-run spread the modes' gains have to exceed.  Per leg: the median and the minimum over the rounds of the
whole call's wall time (tf_lfn_calc_slots to tf_sync), in ms per pair.  Then, per mode at 1080p and one pair, the
library profiler's time per convolution class and the achieved TFLOP/s (the FLOPs of bf16x3 counted once) against the
peak of the mode's MFMA.

Usage on the GPU box:  python tools/bench_lfn_precision.py [--rounds N] [--profile-only 1080p]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lfn_ref  # noqa: E402
from tools import bench_lfn as B  # noqa: E402
from transflow_amd import liteflownet as LF  # noqa: E402

LEGS = (("f32", "f32"), ("bf16", "bf16"), ("bf16x3", "bf16x3"), ("f32_again", "f32"))


def one_call(net, batch):
    B.sync()
    t0 = time.perf_counter()
    net.calc_slots(list(range(batch)), list(range(1, batch + 1)))
    B.sync()
    return time.perf_counter() - t0


def compare(net, batch, rounds):
    for _, mode in LEGS[:3]:                      # warm-up: every mode once (the bf16 planes are made here)
        net.set_precision(mode)
        one_call(net, batch)
    times = {leg: [] for leg, _ in LEGS}
    for _ in range(rounds):
        for leg, mode in LEGS:
            net.set_precision(mode)
            times[leg].append(one_call(net, batch))
    out = {leg: dict(ms_per_pair=round(1e3 * statistics.median(t) / batch, 3), ms_min_per_pair=round(1e3 * min(t) / batch, 3),
                     ms_max_per_pair=round(1e3 * max(t) / batch, 3)) for leg, t in times.items()}
    a, b = out["f32"]["ms_per_pair"], out["f32_again"]["ms_per_pair"]
    out["f32_spread"] = round(abs(a - b) / min(a, b), 4)
    for leg in ("bf16", "bf16x3"):
        out[leg]["speedup_over_f32"] = round(min(a, b) / out[leg]["ms_per_pair"], 3)
    out["rounds"] = rounds
    return out


def profile_only(name):
    """Three calls of one pair per mode at SIZES[name], for a profiler run of its own."""
    w, h = B.SIZES[name]
    net = LF.LiteFlowNet(w, h, LF.pack_weights(lfn_ref.synthetic_weights(1, 0.25)[0]), device=0)
    for s, f in enumerate(B.frames_for(w, h, 2)):
        net.set_frame_bgr(s, f)
    for _, mode in LEGS[:3]:
        net.set_precision(mode)
        for _ in range(3):
            net.calc_slots([0], [1])
    B.sync()
    net.close()


def main():
    if "--profile-only" in sys.argv:
        return profile_only(sys.argv[sys.argv.index("--profile-only") + 1])
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    blob = LF.pack_weights(lfn_ref.synthetic_weights(1, 0.25)[0])
    out = dict(bench="liteflownet_precision", peaks_tflops=B.PEAKS_TF, results={}, kernels={})
    for name, (w, h) in B.SIZES.items():
        net = LF.LiteFlowNet(w, h, blob, frame_slots=5, max_pairs=4, device=0)
        for s, f in enumerate(B.frames_for(w, h, 5)):
            net.set_frame_bgr(s, f)
        for batch in (1, 4):
            out["results"][f"{name}_b{batch}"] = compare(net, batch, rounds)
        if name == "1080p":
            for _, mode in LEGS[:3]:
                net.set_precision(mode)
                out["kernels"][f"{name}_b1_{mode}"] = B.kernel_profile(net, 1, w, h, B.PEAKS_TF[mode])
        net.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
