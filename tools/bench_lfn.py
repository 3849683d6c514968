#!/usr/bin/env python3
"""LiteFlowNet throughput on the GPU: prints one JSON line.

- ms per pair at 854x480, 1080p and 4K, in calls of 1 and 4 pairs (tf_lfn_calc_slots; the frames are in their slots
  beforehand, the flows stay on the device).  Synthetic weights (tests/lfn_ref.synthetic_weights): the time does not
  depend on their values;
- HIP-event times per kernel label (the library's profiler, in a separate pass so that its events do not slow the
  timed one), and, per convolution class, the FLOPs of one call (2 Cin Cout kh kw Hout Wout per layer), the achieved
  TFLOP/s and its fraction of the MFMA peak of the precision's kernel (f32: 157.3 TF; bf16 and bf16x3: 2500 TF, the
  FLOPs of bf16x3 counted once);
- the only CPU figure: the float32 torch-CPU restatement (tests/lfn_ref.py) on 16 threads at 854x480.  The reference
  itself cannot run on this GPU (its correlation is CuPy CUDA code).

--precision f32 | bf16 | bf16x3 runs the handle in that mode (tf_lfn_set_precision; f32, the default, prints what it
always did).  tools/bench_lfn_precision.py compares the three in one run.

Usage on the GPU box:  python tools/bench_lfn.py [--quick] [--precision NAME] [--profile-only SIZE]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lfn_ref  # noqa: E402
from transflow_amd import _lib  # noqa: E402
from transflow_amd import liteflownet as LF  # noqa: E402

SIZES = {"854x480": (854, 480), "1080p": (1920, 1080), "4k": (3840, 2160)}
PEAK_TF = 157.3
PEAKS_TF = {"f32": PEAK_TF, "bf16": 2500.0, "bf16x3": 2500.0}
CLASSES = ("lfn_conv7x7", "lfn_conv3x3_s1", "lfn_conv3x3_s2", "lfn_conv1x1", "lfn_conv_kx1", "lfn_conv_1xk",
           "lfn_conv_head", "lfn_conv_dist")


def sync():
    _lib.check(_lib.load().tf_sync())


def conv_class(l):
    """The profiler label liteflownet.hip gives a layer (lfn_common.h make_net)."""
    if l.cout == 2:
        return "lfn_conv_head"
    if l.kh == 1 and l.kw == 1:
        return "lfn_conv1x1"
    if l.kw == 1:
        return "lfn_conv_kx1"
    if l.kh == 1:
        return "lfn_conv_1xk"
    if l.kh == 7 and l.cin == 3:
        return "lfn_conv7x7"
    if l.cout == l.kh * l.kw:
        return "lfn_conv_dist"
    return "lfn_conv3x3_s2" if l.stride == 2 else "lfn_conv3x3_s1"


def flops_per_pair(w, h):
    """{class: FLOPs} of one pair as the driver runs it (both frames' features; level 2's netFeat on both frames for
    Matching and Subpixel; netScale is part of the tail kernel, not a convolution)."""
    wp, hp = LF.padded_size(w, h)
    out = {c: 0 for c in CLASSES}
    layers = {l.name: l for l in LF.layers()}

    def add(name, hin, win, images):
        l = layers[name]
        ho, wo = l.out_size(hin, win)
        out[conv_class(l)] += 2 * l.cin * l.cout * l.kh * l.kw * ho * wo * images

    feats = [("netOne.0", 0), ("netTwo.0", 0), ("netTwo.2", 1), ("netTwo.4", 1), ("netThr.0", 1), ("netThr.2", 2),
             ("netFou.0", 2), ("netFou.2", 3), ("netFiv.0", 3), ("netSix.0", 4)]
    for name, j in feats:
        add("netFeatures." + name, hp >> j, wp >> j, 2)
    for i, lv in enumerate(LF.LEVELS):
        hh, ww = hp >> (lv - 1), wp >> (lv - 1)
        for p in (f"netMatching.{i}", f"netSubpixel.{i}"):
            if lv == 2:
                add(p + ".netFeat.0", hh, ww, 2)
            for j in range(4):
                add(p + f".netMain.{2 * j}", hh, ww, 1)
        p = f"netRegularization.{i}"
        if lv < 5:
            add(p + ".netFeat.0", hh, ww, 1)
        for j in range(6):
            add(p + f".netMain.{2 * j}", hh, ww, 1)
        add(p + ".netDist.0", hh, ww, 1)
        if lv < 5:
            add(p + ".netDist.1", hh, ww, 1)
    return out


def frames_for(w, h, n):
    return [lfn_ref.textured_pair(h, w, 11 + i, (2, 3))[i % 2] for i in range(n)]


def run_case(net, batch, reps, warmup):
    times = []
    for r in range(warmup + reps):
        sync()
        t0 = time.perf_counter()
        net.calc_slots(list(range(batch)), list(range(1, batch + 1)))
        sync()
        if r >= warmup:
            times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    return dict(ms_per_call=round(1e3 * med, 3), ms_per_pair=round(1e3 * med / batch, 3),
                ms_min_per_pair=round(1e3 * min(times) / batch, 3), reps=reps)


def kernel_profile(net, batch, w, h, peak_tf=PEAK_TF):
    net.calc_slots(list(range(batch)), list(range(1, batch + 1)))
    sync()
    _lib.profile(True)
    net.calc_slots(list(range(batch)), list(range(1, batch + 1)))
    sync()
    rep = _lib.profile_report()
    _lib.profile(False)
    kernels = {name: dict(launches=c, ms_total=round(ms, 4)) for name, (c, ms) in sorted(rep.items())}
    for c in CLASSES:          # the bf16 kernel labels its launches that gather with 128-bit loads `<class>_v`
        if c + "_v" in rep:
            rep[c] = tuple(a + b for a, b in zip(rep.get(c, (0, 0.0)), rep.pop(c + "_v")))
    fl = flops_per_pair(w, h)
    classes = {}
    for c in CLASSES:
        if c in rep and fl[c]:
            ms = rep[c][1]
            tf = fl[c] * batch / (ms * 1e-3) / 1e12
            classes[c] = dict(gflop_per_pair=round(fl[c] / 1e9, 2), ms=round(ms, 3), tflops=round(tf, 2),
                              fraction_of_peak=round(tf / peak_tf, 3 if peak_tf == PEAK_TF else 4))
    total_ms = sum(ms for _, ms in rep.values())
    return dict(kernels=kernels, conv_classes=classes, kernel_ms_total=round(total_ms, 3),
                tflop_per_pair=round(sum(fl.values()) / 1e12, 4))


def cpu_figure():
    import torch
    torch.set_num_threads(16)
    w, h = SIZES["854x480"]
    W = lfn_ref.synthetic_weights(1, 0.25)[0]
    one, two = lfn_ref.textured_pair(h, w, 11, (2, 3))
    t0 = time.perf_counter()
    lfn_ref.estimate(W, one, two, torch.float32)
    return dict(impl="float32 torch-CPU restatement tests/lfn_ref.py, 16 threads (the reference cannot run on this GPU)",
                size="854x480", ms_per_pair=round(1e3 * (time.perf_counter() - t0), 1))


def profile_only(name, calls=3, precision="f32"):
    """A few calls of one pair at SIZES[name], for a profiler run of its own (rocprofv3 --kernel-trace --stats)."""
    w, h = SIZES[name]
    net = LF.LiteFlowNet(w, h, LF.pack_weights(lfn_ref.synthetic_weights(1, 0.25)[0]), device=0, precision=precision)
    for s, f in enumerate(frames_for(w, h, 2)):
        net.set_frame_bgr(s, f)
    for _ in range(calls):
        net.calc_slots([0], [1])
    sync()
    net.close()


def main():
    precision = sys.argv[sys.argv.index("--precision") + 1] if "--precision" in sys.argv else "f32"
    LF.precision_code(precision)
    if "--profile-only" in sys.argv:
        return profile_only(sys.argv[sys.argv.index("--profile-only") + 1], precision=precision)
    quick = "--quick" in sys.argv
    W = lfn_ref.synthetic_weights(1, 0.25)[0]
    blob = LF.pack_weights(W)
    out = dict(bench="liteflownet", peak_tflops=PEAKS_TF[precision], results={}, kernels={})
    if precision != "f32":
        out["precision"] = precision
    for name, (w, h) in SIZES.items():
        batches = (1, 4)
        net = LF.LiteFlowNet(w, h, blob, frame_slots=5, max_pairs=4, device=0, precision=precision)
        for s, f in enumerate(frames_for(w, h, 5)):
            net.set_frame_bgr(s, f)
        for batch in batches:
            reps = 2 if quick else (3 if name == "4k" else 5)
            out["results"][f"{name}_b{batch}"] = run_case(net, batch, reps, 1)
        out["kernels"][f"{name}_b1"] = kernel_profile(net, 1, w, h, PEAKS_TF[precision])
        net.close()
    out["cpu"] = cpu_figure()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
