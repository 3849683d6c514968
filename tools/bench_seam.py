#!/usr/bin/env python3
"""Times the main loop's steps between the flow sources and the compositor with and without
dropin.install(device_seam=True): writes profiles/seam_bench.json.

    python tools/bench_seam.py [--repeats 9] [--warmup 3] [--out profiles/seam_bench.json]

Three workloads, each a DeviceFlow going through the pipeline's own names (a stand-in pipeline module where no
transflow is importable, with oracle/flow_ops_ref.py's numpy statements standing where the reference's functions do --
its upscale is two numpy.repeat, cheaper than the reference's numpy.kron, so the host route is not overstated):

  upscale   1920x1080 -> 3840x2160 (`upscale_array(flow, 2, 2)`), into a 4K moveref compositor: update + render
  merge     two 4K flows merged by `sum`, into the same compositor: update + render
  view      the 4K magnitude view: the expression of pipeline.py:515 and `render1d`

The device route and the host route (the same calls without the option: what the parent commit does) are timed in one
run, alternating, after a warm-up; the JSON holds every repeat, the median and the spread (max - min) of each route.
For k_flow_seam it also holds bytes moved (from the shapes) over the kernel's time, beside a tf_dev_copy that moves
as many bytes, timed in the same run.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pipeline_module():
    """The reference's pipeline module if one is importable, else a stand-in with the names the option replaces."""
    try:
        import transflow.pipeline as module
        return module, "transflow"
    except ImportError:
        pass
    from oracle import flow_ops_ref as F
    package, module = types.ModuleType("transflow"), types.ModuleType("transflow.pipeline")
    package.pipeline, package.__path__ = module, []
    module.upscale_array = F.upscale
    module.render1d = lambda arr, scale=1, colors=None, binary=False: F.render1d(arr, scale, colors or ("#000000", "#ffffff"), binary)
    module.render2d = lambda arr, scale=1, colors=None: F.render2d(arr, scale, colors or ("#ffff00", "#0000ff", "#ff00ff", "#00ff00"))

    class Pipeline:
        FLOW_MERGING_FUNCTIONS = {k: (lambda flows, k=k: F.merge(k, flows)) for k in
                                  ("first", "sum", "average", "difference", "product", "maskbin", "masklin", "absmax")}

    module.Pipeline = Pipeline
    sys.modules["transflow"], sys.modules["transflow.pipeline"] = package, module
    return module, "stand-in (oracle/flow_ops_ref.py)"


def in_frame_flow(h, w, seed, sigma=2.5):
    """A float32 flow no rounded vector of which leaves the frame (what a source's post_process hands on)."""
    f = np.random.default_rng(seed).normal(0, sigma, (h, w, 2)).astype(np.float32)
    j, i = np.arange(w, dtype=np.float32)[None, :], np.arange(h, dtype=np.float32)[:, None]
    f[:, :, 0] = np.clip(f[:, :, 0], -j, w - 1 - j)
    f[:, :, 1] = np.clip(f[:, :, 1], -i, h - 1 - i)
    return f


def device_flow(array, in_frame):
    from transflow_amd.device import DevBuffer
    from transflow_amd.deviceflow import DeviceFlow, _Event
    buf = DevBuffer.from_array(array)
    ev = _Event()
    ev.record()
    flow = DeviceFlow(array.shape, buf.ptr, ev, owner=buf)
    flow.in_frame = in_frame
    return flow


class HostSource:
    def __init__(self, array, mask):
        self.array, self.introduction_mask, self.frame_number = array, mask, 0

    def next(self, timeout=1):
        return self.array


def summary(times):
    return {"median_ms": statistics.median(times) * 1e3, "spread_ms": (max(times) - min(times)) * 1e3,
            "repeats_ms": [t * 1e3 for t in times]}


def kernel_rates(repeats):
    """k_flow_seam on the two shapes of the workloads, and tf_dev_copy moving as many bytes."""
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer, sync
    lib = _lib.load()
    out = {}
    for name, (h, w, wf, hf, n, kind) in (("upscale_1080p_x2", (1080, 1920, 2, 2, 1, 0)), ("merge_sum_4k_n2", (2160, 3840, 1, 1, 2, 1))):
        ins = [DevBuffer.from_array(in_frame_flow(h, w, s)) for s in range(n)]
        dst = DevBuffer(8 * h * hf * w * wf)
        moved = 8 * h * w * n + dst.nbytes
        src = DevBuffer(moved // 2)
        cpy = DevBuffer(moved // 2)
        ptrs = (C.c_void_p * n)(*[b.ptr for b in ins])
        calls = 20

        def seam():
            for _ in range(calls):
                _lib.check(lib.tf_flow_seam_dev(kind, n, ptrs, w, h, wf, hf, C.c_void_p(dst.ptr)))

        def copy():
            for _ in range(calls):
                _lib.check(lib.tf_dev_copy(C.c_void_p(cpy.ptr), C.c_void_p(src.ptr), moved // 2))

        times = {"seam": [], "copy": []}
        for r in range(repeats + 2):
            for key, fn in (("seam", seam), ("copy", copy)):
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                if r >= 2:
                    times[key].append((time.perf_counter() - t0) / calls)
        out[name] = {"bytes_moved": moved,
                     "k_flow_seam": dict(summary(times["seam"]), gb_per_s=moved / statistics.median(times["seam"]) / 1e9),
                     "tf_dev_copy": dict(summary(times["copy"]), gb_per_s=moved / statistics.median(times["copy"]) / 1e9)}
        for b in ins + [dst, src, cpy]:
            b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seam_bench.json"))
    args = ap.parse_args()
    module, which = pipeline_module()
    from transflow_amd import deviceflow, dropin
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import LayerConfig
    from transflow_amd.device import sync
    H, W = 2160, 3840
    comp = HipCompositor.from_args(H, W, [LayerConfig(0)])
    comp.set_sources({0: [HostSource(np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8), np.ones((H, W), bool))]})
    small = in_frame_flow(H // 2, W // 2, 2)
    halves = [in_frame_flow(H, W, s) * np.float32(0.5) for s in (3, 4)]       # their sum stays in the frame
    full = in_frame_flow(H, W, 5)

    # the host route's functions are the ones the option finds; the device route's the ones it leaves (installed once:
    # the view's image and its page-locked frames are made at the first view, as in a run of the pipeline)
    merging = module.Pipeline.FLOW_MERGING_FUNCTIONS
    names = {"host": (module.upscale_array, module.render1d, merging["sum"])}
    dropin.install(flow=False, compositor=False, device_seam=True)
    names["device"] = (module.upscale_array, module.render1d, merging["sum"])

    def upscale(fn, flow):
        flow = fn[0](flow, 2, 2)
        comp.update(flow)
        return comp.render()

    def merge(fn, flows):
        flow = fn[2](flows)
        comp.update(flow)
        return comp.render()

    def view(fn, flow):
        mag = np.sqrt(np.sum(np.power(flow, 2), axis=2))                      # pipeline.py:515
        return np.asarray(fn[1](mag, 0.1, None, False))                       # :516

    # (what a workload is given: fresh DeviceFlows, as a source yields them -- made before the clock starts)
    workloads = {"upscale": (lambda: device_flow(small, True), upscale),
                 "merge": (lambda: [device_flow(a, True) for a in halves], merge),
                 "view": (lambda: device_flow(full, True), view)}
    times = {name: {"device": [], "host": []} for name in workloads}
    try:
        for r in range(args.warmup + args.repeats):
            for route in ("device", "host"):
                deviceflow.DEVICE_VIEW = route == "device"       # off, numpy.power of a flow is numpy's: the parent's behaviour
                for name, (prepare, run) in workloads.items():
                    given = prepare()
                    sync()
                    t0 = time.perf_counter()
                    run(names[route], given)
                    if r >= args.warmup:
                        times[name][route].append(time.perf_counter() - t0)
    finally:
        dropin.uninstall()
    result = {"pipeline_functions": which, "frame": [H, W], "warmup": args.warmup, "repeats": args.repeats, "workloads": {}}
    ok = True
    for name in workloads:
        d, h = summary(times[name]["device"]), summary(times[name]["host"])
        beats = h["median_ms"] - d["median_ms"] > max(d["spread_ms"], h["spread_ms"])
        ok = ok and beats
        result["workloads"][name] = {"device": d, "host": h, "speedup": h["median_ms"] / d["median_ms"],
                                     "device_beats_host_by_more_than_the_spread": beats}
    result["kernel"] = kernel_rates(args.repeats)
    comp.close()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    for name, w in result["workloads"].items():
        print(f"{name}: device {w['device']['median_ms']:.2f} ms (spread {w['device']['spread_ms']:.2f}), "
              f"host {w['host']['median_ms']:.2f} ms (spread {w['host']['spread_ms']:.2f}), x{w['speedup']:.1f}")
    for name, k in result["kernel"].items():
        print(f"{name}: k_flow_seam {k['k_flow_seam']['gb_per_s']:.0f} GB/s, tf_dev_copy {k['tf_dev_copy']['gb_per_s']:.0f} GB/s "
              f"({k['bytes_moved']} bytes)")
    if not ok:
        raise SystemExit("the device route does not beat the host route by more than the spread in every workload")


if __name__ == "__main__":
    main()
