#!/usr/bin/env python3
"""What `hip_resident` is worth per flow for the methods whose flows used to come down raw:
Horn-Schunck (3 iterations), Lucas-Kanade (step 16 and step 4), Farnebäck with OPTFLOW_USE_INITIAL_FLOW and, where
`--lfn-weights` names a state dict on this machine, LiteFlowNet -- at 1080p and 4K, on one device, in one process.

Three routes from frames in host memory (an ArrayFrameProvider) into a HipCompositor with one moveref layer, each flow
followed by `update` and `render`:

  host      hip_resident off: the route before the key existed (the same kernels and build, switched off) -- the flow
            comes down raw, goes up, is post-processed, comes down, and the compositor takes it up again
  resident  hip_resident on, host arrays: one download per flow, the compositor takes it up again
  device    hip_resident and hip_device_flows: the compositor reads the flow where the post-process left it

One endless source (repeat=0) and one compositor per route stay open; the routes alternate window by window, `--rounds`
windows of `--flows` flows each, every window ending in a synchronise, timed by the host clock.  Medians of frames/s and
ms per flow, and the spread.

    python tools/bench_resident_methods.py [--out profiles/resident_methods_bench.json]

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
from bench_jpeg import spread  # noqa: E402
from transflow_amd.compositor import HipCompositor  # noqa: E402
from transflow_amd.config import FlowConfig, HornSchunckConfig, LayerConfig, LiteFlowNetConfig, LucasKanadeConfig  # noqa: E402
from transflow_amd.device import sync  # noqa: E402
from transflow_amd.flow import ArrayFrameProvider, HipFlowSource  # noqa: E402

SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}
ROUTES = {"host": {}, "resident": {"hip_resident": True}, "device": {"hip_resident": True, "hip_device_flows": True}}
N_FRAMES = 7


def frames_of(h, w, colour, seed=11):
    """A blocky seeded texture drifting by (3, 2) pixels a frame: grey (H, W), or BGR (H, W, 3) for LiteFlowNet."""
    rng = np.random.default_rng(seed)
    shape = (-(-h // 8), -(-w // 8)) + ((3,) if colour else ())
    base = np.kron(rng.integers(0, 256, shape, dtype=np.uint8), np.ones((8, 8) + ((1,) if colour else ()), np.uint8))[:h, :w]
    base = (base // 2 + rng.integers(0, 128, base.shape, dtype=np.uint8)).astype(np.uint8)
    return [np.ascontiguousarray(np.roll(base, (2 * i, 3 * i), (0, 1))) for i in range(N_FRAMES)]


def methods(lfn_weights):
    m = {"horn-schunck": (lambda **kw: HornSchunckConfig(hs_iterations=3, **kw), False),
         "lukas-kanade step 16": (lambda **kw: LucasKanadeConfig(lk_step=16, **kw), False),
         "lukas-kanade step 4": (lambda **kw: LucasKanadeConfig(lk_step=4, **kw), False),
         "farneback initial flow": (lambda **kw: FlowConfig(fb_flags=4, **kw), False)}
    if lfn_weights:
        m["liteflownet"] = (lambda **kw: LiteFlowNetConfig(weights=lfn_weights, **kw), True)
    return m


class Route:
    """One source, endless, and the compositor it feeds."""

    def __init__(self, h, w, frames, cfg):
        pix = np.random.default_rng(8).integers(0, 256, (h, w, 3), dtype=np.uint8)

        class Pixmap:
            introduction_mask = np.ones((h, w), bool)

            def next(self, timeout=1):
                return pix
        self.comp = HipCompositor.from_args(h, w, [LayerConfig(0)])
        self.comp.set_sources({0: [Pixmap()]})
        self.builder = HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), direction="backward", cv_config=cfg, repeat=0)
        self.source = self.builder.__enter__()

    def window(self, n):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            self.comp.update(next(self.source))
            self.comp.render()
        sync()
        return (time.perf_counter() - t0) * 1e3 / n

    def close(self):
        self.builder.__exit__(None, None, None)
        self.comp.close()


def measure(h, w, make, colour, args):
    frames = frames_of(h, w, colour)
    routes = {name: Route(h, w, frames, make(**keys)) for name, keys in ROUTES.items()}
    per_flow = {name: [] for name in routes}
    try:
        for route in routes.values():
            route.window(args.warmup)
        for _ in range(args.rounds):
            for name, route in routes.items():
                per_flow[name].append(route.window(args.flows))
    finally:
        for route in routes.values():
            route.close()
    out = {}
    for name, ms in per_flow.items():
        s = spread(ms)
        out[name] = {"per_flow_ms": s, "frames_per_s": 1e3 / s["median_ms"]}
    base = out["host"]["per_flow_ms"]["median_ms"]
    for name in ("resident", "device"):
        out[name]["speedup_over_host"] = base / out[name]["per_flow_ms"]["median_ms"]
    out["ships"] = bool(out["resident"]["speedup_over_host"] >= 1.0 and out["device"]["speedup_over_host"] > 1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--flows", type=int, default=18, help="flows per window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=8, help="flows per route before the first window")
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--methods", default="", help="comma-separated substrings of the method names to run (default: all)")
    ap.add_argument("--lfn-weights", default=os.environ.get("TFHIP_LFN_WEIGHTS"),
                    help="LiteFlowNet's state dict on this machine; without it the method is not measured")
    args = ap.parse_args()
    weights = args.lfn_weights if args.lfn_weights and os.path.isfile(args.lfn_weights) else None
    result = {"tool": "bench_resident_methods", "host": bench.host_description(), "flows_per_window": args.flows,
              "rounds": args.rounds, "warmup_flows": args.warmup, "frames": N_FRAMES, "direction": "backward",
              "each_flow": "next(source), HipCompositor.update (one moveref layer), render",
              "liteflownet": "measured" if weights else "not measured: no weights on this machine", "sizes": {}}
    wanted = [p for p in args.methods.split(",") if p]
    for size in args.sizes.split(","):
        h, w = SIZES[size]
        entry = {"height": h, "width": w, "methods": {}}
        for name, (make, colour) in methods(weights).items():
            if wanted and not any(p in name for p in wanted):
                continue
            entry["methods"][name] = measure(h, w, make, colour, args)
            print(f"{size} {name}: " + ", ".join(f"{r} {entry['methods'][name][r]['per_flow_ms']['median_ms']:.2f} ms"
                                                  for r in ROUTES), file=sys.stderr, flush=True)
        result["sizes"][size] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
