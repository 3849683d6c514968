#!/usr/bin/env python3
"""What the resident tail is worth per flow for a source with a convolution kernel or a polar filter (DESIGN.md section
10): Farnebäck (its own tail) and Horn-Schunck (3 iterations, hip_resident), BACKWARD, at 1080p and 4K, with a 5 x 5
float64 kernel and, separately, with one polar filter.

The route these configurations took before they rode the tail exists only in the parent commit, so this tool measures
across two checkouts: `--parent DIR` names a built checkout of the parent.  Every route is a worker process of this
file whose imports come from the checkout it is given:

  parent    the parent's checkout, same configuration: the raw flow comes down, goes up, is filtered / convolved in
            separate passes, comes down (float64 with the kernel), is rounded on the host and goes up again
  resident  this tree with resident_steps, host-array output: one download per flow, the compositor takes it up again
  device    this tree with resident_steps, DeviceFlow output (float64 with the kernel): nothing crosses the link

One endless source (repeat=0) and one compositor with one moveref layer per worker stay open; the driver asks the
workers for windows in turn, `--rounds` windows of `--flows` flows each (each flow: next(source), update, render), every
window ending in a synchronise and timed by the worker's host clock.  Medians and window ranges per route.  A last pass,
of its own, runs the device route under the library's event profiler and reports the new kernels' times.

    python tools/bench_resident_kernel.py --parent ../parent [--out profiles/resident_kernel_bench.json]

Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}
METHODS = ("farneback", "horn-schunck")
OPTIONS = ("kernel 5x5 f64", "polar")
POLAR = "polar=r*1.1:a+0.1"
NEW_KERNELS = ("flow_conv_tail", "flow_narrow", "flow_polar", "flow_pp")


def worker(args):
    """Serves windows from one checkout: reads `w N` / `p N` / `q` lines, answers one JSON line each."""
    sys.path.insert(0, args.root)
    import numpy as np
    from transflow_amd import _lib
    from transflow_amd.compositor import HipCompositor
    from transflow_amd.config import FlowConfig, HornSchunckConfig, LayerConfig
    from transflow_amd.device import sync
    from transflow_amd.flow import ArrayFrameProvider, HipFlowSource
    h, w = SIZES[args.size]
    rng = np.random.default_rng(11)
    base = np.kron(rng.integers(0, 256, (-(-h // 8), -(-w // 8)), dtype=np.uint8), np.ones((8, 8), np.uint8))[:h, :w]
    base = (base // 2 + rng.integers(0, 128, base.shape, dtype=np.uint8)).astype(np.uint8)
    frames = [np.ascontiguousarray(np.roll(base, (2 * i, 3 * i), (0, 1))) for i in range(7)]
    pix = np.random.default_rng(8).integers(0, 256, (h, w, 3), dtype=np.uint8)
    keys = {"hip_device_flows": True} if args.route == "device" else {}
    cfg = FlowConfig(**keys) if args.method == "farneback" else HornSchunckConfig(hs_iterations=3, hip_resident=True, **keys)
    kw = dict(direction="backward", cv_config=cfg, repeat=0)
    if args.route != "parent":
        kw["resident_steps"] = True
    if args.option == "polar":
        kw["flow_filters"] = POLAR
    else:
        kw["kernel_path"] = args.kernel

    class Pixmap:
        introduction_mask = np.ones((h, w), bool)

        def next(self, timeout=1):
            return pix
    comp = HipCompositor.from_args(h, w, [LayerConfig(0)])
    comp.set_sources({0: [Pixmap()]})
    builder = HipFlowSource.from_args(ArrayFrameProvider(frames, 25.0), **kw)
    source = builder.__enter__()

    def window(n):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            comp.update(next(source))
            comp.render()
        sync()
        return (time.perf_counter() - t0) * 1e3 / n
    print(json.dumps({"ready": True, "resident": bool(source._resident_ok())}), flush=True)
    for line in sys.stdin:
        cmd, _, n = line.strip().partition(" ")
        if cmd == "w":
            print(json.dumps({"ms": window(int(n))}), flush=True)
        elif cmd == "p":
            _lib.profile(True)
            window(int(n))
            rep = _lib.profile_report()
            _lib.profile(False)
            print(json.dumps({"kernels": {k: {"launches": c, "ms_per_launch": ms / c} for k, (c, ms) in sorted(rep.items())
                                          if any(k.startswith(p) for p in NEW_KERNELS)}}), flush=True)
        else:
            break
    builder.__exit__(None, None, None)
    comp.close()


class Worker:
    def __init__(self, root, route, size, method, option, kernel):
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--route", route,
                                      "--size", size, "--method", method, "--option", option, "--kernel", kernel],
                                     stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=root)
        self.info = self._answer()

    def _answer(self):
        line = self.proc.stdout.readline()
        if not line:
            raise RuntimeError(f"a worker ended (exit status {self.proc.wait()})")
        return json.loads(line)

    def ask(self, cmd):
        self.proc.stdin.write(cmd + "\n")
        self.proc.stdin.flush()
        return self._answer()

    def close(self):
        try:
            self.proc.stdin.write("q\n")
            self.proc.stdin.flush()
        except OSError:
            pass
        self.proc.wait(timeout=60)


def spread(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]), "min_ms": s[0],
            "max_ms": s[-1], "windows": len(s)}


def measure(args, size, method, option, kernel):
    workers = {"parent": Worker(args.parent, "parent", size, method, option, kernel)}
    try:
        workers["resident"] = Worker(HERE, "resident", size, method, option, kernel)
        workers["device"] = Worker(HERE, "device", size, method, option, kernel)
        per_flow = {name: [] for name in workers}
        for wk in workers.values():
            wk.ask(f"w {args.warmup}")
        for _ in range(args.rounds):
            for name, wk in workers.items():
                per_flow[name].append(wk.ask(f"w {args.flows}")["ms"])
        kernels = workers["device"].ask(f"p {args.flows}")["kernels"]       # a pass of its own: the events cost time
    finally:
        for wk in workers.values():
            wk.close()
    out = {name: {"per_flow_ms": spread(ms), "took_the_resident_tail": workers[name].info["resident"]}
           for name, ms in per_flow.items()}
    base = out["parent"]["per_flow_ms"]["median_ms"]
    for name in ("resident", "device"):
        out[name]["speedup_over_parent"] = base / out[name]["per_flow_ms"]["median_ms"]
    out["ships"] = bool(out["resident"]["speedup_over_parent"] >= 1.0 and out["device"]["speedup_over_parent"] > 1.0)
    out["device_route_kernels"] = kernels
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--out")
    ap.add_argument("--flows", type=int, default=12, help="flows per window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6, help="flows per route before the first window")
    ap.add_argument("--sizes", default="1080p,4k")
    for name in ("--root", "--route", "--size", "--method", "--option", "--kernel"):
        ap.add_argument(name, help=argparse.SUPPRESS)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent or not os.path.isfile(os.path.join(args.parent, "transflow_amd", "libtfhip.so")):
        ap.error("--parent must name a checkout of the parent commit with transflow_amd/libtfhip.so built")
    args.parent = os.path.abspath(args.parent)
    import numpy as np
    sys.path.insert(0, HERE)
    import bench
    result = {"tool": "bench_resident_kernel", "host": bench.host_description(), "flows_per_window": args.flows,
              "rounds": args.rounds, "warmup_flows": args.warmup, "direction": "backward", "polar_filter": POLAR,
              "each_flow": "next(source), HipCompositor.update (one moveref layer), render", "sizes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        kernel = os.path.join(tmp, "kernel.npy")
        k = np.random.default_rng(4).random((5, 5))
        np.save(kernel, k / k.sum())
        for size in args.sizes.split(","):
            h, w = SIZES[size]
            entry = {"height": h, "width": w, "cases": {}}
            for method in METHODS:
                for option in OPTIONS:
                    r = entry["cases"][f"{method}, {option}"] = measure(args, size, method, option, kernel)
                    print(f"{size} {method}, {option}: " + ", ".join(
                        f"{n} {r[n]['per_flow_ms']['median_ms']:.2f} ms" for n in ("parent", "resident", "device")),
                        file=sys.stderr, flush=True)
            result["sizes"][size] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
