#!/usr/bin/env python3
"""The post-process of one checkout, for comparing two of them in alternation:
    python tools/bench_postprocess.py <checkout root> <out.json> [mem]
Kernel times at 3840x2160 from tf_prof events (the float2 kernels through a Farneback(levels=0) handle with one scale
filter and a mask, the float64 ones through tf_flow_post_process_dev), FlowSource.post_process per frame on a host
array for a Horn-Schunck source (one scale filter, a mask, both directions, 1080p and 4K), and with `mem` the device
memory such a source holds at 4K after its first flow, read with hipMemGetInfo.  Uses only what both a checkout with
and one without flowops.PostProcess offer."""
import ctypes as C
import json
import os
import statistics
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
os.chdir(root)
import numpy as np  # noqa: E402

from transflow_amd import _lib  # noqa: E402
from transflow_amd._lib import check  # noqa: E402
from transflow_amd.device import DevBuffer, sync  # noqa: E402
from transflow_amd.farneback import Farneback  # noqa: E402

lib = _lib.load()
check(lib.tf_init(0))
assert os.path.abspath(_lib.__file__).startswith(root), _lib.__file__
P = C.c_void_p
out = {"tree": root}
rng = np.random.default_rng(3)


def prof(fn, reps):
    fn()
    sync()
    check(lib.tf_prof_reset())
    check(lib.tf_prof_set_filter(None))
    check(lib.tf_prof_enable(1))
    for _ in range(reps):
        fn()
    sync()
    check(lib.tf_prof_enable(0))
    buf = C.create_string_buffer(1 << 16)
    check(lib.tf_prof_report(buf, len(buf)))
    res = {}
    for line in buf.value.decode().splitlines():
        name, n, ms = line.split()
        res[name] = 1e3 * float(ms) / int(n)          # us per launch
    return res


W, H = 3840, 2160
N = W * H
flow = rng.normal(0, 3, (H, W, 2)).astype(np.float32)
pristine = DevBuffer.from_array(flow)
mask = DevBuffer.from_array(rng.random((H, W)).astype(np.float32))
fb = Farneback(W, H, levels=0)
k = {}
for direction in (1, 0):
    def step(direction=direction):
        check(lib.tf_dev_copy(P(fb.flow_ptr(0)), P(pristine.ptr), flow.nbytes))
        fb.post_process_ex(0, direction, [("scale", 1.5)], mask.ptr)
    r = prof(step, 20)
    for name, us in r.items():
        k[f"{name}{'' if name != 'pp_ops' else ('_bwd' if direction else '_fwd')}"] = us
fb.close()
wide = DevBuffer.from_array(flow.astype(np.float64))
work, scr = DevBuffer(N * 16), DevBuffer(N * 4)
for direction, label in ((1, "f64 BACKWARD"), (0, "f64 FORWARD")):
    def step(direction=direction):
        check(lib.tf_dev_copy(P(work.ptr), P(wide.ptr), N * 16))
        check(lib.tf_flow_post_process_dev(P(work.ptr), 1, W, H, direction, P(scr.ptr)))
    k[label] = sum(prof(step, 20).values())
for b in (pristine, mask, wide, work, scr):
    b.close()
out["kernel_us"] = k

# host-array post_process of a Horn-Schunck source: one scale filter and a mask
from transflow_amd.config import HornSchunckConfig  # noqa: E402
from transflow_amd.flow import ArrayFrameProvider, HipFlowSource  # noqa: E402


def hs_source(w, h, direction, mask):
    class Builder(HipFlowSource.Builder):
        def _load_inputs(self):
            super()._load_inputs()
            self.mask = mask
    frames = [rng.integers(0, 255, (h, w), dtype=np.uint8) for _ in range(3)]
    return Builder(ArrayFrameProvider(frames, 25.0), config=HornSchunckConfig(), direction=direction,
                   flow_filters="scale=1.5")


host = {}
for (w, h, frames) in ((1920, 1080, 16), (3840, 2160, 8)):
    m = rng.random((h, w, 1)).astype(np.float32)
    raws = [rng.normal(0, 3, (h, w, 2)).astype(np.float32) for _ in range(frames + 2)]
    for direction in ("backward", "forward"):
        with hs_source(w, h, direction, m) as source:
            times = []
            for i, raw in enumerate(raws):
                t0 = time.perf_counter()
                source.post_process(raw)
                dt = time.perf_counter() - t0
                if i >= 2:
                    times.append(dt * 1e3)
            host[f"{w}x{h} {direction}"] = statistics.median(times)
out["host_post_process_ms"] = host

if len(sys.argv) > 3 and sys.argv[3] == "mem":
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        sync()
        f, t = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    w, h = 3840, 2160
    m = rng.random((h, w, 1)).astype(np.float32)
    before = free_bytes()
    with hs_source(w, h, "forward", m) as source:
        next(source)
        whole = before - free_bytes()
        source._pp.close()
        source._pp = None
        without = before - free_bytes()
    out["hs_source_4k_device_bytes"] = {"source_after_one_flow": whole, "post_process_share": whole - without,
                                        "per_pixel_post_process": (whole - without) / (w * h)}
json.dump(out, open(sys.argv[2], "w"), indent=1)
print(json.dumps(out))
