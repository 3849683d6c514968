#!/usr/bin/env python3
"""What does one launch of the remap step take with nothing beside it?  The bench's pass of remap steps (one tf_remap_steps_dev
call over the pass's flows) on an otherwise idle GPU, per launch, and the bytes per second that is on the step's 26 B/px
by the counters -- next to the rate of the library's 16-byte-per-lane copy kernel (bench.copy_ceiling).  With a library
that has the options, once per value of remap_lean and remap_quad.  usage (GPU box): python3 tools/micro/remap_alone.py [workload] [batch] [reps]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench  # noqa: E402
from transflow_amd import _lib  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "4k"
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 128
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
BYTES_PER_PX = 26   # profiles/NOTES.md, round 5: 2 * FETCH_SIZE + WRITE_SIZE of the step inside a tf_remap_steps_dev call
wl = bench.WORKLOADS[name]
job = bench.Job(wl, batch, bench.make_plan(batch + 1, batch, 0, 1), batch + 1, seed=2000, device=0, lanes=1)
job.calc_pass(0)
job.sync()
def has(option):
    try:
        _lib.get_option(option)
        return True
    except ValueError:
        return False


# a form is the options it sets; with a library that has neither option, the kernel it has
forms = [("(no remap_quad option)", {})]
if has("remap_quad"):
    forms = [("remap_quad=1", {"remap_quad": 1}), ("remap_quad=0", {"remap_quad": 0})]
if has("remap_lean"):
    forms = [("remap_lean=1", {"remap_lean": 1})] + [(f"remap_lean=0 {label}", dict(opts, remap_lean=0)) for label, opts in forms]
for label, opts in forms:
    for option, value in opts.items():
        _lib.set_option(option, value)
    for _ in range(2):
        job.remap_pass(job.layer)
    job.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        job.remap_pass(job.layer)
    job.sync()
    us = (time.perf_counter() - t0) / (reps * job.batch) * 1e6
    px = wl["w"] * wl["h"]
    print(f"{name} x {batch} {label}: {us:.1f} us per remap launch alone, {BYTES_PER_PX * px / us / 1e6:.2f} TB/s on {BYTES_PER_PX} B/px")
print(f"copy kernel: {bench.copy_ceiling(job.lib, job.check) / 1e3:.2f} TB/s")
