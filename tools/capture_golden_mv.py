#!/usr/bin/env python3
"""Generate tests/golden/mv_*.npz by RUNNING the reference's motion-vector flow source.

Run in the build container only (the reference package does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_mv.py

PyAV is not installed there.  The reference's module imports `av.container` at its top, checks its container against
`av.container.InputContainer` and imports `av.sidedata.motionvectors.MotionVectors` for a type cast: stub modules with
those names go into sys.modules BEFORE the reference is imported.  The source is built over a fake container whose
decoded frames carry `side_data = {"MOTION_VECTORS": [...]}`; every line of AvFlowSource.next() is the reference's own.
Each fixture holds the vector table, the frame size and the flow the reference painted; only data is written.
"""
import os
import sys
import types

import numpy as np

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import mv_ref  # noqa: E402


def _install_av_stub():
    av = types.ModuleType("av")
    container = types.ModuleType("av.container")
    sidedata = types.ModuleType("av.sidedata")
    motionvectors = types.ModuleType("av.sidedata.motionvectors")

    class InputContainer:
        def __init__(self, frames):
            self.frames = frames

        def decode(self, video=0):
            return iter(self.frames)

        def seek(self, offset):
            pass

        def close(self):
            pass

    class MotionVectors(list):
        pass

    container.InputContainer = InputContainer
    motionvectors.MotionVectors = MotionVectors
    av.container, av.sidedata, sidedata.motionvectors = container, sidedata, motionvectors
    sys.modules.update({"av": av, "av.container": container, "av.sidedata": sidedata,
                        "av.sidedata.motionvectors": motionvectors})
    return InputContainer, MotionVectors


class _Frame:
    def __init__(self, side_data):
        self.side_data = side_data


def reference_painter():
    """paint(table or None, width, height) -> the flow AvFlowSource.next() returns for a frame with those vectors."""
    InputContainer, MotionVectors = _install_av_stub()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from transflow.flow.sources.av import AvFlowSource
    from transflow.flow.sources.source import FlowSource

    def paint(table, width, height):
        side = {}
        if table is not None:
            side["MOTION_VECTORS"] = MotionVectors(
                types.SimpleNamespace(**{name: int(row[name]) for name in mv_ref.FIELDS}) for row in table)
        # the constructor's rewind() consumes input_frame_index + 1 = 1 frame; next() takes the one after
        container = InputContainer([_Frame({}), _Frame(side)])
        source = AvFlowSource(container, FlowSource.Direction.FORWARD, width, height, 30.0, None, 0, 0, 0)
        return source.next()
    return paint


def cases():
    """(name, width, height, table or None)"""
    w, h = mv_ref.KNOWN_SIZE
    yield "known", w, h, mv_ref.records(mv_ref.KNOWN_VECTORS)
    yield "nosidedata", 53, 37, None
    yield "h264_37x53", 53, 37, mv_ref.h264_like(53, 37, seed=101)
    yield "h264_120x160", 160, 120, mv_ref.h264_like(160, 120, seed=102)
    yield "h264_480x854", 854, 480, mv_ref.h264_like(854, 480, seed=103)
    yield "hostile_120x160", 160, 120, mv_ref.hostile(160, 120, 300, seed=104)


def main():
    paint = reference_painter()
    os.makedirs(OUT, exist_ok=True)
    for name, width, height, table in cases():
        flow = paint(table, width, height)
        assert flow.dtype == np.float32 and flow.shape == (height, width, 2)
        arrays = dict(width=np.int64(width), height=np.int64(height), has_vectors=np.bool_(table is not None),
                      vectors=table if table is not None else np.empty(0, mv_ref.DTYPE), flow=flow)
        path = os.path.join(OUT, f"mv_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}: {0 if table is None else len(table)} vectors, "
              f"{int(np.count_nonzero(mv_ref.bits(flow).reshape(-1, 2).any(axis=1)))} painted pixels, {os.path.getsize(path)} B")


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
