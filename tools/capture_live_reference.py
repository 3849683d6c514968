#!/usr/bin/env python3
"""Store what the reference returns on the differential tests' random cases, under tests/golden/live_*.

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_live_reference.py <reference checkout>

tests/test_oracle_vs_reference_live.py and the differential tests of tests/test_host_mirror.py draw their cases from
fixed seeds (tests/helpers.py: live_*_cases); this runs the importable half of the reference (the compositor,
FlowSource and its Builder, the flow-merging functions, render1d / render2d, the mask rules, the .flow.zip writer and
reader) on the very same cases and writes its outputs as data -- arrays, outcomes, one archive it wrote -- so that
the tests compare this project with the reference without the reference being present.  No reference source is
written.
"""
import json
import os
import sys
import typing
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests import helpers as H  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


class FakeSource:
    """PixmapSourceInterface stand-in (pixmap_source_interface.py:12-37), as tools/capture_golden.py's."""

    def __init__(self, frames, introduction_mask):
        self.frames, self.introduction_mask, self.counter = list(frames), introduction_mask, -1

    def next(self, timeout=1):
        self.counter += 1
        return self.frames[self.counter % len(self.frames)]

    @property
    def frame_number(self):
        return self.counter


def capture_layers():
    from transflow.compositor import Compositor
    from transflow.compositor.layers.layer import Layer
    from transflow.config import LayerConfig
    from transflow.flow.sources.source import FlowSource
    orig = np.random.random
    for cls in H.LIVE_LAYER_SEEDS:
        out = {}
        for c in H.live_layer_cases(cls):
            h, w, i = c["h"], c["w"], c["trial"]
            layer = Layer.from_args(LayerConfig(0, classname=cls, **c["cfg"]), h, w, [])
            for k, v in c["masks"].items():
                setattr(layer, k, v.copy())
            layer.set_sources([FakeSource(c["pixmaps"][s], c["intro"][s]) for s in range(len(c["intro"]))])
            comp = Compositor(h, w, [layer], background_color=c["bg"])
            fs = FlowSource(FlowSource.Direction.BACKWARD, w, h, 30.0, None, 0, 0, 0)
            out[f"t{i}_bg"] = np.asarray(comp.background_color, np.uint8)
            out[f"t{i}_data0"] = np.array(layer.data)
            for t, (raw, u) in enumerate(zip(c["raws"], c["us"])):
                flow = np.asarray(fs.post_process(raw.copy()), dtype=np.float32)
                np.random.random = lambda size=None, _u=u: _u.copy()
                try:
                    comp.update(flow)
                finally:
                    np.random.random = orig
                # stored losslessly in the forms that compress: the flow's bits XOR the raw flow's (they differ only where
                # post_process clipped), rgba only where it is not data[..., :4] (an introduction layer's is that view),
                # the data after render as its change from the data before
                key = f"t{i}_f{t}_"
                assert flow.shape == raw.shape
                out[key + "flow_xor_raw"] = flow.view(np.uint32) ^ raw.view(np.uint32)
                data = np.array(layer.data)
                out[key + "data"] = data
                rgba = np.array(layer.rgba)
                if not (rgba.dtype == data.dtype and np.array_equal(rgba, data[:, :, :4])):
                    out[key + "rgba"] = rgba
                out[key + "frame"] = np.array(comp.render())
                after = np.array(layer.data)
                if not np.array_equal(after, data):
                    out[key + "render_change"] = after - data
        np.savez_compressed(os.path.join(OUT, f"live_layers_{cls}.npz"), **out)


def capture_flow_ops():
    import typing_extensions
    if not hasattr(typing, "Self"):
        typing.Self = typing_extensions.Self          # transflow.pipeline wants Python 3.11's
    from transflow.flow.sources.source import FlowSource
    from transflow.output.render import render1d, render2d
    from transflow.pipeline import Pipeline
    from transflow.utils import upscale_array
    out = {"merge_kinds": np.array(list(Pipeline.FLOW_MERGING_FUNCTIONS))}
    for c in H.live_flow_ops_cases():
        i, flows = c["trial"], c["flows"]
        for kind, fn in Pipeline.FLOW_MERGING_FUNCTIONS.items():
            if kind == "absmax" and len(flows) != 2:
                continue
            out[f"t{i}_merge_{kind}"] = np.asarray(fn([f.copy() for f in flows]))
        out[f"t{i}_upscale"] = np.asarray(upscale_array(flows[0], c["wf"], c["hf"]))
        for d, direction in enumerate((FlowSource.Direction.FORWARD, FlowSource.Direction.BACKWARD)):
            fs = FlowSource(direction, c["w"], c["h"], 30.0, None, 0, 0, 0)
            fs.kernel = c["kernel"]
            out[f"t{i}_pp{d}"] = np.asarray(fs.post_process(c["raws"][d].copy()))
        out[f"t{i}_render1d"] = np.asarray(render1d(c["arr"], scale=c["scale"], binary=c["binary"]))
        out[f"t{i}_render2d"] = np.asarray(render2d(flows[0], scale=c["scale"]))
    np.savez_compressed(os.path.join(OUT, "live_flow_ops.npz"), **out)


def capture_masks():
    from transflow import utils as U
    specs = H.live_mask_specs()
    out = {"specs": np.array([s for s, _ in specs]), "shapes": np.array([sh for _, sh in specs], np.int64)}
    raised = []
    for i, (spec, shape) in enumerate(specs):
        try:
            f = U.load_float_mask(spec, shape, 1)
        except Exception:
            raised.append(True)
            continue
        raised.append(False)
        out[f"f{i}"] = np.asarray(f)
        out[f"b{i}"] = np.asarray(U.load_bool_mask(spec, shape, True))
    out["raised"] = np.array(raised)
    np.savez_compressed(os.path.join(OUT, "live_masks.npz"), **out)


def _scripted(base):
    class S(base):
        def __init__(self, *a, **k):
            self.calls, self.rewinds = 0, 0
            base.__init__(self, *a, **k)

        def next(self):
            self.calls += 1
            return np.full((2, 3, 2), float(self.calls), np.float32)

        def rewind(self):
            self.rewinds += 1
            base.rewind(self)

        def post_process(self, raw):
            return raw
    return S


def capture_iteration():
    from transflow.flow.sources.source import FlowSource as Ref
    Theirs = _scripted(Ref)
    trials = []
    for c in H.live_iteration_cases():
        kw = {}
        if c["mode"] == 1:
            kw = dict(lock_mode=Ref.LockMode.STAY, lock_expr_stay=c["pairs"])
        elif c["mode"] == 2:
            kw = dict(lock_mode=Ref.LockMode.SKIP, lock_expr_skip=lambda t, a=c["window"][0], b=c["window"][1]: a < t < b)
        r = Theirs(Ref.Direction.BACKWARD, 3, 2, c["fps"], c["length"], c["start"], c["ckpt"], c["end"], **kw)
        steps = []
        for _ in range(30):
            try:
                out = ["value", float(next(r)[0, 0, 0])]
            except (StopIteration, IndexError, RuntimeError) as e:
                out = [type(e).__name__, None]
            steps.append(out + [r.calls, r.rewinds, r.input_frame_index, r.output_frame_index])
            if out[0] != "value":
                break
        trials.append(H.as_json(steps))
    with open(os.path.join(OUT, "live_iteration.json"), "w") as f:
        json.dump(trials, f, separators=(",", ":"))


def capture_builder():
    import warnings
    from transflow.flow.sources.source import FlowSource as Ref
    outcomes = []
    for _, kw, base_length, fps in H.live_builder_cases():
        b = Ref.Builder(**kw)
        b.width, b.height, b.framerate, b.base_length = 6, 4, fps, base_length
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                b.build()
            outcomes.append(H.as_json(tuple(getattr(b, f) for f in H.BUILDER_FIELDS)))
        except Exception as e:
            outcomes.append(type(e).__name__)
    with open(os.path.join(OUT, "live_builder.json"), "w") as f:
        json.dump(outcomes, f, separators=(",", ":"))


def capture_archive(tmp):
    from transflow.flow.sources.archive import ArchiveFlowSource as RefArchive
    from transflow.output.numpy import NumpyOutput as RefNumpyOutput
    from transflow.utils import find_unique_path as ref_unique_path
    from transflow_amd.archive import flow_export_meta
    path = os.path.join(OUT, "live_archive_reference.flow.zip")
    out = RefNumpyOutput(path, True)
    out.write_meta(flow_export_meta("clip.mp4", 9, 6, 25.0, "backward"))
    for f in H.live_archive_flows():
        out.write_array(f)
    out.close()
    with zipfile.ZipFile(path) as z:
        assert z.namelist() == ["meta.json", "000000000.npy", "000000001.npy", "000000002.npy"], z.namelist()
    rb = RefArchive.Builder(path)
    rb.build()
    rb.archive.close()
    names = os.path.join(tmp, "names")
    os.makedirs(names)
    unique = {}
    for name in H.UNIQUE_PATH_NAMES:
        target = os.path.join(names, name)
        free = ref_unique_path(target)
        open(target, "wb").close()
        taken = ref_unique_path(target)
        open(os.path.join(names, os.path.basename(taken)), "wb").close()
        unique[name] = [os.path.basename(p) for p in (free, taken, ref_unique_path(target))]
    meta = {"builder": {a: getattr(rb, a) for a in H.ARCHIVE_BUILDER_FIELDS}, "direction": rb.direction.value,
            "unique_path": unique}
    with open(os.path.join(OUT, "live_archive.json"), "w") as f:
        json.dump(meta, f, indent=1)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "transflow")):
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import tempfile
    capture_layers()
    capture_flow_ops()
    capture_masks()
    capture_iteration()
    capture_builder()
    with tempfile.TemporaryDirectory() as tmp:
        capture_archive(tmp)


if __name__ == "__main__":
    main()
