"""The numpy oracle against the reference ITSELF on random configurations.  The captured vectors under tests/golden
pin 18 + 18 hand-picked cases; this walks the configuration space -- every move flag, reset mode and introduce_* flag,
masks, one or two sources of 3 or 4 channels, shapes down to one pixel -- so that the oracle the GPU tests compare
with is the reference's behaviour, not a reading of it.  The cases are drawn from fixed seeds (tests/helpers.py:
live_*); what the reference returned on each of them was recorded by running it (tools/capture_live_reference.py,
tests/golden/live_*).  CPU only."""
import os

import numpy as np
import pytest

from oracle import remap_ref as R
from tests.helpers import (GOLDEN, INTRO_KEYS, LIVE_LAYER_SEEDS, PRM_KEYS, capture_frame_numbers, live_flow_ops_cases,
                           live_layer_cases, live_mask_specs)


@pytest.mark.parametrize("cls", list(LIVE_LAYER_SEEDS))
def test_oracle_equals_live_reference_on_random_configurations(cls):
    z = np.load(os.path.join(GOLDEN, f"live_layers_{cls}.npz"))
    trials = 0
    for c in live_layer_cases(cls):
        h, w, cfg, masks, intro, pixmaps, trial = c["h"], c["w"], c["cfg"], c["masks"], c["intro"], c["pixmaps"], c["trial"]
        if cls == "introduction":
            prm = R.IntroParams(**{k: v for k, v in cfg.items() if k in PRM_KEYS + INTRO_KEYS})
            ora = R.IntroductionLayer(h, w, prm, introduction_masks=intro, **masks)
        else:
            prm = R.LayerParams(**{k: v for k, v in cfg.items() if k in PRM_KEYS})
            ora = (R.SumLayer if cls == "sum" else R.MoveRefLayer)(h, w, prm, introduction_masks=intro, **masks)
        np.testing.assert_array_equal(z[f"t{trial}_data0"], ora.data)
        bg = z[f"t{trial}_bg"]
        for t, (raw, u) in enumerate(zip(c["raws"], c["us"])):
            # the reference's outputs, stored losslessly in forms that compress (tools/capture_live_reference.py): the
            # flow as its bits XOR the raw flow's, rgba only where it is not data[..., :4], the render's change of data
            key = f"t{trial}_f{t}_"
            ref_flow = (z[key + "flow_xor_raw"] ^ raw.view(np.uint32)).view(np.float32)
            ref_data = z[key + "data"]
            ref_rgba = z[key + "rgba"] if key + "rgba" in z.files else ref_data[:, :, :4]
            ref_after = ref_data + z[key + "render_change"] if key + "render_change" in z.files else ref_data
            flow = R.post_process(raw.copy(), R.BACKWARD)
            np.testing.assert_array_equal(ref_flow, flow)
            pms = [pixmaps[s][t] for s in range(len(intro))]
            if cls == "introduction":
                ora.update(ref_flow, pms, frame_numbers=capture_frame_numbers(prm, t, len(intro)))
            else:
                ora.update(ref_flow, pms, u=u)
            msg = f"{cls} trial {trial} {h}x{w} {cfg} frame {t}"
            np.testing.assert_array_equal(ref_data, ora.data, err_msg=msg)
            np.testing.assert_array_equal(ref_rgba, np.asarray(ora.rgba), err_msg=msg)
            exp = R.composite(np.broadcast_to(bg, (h, w, 3)), [ora.render()])
            np.testing.assert_array_equal(z[key + "frame"], exp, err_msg=msg)
            np.testing.assert_array_equal(ref_after, ora.data, err_msg="after render " + msg)
        trials += 1
    assert trials == 60


def test_flow_ops_oracle_equals_live_reference_on_random_inputs():
    """Flow merging, upscale, post_process with a convolution kernel (both directions, random kernel
    shapes and dtypes), render1d / render2d: oracle/flow_ops_ref.py against the reference's functions."""
    from oracle import flow_ops_ref as F
    z = np.load(os.path.join(GOLDEN, "live_flow_ops.npz"))
    kinds = [str(k) for k in z["merge_kinds"]]
    assert kinds
    for c in live_flow_ops_cases():
        i, h, w, flows, kernel = c["trial"], c["h"], c["w"], c["flows"], c["kernel"]
        n = len(flows)
        for kind in kinds:
            if kind == "absmax" and n != 2:
                continue
            np.testing.assert_array_equal(F.merge(kind, [f.copy() for f in flows]), z[f"t{i}_merge_{kind}"],
                                          err_msg=f"{kind} n={n} {h}x{w}")
        np.testing.assert_array_equal(F.upscale(flows[0], c["wf"], c["hf"]), z[f"t{i}_upscale"])
        for d in (0, 1):
            got = F.post_process_with_kernel(c["raws"][d].copy(), kernel, d)
            exp = z[f"t{i}_pp{d}"]
            assert got.dtype == exp.dtype, f"kernel {kernel.dtype} {kernel.shape}"
            np.testing.assert_array_equal(got, exp, err_msg=f"kernel {kernel.dtype} {kernel.shape} dir {d} {h}x{w}")
        np.testing.assert_array_equal(F.render1d(c["arr"], scale=c["scale"], binary=c["binary"]), z[f"t{i}_render1d"])
        np.testing.assert_array_equal(F.render2d(flows[0], scale=c["scale"]), z[f"t{i}_render2d"])


def test_mask_rules_against_the_reference_live():
    """transflow_amd/masks.py is a rule table with builders of its own (row x column outer products,
    a distance test), not a restatement of utils.py:51-140: walk the argument grammar at random --
    every rule name, 0-5 arguments from pixels / percentages / blanks / junk, dimensions larger than the
    frame (where the reference's results are what numpy slicing makes of negative bounds), ':inv' --
    and require the same array and dtype wherever the reference produces one, an exception wherever it
    raises one."""
    from transflow_amd import masks as M
    z = np.load(os.path.join(GOLDEN, "live_masks.npz"))
    specs = live_mask_specs()
    assert [s for s, _ in specs] == [str(s) for s in z["specs"]]
    assert [list(sh) for _, sh in specs] == z["shapes"].tolist()
    produced = 0
    for i, (spec, shape) in enumerate(specs):
        if z["raised"][i]:
            with pytest.raises(Exception):
                M.load_float_mask(spec, shape, 1)
            continue
        want = z[f"f{i}"]
        got = M.load_float_mask(spec, shape, 1)
        assert got.dtype == want.dtype, spec
        np.testing.assert_array_equal(got, want, err_msg=f"{spec} {shape}")
        np.testing.assert_array_equal(M.load_bool_mask(spec, shape, True), z[f"b{i}"])
        produced += 1
    assert produced > 400
