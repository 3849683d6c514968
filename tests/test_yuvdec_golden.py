"""tests/golden/yuvdec_<layout>.npz (tools/capture_golden_yuvdec.py): the pixels the restatement gave when the conversion
back from YUV was written down.  The restatement and host_convert_back still give them."""
import os

import numpy as np
import pytest

from tests import yuvdec_cases, yuvdec_ref


@pytest.mark.parametrize("layout", yuvdec_cases.LAYOUTS)
def test_the_restatement_and_host_convert_back_give_the_recorded_pixels(golden_dir, layout):
    from transflow_amd.yuvdec import host_convert_back
    with np.load(os.path.join(golden_dir, f"yuvdec_{layout}.npz")) as gold:
        names = [str(n) for n in gold["names"]]
        assert len(names) >= 200
        for i, (name, matrix, rng, chroma) in enumerate(zip(names, gold["matrices"], gold["ranges"], gold["chromas"])):
            planes, (w, h), want = gold[f"planes_{i}"], (int(v) for v in gold[f"size_{i}"]), gold[f"out_{i}"]
            matrix, rng, chroma = str(matrix), str(rng), str(chroma)
            np.testing.assert_array_equal(yuvdec_ref.convert_back(planes, w, h, layout, matrix, rng, chroma), want, err_msg=name)
            np.testing.assert_array_equal(host_convert_back(planes, w, h, layout, matrix, rng, chroma, "rgb"), want, err_msg=name)
