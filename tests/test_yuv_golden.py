"""tests/golden/yuv_<layout>.npz (tools/capture_golden_yuv.py): the bytes the restatement gave when the format was
written down.  The restatement and host_convert still give them."""
import os

import numpy as np
import pytest

from tests import yuv_cases, yuv_ref


@pytest.mark.parametrize("layout", yuv_cases.LAYOUTS)
def test_the_restatement_and_host_convert_give_the_recorded_bytes(golden_dir, layout):
    from transflow_amd.yuv import host_convert
    with np.load(os.path.join(golden_dir, f"yuv_{layout}.npz")) as gold:
        names = [str(n) for n in gold["names"]]
        assert len(names) >= 100
        for i, (name, matrix, rng) in enumerate(zip(names, gold["matrices"], gold["ranges"])):
            rgb, want = gold[f"rgb_{i}"], gold[f"out_{i}"].tobytes()
            assert yuv_ref.convert(rgb, layout, str(matrix), str(rng)) == want, name
            assert host_convert(rgb, layout, str(matrix), str(rng)).tobytes() == want, name
