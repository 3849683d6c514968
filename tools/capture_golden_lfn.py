#!/usr/bin/env python3
"""Generate tests/golden/lfn_*.npz by RUNNING the reference's LiteFlowNet function on the CPU.

Run in the build container only (the reference package does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_lfn.py

calc_optical_flow_liteflownet needs CuPy, CUDA and a downloaded weights file; none is here.  Four stubs stand in,
installed before the reference module is imported or called:
  - a `cupy` module (the import; no CuPy kernel is ever launched);
  - FunctionCorrelation -> tests/lfn_ref.correlation in float32, the CuPy kernel's order with an exact fmaf;
  - torch.Tensor.cuda and torch.nn.Module.cuda -> the identity (everything stays on the CPU);
  - torch.hub.load_state_dict_from_url -> lfn_ref.synthetic_weights(seed, gain) under the file's `module*` names.  It
    asserts file_name='liteflownet-default' and never touches a URL.
Every other line -- the BGR flip, x 1/255, the resizes, the mean subtraction, the network, backwarp, the output's x 20,
resize and scaling -- is the reference's own code, run by torch on the CPU.  The module's global netNetwork is reset
between weight seeds.  Each fixture holds the frames (BGR, as the flow source decodes them), the seed, the gain, the
sha256 of the weight blob, the reference's float32 flow and the float64 restatement's flow; or, where the reference
raises, the exception's type name.
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import lfn_ref  # noqa: E402

_weights = {}


def _install_stubs():
    cupy = types.ModuleType("cupy")
    cupy.memoize = lambda **kw: (lambda f: f)

    def _no_kernels(*a, **k):
        raise RuntimeError("the cupy stub launches no kernel")

    cupy.RawKernel = _no_kernels
    cupy.int32 = np.int32
    sys.modules["cupy"] = cupy
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self

    def load_state_dict_from_url(url, model_dir=None, map_location=None, progress=True, check_hash=False,
                                 file_name=None, **kw):
        assert file_name == "liteflownet-default", file_name
        return {k: torch.from_numpy(v.copy()) for k, v in _weights["module"].items()}

    torch.hub.load_state_dict_from_url = load_state_dict_from_url


def reference_module():
    _install_stubs()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import transflow.flow.methods.liteflownet as M
    M.FunctionCorrelation = lambda tenOne, tenTwo, intStride: lfn_ref.correlation(tenOne, tenTwo, intStride,
                                                                                   torch.float32)
    return M


CASES = [
    # name, (h, w), frame seed, shift, weight seed, gain, identical frames
    ("64x96_s1", (64, 96), 1, (2, 3), 1, 1.0, False),
    ("64x96_s2_g025", (64, 96), 2, (1, -2), 2, 0.25, False),
    ("45x61_s3", (45, 61), 3, (-2, 1), 3, 1.0, False),
    ("37x200_s1_g025", (37, 200), 4, (1, 4), 1, 0.25, False),
    ("120x160_s2", (120, 160), 5, (3, -3), 2, 1.0, False),
    ("64x96_same_s3", (64, 96), 6, (0, 0), 3, 1.0, True),
    ("48x80_leave_s1", (48, 80), 7, (6, 9), 1, 1.0, False),
    ("20x30_s1", (20, 30), 8, (1, 1), 1, 1.0, False),
]


def main():
    M = reference_module()
    os.makedirs(OUT, exist_ok=True)
    for name, (h, w), fseed, shift, seed, gain, same in CASES:
        W, sha = lfn_ref.synthetic_weights(seed, gain)
        _weights["module"] = lfn_ref.with_module_names(W)
        M.netNetwork = None
        M.backwarp_tenGrid.clear()
        one, two = lfn_ref.textured_pair(h, w, fseed, shift)
        if same:
            two = one.copy()
        rec = dict(prev=one, next=two, seed=seed, gain=gain, sha256=sha, shift=np.array(shift))
        try:
            # the flow source hands the function RGB frames (cv.py:465); it flips them back to BGR
            flow = M.calc_optical_flow_liteflownet(np.ascontiguousarray(one[:, :, ::-1]),
                                                   np.ascontiguousarray(two[:, :, ::-1]))
            rec["flow"] = flow
            rec["flow64"] = lfn_ref.estimate(W, one, two, torch.float64)
            err = float(np.abs(flow - rec["flow64"]).max())
            print(f"{name}: |flow| max {np.abs(flow).max():.3f} mean {np.abs(flow).mean():.3f}, f32 vs f64 {err:.3g}")
        except Exception as e:        # recorded as what the reference does there
            rec["raises"] = type(e).__name__
            print(f"{name}: the reference raises {type(e).__name__}: {e}")
        path = os.path.join(OUT, f"lfn_{name}.npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < 1 << 20, path


if __name__ == "__main__":
    main()
