"""tests/lfn_ref.py's LiteFlowNet with the convolutions of the bf16 and bf16x3 precision modes (tf_lfn_set_precision,
transflow_amd/csrc/lfn_conv_bf16.hip), in float32 or float64: the yardstick of those modes.

  q(x, dtype)                              x rounded to float32, then to bfloat16 (ties to even), as dtype
  split(x, dtype)                          (xh, xl) = (q(x), q(x - xh))
  estimate(w, prev_bgr, next_bgr, dtype, mode)   the flow [H][W][2] with every convolution in `mode`:
      "bf16"     conv(q(x), q(w)) + b
      "bf16x3"   conv(xh, wh) + b, + conv(xh, wl), + conv(xl, wh)   (added in this order)
      "f32"      lfn_ref's own

Only `conv` changes: the correlation, the transposed convs, backwarp, the resizes and netScaleX/Y (inside
regularize_tail) are lfn_ref's in every mode.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests import lfn_ref
from transflow_amd import liteflownet as LF

MODES = ("bf16", "bf16x3")


def q(x: torch.Tensor, dtype=None) -> torch.Tensor:
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype if dtype is None else dtype)


def split(x: torch.Tensor, dtype=None):
    dtype = x.dtype if dtype is None else dtype
    xh = q(x, dtype)
    return xh, q(x.to(dtype) - xh, dtype)


class _QNet(lfn_ref._Net):
    def __init__(self, w: dict, dtype, mode: str):
        if mode not in MODES:
            raise ValueError(mode)
        super().__init__(w, dtype)
        self.mode = mode
        self.wq = {k: split(v) for k, v in self.w.items() if k.endswith(".weight")}

    def conv(self, name, x, leaky=None):
        l = self.layers[name]
        wh, wl = self.wq[name + ".weight"]
        kw = dict(stride=l.stride, padding=(l.ph, l.pw))
        if self.mode == "bf16":
            y = F.conv2d(q(x), wh, self.w[name + ".bias"], **kw)
        else:
            xh, xl = split(x)
            y = F.conv2d(xh, wh, self.w[name + ".bias"], **kw) + F.conv2d(xh, wl, None, **kw) + F.conv2d(xl, wh, None, **kw)
        return lfn_ref._lrelu(y) if (l.leaky if leaky is None else leaky) else y


def estimate(w: dict, prev_bgr: np.ndarray, next_bgr: np.ndarray, dtype=torch.float32, mode: str = "bf16") -> np.ndarray:
    """lfn_ref.estimate with the network's convolutions in `mode`."""
    if mode == "f32":
        return lfn_ref.estimate(w, prev_bgr, next_bgr, dtype)
    h, wd = prev_bgr.shape[:2]
    wp, hp = LF.padded_size(wd, h)
    with torch.no_grad():
        flow = _QNet(w, dtype, mode)(lfn_ref.prep(prev_bgr, 0, dtype), lfn_ref.prep(next_bgr, 1, dtype))
        flow = F.interpolate(flow, size=(h, wd), mode="bilinear", align_corners=False).clone()
        flow[:, 0] *= float(wd) / float(wp)
        flow[:, 1] *= float(h) / float(hp)
    return np.ascontiguousarray(flow[0].numpy().transpose(1, 2, 0))
