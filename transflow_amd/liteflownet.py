"""LiteFlowNet handle: thin object over the tf_lfn_* entry points of libtfhip.so, and the weights it runs.

`LiteFlowNet.calc(prev_bgr, next_bgr)` is transflow's calc_optical_flow_liteflownet (transflow/flow/methods/
liteflownet.py) called as cv.py:509-516 calls it: the two frames of a pair, resized INTER_NEAREST to the handle's size,
in, and the float32 [H][W][2] flow out.  The frames go up in BGR: the reference's RGB -> BGR flip (it feeds the network
BGR) and cv.py's BGR -> RGB conversion cancel.

The network's weights are the user's: the reference downloads them ('liteflownet-default'); this backend never does.
`load_weights(path)` reads that file (torch.load, CPU, weights only -- the one place torch is touched), checks every
key and shape against `param_spec()` and returns float32 numpy arrays; `pack_weights` lays them out as the one blob
tf_lfn_set_weights takes, in `param_spec()` order.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

LEVELS = (2, 3, 4, 5, 6)                      # coarse-to-fine levels, feature resolution 1 / 2**(level - 1)
UNFOLD = {2: 7, 3: 5, 4: 5, 5: 3, 6: 3}       # flow-head, distance and unfold kernel size per level
BACKWARP = {2: 10.0, 3: 5.0, 4: 2.5, 5: 1.25, 6: 0.625}
FEAT_C = (32, 32, 64, 96, 128, 192)           # channels of the six feature stages (index 0 = full resolution)
SUB_CIN = {2: 130, 3: 130, 4: 194, 5: 258, 6: 386}
REG_CIN = {2: 131, 3: 131, 4: 131, 5: 131, 6: 195}
MEAN_ONE = (0.411618, 0.434631, 0.454253)    # per BGR channel, subtracted from frame one ...
MEAN_TWO = (0.410782, 0.433645, 0.452793)    # ... and from frame two
MAX_PAIRS = 16                                # TF_LFN_MAX_PAIRS
# how the network's convolutions multiply (tf_lfn_set_precision): float32; operands rounded to bfloat16; or each
# operand as a bfloat16 pair hi + lo and the three products that matter (hi hi, hi lo, lo hi).  Sums are float32.
PRECISIONS = {"f32": 0, "bf16": 1, "bf16x3": 2}     # TF_LFN_F32, TF_LFN_BF16, TF_LFN_BF16X3


def precision_code(name) -> int:
    """The TF_LFN_* value of a precision name; ValueError for anything else."""
    if not isinstance(name, str) or name not in PRECISIONS:
        raise ValueError(f"LiteFlowNet precision {name!r} is not one of {', '.join(map(repr, PRECISIONS))}")
    return PRECISIONS[name]


class Layer:
    """One parametrised layer: a convolution (weight [Cout][Cin][kh][kw] + bias [Cout]) or a depthwise 4x4 stride-2
    transposed convolution (weight [C][1][4][4], no bias)."""

    def __init__(self, name, cout, cin, kh, kw, stride=1, ph=0, pw=0, leaky=False, deconv=False):
        self.name, self.cout, self.cin, self.kh, self.kw = name, cout, cin, kh, kw
        self.stride, self.ph, self.pw, self.leaky, self.deconv = stride, ph, pw, leaky, deconv

    @property
    def shapes(self):
        if self.deconv:
            return [(self.name + ".weight", (self.cout, 1, 4, 4))]
        return [(self.name + ".weight", (self.cout, self.cin, self.kh, self.kw)), (self.name + ".bias", (self.cout,))]

    def out_size(self, h, w):
        if self.deconv:
            return 2 * h, 2 * w
        return ((h + 2 * self.ph - self.kh) // self.stride + 1, (w + 2 * self.pw - self.kw) // self.stride + 1)


def layers():
    """Every parametrised layer of the network, in the order of the weight blob (the modules' definition order)."""
    L = []

    def conv(name, cout, cin, k, stride=1, leaky=True, kh=None, kw=None):
        kh, kw = (k, k) if kh is None else (kh, kw)
        L.append(Layer(name, cout, cin, kh, kw, stride, (kh - 1) // 2, (kw - 1) // 2, leaky))

    conv("netFeatures.netOne.0", 32, 3, 7)
    conv("netFeatures.netTwo.0", 32, 32, 3, 2)
    conv("netFeatures.netTwo.2", 32, 32, 3)
    conv("netFeatures.netTwo.4", 32, 32, 3)
    conv("netFeatures.netThr.0", 64, 32, 3, 2)
    conv("netFeatures.netThr.2", 64, 64, 3)
    conv("netFeatures.netFou.0", 96, 64, 3, 2)
    conv("netFeatures.netFou.2", 96, 96, 3)
    conv("netFeatures.netFiv.0", 128, 96, 3, 2)
    conv("netFeatures.netSix.0", 192, 128, 3, 2)
    for i, lv in enumerate(LEVELS):
        k, p = f"netMatching.{i}", UNFOLD[lv]
        if lv == 2:
            conv(k + ".netFeat.0", 64, 32, 1)
        if lv != 6:
            L.append(Layer(k + ".netUpflow", 2, 2, 4, 4, deconv=True))
        if lv < 4:
            L.append(Layer(k + ".netUpcorr", 49, 49, 4, 4, deconv=True))
        conv(k + ".netMain.0", 128, 49, 3)
        conv(k + ".netMain.2", 64, 128, 3)
        conv(k + ".netMain.4", 32, 64, 3)
        conv(k + ".netMain.6", 2, 32, p, leaky=False)
    for i, lv in enumerate(LEVELS):
        k, p = f"netSubpixel.{i}", UNFOLD[lv]
        if lv == 2:
            conv(k + ".netFeat.0", 64, 32, 1)
        conv(k + ".netMain.0", 128, SUB_CIN[lv], 3)
        conv(k + ".netMain.2", 64, 128, 3)
        conv(k + ".netMain.4", 32, 64, 3)
        conv(k + ".netMain.6", 2, 32, p, leaky=False)
    for i, lv in enumerate(LEVELS):
        k, p = f"netRegularization.{i}", UNFOLD[lv]
        if lv < 5:
            conv(k + ".netFeat.0", 128, FEAT_C[lv - 1], 1)
        for j, (co, ci) in enumerate([(128, REG_CIN[lv]), (128, 128), (64, 128), (64, 64), (32, 64), (32, 32)]):
            conv(k + f".netMain.{2 * j}", co, ci, 3)
        if lv < 5:
            conv(k + ".netDist.0", p * p, 32, 0, leaky=False, kh=p, kw=1)
            conv(k + ".netDist.1", p * p, p * p, 0, leaky=False, kh=1, kw=p)
        else:
            conv(k + ".netDist.0", p * p, 32, p, leaky=False)
        conv(k + ".netScaleX", 1, p * p, 1, leaky=False)
        conv(k + ".netScaleY", 1, p * p, 1, leaky=False)
    return L


def param_spec():
    """[(key, shape)] of every weight, in blob order (key names as the network's state_dict, 'net' prefixes)."""
    return [s for layer in layers() for s in layer.shapes]


def blob_size() -> int:
    return sum(int(np.prod(shape)) for _, shape in param_spec())


def _layer(index: int, deconv: bool) -> Layer:
    """layers()[index], which must be a transposed conv (deconv) or a convolution (not deconv); else ValueError."""
    ls = layers()
    if not 0 <= index < len(ls) or ls[index].deconv != deconv:
        raise ValueError(f"layer {index} is not a {'transposed ' if deconv else ''}convolution")
    return ls[index]


def layer_index(name: str) -> int:
    """Index of a layer (its name without .weight / .bias) among layers(): the tf_lfn_stage_conv layer number."""
    for i, layer in enumerate(layers()):
        if layer.name == name:
            return i
    raise KeyError(name)


def check_weights(d: dict) -> dict:
    """`module*` or `net*` key names -> {net key: float32 C-contiguous array}; ValueError naming the first missing,
    extra or mis-shaped key."""
    got = {}
    for k, v in d.items():
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        got[k.replace("module", "net")] = v
    spec = param_spec()
    want = dict(spec)
    for key, shape in spec:
        if key not in got:
            raise ValueError(f"LiteFlowNet weights: missing key {key!r} (shape {shape})")
        if tuple(np.shape(got[key])) != shape:
            raise ValueError(f"LiteFlowNet weights: {key!r} has shape {tuple(np.shape(got[key]))}, expected {shape}")
    for key in got:
        if key not in want:
            raise ValueError(f"LiteFlowNet weights: unexpected key {key!r}")
    return {key: np.ascontiguousarray(np.asarray(got[key], dtype=np.float32)) for key, _ in spec}


def load_weights(path) -> dict:
    """The 'liteflownet-default' state dict of the reference (torch.load on the CPU, weights only), checked."""
    import torch
    return check_weights(torch.load(path, map_location="cpu", weights_only=True))


def pack_weights(d: dict) -> np.ndarray:
    """The float32 blob of tf_lfn_set_weights: every array of param_spec() flattened (C order), one after another."""
    d = check_weights(d)
    return np.concatenate([d[key].reshape(-1) for key, _ in param_spec()]).astype(np.float32)


def as_weights(w) -> dict:
    """A weights path, or a dict of arrays (module* or net* names) -> checked float32 arrays."""
    if isinstance(w, dict):
        return check_weights(w)
    return load_weights(w)


def padded_size(width: int, height: int):
    """The network's input size: W and H rounded up to multiples of 32."""
    return (width + 31) // 32 * 32, (height + 31) // 32 * 32


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _nhwc(a, what: str, lead=None, channels=None) -> np.ndarray:
    """a as float32 NHWC; ValueError unless it has 4 dimensions, the leading (n, h, w) `lead` and `channels` channels
    when those are given (the C side reads and writes by the sizes it computes from them)."""
    a = _f32(a)
    if a.ndim != 4 or (lead is not None and a.shape[:3] != tuple(lead)) or (channels is not None and a.shape[3] != channels):
        want = f"({', '.join(map(str, lead)) if lead else 'n, h, w'}, {channels if channels is not None else 'c'})"
        raise ValueError(f"{what}: expected an NHWC array of shape {want}, got {a.shape}")
    return a


class LiteFlowNet:
    def __init__(self, width: int, height: int, weights, frame_slots: int = 2, max_pairs: int = 1,
                 device: int | None = None, precision: str = "f32"):
        code = precision_code(precision)
        self._lib = _lib.load()
        self._h = C.c_void_p()
        if device is not None:
            check(self._lib.tf_init(int(device)))
        self.width, self.height = int(width), int(height)
        self.frame_slots, self.max_pairs = int(frame_slots), int(max_pairs)
        check(self._lib.tf_lfn_create(C.byref(self._h), self.width, self.height, self.frame_slots, self.max_pairs))
        if code:
            check(self._lib.tf_lfn_set_precision(self._h, code))
        self.set_weights(weights)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tf_lfn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_weights(self, weights) -> None:
        """A path, a dict of arrays, or an already packed float32 blob."""
        if isinstance(weights, np.ndarray) and weights.ndim == 1:
            blob = _f32(weights)
        else:
            blob = pack_weights(as_weights(weights))
        check(self._lib.tf_lfn_set_weights(self._h, _ptr(blob), int(blob.size)))

    def set_precision(self, name: str) -> None:
        """ "f32", "bf16" or "bf16x3": how the convolutions of the calls that follow multiply (PRECISIONS)."""
        code = precision_code(name)
        check(self._lib.tf_lfn_set_precision(self._h, code))

    @property
    def precision(self) -> str:
        code = C.c_int()
        check(self._lib.tf_lfn_get_precision(self._h, C.byref(code)))
        return {v: k for k, v in PRECISIONS.items()}[code.value]

    # -- frames ------------------------------------------------------------------------------
    def set_frame_bgr(self, slot: int, frame) -> None:
        """cv.py:461-464 on the device: a decoded BGR frame of any size -> nearest-neighbour resize into the slot."""
        a = np.asarray(frame)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError(f"LiteFlowNet needs uint8 BGR frames (H, W, 3), got {a.dtype} {a.shape}")
        if a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
            a = np.ascontiguousarray(a)
        check(self._lib.tf_lfn_set_frame_bgr(self._h, int(slot), _ptr(a), a.shape[1], a.shape[0], a.strides[0]))

    def set_frame(self, slot: int, frame) -> None:
        a = np.asarray(frame)
        if a.ndim != 3:
            raise ValueError("LiteFlowNet needs colour (BGR) frames; a grey frame cannot be used")
        self.set_frame_bgr(slot, a)

    # -- calls ---------------------------------------------------------------------------------
    def calc_slots(self, prev_slots, next_slots) -> None:
        """One call over len(prev_slots) pairs, batched; flows stay on the device (get_flow, flow_ptr)."""
        n = len(prev_slots)
        if n != len(next_slots) or n < 1:
            raise ValueError("prev_slots and next_slots must be non-empty and of the same length")
        ps, ns = (C.c_int * n)(*map(int, prev_slots)), (C.c_int * n)(*map(int, next_slots))
        check(self._lib.tf_lfn_calc_slots(self._h, n, ps, ns))

    def calc(self, prev, nxt) -> np.ndarray:
        """calc_optical_flow_liteflownet on the pair (BGR frames): a new float32 [H][W][2] array."""
        self.set_frame_bgr(0, prev)
        self.set_frame_bgr(1, nxt)
        self.calc_slots([0], [1])
        return self.get_flow(0)

    def get_flow(self, pair: int) -> np.ndarray:
        out = np.empty((self.height, self.width, 2), np.float32)
        check(self._lib.tf_lfn_get_flow(self._h, int(pair), _ptr(out)))
        return out

    def flow_ptr(self, pair: int) -> int:
        p = C.c_void_p()
        check(self._lib.tf_lfn_flow_ptr(self._h, int(pair), C.byref(p)))
        return p.value

    # -- stage entry points (tests) ----------------------------------------------------------------
    def stage_conv(self, layer: int, x, out=None, in_off: int = 0, out_off: int = 0, residual=None, res_off: int = 0):
        """Layer `layer` of layers() on x [n][h][w][C_total] (its input channels are x[..., in_off:in_off + Cin]),
        into `out` [n][ho][wo][C_out_total] at channel out_off (other channels kept; zeros when out is None), plus
        residual[..., res_off:res_off + Cout] when given.  Bias and LeakyReLU as the layer has them."""
        spec = _layer(layer, deconv=False)
        x = _nhwc(x, "stage_conv input")
        n, h, w, cs = x.shape
        ho, wo = spec.out_size(h, w)
        if out is None:
            out = np.zeros((n, ho, wo, spec.cout), np.float32)
        out = _nhwc(out, "stage_conv output", (n, ho, wo)).copy()
        res_p, res_cs = None, 0
        if residual is not None:
            residual = _nhwc(residual, "stage_conv residual", (n, ho, wo))
            res_p, res_cs = _ptr(residual), residual.shape[3]
        check(self._lib.tf_lfn_stage_conv(self._h, int(layer), n, h, w, _ptr(x), cs, int(in_off), res_p, res_cs,
                                          int(res_off), _ptr(out), out.shape[3], int(out_off)))
        return out

    def stage_deconv(self, layer: int, x):
        """The depthwise 4x4 stride-2 transposed conv `layer` on x [n][h][w][C]: [n][2h][2w][C]."""
        x = _nhwc(x, "stage_deconv input", channels=_layer(layer, deconv=True).cout)
        n, h, w, c = x.shape
        out = np.empty((n, 2 * h, 2 * w, c), np.float32)
        check(self._lib.tf_lfn_stage_deconv(self._h, int(layer), n, h, w, _ptr(x), _ptr(out)))
        return out

    def stage_correlation(self, one, two, stride: int):
        """LeakyReLU(correlation(one, two, stride)) of NHWC features: [n][ceil(h/s)][ceil(w/s)][49]."""
        one = _nhwc(one, "stage_correlation one")
        n, h, w, c = one.shape
        two = _nhwc(two, "stage_correlation two", (n, h, w), c)
        ho, wo = -(-h // stride), -(-w // stride)
        out = np.empty((n, ho, wo, 49), np.float32)
        check(self._lib.tf_lfn_stage_correlation(self._h, int(stride), n, h, w, c, _ptr(one), _ptr(two), _ptr(out)))
        return out

    def stage_backwarp(self, x, flow, scale: float):
        """backwarp(x, flow * scale) of NHWC x [n][h][w][c] and flow [n][h][w][2]."""
        x = _nhwc(x, "stage_backwarp input")
        n, h, w, c = x.shape
        flow = _nhwc(flow, "stage_backwarp flow", (n, h, w), 2)
        out = np.empty_like(x)
        check(self._lib.tf_lfn_stage_backwarp(self._h, n, h, w, c, _ptr(x), _ptr(flow), C.c_float(scale), _ptr(out)))
        return out

    def stage_regularize_tail(self, level: int, dist, flow):
        """-d^2 -> softmax over the k^2 channels -> netScaleX/Y of the weighted unfolded flow -> x divisor, with the
        level's netScale weights: dist [n][h][w][k^2], flow [n][h][w][2] -> [n][h][w][2]."""
        if level not in UNFOLD:
            raise ValueError(f"stage_regularize_tail: level {level} not in {LEVELS}")
        dist = _nhwc(dist, "stage_regularize_tail dist", channels=UNFOLD[level] ** 2)
        n, h, w, _ = dist.shape
        flow = _nhwc(flow, "stage_regularize_tail flow", (n, h, w), 2)
        out = np.empty((n, h, w, 2), np.float32)
        check(self._lib.tf_lfn_stage_regularize_tail(self._h, int(level), n, h, w, _ptr(dist), _ptr(flow), _ptr(out)))
        return out

    def stage_prep(self, slot: int, role: int):
        """The slot's frame as the network sees it in role 0 (one) or 1 (two): x 1/255, bilinear to Hp x Wp, minus the
        role's mean: float32 [Hp][Wp][3] (BGR)."""
        wp, hp = padded_size(self.width, self.height)
        out = np.empty((hp, wp, 3), np.float32)
        check(self._lib.tf_lfn_stage_prep(self._h, int(slot), int(role), _ptr(out)))
        return out
