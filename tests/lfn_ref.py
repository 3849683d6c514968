"""A functional torch-CPU statement of transflow's LiteFlowNet flow (transflow/flow/methods/liteflownet.py), written from
the network's description, in float32 or float64, from a weight dict (transflow_amd.liteflownet.param_spec names).

  estimate(w, prev_bgr, next_bgr, dtype)   calc_optical_flow_liteflownet of a pair of uint8 BGR frames: float [H][W][2]
  correlation(one, two, stride, dtype)     the 7x7-displacement cost volume; in float32 in the CuPy kernel's order
  fmaf(a, b, c)                            an exact float32 fused multiply-add of float32 arrays
  synthetic_weights(seed, gain)            random weights of the network's shapes and the sha256 of their blob

The correlation of the reference runs on the GPU as a CuPy kernel: for an output position and displacement, lane t of
32 accumulates the channels ch = t, t + 32, ... in ascending order with `sum += a * b` (contracted to an fma: NVRTC's
default --fmad=true), the 32 partials are then added in lane order starting from 0, and the total is divided by
(float)C.  `correlation(..., torch.float32)` computes exactly that; in float64 it is the plain mean of the products.
"""
from __future__ import annotations

import hashlib
import os
import sys
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transflow_amd import liteflownet as LF  # noqa: E402

# ---- exact float32 fma ---------------------------------------------------------------------------------------------


def fmaf(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """round_f32(a*b + c) with one rounding (ties to even), for float32 arrays in the normal range.  The product of two
    float32 values is exact in float64; TwoSum gives s + e == a*b + c exactly with s = fl64(a*b + c).  Rounding s to
    float32 is then right unless s lies exactly halfway between two float32 values and e != 0: there the exact sum is
    off the tie, on e's side, so s is moved one float64 ulp towards e first (towards +-inf by e's sign: |e| is below
    half an ulp of s, so s + e would round back to s)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    tie = ((s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)) & (e != 0)
    if np.any(tie):
        s = s.copy()
        s[tie] = np.nextafter(s[tie], np.copysign(np.inf, e[tie]))
    return s.astype(np.float32)


def _round_f32(x: Fraction) -> np.float32:
    """The float32 nearest to x, ties to even (exact: candidates compared as fractions)."""
    if x == 0:
        return np.float32(0.0)
    f = np.float32(float(x))
    cands = {f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))}
    best = sorted(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(np.array(v).view(np.uint32)) & 1))
    return best[0]


def fmaf_fraction(a, b, c) -> np.float32:
    """The scalar transcription fmaf is checked against: exact rational arithmetic, one rounding."""
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


# ---- correlation ---------------------------------------------------------------------------------------------------


def correlation(one: torch.Tensor, two: torch.Tensor, stride: int, dtype=torch.float32) -> torch.Tensor:
    """[N][C][H][W] x2 -> [N][49][ceil(H/s)][ceil(W/s)]: channel c compares (y s, x s) of one with
    (y s + (c // 7 - 3) s, x s + (c % 7 - 3) s) of two, zero outside the frame."""
    n, c, h, w = one.shape
    s = stride
    ho, wo = -(-h // s), -(-w // s)
    a = one[:, :, ::s, ::s].numpy()
    pad = 3 * s
    tp = np.zeros((n, c, h + 2 * pad, w + 2 * pad), a.dtype)
    tp[:, :, pad:pad + h, pad:pad + w] = two.numpy()
    out = np.zeros((n, 49, ho, wo), a.dtype)
    for d in range(49):
        dy, dx = (d // 7 - 3) * s, (d % 7 - 3) * s
        b = tp[:, :, pad + dy:pad + dy + ho * s:s, pad + dx:pad + dx + wo * s:s]
        if dtype == torch.float64:
            out[:, d] = (a.astype(np.float64) * b.astype(np.float64)).sum(1) / c
            continue
        total = np.zeros((n, ho, wo), np.float32)
        for t in range(32):
            part = np.zeros((n, ho, wo), np.float32)
            for ch in range(t, c, 32):
                part = fmaf(a[:, ch], b[:, ch], part)
            total = total + part
        out[:, d] = total / np.float32(c)
    return torch.from_numpy(out)


# ---- network ---------------------------------------------------------------------------------------------------------


def _lrelu(x):
    return F.leaky_relu(x, 0.1)


def backwarp(x: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """grid_sample(bilinear, zeros, align_corners=True) at linspace(-1, 1) + flow * 2 / (size - 1)."""
    n, _, h, w = flow.shape
    gx = torch.linspace(-1.0, 1.0, w, dtype=flow.dtype).view(1, 1, 1, w).expand(n, 1, h, w)
    gy = torch.linspace(-1.0, 1.0, h, dtype=flow.dtype).view(1, 1, h, 1).expand(n, 1, h, w)
    fx = flow[:, 0:1] * (2.0 / (x.shape[3] - 1.0))
    fy = flow[:, 1:2] * (2.0 / (x.shape[2] - 1.0))
    grid = torch.cat([gx + fx, gy + fy], 1).permute(0, 2, 3, 1)
    return F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


class _Net:
    def __init__(self, w: dict, dtype):
        self.w = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in w.items()}
        self.layers = {l.name: l for l in LF.layers()}
        self.dtype = dtype

    def conv(self, name, x, leaky=None):
        l = self.layers[name]
        y = F.conv2d(x, self.w[name + ".weight"], self.w[name + ".bias"], stride=l.stride, padding=(l.ph, l.pw))
        return _lrelu(y) if (l.leaky if leaky is None else leaky) else y

    def deconv(self, name, x):
        c = x.shape[1]
        return F.conv_transpose2d(x, self.w[name + ".weight"], None, stride=2, padding=1, groups=c)

    def features(self, x):
        out = []
        x = self.conv("netFeatures.netOne.0", x)
        out.append(x)
        for stage, convs in (("netTwo", (0, 2, 4)), ("netThr", (0, 2)), ("netFou", (0, 2)), ("netFiv", (0,)),
                             ("netSix", (0,))):
            for j in convs:
                x = self.conv(f"netFeatures.{stage}.{j}", x)
            out.append(x)
        return out

    def head(self, prefix, x, n):
        for j in range(n):
            x = self.conv(f"{prefix}.netMain.{2 * j}", x)
        return x

    def matching(self, i, lv, f1, f2, flow):
        p = f"netMatching.{i}"
        if lv == 2:
            f1, f2 = self.conv(p + ".netFeat.0", f1), self.conv(p + ".netFeat.0", f2)
        if flow is not None:
            flow = self.deconv(p + ".netUpflow", flow)
            f2 = backwarp(f2, flow * LF.BACKWARP[lv])
        if lv >= 4:
            corr = _lrelu(correlation(f1, f2, 1, self.dtype))
        else:
            corr = self.deconv(p + ".netUpcorr", _lrelu(correlation(f1, f2, 2, self.dtype)))
        d = self.head(p, corr, 4)
        return d if flow is None else flow + d

    def subpixel(self, i, lv, f1, f2, flow):
        p = f"netSubpixel.{i}"
        if lv == 2:
            f1, f2 = self.conv(p + ".netFeat.0", f1), self.conv(p + ".netFeat.0", f2)
        f2 = backwarp(f2, flow * LF.BACKWARP[lv])
        return flow + self.head(p, torch.cat([f1, f2, flow], 1), 4)

    def regularization(self, i, lv, im1, im2, f1, flow):
        p, k = f"netRegularization.{i}", LF.UNFOLD[lv]
        diff = (im1 - backwarp(im2, flow * LF.BACKWARP[lv])).square().sum(1, keepdim=True).sqrt()
        feat = self.conv(p + ".netFeat.0", f1) if lv < 5 else f1
        x = self.head(p, torch.cat([diff, flow - flow.mean([2, 3], keepdim=True), feat], 1), 6)
        x = self.conv(p + ".netDist.0", x)
        if lv < 5:
            x = self.conv(p + ".netDist.1", x)
        return regularize_tail(x, flow, self.w[p + ".netScaleX.weight"], self.w[p + ".netScaleX.bias"],
                               self.w[p + ".netScaleY.weight"], self.w[p + ".netScaleY.bias"])

    def __call__(self, one, two):
        fo, ft = self.features(one), self.features(two)
        io, it = [one], [two]
        for j in range(1, 6):
            io.append(F.interpolate(io[-1], size=fo[j].shape[2:], mode="bilinear", align_corners=False))
            it.append(F.interpolate(it[-1], size=ft[j].shape[2:], mode="bilinear", align_corners=False))
        flow = None
        for i in (4, 3, 2, 1, 0):
            lv = LF.LEVELS[i]
            j = lv - 1
            flow = self.matching(i, lv, fo[j], ft[j], flow)
            flow = self.subpixel(i, lv, fo[j], ft[j], flow)
            flow = self.regularization(i, lv, io[j], it[j], fo[j], flow)
        return flow * 20.0


def regularize_tail(dist, flow, wx, bx, wy, by):
    """-d^2, softmax over the k^2 channels, netScaleX/Y of it times the k x k-unfolded flow, times the divisor."""
    k2 = dist.shape[1]
    k = int(round(k2 ** 0.5))
    d = dist.square().neg()
    d = (d - d.max(1, keepdim=True)[0]).exp()
    div = d.sum(1, keepdim=True).reciprocal()
    ux = F.unfold(flow[:, 0:1], kernel_size=k, stride=1, padding=(k - 1) // 2).view_as(d)
    uy = F.unfold(flow[:, 1:2], kernel_size=k, stride=1, padding=(k - 1) // 2).view_as(d)
    sx = F.conv2d(d * ux, wx, bx) * div
    sy = F.conv2d(d * uy, wy, by) * div
    return torch.cat([sx, sy], 1)


def prep(bgr: np.ndarray, role: int, dtype=torch.float32) -> torch.Tensor:
    """A uint8 BGR frame -> x 1/255 -> bilinear to the padded size -> minus the role's mean: [1][3][Hp][Wp]."""
    h, w = bgr.shape[:2]
    wp, hp = LF.padded_size(w, h)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    x = torch.from_numpy(np.ascontiguousarray(bgr.transpose(2, 0, 1)).astype(npdt) * npdt(1.0 / 255.0))[None]
    x = F.interpolate(x, size=(hp, wp), mode="bilinear", align_corners=False)
    mean = LF.MEAN_ONE if role == 0 else LF.MEAN_TWO
    x = x.clone()
    for c in range(3):
        x[:, c] = x[:, c] - mean[c]
    return x


def estimate(w: dict, prev_bgr: np.ndarray, next_bgr: np.ndarray, dtype=torch.float32) -> np.ndarray:
    """calc_optical_flow_liteflownet(prev, next) of two uint8 BGR frames [H][W][3]: the flow [H][W][2] in dtype."""
    h, wd = prev_bgr.shape[:2]
    wp, hp = LF.padded_size(wd, h)
    with torch.no_grad():
        flow = _Net(w, dtype)(prep(prev_bgr, 0, dtype), prep(next_bgr, 1, dtype))
        flow = F.interpolate(flow, size=(h, wd), mode="bilinear", align_corners=False).clone()
        flow[:, 0] *= float(wd) / float(wp)
        flow[:, 1] *= float(h) / float(hp)
    return np.ascontiguousarray(flow[0].numpy().transpose(1, 2, 0))


# ---- synthetic weights -----------------------------------------------------------------------------------------------


def synthetic_weights(seed: int, gain: float = 1.0):
    """({key: float32 array}, sha256 hex of the packed blob).  Uniform doubles of Generator(PCG64(seed)).random, drawn
    key by key in blob order: convolution weights in +-sqrt(6 / fan_in), biases in +-0.1; the flow heads (netMain.6)
    scaled by `gain`; the transposed convs in [0, 0.5) (about a bilinear x2); netScaleX/Y weights in [0.5, 1.5) and
    their biases in +-0.01 (a weighted mean of the unfolded flow)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for key, shape in LF.param_spec():
        u = rng.random(int(np.prod(shape))).reshape(shape)
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        if ".netUp" in key:
            v = u * 0.5
        elif ".netScale" in key:
            v = (0.5 + u) if key.endswith(".weight") else (2 * u - 1) * 0.01
        elif key.endswith(".bias"):
            v = (2 * u - 1) * 0.1
        else:
            v = (2 * u - 1) * np.sqrt(6.0 / fan_in)
            if ".netMain.6." in key:
                v = v * gain
        out[key] = v.astype(np.float32)
    blob = LF.pack_weights(out)
    return out, hashlib.sha256(blob.tobytes()).hexdigest()


def textured_pair(h, w, seed, shift):
    """Two BGR frames of a smooth colour texture, the second showing it moved by `shift` = (dy, dx) whole pixels."""
    rng = np.random.default_rng(seed)
    H, W = h + 2 * abs(shift[0]) + 8, w + 2 * abs(shift[1]) + 8
    base = rng.random((H // 4 + 3, W // 4 + 3, 3))
    big = np.kron(base, np.ones((4, 4, 1)))[:H, :W]
    k = np.ones(5) / 5
    for ax in (0, 1):
        big = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, big)
    big = (big * 220 + rng.normal(0, 6, big.shape)).clip(0, 255).astype(np.uint8)
    y0, x0 = abs(shift[0]) + 4, abs(shift[1]) + 4
    one = big[y0:y0 + h, x0:x0 + w]
    two = big[y0 - shift[0]:y0 - shift[0] + h, x0 - shift[1]:x0 - shift[1] + w]
    return np.ascontiguousarray(one), np.ascontiguousarray(two)


def with_module_names(w: dict) -> dict:
    """The same weights under the names of the published file ('module' for 'net')."""
    return {k.replace("net", "module"): v for k, v in w.items()}
