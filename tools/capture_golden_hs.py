#!/usr/bin/env python3
"""Generate tests/golden/hs_*.npz by RUNNING the reference's Horn-Schunck function.

Run in the build container only (the reference package does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_hs.py

OpenCV is not installed there.  The one OpenCV call of the function, cv2.GaussianBlur(float32, (5, 5), 0), is served
by a stub put into sys.modules BEFORE the reference is imported: OpenCV's fixed 5-tap kernel [1, 4, 6, 4, 1] / 16
with BORDER_REFLECT_101 (its default border), which is exact on uint8-valued input (tests/hs_ref.py says why).  Every
other line runs the reference's own numpy and scipy code.  Each fixture holds the frames, the initial flow (if any),
the parameters, the flow and the number of iterations run; only data is written.
"""
import hashlib
import os
import sys
import types

import numpy as np

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.hs_ref import delta_u_at, gaussian_blur5, sigma_max  # noqa: E402
from tests.helpers import synth_pair  # noqa: E402


def _install_cv2_stub():
    def GaussianBlur(src, ksize, sigmaX, *args, **kwargs):
        if tuple(ksize) != (5, 5) or sigmaX > 0 or args or kwargs:
            raise NotImplementedError("the stub serves GaussianBlur(img, (5, 5), 0) only")
        return gaussian_blur5(src)

    stub = types.ModuleType("cv2")
    stub.GaussianBlur = GaussianBlur
    sys.modules["cv2"] = stub


def reference_function():
    """The reference's function, imported with the cv2 stub in place (the caller restores sys.modules if it must)."""
    _install_cv2_stub()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from transflow.flow.methods.horn_schunck import calc_optical_flow_horn_schunck
    return calc_optical_flow_horn_schunck


def counting(fn):
    """Runs fn and counts the iterations through numpy.linalg.norm calls (delta set) or max_iters."""
    def run(prev, nxt, flow, alpha, max_iters, decay, delta):
        calls = [0]
        orig = np.linalg.norm

        def norm(*a, **k):
            calls[0] += 1
            return orig(*a, **k)
        np.linalg.norm = norm
        try:
            out = fn(prev, nxt, flow=flow, alpha=alpha, max_iters=max_iters, decay=decay, delta=delta)
        finally:
            np.linalg.norm = orig
        return out, (calls[0] if delta is not None else max(0, max_iters))
    return run


def cases():
    """(name, h, w, seed, chain, alpha, iters, decay, delta, delta_rel): delta_rel = (k, r) places delta at
    sigma_k * r, sigma_k the spectral norm of u_k - u_{k-1}."""
    out = []
    sizes = [(9, 200, 11), (37, 53, 12), (120, 160, 13)]
    for (h, w, seed) in sizes:
        for chain in ("f64", "f32"):
            out.append((f"{h}x{w}_{chain}_default", h, w, seed, chain, 1, 3, 0, 1, None))
            out.append((f"{h}x{w}_{chain}_iters50_dnone", h, w, seed, chain, 1, 50, 0.95, None, None))
    for alpha in (0.5, 3):
        out.append((f"37x53_f32_alpha{alpha}", 37, 53, 21, "f32", alpha, 3, 0.95, None, None))
        out.append((f"37x53_f64_alpha{alpha}", 37, 53, 21, "f64", alpha, 3, 0, None, None))
    for decay in (0, 0.95, 1):
        out.append((f"120x160_f32_decay{decay}", 120, 160, 22, "f32", 1, 3, decay, 1, None))
    for iters in (0, 1, 3):
        for chain in ("f64", "f32"):
            out.append((f"37x53_{chain}_iters{iters}", 37, 53, 23, chain, 1, iters, 0.95, 1, None))
    for chain in ("f64", "f32"):
        out.append((f"37x53_{chain}_delta0", 37, 53, 24, chain, 1, 5, 0.95, 0, None))
        out.append((f"120x160_{chain}_static", 120, 160, 25, chain, 1, 50, 0.95, 1, None))
        for k in (2, 10, 21):
            for r in (1 + 1e-2, 1 - 1e-2, 1 + 1e-4, 1 - 1e-4):
                out.append((f"64x96_{chain}_stop{k}_{r:.4f}", 64, 96, 26, chain, 1, 50, 0.95, None, (k, r)))
    out.append(("480x854_f64_default", 480, 854, 27, "f64", 1, 3, 0, 1, None))
    return out


BIG = 200_000      # pixels above which a fixture keeps the flow's SHA-256 and a sample instead of the flow


def main():
    fn = counting(reference_function())
    os.makedirs(OUT, exist_ok=True)
    for (name, h, w, seed, chain, alpha, iters, decay, delta, delta_rel) in cases():
        a, b = synth_pair(h, w, seed=seed, shift=(2.0, 1.5), noise=4.0)
        if name.endswith("_static"):
            b = a.copy()
        flow = None
        if chain == "f32":
            # multiples of 1/16 in [-4, 4]: an initial flow that compresses
            flow = (np.clip(np.round(np.random.default_rng(seed + 100).normal(0, 24, (h, w, 2))), -64, 64) / 16).astype(np.float32)
        if delta_rel is not None:
            k, r = delta_rel
            delta = sigma_max(delta_u_at(a, b, flow, alpha, k, decay)) * r
        out, n = fn(a, b, flow.copy() if flow is not None else None, alpha, iters, decay, delta)
        arrays = dict(prev=a, next=b, iters_run=np.int64(n), alpha=np.float64(alpha),
                      alpha_is_int=np.bool_(isinstance(alpha, int)), max_iters=np.int64(iters),
                      decay=np.float64(decay), decay_is_int=np.bool_(isinstance(decay, int)),
                      has_delta=np.bool_(delta is not None), delta=np.float64(0 if delta is None else delta))
        if flow is not None:
            arrays["flow_in"] = flow
        if h * w > BIG:
            idx = np.random.default_rng(seed).choice(h * w, 4096, replace=False)
            arrays.update(flow_sha256=np.bytes_(hashlib.sha256(out.tobytes()).hexdigest()), sample_index=idx,
                          flow_sample=out.reshape(-1, 2)[idx])
        else:
            arrays["flow_out"] = out
        path = os.path.join(OUT, f"hs_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}: iters {n}, {os.path.getsize(path)} B")


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
