"""Horn-Schunck restated in numpy, for the tests only (the product never imports it).

transflow's `calc_optical_flow_horn_schunck` (flow/methods/horn_schunck.py) calls one OpenCV function,
`GaussianBlur(float32, (5, 5), 0)`, and four `scipy.ndimage.convolve`s.  Both are restated here in a form whose
rounding is pinned, so the module equals the reference bit for bit without OpenCV or scipy:

- The blur is OpenCV's fixed 5-tap kernel [1, 4, 6, 4, 1] / 16 in both directions with BORDER_REFLECT_101.  On
  uint8-valued input every partial sum is a multiple of 1/256 below 256: exact in float32 in any order, so it is
  computed here as an integer sum over 256.
- `scipy.ndimage.convolve(x, k)` (mode "reflect", origin 0) is a C-order sum over the nonzero weights of the flipped
  kernel, started at 0.0 and accumulated in float64, then cast to x's dtype.  For the even 2x2 kernels, output (i, j)
  reads inputs (i..i+1, j..j+1); for 3x3 the window is centred.  "reflect" is numpy's "symmetric" padding.
- Everything else is numpy on the same dtypes, in the reference's statement order (numpy 2 scalar promotion: a
  Python scalar takes the array's dtype).
"""
from __future__ import annotations

import numpy as np

X_KERNEL = np.array([[1, -1], [1, -1]]) * 0.25
Y_KERNEL = np.array([[1, 1], [-1, -1]]) * 0.25
T_KERNEL = np.ones((2, 2)) * 0.25
AVG_KERNEL = np.array([[1, 2, 1], [2, 0, 2], [1, 2, 1]]) / 12


def gaussian_blur5(img: np.ndarray) -> np.ndarray:
    """cv2.GaussianBlur(img, (5, 5), 0) for float32 images holding uint8 values (exact)."""
    x = np.asarray(img, np.float32)
    assert np.array_equal(x, np.round(x)) and x.min() >= 0 and x.max() <= 255, "uint8-valued input only"
    k = np.array([1, 4, 6, 4, 1], np.int64)
    p = np.pad(x.astype(np.int64), 2, mode="reflect")          # numpy "reflect" == BORDER_REFLECT_101
    h, w = x.shape
    rows = sum(k[i] * p[i:i + h, :] for i in range(5))
    acc = sum(k[j] * rows[:, j:j + w] for j in range(5))
    return (acc.astype(np.float64) / 256.0).astype(np.float32)


def convolve(x: np.ndarray, kernel: np.ndarray) -> np.ndarray:
    """scipy.ndimage.convolve(x, kernel) (mode "reflect") for the 2x2 and 3x3 kernels used here."""
    kh, kw = kernel.shape
    flipped = np.asarray(kernel, np.float64)[::-1, ::-1]
    top, left = (kh - 1) // 2, (kw - 1) // 2           # 3 -> 1 (centred), 2 -> 0 (reads i..i+1)
    p = np.pad(x, ((top, kh - 1 - top), (left, kw - 1 - left)), mode="symmetric")
    h, w = x.shape
    acc = np.zeros((h, w), np.float64)
    for a in range(kh):
        for b in range(kw):
            wt = flipped[a, b]
            if wt != 0:
                acc = acc + p[a:a + h, b:b + w].astype(np.float64) * wt
    return acc.astype(x.dtype)


def derivatives(prev_grey: np.ndarray, next_grey: np.ndarray):
    """ex, ey, et (float32) of the two blurred frames."""
    a = gaussian_blur5(np.asarray(prev_grey).astype(np.float32))
    b = gaussian_blur5(np.asarray(next_grey).astype(np.float32))
    ex = convolve(a, X_KERNEL) + convolve(b, X_KERNEL)
    ey = convolve(a, Y_KERNEL) + convolve(b, Y_KERNEL)
    et = convolve(b, T_KERNEL) - convolve(a, T_KERNEL)
    return ex, ey, et


def denominator(ex: np.ndarray, ey: np.ndarray, alpha) -> np.ndarray:
    """alpha ** 2 + ex ** 2 + ey ** 2, float32: the Python scalar is rounded to float32 first."""
    return (np.float32(alpha ** 2) + ex * ex) + ey * ey


def horn_schunck(prev_grey, next_grey, flow=None, alpha=1, max_iters=3, decay=0, delta=1, return_iters=False):
    """The reference function's result, bit for bit.  return_iters: also the number of iterations run."""
    ex, ey, et = derivatives(prev_grey, next_grey)
    if flow is None:                            # the float64 chain
        u = np.zeros(ex.shape)
        v = np.zeros(ex.shape)
    else:                                       # the float32 chain
        u = np.float32(decay) * flow[:, :, 0]
        v = np.float32(decay) * flow[:, :, 1]
    den = denominator(ex, ey, alpha)
    n = 0
    for _ in range(max_iters):
        n += 1
        u_avg = convolve(u, AVG_KERNEL)
        v_avg = convolve(v, AVG_KERNEL)
        c = (ex * u_avg + ey * v_avg + et) / den
        prev = u
        u = u_avg - ex * c
        v = v_avg - ey * c
        if delta is not None and np.linalg.norm(u - prev, 2) < delta:
            break
    out = np.stack([u, v], axis=-1).astype(np.float32)
    return (out, n) if return_iters else out


def sigma_max(du: np.ndarray) -> float:
    """The reference's convergence quantity, numpy.linalg.norm(du, 2)."""
    return float(np.linalg.norm(du, 2))


def delta_u_at(prev_grey, next_grey, flow, alpha, k, decay=0):
    """u_k - u_{k-1} (in the chain's dtype) of a run without early exit: for placing delta around sigma_k."""
    ex, ey, et = derivatives(prev_grey, next_grey)
    if flow is None:
        u, v = np.zeros(ex.shape), np.zeros(ex.shape)
    else:
        u, v = np.float32(decay) * flow[:, :, 0], np.float32(decay) * flow[:, :, 1]
    den = denominator(ex, ey, alpha)
    prev = u
    for _ in range(k):
        u_avg, v_avg = convolve(u, AVG_KERNEL), convolve(v, AVG_KERNEL)
        c = (ex * u_avg + ey * v_avg + et) / den
        prev = u
        u, v = u_avg - ex * c, v_avg - ey * c
    return u - prev
