"""Cases for the fused merge + upscale kernel and the magnitude view (transflow_amd/csrc/flowseam.hip), on top of
tests/flow_ops_cases.py.  numpy only: no GPU, no reference checkout.

The reference's outputs on these cases are recorded in tests/golden/seam.npz by tools/capture_golden_seam.py (key =
the case's name); the inputs are regenerated here.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import flow_ops_cases as K

f32 = np.float32

# ---- merge, then upscale ----------------------------------------------------------------------------------------------
# odd and even W*wf, pairs of output pixels that straddle two source pixels (odd wf), a row longer than one
# work-group's 256 lanes (129 * 7 = 903 pixels, 452 pairs), a single pixel
FUSED_SHAPES = ((1, 1), (5, 3), (9, 31), (2, 129))                     # (h, w)
FUSED_FACTORS = ((3, 2), (2, 3), (1, 5), (7, 1), (2, 1))               # (wf, hf)
FUSED_NS = (2, 3)


@functools.lru_cache(maxsize=None)
def fused_cases() -> tuple:
    out = []
    for kind in K.MERGE_KINDS:
        for n in ((2,) if kind == "absmax" else FUSED_NS):
            for (h, w) in FUSED_SHAPES:
                for (wf, hf) in FUSED_FACTORS:
                    out.append(dict(name=f"seam.{kind}.n{n}.{h}x{w}.wf{wf}.hf{hf}", kind=kind, n=n, h=h, w=w, wf=wf, hf=hf))
    return tuple(out)


def fused_inputs(c: dict) -> list:
    """K.merge_inputs of the case's value count, reshaped to (h, w, 2)."""
    return [K.frozen(f.reshape(c["h"], c["w"], 2).copy()) for f in K.merge_inputs(c["n"], c["h"] * c["w"] * 2)]


def fused_form(c: dict, flows) -> np.ndarray:
    return K.upscale_form(K.merge_form(c["kind"], flows), c["wf"], c["hf"])


# ---- the magnitude view ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def magnitude_vectors() -> np.ndarray:
    """(L, 2): vectors times the scale, the ones that matter most first (short cases take a prefix).  For every target
    t in 0, 0.5 (the tie of `binary`) and 1 and each of K.neighbours(t): the axis-aligned vectors of that length
    (sqrt(x * x) is |x| exactly) and general ones along (0.6, 0.8) whose second component steps through the floats
    around 0.8 t, so that their magnitudes land on t and on either side of it.  Then zeros of both signs, infinities,
    squares that overflow and that underflow, and as many values of K.render_pool() as fit as lengths along the axes and along
    (0.6, 0.8)."""
    v = []
    for t in (1.0, 0.5, 0.0):
        for m in K.neighbours(t):
            v += [(m, 0.0), (0.0, m), (-m, -0.0), (-0.0, -m)]
            x, y = f32(m) * f32(0.6), f32(m) * f32(0.8)
            lo = hi = y
            v.append((x, y))
            for _ in range(6):
                lo, hi = np.nextafter(lo, -K.INF, dtype=f32), np.nextafter(hi, K.INF, dtype=f32)
                v += [(x, lo), (-x, hi)]
    v += [(0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (K.INF, 1.0), (-K.INF, K.INF), (1.0, -K.INF), (3e38, 3e38), (2e19, 2e19),
          (1e-30, 1e-30), (1e-40, 0.0), (1.5, 0.0), (0.0, 2.5), (1e-23, 1e-23),
          (2.7e-23, 2.7e-23)]
    pool = K.render_pool()
    for i, m in enumerate(pool[:1023 - len(v)]):
        m = f32(abs(m))
        v.append([(m, 0.0), (0.0, -m), (m * f32(0.6), m * f32(0.8)), (-m * f32(0.8), m * f32(0.6))][i % 4])
    with np.errstate(all="ignore"):
        a = np.array(v, f32)
    assert len(a) <= 1023, len(a)
    return K.frozen(a)


def magnitude_input(n: int, scale: float, nans: bool) -> np.ndarray:
    """(1, n, 2): magnitude_vectors() / |scale| (a power of two: exact), in order, again from the start where n is
    larger.  NaN pixels at K.nan_pixels(n): x only, y only, both."""
    vals = magnitude_vectors()
    with np.errstate(all="ignore"):
        a = (vals[np.arange(n) % len(vals)] / f32(abs(scale))).astype(f32).reshape(1, n, 2)
    if nans:
        for k, i in enumerate(K.nan_pixels(n)):
            a[0, i, :] = [(K.NAN, a[0, i, 1]), (a[0, i, 0], K.NAN), (K.NAN, K.NAN)][k % 3]
    return K.frozen(a)


@functools.lru_cache(maxsize=None)
def magnitude_cases() -> tuple:
    """K.render1d_cases(): its pixel counts, scales, colours, `binary` both ways and planted NaNs."""
    return tuple(dict(c, name="mag." + c["name"]) for c in K.render1d_cases())


def magnitude_form(flow) -> np.ndarray:
    """numpy.sqrt(numpy.sum(numpy.power(f, 2), axis=2)) in the form the kernel states it: sqrtf(x * x + y * y)."""
    a = np.asarray(flow, f32)
    with np.errstate(all="ignore"):
        return np.sqrt(a[:, :, 0] * a[:, :, 0] + a[:, :, 1] * a[:, :, 1])


def magnitude_view_form(c: dict, flow) -> np.ndarray:
    return K.render1d_form(magnitude_form(flow), c["scale"], c["colors"], c["binary"])


def assert_magnitude_cases_reach_their_targets() -> None:
    """scale * magnitude sits on, below and above 0.5 and 1, for axis-aligned and for general vectors, within the
    first 1023 pixels of a case; and on 0 and just above it -- the float32 neighbours of 0 as lengths give 0 (their
    squares underflow); the smallest magnitudes that are not 0 come from squares that round to the smallest
    denormal."""
    a = magnitude_input(1023, 0.5, False)
    sm = f32(0.5) * magnitude_form(a)[0]
    general = (a[0, :, 0] != 0) & (a[0, :, 1] != 0)
    for t in (0.5, 1.0):
        lo, on, hi = K.neighbours(t)
        for sel in (general, ~general):
            assert (sm[sel] == on).any() and (sm[sel] == lo).any() and (sm[sel] == hi).any(), t
    tiny = K.neighbours(0.0)[2]
    assert ((a[0] == tiny / f32(0.5)).any(axis=1) & (sm == 0)).any() and ((sm > 0) & (sm < 1e-20)).any() and np.isinf(sm).any()
    assert np.signbit(a[0][(a[0] == 0)]).any()
