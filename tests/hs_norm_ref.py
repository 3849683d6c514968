"""A numpy model of the staged convergence test of Horn-Schunck (transflow_amd/csrc/hs_norm.hip), for the tests only.

`values(du, dtype)` computes, in `dtype`, what the device's stages compute for a field du: the cheap bounds F, U, L, the
16 lower bounds of the power iteration in the device's order, and the three Gram bounds.  `decide(values, delta)` applies
the device's rule to them.  The formulas are the device's; the order of the sums is numpy's.  With
`dtype=np.longdouble` the same code is the yardstick of the float64 one and of the device.

The fields of the tests' sweep are generated here as well (numpy only), so that the CPU test of this model and the GPU
tests run the very same cases.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

GUARD = 1e-3
POWER_STEPS = 8
TINY_F2 = 2.0 ** -960          # hs_common.h: below it the squares of du are not trusted
UNDECIDED, NOT_CONVERGED, CONVERGED = -1, 0, 1
ST_BOUNDS, ST_POWER, ST_GRAM, ST_HOST = 0, 1, 2, 3


@dataclass
class Values:
    F: float
    U: float
    L: float
    power: np.ndarray   # [2 * POWER_STEPS] lower bounds: ||du x||, ||du^T y|| per step
    gram: np.ndarray    # [3] upper bounds of k = 1, 2, 4
    nonfinite: bool = False
    tiny: bool = False

    def upper(self):
        return [self.F, self.U] + list(self.gram)

    def lower(self):
        return [self.L] + list(self.power)


def _norm(x):
    return np.sqrt((x * x).sum())


def bounds(du, dtype=np.float64):
    """F = ||du||_F, U = sqrt(||du||_1 ||du||_inf), L = the largest column or row 2-norm."""
    m = np.asarray(du).astype(dtype)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        sq, ab = m * m, np.abs(m)
        F = np.sqrt(sq.sum())
        n1, ninf = ab.sum(axis=0).max(), ab.sum(axis=1).max()
        U = np.sqrt(n1 * ninf) if F * F >= TINY_F2 else np.sqrt(n1) * np.sqrt(ninf)     # (the product underflows)
        L = np.sqrt(max(sq.sum(axis=0).max(), sq.sum(axis=1).max()))
    return F, U, L


def power_bounds(du, dtype=np.float64):
    """From the normalised ones vector: y = du x, x = du^T (y / ||y||), ...; ||y|| and ||x|| of every step."""
    m = np.asarray(du).astype(dtype)
    one = dtype(1)
    x = np.ones(m.shape[1], dtype)
    inv = one / _norm(x)
    out = np.zeros(2 * POWER_STEPS, dtype)
    for step in range(POWER_STEPS):
        y = (m @ x) * inv
        n = _norm(y)
        out[2 * step] = n
        inv = one / n if n > 0 else dtype(0)
        x = (m.T @ y) * inv
        n = _norm(x)
        out[2 * step + 1] = n
        inv = one / n if n > 0 else dtype(0)
    return out


def gram_bounds(du, F, dtype=np.float64):
    """F ||G^k||_F^(1 / 2k) for k = 1, 2, 4, with G = A A^T on the smaller side and A = du / F."""
    m = np.asarray(du).astype(dtype)
    if not (F > 0 and np.isfinite(F)):
        return np.full(3, np.nan, dtype)
    a = m * (dtype(1) / F)
    if m.shape[0] > m.shape[1]:
        a = a.T
    g = a @ a.T
    out = np.zeros(3, dtype)
    for i, k in enumerate((1, 2, 4)):
        if k > 1:
            g = g @ g.T
        out[i] = F * _norm(g) ** (dtype(1) / dtype(2 * k))
    return out


def values(du, dtype=np.float64) -> Values:
    m = np.asarray(du)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        F, U, L = bounds(m, dtype)
        nonfinite = not (np.isfinite(F * F) and np.isfinite(U * U) and np.isfinite(m).all())
        tiny = not nonfinite and F * F < TINY_F2
        if nonfinite or tiny:    # the device runs no stage after the bounds
            return Values(F, U, L, np.full(2 * POWER_STEPS, np.nan, dtype), np.full(3, np.nan, dtype), nonfinite, tiny)
        return Values(F, U, L, power_bounds(m, dtype), gram_bounds(m, F, dtype))


def gram_k(v: Values, delta):
    """The first k of the Gram stage that certifies sigma < delta, or None."""
    lo = delta * (1 - GUARD)
    for k, b in zip((1, 2, 4), v.gram):
        if b < lo:
            return k
    return None


def decide(v: Values, delta):
    """(decision, stage) by the device's rule."""
    if v.nonfinite:
        return UNDECIDED, ST_HOST
    if not delta > 0:
        return NOT_CONVERGED, ST_BOUNDS
    hi, lo = delta * (1 + GUARD), delta * (1 - GUARD)
    if v.tiny:
        # (the device also leaves a denormal U to the host; no case of the tests has one)
        return (CONVERGED, ST_BOUNDS) if v.U < lo else (UNDECIDED, ST_HOST)
    if min(v.F, v.U) < lo:
        return CONVERGED, ST_BOUNDS
    if v.L >= hi:
        return NOT_CONVERGED, ST_BOUNDS
    for step in range(1, POWER_STEPS, 2):          # read back after every second step
        if (v.power[:2 * step + 2] >= hi).any():
            return NOT_CONVERGED, ST_POWER
    if gram_k(v, delta) is not None:
        return CONVERGED, ST_GRAM
    return UNDECIDED, ST_HOST


def comparand_margin(v: Values, delta):
    """The smallest relative distance of a value the rule compares from its threshold."""
    hi, lo = delta * (1 + GUARD), delta * (1 - GUARD)
    d = [abs(float(x) / lo - 1) for x in v.upper()] + [abs(float(x) / hi - 1) for x in v.lower()]
    return min(x for x in d if np.isfinite(x))


# ---- the sweep ------------------------------------------------------------------------------------------------
SEED = 2025
SHAPES = [(1, 1), (1, 300), (300, 1), (9, 200), (200, 9), (64, 64), (65, 63), (63, 65), (129, 257), (257, 129), (300, 517),
          (517, 300), (33, 600)]
FAMILIES = ("noise", "rank1n", "corner", "lastrow", "lastcol", "edges", "zerosum")
DTYPES = (np.float32, np.float64)
RELS = (0.5, 0.8, 0.9, 0.99, 1 - 1e-4, 1 + 1e-4, 1.01, 1.1, 2)     # sigma / delta
GUARD_BAND_RELS = (1 - 1e-4, 1 + 1e-4)


def orientation(h, w):
    return "square" if h == w else "portrait" if h > w else "landscape"


def field(family, h, w, dtype):
    """A field of the sweep, generated in float64 from SEED and cast; None where the family has none at this shape (a
    zero field: `zerosum` of a single column)."""
    rng = np.random.default_rng([SEED, FAMILIES.index(family), h, w])
    if family == "noise":
        m = rng.normal(size=(h, w))
    elif family == "rank1n":
        x, y = rng.normal(size=h), rng.normal(size=w)
        m = np.outer(x / np.linalg.norm(x), y / np.linalg.norm(y)) + 0.5 * rng.normal(size=(h, w)) / np.sqrt(h + w)
    elif family == "corner":
        q = min(5, h, w)
        m = np.zeros((h, w))
        m[h - q:, w - q:] = np.linalg.qr(rng.normal(size=(q, q)))[0]
    elif family == "lastrow":
        m = np.zeros((h, w))
        m[-1] = rng.normal(size=w)
    elif family == "lastcol":
        m = np.zeros((h, w))
        m[:, -1] = rng.normal(size=h)
    elif family == "edges":
        m = 1e-2 * rng.normal(size=(h, w))
        m[-1] += rng.normal(size=w)
        m[:, -1] += rng.normal(size=h)
    elif family == "zerosum":
        m = rng.normal(size=(h, w))
        m -= m.mean(axis=1, keepdims=True)
    else:
        raise ValueError(family)
    m = m.astype(dtype)
    return m if m.any() else None


def sweep():
    """(family, (h, w), dtype, field) of every case."""
    for h, w in SHAPES:
        for family in FAMILIES:
            for dtype in DTYPES:
                m = field(family, h, w, dtype)
                if m is not None:
                    yield family, (h, w), dtype, m
