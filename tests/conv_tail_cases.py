"""Inputs for the convolution tail (tf_flow_convolve_post_process_dev) and the float64 narrowing (tf_flow_narrow_dev),
built from tests/flow_ops_cases.py.  numpy only: no GPU, no reference checkout.

Every case is a float32 flow and a kernel; the flow is conv_flow() times a power of two chosen so that FORWARD is a
useful test of the convolved field (tests/test_conv_tail_cases.py asserts what "useful" means, from the oracle's
output).  `tail_form` is the tail behind the convolution written in the right form and in the wrong forms a fused
kernel could slip into; the CPU test ties the right form to the oracle and shows that every wrong one changes bits.

One rule is pinned here that numpy leaves open: FORWARD converts the clipped, rounded vector to an integer, and numpy's
cast of a NaN to int32 is undefined (it warns; x86 gives INT_MIN).  The project's kernels (k_pp_fwd_scatter and every
copy of its statements) convert a NaN to 0.  `expected()` therefore hands the oracle's direction handling the convolved
field with its NaN components set to 0 where direction is FORWARD -- the output of FORWARD holds no value of the field,
only source positions, so nothing else changes -- and the field as it is otherwise.
"""
from __future__ import annotations

import functools

import numpy as np

from tests.flow_ops_cases import (CONV_BOUNDARY, CONV_IMAGES, CONV_SMALL_KERNELS, conv_flow, conv_kernel, convolve_form,
                                  frozen)

f32, f64 = np.float32, np.float64
FORWARD, BACKWARD, NONE = 0, 1, -1
DIRECTIONS = (FORWARD, BACKWARD, NONE)
THIN_IMAGES = ((1, 1), (1, 129), (33, 1))
THIN_KERNELS = ((16, 1), (1, 2))
SCALES = tuple(2.0 ** e for e in (0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6, 7, -7, 8, -8))


@functools.lru_cache(maxsize=None)
def tail_cases() -> tuple:
    out = []

    def add(h, w, kh, kw, dtype, specials=False, tag=""):
        out.append(dict(name=f"tail.{h}x{w}.k{kh}x{kw}.{dtype}{tag}", h=h, w=w, kh=kh, kw=kw, dtype=dtype, specials=specials))

    for (h, w) in CONV_IMAGES:                              # tile edges, both types
        add(h, w, 3, 5, "f64")
        add(h, w, 2, 2, "f32")
    for (kh, kw) in CONV_SMALL_KERNELS:                     # kernel shapes: even sizes, one row, one column
        for dtype in ("f64", "f32"):
            if not ((kh, kw, dtype) in ((3, 5, "f64"), (2, 2, "f32"))):
                add(17, 65, kh, kw, dtype)
    for (kh, kw), dtype, nbytes, tiled in CONV_BOUNDARY:    # either side of the 64 KB rule
        add(17, 65, kh, kw, dtype, tag=".lds%d" % nbytes)
    for (h, w) in THIN_IMAGES:
        for (kh, kw) in THIN_KERNELS:
            for dtype in ("f64", "f32"):
                add(h, w, kh, kw, dtype, tag=".thin")
    for dtype in ("f64", "f32"):                            # +-inf and NaN beside +-0.0 taps
        add(17, 65, 3, 5, dtype, specials=True, tag=".nonfinite")
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def _clip(f: np.ndarray) -> np.ndarray:
    """source.py:361-362 on a copy, in the array's own type."""
    f = f.copy()
    h, w, _ = f.shape
    jj = np.arange(w, dtype=np.int32)[None, :]
    ii = np.arange(h, dtype=np.int32)[:, None]
    np.clip(f[:, :, 0], -jj, w - 1 - jj, out=f[:, :, 0])
    np.clip(f[:, :, 1], -ii, h - 1 - ii, out=f[:, :, 1])
    return f


def rounded_steps(clipped: np.ndarray) -> np.ndarray:
    """d = iy * W + ix of a clipped field, flat; a NaN component counts as 0 (see the module text)."""
    w = clipped.shape[1]
    with np.errstate(invalid="ignore"):
        fi = np.rint(np.where(np.isnan(clipped), 0, clipped)).astype(np.int64)
    return (fi[:, :, 1] * w + fi[:, :, 0]).ravel()


def tail_form(conv: np.ndarray, direction: int, form: str = "right") -> np.ndarray:
    """What follows the convolution in post_process (source.py:349-362), in the convolved field's type T; or
      clip_f32         the clip computed in float32 and widened (differs for T = float64)
      round_first      the stored vector rounded before the clip (the scatter's rounding applied to the output)
      first_write_wins FORWARD keeping the lowest source that claims a target"""
    t = conv.dtype
    h, w, _ = conv.shape

    def clip(f):
        return _clip(f.astype(f32)).astype(t) if form == "clip_f32" else _clip(f)

    if direction == NONE:
        return conv.copy()
    if direction == BACKWARD:
        return clip(np.rint(conv) if form == "round_first" else conv)
    d = rounded_steps(clip(conv))
    p = np.arange(h * w, dtype=np.int64)
    moving = d != 0
    tgt = np.clip(p[moving] + d[moving], 0, h * w - 1)
    if form == "first_write_wins":
        winner = np.full(h * w, h * w, np.int64)
        np.minimum.at(winner, tgt, p[moving])
        winner[winner == h * w] = -1
    else:
        winner = np.full(h * w, -1, np.int64)
        np.maximum.at(winner, tgt, p[moving])
    src = np.where(winner >= 0, winner, p)
    out = np.empty_like(conv)
    out[:, :, 0] = (src % w - p % w).reshape(h, w)
    out[:, :, 1] = (src // w - p // w).reshape(h, w)
    return clip(out)


def _kernel(c: dict) -> np.ndarray:
    return conv_kernel(c["kh"], c["kw"], c["dtype"], zeros=c["specials"])


def _badness(conv: np.ndarray) -> float:
    """How far the moving share of a convolved field is from one half; a field in which no two sources claim one
    target, or whose share leaves [0.1, 0.9], ranks behind every field that does better."""
    d = rounded_steps(_clip(conv))
    moving = d != 0
    share = float(moving.mean())
    p = np.arange(d.size)
    targets = np.clip(p[moving] + d[moving], 0, d.size - 1)
    collide = len(np.unique(targets)) < len(targets)
    return abs(share - 0.5) + (0 if collide and 0.1 <= share <= 0.9 else 1)


@functools.lru_cache(maxsize=None)
def _scale(name: str) -> float:
    """The power of two in SCALES (the first of equals) that makes FORWARD the most useful test, by _badness."""
    c = next(c for c in tail_cases() if c["name"] == name)
    base, kernel = conv_flow(c["h"], c["w"], c["specials"]), _kernel(c)
    conv = convolve_form(base, kernel)                      # (s * flow convolves to s * conv, up to rounding)
    with np.errstate(all="ignore"):
        return min(SCALES, key=lambda s: _badness(conv * conv.dtype.type(s)))


def tail_inputs(c: dict) -> tuple:
    """(flow, kernel) of a case: float32 (h, w, 2), and the kernel in its own type."""
    with np.errstate(all="ignore"):
        flow = (conv_flow(c["h"], c["w"], c["specials"]) * f32(_scale(c["name"]))).astype(f32)
    return frozen(flow), _kernel(c)


_EXPECTED: dict = {}


def expected(c: dict, direction: int) -> np.ndarray:
    """oracle.flow_ops_ref.post_process_with_kernel of the case, computed once (the convolution once per case)."""
    from oracle import flow_ops_ref as F
    key = c["name"]
    if key not in _EXPECTED:
        flow, kernel = tail_inputs(c)
        with np.errstate(all="ignore"):
            conv = np.stack([F.convolve_same(flow[:, :, 0], kernel), F.convolve_same(flow[:, :, 1], kernel)], axis=-1)
        per = {NONE: frozen(conv)}
        for d in (BACKWARD, FORWARD):
            given = np.where(np.isnan(conv), 0, conv).astype(conv.dtype) if d == FORWARD else conv.copy()
            with np.errstate(all="ignore"):
                per[d] = frozen(F.post_process_any(given, d))
        if not c["specials"]:                              # where no NaN can reach the cast: the oracle's own entry, whole
            for d in (BACKWARD, FORWARD):
                with np.errstate(all="ignore"):
                    whole = F.post_process_with_kernel(flow.copy(), kernel, d)
                assert whole.dtype == per[d].dtype and whole.tobytes() == per[d].tobytes(), (key, d)
        _EXPECTED[key] = per
    return _EXPECTED[key][direction]


def fma_conv(flow: np.ndarray, kernel: np.ndarray) -> np.ndarray:
    """The convolution with every product fused into its addition (float32 kernels)."""
    return convolve_form(flow, kernel, "fma")


# ---- the narrowing ------------------------------------------------------------------------------------------------
NARROW_VALUES = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 1.4999999999, 0.49999999999999994, 2.5000000000000004, 0.0, -0.0,
                          16383.5, -16383.5, np.nan], f64)
NARROW_COUNTS = (1, 2, 3, 255, 256, 257)


def narrow_input(count: int) -> np.ndarray:
    """`count` values: the list, again from the start where count is larger, the start moving with the count so that a
    short case is not always the head; every third NaN of the longer ones negative."""
    idx = (np.arange(count) + 3 * count) % len(NARROW_VALUES)
    a = NARROW_VALUES[idx].copy()
    nan_at = np.flatnonzero(np.isnan(a))
    a[nan_at[::3]] = np.copysign(np.nan, -1.0)
    return frozen(a)


def narrow_form(a: np.ndarray, mode: int, form: str = "right") -> np.ndarray:
    """float32(rint(x)) (mode 0) or float32(floor(x)) (mode 1) in double; `cast_first`: the cast before the rounding."""
    op = np.floor if mode else np.rint
    if form == "cast_first":
        return op(a.astype(f32))
    return op(a).astype(f32)
