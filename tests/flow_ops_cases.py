"""Deterministic edge cases for the flow-array kernels (transflow_amd/csrc/flowops.hip): thresholds, ties, tails and
tile edges.  numpy only: no GPU, no reference checkout.

Every family comes with `*_forms`: the operation written in the right form and in the named wrong forms a kernel
could slip into (a fused multiply-add, a sum in another order, `>=` for `>`, ...), and `assert_*_discriminate()`,
which fails unless every wrong form changes the family's output.  tests/test_flow_ops_cases.py runs those
assertions on the CPU, so a family that stops discriminating fails there before it can pass vacuously on the GPU.

The reference's outputs on these cases are recorded in tests/golden/flow_ops_edges.npz by
tools/capture_golden_flow_ops_edges.py (key = the case's name); the inputs are regenerated here.
"""
from __future__ import annotations

import functools
import math

import numpy as np

f32, f64 = np.float32, np.float64
INF, NAN = f32(np.inf), f32(np.nan)


def _from_bits(*words) -> np.ndarray:
    return np.array(words, np.uint32).view(np.float32)


def neighbours(x) -> tuple:
    """(the float32 below, the float32 nearest x, the float32 above)."""
    x = f32(x)
    return np.nextafter(x, -INF, dtype=f32), x, np.nextafter(x, INF, dtype=f32)


def frozen(a: np.ndarray) -> np.ndarray:
    a.flags.writeable = False
    return a


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Equal shape, type and bit patterns: the rule for values that were merely selected (NaN sign and payload count)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64, 1: np.uint8, 2: np.uint16}[a.dtype.itemsize]
    return bool((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)).all())


def same_values(a: np.ndarray, b: np.ndarray) -> bool:
    """The rule for values an operation computed: a NaN where the other has one (whatever its payload), equal bits
    everywhere else (so -0.0 is not 0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and same_bits(np.where(na, 0, a).astype(a.dtype), np.where(nb, 0, b).astype(a.dtype))


# =====================================================================================================================
# merge
# =====================================================================================================================
MERGE_KINDS = ("first", "sum", "average", "difference", "product", "maskbin", "masklin", "absmax")
MERGE_SELECTS = ("first", "absmax")           # kinds that hand a stored value on: compared with same_bits
MERGE_NS = (1, 2, 3, 8)
MERGE_COUNTS = (2, 254, 256, 258, 1026)       # h * w * 2: one block of 256 threads, its two sides, several blocks

QNAN, QNAN_NEG = _from_bits(0x7FC00000, 0xFFC12345)      # the default NaN; a negative one with a payload
P2, P2_LO, P2_HI = neighbours(0.2)[1], neighbours(0.2)[0], neighbours(0.2)[2]
MERGE_SPECIALS = np.array([0.0, -0.0, INF, -INF, QNAN, QNAN_NEG, 1.5, -1.5, P2, P2_LO, P2_HI, -P2, 0.1, 3.0, 1e-40], f32)
MERGE_SPECIALS[4:6] = (QNAN, QNAN_NEG)        # np.array() may not keep a payload: write the bits back
# (a + b) + c != a + (b + c) in float32
MERGE_TRIPLES = np.array([(1e8, -1e8, 1.0), (1.0, 2.0 ** -24, 2.0 ** -24), (3.0, -3.0, 2.0 ** -30), (1.1, 2.2, 3.3)], f32)


@functools.lru_cache(maxsize=None)
def _merge_columns(n: int) -> np.ndarray:
    """(n, C): every column is one value per flow.  Pairs of specials sit in the first flow and one later flow (the
    later position cycles through 1..n-1, so `NaN in a later operand only` reaches every position); the others hold
    ordinary values.  For n >= 3 the rounding triples follow, in the first three and in the last three flows, with
    zeros elsewhere.  Seeded noise fills the rest, with zeros in the later flows."""
    s = MERGE_SPECIALS
    rng = np.random.default_rng(1000 + n)
    cols = []
    if n == 1:
        cols += [[v] for v in s]
    else:
        filler = np.array([0.75, -1.25, 2.5, -0.375, 1.0, -6.0, 0.21875], f32)
        for p, (a, b) in enumerate((a, b) for a in s for b in s):
            c = filler[(np.arange(n) + p) % len(filler)].copy()
            c[0], c[1 + p % (n - 1)] = a, b
            cols.append(c)
        for first in (-0.0, 0.0):             # every later operand -0.0: their sum is -0.0 unless it started from 0
            cols.append(np.array([first] + [-0.0] * (n - 1), f32))
    if n >= 3:
        for t in MERGE_TRIPLES:
            for at in (0, n - 3):
                c = np.zeros(n, f32)
                c[at:at + 3] = t
                cols.append(c)
    rows = max(MERGE_COUNTS) - len(cols)     # the longest case holds every special column
    noise = rng.normal(0, 2, (rows, n)).astype(f32)
    noise[:, 1:][rng.random((rows, n - 1)) < 0.25] = 0
    m = np.array(cols + list(noise), f32).reshape(-1, n)
    k = len(s) if n == 1 else len(s) ** 2
    for j in range(n):                        # the payloads again, for the same reason
        col = m[:k, j]
        col[np.isnan(col) & np.signbit(col)] = QNAN_NEG
    return frozen(np.ascontiguousarray(m.T))


def merge_inputs(n: int, count: int) -> list:
    """n flows of shape (1, count / 2, 2).  Counts below the number of special columns start at another column each."""
    m = _merge_columns(n)
    c = m.shape[1]
    start = min((count * 37) % 200, c - count)
    return [frozen(m[j, start:start + count].copy().reshape(1, count // 2, 2)) for j in range(n)]


@functools.lru_cache(maxsize=None)
def merge_cases() -> tuple:
    out = []
    for kind in MERGE_KINDS:
        for n in ((2,) if kind == "absmax" else MERGE_NS):
            for count in MERGE_COUNTS:
                out.append(dict(name=f"merge.{kind}.n{n}.c{count}", kind=kind, n=n, count=count))
    return tuple(out)


def _fold(arrays, op):
    acc = arrays[0]
    for a in arrays[1:]:
        acc = op(acc, a)
    return acc


def merge_form(kind: str, flows, form: str = "right") -> np.ndarray:
    """Pipeline.FLOW_MERGING_FUNCTIONS[kind], all float32, or one of its wrong forms:
      right_to_left  sums and products folded from the last flow
      reciprocal     average as `* (1 / n)`
      no_zero_start  sums that start from their first operand instead of +0.0 (numpy.sum starts from add's identity,
                     Python's sum() from 0: operands that are all -0.0 sum to +0.0)
      ge             maskbin with `>=`
      double_0.2     maskbin comparing against the double 0.2
      no_abs         masklin without the absolute value
      second_on_tie  absmax preferring the second operand on equal magnitudes
      drop_nan       absmax as `a1 > a0 ? f1 : f0`: a NaN in the second operand is dropped
      fmax_nan       absmax preferring the operand that is not a NaN"""
    f = [np.asarray(a, f32) for a in flows]
    add, mul = (lambda x, y: x + y), (lambda x, y: x * y)
    order = (lambda xs: xs[::-1]) if form == "right_to_left" else (lambda xs: xs)
    with np.errstate(all="ignore"):
        if kind == "first":
            return f[0]
        zero = [] if form == "no_zero_start" else [np.zeros_like(f[0])]
        if kind == "sum":
            return _fold(zero + order(f), add)
        if kind == "average":
            s = _fold(zero + order(f), add)
            return s * (f32(1) / f32(len(f))) if form == "reciprocal" else s / f32(len(f))
        if kind == "difference":
            return f[0] - _fold((zero + order(f[1:])) or [np.zeros_like(f[0])], add)
        if kind == "product":
            return _fold(order(f), mul)
        if kind == "maskbin":
            if form == "ge":
                masks = [(np.abs(a) >= f32(0.2)).astype(f32) for a in f[1:]]
            elif form == "double_0.2":
                masks = [(np.abs(a).astype(f64) > 0.2).astype(f32) for a in f[1:]]
            else:
                masks = [(np.abs(a) > f32(0.2)).astype(f32) for a in f[1:]]
            return _fold([f[0]] + masks, mul)
        if kind == "masklin":
            return _fold([f[0]] + [a if form == "no_abs" else np.abs(a) for a in f[1:]], mul)
        if kind == "absmax":
            a0, a1 = np.abs(f[0]), np.abs(f[1])
            n0, n1 = np.isnan(a0), np.isnan(a1)
            if form == "second_on_tie":
                return np.where((a1 >= a0) | (n1 & ~n0), f[1], f[0])
            if form == "drop_nan":
                return np.where(a1 > a0, f[1], f[0])
            if form == "fmax_nan":
                return np.where(n0 | ((a1 > a0) & ~n1), f[1], f[0])
            return np.where((a1 > a0) | (n1 & ~n0), f[1], f[0])
    raise ValueError(kind)


# wrong form -> the flow counts at which it can differ at all (x / 2 and x / 8 equal x * 0.5 and x * 0.125; two
# terms commute)
MERGE_WRONG = {
    "sum": {"right_to_left": (3, 8), "no_zero_start": (1, 2, 3, 8)},
    "average": {"right_to_left": (3, 8), "reciprocal": (3,), "no_zero_start": (1, 2, 3, 8)},
    "difference": {"right_to_left": (8,), "no_zero_start": (2, 3, 8)},
    "product": {"right_to_left": (3, 8)},
    "maskbin": {"ge": (2, 3, 8), "double_0.2": (2, 3, 8)},
    "masklin": {"no_abs": (2, 3, 8)},
    "absmax": {"second_on_tie": (2,), "drop_nan": (2,), "fmax_nan": (2,)},
}


def merge_same(kind: str, a, b) -> bool:
    return same_bits(a, b) if kind in MERGE_SELECTS else same_values(a, b)


def assert_merge_discriminates(right=merge_form) -> None:
    """`right(kind, flows)`: the statement under test (the oracle's, by default this module's)."""
    for t in MERGE_TRIPLES:
        assert (t[0] + t[1]) + t[2] != t[0] + (t[1] + t[2]), t
    for kind, forms in MERGE_WRONG.items():
        for form, ns in forms.items():
            for n in ns:
                flows = merge_inputs(n, 1026)
                assert not merge_same(kind, right(kind, flows), merge_form(kind, flows, form)), (kind, form, n)
    s = MERGE_SPECIALS
    for n in (2, 3, 8):                       # NaN in the first operand only, a later one only (each position), both
        m = np.isnan(_merge_columns(n)[:, :len(s) ** 2])
        later = m[1:].any(axis=0)
        assert (m[0] & ~later).any() and (m[0] & later).any()
        for j in range(1, n):
            assert (~m[0] & m[j]).any(), (n, j)
    a, b = (x.ravel() for x in merge_inputs(2, 1026))
    assert ((a == -b) & (a != 0) & np.isfinite(a)).any() and ((a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))).any()
    assert (np.isinf(a) & (b == 0)).any() and ((a == 0) & np.isinf(b)).any()
    assert {P2.tobytes(), P2_LO.tobytes(), P2_HI.tobytes()} <= {v.tobytes() for v in b}


# =====================================================================================================================
# upscale
# =====================================================================================================================
UPSCALE_FACTORS = ((1, 1), (1, 5), (7, 1), (3, 2), (2, 3), (16, 16))       # (wf, hf)
UPSCALE_SHAPES = ((1, 1), (5, 3), (9, 31))                                  # (h, w)


def upscale_input(h: int, w: int) -> np.ndarray:
    rng = np.random.default_rng(2000 + 100 * h + w)
    a = rng.normal(0, 3, (h, w, 2)).astype(f32)
    a[0, 0] = (0.1, -0.7)                                                   # 0.1f * 3, * 7 and -0.7f * 3, * 7 all round
    if h * w > 1:
        sp = np.array([INF, -INF, NAN, -0.0, 1e-40, 3e38, -3e38, 16777215.0, 1.0 / 3.0, 1e-38], f32)
        flat = a.reshape(-1)
        at = (np.arange(len(sp)) * 5 + 3) % flat.size                        # odd and even positions: both channels
        flat[at] = sp
    return frozen(a)


@functools.lru_cache(maxsize=None)
def upscale_cases() -> tuple:
    return tuple(dict(name=f"upscale.{h}x{w}.wf{wf}.hf{hf}", h=h, w=w, wf=wf, hf=hf)
                 for (h, w) in UPSCALE_SHAPES for (wf, hf) in UPSCALE_FACTORS)


def upscale_form(arr, wf: int, hf: int, form: str = "right") -> np.ndarray:
    """utils.upscale_array: (x * wf, y * hf) repeated hf times down and wf times across; wrong forms:
      swapped_scale   (x * hf, y * wf)
      swapped_repeat  repeated wf times down and hf times across
      swapped_axes    both
      truncated       the product truncated to float32 instead of rounded"""
    a = np.asarray(arr, f32)
    sw, sh = (hf, wf) if form in ("swapped_scale", "swapped_axes") else (wf, hf)
    rw, rh = (hf, wf) if form in ("swapped_repeat", "swapped_axes") else (wf, hf)
    with np.errstate(all="ignore"):
        if form == "truncated":
            exact = a.astype(f64) * np.array([sw, sh], f64)
            r = exact.astype(f32)
            away = np.isfinite(r) & (np.abs(r.astype(f64)) > np.abs(exact))
            p = np.where(away, np.nextafter(r, f32(0), dtype=f32), r)
        else:
            p = a * np.array([sw, sh], f32)
    return np.repeat(np.repeat(p, rh, axis=0), rw, axis=1)


def assert_upscale_discriminates(right=upscale_form) -> None:
    for c in upscale_cases():
        a, wf, hf = upscale_input(c["h"], c["w"]), c["wf"], c["hf"]
        if wf != hf:
            for form in ("swapped_scale", "swapped_repeat", "swapped_axes"):
                assert not same_values(right(a, wf, hf), upscale_form(a, wf, hf, form)), (c["name"], form)
        if 3 in (wf, hf) or 7 in (wf, hf):                  # some product is inexact: the one rounding shows
            exact = a.astype(f64) * np.array([wf, hf], f64)
            with np.errstate(all="ignore"):
                assert (np.isfinite(exact) & (exact.astype(f32).astype(f64) != exact)).any(), c["name"]
            if c["h"] * c["w"] > 1:
                assert not same_values(right(a, wf, hf), upscale_form(a, wf, hf, "truncated")), c["name"]
    assert any(c["h"] != c["w"] for c in upscale_cases())


# =====================================================================================================================
# render1d / render2d
# =====================================================================================================================
RENDER_COUNTS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 1027)       # every residue mod 4, either side of a block's last thread
R1_COLORS = ("#fe0340", "#03fe11")                            # cb - ca = -251, +251, -47: no zero channel
R1_DEFAULT = ("#000000", "#ffffff")
R2_COLORS = ("#7f2f7f", "#2f7f7f", "#7f7f2f", "#2f2f7f")     # channels 127 and 47: no zero, no sum above 2 * 255
R2_DEFAULT = ("#ffff00", "#0000ff", "#ff00ff", "#00ff00")
NAN_AT = (0, 17)                                              # and the last pixel


def parse_color(c: str) -> tuple:
    c = c.lstrip("#")
    return tuple(int(c[i:i + 2], 16) for i in (0, 2, 4))


R1_STEPS, R2_STEPS = (251, 47), (127, 47)                     # |cb - ca| per channel; the channels of R2_COLORS


@functools.lru_cache(maxsize=None)
def render_pool(steps: tuple = R1_STEPS) -> np.ndarray:
    """The values `scale * a` takes, the ones that matter most first (short cases take a prefix): 0 and 1 and their
    neighbours, the x.5 ties of `binary`, negative, huge and infinite values, then for every m and every d in
    `steps` the float32 neighbours of m / d -- where a term k * c, or ca + k * (cb - ca), sits on an integer and
    the truncation to a byte sees every rounding of the products and sums."""
    head = [0.0, 1.0, 0.5, 1.5, 2.5, *neighbours(1.0)[::2], -0.5, -0.0, *neighbours(0.5)[::2], -1.5, -2.5, 2.0 ** -126,
            1e-40, -0.25, -3.0, 1e30, -1e30, INF, -INF, 3.0, 0.25, 0.75]
    body = []
    for d in steps:
        for m in range(d + 1):
            body += list(neighbours(f32(m) / f32(d)))
    pool = np.array(head + body, f32)
    assert len(pool) <= 1023
    return frozen(pool)


def _plant(a: np.ndarray, nan_at) -> None:
    flat = a.reshape(-1, *a.shape[2:])
    for i in nan_at:
        flat[i] = NAN


def nan_pixels(n: int) -> tuple:
    return tuple(sorted({i for i in NAN_AT + (n - 1,) if i < n}))


def render1d_input(n: int, scale: float, nans: bool) -> np.ndarray:
    """(1, n): pool / scale (scale is a power of two: exact)."""
    pool = render_pool()
    a = (pool[np.arange(n) % len(pool)] / f32(scale)).astype(f32).reshape(1, n)
    if nans:
        _plant(a, nan_pixels(n))
    return frozen(a)


R2_PER_FORM = 120


@functools.lru_cache(maxsize=None)
def render2d_values() -> np.ndarray:
    """(L, 2): what (scale * x, scale * y) takes in the render2d cases.  One of k_y, k_b and one of k_m, k_g is always
    exactly 1, so with whole-number colours a pixel shows a rounding only where its sum lands within an ulp of a
    whole number *and* the wrong form rounds the other way; the neighbours of m / d alone rarely do both.  So the
    body is found by a search: the candidates are the floats up to three steps either side of m / d, for every m
    and both channel values d, put into one coefficient at a time -- (-v, 0) moves k_y alone, (v, 0) k_b, (0, -v) k_m,
    (0, v) k_g -- and into both channels at once; for every wrong form of render2d_form the search keeps up to
    R2_PER_FORM candidates, spread over the whole list, on which that form changes a byte.  The head, which short
    cases take a prefix of, sends the special values of render_pool() through each coefficient in turn."""
    def pixels(values):
        v = np.asarray(values, f32)
        u = v[(np.arange(len(v)) * 5 + 11) % len(v)]
        z = np.zeros_like(v)
        return np.stack([np.stack([-v, z], -1), np.stack([v, z], -1), np.stack([z, -v], -1), np.stack([z, v], -1),
                         np.stack([v, -u], -1)], axis=1).reshape(-1, 2)

    head = pixels(render_pool(()))
    cand = []
    for d in R2_STEPS:
        for m in range(d + 1):
            v = f32(m) / f32(d)
            lo = hi = v
            for _ in range(3):
                lo, hi = np.nextafter(lo, -INF, dtype=f32), np.nextafter(hi, INF, dtype=f32)
                cand += [lo, hi]
            cand.append(v)
    cand = pixels(cand)
    good = render2d_form(cand[None], 1, R2_COLORS)
    keep = set()
    for form in R2_WRONG:
        hit = np.flatnonzero((render2d_form(cand[None], 1, R2_COLORS, form) != good).any(axis=-1)[0])
        keep.update(hit[np.unique(np.linspace(0, len(hit) - 1, min(len(hit), R2_PER_FORM)).astype(int))] if len(hit) else ())
    vals = np.concatenate([head, cand[sorted(keep)]]).astype(f32)
    assert len(vals) <= 1023, len(vals)
    return frozen(vals)


def render2d_input(n: int, scale: float, nans: bool) -> np.ndarray:
    """(1, n, 2): render2d_values() / scale, in order, again from the start where n is larger.  NaN pixels: x only, y
    only, both."""
    vals = render2d_values()
    a = (vals[np.arange(n) % len(vals)] / f32(scale)).astype(f32).reshape(1, n, 2)
    if nans:
        for k, i in enumerate(nan_pixels(n)):
            a[0, i, :] = [(NAN, a[0, i, 1]), (a[0, i, 0], NAN), (NAN, NAN)][k % 3]
    return frozen(a)


@functools.lru_cache(maxsize=None)
def render1d_cases() -> tuple:
    out = []
    for binary in (False, True):
        b = "binary" if binary else "linear"
        for n in RENDER_COUNTS:
            out.append(dict(name=f"render1d.{b}.n{n}", n=n, scale=0.5, colors=R1_COLORS, binary=binary, nans=False))
        out.append(dict(name=f"render1d.{b}.n1027.negscale", n=1027, scale=-0.25, colors=R1_COLORS, binary=binary, nans=False))
        out.append(dict(name=f"render1d.{b}.n1027.default", n=1027, scale=0.5, colors=R1_DEFAULT, binary=binary, nans=False))
        for n in (1024, 1027):
            out.append(dict(name=f"render1d.{b}.n{n}.nan", n=n, scale=0.5, colors=R1_COLORS, binary=binary, nans=True))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def render2d_cases() -> tuple:
    out = [dict(name=f"render2d.n{n}", n=n, scale=0.5, colors=R2_COLORS, nans=False) for n in RENDER_COUNTS]
    out.append(dict(name="render2d.n1027.negscale", n=1027, scale=-0.25, colors=R2_COLORS, nans=False))
    out.append(dict(name="render2d.n1027.default", n=1027, scale=0.5, colors=R2_DEFAULT, nans=False))
    out += [dict(name=f"render2d.n{n}.nan", n=n, scale=0.5, colors=R2_COLORS, nans=True) for n in (1024, 1027)]
    return tuple(out)


def _fma32(a, b, c):
    """a * b + c rounded once to float32 (the product of two float32 is exact in float64)."""
    return (a.astype(f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _to_u8(frame, form):
    v = np.clip(frame, 0, 255)
    if form == "nearest":
        v = np.rint(v)
    return np.where(np.isnan(v), 0, v).astype(np.uint8)        # NaN pixels: see nan_pixels(); never compared through this


def render1d_form(arr, scale, colors, binary, form: str = "right") -> np.ndarray:
    """output/render.py:9-27, or: fma_a / fma_b (the first / second product fused into the addition), half_up
    (`binary` rounding x.5 up instead of to even), nearest (the byte rounded instead of truncated)."""
    a = np.asarray(arr, f32)
    ca, cb = (np.array(parse_color(c), f32) for c in colors)
    with np.errstate(all="ignore"):
        sa = f32(scale) * a
        if binary:
            r = np.floor(sa + f32(0.5)) if form == "half_up" else np.rint(sa)
            kb = np.clip(r, 0, 1)[..., None]
            ka = f32(1) - kb
        else:
            ka, kb = np.clip(f32(1) - sa, 0, 1)[..., None], np.clip(sa, 0, 1)[..., None]
        if form == "fma_a":
            frame = _fma32(ka, ca, kb * cb)
        elif form == "fma_b":
            frame = _fma32(kb, cb, ka * ca)
        else:
            frame = ka * ca + kb * cb
        return _to_u8(frame, form)


def render2d_form(arr, scale, colors, form: str = "right") -> np.ndarray:
    """output/render.py:30-48, or: fma_y / fma_b / fma_m / fma_g (that product fused into its addition), nested
    (y + (b + (m + g))), pairwise ((y + b) + (m + g)), half_per_term, nearest."""
    a = np.asarray(arr, f32)
    cy, cb, cm, cg = (np.array(parse_color(c), f32) for c in colors)
    one, half = f32(1), f32(0.5)
    with np.errstate(all="ignore"):
        sx, sy = f32(scale) * a[:, :, 0], f32(scale) * a[:, :, 1]
        ky, kb = np.clip(one + sx, 0, 1)[..., None], np.clip(one - sx, 0, 1)[..., None]
        km, kg = np.clip(one + sy, 0, 1)[..., None], np.clip(one - sy, 0, 1)[..., None]
        ty, tb, tm, tg = ky * cy, kb * cb, km * cm, kg * cg
        if form == "fma_y":
            total = (_fma32(ky, cy, tb) + tm) + tg
        elif form == "fma_b":
            total = (_fma32(kb, cb, ty) + tm) + tg
        elif form == "fma_m":
            total = _fma32(km, cm, ty + tb) + tg
        elif form == "fma_g":
            total = _fma32(kg, cg, (ty + tb) + tm)
        elif form == "nested":
            total = ty + (tb + (tm + tg))
        elif form == "pairwise":
            total = (ty + tb) + (tm + tg)
        elif form == "half_per_term":
            total = ((half * ty + half * tb) + half * tm) + half * tg
            return _to_u8(total, form)
        else:
            total = ((ty + tb) + tm) + tg
        return _to_u8(half * total, form)


R1_WRONG = {False: ("fma_a", "fma_b", "nearest"), True: ("half_up",)}
R2_WRONG = ("fma_y", "fma_b", "fma_m", "fma_g", "nested", "pairwise", "nearest")
# half_per_term is no wrong form: halving a float32 is exact short of underflow, and a term that underflows is far
# below a byte's step, so 0.5 * (a + b + c + d) and 0.5 * a + 0.5 * b + 0.5 * c + 0.5 * d give the same bytes on every
# input.  assert_render_discriminates() states that equality instead of a difference.


def assert_render_discriminates(right1d=render1d_form, right2d=render2d_form) -> None:
    pool = render_pool()
    for p in (pool, render2d_values()[:, 0], render2d_values()[:, 1]):
        for v in (0.0, 1.0, 0.5, 1.5, 2.5, INF, -INF, 1e30, -1e30):
            assert (p == f32(v)).any(), v
        assert (p < 0).any()
    for steps, colors in ((R1_STEPS, R1_COLORS), (R2_STEPS, R2_COLORS)):
        ch = np.array([parse_color(c) for c in colors])
        assert set(np.abs(ch[1] - ch[0])) <= set(steps) if len(colors) == 2 else set(ch.ravel()) <= set(steps)
    for c in render1d_cases():
        if c["n"] < 1023 or c["nans"] or c["colors"] == R1_DEFAULT:
            continue
        a = render1d_input(c["n"], c["scale"], False)
        assert same_bits(f32(c["scale"]) * a.ravel()[:len(pool)], pool[:c["n"]]), c["name"]     # scale * a is the pool, exactly
        good = right1d(a, c["scale"], c["colors"], c["binary"])
        for form in R1_WRONG[c["binary"]]:
            assert not same_bits(good, render1d_form(a, c["scale"], c["colors"], c["binary"], form)), (c["name"], form)
    for c in render2d_cases():
        if c["n"] < 1023 or c["nans"] or c["colors"] == R2_DEFAULT:
            continue
        a = render2d_input(c["n"], c["scale"], False)
        assert same_bits(f32(c["scale"]) * a[0, :len(render2d_values())], render2d_values()[:c["n"]]), c["name"]
        good = right2d(a, c["scale"], c["colors"])
        for form in R2_WRONG:
            assert not same_bits(good, render2d_form(a, c["scale"], c["colors"], form)), (c["name"], form)
        assert same_bits(good, render2d_form(a, c["scale"], c["colors"], "half_per_term")), c["name"]
    for colors in (R1_COLORS, R2_COLORS):
        assert all(ch != 0 for c in colors for ch in parse_color(c))
    assert nan_pixels(1027) == (0, 17, 1026) and nan_pixels(1024) == (0, 17, 1023)


# =====================================================================================================================
# convolution
# =====================================================================================================================
CV_TW, CV_TH = 64, 16                         # the LDS tile of k_flow_convolve_tiled
CONV_IMAGES = ((1, 1), (15, 63), (16, 64), (17, 65), (33, 129), (1, 129), (33, 1), (16, 65), (17, 63), (15, 64))   # (h, w)
CONV_SMALL_KERNELS = ((1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (16, 1))
CONV_DTYPES = {"f64": np.float64, "f32": np.float32, "f16": np.float16, "i64": np.int64, "bool": np.bool_}
# 64 KB of dynamic LDS decides between the tiled and the per-pixel kernel: (kernel shape, type, bytes, tiled?)
CONV_BOUNDARY = (((14, 148), "f64", 65536, True), ((21, 104), "f64", 65568, False),
                 ((79, 17), "f32", 65532, True), ((91, 10), "f32", 65544, False))


def conv_tile_bytes(kh: int, kw: int, itemsize: int) -> int:
    """tf_flow_convolve_dev's rule: the float2 tile, padded to 16 bytes, then the kernel's values."""
    return (((CV_TW + kw - 1) * (CV_TH + kh - 1) * 8 + 15) & ~15) + kh * kw * itemsize


def conv_flow(h: int, w: int, specials: bool = False) -> np.ndarray:
    rng = np.random.default_rng(3000 + 1000 * h + w)
    a = rng.normal(0, 3, (h, w, 2)).astype(f32)
    if specials:                              # a corner and the interior, in either channel, far enough apart to tell
        a[0, 0, 0], a[h - 1, w - 1, 1] = INF, NAN
        a[h // 2, w // 3, 0], a[h // 2, w // 3, 1] = -INF, INF
        a[h // 3, (2 * w) // 3, 0] = NAN
    return frozen(a)


def conv_kernel(kh: int, kw: int, dtype: str, zeros: bool = False) -> np.ndarray:
    rng = np.random.default_rng(4000 + 100 * kh + kw + 7 * sorted(CONV_DTYPES).index(dtype))
    t = CONV_DTYPES[dtype]
    if dtype == "i64":
        k = rng.integers(-3, 4, (kh, kw)).astype(t)
    elif dtype == "bool":
        k = rng.random((kh, kw)) < 0.6
    else:
        k = rng.normal(0, 0.3, (kh, kw)).astype(t)
    if zeros:                                 # zeros of both signs among the taps
        flat = k.reshape(-1)
        flat[1::4] = 0.0
        flat[3::4] = -0.0
    return frozen(k)


@functools.lru_cache(maxsize=None)
def convolve_cases() -> tuple:
    out = []

    def add(h, w, kh, kw, dtype, specials=False, tag=""):
        out.append(dict(name=f"conv.{h}x{w}.k{kh}x{kw}.{dtype}{tag}", h=h, w=w, kh=kh, kw=kw, dtype=dtype, specials=specials))

    for (h, w) in CONV_IMAGES:                              # tile edges
        if (h, w) == (33, 129):
            add(h, w, 3, 5, "f32")
            add(h, w, 2, 2, "f64")
        else:
            add(h, w, 3, 5, "f64")
            add(h, w, 2, 2, "f32")
    for (kh, kw) in CONV_SMALL_KERNELS:                     # kernel shapes: even sizes, one row, one column
        if (kh, kw) != (3, 5):
            add(17, 65, kh, kw, "f64")
        if (kh, kw) != (2, 2):
            add(16, 64, kh, kw, "f32")
    for dtype in ("f16", "i64", "bool"):
        add(17, 65, 3, 5, dtype)
        add(15, 63, 2, 2, dtype)
    add(3, 4, 9, 9, "f64")                                  # larger than the image on both axes
    add(3, 4, 9, 9, "f32")
    for (kh, kw), dtype, nbytes, tiled in CONV_BOUNDARY:
        add(17, 65, kh, kw, dtype, tag=".lds%d" % nbytes)
    for dtype, (kh, kw) in (("f64", (3, 5)), ("f32", (3, 5)), ("f64", (2, 2)), ("f32", (4, 4))):
        add(17, 65, kh, kw, dtype, specials=True, tag=".nonfinite")
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def convolve_inputs(c: dict) -> tuple:
    return conv_flow(c["h"], c["w"], c["specials"]), conv_kernel(c["kh"], c["kw"], c["dtype"], zeros=c["specials"])


def conv_result_type(kernel: np.ndarray):
    return np.result_type(np.float32, kernel.dtype)


def convolve_form(flow: np.ndarray, kernel: np.ndarray, form: str = "right") -> np.ndarray:
    """scipy.signal.convolve2d(channel, kernel, "same", "fill", 0) on both channels: kernel rows, then columns, each
    product and each sum rounded in the result type, the centre at (k - 1) // 2; or
      centre_hi      the centre at k // 2
      cols_first     columns summed before rows
      fma            every product fused into its addition (float32 results only)
      other_acc      accumulated in the other float type, rounded at the end
      skip_zero_taps zero taps left out (0 * inf makes no NaN)"""
    rt = conv_result_type(kernel)
    at = rt if form != "other_acc" else np.dtype(f64 if rt == f32 else f32)
    k = np.asarray(kernel).astype(rt).astype(at)
    kh, kw = k.shape
    h, w, _ = flow.shape
    oy, ox = (kh // 2, kw // 2) if form == "centre_hi" else ((kh - 1) // 2, (kw - 1) // 2)
    pad = np.zeros((h + 2 * kh, w + 2 * kw, 2), at)
    pad[kh:kh + h, kw:kw + w] = flow
    taps = [(j, i) for j in range(kh) for i in range(kw)]
    if form == "cols_first":
        taps = [(j, i) for i in range(kw) for j in range(kh)]
    out = np.zeros((h, w, 2), at)
    with np.errstate(all="ignore"):
        for j, i in taps:
            if form == "skip_zero_taps" and k[j, i] == 0:
                continue
            y0, x0 = kh + oy - j, kw + ox - i
            v = pad[y0:y0 + h, x0:x0 + w]
            if form == "fma":
                assert rt == f32
                out = _fma32(v, k[j, i], out)
            else:
                out = out + k[j, i] * v
        return out.astype(rt)


def assert_convolve_discriminates(right=convolve_form) -> None:
    cases = convolve_cases()
    for (kh, kw), dtype, nbytes, tiled in CONV_BOUNDARY:
        assert conv_tile_bytes(kh, kw, 8 if dtype == "f64" else 4) == nbytes and (nbytes <= 65536) == tiled
    seen = set()
    for c in cases:
        flow, kernel = convolve_inputs(c)
        good = right(flow, kernel)
        assert good.dtype == conv_result_type(kernel)
        forms = []
        if c["kh"] % 2 == 0 or c["kw"] % 2 == 0:
            forms.append("centre_hi")
        if min(c["kh"], c["kw"], c["h"], c["w"]) > 1 and c["dtype"] not in ("i64", "bool") and not c["specials"]:
            forms.append("cols_first")                     # one row or column has one order; small integers sum exactly
        if c["dtype"] in ("f64", "f32") and c["kh"] * c["kw"] > 1 and not c["specials"] and c["h"] * c["w"] > 1:
            forms.append("other_acc")
            if c["dtype"] == "f32":
                forms.append("fma")
        if c["specials"]:
            forms.append("skip_zero_taps")
        for form in forms:
            assert not same_values(good, convolve_form(flow, kernel, form)), (c["name"], form)
            seen.add((form, str(good.dtype)))
        if c["specials"]:
            taps = np.asarray(kernel).ravel()
            assert (np.signbit(taps) & (taps == 0)).any() and (~np.signbit(taps) & (taps == 0)).any()
            assert np.isnan(good).any() and not np.isnan(good).all()
    for form in ("centre_hi", "cols_first", "other_acc", "skip_zero_taps"):
        assert (form, "float32") in seen and (form, "float64") in seen, form
    assert ("fma", "float32") in seen
    assert {c["w"] for c in cases} >= {1, 63, 64, 65, 129} and {c["h"] for c in cases} >= {1, 15, 16, 17, 33}


# =====================================================================================================================
# grey
# =====================================================================================================================
def all_bgr_triples() -> np.ndarray:
    """All 2^24 BGR triples as one 4096 x 4096 frame: pixel i holds B = i & 255, G = (i >> 8) & 255, R = i >> 16."""
    i = np.arange(1 << 24, dtype=np.uint32)
    t = np.empty((1 << 24, 3), np.uint8)
    for c in range(3):
        t[:, c] = (i >> (8 * c)) & 255
    return t.reshape(4096, 4096, 3)


def grey_of(bgr: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(BGR2GRAY) on bytes, as this project states it: (B*3735 + G*19235 + R*9798 + 2^14) >> 15."""
    p = np.asarray(bgr)
    b, g, r = (p[..., c].astype(np.uint32) for c in range(3))           # 255 * 32768 + 16384 < 2^32
    return ((b * np.uint32(3735) + g * np.uint32(19235) + r * np.uint32(9798) + np.uint32(16384)) >> np.uint32(15)).astype(np.uint8)


def nearest_map(src: int, dst: int, form: str = "right") -> list:
    """cv2.resize(INTER_NEAREST)'s source index of every destination index, in a plain loop:
    min(floor(x * (1.0 / (dst / src))), src - 1) in doubles; or
      rational   x * src // dst, exact
      one_div    floor(x * (src / dst))
      float32    the right form in float32"""
    out = []
    for x in range(dst):
        if form == "rational":
            i = x * src // dst
        elif form == "one_div":
            i = math.floor(x * (src / dst))
        elif form == "float32":
            i = math.floor(f32(x) * (f32(1) / (f32(dst) / f32(src))))
        else:
            i = math.floor(x * (1.0 / (dst / src)))
        out.append(min(int(i), src - 1))
    return out


NEAREST_WRONG = ("rational", "one_div", "float32")
SEARCH_SRC, SEARCH_DST = 16, 160


def _maps(src: int, dst: int) -> dict:
    """The four maps of nearest_map, vectorised (the search walks 2560 pairs)."""
    x = np.arange(dst)
    m = {"right": np.floor(x * (1.0 / (dst / src))), "rational": x * src // dst, "one_div": np.floor(x * (src / dst)),
         "float32": np.floor(x.astype(f32) * (f32(1) / (f32(dst) / f32(src))))}
    return {k: np.minimum(v.astype(np.int64), src - 1) for k, v in m.items()}


def differs_from(src: int, dst: int) -> tuple:
    """The wrong maps that the pair tells apart from the right one."""
    m = _maps(src, dst)
    return tuple(f for f in NEAREST_WRONG if (m[f] != m["right"]).any())


@functools.lru_cache(maxsize=None)
def discriminating_pairs() -> tuple:
    """Every (src, dst) with src <= 16 and dst <= 160 on which the right map differs from all three wrong ones."""
    return tuple((s, d) for s in range(1, SEARCH_SRC + 1) for d in range(1, SEARCH_DST + 1)
                 if len(differs_from(s, d)) == len(NEAREST_WRONG))


@functools.lru_cache(maxsize=None)
def resize_cases() -> tuple:
    """Frames resized by one pair on x and another on y.  The pairs: those named in the issue, then the search's,
    taken from both ends of its list; `ingest` marks the cases whose destination is at least 33 px on both axes
    (the smallest frame the flow methods' own ingests take)."""
    pairs = discriminating_pairs()
    named_all, named_some = ((6, 34), (9, 51)), ((2, 98), (3, 147), (6, 94))
    for p in named_all:
        assert p in pairs, p
    for p in named_some:
        assert differs_from(*p), p
    big = [p for p in pairs if p[1] >= 33 and p not in named_all]
    small = [p for p in pairs if p[1] < 33]
    chosen = [((6, 34), (9, 51)), ((9, 51), (6, 34)), ((2, 98), (3, 147)), ((6, 94), (2, 98)), ((3, 147), (6, 94))]
    chosen += [(big[i], big[-1 - i]) for i in range(min(3, len(big) // 2))]
    chosen += [(small[i], small[-1 - i]) for i in range(min(3, len(small) // 2))]
    out = []
    for (sx, dx), (sy, dy) in chosen:
        assert (sx, dx) != (sy, dy)
        out.append(dict(name=f"grey.x{sx}to{dx}.y{sy}to{dy}", sx=sx, dx=dx, sy=sy, dy=dy,
                        ingest=min(dx, dy) >= 33 and (sx, dx) in pairs and (sy, dy) in pairs))
    return tuple(out)


def resize_frame(c: dict) -> np.ndarray:
    """The (sy, sx, 3) source frame of a case: seeded bytes, no two neighbours of equal grey."""
    rng = np.random.default_rng(5000 + 160 * c["sx"] + c["dx"] + 7 * c["sy"])
    while True:
        f = rng.integers(0, 256, (c["sy"], c["sx"], 3), dtype=np.uint8)
        g = grey_of(f).astype(int)
        if (np.diff(g, axis=0) != 0).all() and (np.diff(g, axis=1) != 0).all():
            return frozen(f)


def gentle_frame(c: dict) -> np.ndarray:
    """A (sy, sx, 3) source frame whose neighbours differ in every channel, by 2 to 4 levels: for a consumer that
    interpolates the resized frame in float32 (LiteFlowNet's prep), where a float32 sample position off by 2^-16
    times a step of up to 255 levels would swamp the 2^-20 it is held to.  A pixel taken from the wrong source index
    is still 2 levels, 2^-7, off."""
    y, x = np.mgrid[0:c["sy"], 0:c["sx"]]
    f = np.stack([40 + 3 * x + 2 * y, 200 - 2 * x - 4 * y, 90 + 4 * x + 3 * y], axis=-1)
    assert f.min() >= 0 and f.max() <= 255
    return frozen(f.astype(np.uint8))


def resized(frame: np.ndarray, dx: int, dy: int, form_x: str = "right", form_y: str = "right", swap: bool = False) -> np.ndarray:
    """The frame resized to dx x dy by nearest_map; `swap` steps along x by y's ratio and along y by x's."""
    sy, sx, _ = frame.shape
    ix, iy = nearest_map(sx, dx, form_x), nearest_map(sy, dy, form_y)
    if swap:
        ix = [min(math.floor(x * (1.0 / (dy / sy))), sx - 1) for x in range(dx)]
        iy = [min(math.floor(y * (1.0 / (dx / sx))), sy - 1) for y in range(dy)]
    return np.ascontiguousarray(np.asarray(frame)[np.array(iy)][:, np.array(ix)])


def assert_grey_discriminates() -> None:
    pairs = discriminating_pairs()
    assert len(pairs) >= 8
    cases = resize_cases()
    assert sum(c["ingest"] for c in cases) >= 3 and sum(c["dx"] * c["sy"] != c["dy"] * c["sx"] for c in cases) >= 3
    for c in cases:
        f = resize_frame(c)
        good = grey_of(resized(f, c["dx"], c["dy"]))
        for axis, (s, d) in (("x", (c["sx"], c["dx"])), ("y", (c["sy"], c["dy"]))):
            for form in differs_from(s, d):
                bad = resized(f, c["dx"], c["dy"], form if axis == "x" else "right", form if axis == "y" else "right")
                assert not same_bits(good, grey_of(bad)), (c["name"], axis, form)
        if c["dx"] * c["sy"] != c["dy"] * c["sx"]:         # 6 -> 34 and 9 -> 51 are one ratio
            assert not same_bits(good, grey_of(resized(f, c["dx"], c["dy"], swap=True))), c["name"]
        if c["ingest"]:
            f = gentle_frame(c)
            good = resized(f, c["dx"], c["dy"]).astype(int)
            for axis, (s, d) in (("x", (c["sx"], c["dx"])), ("y", (c["sy"], c["dy"]))):
                for form in NEAREST_WRONG:
                    bad = resized(f, c["dx"], c["dy"], form if axis == "x" else "right", form if axis == "y" else "right")
                    assert np.abs(bad.astype(int) - good).max(axis=(0, 1)).min() >= 2, (c["name"], axis, form)
    t = all_bgr_triples()[::257, ::17]
    for w in ((1868, 9617, 4899, 14), (3736, 19234, 9798, 15)):        # the 14-bit form; weights one step off
        p = t.astype(np.int64)
        other = ((p[..., 0] * w[0] + p[..., 1] * w[1] + p[..., 2] * w[2] + (1 << (w[3] - 1))) >> w[3]).astype(np.uint8)
        assert not same_bits(grey_of(t), other), w
