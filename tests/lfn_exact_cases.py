"""Inputs on which LiteFlowNet's convolutions have ONE right answer, and that answer, in numpy integer arithmetic.

Every term of every sum is a multiple of a unit u and sum|terms| < 2^24 u, so that any order of float32 additions gives
the same float32: the kernels (k_lfn_conv, k_lfn_conv_q, k_lfn_deconv) are compared with `expected` for equality of
bits (tests/test_gpu_liteflownet_exact.py); tests/test_lfn_exact_cases.py checks this file on the CPU.

  family   x                          w                         bias       modes              unit
  A        integers in [-8, 8]        integers in [-4, 4]       integers   f32 bf16 bf16x3    1
  B        {0, +-1, +-(1 +- 2^-9)}    {0, +-1, +-(1 +- 2^-9)}   integers   bf16 bf16x3        2^-9
  C        +-(1 + t 2^-8), t = 0..3   {0, +-1}                  integers   f32 bf16 bf16x3    2^-7 (bf16), 2^-8

A: every operand is a bfloat16 value, so the three modes must agree in every bit.  B: hi = +-1 and lo = +-2^-9; bf16
is sum xh wh, bf16x3 is sum (xh wh + xh wl + xl wh) and the dropped xl wl would show.  C: t = 1 is a tie that goes down
to the even mantissa, t = 3 a tie that goes up, so bf16 is sum q(x) w and differs from f32 and bf16x3, which are sum x w.

q and split are stated on the bits (`_rne_bf16`).  `conv_sum` also models wrong kernels (its keyword arguments): the CPU
test uses them to show that the cases discriminate.  Nothing here imports torch.
"""
from __future__ import annotations

import functools

import numpy as np

from transflow_amd import liteflownet as LF

MODES = ("f32", "bf16", "bf16x3")
FAMILY_MODES = {"A": MODES, "B": ("bf16", "bf16x3"), "C": MODES}
FAMILIES = tuple(FAMILY_MODES)
WEIGHT_SETS = FAMILIES + ("S",)             # S: the one-hot weights of the specials
QCONV_BK, CONV_BK = 32, 16                  # the K chunks of k_lfn_conv_q and k_lfn_conv
SCALE = 512                                 # every operand of every family times 2^9 is an integer
LIMIT = 1 << 24
_SEED = {"A": 11, "B": 12, "C": 13, "S": 14}
_LO = np.float32(2.0 ** -9)
_B_VALUES = np.array([0, 1, -1, 1 + _LO, 1 - _LO, -1 - _LO, -1 + _LO], np.float32)


def unit_den(family: str, mode: str) -> int:
    """1 / u of the family in the mode."""
    if mode not in FAMILY_MODES[family]:
        raise ValueError(f"family {family} is not exact in mode {mode}")
    return {"A": 1, "B": 512, "C": 128 if mode == "bf16" else 256}[family]


# ---- rounding to bfloat16, on the bits --------------------------------------------------------------------------------

def _values():
    """float32 values: normals of many magnitudes, exact ties between two bfloat16 values (even and odd below, both
    signs), their float32 neighbours, and the top of the range (the largest float32 values round to infinity)."""
    rng = np.random.default_rng(5)
    v = [rng.standard_normal(3000).astype(np.float32) * np.float32(10.0) ** rng.integers(-20, 20, 3000).astype(np.float32)]
    hi = rng.integers(0x0080, 0x7f7f, 500).astype(np.uint32)        # positive normal bfloat16 patterns
    hi[:4] = (0x3f80, 0x3f81, 0x7f7e, 0x7f7f)
    for low in (0x8000, 0x7fff, 0x8001, 0x0001, 0xffff, 0x0000):
        bits = (hi << np.uint32(16)) | np.uint32(low)
        v += [bits.view(np.float32), (bits | np.uint32(0x80000000)).view(np.float32)]
    v.append(np.array([0.0, -0.0, 3.4028235e38, -3.4028235e38, 3.3895314e38, 3.38e38, 1e38, -1e38], np.float32))
    return np.concatenate(v)


def _rne_bf16(x: np.ndarray) -> np.ndarray:
    """Round to nearest even on the bits: add 0x7fff plus the lowest kept bit, drop 16 bits (finite values; a carry out
    of the largest exponent is the infinity)."""
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return r.astype(np.uint32).view(np.float32)


def _half_up_bf16(x: np.ndarray) -> np.ndarray:
    """A wrong rounding: ties away from zero."""
    u = x.view(np.uint32).astype(np.uint64)
    return (((u + np.uint64(0x8000)) >> np.uint64(16)) << np.uint64(16)).astype(np.uint32).view(np.float32)


def _trunc_bf16(x: np.ndarray) -> np.ndarray:
    """A wrong rounding: the low 16 bits dropped."""
    return (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


_ROUNDINGS = {"rne": _rne_bf16, "half_up": _half_up_bf16, "trunc": _trunc_bf16}


def q(x: np.ndarray, rounding: str = "rne") -> np.ndarray:
    """x rounded to bfloat16, as float32; a NaN stays a NaN whatever its payload."""
    x = np.ascontiguousarray(x, np.float32)
    return np.where(np.isnan(x), np.float32(np.nan), _ROUNDINGS[rounding](x)).astype(np.float32)


def split(x: np.ndarray, rounding: str = "rne"):
    """(xh, xl) = (q(x), q(x - xh)); the float32 difference is exact for finite xh."""
    x = np.ascontiguousarray(x, np.float32)
    xh = q(x, rounding)
    with np.errstate(invalid="ignore", over="ignore"):
        return xh, q(x - xh, rounding)


# ---- layers, geometries, shapes -----------------------------------------------------------------------------------------

LAYERS = LF.layers()
CONV_LAYERS = [i for i, l in enumerate(LAYERS) if not l.deconv]
DECONV_LAYERS = [i for i, l in enumerate(LAYERS) if l.deconv]


def _geometries():
    seen, out = set(), []
    for i in CONV_LAYERS:
        l = LAYERS[i]
        key = (l.cout, l.cin, l.kh, l.kw, l.stride, l.leaky)
        if key not in seen:
            seen.add(key)
            out.append(i)
    return out


GEOMETRIES = _geometries()      # one representative layer index per distinct (cout, cin, kh, kw, stride, leaky)

# output sizes (n, ho, wo): n ho wo = 1, 31, 32, 33, 127, 128, 129, 257 (M around the edges of a wave and of a block of
# 128 pixels), three images of 25 pixels (images change inside a wave), 2 x 3 and 2 x 2
_OUT_SIZES = ((1, 1, 1), (31, 1, 1), (2, 4, 4), (1, 3, 11), (1, 127, 1), (2, 8, 8), (1, 3, 43), (1, 1, 257), (3, 5, 5),
              (1, 2, 3), (1, 2, 2))
# stride 2 (3 x 3, padding 1): ho = ceil(h / 2); the input sizes alternate the parities of h and of w
_S2_IN_SIZES = ((1, 1, 1), (1, 2, 2), (31, 1, 2), (2, 8, 7), (1, 5, 22), (1, 254, 1), (2, 15, 16), (1, 6, 85),
                (1, 2, 513), (3, 9, 10), (3, 10, 9), (1, 3, 6), (1, 4, 5))


def shapes(li: int):
    """The input sizes (n, h, w) of layer li's cases."""
    l = LAYERS[li]
    if l.stride == 2:
        return _S2_IN_SIZES
    out = list(_OUT_SIZES)              # stride 1 with 'same' padding: the output has the input's size
    if l.kh > 3 and l.kw == 1:
        out.append((1, l.kh - 2, 4))    # k x 1: h < k
    if l.kw > 3 and l.kh == 1:
        out.append((1, 4, l.kw - 2))    # 1 x k: w < k
    return tuple(out)


def slice_layout(layer, aligned: bool):
    """(in_off, in_cs, out_off, out_cs, res_off, res_cs): the misaligned slices of the stage tests, or every offset and
    channel stride a multiple of 4 (with Cin a multiple of 4 the bf16 kernels then gather with 128-bit loads)."""
    if aligned:
        return 4, layer.cin + 8, 4, (layer.cout + 8 + 3) // 4 * 4, 4, 8
    return 2, layer.cin + 3, 1, layer.cout + 4, 1, layer.cout + 1


def layouts(layer, mode: str):
    """The slice layouts a case runs with, as (aligned, expect the 128-bit gather)."""
    out = [(False, False)]
    if layer.cin % 4 == 0:
        out.append((True, mode != "f32"))
    return out


# ---- weights and inputs -------------------------------------------------------------------------------------------------

def _draw(rng, family: str, shape, what: str) -> np.ndarray:
    if what == "bias":
        return rng.integers(-16, 17, shape).astype(np.float32)
    if family == "A":
        lim = 8 if what == "x" else 4
        return rng.integers(-lim, lim + 1, shape).astype(np.float32)
    if family == "B":
        return _B_VALUES[rng.integers(0, len(_B_VALUES), shape)]
    if what == "w":
        return rng.integers(-1, 2, shape).astype(np.float32)
    t = rng.integers(0, 4, shape).astype(np.float32)
    sign = (1 - 2 * rng.integers(0, 2, shape)).astype(np.float32)
    return sign * (np.float32(1) + t * np.float32(2.0 ** -8))


@functools.lru_cache(maxsize=None)
def weights(name: str) -> dict:
    """A full weights dict of LF.param_spec() shapes: family A, B or C, or "S" (one-hot at the centre tap, w[n][n] = 1,
    zero bias).  Every layer is drawn from its own stream.  The transposed convs carry integers in [-4, 4]."""
    W = {}
    for i, l in enumerate(LAYERS):
        rng = np.random.default_rng([_SEED[name], i])
        if l.deconv:
            W[l.name + ".weight"] = rng.integers(-4, 5, (l.cout, 1, 4, 4)).astype(np.float32)
            continue
        shape = (l.cout, l.cin, l.kh, l.kw)
        if name == "S":
            w = np.zeros(shape, np.float32)
            n = np.arange(min(l.cout, l.cin))
            w[n, n, l.kh // 2, l.kw // 2] = 1
            W[l.name + ".weight"], W[l.name + ".bias"] = w, np.zeros(l.cout, np.float32)
        else:
            W[l.name + ".weight"] = _draw(rng, name, shape, "w")
            W[l.name + ".bias"] = _draw(rng, name, (l.cout,), "bias")
    return W


def case_input(li: int, shape, family: str):
    """(x [n][h][w][Cin], residual [n][ho][wo][Cout] or None) of a case: x of the family, the residual (flow heads)
    arbitrary normal floats."""
    l = LAYERS[li]
    n, h, w = shape
    rng = np.random.default_rng([_SEED[family], 1000 + li, n, h, w])
    x = _draw(rng, family, (n, h, w, l.cin), "x")
    ho, wo = l.out_size(h, w)
    res = rng.standard_normal((n, ho, wo, l.cout)).astype(np.float32) if l.cout == 2 else None
    return x, res


def embed(core: np.ndarray, off: int, cs: int, seed) -> np.ndarray:
    """core as the channels [off, off + C) of a buffer of cs channels; the others are standard-normal noise."""
    buf = np.random.default_rng(seed).standard_normal(core.shape[:3] + (cs,)).astype(np.float32)
    buf[..., off:off + core.shape[3]] = core
    return buf


# ---- the sums -------------------------------------------------------------------------------------------------------------

def _ints(a: np.ndarray) -> np.ndarray:
    s = a.astype(np.float64) * SCALE
    i = np.rint(s).astype(np.int64)
    assert np.array_equal(i.astype(np.float64), s), "an operand is not a multiple of 2^-9"
    return i


def term_planes(mode: str, x, w, rounding="rne", add_lolo=False, drop_hilo=False):
    """The (x plane, w plane) pairs whose convolutions a mode adds."""
    if mode == "f32":
        return [(x, w)]
    xh, xl = split(x, rounding)
    wh, wl = split(w, rounding)
    if mode == "bf16":
        return [(xh, wh)]
    return [(xh, wh)] + ([] if drop_hilo else [(xh, wl)]) + [(xl, wh)] + ([(xl, wl)] if add_lolo else [])


def _k_index(l, kext: int):
    k = np.arange(kext)
    tap, ci = k // l.cin, k % l.cin
    return tap // l.kw, tap % l.kw, ci


def im2col(x: np.ndarray, l, kext=None, swap_taps=False, right_short=0, bottom_short=0, image_div_bug=False):
    """[M][K] rows of the implicit GEMM, K ordered (ky, kx, ci), zeros outside the image.  kext > K appends the columns
    an unguarded gather would read past K (tap kh kw and on).  The other arguments model wrong gathers: the taps' offsets
    applied to the other axis; the last column or row taken as padding; the image index as m / (ho wo + 1)."""
    n, h, w, _ = x.shape
    ho, wo = l.out_size(h, w)
    hw = ho * wo
    m = np.arange(n * hw)
    b = m // (hw + 1) if image_div_bug else m // hw
    r = m - b * hw
    oy = r // wo
    ox = r - oy * wo
    ky, kx, ci = _k_index(l, l.kh * l.kw * l.cin if kext is None else kext)
    if swap_taps:
        ky, kx = kx, ky
    iy = (oy * l.stride - l.ph)[:, None] + ky[None, :]
    ix = (ox * l.stride - l.pw)[:, None] + kx[None, :]
    ok = (iy >= 0) & (iy < h - bottom_short) & (ix >= 0) & (ix < w - right_short)
    g = x[b[:, None], np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1), ci[None, :]]
    return np.where(ok, g, 0)


def weight_matrix(w: np.ndarray, l, kext=None):
    """[K][Cout] of w [Cout][Cin][kh][kw].  kext > K appends what a read past a row's K finds in a plane [Cout][K]:
    the rows that follow (after the last row, the first)."""
    K = l.kh * l.kw * l.cin
    wm = w.transpose(2, 3, 1, 0).reshape(K, l.cout)
    if kext is None or kext == K:
        return wm
    k, n = np.arange(K, kext)[:, None], np.arange(l.cout)[None, :]
    return np.concatenate([wm, wm[k % K, (n + k // K) % l.cout]])


def conv_sum(l, mode: str, x, w, bias, rounding="rne", add_lolo=False, drop_hilo=False, chunk_tail=False, **gather):
    """sum over the mode's terms + bias, exactly, as int64 in units of 2^-18: [n][ho][wo][Cout].  chunk_tail: the K
    chunk's tail past K read from the buffers instead of being zero."""
    K = l.kh * l.kw * l.cin
    chunk = CONV_BK if mode == "f32" else QCONV_BK
    kext = (K + chunk - 1) // chunk * chunk if chunk_tail else K
    groups = {}
    for xp, wp in term_planes(mode, x, w, rounding, add_lolo, drop_hilo):
        if not xp.any() or not wp.any():
            continue
        g = groups.setdefault(id(xp), [xp, 0])
        g[1] = g[1] + _ints(wp)
    n, h, wd, _ = x.shape
    ho, wo = l.out_size(h, wd)
    s = np.zeros((n * ho * wo, l.cout), np.int64)
    for xp, wi in groups.values():
        s += np.einsum("mk,kn->mn", im2col(_ints(xp), l, kext, **gather), weight_matrix(wi, l, kext))
    s += _ints(bias)[None, :] * SCALE
    return s.reshape(n, ho, wo, l.cout)


def finish(s: np.ndarray, l, res=None, den=None) -> np.ndarray:
    """The float32 output of the exact sum s (units of 2^-18): with den = 1 / u the sum must be a multiple of u below
    2^24 u, and its float32 is exact; without, the nearest float32 (the models of wrong kernels).  Then LeakyReLU and
    the residual, one IEEE operation each, as the kernels' epilogue has them."""
    if den is None:
        y = (s.astype(np.float64) / (SCALE * SCALE)).astype(np.float32)
    else:
        per = SCALE * SCALE // den
        assert not (s % per).any(), "a sum is not a multiple of the unit"
        t = s // per
        assert np.abs(t).max() < LIMIT
        y = t.astype(np.float32) / np.float32(den)
    if l.leaky:
        y = np.where(y > 0, y, y * np.float32(0.1))
    if res is not None:
        y = res.astype(np.float32) + y
    return y.astype(np.float32)


def _granule(i: np.ndarray) -> int:
    """The largest power of two (up to 2^18) that divides every element."""
    g = int(np.bitwise_or.reduce(np.abs(i).ravel(), initial=0)) | (1 << 18)
    return g & -g


def admissible(li: int, mode: str, family: str, x: np.ndarray) -> float:
    """Asserts the premise for layer li's weights of the family and the input x, on the arrays themselves: every term
    x_k w_k of the mode and the bias are multiples of u, and sum|terms| + |b| < 2^24 u for every output.  Returns
    the bound on sum|terms| / u it found: max|x plane| times the largest row sum of |w plane|, over the term pairs."""
    den = unit_den(family, mode)
    l, W = LAYERS[li], weights(family)
    w, bias = W[l.name + ".weight"], W[l.name + ".bias"]
    per = SCALE * SCALE // den
    total = 0
    for xp, wp in term_planes(mode, x, w):
        xi, wi = _ints(xp), _ints(wp)
        if not xi.any() or not wi.any():
            continue
        assert _granule(xi) * _granule(wi) % per == 0, f"{l.name} {family} {mode}: a term is not a multiple of 2^-{den.bit_length() - 1}"
        total += int(np.abs(xi).max()) * int(np.abs(wi).reshape(l.cout, -1).sum(axis=1).max())
    bi = _ints(bias) * SCALE
    assert not (bi % per).any()
    total += int(np.abs(bi).max())
    assert total < LIMIT * per, f"{l.name} {family} {mode}: sum|terms| / u may reach {total / per:.3g} >= 2^24"
    return total / per


@functools.lru_cache(maxsize=None)
def expected(li: int, shape, family: str, mode: str) -> np.ndarray:
    """The one right output [n][ho][wo][Cout] of layer li on case_input(li, shape, family) with weights(family)."""
    l, W = LAYERS[li], weights(family)
    x, res = case_input(li, shape, family)
    admissible(li, mode, family, x)
    y = finish(conv_sum(l, mode, x, W[l.name + ".weight"], W[l.name + ".bias"]), l, res, unit_den(family, mode))
    y.setflags(write=False)
    return y


def first_difference(got: np.ndarray, exp: np.ndarray):
    """None when got and exp [n][h][w][c] are equal in every bit (NaNs: by position); else a message naming the first
    differing (image, y, x, channel) and both values."""
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.float32, (got.shape, exp.shape)
    bad = (got.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(got) & np.isnan(exp))
    if not bad.any():
        return None
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    return (f"{int(bad.sum())} of {bad.size} differ; first at (image, y, x, channel) = {at}: got {got[at]!r} "
            f"(0x{int(got.view(np.uint32)[at]):08x}), expected {exp[at]!r} (0x{int(exp.view(np.uint32)[at]):08x})")


# ---- transposed convolutions --------------------------------------------------------------------------------------------

DECONV_SHAPES = ((2, 1, 1), (2, 1, 4), (2, 3, 1), (2, 7, 9))


def deconv_case(li: int, shape):
    """(x, expected) of ConvTranspose2d(C, C, 4, stride 2, padding 1, groups C) with weights("A")'s integers on integer
    x in [-8, 8]: out[2 iy - 1 + ky][2 ix - 1 + kx] += x[iy][ix] w[ky][kx], in int64."""
    l = LAYERS[li]
    n, h, w = shape
    x = np.random.default_rng([15, li, n, h, w]).integers(-8, 9, (n, h, w, l.cout)).astype(np.float32)
    k = weights("A")[l.name + ".weight"].astype(np.int64)[:, 0]       # [C][4][4]
    xi = x.astype(np.int64)
    out = np.zeros((n, 2 * h + 2, 2 * w + 2, l.cout), np.int64)
    for ky in range(4):
        for kx in range(4):
            out[:, ky:ky + 2 * h:2, kx:kx + 2 * w:2, :] += xi * k[None, None, None, :, ky, kx]
    out = out[:, 1:2 * h + 1, 1:2 * w + 1, :]
    assert np.abs(out).max() < LIMIT
    return x, out.astype(np.float32)


# ---- specials -----------------------------------------------------------------------------------------------------------

# 1 x 1 with Cin 49 and with Cin 9, Cout 1: the scalar gather; 3 x 3, Cin 32, Cout 9: the 128-bit gather on aligned slices
SPECIAL_LAYERS = ("netRegularization.0.netScaleX", "netRegularization.3.netScaleX", "netRegularization.3.netDist.0")
_TINY = np.float32(2.0 ** -126)


def specials() -> np.ndarray:
    """_values() and: infinities; NaNs with their payload only in the low 16 bits, and in the high bits; float32
    subnormals; values that round to the smallest normal and to the largest subnormal bfloat16, and their neighbours."""
    bits = np.array([0x7f800000, 0x7f800001, 0x7f80ffff, 0x7fc00000, 0x7fa00000, 0x7fffffff,
                     0x00000001, 0x00007fff, 0x00008000, 0x00008001, 0x00010000, 0x00018000, 0x00028000, 0x00400000,
                     0x007e8000, 0x007effff, 0x007f0000, 0x007f7fff, 0x007f8000, 0x007f8001, 0x007fffff,
                     0x00800000, 0x00800001, 0x00808000, 0x00810000, 0x00818000], np.uint32)
    extra = np.concatenate([bits, bits | np.uint32(0x80000000)]).view(np.float32)
    return np.concatenate([_values(), extra])


def _is_sub(v: np.ndarray) -> np.ndarray:
    return (v != 0) & (np.abs(v) < _TINY)


def _flush(v: np.ndarray, on: bool) -> np.ndarray:
    return np.where(_is_sub(v), np.copysign(np.float32(0), v), v).astype(np.float32) if on else v


FLUSH_MODELS = tuple((a, b, c) for a in (False, True) for b in (False, True) for c in (False, True))


def special_values(v: np.ndarray, mode: str, flush=(False, False, False)):
    """(value, bad) per special under weight 1: bf16 0 + q(v); bf16x3 (0 + xh) + xl with (xh, xl) = split(v), NaN where
    xh is infinite.  bad: an operand is not finite, so the special times a zero weight is a NaN as well.
    flush = (float32 subnormals read as zero by the conversion, bfloat16 subnormal operands read as zero by the
    matrix instruction, float32 subnormal results written as zero): the restatement has none of the three."""
    f_in, f_op, f_out = flush
    v = _flush(np.ascontiguousarray(v, np.float32), f_in)
    with np.errstate(invalid="ignore", over="ignore"):
        xh = _flush(q(v), f_op)
        val = np.float32(0) + xh
        bad = ~np.isfinite(xh)
        if mode == "bf16x3":
            xl = _flush(q(_flush(v - q(v), f_in)), f_op)
            val = val + xl
            bad |= ~np.isfinite(xl)
        elif mode != "bf16":
            raise ValueError(mode)
    return _flush(val.astype(np.float32), f_out), bad


def special_input(li: int) -> np.ndarray:
    """[1][1][P][Cin], P = Cin * len(specials()): pixel p carries special p // Cin in channel p mod Cin and zeros
    elsewhere, so every special meets every weight of a one-hot row.  One image row: a 3 x 3 window only sees the
    pixel's two neighbours."""
    l = LAYERS[li]
    s = specials()
    x = np.zeros((1, 1, len(s) * l.cin, l.cin), np.float32)
    p = np.arange(x.shape[2])
    x[0, 0, p, p % l.cin] = s[p // l.cin]
    return x


def special_expected(li: int, mode: str, flush=(False, False, False)) -> np.ndarray:
    """[1][1][P][Cout] of weights("S") on special_input(li): channel n of pixel p is the special's value where
    n = p mod Cin and 0 x (the special) summed from +0 elsewhere: +0.0, or NaN when an operand of the special is not
    finite; every channel of a pixel is NaN when a neighbour in its window carries such a special."""
    l = LAYERS[li]
    s = specials()
    val, bad = special_values(s, mode, flush)
    P = len(s) * l.cin
    p = np.arange(P)
    out = np.zeros((P, l.cout), np.float32)
    sel = p % l.cin < l.cout
    out[p[sel], (p % l.cin)[sel]] = val[p[sel] // l.cin]
    own = bad[p // l.cin]
    out[own[:, None] & (np.arange(l.cout)[None, :] != (p % l.cin)[:, None])] = np.nan
    near = np.zeros(P, bool)
    for d in range(1, l.kw // 2 + 1):
        near[d:] |= own[:-d]
        near[:-d] |= own[d:]
    out[near] = np.nan
    return out.reshape(1, 1, P, l.cout)


def special_classes(li: int, mode: str):
    """Per output element [1][1][P][Cout], which kind of subnormal its value rests on (0: none):
    1 q(v) is a subnormal bfloat16; 2 v is a float32 subnormal that rounds to the smallest normal; 3 (bf16x3) v and
    q(v) are normal and the lo part or its float32 source is subnormal."""
    l = LAYERS[li]
    s = specials()
    xh, xl = split(s)
    with np.errstate(invalid="ignore", over="ignore"):
        d = s - xh
    c = np.zeros(len(s), np.int8)
    if mode == "bf16x3":
        c[_is_sub(xl) | _is_sub(d)] = 3
    c[_is_sub(s) & (np.abs(xh) == _TINY)] = 2
    c[_is_sub(xh)] = 1
    P = len(s) * l.cin
    p = np.arange(P)
    out = np.zeros((P, l.cout), np.int8)
    sel = p % l.cin < l.cout
    out[p[sel], (p % l.cin)[sel]] = c[p[sel] // l.cin]
    return out.reshape(1, 1, P, l.cout)
