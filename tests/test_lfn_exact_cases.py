"""CPU checks of tests/lfn_exact_cases.py, the inputs and expected outputs of tests/test_gpu_liteflownet_exact.py: the
premise holds for every case the GPU file runs, the expected arrays are torch's convolution in float64 and, bit for bit,
in float32 (which is the premise itself), and the cases tell the right kernel from a list of subtly wrong ones."""
import numpy as np
import pytest

from tests import lfn_exact_cases as X


class _Lazy:
    """A module imported at its first use: collecting this file must not import torch (tests/test_gpu_batch.py
    checks that the C ABI runs without it in the same session)."""

    def __init__(self, name):
        self._name = name

    def __getattr__(self, attr):
        if attr.startswith("_"):
            raise AttributeError(attr)
        import importlib
        return getattr(importlib.import_module(self._name), attr)


torch = _Lazy("torch")
F = _Lazy("torch.nn.functional")
lfn_q_ref = _Lazy("tests.lfn_q_ref")

GEOM_IDS = [X.LAYERS[i].name for i in X.GEOMETRIES]


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_geometries_and_shapes_cover_what_they_should():
    keys = {(l.cout, l.cin, l.kh, l.kw, l.stride, l.leaky) for l in X.LAYERS if not l.deconv}
    got = [(l.cout, l.cin, l.kh, l.kw, l.stride, l.leaky) for l in (X.LAYERS[i] for i in X.GEOMETRIES)]
    assert len(got) == len(set(got)) == len(keys) >= 20 and set(got) == keys
    assert any(k[2:4] == (7, 7) and k[1] == 3 for k in keys) and any(k[0] == 1 and k[2:4] == (1, 1) for k in keys)
    assert any(k[2] > 1 and k[3] == 1 for k in keys) and any(k[2] == 1 and k[3] > 1 for k in keys)
    for li in X.GEOMETRIES:
        l = X.LAYERS[li]
        sh = X.shapes(li)
        ms = [n * l.out_size(h, w)[0] * l.out_size(h, w)[1] for n, h, w in sh]
        assert {1, 31, 32, 33, 127, 128, 129, 257} <= set(ms) and max(ms) == 257, (l.name, ms)
        assert any(n == 3 and np.prod(l.out_size(h, w)) == 25 for n, h, w in sh)
        if l.kh > 1 and l.kw > 1:
            assert any(h < l.kh and w < l.kw and (h, w) != (1, 1) for n, h, w in sh) and (1, 1, 1) in sh
        if l.kh > 1:
            assert any(1 < h < l.kh for n, h, w in sh)
        if l.kw > 1:
            assert any(1 < w < l.kw for n, h, w in sh)
        if l.stride == 2:
            assert {(h % 2, w % 2) for n, h, w in sh} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_weight_sets_load_and_every_layer_has_its_own_stream():
    from transflow_amd import liteflownet as LF
    for name in X.WEIGHT_SETS:
        W = X.weights(name)
        assert LF.check_weights(W).keys() == dict(LF.param_spec()).keys()
    W = X.weights("A")
    same = [l for l in X.LAYERS if not l.deconv and (l.cout, l.cin, l.kh, l.kw) == (128, 128, 3, 3)]
    assert len(same) >= 2
    for a, b in zip(same, same[1:]):
        assert not np.array_equal(W[a.name + ".weight"], W[b.name + ".weight"])
        assert not np.array_equal(W[a.name + ".bias"], W[b.name + ".bias"])


def test_families_are_what_the_table_says():
    x, _ = X.case_input(X.GEOMETRIES[1], (2, 8, 7), "B")
    xh, xl = X.split(x)
    assert set(np.unique(xh)) == {-1.0, 0.0, 1.0} and set(np.unique(xl)) == {-2.0 ** -9, 0.0, 2.0 ** -9}
    x, _ = X.case_input(X.GEOMETRIES[1], (2, 8, 7), "C")
    t = (np.abs(x) - 1) * 256
    assert set(np.unique(t)) == {0.0, 1.0, 2.0, 3.0} and set(np.unique(np.sign(x))) == {-1.0, 1.0}
    qx = np.abs(X.q(x))
    assert (qx[t == 1] == 1).all() and (qx[t == 3] == 1 + 2.0 ** -6).all() and (qx[t == 2] == 1 + 2.0 ** -7).all()
    x, _ = X.case_input(X.GEOMETRIES[1], (2, 8, 7), "A")
    assert _bits_equal(X.q(x), x) and np.abs(x).max() == 8 and (x == np.rint(x)).all()


def test_q_and_split_are_the_restatements():
    v = X.specials()
    got, exp = X.q(v), lfn_q_ref.q(torch.from_numpy(v)).numpy()
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.isnan(got).sum() >= 10
    ok = ~np.isnan(got)
    assert np.array_equal(got[ok].view(np.uint32), exp[ok].view(np.uint32))
    for mine, theirs in zip(X.split(v), lfn_q_ref.split(torch.from_numpy(v))):
        theirs = theirs.numpy()
        assert np.array_equal(np.isnan(mine), np.isnan(theirs))
        assert np.array_equal(mine[~np.isnan(mine)].view(np.uint32), theirs[~np.isnan(mine)].view(np.uint32))
    # the specials hold what they promise
    qs = X.q(v)
    assert (np.abs(qs) == 2.0 ** -126).sum() >= 4 and (np.abs(qs) == 2.0 ** -126 - 2.0 ** -133).sum() >= 4
    assert ((v != 0) & (np.abs(v) < 2.0 ** -126)).sum() >= 20 and np.isinf(v).sum() == 2


def _torch_conv(l, pairs, bias, dtype):
    kw = dict(stride=l.stride, padding=(l.ph, l.pw))
    y = None
    for xp, wp in pairs:
        xt = torch.from_numpy(np.ascontiguousarray(xp)).permute(0, 3, 1, 2).to(dtype)
        c = F.conv2d(xt, torch.from_numpy(wp).to(dtype), torch.from_numpy(bias).to(dtype) if y is None else None, **kw)
        y = c if y is None else y + c
    return y.permute(0, 2, 3, 1).numpy()


def _epilogue(y, l, res):
    if l.leaky:
        y = np.where(y > 0, y, y * np.float32(0.1))
    return (res + y if res is not None else y).astype(np.float32)


@pytest.mark.parametrize("li", X.GEOMETRIES, ids=GEOM_IDS)
def test_expected_is_the_convolution_in_float64_and_in_float32(li):
    """admissible holds for every (geometry, shape, family, mode) of the GPU file (expected asserts it on the case's
    own arrays); the expected array is the float64 convolution rounded once, and the float32 convolution in every bit:
    on these inputs the order of a float32 sum does not matter.  bf16x3 is the three float32 convolutions added."""
    l = X.LAYERS[li]
    for shape in X.shapes(li):
        a_bits = None
        for family in X.FAMILIES:
            W = X.weights(family)
            w, bias = W[l.name + ".weight"], W[l.name + ".bias"]
            x, res = X.case_input(li, shape, family)
            for mode in X.FAMILY_MODES[family]:
                assert X.admissible(li, mode, family, x) < 2 ** 24
                exp = X.expected(li, shape, family, mode)
                pairs = X.term_planes(mode, x, w)
                y64 = _torch_conv(l, pairs, bias, torch.float64)
                assert np.array_equal(y64, np.rint(y64 * 512) / 512) and np.abs(y64).max() * X.unit_den(family, mode) < 2 ** 24
                y32 = _torch_conv(l, pairs, bias, torch.float32)
                what = f"{l.name} {shape} {family} {mode}"
                assert _bits_equal(_epilogue(y64.astype(np.float32), l, res), exp), what
                assert _bits_equal(_epilogue(y32, l, res), exp), what
                if family == "A":
                    a_bits = exp if a_bits is None else a_bits
                    assert _bits_equal(exp, a_bits), what
            if family == "C":
                assert _bits_equal(X.expected(li, shape, "C", "f32"), X.expected(li, shape, "C", "bf16x3"))
    # the ties: bf16 rounds them, the other modes do not
    for s in X.shapes(li):
        if s[0] * s[1] * s[2] >= 31:
            assert not _bits_equal(X.expected(li, s, "C", "bf16"), X.expected(li, s, "C", "f32")), (l.name, s)


def test_admissible_refuses_what_is_not_exact():
    li = X.GEOMETRIES[-1]
    x, _ = X.case_input(li, (1, 3, 11), "B")
    with pytest.raises(ValueError):
        X.admissible(li, "f32", "B", x)
    from transflow_amd import liteflownet as LF
    big = LF.layer_index("netSubpixel.4.netMain.0")
    x, _ = X.case_input(big, (1, 1, 1), "A")
    with pytest.raises(AssertionError):
        X.admissible(big, "f32", "A", x * 1024)          # sum|terms| past 2^24
    with pytest.raises(AssertionError):
        X.admissible(big, "f32", "A", x + np.float32(0.5))   # terms that are odd multiples of a half


# ---- the cases discriminate ---------------------------------------------------------------------------------------------

# wrong kernels, as arguments of X.conv_sum, and the (family, mode) cases that can see each
VARIANTS = {
    "round_half_up": (dict(rounding="half_up"), [("C", "bf16")]),
    "truncation": (dict(rounding="trunc"), [("C", "bf16")]),
    "lo_lo_added": (dict(add_lolo=True), [("B", "bf16x3")]),
    "hi_lo_dropped": (dict(drop_hilo=True), [("B", "bf16x3")]),
    "ky_kx_exchanged": (dict(swap_taps=True), None),
    "padding_right": (dict(right_short=1), None),
    "padding_bottom": (dict(bottom_short=1), None),
    "k_tail_read": (dict(chunk_tail=True), None),
    "last_pixel_dropped": ("drop_last", None),
    "image_index": (dict(image_div_bug=True), None),
}
ALL_CASES = [(f, m) for f in X.FAMILIES for m in X.FAMILY_MODES[f]]


def _applies(name, l):
    K = l.kh * l.kw * l.cin
    if name == "ky_kx_exchanged":
        return l.kh * l.kw > 1
    if name == "k_tail_read":
        return K % X.QCONV_BK != 0
    return True


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("li", X.GEOMETRIES, ids=GEOM_IDS)
def test_cases_discriminate(li, variant):
    """Each wrong kernel changes at least one bit of at least one case of the geometry (the smallest shapes first)."""
    l = X.LAYERS[li]
    if not _applies(variant, l):
        assert variant in ("ky_kx_exchanged", "k_tail_read")
        return
    kw, cases = VARIANTS[variant]
    for shape in sorted(X.shapes(li), key=lambda s: s[0] * s[1] * s[2]):
        for family, mode in cases or ALL_CASES:
            if variant == "k_tail_read" and mode == "f32" and l.kh * l.kw * l.cin % X.CONV_BK == 0:
                continue
            exp = X.expected(li, shape, family, mode)
            if kw == "drop_last":
                wrong = exp.copy()
                wrong.reshape(-1, l.cout)[-1] = 0
            else:
                W = X.weights(family)
                x, res = X.case_input(li, shape, family)
                wrong = X.finish(X.conv_sum(l, mode, x, W[l.name + ".weight"], W[l.name + ".bias"], **kw), l, res)
            if not _bits_equal(wrong, exp):
                return
    pytest.fail(f"no case of {l.name} sees {variant}")


def test_deconv_cases_are_torch_conv_transpose():
    for li in X.DECONV_LAYERS[:2] + X.DECONV_LAYERS[-1:]:
        l = X.LAYERS[li]
        for shape in X.DECONV_SHAPES:
            x, exp = X.deconv_case(li, shape)
            w = torch.from_numpy(X.weights("A")[l.name + ".weight"]).double()
            y = F.conv_transpose2d(torch.from_numpy(x).permute(0, 3, 1, 2).double(), w, None, stride=2, padding=1, groups=l.cout)
            assert np.array_equal(y.permute(0, 2, 3, 1).numpy(), exp.astype(np.float64)), (l.name, shape)


def test_special_cases_are_the_restatement_by_torch():
    """The specials' expected outputs against torch: conv2d of the quantised operands in float32, on a thinned input
    (every 7th pixel run) so that the CPU convolution stays small."""
    from transflow_amd import liteflownet as LF
    for name in X.SPECIAL_LAYERS:
        li = LF.layer_index(name)
        l = X.LAYERS[li]
        W = X.weights("S")
        w = W[l.name + ".weight"]
        assert w.sum() == min(l.cin, l.cout) and not W[l.name + ".bias"].any()
        x = X.special_input(li)
        assert ((x[0, 0] != 0).sum(axis=1) <= 1).all()
        P = x.shape[2]
        lo, hi = P - 40 * l.cin, P                  # the tail: the hand-picked specials
        xs = x[:, :, lo:hi]
        for mode in ("bf16", "bf16x3"):
            base = X.special_expected(li, mode)
            exp = base[:, :, lo:hi]
            with np.errstate(invalid="ignore", over="ignore"):
                y = _torch_conv(l, X.term_planes(mode, xs, w), W[l.name + ".bias"], torch.float32)
            inner = slice(l.kw // 2, hi - lo - l.kw // 2)         # the cut's edges see other neighbours
            assert np.array_equal(np.isnan(y[:, :, inner]), np.isnan(exp[:, :, inner])), (name, mode)
            ok = ~np.isnan(exp[:, :, inner])
            assert np.array_equal(y[:, :, inner][ok].view(np.uint32), exp[:, :, inner][ok].view(np.uint32)), (name, mode)
            assert np.isnan(exp).any() and (~np.isnan(exp)).any()
            cls = X.special_classes(li, mode)
            assert {1, 2} <= set(np.unique(cls)) and ((3 in np.unique(cls)) == (mode == "bf16x3"))
            # the flush models differ from the restatement only where a class says so
            for flush in X.FLUSH_MODELS[1:]:
                alt = X.special_expected(li, mode, flush)
                same = (alt.view(np.uint32) == base.view(np.uint32)) | (np.isnan(alt) & np.isnan(base))
                assert same[cls == 0].all(), (name, mode, flush)
