"""LiteFlowNet's convolution kernels (k_lfn_conv, k_lfn_conv_q with both gathers, k_lfn_pack_q, k_lfn_deconv) on inputs
with ONE right answer: tests/lfn_exact_cases.py.  Every term of every sum is a multiple of a unit u and sum|terms| is
below 2^24 u, so any order of float32 additions gives the same bits, computed there in integers; the kernels are compared
with them for equality.  Nothing in this file carries a tolerance.

What a rounding bound cannot see and these cases can: a tie rounded the wrong way on the device, a tap taken one pixel
off at one border, the last K chunk's padding, the last pixel of a block, an image boundary inside a wave, a product the
bf16x3 mode must not add, a layer reading another layer's weights."""
import numpy as np
import pytest

from tests import lfn_exact_cases as X
from transflow_amd import liteflownet as LF
from transflow_amd.liteflownet import LiteFlowNet

pytestmark = pytest.mark.gpu

Q_MODES = ("bf16", "bf16x3")


@pytest.fixture(scope="module")
def nets():
    """name -> a 64 x 64 handle with X.weights(name), made at its first use."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = LiteFlowNet(64, 64, X.weights(name))
        return made[name]

    yield get
    for net in made.values():
        net.close()


def _run(net, li, mode, x, res, aligned, vec):
    """Layer li in `mode` through net.stage_conv, with x and res as channel slices of wider buffers of noise: the
    layer's output channels.  Checks the mode, which gather ran, and that the output's other channels are untouched."""
    from transflow_amd import _lib
    l = X.LAYERS[li]
    off_in, cs_in, off_out, cs_out, off_res, cs_res = X.slice_layout(l, aligned)
    n, h, w, _ = x.shape
    ho, wo = l.out_size(h, w)
    out0 = np.random.default_rng(3).standard_normal((n, ho, wo, cs_out)).astype(np.float32)
    net.set_precision(mode)
    assert net.precision == mode
    _lib.profile(True, "lfn_conv")
    try:
        got = net.stage_conv(li, X.embed(x, off_in, cs_in, 1), out=out0, in_off=off_in, out_off=off_out,
                             residual=None if res is None else X.embed(res, off_res, cs_res, 2), res_off=off_res)
        _lib.check(_lib.load().tf_sync())
        labels = _lib.profile_report()
    finally:
        _lib.profile(False)
    # the launch's label says which gather ran: `<class>_v` with 128-bit loads, `<class>` one channel at a time
    assert len(labels) == 1 and next(iter(labels)).endswith("_v") == vec, (labels, l.name, mode, aligned)
    keep = np.ones(cs_out, bool)
    keep[off_out:off_out + l.cout] = False
    assert np.array_equal(got[..., keep].view(np.uint32), out0[..., keep].view(np.uint32)), f"{l.name} {mode}: wrote outside its slice"
    return np.ascontiguousarray(got[..., off_out:off_out + l.cout])


def _check_case(nets, li, shape, family, mode):
    l = X.LAYERS[li]
    x, res = X.case_input(li, shape, family)
    exp = X.expected(li, shape, family, mode)         # asserts admissible(li, mode, family, x)
    for aligned, vec in X.layouts(l, mode):
        got = _run(nets(family), li, mode, x, res, aligned, vec)
        diff = X.first_difference(got, exp)
        assert diff is None, f"{l.name} {mode} family {family} input {shape}{' aligned' if aligned else ''}: {diff}"


# ---- every geometry, around the edges of waves, blocks and images -----------------------------------------------------

@pytest.mark.parametrize("mode", X.MODES)
@pytest.mark.parametrize("li", X.GEOMETRIES, ids=[X.LAYERS[i].name for i in X.GEOMETRIES])
def test_geometry_sweep(nets, li, mode):
    """Every distinct (Cout, Cin, kh, kw, stride, LeakyReLU) of the network at n ho wo = 1, 31, 32, 33, 127, 128, 129,
    257, three images of 25 pixels, inputs smaller than the kernel and, for stride 2, both parities of h and w; every
    family that is exact in the mode; both slice layouts."""
    for shape in X.shapes(li):
        for family in X.FAMILIES:
            if mode in X.FAMILY_MODES[family]:
                _check_case(nets, li, shape, family, mode)
    # the ties of family C: bf16 rounds them, f32 and bf16x3 do not
    big = max(X.shapes(li), key=lambda s: s[0] * s[1] * s[2])
    assert not np.array_equal(X.expected(li, big, "C", "bf16"), X.expected(li, big, "C", "f32"))


# ---- every layer ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("li", X.CONV_LAYERS, ids=[X.LAYERS[i].name for i in X.CONV_LAYERS])
def test_every_layer_family_a(nets, li):
    """Every convolution layer in the three modes on family A: each layer's weights and bias come from its own stream,
    so a wrong offset into the blob or the packed planes gives other bits; and the three modes agree in every bit."""
    shape = (2, 6, 9) if X.LAYERS[li].stride == 2 else (2, 5, 7)
    for mode in X.MODES:
        _check_case(nets, li, shape, "A", mode)
    assert np.array_equal(X.expected(li, shape, "A", "f32"), X.expected(li, shape, "A", "bf16x3"))


# ---- what the device's rounding does with ties, the top of the range, NaNs, zeros and subnormals -------------------

def _same(got, exp):
    """Equal bits, NaN by position, and a zero of either sign for a zero."""
    return (got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp)) | ((got == 0) & (exp == 0))


@pytest.mark.parametrize("mode", Q_MODES)
@pytest.mark.parametrize("name", X.SPECIAL_LAYERS)
def test_specials_through_one_hot_weights(nets, name, mode):
    """One special value per pixel through weights that are 1 at w[n][n]'s centre tap and 0 elsewhere: the selected
    channel is q(x) (bf16) or xh + xl (bf16x3, NaN where xh is infinite), the others 0 x q(x) summed from +0.  Bits are
    compared, signed zeros included, NaN by position.

    Subnormals are a condition: where the value rests on a subnormal (X.special_classes), the output is the
    restatement's or what one flush behaviour of the hardware makes of it -- the same behaviour for every element of
    the mode, and for the subnormal operands themselves the restatement's value or a zero, the same for all of one
    kind.  The outcome is printed."""
    li = LF.layer_index(name)
    l = X.LAYERS[li]
    x = X.special_input(li)
    base = X.special_expected(li, mode)
    cls = X.special_classes(li, mode)
    kinds = {1: "q(x) a subnormal bfloat16", 2: "float32 subnormal rounding to 2^-126", 3: "subnormal lo part"}
    for aligned, vec in X.layouts(l, mode):
        what = f"{name} {mode}{' aligned' if aligned else ''}"
        got = _run(nets("S"), li, mode, x, None, aligned, vec)
        plain = cls == 0
        diff = X.first_difference(np.where(plain, got, np.float32(0)), np.where(plain, base, np.float32(0)))
        assert diff is None, f"{what} (pixel x carries special x // {l.cin}): {diff}"
        for c in (1, 2, 3):
            m = cls == c
            if not m.any():
                continue
            kept = int((got[m].view(np.uint32) == base[m].view(np.uint32)).sum())
            zero = int((got[m] == 0).sum())
            print(f"{what}: {kinds[c]}: {int(m.sum())} elements, {kept} as the restatement, {zero} zero")
            if c < 3:
                assert kept + zero == int(m.sum()), f"{what}: {kinds[c]}: neither the restatement's value nor a zero"
                assert kept in (0, int(m.sum())), f"{what}: {kinds[c]}: mixed outcomes"
        fits = [f for f in X.FLUSH_MODELS if _same(got, X.special_expected(li, mode, f))[~plain].all()]
        print(f"{what}: flush behaviours (conversion input, bf16 operand, float32 result) that explain every element: {fits}")
        assert fits, f"{what}: no single flush behaviour explains the subnormal elements"


# ---- transposed convolutions ---------------------------------------------------------------------------------------------

DECONVS = [next(i for i in X.DECONV_LAYERS if X.LAYERS[i].cout == c) for c in (2, 49)]


@pytest.mark.parametrize("li", DECONVS, ids=[X.LAYERS[i].name for i in DECONVS])
def test_deconv_integer_sums(nets, li):
    for shape in X.DECONV_SHAPES:
        x, exp = X.deconv_case(li, shape)
        got = nets("A").stage_deconv(li, x)
        diff = X.first_difference(got, exp)
        assert diff is None, f"{X.LAYERS[li].name} input {shape}: {diff}"
