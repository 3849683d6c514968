"""The inputs of tests/test_gpu_conv_tail.py can tell a right convolution tail from a wrong one.  CPU only: the cases of
tests/conv_tail_cases.py against the oracle (oracle.flow_ops_ref.post_process_with_kernel), the modelled wrong tails
against the right one."""
import numpy as np

from tests import conv_tail_cases as T
from tests.flow_ops_cases import same_bits


def _backward(c):
    return T.expected(c, T.BACKWARD)


def test_right_form_is_the_oracle():
    for c in T.tail_cases():
        conv = T.expected(c, T.NONE)
        for d in T.DIRECTIONS:
            assert same_bits(T.tail_form(conv, d), T.expected(c, d)), (c["name"], d)


def test_forward_cases_move_and_collide():
    """From the oracle's BACKWARD output (the clipped convolved field): a non-zero rounded vector on between a tenth and
    nine tenths of the pixels, and a target that two sources claim, wherever the image has at least 16 pixels."""
    checked = 0
    for c in T.tail_cases():
        n = c["h"] * c["w"]
        if n < 16:
            continue
        d = T.rounded_steps(_backward(c))
        moving = d != 0
        share = moving.mean()
        assert 0.1 <= share <= 0.9, (c["name"], share)
        p = np.arange(n)
        targets = np.clip(p[moving] + d[moving], 0, n - 1)
        assert len(np.unique(targets)) < len(targets), c["name"]
        checked += 1
    assert checked == sum(1 for c in T.tail_cases() if (c["h"], c["w"]) != (1, 1))     # only the 1 x 1 image is too small


def test_wrong_tails_change_bits():
    changed = {"clip_f32": 0, "round_first": 0, "first_write_wins": 0, "fma": 0}
    for c in T.tail_cases():
        if c["specials"]:
            continue
        conv = T.expected(c, T.NONE)
        if conv.dtype == np.float64:
            for d in (T.BACKWARD, T.FORWARD):
                changed["clip_f32"] += not same_bits(T.tail_form(conv, d, "clip_f32"), T.expected(c, d))
        changed["round_first"] += not same_bits(T.tail_form(conv, T.BACKWARD, "round_first"), T.expected(c, T.BACKWARD))
        changed["first_write_wins"] += not same_bits(T.tail_form(conv, T.FORWARD, "first_write_wins"), T.expected(c, T.FORWARD))
        if conv.dtype == np.float32 and c["kh"] * c["kw"] > 1:
            flow, kernel = T.tail_inputs(c)
            fused = T.fma_conv(flow, kernel)
            changed["fma"] += any(not same_bits(T.tail_form(fused, d), T.expected(c, d)) for d in T.DIRECTIONS)
    for form, n in changed.items():
        assert n > 0, form


def test_cases_cover_the_issue():
    names = {c["name"] for c in T.tail_cases()}
    assert {"tail.17x65.k14x148.f64.lds65536", "tail.17x65.k21x104.f64.lds65568"} <= names
    for (h, w) in T.THIN_IMAGES:
        for (kh, kw) in T.THIN_KERNELS:
            assert f"tail.{h}x{w}.k{kh}x{kw}.f64.thin" in names and f"tail.{h}x{w}.k{kh}x{kw}.f32.thin" in names
    for c in T.tail_cases():
        if c["specials"]:
            flow, kernel = T.tail_inputs(c)
            taps = np.asarray(kernel).ravel()
            assert np.isinf(flow).any() and np.isnan(flow).any()
            assert (np.signbit(taps) & (taps == 0)).any() and (~np.signbit(taps) & (taps == 0)).any()
            out = T.expected(c, T.BACKWARD)
            assert np.isnan(out).any() and not np.isnan(out).all()


def test_narrowing_values_discriminate():
    v = T.NARROW_VALUES
    with np.errstate(invalid="ignore"):
        right, cast_first = T.narrow_form(v, 0), T.narrow_form(v, 0, "cast_first")
        floor = T.narrow_form(v, 1)
    ok = ~np.isnan(v)
    assert (right[ok] != cast_first[ok]).any()                 # 1.4999999999 is 1.5 as a float32
    assert (right[ok] != floor[ok]).any()
    assert np.signbit(right[v == -0.5]).all() and (right[v == -0.5] == 0).all()      # -0.5 -> -0.0
    assert right[v == 2.5][0] == 2 and right[v == 1.5][0] == 2                          # ties to even
    for count in T.NARROW_COUNTS:
        a = T.narrow_input(count)
        assert len(a) == count
    assert np.isnan(T.narrow_input(257)).any() and np.signbit(T.narrow_input(257)[np.isnan(T.narrow_input(257))]).any()
