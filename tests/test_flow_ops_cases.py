"""The edge cases of tests/flow_ops_cases.py on the CPU: the oracle (oracle/flow_ops_ref.py) equals what the
reference returned on every case (tests/golden/flow_ops_edges.npz), every family's inputs tell the right form of its
operation from the named wrong ones, and the plain nearest-neighbour map equals oracle/frames_ref.py's."""
import os

import numpy as np
import pytest

from oracle import flow_ops_ref as F
from oracle import frames_ref
from tests import flow_ops_cases as K
from tests.helpers import GOLDEN

Z = np.load(os.path.join(GOLDEN, "flow_ops_edges.npz"))


def render_compared(case, n_pixels):
    """The pixels of a render case that are compared: all of them, the planted NaN pixels included, if the
    reference wrote one byte value into every planted NaN pixel of every case (then that value is the rule);
    otherwise all but exactly the planted ones."""
    keep = np.ones(n_pixels, bool)
    if case["nans"] and len(nan_bytes()) != 1:
        keep[list(K.nan_pixels(n_pixels))] = False
    return keep


def nan_bytes() -> set:
    seen = set()
    for c in K.render1d_cases() + K.render2d_cases():
        if c["nans"]:
            seen |= set(Z[c["name"]].reshape(-1, 3)[list(K.nan_pixels(c["n"]))].ravel().tolist())
    return seen


def test_the_fixture_holds_one_output_per_case_and_nothing_else():
    names = [c["name"] for family in (K.merge_cases(), K.upscale_cases(), K.render1d_cases(), K.render2d_cases(),
                                      K.convolve_cases()) for c in family]
    assert sorted(names) == sorted(Z.files)
    assert os.path.getsize(os.path.join(GOLDEN, "flow_ops_edges.npz")) <= 1 << 20


@pytest.mark.parametrize("kind", K.MERGE_KINDS)
def test_oracle_merge_equals_the_reference(kind):
    with np.errstate(all="ignore"):
        for c in K.merge_cases():
            if c["kind"] == kind:
                got = F.merge(kind, K.merge_inputs(c["n"], c["count"]))
                assert K.merge_same(kind, got, Z[c["name"]]), c["name"]


def test_oracle_upscale_equals_the_reference():
    with np.errstate(all="ignore"):
        for c in K.upscale_cases():
            got = F.upscale(K.upscale_input(c["h"], c["w"]), c["wf"], c["hf"])
            assert K.same_values(got, Z[c["name"]]), c["name"]


def test_planted_nan_pixels_are_few_and_the_reference_writes_one_value_into_them():
    """What numpy makes of a NaN cast to uint8 is the platform's choice; the recorded reference wrote 0 into every
    byte of every planted pixel, so 0 is what the oracle and the device are held to (render_compared leaves
    nothing out).  Were the fixture ever recorded with mixed values, exactly the planted pixels would be left out."""
    cases = [c for c in K.render1d_cases() + K.render2d_cases() if c["nans"]]
    assert sum(len(K.nan_pixels(c["n"])) for c in cases) == 3 * len(cases) == 18
    assert nan_bytes() == {0}


@pytest.mark.filterwarnings("ignore:invalid value encountered in cast")
def test_oracle_renders_equal_the_reference():
    with np.errstate(all="ignore"):
        for c in K.render1d_cases():
            got = F.render1d(K.render1d_input(c["n"], c["scale"], c["nans"]), c["scale"], c["colors"], c["binary"])
            keep = render_compared(c, c["n"])
            assert got.shape == Z[c["name"]].shape == (1, c["n"], 3)
            assert K.same_bits(got[0, keep], Z[c["name"]][0, keep]), c["name"]
        for c in K.render2d_cases():
            got = F.render2d(K.render2d_input(c["n"], c["scale"], c["nans"]), c["scale"], c["colors"])
            keep = render_compared(c, c["n"])
            assert got.shape == Z[c["name"]].shape == (1, c["n"], 3)
            assert K.same_bits(got[0, keep], Z[c["name"]][0, keep]), c["name"]


def oracle_convolve(flow, kernel):
    return np.stack([F.convolve_same(flow[:, :, 0], kernel), F.convolve_same(flow[:, :, 1], kernel)], axis=-1)


def test_oracle_convolution_equals_the_reference():
    with np.errstate(all="ignore"):
        for c in K.convolve_cases():
            got = oracle_convolve(*K.convolve_inputs(c))
            assert K.same_values(got, Z[c["name"]]), c["name"]


def test_convolution_kernel_types():
    from transflow_amd.flowops import kernel_result_type
    for name, t in K.CONV_DTYPES.items():
        want = np.float64 if name in ("f64", "i64") else np.float32
        assert kernel_result_type(np.zeros((2, 2), t)) == want == K.conv_result_type(np.zeros((2, 2), t))
    for t in (np.complex64, np.complex128, np.longdouble):
        with pytest.raises(NotImplementedError):
            kernel_result_type(np.zeros((2, 2), t))


# ---- the inputs discriminate: against this module's right forms, against the oracle, and the wrong forms are what
# ---- differs (swapping one into the oracle fails the comparisons with the reference above)

def test_merge_cases_discriminate():
    K.assert_merge_discriminates()
    with np.errstate(all="ignore"):
        K.assert_merge_discriminates(F.merge)


def test_upscale_cases_discriminate():
    K.assert_upscale_discriminates()
    with np.errstate(all="ignore"):
        K.assert_upscale_discriminates(F.upscale)


@pytest.mark.filterwarnings("ignore:invalid value encountered in cast")
def test_render_cases_discriminate():
    K.assert_render_discriminates()
    with np.errstate(all="ignore"):
        K.assert_render_discriminates(F.render1d, F.render2d)


def test_convolution_cases_discriminate():
    K.assert_convolve_discriminates()
    with np.errstate(all="ignore"):
        K.assert_convolve_discriminates(oracle_convolve)


def test_grey_cases_discriminate():
    K.assert_grey_discriminates()


def test_every_wrong_form_misses_the_recorded_reference():
    """Each named wrong form, in place of the right one, disagrees with the fixture on at least one case."""
    with np.errstate(all="ignore"):
        for kind, forms in K.MERGE_WRONG.items():
            for form in forms:
                assert any(not K.merge_same(kind, K.merge_form(kind, K.merge_inputs(c["n"], c["count"]), form), Z[c["name"]])
                           for c in K.merge_cases() if c["kind"] == kind), (kind, form)
        for form in ("swapped_scale", "swapped_repeat", "swapped_axes", "truncated"):
            assert any(not K.same_values(K.upscale_form(K.upscale_input(c["h"], c["w"]), c["wf"], c["hf"], form), Z[c["name"]])
                       for c in K.upscale_cases()), form
        for binary, forms in K.R1_WRONG.items():
            for form in forms:
                assert any(not K.same_bits(K.render1d_form(K.render1d_input(c["n"], c["scale"], False), c["scale"], c["colors"],
                                                           binary, form), Z[c["name"]])
                           for c in K.render1d_cases() if c["binary"] == binary and not c["nans"]), form
        for form in K.R2_WRONG:
            assert any(not K.same_bits(K.render2d_form(K.render2d_input(c["n"], c["scale"], False), c["scale"], c["colors"], form),
                                       Z[c["name"]]) for c in K.render2d_cases() if not c["nans"]), form
        for form in ("centre_hi", "cols_first", "fma", "other_acc", "skip_zero_taps"):
            cases = [c for c in K.convolve_cases() if form != "fma" or c["dtype"] in ("f32", "f16", "bool")]
            assert any(not K.same_values(K.convolve_form(*K.convolve_inputs(c), form), Z[c["name"]]) for c in cases), form


def test_right_forms_of_the_case_module_equal_the_reference_too():
    with np.errstate(all="ignore"):
        for c in K.merge_cases():
            assert K.merge_same(c["kind"], K.merge_form(c["kind"], K.merge_inputs(c["n"], c["count"])), Z[c["name"]]), c["name"]
        for c in K.upscale_cases():
            assert K.same_values(K.upscale_form(K.upscale_input(c["h"], c["w"]), c["wf"], c["hf"]), Z[c["name"]]), c["name"]
        for c in K.render1d_cases():
            got = K.render1d_form(K.render1d_input(c["n"], c["scale"], c["nans"]), c["scale"], c["colors"], c["binary"])
            assert K.same_bits(got, Z[c["name"]]), c["name"]
        for c in K.render2d_cases():
            got = K.render2d_form(K.render2d_input(c["n"], c["scale"], c["nans"]), c["scale"], c["colors"])
            assert K.same_bits(got, Z[c["name"]]), c["name"]
        for c in K.convolve_cases():
            assert K.same_values(K.convolve_form(*K.convolve_inputs(c)), Z[c["name"]]), c["name"]


# ---- grey --------------------------------------------------------------------------------------------------------

def test_the_search_finds_the_named_pairs_and_the_suites_old_pairs_do_not_qualify():
    pairs = K.discriminating_pairs()
    assert (6, 34) in pairs and (9, 51) in pairs
    for p in ((2, 98), (3, 147), (6, 94)):
        assert K.differs_from(*p), p
    old = ((1920, 854), (1920, 333), (1920, 3840), (1080, 480), (1080, 77), (1080, 2160), (500, 854), (300, 480),
           (1282, 640), (961, 360))
    assert sum("rational" in K.differs_from(*p) for p in old) == 0
    assert sum("one_div" in K.differs_from(*p) for p in old) == 1
    for s, d in pairs[:6] + ((2, 98), (3, 147), (6, 94), (1920, 333)):       # the vectorised search is the plain loop
        for form in ("right",) + K.NEAREST_WRONG:
            assert K.nearest_map(s, d, form) == K._maps(s, d)[form].tolist(), (s, d, form)


def test_plain_nearest_map_equals_the_frames_oracle():
    for c in K.resize_cases():
        f = K.resize_frame(c)
        exp = K.grey_of(K.resized(f, c["dx"], c["dy"]))
        np.testing.assert_array_equal(frames_ref.bgr_to_grey(f, (c["dx"], c["dy"])), exp, err_msg=c["name"])
    t = K.all_bgr_triples()[::64]
    np.testing.assert_array_equal(frames_ref.bgr_to_grey(t), K.grey_of(t))
