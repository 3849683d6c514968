"""The fused merge + upscale kernel and the magnitude view (transflow_amd/csrc/flowseam.hip) through the C ABI:
tf_flow_seam_dev against what the reference returned for the merge alone and the upscale alone
(tests/golden/flow_ops_edges.npz) and for the two in a row (tests/golden/seam.npz, and the case module's restatement);
every store path once more between guard zones and at an output that is only 8-byte aligned; every refused argument;
tf_flow_view_magnitude_dev against the reference's magnitude expression and render1d.  Equal bits, a NaN for a NaN
where the operation computed it, no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import flow_ops_cases as K
from tests import seam_cases as S
from tests.helpers import GOLDEN
from tests.test_flow_ops_cases import render_compared

pytestmark = pytest.mark.gpu
Z = np.load(os.path.join(GOLDEN, "flow_ops_edges.npz"))
ZS = np.load(os.path.join(GOLDEN, "seam.npz"))
GUARD = 1 << 16


def _seam(kind, flows, wf=1, hf=1, lead=0):
    """tf_flow_seam_dev of host flows with the output `lead` bytes past a 256-byte boundary, between two guard zones
    filled with 0x5A: (status, the output, whether both zones are intact)."""
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer
    from transflow_amd.flowops import MERGE_KINDS
    h, w, _ = flows[0].shape
    nbytes = 8 * h * hf * w * wf
    total = GUARD + lead + nbytes + GUARD
    bufs = [DevBuffer.from_array(np.ascontiguousarray(f)) for f in flows]
    out = DevBuffer(total)
    try:
        assert out.ptr % 256 == 0
        out.upload(np.full(total, 0x5A, np.uint8))
        ptrs = (C.c_void_p * len(bufs))(*[b.ptr for b in bufs])
        rc = _lib.load().tf_flow_seam_dev(MERGE_KINDS[kind], len(bufs), ptrs, w, h, wf, hf, C.c_void_p(out.ptr + GUARD + lead))
        got = out.download((total,), np.uint8)
    finally:
        for b in bufs + [out]:
            b.close()
    at = GUARD + lead
    intact = bool((got[:at] == 0x5A).all() and (got[at + nbytes:] == 0x5A).all())
    return rc, got[at:at + nbytes].view(np.float32).reshape(h * hf, w * wf, 2), intact


@pytest.mark.parametrize("kind", K.MERGE_KINDS)
def test_merge_alone(kind):
    from transflow_amd import _lib
    for c in K.merge_cases():
        if c["kind"] == kind:
            rc, got, intact = _seam(kind, K.merge_inputs(c["n"], c["count"]))
            assert rc == _lib.TF_OK and intact, c["name"]
            assert K.merge_same(kind, got, Z[c["name"]]), c["name"]


def test_upscale_alone():
    from transflow_amd import _lib
    for c in K.upscale_cases():
        rc, got, intact = _seam("first", [K.upscale_input(c["h"], c["w"])], c["wf"], c["hf"])
        assert rc == _lib.TF_OK and intact, c["name"]
        assert K.same_values(got, Z[c["name"]]), c["name"]


@pytest.mark.parametrize("kind", K.MERGE_KINDS)
def test_fused(kind):
    from transflow_amd import _lib
    seen = 0
    with np.errstate(all="ignore"):
        for c in S.fused_cases():
            if c["kind"] == kind:
                flows = S.fused_inputs(c)
                rc, got, intact = _seam(kind, flows, c["wf"], c["hf"])
                assert rc == _lib.TF_OK and intact, c["name"]
                assert K.same_values(got, S.fused_form(c, flows)), c["name"]
                assert K.same_values(got, ZS[c["name"]]), c["name"]
                seen += 1
    assert seen == (1 if kind == "absmax" else 2) * len(S.FUSED_SHAPES) * len(S.FUSED_FACTORS)


# (kind, n, (h, w), (wf, hf)): even W*wf (16-byte stores when the output is 16-byte aligned, 8-byte ones when it is
# not), odd W*wf with hf > 1 (the two widths on alternate rows, the last lane's single pixel), wf = 1 with even and odd W
# (16-byte loads on all rows / on the rows that start on a boundary), a row of several work-groups
STORE_PATHS = (("sum", 3, (5, 3), (2, 3)), ("maskbin", 2, (5, 3), (3, 2)), ("absmax", 2, (9, 31), (1, 5)),
               ("average", 3, (2, 129), (1, 1)), ("difference", 2, (9, 31), (7, 1)), ("product", 2, (2, 129), (7, 1)),
               ("first", 2, (1, 1), (1, 5)), ("masklin", 3, (2, 129), (2, 1)))


@pytest.mark.parametrize("lead", (0, 8))
def test_every_store_path_between_guards_and_at_an_8_byte_aligned_output(lead):
    from transflow_amd import _lib
    with np.errstate(all="ignore"):
        for kind, n, (h, w), (wf, hf) in STORE_PATHS:
            c = dict(kind=kind, n=n, h=h, w=w, wf=wf, hf=hf)
            flows = S.fused_inputs(c)
            rc, got, intact = _seam(kind, flows, wf, hf, lead=lead)
            assert rc == _lib.TF_OK and intact, (c, lead)
            assert K.same_values(got, S.fused_form(c, flows)), (c, lead)
    assert {(w * wf) % 2 for _, _, (h, w), (wf, hf) in STORE_PATHS} == {0, 1}


def test_inputs_that_are_only_8_byte_aligned():
    """wf = 1 reads pairs as 16 bytes only where every flow's row starts on a 16-byte boundary: flows 8 bytes past one,
    all of them and one of them."""
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer
    from transflow_amd.flowops import MERGE_KINDS
    c = dict(kind="sum", n=2, h=5, w=3, wf=1, hf=2)
    flows = S.fused_inputs(c)
    want = S.fused_form(c, flows)
    for leads in ((8, 8), (0, 8)):
        bufs = [DevBuffer(f.nbytes + 16) for f in flows]
        out = DevBuffer(want.nbytes)
        try:
            for b, f, lead in zip(bufs, flows, leads):
                b.upload(np.concatenate([np.zeros(lead, np.uint8), f.view(np.uint8).ravel(), np.zeros(16 - lead, np.uint8)]))
            ptrs = (C.c_void_p * 2)(*[b.ptr + lead for b, lead in zip(bufs, leads)])
            assert _lib.load().tf_flow_seam_dev(MERGE_KINDS["sum"], 2, ptrs, 3, 5, 1, 2, C.c_void_p(out.ptr)) == _lib.TF_OK
            assert K.same_values(out.download(want.shape, np.float32), want), leads
        finally:
            for b in bufs + [out]:
                b.close()


def test_refused_arguments_write_nothing():
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer
    lib = _lib.load()
    flows = [K.upscale_input(5, 3)] * 3
    bufs = [DevBuffer.from_array(f) for f in flows]
    out = DevBuffer(8 * 15 * 6)
    try:
        out.upload(np.full(8 * 15 * 6, 0x5A, np.uint8))
        ptrs = (C.c_void_p * 9)(*([b.ptr for b in bufs] * 3))
        holed = (C.c_void_p * 3)(bufs[0].ptr, None, bufs[2].ptr)
        o = C.c_void_p(out.ptr)
        big = 1 << 16
        refused = [
            lib.tf_flow_seam_dev(-1, 2, ptrs, 3, 5, 1, 1, o), lib.tf_flow_seam_dev(8, 2, ptrs, 3, 5, 1, 1, o),     # the kind
            lib.tf_flow_seam_dev(1, 0, ptrs, 3, 5, 1, 1, o), lib.tf_flow_seam_dev(1, 9, ptrs, 3, 5, 1, 1, o),      # n
            lib.tf_flow_seam_dev(7, 1, ptrs, 3, 5, 1, 1, o), lib.tf_flow_seam_dev(7, 3, ptrs, 3, 5, 1, 1, o),      # absmax
            lib.tf_flow_seam_dev(1, 2, ptrs, 3, 5, 0, 1, o), lib.tf_flow_seam_dev(1, 2, ptrs, 3, 5, 1, -2, o),     # a factor
            lib.tf_flow_seam_dev(1, 2, ptrs, -3, 5, 1, 1, o),
            lib.tf_flow_seam_dev(1, 2, None, 3, 5, 1, 1, o), lib.tf_flow_seam_dev(1, 2, ptrs, 3, 5, 1, 1, None),   # null
            lib.tf_flow_seam_dev(1, 3, holed, 3, 5, 1, 1, o),
            lib.tf_flow_seam_dev(1, 2, ptrs, 3, big, 1, big, o), lib.tf_flow_seam_dev(1, 2, ptrs, big, 5, big, 1, o),   # beyond int
        ]
        assert refused == [_lib.TF_ERR_ARG] * len(refused)
        assert (out.download((8 * 15 * 6,), np.uint8) == 0x5A).all()
        # an empty flow is a success and launches nothing
        assert lib.tf_flow_seam_dev(1, 2, ptrs, 0, 5, 2, 2, None) == _lib.TF_OK
        assert lib.tf_flow_seam_dev(1, 2, ptrs, 3, 0, 2, 2, o) == _lib.TF_OK
        assert (out.download((8 * 15 * 6,), np.uint8) == 0x5A).all()
        colors = (C.c_float * 6)(0, 0, 0, 255, 255, 255)
        assert lib.tf_flow_view_magnitude_dev(C.c_void_p(bufs[0].ptr), None, 15, 1.0, colors, 0) == _lib.TF_ERR_ARG
        assert lib.tf_flow_view_magnitude_dev(None, o, 15, 1.0, colors, 0) == _lib.TF_ERR_ARG
        assert lib.tf_flow_view_magnitude_dev(C.c_void_p(bufs[0].ptr), o, 15, 1.0, None, 0) == _lib.TF_ERR_ARG
        assert lib.tf_flow_view_magnitude_dev(None, None, 0, 1.0, colors, 0) == _lib.TF_OK
        assert (out.download((8 * 15 * 6,), np.uint8) == 0x5A).all()
    finally:
        for b in bufs + [out]:
            b.close()


def _colors(colors):
    flat = [float(v) for c in colors for v in K.parse_color(c)]
    return (C.c_float * len(flat))(*flat)


@pytest.mark.parametrize("lead", (0, 8))
def test_magnitude_view(lead):
    """Every case with the flow on a 16-byte boundary (16-byte loads) and 8 bytes past one, the image between guards."""
    from transflow_amd import _lib
    from transflow_amd.device import DevBuffer
    lib = _lib.load()
    assert {c["n"] for c in S.magnitude_cases()} == set(K.RENDER_COUNTS)
    for c in S.magnitude_cases():
        flow = S.magnitude_input(c["n"], c["scale"], c["nans"])
        src = DevBuffer(flow.nbytes + 16)
        dst = DevBuffer(2 * GUARD + 3 * c["n"])
        try:
            src.upload(np.concatenate([np.zeros(lead, np.uint8), flow.view(np.uint8).ravel(), np.zeros(16 - lead, np.uint8)]))
            dst.upload(np.full(2 * GUARD + 3 * c["n"], 0x5A, np.uint8))
            rc = lib.tf_flow_view_magnitude_dev(C.c_void_p(src.ptr + lead), C.c_void_p(dst.ptr + GUARD), c["n"], c["scale"],
                                                _colors(c["colors"]), int(c["binary"]))
            got = dst.download((2 * GUARD + 3 * c["n"],), np.uint8)
        finally:
            src.close()
            dst.close()
        assert rc == _lib.TF_OK, c["name"]
        assert (got[:GUARD] == 0x5A).all() and (got[GUARD + 3 * c["n"]:] == 0x5A).all(), c["name"]
        keep = render_compared(c, c["n"])
        assert c["n"] - keep.sum() <= 3
        assert K.same_bits(got[GUARD:GUARD + 3 * c["n"]].reshape(c["n"], 3)[keep], ZS[c["name"]][0, keep]), c["name"]
