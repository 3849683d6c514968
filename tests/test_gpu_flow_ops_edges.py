"""The flow-array kernels (transflow_amd/csrc/flowops.hip) on the edge cases of tests/flow_ops_cases.py: every case
through the public functions of transflow_amd/flowops.py against what the reference returned on it
(tests/golden/flow_ops_edges.npz) -- equal bits, a NaN for a NaN where the operation computed it, no tolerance --
and the grey conversion against the plain Python statement of the case module.  Then every entry point of the C ABI
once more with its output between two guard zones, the three forms of the grey kernel, the convolution either side
of its 64 KB rule, and the same resize pairs through the two flow methods that restate the nearest-neighbour map."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import flow_ops_cases as K
from tests.helpers import GOLDEN
from tests.test_flow_ops_cases import render_compared

pytestmark = pytest.mark.gpu
Z = np.load(os.path.join(GOLDEN, "flow_ops_edges.npz"))
GUARD = 1 << 16                     # bytes either side of a guarded output: more than a tile row of any case


# ---- the public functions -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", K.MERGE_KINDS)
def test_merge_edges(kind):
    from transflow_amd.flowops import merge_flows
    for c in K.merge_cases():
        if c["kind"] == kind:
            got = merge_flows(kind, K.merge_inputs(c["n"], c["count"]))
            assert K.merge_same(kind, got, Z[c["name"]]), c["name"]


def test_upscale_edges():
    from transflow_amd.flowops import upscale_array
    for c in K.upscale_cases():
        got = upscale_array(K.upscale_input(c["h"], c["w"]), c["wf"], c["hf"])
        assert K.same_values(got, Z[c["name"]]), c["name"]


def test_render1d_edges():
    from transflow_amd.flowops import render1d
    for c in K.render1d_cases():
        got = render1d(K.render1d_input(c["n"], c["scale"], c["nans"]), c["scale"], c["colors"], c["binary"])
        keep = render_compared(c, c["n"])
        assert got.shape == (1, c["n"], 3) and got.dtype == np.uint8
        assert K.same_bits(got[0, keep], Z[c["name"]][0, keep]), c["name"]


def test_render2d_edges():
    from transflow_amd.flowops import render2d
    for c in K.render2d_cases():
        got = render2d(K.render2d_input(c["n"], c["scale"], c["nans"]), c["scale"], c["colors"])
        keep = render_compared(c, c["n"])
        assert got.shape == (1, c["n"], 3) and got.dtype == np.uint8
        assert K.same_bits(got[0, keep], Z[c["name"]][0, keep]), c["name"]


@pytest.mark.parametrize("name", [c["name"] for c in K.convolve_cases()])
def test_convolution_edges(name):
    from transflow_amd.flowops import convolve_post_process
    c = next(c for c in K.convolve_cases() if c["name"] == name)
    got = convolve_post_process(*K.convolve_inputs(c), None)
    assert K.same_values(got, Z[name])


def test_convolution_refuses_complex_and_long_double_kernels():
    from transflow_amd.flowops import convolve_post_process
    flow = K.conv_flow(3, 4)
    for t in (np.complex64, np.complex128, np.longdouble):
        with pytest.raises(NotImplementedError):
            convolve_post_process(flow, np.ones((2, 2), t), None)


def test_grey_of_all_bgr_triples():
    from transflow_amd.flowops import bgr_to_grey
    frame = K.all_bgr_triples()
    np.testing.assert_array_equal(bgr_to_grey(frame), K.grey_of(frame))


@pytest.mark.parametrize("name", [c["name"] for c in K.resize_cases()])
def test_grey_resize_pairs(name):
    from transflow_amd.flowops import bgr_to_grey
    c = next(c for c in K.resize_cases() if c["name"] == name)
    f = K.resize_frame(c)
    np.testing.assert_array_equal(bgr_to_grey(f, (c["dx"], c["dy"])), K.grey_of(K.resized(f, c["dx"], c["dy"])))


# ---- the C ABI, the output between guard zones ------------------------------------------------------------------------

def _between_guards(nbytes: int, call, lead: int = 0):
    """Runs call(pointer) with `pointer` in the middle of a device buffer filled with 0x5A (`lead` more bytes in
    front: an output that is not 4-aligned): (status, the nbytes at the pointer, whether both guard zones are intact)."""
    from transflow_amd.device import DevBuffer
    total = GUARD + lead + nbytes + GUARD
    buf = DevBuffer(total)
    try:
        buf.upload(np.full(total, 0x5A, np.uint8))
        rc = call(C.c_void_p(buf.ptr + GUARD + lead))
        out = buf.download((total,), np.uint8)
    finally:
        buf.close()
    intact = bool((out[:GUARD + lead] == 0x5A).all() and (out[GUARD + lead + nbytes:] == 0x5A).all())
    return rc, out[GUARD + lead:GUARD + lead + nbytes], intact


def _uploaded(*arrays):
    from transflow_amd.device import DevBuffer
    return [DevBuffer.from_array(a) for a in arrays]


def _colors(colors):
    flat = [float(v) for c in colors for v in K.parse_color(c)]
    return (C.c_float * len(flat))(*flat)


def test_merge_writes_nothing_around_its_output():
    from transflow_amd import _lib
    from transflow_amd.flowops import MERGE_KINDS
    lib = _lib.load()
    for kind, n, count in (("sum", 3, 258), ("absmax", 2, 254), ("product", 8, 2)):
        flows = K.merge_inputs(n, count)
        bufs = _uploaded(*flows)
        ptrs = (C.c_void_p * n)(*[b.ptr for b in bufs])
        rc, out, intact = _between_guards(4 * count, lambda p: lib.tf_flow_merge_dev(MERGE_KINDS[kind], n, ptrs, p, count))
        for b in bufs:
            b.close()
        name = f"merge.{kind}.n{n}.c{count}"
        assert rc == _lib.TF_OK and intact, name
        assert K.merge_same(kind, out.view(np.float32).reshape(Z[name].shape), Z[name]), name


def test_upscale_writes_nothing_around_its_output():
    from transflow_amd import _lib
    lib = _lib.load()
    for h, w, wf, hf in ((5, 3, 3, 2), (9, 31, 2, 3), (1, 1, 7, 1)):
        src, = _uploaded(K.upscale_input(h, w))
        rc, out, intact = _between_guards(8 * h * w * wf * hf, lambda p: lib.tf_flow_upscale_dev(C.c_void_p(src.ptr), p, w, h, wf, hf))
        src.close()
        name = f"upscale.{h}x{w}.wf{wf}.hf{hf}"
        assert rc == _lib.TF_OK and intact, name
        assert K.same_values(out.view(np.float32).reshape(Z[name].shape), Z[name]), name


def _convolve_between_guards(c):
    from transflow_amd import _lib
    lib = _lib.load()
    flow, kernel = K.convolve_inputs(c)
    rt = K.conv_result_type(kernel)
    src, kb = _uploaded(flow, np.ascontiguousarray(kernel, dtype=rt))
    rc, out, intact = _between_guards(flow.size * rt.itemsize, lambda p: lib.tf_flow_convolve_dev(
        C.c_void_p(src.ptr), C.c_void_p(kb.ptr), c["kh"], c["kw"], int(rt == np.float64), p, c["w"], c["h"]))
    src.close()
    kb.close()
    return rc, out.view(rt).reshape(flow.shape), intact


@pytest.mark.parametrize("shape,dtype,nbytes,tiled", K.CONV_BOUNDARY)
def test_convolution_either_side_of_the_64_kb_rule(shape, dtype, nbytes, tiled):
    """The largest kernels that take the LDS-tiled kernel (a float64 kernel of 14 x 148 asks for exactly 64 KB of
    dynamic LDS) and the smallest that take the per-pixel one: TF_OK, the recorded bits, nothing written around."""
    from transflow_amd import _lib
    name = "conv.17x65.k%dx%d.%s.lds%d" % (*shape, dtype, nbytes)
    c = next(c for c in K.convolve_cases() if c["name"] == name)
    assert K.conv_tile_bytes(*shape, 8 if dtype == "f64" else 4) == nbytes and (nbytes <= 64 * 1024) == tiled
    rc, out, intact = _convolve_between_guards(c)
    assert rc == _lib.TF_OK and intact
    assert K.same_values(out, Z[name])


def test_convolution_writes_nothing_around_its_output():
    from transflow_amd import _lib
    for name in ("conv.17x65.k3x5.f64", "conv.16x64.k16x1.f32", "conv.1x129.k2x2.f32", "conv.33x1.k3x5.f64", "conv.3x4.k9x9.f32"):
        c = next(c for c in K.convolve_cases() if c["name"] == name)
        rc, out, intact = _convolve_between_guards(c)
        assert rc == _lib.TF_OK and intact, name
        assert K.same_values(out, Z[name]), name


def test_renders_write_nothing_around_their_output():
    """Every pixel count through both render entries: the kernels store three dwords per four pixels, the last
    thread bytes."""
    from transflow_amd import _lib
    lib = _lib.load()
    for c in K.render1d_cases():
        if c["nans"] or c["colors"] != K.R1_COLORS or c["scale"] != 0.5:
            continue
        src, = _uploaded(K.render1d_input(c["n"], c["scale"], False))
        rc, out, intact = _between_guards(3 * c["n"], lambda p: lib.tf_flow_render1d_dev(
            C.c_void_p(src.ptr), p, c["n"], c["scale"], _colors(c["colors"]), int(c["binary"])))
        src.close()
        assert rc == _lib.TF_OK and intact, c["name"]
        assert K.same_bits(out.reshape(1, c["n"], 3), Z[c["name"]]), c["name"]
    for c in K.render2d_cases():
        if c["nans"] or c["colors"] != K.R2_COLORS or c["scale"] != 0.5:
            continue
        src, = _uploaded(K.render2d_input(c["n"], c["scale"], False))
        rc, out, intact = _between_guards(3 * c["n"], lambda p: lib.tf_flow_render2d_dev(
            C.c_void_p(src.ptr), p, c["n"], c["scale"], _colors(c["colors"])))
        src.close()
        assert rc == _lib.TF_OK and intact, c["name"]
        assert K.same_bits(out.reshape(1, c["n"], 3), Z[c["name"]]), c["name"]
    assert {c["n"] for c in K.render1d_cases()} == {c["n"] for c in K.render2d_cases()} == set(K.RENDER_COUNTS)


def _grey_dev(lib, src_ptr, sw, sh, w, h, lead=0):
    return _between_guards(w * h, lambda p: lib.tf_frame_grey_dev(C.c_void_p(src_ptr), sw, sh, p, w, h), lead=lead)


def test_grey_writes_nothing_around_its_output():
    from transflow_amd import _lib
    lib = _lib.load()
    for c in K.resize_cases()[:4]:
        f = K.resize_frame(c)
        src, = _uploaded(f)
        rc, out, intact = _grey_dev(lib, src.ptr, c["sx"], c["sy"], c["dx"], c["dy"])
        src.close()
        assert rc == _lib.TF_OK and intact, c["name"]
        np.testing.assert_array_equal(out.reshape(c["dy"], c["dx"]), K.grey_of(K.resized(f, c["dx"], c["dy"])), err_msg=c["name"])


def test_grey_kernel_forms_agree():
    """The four-pixel kernel (equal sizes, a pixel count that is a multiple of 4, both pointers 4-aligned), the byte
    kernel on one more pixel, on a source one byte into its buffer and on an output one byte off: the same bytes."""
    from transflow_amd import _lib
    lib = _lib.load()
    n = 4096
    i = np.arange(n + 1, dtype=np.uint32) * 4093                                 # spread over all 2^24 triples
    triples = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=-1).astype(np.uint8)
    exp = K.grey_of(triples)
    src, = _uploaded(triples)
    shifted, = _uploaded(np.concatenate([np.zeros(1, np.uint8), triples.ravel()]))
    try:
        rc4, quad, ok4 = _grey_dev(lib, src.ptr, n, 1, n, 1)                     # k_bgr_to_grey4
        rc1, more, ok1 = _grey_dev(lib, src.ptr, n + 1, 1, n + 1, 1)             # one extra pixel: bytes
        rcs, off, oks = _grey_dev(lib, shifted.ptr + 1, n, 1, n, 1)              # source pointer not aligned: bytes
        rco, out1, oko = _grey_dev(lib, src.ptr, n, 1, n, 1, lead=1)             # output pointer not aligned: bytes
        rcr, rows, okr = _grey_dev(lib, src.ptr, 64, 64, 64, 64)                 # the same pixels as a 64 x 64 frame
    finally:
        src.close()
        shifted.close()
    assert (rc4, rc1, rcs, rco, rcr) == (_lib.TF_OK,) * 5
    assert ok4 and ok1 and oks and oko and okr
    np.testing.assert_array_equal(quad, exp[:n])
    np.testing.assert_array_equal(more, exp)
    np.testing.assert_array_equal(off, exp[:n])
    np.testing.assert_array_equal(out1, exp[:n])
    np.testing.assert_array_equal(rows, exp[:n])


# ---- the same map in the flow methods' own ingest kernels ---------------------------------------------------------------

INGEST = [c["name"] for c in K.resize_cases() if c["ingest"]]
_WEIGHTS = []


def _second_frame(f):
    return np.ascontiguousarray(f[::-1, ::-1])


@pytest.mark.parametrize("name", INGEST)
def test_farneback_ingest_resizes_by_the_same_map(name):
    """tf_fb_set_frame_bgr on a discriminating resize pair: the flow equals, bit for bit, the flow from grey frames
    resized on the host by the plain Python map."""
    from transflow_amd.farneback import Farneback
    c = next(c for c in K.resize_cases() if c["name"] == name)
    w, h = c["dx"], c["dy"]
    one = K.resize_frame(c)
    two = _second_frame(one)
    fb, fb2 = Farneback(w, h), Farneback(w, h)
    try:
        fb.set_frame_bgr(0, one)
        fb.set_frame_bgr(1, two)
        fb.calc_slots([0], [1])
        got = fb.get_flow(0)
        exp = fb2.calc(K.grey_of(K.resized(one, w, h)), K.grey_of(K.resized(two, w, h)))
    finally:
        fb.close()
        fb2.close()
    assert K.same_bits(got, exp)
    assert np.abs(exp).max() > 0


@pytest.mark.parametrize("name", INGEST)
def test_liteflownet_ingest_resizes_by_the_same_map(name):
    """LiteFlowNet.set_frame_bgr + stage_prep within the prep stage's 2^-20 of lfn_ref.prep of the frame resized by
    the plain Python map.  The frame is the case module's gentle one (neighbours 2 to 4 levels apart; a pixel from
    the wrong source index is 2^-7 off): prep interpolates bilinearly at float32 sample positions, as torch's
    float32 statement does, and at these sizes a position is up to 2^-16 off, so the 2^-20 holds only where
    neighbours differ by a few levels -- on the seeded noise frame of the grey cases 68 x 147 measured 7.8e-6."""
    import torch
    from tests import lfn_ref
    from transflow_amd.liteflownet import LiteFlowNet
    if not _WEIGHTS:
        _WEIGHTS.append(lfn_ref.synthetic_weights(1, 1.0)[0])
    c = next(c for c in K.resize_cases() if c["name"] == name)
    w, h = c["dx"], c["dy"]
    f = K.gentle_frame(c)
    net = LiteFlowNet(w, h, _WEIGHTS[0])
    try:
        net.set_frame_bgr(0, f)
        got = net.stage_prep(0, 0)
    finally:
        net.close()
    exp = lfn_ref.prep(K.resized(f, w, h), 0, torch.float64)[0].permute(1, 2, 0).numpy()
    assert got.shape == exp.shape
    assert np.abs(got - exp).max() <= 2.0 ** -20
