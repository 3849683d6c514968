"""The hand-built JPEG files of tests/jpegdec_sweep.py on the CPU ("Hand-built scans"): Pillow's
pixels equal the restatement's (tests/jpegdec_ref.py) on every file of the families pinned by Pillow; the parallel
path's restatement (tests/jpegdec_par_ref.py) agrees with the serial one at subsequences of 16 and 128 bytes; each family
covers what it was built for -- code lengths by bit phases, the serial reader's refills by phase and window edge, the
block length the window's margin is sized for, a refill inside an MCU -- as a trace of the file and a model of the
reader's window say; and tests/golden/jpegdec_sweep.npz is what the builder and the restatement make today.  The files
also join the corpora of the two host check programs (test_jpegdec_ref.py, test_jpegdec_par_ref.py).  No GPU."""
import os

import numpy as np
import pytest

from tests import jpegdec_par_ref as PR
from tests import jpegdec_ref as JR
from tests import jpegdec_sweep as SW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = SW.all_cases()
FILES = dict(CASES)
FAMILY = {key: [name for name, _ in CASES if SW.family_of(name) == key] for key in SW.FAMILIES}
REJECTED = {"f_dht_cut_short": "bad_dht"}
NO_DRI = [name for name, b in CASES if name not in REJECTED and JR.parse_header(b.data)["restart_mcus"] == 0]


def _moves(names):
    """The refills that move the window (the first of an interval, at byte 0, fills it)."""
    return [r for name in names for r in SW.refills(FILES[name])[0] if r.next > 0]


def test_every_family_has_its_files():
    counts = {key: len(names) for key, names in FAMILY.items()}
    assert counts == {"a": 3, "b": 17, "c": 2, "d": 6, "e": 2, "f": 8}, counts
    assert len(CASES) == len(FILES) == sum(counts.values())
    for name, built in CASES:
        hd = JR.parse_header(built.data) if name not in REJECTED else None
        assert hd is None or (hd["width"] <= 512 and hd["height"] <= 512), name
        assert len(built.data) < 26000, name


def test_verdicts():
    for name, built in CASES:
        assert JR.verdict(built.data) == REJECTED.get(name, "ok"), name
    assert set(REJECTED) <= set(FAMILY["f"])


def test_pillow_equals_the_restatement_on_every_pinned_file():
    """Families A, B, D, E and the accepted files of F.  Family C is not asked of Pillow: its samples leave the range in
    which libjpeg's C and SIMD IDCT agree."""
    pytest.importorskip("PIL")
    from tests.jpegdec_cases import pillow_pixels
    pinned = [name for name, _ in CASES if SW.family_of(name) not in SW.RESTATEMENT_ONLY and name not in REJECTED]
    assert len(pinned) == len(CASES) - len(FAMILY["c"]) - len(REJECTED) >= 35
    for name in pinned:
        data = FILES[name].data
        want = pillow_pixels(data)
        np.testing.assert_array_equal(JR.decode(data), want, err_msg=name)
        np.testing.assert_array_equal(JR.decode(data, "bgr"), want[:, :, ::-1], err_msg=name)


def test_the_fixture_is_what_the_builder_and_the_restatement_make():
    z = np.load(os.path.join(GOLDEN, "jpegdec_sweep.npz"))
    assert [str(n) for n in z["names"]] == [name for name, _ in CASES]
    for name, built in CASES:
        assert z[name + ".file"].tobytes() == built.data, name
        assert int(z[name + ".reject"]) == JR.R[JR.verdict(built.data)], name
        if name in REJECTED:
            assert name + ".rgb" not in z.files
            continue
        np.testing.assert_array_equal(z[name + ".rgb"], JR.decode(built.data), err_msg=name)
        for sub in SW.SUBS:
            assert (f"{name}.entries{sub}" in z.files) == (name in NO_DRI), name
    assert os.path.getsize(os.path.join(GOLDEN, "jpegdec_sweep.npz")) <= os.path.getsize(os.path.join(GOLDEN, "jpegdec_par_valid.npz"))


@pytest.mark.parametrize("sub", (16, 128))
def test_the_parallel_restatement_agrees(sub):
    """Every file: the verdict is the serial decoder's; without DRI the fixed point's entries are the serial decode's
    states (what the fixture keeps as rows), reached within `subsequences` rounds, and the coefficients are equal."""
    z = np.load(os.path.join(GOLDEN, "jpegdec_sweep.npz"))
    assert len(NO_DRI) >= 25
    for name, built in CASES:
        data = built.data
        assert PR.verdict(data, sub) == REJECTED.get(name, "ok"), name
        if name not in NO_DRI:
            continue
        ps = PR.ParScan(data, sub)
        coef, verdict, entries, rows, rounds = ps.decode()
        assert verdict == "ok" and entries == ps.serial_entries() and 1 <= rounds <= ps.n_subs, name
        np.testing.assert_array_equal(ps.dequantised(coef), JR.decode_coefficients(data)[1], err_msg=name)
        np.testing.assert_array_equal(PR.entry_rows(data, sub), z[f"{name}.entries{sub}"], err_msg=name)
        mine = np.array([[p & 0xFFFFFFFF, p >> 32, b, k, *row] for (p, b, k), row in zip(entries, rows)], np.uint32)
        np.testing.assert_array_equal(mine, z[f"{name}.entries{sub}"], err_msg=name)
    for name in NO_DRI:
        np.testing.assert_array_equal(PR.entry_rows(FILES[name].data, 64), z[f"{name}.entries64"], err_msg=name)


def test_no_block_outruns_the_window():
    """The model itself: with the header's margin no symbol of any file finds the window empty."""
    for name, built in CASES:
        if name not in REJECTED:
            assert SW.refills(built)[1] == 0, name


# ---- family A ----------------------------------------------------------------------------------------------------------
def test_a_every_ladder_code_begins_at_every_bit_phase():
    seen = SW.symbol_phases(FILES["a_ladder_phases"])
    assert {("a", length, ph) for length in range(1, 17) for ph in range(8)} <= seen
    assert {("d", length, ph) for length in range(1, 13) for ph in range(8)} <= seen
    trace = {}
    _, coefs = JR.decode_coefficients(FILES["a_ladder_phases"].data, trace)
    assert trace["dc_sizes"] == set(range(12)) and set(trace["ac_symbols"]) == set(SW.ladder_ac()[1])
    assert np.abs(coefs[:, :, 1:]).max() == 1
    # and the serial reader refills this file with more than 56 bits in hand
    assert max(r.cnt for r in _moves(["a_ladder_phases"])) >= 56


@pytest.mark.parametrize("name", ["a_standard_all_symbols", "a_seam_9_10"])
def test_a_all_symbols_are_used(name):
    """The restatement's trace of the file: the 160 (run, size) symbols, ZRL and EOB, and with the standard tables the
    twelve DC categories; a block that ends at k = 63 without EOB behind three ZRLs and a run of 14, and one whose
    run-15 symbol lands on k = 63.  (Three ZRLs and a run of 15 would land on k = 64: a fault.)"""
    trace = {}
    JR.decode_coefficients(FILES[name].data, trace)
    want = {(r << 4) | s for r in range(16) for s in range(1, 11)} | {0xF0, 0x00}
    assert len(want) == 162 and set(trace["ac_symbols"]) == want
    assert trace["dc_sizes"] == set(range(12))
    blocks = FILES[name].ops[0]
    syms = trace["ac_symbols"]
    joined = ",".join(f"{s:02x}" for s in syms)
    assert "f0,f0,f0,e1" in joined and "f0,f0,e1,f1" in joined
    assert any(len(ops) == 64 and all(op[2] == 1 for op in ops[1:]) for ops in blocks)       # 63 coefficients, no EOB
    lengths = {length for kind, length, _ in SW.symbol_phases(FILES[name]) if kind == "a"}
    if name == "a_seam_9_10":
        assert lengths == {2, 9, 10, 11}
        used = [(length, s) for ops in blocks for kind, length, s in ops if kind == "a"]
        assert sum(length == 9 for length, _ in used) >= 60 and sum(length == 10 for length, _ in used) >= 100
    else:
        assert lengths >= set(range(2, 12)) | {15, 16}              # Annex K's AC code lengths: 2..12, 15 and 16


# ---- family B ----------------------------------------------------------------------------------------------------------
def test_b_the_refills_cover_phases_and_window_edges():
    moves = _moves(FAMILY["b"])
    split = sum(r.tail[-1:] == b"\xff" and r.behind == 0 for r in moves)
    whole, head = sum(r.tail == b"\xff\x00" for r in moves), sum(r.head == b"\xff\x00" for r in moves)
    print(f"family B: {len(moves)} refills that move the window; by cnt & 7: {[sum((r.cnt & 7) == p for r in moves) for p in range(8)]}; "
          f"FF | 00: {split}; FF 00 |: {whole}; | FF 00: {head}; next mod 1024: {len({r.next % 1024 for r in moves})} values")
    assert {r.cnt & 7 for r in moves} == set(range(8))
    assert any(r.tail[-1:] == b"\xff" and r.behind == 0 for r in moves)         # the FF in the window, its 00 outside
    assert any(r.tail == b"\xff\x00" for r in moves)                            # the window ends with a whole pair
    assert any(r.head == b"\xff\x00" for r in moves)                            # and begins with one
    assert len({r.next % 1024 for r in moves}) >= 64


def test_b_interval_lengths():
    nodri = [n for n in FAMILY["b"] if "nodri" in n]
    assert len(nodri) >= 12
    for name in nodri:
        (chunk,) = SW.intervals_of(FILES[name].data)
        assert len(chunk) >= 4.5 * 1024 and len(_moves([name])) >= 4, name
    sizes = {name: [len(c) for c in SW.intervals_of(FILES[name].data)] for name in FAMILY["b"] if "_dri_" in name}
    assert all(1024 - 32 <= n < 1024 for n in sizes["b_dri_05"][:-1])
    assert all(1024 < n < 1024 + SW.BLOCK_MARGIN for n in sizes["b_dri_07"][:-1])
    assert all(n > 2048 for n in sizes["b_dri_11"][:-1])
    assert not _moves(["b_dri_05"]) and _moves(["b_dri_07"]) and _moves(["b_dri_11"])


# ---- family C ----------------------------------------------------------------------------------------------------------
def test_c_blocks_are_as_long_as_the_margin_is_for():
    """63 coefficients of +1023 under the 16-bit code.  The expected pixels are the restatement's alone (Pillow is not
    consulted: the samples wrap in libjpeg's C IDCT and saturate in its SIMD one).  A window margin of 216 + 16 bytes
    would leave symbols of the file without DRI unfed: the file would notice a margin that is too small."""
    for name in FAMILY["c"]:
        trace = {}
        _, coefs = JR.decode_coefficients(FILES[name].data, trace)
        heavy = (np.abs(coefs[:, 0, 1:]) == 1023).all(axis=1)
        assert heavy.sum() >= 8, name
    (chunk,) = SW.intervals_of(FILES["c_margin_nodri"].data)
    bits = 1 + 63 * 26
    assert len(chunk) > 6000 and chunk.count(b"\xff\x00") > 0.35 * len(chunk)
    assert SW.refills(FILES["c_margin_nodri"], 216 + 16)[1] > 0
    assert SW.refills(FILES["c_margin_nodri"])[1] == 0
    heavy_bytes = len(SW.intervals_of(SW.build([(0, [(0, 1023)] * 63)], (1, 1), dc=SW.LADDER_DC, ac=SW.ladder_ac(0x0A)).data)[0])
    assert bits // 8 * 1.6 < heavy_bytes <= SW.BLOCK_MARGIN - 16
    assert JR.parse_header(FILES["c_margin_dri2"].data)["restart_mcus"] == 2
    # the parallel path's longest take: a 16-bit code and 10 value bits that begin at bit phase 7, under FF bytes
    pos, phases = 0, set()
    for ops in FILES["c_margin_nodri"].ops[0]:
        for _, length, s in ops:
            phases |= {pos & 7} if (length, s) == (16, 10) else set()
            pos += length + s
    assert phases == set(range(8))


# ---- family D ----------------------------------------------------------------------------------------------------------
def test_d_reaches_the_largest_categories():
    trace = {}
    hd, coefs = JR.decode_coefficients(FILES["d_dc_walk"].data, trace)
    assert 11 in trace["dc_sizes"] and coefs[:, 0, 0].max() == 2047 and coefs[:, 0, 0].min() == -2047
    assert list(coefs[:4, 0, 0]) == [1023, -1024, 1023, -1024]
    pixels = JR.decode(FILES["d_dc_walk"].data)
    assert pixels.min() == 0 and pixels.max() == 255                              # clamped, both ways
    _, coefs = JR.decode_coefficients(FILES["d_ac10_positions"].data)
    blocks = coefs[:252, 0]
    for k in range(1, 64):
        assert sorted(blocks[4 * (k - 1):4 * k, JR.ZIGZAG[k]]) == [-1023, -512, 512, 1023], k
    assert (np.count_nonzero(blocks, axis=1) == 1).all()
    trace = {}
    _, coefs = JR.decode_coefficients(FILES["d_category_edges"].data, trace)
    values = set(int(v) for v in coefs[:, 0, 1:].ravel())
    for s in range(1, 11):
        assert {1 << (s - 1), -(1 << (s - 1)), (1 << s) - 1, 1 - (1 << s)} <= values, s
    assert trace["dc_sizes"] == set(range(12))
    hd, coefs = JR.decode_coefficients(FILES["d_quant_255"].data)
    assert int(hd["tables"][0][2].min()) == 255 and np.abs(coefs).max() >= 8 * 255


# ---- family E ----------------------------------------------------------------------------------------------------------
def test_e_a_refill_falls_inside_an_mcu():
    for name in FAMILY["e"]:
        hd = JR.parse_header(FILES[name].data)
        assert (hd["h_samp"], hd["v_samp"], hd["components"]) == (2, 2, 3)
        assert len({id(t[2]) for t in hd["tables"]}) == 3 and [int(t[2][0]) for t in hd["tables"]] == [1, 2, 3]
    assert JR.parse_header(FILES["e_420_dri1"].data)["intervals"] == 6
    assert any(r.block % 6 == 4 for r in _moves(["e_420_nodri"]))                # between the fourth luma block and Cb


# ---- family F ----------------------------------------------------------------------------------------------------------
def test_f_the_segments_are_what_the_names_say():
    def markers(data):
        out, at = [], 2
        while True:
            while data[at + 1] == 0xFF:
                at += 1
            out.append(data[at + 1])
            if data[at + 1] == 0xDA:
                return out
            at += 2 + int.from_bytes(data[at + 2:at + 4], "big")

    plain = markers(FILES["f_plain"].data)
    assert plain.count(0xC4) == 4 and plain.count(0xDB) == 2
    assert markers(FILES["f_dht_in_one_segment"].data).count(0xC4) == 1
    assert markers(FILES["f_dqt_in_one_segment"].data).count(0xDB) == 1
    assert markers(FILES["f_unused_tables"].data).count(0xC4) == 6
    assert {0xFE, 0xE5, 0xEF} <= set(markers(FILES["f_com_and_app"].data))
    assert FILES["f_fill_bytes"].data.count(b"\xff\xff\xff\xc4") == 4
    hd = JR.parse_header(FILES["f_dri_past_the_end"].data)
    assert hd["restart_mcus"] == 9 > hd["n_mcus"] and hd["intervals"] == 1
    want = JR.decode(FILES["f_plain"].data)
    for name in FAMILY["f"]:
        if name not in REJECTED:
            np.testing.assert_array_equal(JR.decode(FILES[name].data), want, err_msg=name)


def test_a_block_of_raw_bits_is_the_block_it_spells():
    """The builder's other form of a block: DC category 2 (110 under the ladder) value +3, run 1 size 1 (10) value -1, EOB."""
    kw = dict(dc=SW.LADDER_DC, ac=SW.ladder_ac())
    assert SW.build(["110" "11" "10" "0" "0"], (1, 1), **kw).data == SW.build([(3, [(1, -1)])], (1, 1), **kw).data


# ---- families G, H, I: the pixel stages ----------------------------------------------------------------------------------
PIXEL_CASES = SW.pixel_cases()
PIXEL_FILES = dict(PIXEL_CASES)


def test_the_builder_writes_each_sampling():
    """sampling (1, 1), (2, 1), (2, 2): 3, 4 or 6 blocks an MCU, 0x11, 0x21 or 0x22 in SOF, MCUs of 8 x 8, 16 x 8 or
    16 x 16; and a call without it is the 4:2:0 file it always was."""
    std = SW.standard_tables()
    kw = dict(colour=True, dc=[std["dc_luma"], std["dc_chroma"], std["dc_chroma"]], ac=[std["ac_luma"], std["ac_chroma"], std["ac_chroma"]])
    for sampling, per_mcu, byte in (((1, 1), 3, 0x11), ((2, 1), 4, 0x21), ((2, 2), 6, 0x22)):
        built = SW.build([(1, [])] + [(0, [])] * (2 * 3 * per_mcu - 1), (2, 3), sampling=sampling, **kw)
        hd = JR.parse_header(built.data)
        sof, _ = JR.find_segment(built.data, 0xC0)
        assert built.data[sof + 11] == byte and (hd["h_samp"], hd["v_samp"]) == sampling
        assert (hd["blocks_per_mcu"], hd["width"], hd["height"]) == (per_mcu, 16 * sampling[0], 24 * sampling[1])
        assert JR.verdict(built.data) == "ok"
        with pytest.raises(AssertionError):
            SW.build([(0, [])] * (2 * 3 * per_mcu - 1), (2, 3), sampling=sampling, **kw)
    blocks = [(0, [])] * 6
    assert SW.build(blocks, (1, 1), **kw).data == SW.build(blocks, (1, 1), sampling=(2, 2), **kw).data
    assert SW.build([(0, [])], (1, 1), dc=std["dc_luma"], ac=std["ac_luma"], sampling=(2, 1)).data == SW.build([(0, [])], (1, 1), dc=std["dc_luma"], ac=std["ac_luma"]).data


def test_pixel_families_have_their_files():
    names = [name for name, _ in PIXEL_CASES]
    assert [n[0] for n in names] == list("ghhhhhhi") and len(set(names)) == 8
    assert not set(names) & set(FILES)                                      # jpegdec_sweep.npz keeps what it kept
    for name, built in PIXEL_CASES:
        assert JR.verdict(built.data) == "ok", name


def test_pillow_equals_the_restatement_on_the_pixel_families():
    pytest.importorskip("PIL")
    from tests.jpegdec_cases import pillow_pixels
    z = np.load(os.path.join(GOLDEN, "jpegdec_sweep_pixels.npz"))
    assert [str(n) for n in z["names"]] == [name for name, _ in PIXEL_CASES]
    for name, built in PIXEL_CASES:
        want = pillow_pixels(built.data)
        if name == "i_idct_basis":
            _assert_basis(JR.decode(built.data), want)
        np.testing.assert_array_equal(JR.decode(built.data), want, err_msg=name)
        np.testing.assert_array_equal(JR.decode(built.data, "bgr"), want[:, :, ::-1], err_msg=name)
        assert z[name + ".file"].tobytes() == built.data, name
        np.testing.assert_array_equal(z[name + ".rgb"], want, err_msg=name)


def test_the_restatement_equals_the_pixel_fixture():
    """Pillow's pixels as kept in tests/golden, whatever Pillow is here."""
    z = np.load(os.path.join(GOLDEN, "jpegdec_sweep_pixels.npz"))
    for name, built in PIXEL_CASES:
        assert z[name + ".file"].tobytes() == built.data, name
        if name == "i_idct_basis":
            _assert_basis(JR.decode(built.data), z[name + ".rgb"])
        np.testing.assert_array_equal(JR.decode(built.data), z[name + ".rgb"], err_msg=name)


def _assert_basis(got, want):
    """The IDCT file block by block, so that a difference names the coefficient."""
    for i, (k, v) in enumerate(SW.basis_blocks()):
        by, bx = divmod(i, SW.BASIS_SIZE[0])
        a, b = (p[8 * by:8 * by + 8, 8 * bx:8 * bx + 8, 0] for p in (got, want))
        assert np.array_equal(a, b), f"zigzag position {k} (natural {int(JR.ZIGZAG[k])}), coefficient {v} x quantiser {SW.BASIS_QUANT[k]}:\n{a}\nnot\n{b}"


def test_g_every_channel_clamps_both_ways_and_passes():
    """The lattice's triples through jdcolor.c's arithmetic before the clamp: each of R, G, B falls below 0, rises above
    255 and lies inside for some MCU; and the decoded file is, MCU for MCU, the triple's colour."""
    triples = np.array(SW.lattice(), np.int64)
    assert len(triples) == 968 == SW.LATTICE_SIZE[0] * SW.LATTICE_SIZE[1]
    y, cb, cr = triples[:, 0], triples[:, 1] - 128, triples[:, 2] - 128
    raw = {"r": y + ((91881 * cr + 32768) >> 16), "g": y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), "b": y + ((116130 * cb + 32768) >> 16)}
    for name, v in raw.items():
        assert (v < 0).any() and (v > 255).any() and ((v > 0) & (v < 255)).any(), name
        assert (v == 0).any() or (v == -1).any() or (v == 1).any(), name            # and next to a clamp's edge
    data = PIXEL_FILES["g_lattice_444"].data
    hd, coefs = JR.decode_coefficients(data)
    assert (hd["h_samp"], hd["v_samp"], hd["blocks_per_mcu"], hd["mcus_x"], hd["mcus_y"]) == (1, 1, 3, 44, 22)
    assert not coefs[:, :, 1:].any() and np.array_equal(coefs[:, :, 0] // 8 + 128, triples)
    pixels = JR.decode(data)
    assert pixels.shape == (176, 352, 3)
    want = np.clip(np.stack([raw["r"], raw["g"], raw["b"]], -1), 0, 255).reshape(22, 44, 3)
    np.testing.assert_array_equal(pixels, np.kron(want, np.ones((8, 8, 1), np.int64)))


def test_h_the_blocks_of_an_mcu_differ_and_the_chroma_steps_are_the_largest():
    for name in [n for n in PIXEL_FILES if n[0] == "h"]:
        hd, coefs = JR.decode_coefficients(PIXEL_FILES[name].data)
        luma = hd["h_samp"] * hd["v_samp"]
        assert (hd["mcus_x"], hd["mcus_y"]) == SW.H_SIZE and luma == (2 if "_422_" in name else 4)
        assert hd["width"] % 16 in (1, 15) and hd["height"] % (8 * hd["v_samp"]) == 3
        assert hd["restart_mcus"] == (5 if name.endswith("dri5") else 0)
        samples = coefs[:, :, 0] // 8 + 128
        assert all(len(set(row[:luma])) == luma for row in samples.tolist())          # a swapped block order shows
        cb = samples[:, luma].reshape(SW.H_SIZE[1], SW.H_SIZE[0])
        assert set(cb.ravel().tolist()) == {0, 255} and (np.abs(np.diff(cb, axis=0)) == 255).all() and (np.abs(np.diff(cb, axis=1)) == 255).all()
        np.testing.assert_array_equal(samples[:, luma + 1], 255 - samples[:, luma])
    assert sum(n.endswith("dri5") for n in PIXEL_FILES) == 2


def test_i_every_position_alone_at_both_ends():
    blocks = SW.basis_blocks()
    hd, coefs = JR.decode_coefficients(PIXEL_FILES["i_idct_basis"].data)
    assert len(blocks) == 256 == hd["n_mcus"] and hd["components"] == 1
    assert [int(q) for q in hd["tables"][0][2]] == list(range(1, 65))
    for i, (k, v) in enumerate(blocks):
        assert np.count_nonzero(coefs[i, 0]) == 1 and coefs[i, 0, JR.ZIGZAG[k]] == v * (k + 1), (i, k, v)
    for k in range(64):
        values = sorted(v for kk, v in blocks if kk == k)
        top = values[-1]
        assert values == [-top, -1, 1, top] and top >= 2
        bound = top * (k + 1) / (8 if k == 0 else 4)
        assert bound <= SW.SAMPLE_BUDGET and (top == 1023 or (top + 1) * (k + 1) / 4 > SW.SAMPLE_BUDGET), k
    pixels = JR.decode(PIXEL_FILES["i_idct_basis"].data)
    assert pixels.min() == 0 and pixels.max() == 255                                  # the large amplitudes reach both clamps
