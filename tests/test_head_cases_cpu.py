"""CPU: the references and case generators of tests/head_cases.py are what they say they are.

  * finalize_ref reproduces the golden tile loops (G3), fold ensembles (G3b) and argmax fixture (G6) bit for bit, and agrees with the
    oracle's finalize_logits / ensemble_folds / argmax_labels on its own inputs;
  * the three activation layouts round-trip and put a channel where the kernels' index expressions read it;
  * every head case reaches the kernel form it is named for under launch_head's dispatch, every finalize case the form it states under
    boa_finalize_labels_planes' predicate, and the option cases cover every pair of option values;
  * the large-magnitude case is what it is meant to be: finite and large without the Gaussian, overflowing to inf with it.
"""
import itertools
import os

import numpy as np
import pytest

from conftest import GOLDEN

import head_cases as hc
from oracle import labels as olab
from oracle import sliding_window as osw


def _npz(name):
    return np.load(os.path.join(GOLDEN, name))


# ---- finalize_ref against the golden vectors -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_finalize_ref_reproduces_g3(case):
    z = _npz("g3_sliding_window.npz")
    tiles, x = z[f"{case}_tiles"], z[f"{case}_x"]
    patch, step = [int(v) for v in z[f"{case}_patch"]], float(z[f"{case}_step"])
    V = list(x.shape[1:])
    xp, revert = osw.pad_nd_image(x, patch)
    PV = xp.shape[1:]
    below = [s.start for s in revert[1:]]
    origins = osw.get_sliding_window_slicers(PV, patch, step)
    assert len(origins) == len(tiles)
    g = osw.compute_gaussian(tuple(patch), 1. / 8, 10) if case != "e" else None
    acc, n = np.zeros((tiles.shape[1], *PV), np.float16), np.zeros(PV, np.float16)
    for t, o in zip(tiles, origins):
        hc.accumulate_tile(acc, n, t.astype(np.float32), g, o)
    crop = (below, V) if list(PV) != V else None
    new_acc, fold, lab, inf = hc.finalize_ref(acc.view(np.uint16), n.view(np.uint16), labels_in=np.zeros(V, np.uint8), crop=crop)
    assert inf == 0 and fold is None
    np.testing.assert_array_equal(new_acc[(slice(None), *revert[1:])], z[f"{case}_logits_bits"])
    if f"{case}_seg" in z.files:
        np.testing.assert_array_equal(lab, z[f"{case}_seg"])
    # the un-cropped planes, in two plane ranges and without writing the logits back: same labels, accumulators untouched
    k = PV[0] // 2
    lab2 = np.full(V, 77, np.uint8)
    for planes in ((0, k), (k, PV[0])):
        a2, _, lab2, _ = hc.finalize_ref(acc.view(np.uint16), n.view(np.uint16), write_logits=0, labels_in=lab2, crop=crop, planes=planes)
        np.testing.assert_array_equal(a2, acc.view(np.uint16))
    np.testing.assert_array_equal(lab2, lab)


def test_finalize_ref_reproduces_g3b_folds():
    z = _npz("g3b_folds.npz")
    folds = z["fold_logits_bits"]
    nf, V = folds.shape[0], folds.shape[2:]
    one = np.full(V, 0x3C00, np.uint16)
    fsum, lab = np.zeros(folds.shape[1:], np.uint16), None
    for f in range(nf):
        last = f == nf - 1
        _, fsum, lab, inf = hc.finalize_ref(folds[f], one, fold_bits=fsum, fold_mode=0 if f == 0 else 1, n_folds_final=nf if last else 0,
                                            write_logits=0, labels_in=np.zeros(V, np.uint8))
        assert inf == 0 and (lab is not None) == last
    np.testing.assert_array_equal(fsum, z["ensemble_bits"])
    np.testing.assert_array_equal(fsum, osw.ensemble_folds([f.view(np.float16) for f in folds]).view(np.uint16))
    np.testing.assert_array_equal(lab, olab.argmax_labels(z["ensemble_bits"].view(np.float16)))


def test_finalize_ref_reproduces_g6_argmax():
    z = _npz("g6_argmax.npz")
    bits = z["logits_bits"]
    V = bits.shape[1:]
    acc, _, lab, inf = hc.finalize_ref(bits, np.full(V, 0x3C00, np.uint16), write_logits=1, labels_in=np.zeros(V, np.uint8))
    assert inf == 1                      # the fixture holds +inf logits
    np.testing.assert_array_equal(lab, z["seg"])
    np.testing.assert_array_equal(hc.canon_nan(acc), hc.canon_nan(bits))     # x / 1 == x


def test_finalize_ref_equals_the_oracle_statements():
    """On finite inputs finalize_ref is finalize_logits, ensemble_folds and argmax_labels, statement for statement; lut, merge and
    crop are what their names say."""
    rng = np.random.default_rng(0)
    V, C = (4, 3, 6), 5
    folds = [(rng.standard_normal((C, *V)) * 3).astype(np.float16) for _ in range(3)]
    n = rng.uniform(0.5, 9, V).astype(np.float16)
    want = [osw.finalize_logits(f, n) for f in folds]
    fsum = np.zeros((C, *V), np.uint16)
    lut = ((np.arange(256) * 5 + 1) % 256).astype(np.uint8)
    before = rng.integers(100, 200, (2, 2, 3)).astype(np.uint8)
    crop = ((1, 1, 2), (2, 2, 3))
    for f in range(3):
        acc, fsum, lab, inf = hc.finalize_ref(folds[f].view(np.uint16), n.view(np.uint16), fold_bits=fsum, fold_mode=min(f, 1),
                                              n_folds_final=3 if f == 2 else 0, lut=lut, merge=1, labels_in=before, crop=crop)
        np.testing.assert_array_equal(acc, want[f].view(np.uint16))
        assert inf == 0
    ens = osw.ensemble_folds(want)
    np.testing.assert_array_equal(fsum, ens.view(np.uint16))
    idx = olab.argmax_labels(ens)[1:3, 1:3, 2:5]
    assert (idx == 0).any() and (idx != 0).any()
    np.testing.assert_array_equal(lab, np.where(idx != 0, lut[idx], before))


def test_finalize_ref_zero_weights_report_instead_of_raising():
    acc = np.array([[0x0000, 0x3C00, 0xBC00, 0x0001], [0x3C00, 0x0000, 0x3C00, 0x0001]], np.uint16).reshape(2, 1, 1, 4)
    n = np.array([0, 0, 0, 0x0001], np.uint16).reshape(1, 1, 4)            # 0 / 0, x / 0, -x / 0, and a subnormal weight
    out, _, lab, inf = hc.finalize_ref(acc, n, labels_in=np.zeros((1, 1, 4), np.uint8))
    assert inf == 1
    f = out.view(np.float16)
    assert np.isnan(f[0, 0, 0, 0]) and np.isposinf(f[1, 0, 0, 0]) and np.isposinf(f[0, 0, 0, 1]) and np.isnan(f[1, 0, 0, 1])
    assert np.isneginf(f[0, 0, 0, 2]) and f[0, 0, 0, 3] == 1 and f[1, 0, 0, 3] == 1
    np.testing.assert_array_equal(lab.reshape(-1), [0, 1, 1, 0])          # the first NaN wins; +inf is a maximum; a tie goes to the first


# ---- layouts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F0", [8, 32, 64])
def test_layouts_round_trip_and_index_as_the_kernels_do(F0):
    rng = np.random.default_rng(F0)
    P = (3, 4, 5)
    pv = 60
    act = rng.standard_normal((*P, F0)).astype(np.float32)
    flat = act.reshape(pv, F0)
    for stride in (pv, pv + 7):
        o = hc.octet32(act, stride)
        np.testing.assert_array_equal(hc.unplanes(o, P), act)
        of = o.reshape(-1)
        for k, i in itertools.product((0, 7, F0 - 1), (0, 17, pv - 1)):      # k_head_f32 / k_head_x3: ((k >> 3) * stride + i) * 8 + (k & 7)
            assert of[((k >> 3) * stride + i) * 8 + (k & 7)] == flat[i, k]
    if F0 % 16 == 0:
        a16 = act.astype(np.float16)
        p = hc.planar16(a16)
        np.testing.assert_array_equal(hc.unplanes(p, P), a16)
        pf = p.reshape(-1)
        for v, j, i in itertools.product(range(F0 // 8), (0, 7), (0, 17, pv - 1)):   # k_head: ((v >> 1) * stride + i) * 16 + 8 * (v & 1) + j
            assert pf[((v >> 1) * pv + i) * 16 + 8 * (v & 1) + j] == a16.reshape(pv, F0)[i, 8 * v + j]
    if F0 == 32:   # the layout tests/test_gpu_head.py feeds the MFMA head
        a16 = act.astype(np.float16)
        want = np.ascontiguousarray(a16.reshape(*P, 2, 16).transpose(3, 0, 1, 2, 4))
        np.testing.assert_array_equal(hc.planar16(a16).reshape(want.shape), want)
    np.testing.assert_array_equal(hc.channels_last(act).reshape(-1)[17 * F0 + 3], flat[17, 3])


def test_head64_is_the_layer_reference_on_the_normalised_activation():
    rng = np.random.default_rng(1)
    act = rng.standard_normal((2, 3, 4, 32)).astype(np.float16)
    ss = np.stack([rng.uniform(0.5, 1.5, 32), rng.normal(0, 0.3, 32)], 1).astype(np.float32)
    w, b = rng.standard_normal((5, 32)).astype(np.float32), rng.standard_normal(5).astype(np.float32)
    L, A = hc.head64(act, ss, w, b)
    assert L.dtype == np.float64 and L.shape == (5, 2, 3, 4) and (A >= np.abs(L)).all()
    x = act[1, 2, 3].astype(np.float64) * ss[:, 0] + ss[:, 1]
    y = np.where(x > 0, x, x * float(np.float32(0.01)))
    assert abs(L[2, 1, 2, 3] - (w[2].astype(np.float64) @ y + b[2])) <= 1e-13 * A[2, 1, 2, 3]
    assert abs(A[2, 1, 2, 3] - (np.abs(w[2]).astype(np.float64) @ np.abs(y) + abs(b[2]))) <= 1e-13 * A[2, 1, 2, 3]


# ---- every case reaches the form it is named for -----------------------------------------------------------------------------------
def _fp16_expectation(c):
    """the forms a case NAME promises, written out here independently of head_cases._fp16_case"""
    if c.name.startswith("pair"):
        return ["k_head<32,2>"] * len(c.starts), "k_head<32,2>"
    if c.name.startswith("single") and c.name.endswith("odd-start"):      # the far-corner tile starts at an even z again
        return ["k_head<32,1>"] * (len(c.starts) - 1) + ["k_head<32,2>"], "k_head<32,2>"
    if c.name.startswith("single") and c.name.endswith("odd-PV"):
        return ["k_head<32,1>"] * len(c.starts), "k_head<32,2>"
    if c.name.startswith("single"):
        return ["k_head<32,1>"] * len(c.starts), "k_head<32,1>"
    if c.name.startswith("f64"):
        return ["k_head<64,1>"] * len(c.starts), "k_head<64,1>"
    assert c.name.startswith("mfma-logits-accumulate")
    return ["k_head_mfma<logits>+k_accumulate_tile"] * len(c.starts), "k_head_mfma<logits>"


def test_fp16_cases_reach_their_forms():
    cases = hc.fp16_cases()
    seen = set()
    for c in cases:
        forms, lform = _fp16_expectation(c)
        # the accumulators sit GUARD elements into a 256-byte aligned allocation: every pointer stays 16-byte aligned
        assert (2 * hc.GUARD) % 16 == 0
        got = [hc.head_form(c.F0, c.P, c.C, False, c.PV, s) for s in c.starts]
        assert got == forms == list(c.forms), (c.name, got)
        assert hc.head_form(c.F0, c.P, c.C, True) == lform == c.logits_form, c.name
        assert len(c.starts) >= 3 and c.starts[-1] == c.far
        for s in c.starts:
            assert all(0 <= a and a + p <= v for a, p, v in zip(s, c.P, c.PV))
        boxes = [tuple(slice(a, a + p) for a, p in zip(s, c.P)) for s in c.starts]
        cover = np.zeros(c.PV, int)
        for bx in boxes:
            cover[bx] += 1
        assert cover.max() >= 2                                            # the tiles overlap
        seen.update(got)
    assert seen == {"k_head<32,2>", "k_head<32,1>", "k_head<64,1>", "k_head_mfma<logits>+k_accumulate_tile"}
    by = {c.name: c for c in cases}
    # the issue's table
    assert {(c.C, c.P) for c in cases if c.name.startswith("pair") and c.scale == 1} == set(itertools.product((32, 118), ((3, 5, 32), (2, 3, 6))))
    assert {(c.C, c.P) for c in cases if c.name.startswith("single")} == set(itertools.product((5, 33), ((3, 5, 7), (2, 3, 6))))
    assert {(c.C, c.P) for c in cases if c.name.startswith("f64") and c.C < 255} == set(itertools.product((1, 7, 40), ((3, 4, 32), (2, 3, 5))))
    assert all(s[2] % 2 == 1 for s in by["single-C5-P2x3x6-odd-start"].starts[:-1]) and by["single-C5-P2x3x6-odd-start"].PV[2] % 2 == 0
    assert by["single-C33-P2x3x6-odd-PV"].PV[2] % 2 == 1
    m = by["mfma-logits-accumulate-C31"]
    assert (m.F0, m.C, m.P, m.PV[2], m.starts[0][2]) == (32, 31, (2, 2, 32), 70, 3)
    for c in cases:                                                        # 8-aligned and unaligned origins for k_head<64,1>
        if c.name.startswith("f64"):
            assert {s[2] % 8 == 0 for s in c.starts} == {True, False} or c.P[2] != 32
    # (3, 5, 32): the shape alone would go to the matrix cores -- the class count is what keeps it off them
    assert hc.head_form(32, (3, 5, 32), 31, False, (5, 8, 40), (0, 0, 0)) == "k_head_mfma<acc>"
    assert hc.head_form(32, (3, 5, 32), 32, False, (5, 8, 40), (0, 0, 0)) == "k_head<32,2>"
    # and the LDS case is above the default limit, everything else below
    assert hc.head_lds_bytes(64, 251) > 64 * 1024 >= hc.head_lds_bytes(64, 250)
    assert hc.head_lds_bytes(by["f64-C255-lds"].F0, by["f64-C255-lds"].C) == 66812
    assert all(hc.head_lds_bytes(c.F0, c.C) <= 64 * 1024 for c in cases if c.name != "f64-C255-lds")


def test_head_form_alignment_branches():
    """the pointer conditions of launch_head's dispatch (the GPU cases keep every pointer aligned; the predicate still has to say what
    a misaligned one would do)"""
    P, PV, s = (2, 2, 32), (4, 4, 64), (0, 0, 8)
    assert hc.head_form(32, P, 5, False, PV, s) == "k_head_mfma<acc>"
    assert hc.head_form(32, P, 5, False, PV, s, acc_align=8) == "k_head_mfma<logits>+k_accumulate_tile"
    assert hc.head_form(32, P, 5, False, PV, s, nacc_align=2) == "k_head_mfma<logits>+k_accumulate_tile"
    assert hc.head_form(32, P, 5, False, PV, s, gauss_align=4) == "k_head_mfma<logits>+k_accumulate_tile"
    assert hc.head_form(32, P, 5, False, PV, s, act_align=8) == "k_head<32,2>"
    assert hc.head_form(32, P, 5, False, PV, s, act_align=8, acc_align=2) == "k_head<32,1>"
    assert hc.head_form(32, P, 5, True, logits_align=8) == "k_head<32,2>"
    assert hc.head_form(32, P, 5, True) == "k_head_mfma<logits>"
    assert hc.head_form(64, P, 5, True) == "k_head<64,1>"


def test_f32_cases_are_the_issues_set():
    x3 = hc.x3_cases()
    assert {(c.C, c.pv) for c in x3} == set(itertools.product((1, 4, 5, 31, 32), (96, 100, 315, 129, 256)))
    for c in x3:
        assert c.F0 == 32 and c.kind == "x3" and c.starts[-1] == c.far
        assert {s[2] % 2 for s in c.starts} == {0, 1}                      # aligned and odd starts
    pvs = {c.pv for c in x3}
    assert any(pv % 32 == 0 and pv % 128 for pv in pvs)                     # whole waves, a partial block
    assert any(pv % 32 for pv in pvs)                                      # a partial wave
    assert any(pv % 128 == 1 for pv in pvs)                                # three waves of the last block without a valid lane
    assert {c.pad for c in x3} == {0, 5}                                   # plane stride == and != the tile's voxel count
    f32 = hc.f32_cases()
    assert {(c.F0, c.kind, c.C, c.pv) for c in f32} == set(itertools.product((8, 32, 64), ("f32cl", "f32oct"), (1, 33, 118), (315, 512)))
    assert all(c.pad == 0 for c in f32 if c.kind == "f32cl") and {c.pad for c in f32 if c.kind == "f32oct"} == {0, 3}
    for c in x3 + f32:
        w, b, tiles = hc.head_inputs(c)
        packed, stride = hc.pack_act(c, tiles[0][0])
        assert packed.dtype == np.float32 and (stride == 0) == (c.kind == "f32cl")
        assert packed.size == (c.pv + c.pad) * c.F0


def test_large_magnitude_case_overflows_only_with_the_gaussian():
    """`pair-large-C32`: logits of 1e3 to above 1e4.  Three tiles on zero accumulators: finite and above a quarter of the fp16 maximum without the
    Gaussian, +-inf somewhere (not everywhere) with it -- the reference's own fp16 `+=` overflow."""
    c = next(c for c in hc.fp16_cases() if c.name == "pair-large-C32")
    w, b, tiles = hc.head_inputs(c)
    res = {}
    for name, g in (("plain", None), ("gauss", hc.gaussian(c.P))):
        acc, n = np.zeros((c.C, *c.PV), np.float16), np.zeros(c.PV, np.float16)
        for (act, ss), s in zip(tiles, c.starts):
            L = hc.head64(act, ss, w, b)[0].astype(np.float32)
            hc.accumulate_tile(acc, n, L, g, s)
        res[name] = acc.astype(np.float32)
    big = np.abs(hc.head64(*tiles[0], w, b)[0])
    assert 1e3 < np.median(big) < 1e4 < big.max() < 65504
    assert np.isfinite(res["plain"]).all() and np.abs(res["plain"]).max() > 16384
    assert np.isinf(res["gauss"]).any() and np.isfinite(res["gauss"]).mean() > 0.5


# ---- finalize cases ------------------------------------------------------------------------------------------------------------------
def test_finalize_cases_reach_their_forms_and_cover_the_option_pairs():
    cases = hc.finalize_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        nv = int(np.prod(c.V))
        assert hc.finalize_form(c.V) == c.vec == (8 if nv % 8 == 0 else 1), c.name
        acc, n, fold, lut, labels = hc.finalize_inputs(c)
        assert acc.shape == (c.C, *c.V) and (fold is not None) == (c.fold_mode is not None) and (labels is not None) == c.labels
        assert (lut is not None) == c.lut
        if c.crop:
            assert all(o >= 0 and o + d <= v for o, d, v in zip(*c.crop, c.V)) and all(o > 0 for o in c.crop[0][1:])
        nan = (acc & 0x7FFF) > 0x7C00
        assert nan.any() == c.special or not c.special
        if c.C > 1:
            f = acc.view(np.float16).astype(np.float32)
            assert ((f == f.max(0)).sum(0) > 1).any() or c.special         # exact ties for the argmax
    assert {c.C for c in cases} >= {1, 2, 255}
    assert {(c.C, c.vec) for c in cases} >= set(itertools.product((1, 2, 255), (1, 8)))
    assert any(c.special for c in cases if c.vec == 1) and any(c.special for c in cases if c.vec == 8)
    # pairwise coverage of the option values over every meaningful combination
    want = set().union(*(hc.option_pairs(r) for r in hc._valid_option_rows()))
    got = set().union(*(hc.option_pairs(hc.finalize_options(c)) for c in cases if c.name.startswith("opt")))
    assert want <= got, sorted(map(str, want - got))
    for a, b in (("fold_mode", 1), ("write_logits", 1)), (("crop", True), ("merge", 1)), (("crop", True), ("lut", True)):
        assert any((x == a and y == b) or (x == b and y == a) for x, y in got)            # the combinations the issue names
    assert {c.vec for c in cases if c.name.startswith("opt")} == {1, 8}


def test_finalize_form_predicate():
    assert hc.finalize_form((3, 5, 7)) == 1 and hc.finalize_form((2, 4, 8)) == 8
    V = (4, 3, 6)                                                          # 72 voxels, planes of 18
    assert hc.finalize_form(V) == 8
    assert [hc.finalize_form(V, (0, k)) for k in range(1, 5)] == [1, 1, 1, 8]     # v_count % 8
    assert hc.finalize_form(V, (2, 4)) == 1                                  # v_begin = 36
    assert hc.finalize_form((4, 2, 4), (1, 3)) == 8 and hc.finalize_form((4, 2, 4), (1, 2)) == 8
    for kw in ("acc_align", "n_align", "fold_align"):
        assert hc.finalize_form((2, 4, 8), **{kw: 2}) == 1


def test_fp16_patterns_hold_every_class_of_value():
    b = hc.fp16_patterns(np.random.default_rng(0), (4000,), special=True)
    m = b & 0x7FFF
    assert (m == 0).any() and (b == 0x8000).any() and ((m > 0) & (m < 0x0400)).any() and (m == 0x7C00).any() and (m > 0x7C00).any()
    assert ((m >= 0x0400) & (m < 0x7C00)).mean() > 0.8
    b = hc.fp16_patterns(np.random.default_rng(0), (4000,))
    assert ((b & 0x7FFF) < 0x7C00).all()
