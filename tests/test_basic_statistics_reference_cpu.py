"""CPU: tests/basic_statistics_reference.py (the numpy restatement the GPU tests compare with) and the host arithmetic of
boa_hip/statistics.py (`stats_from_table`) against golden G17 -- the reference's OWN get_basic_statistics (TS/statistics.py:91-141)
executed on the calls of tests/basic_statistics_cases.py by tests/golden/make_golden_statistics.py.

Everything but the normalised mean is compared bit for bit (volume and intensity as float64, the key order).  The normalised mean is a
sum of n non-integer doubles in the reference (pairwise summation): the restatement runs the same numpy code and must give the same
double; the product's closed form (sum - n min) / (n (max - min)) is compared on the unrounded value at rtol 1e-12 and on the rounded
value within one unit of the fifth decimal."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import basic_statistics_cases as cases
import basic_statistics_reference as R


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "g17_basic_statistics.json")) as f:
        g = json.load(f)
    z = np.load(os.path.join(GOLDEN, "g17_basic_statistics.npz"))
    return g, z


def _class_map(g):
    return {int(k): v for k, v in g["class_map"]}


def test_cases_are_the_golden_inputs(golden):
    g, z = golden
    for name in cases.VOLUMES:
        seg, ct, zooms = cases.volume(name)
        np.testing.assert_array_equal(seg, z[f"{name}.seg"])
        np.testing.assert_array_equal(ct, z[f"{name}.ct"])
        assert ct.dtype == z[f"{name}.ct"].dtype and zooms.tobytes() == z[f"{name}.zooms"].tobytes()
    assert sorted(g["calls"]) == [cases.call_key(k) for k in range(len(cases.CALLS))]
    for k, (_, kw) in enumerate(cases.CALLS):
        assert g["calls"][cases.call_key(k)]["kwargs"] == kw


def test_class_map_is_the_products(golden):
    """the reference's class map, in its own order, is the product's sorted by label id (what basic_statistics iterates)"""
    from boa_hip import label_maps
    assert sorted(label_maps.class_map(cases.TASK).items()) == list(_class_map(golden[0]).items())


@pytest.mark.parametrize("k", range(len(cases.CALLS)), ids=[cases.call_key(k) for k in range(len(cases.CALLS))])
def test_restatement_equals_the_reference(golden, k):
    g, _ = golden
    name, kw = cases.CALLS[k]
    seg, ct, zooms = cases.volume(name)
    got = R.basic_statistics(seg, ct, zooms, _class_map(g), **kw)
    want = g["calls"][cases.call_key(k)]["stats"]
    assert list(got) == [w[0] for w in want]                        # names and their order (roi_subset filters)
    for nme, vol, inten in want:
        assert float(got[nme]["volume"]) == vol and float(got[nme]["intensity"]) == inten, (nme, got[nme], vol, inten)
    if "roi_subset" in kw:
        assert set(got) == set(kw["roi_subset"])
    # the cases mean something: reported and excluded structures both occur
    if name == "blocks" and kw["exclude_masks_at_border"] and "roi_subset" not in kw:
        assert got["liver"]["volume"] > 0 and got["stomach"]["volume"] == 0 and got["heart"]["volume"] == 0 and got["brain"]["volume"] > 0


def _host_medians(seg, hu, class_map):
    out = {}
    for idx in class_map:
        v = np.sort(hu[seg == idx])
        if v.size:
            out[idx] = (int(v[(v.size - 1) // 2]), int(v[v.size // 2]))
    return out


@pytest.mark.parametrize("k", range(len(cases.CALLS)), ids=[cases.call_key(k) for k in range(len(cases.CALLS))])
def test_product_host_arithmetic_equals_the_reference(golden, k):
    """stats_from_table on the restated device table (tests/basic_statistics_reference.py:stats_table)"""
    from boa_hip import statistics as S
    g, _ = golden
    name, kw = cases.CALLS[k]
    seg, ct, zooms = cases.volume(name)
    hu = np.asarray(ct).astype(np.int16)
    t = R.stats_table(seg, hu)
    mm = t[768:].view(np.int64)
    cm = _class_map(g)
    got, raw = S.stats_from_table(t[:256], t[256:512].view(np.int64), t[512:768] != 0, int(mm[0]), int(mm[1]), zooms, cm,
                                  medians=_host_medians(seg, hu, cm), return_unrounded=True, **kw)
    want = g["calls"][cases.call_key(k)]["stats"]
    assert list(got) == [w[0] for w in want]
    norm_mean = kw.get("normalized_intensities") and kw["metric"] == "mean"
    for nme, vol, inten in want:
        assert float(got[nme]["volume"]) == vol, (nme, got[nme], vol)
        if not norm_mean:
            assert float(got[nme]["intensity"]) == inten, (nme, got[nme], inten)
        else:
            assert abs(float(got[nme]["intensity"]) - inten) <= 1.0000001e-5, (nme, got[nme], inten)
    if norm_mean:            # the unrounded value against the reference's summation, restated
        f = (hu - hu.min()) / (hu.max() - hu.min())
        for nme, v in raw.items():
            idx = [i for i, n in cm.items() if n == nme][0]
            np.testing.assert_allclose(v, np.average(f, weights=(seg == idx).astype(np.uint8)), rtol=1e-12, atol=0)


def test_stats_table_restatement_border_slabs():
    """`i < 3 || i >= dim - 3` is numpy's mask[:3] / mask[-3:] for every dim from 1 on (the slabs overlap below 6, cover all below 3)"""
    for d in range(1, 9):
        for pos in range(d):
            seg = np.zeros((d, 9, 9), np.uint8)
            seg[pos, 4, 4] = 7
            t = R.stats_table(seg, np.zeros(seg.shape, np.int16))
            assert bool(t[512 + 7]) == R.touches_border(seg == 7), (d, pos)
            assert bool(t[512 + 7]) == (pos < 3 or pos >= d - 3)
