"""CPU: the plan query returns the parent commit's plans for every layer the suite and the benchmark build, and the generated
single-layer cases (tests/conv_form_cases.py) cover every required form key below the size cap."""
import json
import os

import conv_form_cases as cf
from conftest import GOLDEN


def test_plans_equal_the_parent_commits_table():
    """tests/golden/conv_plans_parent.json was written by the parent commit's build (its choose_conv_tile and its inline cy_fast
    expression, before they were split into conv_tile_complete / conv_ws_cy_fast): the refactoring changes no plan."""
    with open(os.path.join(GOLDEN, "conv_plans_parent.json")) as f:
        want = json.load(f)
    got = cf.plan_table(cf.load_lib())
    assert sorted(got) == sorted(want)
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not diff, diff
    # both modes, every net, and a cost model that does depend on the CU count
    assert len(want) == 2 * len(cf.CU_COUNTS) * sum(len(cf.net_layers(c)) for c in cf.NETS.values())
    a, b = cf.CU_COUNTS
    assert any(want[k] != want[k.replace(f"/cu{a}/", f"/cu{b}/")] for k in want if f"/cu{a}/" in k)


def test_override_is_checked_as_the_planners_candidates_are():
    lib = cf.load_lib()
    geo = dict(cin0=32, cin1=0, dims=(9, 10, 40), cout=32, k=(3, 3, 3), s=(1, 1, 1), cu=cf.TEST_CU)
    p = cf.conv_plan(lib, mode="fp16", **geo)
    assert cf.conv_plan(lib, mode="fp16", override=p[0:8], **geo) == p        # the planner's own choice, completed identically
    assert cf.conv_plan(lib, mode="split", override=[0, 1, 1, 4, 8, 1, 1, 4], **geo) is None     # split precision: variant 1 / 2 only
    assert cf.conv_plan(lib, mode="fp16", override=[1, 4, 1, 1, 32, 16, 1, 1], **geo) is None    # 2 HV beyond the producers' reach / LDS
    assert cf.conv_plan(lib, mode="fp16", override=[1, 1, 1, 4, 8, 1, 1, 2], **geo) is None      # block tile is not 4 R M-tiles
    assert cf.conv_plan(lib, mode="fp16", override=[1, 1, 1, 3, 8, 1, 1, 4], **geo) is None      # wave tile is not 32 voxels
    assert cf.conv_plan(lib, mode="fp16", override=[2, 4, 1, 4, 8, 4, 1, 1], **geo) is None      # k_conv_ns does not take stride 1
    geo5 = dict(geo, k=(5, 3, 3))
    assert cf.conv_plan(lib, mode="fp16", override=[1, 1, 1, 4, 8, 1, 1, 4], **geo5) is None     # conv_ws_supported


def test_every_required_key_has_a_case():
    r = cf.report()
    assert r["conv_uncovered"] == [] and r["convt_uncovered"] == []
    have = {c["key"] for c in r["conv"]}
    missing = [k for k in r["conv_required"] if k not in have]
    assert len(missing) / len(r["conv_required"]) == 0.0, missing
    thave = {c["key"] for c in r["convt"]}
    tmissing = [k for k in r["convt_required"] if k not in thave]
    assert len(tmissing) / len(r["convt_required"]) == 0.0, tmissing
    # every key of the networks' layers is among the required ones (not only the grid's)
    assert sum(1 for v in r["conv_required"].values() if v != "grid") >= 10
    # the template instantiations the launchers choose between
    forms = {(k[0], k[1], k[2], k[3], k[4]) for k in have}   # family, R, K0, row reuse, X3
    for x3 in (0, 1):
        for k0 in (1, 3):
            for R in (1, 2, 4):
                assert ("ws", R, k0, 0, x3) in forms, (R, k0, x3)
            assert ("ws", 2, k0, 1, x3) in forms and ("ws", 4, k0, 1, x3) in forms, (k0, x3)
        assert {k[10] for k in have if k[0] == "ns" and k[4] == x3} == {2, 4}
        assert {k[5] for k in have if k[0] == "ws" and k[4] == x3} == {0, 1}       # resident
        assert {k[6] for k in have if k[0] == "ws" and k[4] == x3} == {0, 1}       # cy_fast
        assert {k[13] for k in have if k[0] == "ws" and k[4] == x3} == {False, True}   # the vw % 8 branch of ws_run_table
        assert any(k[6] == 1 and k[11] == 2 for k in have if k[4] == x3), "cy_fast with a second source"
    assert {("mfma", R) for R in (1, 2, 4)} <= {(k[0], k[1]) for k in have}
    templates = {k[0] for k in thave}
    assert templates == {"k_convt_mfma<1>", "k_convt_mfma<2>", "k_convt_mfma_rw<2,4,2>", "k_convt_mfma_rw<2,8,2>", "k_convt_deep<16>",
                         "k_convt_deep<20>", "k_convt_x3<1>", "k_convt_x3<2>"}, templates


def test_the_planner_never_picks_the_fallback_kernel_here():
    """k_conv_mfma runs in this suite through the override only: were the planner to start choosing it, its forms would have to join
    the required set through the grid like every other."""
    r = cf.report()
    assert all(v.startswith("k_conv_mfma") for k, v in r["conv_required"].items() if k[0] == "mfma")
    assert all(c["override"] is not None for c in r["conv"] if c["key"][0] == "mfma")


def test_situations_occur_for_every_family():
    r = cf.report()
    for x3 in (0, 1):
        for fam in ("mfma", "ws", "ns"):
            cs = [c for c in r["conv"] if c["key"][0] == fam and c["key"][4] == x3]
            if fam == "mfma" and x3:
                assert not cs
                continue
            assert {a for c in cs for a in c["overhang"]} == {0, 1, 2}, (fam, x3)
            assert any(not c["overhang"] for c in cs), (fam, x3)
            if fam != "mfma":   # (k_conv_mfma: one block per (tile, sample), no runs)
                assert {c["crossing"] for c in cs} == {False, True}, (fam, x3)
    for tmpl in {c["key"][0] for c in r["convt"]}:
        sit = {c["situation"] for c in r["convt"] if c["key"][0] == tmpl}
        assert {s[0] for s in sit} == {False, True}, (tmpl, sit)               # a partial last wave, and none
        if "x3" not in tmpl:
            assert any(s[1] for s in sit), (tmpl, sit)                          # a wave that spans two samples


def test_every_case_respects_the_cap_and_uses_the_override_only_where_needed():
    r = cf.report()
    lib = cf.load_lib()
    for c in r["conv"]:
        assert c["macs"] <= cf.MAC_CAP, c["id"]
        assert cf.conv_macs(c["dims"], c["cin0"] + c["cin1"], c["cout"], c["k"], c["s"], cf.BATCH) == c["macs"]
        p = cf.conv_plan(lib, c["cin0"], c["cin1"], c["dims"], c["cout"], c["k"], c["s"], cf.TEST_CU, c["mode"], c["override"])
        assert p == c["plan"], c["id"]
        if c["override"] is not None:
            own = cf.conv_plan(lib, c["cin0"], c["cin1"], c["dims"], c["cout"], c["k"], c["s"], cf.TEST_CU, c["mode"])
            assert own[0:8] != c["plan"][0:8], f"{c['id']}: the planner picks this plan itself"
    for c in r["convt"]:
        assert c["macs"] <= cf.MAC_CAP, c["id"]
    assert len({c["id"] for c in r["conv"]}) == len(r["conv"]) and len({c["id"] for c in r["convt"]}) == len(r["convt"])


def test_k16_xfails_are_the_arithmetic_not_the_kernel():
    """The three strict xfails of tests/test_gpu_conv_forms.py: the numpy model of the split-precision product (hi / lo fp16 parts, the lo
    parts of small activations subnormal) is over tau_x3 on the very inputs of those cases, by what the GPU measures, and under it on
    the other split-precision transposed-conv cases of the same form."""
    import zlib

    import numpy as np

    import layer_reference as lr
    import test_gpu_conv_forms as g
    ids = {c["id"] for c in cf.convt_cases()}
    assert set(g.XFAIL) <= ids
    for case in cf.convt_cases():
        if not (case["mode"] == "split" and case["norm"] is True and case["key"][0] == "k_convt_x3<2>"):
            continue
        rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
        cin, cout, s = case["cin"], case["cout"], case["s"]
        x = rng.standard_normal((cin, *case["dims"])).astype(np.float32)
        ss, _ = g._tables(rng, cin, True, False)
        w = (rng.standard_normal((cin, cout, *s)) / np.sqrt(cin)).astype(np.float32)
        b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
        X = lr.norm_act_x3(x, ss).reshape(cin, -1)
        worst = 0.0
        for t in np.ndindex(*s):
            wt = np.ascontiguousarray(w[(slice(None), slice(None)) + t].T)   # [Cout, Cin] of one tap
            c64 = wt.astype(np.float64) @ X.astype(np.float64) + b.astype(np.float64)[:, None]
            A = np.abs(wt).astype(np.float64) @ np.abs(X).astype(np.float64) + np.abs(b).astype(np.float64)[:, None]
            worst = max(worst, float((np.abs(lr.x3_dot_emulate(wt, X, b).astype(np.float64) - c64) / A).max()))
        assert (worst > lr.tau_x3(cin)) == (case["id"] in g.XFAIL), (case["id"], worst)
