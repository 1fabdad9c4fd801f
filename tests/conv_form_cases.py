"""Single-layer cases for every kernel form and tile plan of the conv stack (tests/test_conv_form_cases_cpu.py proves the set on the
CPU, tests/test_gpu_conv_forms.py runs it).

A FORM is everything that selects code for one layer: boa_conv_plan / boa_convt_plan report it from the functions the network set-up
and the launchers call, without touching a GPU.  The form key of a conv:
    family (mfma / ws / ns), R, K0, row reuse, X3, resident weights, cy_fast, xs padded, wave tile w, stride s, the cout wave split of
    k_conv_ns, one or two sources, each source raw or normalised, the vw % 8 == 0 branch of ws_run_table
  + the situation of the case: which axes a block tile overhangs the tensor on, whether a workgroup's run crosses a sample boundary at
    the test's batch (N * vw > grid).
of a transposed conv:
    template (k_convt_mfma<1|2>, k_convt_mfma_rw<2,4|8,2>, k_convt_deep<16|20>, k_convt_x3<1|2>), s, X3, MT, source raw / with the
    producer's tables / with the fp32 table alone
  + a partial last wave, a wave that spans two samples.

REQUIRED keys = the keys of every layer of every network the suite and the benchmark build (NETS x both modes x CU_COUNTS: the table
tests/golden/conv_plans_parent.json pins those plans to the parent commit's) + every key the planner itself chooses over GRID, a
declared set of small geometries.  For each required key the case with the fewest multiply-accumulates is taken (tensors at least as wide as the kernel first); the planner's own
choice where it gives the key below MAC_CAP, else the table row's plan as an override (the seam completes and checks it as the
planner's candidates are) on a GRID extent.  Situations are then topped up: every overhang axis (and none) and both batch situations
for every kernel family.  Plans of the smaller CU count enter as the form they take on TEST_CU compute units (the device the suite
runs on): vw, and with it the run-table branch, is a function of the device."""
from __future__ import annotations

import ctypes as C
import functools
import itertools
from typing import Dict, List, Optional

import numpy as np

PLAN_WORDS = 32
MODES = {"fp16": 0, "split": 2}
TEST_CU = 256                 # MI355X
CU_COUNTS = (256, 104)
MAC_CAP = 2 ** 30
BATCH = 3                     # the second batch size of a conv case (sample 0 repeated)

NETS = {
    "total128": dict(patch=(128, 128, 128), features=(32, 64, 128, 256, 320, 320)),
    "bca": dict(patch=(16, 64, 64), features=(32, 64, 128, 256), kernels=[[1, 3, 3], [1, 3, 3], [3, 3, 3], [3, 3, 3]],
                strides=[[1, 1, 1], [1, 2, 2], [1, 2, 2], [2, 2, 2]]),
    "ragged": dict(patch=(16, 48, 40), features=(32, 64, 128, 256), kernels=[[1, 3, 3], [3, 3, 3], [3, 3, 3], [3, 3, 3]],
                   strides=[[1, 1, 1], [1, 2, 2], [2, 2, 2], [2, 2, 2]]),
    "small32": dict(patch=(32, 32, 32), features=(32, 64, 128)),
    "cfg64x96x64": dict(patch=(64, 96, 64), features=(32, 64, 128)),
    "cfg64": dict(patch=(64, 64, 64), features=(32, 64, 128)),
}

# the declared grid of small geometries (input extents; ragged, tiny, one voxel, last axis 2, one whose stride-2 output overhangs
# k_conv_ns's 4 x 4 x 8 tile on every axis, and two with enough tiles per sample that a workgroup's run crosses a sample boundary at BATCH)
GRID_EXTENTS = [(1, 1, 1), (2, 3, 2), (3, 5, 7), (4, 4, 4), (8, 8, 8), (6, 20, 20), (9, 10, 40), (5, 17, 33), (16, 16, 16), (18, 20, 20), (16, 16, 32), (12, 24, 48),
                (32, 32, 96)]
GRID_CIN = [16, 32, 64, 128, 256, 320, 640]
GRID_COUT = [32, 64, 96, 128, 256, 320]
GRID_K = [(3, 3, 3), (1, 3, 3)]
GRID_S = [(1, 1, 1), (2, 2, 2), (1, 2, 2)]
GRID_CONVT_EXTENTS = [(1, 1, 1), (3, 5, 7), (4, 4, 4), (5, 17, 33), (8, 8, 8), (16, 16, 16), (17, 16, 17)]
GRID_CONVT_S = [(2, 2, 2), (1, 2, 2), (2, 2, 1)]
CONVT_BATCHES = (1, 3)


def _int3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


def load_lib():
    from boa_hip import _lib
    return _lib.lib()


def conv_plan(lib, cin0, cin1, dims, cout, k, s, cu, mode, override=None) -> Optional[List[int]]:
    out = (C.c_int * PLAN_WORDS)()
    ov = None if override is None else (C.c_int * 8)(*override)
    rc = lib.boa_conv_plan(cin0, cin1, _int3(dims), cout, _int3(k), _int3(s), cu, MODES[mode], ov, out)
    return list(out) if rc == 0 else None


def convt_plan(lib, cin, dims, cout, s, cu, mode, norm) -> Optional[List[int]]:
    out = (C.c_int * PLAN_WORDS)()
    rc = lib.boa_convt_plan(cin, _int3(dims), cout, _int3(s), cu, MODES[mode], 1 if norm else 0, out)
    return list(out) if rc == 0 else None


# ---- the layers of a network (what net.hip's setup walks; the first conv and the head are not MFMA-conv layers) -------------------------
def net_layers(cfg) -> List[Dict]:
    feats, patch = list(cfg["features"]), list(cfg["patch"])
    n = len(feats)
    kernels = cfg.get("kernels") or [[3, 3, 3]] * n
    strides = cfg.get("strides") or [[1, 1, 1]] + [[2, 2, 2]] * (n - 1)
    out, dims, stage_dims = [], patch, []
    cin = None
    for st in range(n):
        for i in range(2):
            k, s = tuple(kernels[st]), tuple(strides[st]) if i == 0 else (1, 1, 1)
            din = dims
            if i == 0:
                dims = [(d + 2 * ((kk - 1) // 2) - kk) // ss + 1 for d, kk, ss in zip(dims, k, s)]
            if not (st == 0 and i == 0):
                out.append(dict(name=f"enc{st}.conv{i}", kind="conv", cin0=cin, cin1=0, norms=(True,), dims=tuple(din), cout=feats[st], k=k, s=s))
            cin = feats[st]
        stage_dims.append(tuple(dims))
    for kk in range(n - 1):
        sb = n - 1 - kk
        below, skip, s = feats[sb], feats[sb - 1], tuple(strides[sb])
        out.append(dict(name=f"up{kk}", kind="convt", cin=below, norm=True, dims=stage_dims[sb], cout=skip, s=s))
        k = tuple(kernels[sb - 1])
        out.append(dict(name=f"dec{kk}.conv0", kind="conv", cin0=skip, cin1=skip, norms=(False, True), dims=stage_dims[sb - 1], cout=skip, k=k,
                        s=(1, 1, 1)))
        out.append(dict(name=f"dec{kk}.conv1", kind="conv", cin0=skip, cin1=0, norms=(True,), dims=stage_dims[sb - 1], cout=skip, k=k, s=(1, 1, 1)))
    return out


def plan_table(lib) -> Dict[str, List[int]]:
    """The plan of every layer of NETS in both modes at CU_COUNTS (the fixture tests/golden/conv_plans_parent.json)."""
    tab = {}
    for net, cfg in NETS.items():
        for L in net_layers(cfg):
            for mode in MODES:
                for cu in CU_COUNTS:
                    if L["kind"] == "conv":
                        p = conv_plan(lib, L["cin0"], L["cin1"], L["dims"], L["cout"], L["k"], L["s"], cu, mode)
                    else:
                        p = convt_plan(lib, L["cin"], L["dims"], L["cout"], L["s"], cu, mode, L["norm"])
                    assert p is not None, (net, L, mode, cu)
                    tab[f"{net}/{mode}/cu{cu}/{L['name']}"] = p[:29]
    return tab


# ---- keys ------------------------------------------------------------------------------------------------------------------------------
FAMILY = {0: "mfma", 1: "ws", 2: "ns"}


def conv_base_key(p, k, s, norms):
    variant = p[0]
    return (FAMILY[variant], p[1], k[0], p[16], p[28], p[17], p[18], int(p[11] != p[9] * p[10]), tuple(p[2:5]), tuple(s), p[21],
            len(norms), tuple(bool(x) for x in norms), (p[19] % 8 == 0) if variant else None)


CONV_KEY_FIELDS = ("family", "R", "K0", "row_reuse", "X3", "resident", "cy_fast", "xs_padded", "w", "s", "ns_waves", "sources", "normalised",
                   "vw%8==0")


def conv_overhang(p):
    return tuple(a for a in range(3) if p[12 + a] * p[5 + a] * p[2 + a] > p[24 + a])


def conv_crossing(p, n, cu=TEST_CU):
    """Does a workgroup walk runs of more than one sample: grid = min(N vw, CUs) < N vw (k_conv_mfma: one block per (tile, n))."""
    return None if p[0] == 0 else bool(n * p[19] > min(n * p[19], cu))


def conv_macs(dims, cin, cout, k, s, n=1):
    do = [(d + 2 * ((kk - 1) // 2) - kk) // ss + 1 for d, kk, ss in zip(dims, k, s)]
    return n * int(np.prod(do)) * int(np.prod(k)) * cin * cout


def convt_template(p, cin):
    form = p[0]
    if form == -1:
        return f"k_convt_x3<{p[1]}>"
    if form == 2:
        return f"k_convt_deep<{cin // 16}>"
    if form == 1:
        return f"k_convt_mfma_rw<2,{cin // 16},2>"
    return f"k_convt_mfma<{p[3]}>"


def convt_base_key(p, cin, s, norm):
    return (convt_template(p, cin), tuple(s), int(p[0] == -1), p[1], {True: "tables", False: "raw", "f32": "fp32 table"}[norm])


def convt_situation(p, dims, n):
    """(partial last wave, a wave spans two samples): the fp16 kernels walk the N * vin voxels of the batch in waves of 32, k_convt_x3
    those of one sample (gridDim.y = N) in blocks of 32 MT."""
    vin = int(np.prod(dims))
    if p[0] == -1:
        return (vin % (32 * p[1]) != 0, False)
    return ((n * vin) % 32 != 0, n > 1 and vin % 32 != 0)


# ---- generation ------------------------------------------------------------------------------------------------------------------------
def _grid_conv(lib):
    """Every planner choice over the grid: dicts with the plan at TEST_CU."""
    for mode in MODES:
        for dims, k, s in itertools.product(GRID_EXTENTS, GRID_K, GRID_S):
            chans = [(ci, 0, co, (True,)) for ci in GRID_CIN for co in GRID_COUT]
            chans += [(c, c, c, (False, True)) for c in (32, 64, 128, 256, 320)]   # decoder conv0: cat(raw up, normalised skip)
            # two sources of one staged chunk each under cy_fast (32 -> 64 in the kernel's channel units), raw + normalised and both
            # normalised: the second source's table at the smallest channel counts
            half = 8 if mode == "split" else 16
            chans += [(half, half, 64, (False, True)), (half, half, 64, (True, True))]
            for cin0, cin1, cout, norms in chans:
                if conv_macs(dims, cin0 + cin1, cout, k, s, BATCH) > MAC_CAP:
                    continue
                p = conv_plan(lib, cin0, cin1, dims, cout, k, s, TEST_CU, mode)
                if p is None:
                    continue
                yield dict(kind="conv", mode=mode, cin0=cin0, cin1=cin1, norms=norms, dims=dims, cout=cout, k=k, s=s, override=None, plan=p)


def _with_key(c):
    c["key"] = conv_base_key(c["plan"], c["k"], c["s"], c["norms"])
    c["overhang"] = conv_overhang(c["plan"])
    c["crossing"] = conv_crossing(c["plan"], BATCH)
    c["macs"] = conv_macs(c["dims"], c["cin0"] + c["cin1"], c["cout"], c["k"], c["s"], BATCH)
    return c


def _order(c):
    # fewest multiply-accumulates among the tensors on which every tap meets data (an extent shorter than the kernel leaves taps that
    # only ever see padding: such a tensor is taken for the keys the planner emits on nothing larger)
    return (any(d < kk for d, kk in zip(c["dims"], c["k"])), c["macs"], c["mode"], c["dims"], c["cin0"], c["cin1"], c["cout"], c["k"], c["s"], c["override"] is not None)


def _table_conv_candidates(lib):
    """The plans of the networks' layers, as overrides on the grid extents (and as the planner's choice on the layer's own extents)."""
    seen = set()
    for net, cfg in NETS.items():
        for L in net_layers(cfg):
            if L["kind"] != "conv":
                continue
            for mode in MODES:
                for cu in CU_COUNTS:
                    p = conv_plan(lib, L["cin0"], L["cin1"], L["dims"], L["cout"], L["k"], L["s"], cu, mode)
                    ov = tuple(p[0:8])
                    sig = (mode, L["cin0"], L["cin1"], L["cout"], L["k"], L["s"], ov)
                    if sig in seen:
                        continue
                    seen.add(sig)
                    # the form this plan takes on the test device, on the layer's own extents: the required key
                    p_here = conv_plan(lib, L["cin0"], L["cin1"], L["dims"], L["cout"], L["k"], L["s"], TEST_CU, mode, ov)
                    assert p_here is not None, (net, L["name"], mode, cu, ov)
                    req = conv_base_key(p_here, L["k"], L["s"], L["norms"])
                    cands = []
                    for dims in GRID_EXTENTS + [L["dims"]]:
                        if conv_macs(dims, L["cin0"] + L["cin1"], L["cout"], L["k"], L["s"], BATCH) > MAC_CAP:
                            continue
                        q = conv_plan(lib, L["cin0"], L["cin1"], dims, L["cout"], L["k"], L["s"], TEST_CU, mode, ov)
                        if q is None:
                            continue
                        cands.append(_with_key(dict(kind="conv", mode=mode, cin0=L["cin0"], cin1=L["cin1"], norms=L["norms"], dims=tuple(dims),
                                                    cout=L["cout"], k=L["k"], s=L["s"], override=list(ov), plan=q)))
                    yield f"{net}/{mode}/cu{cu}/{L['name']}", req, cands


@functools.lru_cache(maxsize=1)
def _generate():
    lib = load_lib()
    grid = [_with_key(c) for c in _grid_conv(lib)]
    best: Dict[tuple, Dict] = {}
    for c in grid:   # every key the planner chooses over the grid, at its cheapest
        if c["key"] not in best or _order(c) < _order(best[c["key"]]):
            best[c["key"]] = c
    required = {k: "grid" for k in best}
    pool = list(grid)
    uncovered = []
    for row, req, cands in _table_conv_candidates(lib):
        required.setdefault(req, row)
        pool += cands
        if req in best and best[req]["override"] is None:
            continue   # the planner itself picks this form on a small geometry
        hit = [c for c in cands if c["key"] == req]
        if hit:
            c = min(hit, key=_order)
            if req not in best or _order(c) < _order(best[req]):
                best[req] = c
        elif req not in best:
            uncovered.append((row, req))
    # k_conv_mfma (variant 0) is the planner's fallback: no layer of NETS and no grid geometry takes it (the CPU test asserts that), so
    # its three instantiations run as overrides, on extents that overhang every axis and on one that fits
    for R, dims in itertools.product((1, 2, 4), ((9, 10, 40), (5, 17, 33), (8, 8, 16))):
        for b in ((1, 1, 4 * R), (2, 2, R)):
            ov = [0, R, 1, 4, 8, *b]
            q = conv_plan(lib, 32, 0, dims, 32, (3, 3, 3), (1, 1, 1), TEST_CU, "fp16", ov)
            if q is not None:
                c = _with_key(dict(kind="conv", mode="fp16", cin0=32, cin1=0, norms=(True,), dims=dims, cout=32, k=(3, 3, 3), s=(1, 1, 1),
                                   override=ov, plan=q))
                pool.append(c)
                required.setdefault(c["key"], "k_conv_mfma (override only)")
                if c["key"] not in best or _order(c) < _order(best[c["key"]]):
                    best[c["key"]] = c
    # k_conv_ws<R, K0, ., ., YR, X3>: an instantiation the planner reaches neither in NETS nor on the grid runs as an override too
    def tmpl(key):
        return key[0:5]
    for mode, x3 in (("fp16", 0), ("split", 1)):
        for R, k0, yr in itertools.product((1, 2, 4), (1, 3), (0, 1)):
            if (yr and R == 1) or any(tmpl(k) == ("ws", R, k0, yr, x3) for k in best):
                continue
            found = []
            for dims, w in itertools.product(((9, 10, 40), (8, 8, 16)), ((1, 1, 32), (1, 2, 16), (1, 4, 8), (2, 2, 8), (4, 1, 8))):
                for b0, b1 in itertools.product((1, 2, 4, 8, 16), repeat=2):
                    if (4 * R) % (b0 * b1):
                        continue
                    ov = [1, R, *w, b0, b1, 4 * R // (b0 * b1)]
                    q = conv_plan(lib, 32, 0, dims, 32, (k0, 3, 3), (1, 1, 1), TEST_CU, mode, ov)
                    if q is not None and q[16] == yr:
                        found.append(_with_key(dict(kind="conv", mode=mode, cin0=32, cin1=0, norms=(True,), dims=dims, cout=32, k=(k0, 3, 3),
                                                    s=(1, 1, 1), override=ov, plan=q)))
            if found:
                c = min(found, key=lambda c: (_order(c), c["override"]))
                pool.append(c)
                required.setdefault(c["key"], "k_conv_ws instantiation (override only)")
                best.setdefault(c["key"], c)
    chosen = list(best.values())
    # situations: every overhang axis (and a case without overhang) and both batch situations for every family
    def top_up(pred):
        if not any(pred(c) for c in chosen):
            extra = [c for c in pool if pred(c)]
            if extra:
                chosen.append(min(extra, key=_order))
    for x3 in (0, 1):
        for fam in ("mfma", "ws", "ns"):
            if x3 and fam == "mfma":
                continue   # (the split-precision mode has no variant 0)
            mine = lambda c, fam=fam, x3=x3: c["key"][0] == fam and c["key"][4] == x3
            for a in range(3):
                top_up(lambda c, a=a: mine(c) and a in c["overhang"])
            top_up(lambda c: mine(c) and not c["overhang"])
            if fam != "mfma":
                top_up(lambda c: mine(c) and c["crossing"] is True)
                top_up(lambda c: mine(c) and c["crossing"] is False)
    chosen.sort(key=lambda c: (c["mode"], c["key"][0], _order(c)))
    for i, c in enumerate(chosen):
        ov = "" if c["override"] is None else "-ov" + "".join(str(v) for v in c["override"])
        c["id"] = (f"{c['mode']}-{c['key'][0]}R{c['key'][1]}-{c['cin0']}+{c['cin1']}to{c['cout']}-" + "x".join(map(str, c["dims"])) + "-k"
                   + "".join(map(str, c["k"])) + "s" + "".join(map(str, c["s"])) + "-" + "".join("n" if x else "r" for x in c["norms"]) + ov)
    assert len({c["id"] for c in chosen}) == len(chosen)

    # transposed convs
    tbest: Dict[tuple, Dict] = {}
    treq = {}
    def tcase(mode, cin, cout, dims, s, norm, n):
        # norm: False = raw source, True = the producer's tables as the network passes them (fp16: fp32 + packed fp16; the fp16 kernels
        # read the packed one), "f32" = the fp32 table alone (fp16 mode: k_convt_mfma's norm_act8 path, which no network reaches)
        if norm == "f32" and mode != "fp16":
            return None
        p = convt_plan(lib, cin, dims, cout, s, TEST_CU, mode, norm is True)
        if p is None:
            return None
        vin = int(np.prod(dims))
        return dict(kind="convt", mode=mode, cin=cin, cout=cout, dims=tuple(dims), s=tuple(s), norm=norm, N=n, plan=p,
                    key=convt_base_key(p, cin, s, norm), situation=convt_situation(p, dims, n), macs=n * vin * int(np.prod(s)) * cin * cout)
    tpool = []
    for mode in MODES:
        for dims, s, cin, cout, norm, n in itertools.product(GRID_CONVT_EXTENTS, GRID_CONVT_S, GRID_CIN, (32, 64), (True, False, "f32"), CONVT_BATCHES):
            c = tcase(mode, cin, cout, dims, s, norm, n)
            if c is None or c["macs"] > MAC_CAP:
                continue
            tpool.append(c)
            full = c["key"] + c["situation"]
            if full not in tbest or (c["macs"], c["dims"], c["cin"]) < (tbest[full]["macs"], tbest[full]["dims"], tbest[full]["cin"]):
                tbest[full] = c
            treq.setdefault(c["key"], "grid")
    tuncovered = []
    for net, cfg in NETS.items():
        for L in net_layers(cfg):
            if L["kind"] != "convt":
                continue
            for mode in MODES:
                p = convt_plan(lib, L["cin"], L["dims"], L["cout"], L["s"], TEST_CU, mode, L["norm"])
                key = convt_base_key(p, L["cin"], L["s"], L["norm"])
                treq.setdefault(key, f"{net}/{mode}/{L['name']}")
                if not any(k[:len(key)] == key for k in tbest):
                    c = tcase(mode, L["cin"], L["cout"], L["dims"], L["s"], L["norm"], 1)
                    if c["macs"] <= MAC_CAP:
                        tbest[c["key"] + c["situation"]] = c
                    else:
                        tuncovered.append((f"{net}/{mode}/{L['name']}", key))
    tchosen = sorted(tbest.values(), key=lambda c: (c["mode"], c["key"][0], c["macs"], c["dims"], c["N"]))
    for c in tchosen:
        c["id"] = (f"{c['mode']}-{c['key'][0]}-{c['cin']}to{c['cout']}-" + "x".join(map(str, c["dims"])) + "-s" + "".join(map(str, c["s"]))
                   + {True: "-norm", False: "-raw", "f32": "-f32tab"}[c["norm"]] + f"-N{c['N']}")
    assert len({c["id"] for c in tchosen}) == len(tchosen)
    return dict(conv=chosen, conv_required=required, conv_uncovered=uncovered, convt=tchosen, convt_required=treq, convt_uncovered=tuncovered)


def conv_cases():
    return _generate()["conv"]


def convt_cases():
    return _generate()["convt"]


def report():
    return _generate()
