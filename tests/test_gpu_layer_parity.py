"""Per-layer fp64 parity of the conv stack (exact mode = precision 2, fp16 mode = precision 0, fp32_ref = precision 1).

Every layer's RAW stored output (boa_net_debug_layer) is compared with a float64 recomputation of the same layer from the GPU's
OWN inputs -- the stored raw outputs of its sources put through the consuming kernel's input transform, bit for bit
(tests/layer_reference.py) -- so each layer is judged alone, at the level where its kernel works:
    |c - c64| <= tau * A,   A = sum |w| |x| + |b|   (+ 2^-11 |c64| + 2^-25 for the fp16 storage of the fp16 mode)
tau_x3(K) (exact and fp32_ref modes) and TAU_FP16 are set from the MI355X measurement (<= 2x margin, never above the fp32-class
ceiling 2^-20 max(1, sqrt(K / 4096))); the test prints a per-layer table of max / rms err/A and the kernel that ran.  The
InstanceNorm (scale, shift) of every conv is compared with the fp64 statistics of the same raw output; in the fp16 mode the packed
fp16 table must be the fp16 rounding of the fp32 one, bit for bit.

Production `total` geometry: patch 128^3, features 32/64/128/256/320/320, 25 classes, two tiles (one overhangs the volume: the
first conv's zero padding), exact mode on both, fp16 on tile 0; coverage of the kernel forms is asserted from host_info and the
launch counters.  Edges on small geometries: (1,3,3) kernels with (1,2,2) strides (consume_chunk_y_x3 with K0 = 1), a non-cubic
patch with ragged tiles, a transposed conv / decoder conv0 pair rescaled by 2^-k / 2^k (k = 6, 14: the same function with a tiny
raw source), output channels whose weights sit 2^-16 / 2^-24 below the layer's largest (the per-layer power-of-two weight
scale), and a conv bias of ~30 standard deviations of the conv output (E[c^2] - mean^2 in the statistics)."""
import ctypes as C

import numpy as np
import pytest

import layer_reference as lr

pytestmark = pytest.mark.gpu

LK = {1: "first_valu", 2: "first_mfma", 3: "conv_ws", 4: "conv_ns", 5: "conv_mfma", 6: "conv_f32", 7: "convt_x3", 8: "convt_mfma",
      9: "convt_rw", 10: "convt_deep", 11: "convt_f32", 12: "head_x3", 13: "head_f32", 14: "head_mfma"}

# the (scale, shift) bars and SS_EPS: layer_reference.ss_bars (shared with tests/test_gpu_conv_forms.py)


@pytest.fixture(scope="module")
def ctx():
    import torch
    from boa_hip.device import Context
    torch.set_num_threads(16)
    c = Context(0)
    yield c
    c.close()


def _model(patch, features, classes, kernels=None, strides=None, seed=0):
    from boa_hip import plans
    pj, dj = plans.synthetic_plans(patch=patch, features=features, num_classes=classes, kernels=kernels, strides=strides)
    geom = plans.model_config_from_plans(pj, dj).geometry
    return geom, plans.synthetic_state_dict(geom, seed)


def _tile(vol, o, patch):
    """The network input of a tile at origin o: zeros outside the volume (pad_nd_image + overhang)."""
    out = np.zeros((vol.shape[0],) + tuple(patch), np.float32)
    src, dst = [], []
    for a in range(3):
        lo, hi = max(0, o[a]), min(vol.shape[1 + a], o[a] + patch[a])
        src.append(slice(lo, hi))
        dst.append(slice(lo - o[a], hi - o[a]))
    out[(slice(None),) + tuple(dst)] = vol[(slice(None),) + tuple(src)]
    return out


def _read(ctx, pred, L, tile, fp16):
    lib = ctx.lib
    ch, dims, info = C.c_int(), (C.c_int * 3)(), (C.c_int * 3)()
    assert lib.boa_net_debug_layer(pred._net, L.kind, L.stage, L.conv, tile, None, None, None, C.byref(ch), dims, info) == 0
    shape = (ch.value, dims[0], dims[1], dims[2])
    buf = ctx.alloc(int(np.prod(shape)) * 4)
    ss = np.zeros((ch.value, 2), np.float32)
    ss16 = np.zeros(ch.value * 2, np.uint16) if (fp16 and L.kind != 1) else None
    rc = lib.boa_net_debug_layer(pred._net, L.kind, L.stage, L.conv, tile, buf.vp, ss.ctypes.data_as(C.c_void_p),
                                 None if ss16 is None else ss16.ctypes.data_as(C.c_void_p), C.byref(ch), dims, info)
    assert rc == 0, lib.boa_last_error()
    ctx.sync()
    raw = buf.download(shape, np.float32)
    buf.free()
    return {"raw": raw, "ss": ss, "ss16": ss16, "info": (info[0], info[1], info[2])}


def _run(ctx, geom, sd, vol, origins, prec, tiles):
    """Forward the batch in one precision; per tile: every layer's stored output + tables + kernel, and the logits."""
    from boa_hip import plans
    from boa_hip.predictor import HipPredictor
    blob = plans.weight_blob_from_state_dict(geom, sd)
    p = HipPredictor(ctx, geom, max_batch=len(origins), precision=prec)
    assert p.precision == prec, "no silent fall-back to another precision"
    p.set_parameters([blob])
    ctx.counters(reset=True)
    logits = p.network_forward(vol, np.asarray(origins, dtype=np.int32))
    cnt = ctx.counters()
    walk = lr.layer_walk(geom)
    out = [{L.name: _read(ctx, p, L, t, prec == "fp16") for L in walk if L.kind != 3} for t in tiles]
    ch, dims, info = C.c_int(), (C.c_int * 3)(), (C.c_int * 3)()
    assert ctx.lib.boa_net_debug_layer(p._net, 3, 0, 0, 0, None, None, None, C.byref(ch), dims, info) == 0
    p.close()
    for t, d in zip(tiles, out):
        d["head"] = {"raw": logits[t], "info": (info[0], 0, 0)}
    return out, cnt


def _consumer_input(prec, layers, L, src_name, src, consumer_info):
    """What the consumer of `src` builds from it (tests/layer_reference.py): exact / fp32_ref: lrelu(fmaf(raw, s, t)) in fp32;
    fp16: the packed fp16 transform for k_conv_ws / k_conv_ns / k_convt_mfma_rw / k_convt_deep, the fp32-table one otherwise."""
    S = layers[src_name]
    if S.normkey is None:   # transposed conv output: consumed raw
        return src["raw"].astype(np.float64)
    if prec != "fp16":
        return lr.norm_act_x3(src["raw"], src["ss"]).astype(np.float64)
    if LK[consumer_info[0]] in ("conv_ws", "conv_ns", "convt_rw", "convt_deep"):
        return lr.norm_act8_pk(src["raw"].astype(np.float16), lr.ss16_unpack(src["ss16"])).astype(np.float64)
    return lr.norm_act8(src["raw"].astype(np.float16), src["ss"]).astype(np.float64)


def _check(prec, geom, sd, tile_in, got, tag, rows, fails):
    """All layers of one tile: conv error against tau * A, (scale, shift) against the fp64 statistics."""
    walk = lr.layer_walk(geom)
    layers = {L.name: L for L in walk}
    for L in walk:
        d = got[L.name]
        info = d.get("info", (0, 0, 0))
        if L.kind == 3 and prec == "fp16":
            continue   # (the fp16 head is pinned bit for bit by test_gpu_head.py / test_gpu_gather_head.py)
        if L.kind == 3:
            xin = _consumer_input(prec, layers, L, L.sources[0], got[L.sources[0]], (0, 0, 0))
        else:
            xin = np.concatenate([tile_in.astype(np.float64) if s == "input" else _consumer_input(prec, layers, L, s, got[s], info)
                                  for s in L.sources], 0)
        w, b = sd[L.wkey + ".weight"].astype(np.float32), sd[L.wkey + ".bias"].astype(np.float32)
        if prec == "fp16" and L.kind != 3 and LK.get(info[0]) != "first_valu":
            w = w.astype(np.float16).astype(np.float32)          # pack_conv_weights / pack_convt_weights: fp16 weights
            if L.first:
                xin = xin.astype(np.float16).astype(np.float64)  # k_conv_first_mfma<false>: fp16 halo
        c64 = lr.layer64(L, xin, w, b)
        A = lr.abs_bound(L, xin, w, b).astype(np.float64)
        c = d["raw"].astype(np.float64)
        assert c.shape == c64.shape, (L.name, c.shape, c64.shape)
        K = L.K(sd)
        if prec == "fp16":
            bound = lr.TAU_FP16 * A + lr.FP16_STORE * np.abs(c64) + 2.0 ** -25
            r = np.abs(c - c64) / (A + (lr.FP16_STORE * np.abs(c64) + 2.0 ** -25) / lr.TAU_FP16)
            tau = lr.TAU_FP16
        else:
            tau = lr.tau_x3(K)
            bound = tau * A
            r = np.abs(c - c64) / A
        ok = bool((np.abs(c - c64) <= bound).all())
        at = np.unravel_index(int(np.argmax(r)), r.shape)   # where the worst err/A sits: channel, voxel
        row = {"tag": tag, "layer": L.name, "K": K, "kernel": LK.get(info[0], "?"), "R": info[1],
               "paired": info[2], "max": float(r.max()), "rms": float(np.sqrt(np.mean(r ** 2))), "tau": tau, "ok": ok,
               "conv_ok": ok, "stats_ok": True, "at": tuple(int(v) for v in at)}
        if L.normkey:
            ss64, mean, var = lr.norm_reference(d["raw"], sd[L.normkey + ".weight"], sd[L.normkey + ".bias"])
            row["ss"], row["sh"], row["mean/std"] = lr.ss_bars(d["raw"], d["ss"], ss64, mean, var, prec == "fp16")
            if row["ss"] > 1 or row["sh"] > 1:
                row["ok"] = row["stats_ok"] = ok = False
            if prec == "fp16" and not np.array_equal(d["ss16"], lr.ss16_pack(d["ss"])):
                row["ok"] = row["stats_ok"] = ok = False
                row["ss16"] = "MISMATCH"
        rows.append(row)
        if not ok:
            fails.append(row)


def _print(rows):
    print(f"\n{'case':<22}{'layer':<11}{'K':>6} {'kernel':<11}{'R':>2}{'pr':>3}{'max err/A':>11}{'rms err/A':>11}{'tau':>10}"
          f"{'ss/bar':>8}{'sh/bar':>8}{'mu/sd':>7}")
    for r in rows:
        print(f"{r['tag']:<22}{r['layer']:<11}{r['K']:>6} {r['kernel']:<11}{r['R']:>2}{r['paired']:>3}{r['max']:>11.3g}{r['rms']:>11.3g}"
              f"{r['tau']:>10.3g}{r.get('ss', float('nan')):>8.3g}{r.get('sh', float('nan')):>8.3g}{r.get('mean/std', float('nan')):>7.3g}"
              f"  at c{r['at'][0]} {r['at'][1:]}{'' if r['ok'] else '  FAIL'}{'  ss16 ' + r['ss16'] if 'ss16' in r else ''}")


def _case(ctx, tag, geom, sd, vol, origins, precs):
    rows, fails, cov = [], [], {}
    for prec, tiles in precs:
        got, cnt = _run(ctx, geom, sd, vol, origins, prec, tiles)
        cov[prec] = (got, cnt)
        for t, g in zip(tiles, got):
            _check(prec, geom, sd, _tile(vol, origins[t], geom.patch_size), g, f"{tag} {prec} t{t}", rows, fails)
    _print(rows)
    return rows, fails, cov


# ---- production geometry -----------------------------------------------------------------------------------------------------
def test_production_geometry_layer_parity(ctx):
    patch, features = (128, 128, 128), (32, 64, 128, 256, 320, 320)
    geom, sd = _model(patch, features, 25)
    rng = np.random.default_rng(11)
    vol = rng.standard_normal((1, 200, 150, 140)).astype(np.float32)
    origins = [[10, 5, 3], [100, 60, 40]]   # the second tile overhangs the volume on two axes
    rows, fails, cov = _case(ctx, "total", geom, sd, vol, origins, [("fp32", [0, 1]), ("fp16", [0])])
    assert not fails, fails
    got, cnt = cov["fp32"]
    kinds = {(LK[v["info"][0]], v["info"][1], v["info"][2]) for k, v in got[0].items() if "info" in v}
    names = {k[0] for k in kinds}
    assert names & {"first_mfma", "first_valu"}, kinds
    assert any(k[0] == "conv_ws" and k[1] >= 2 and k[2] == 1 for k in kinds), f"no tap-paired k_conv_ws<X3> (R >= 2): {kinds}"
    assert any(k[0] == "conv_ws" and k[1] == 1 for k in kinds), f"no R = 1 k_conv_ws<X3>: {kinds}"
    assert "conv_ns" in names and "convt_x3" in names and "head_x3" in names, kinds
    assert names <= {"first_mfma", "first_valu", "conv_ws", "conv_ns", "convt_x3", "head_x3"}, kinds
    # the output fold of the transposed convs (x3_output_fold) is 1 for these weights: the production net computes what it did before
    assert all(v["info"][2] == 0 for k, v in got[0].items() if k.startswith("up")), [(k, v["info"]) for k, v in got[0].items()]
    assert cnt["conv_simple"] == 0 and cnt["head_valu"] == 0 and cnt["f32"] == 0 and cnt["x3"] > 0 and cnt["conv_x3"] > 0, cnt


# ---- edges -------------------------------------------------------------------------------------------------------------------
BCA = dict(patch=(16, 64, 64), features=(32, 64, 128, 256), kernels=[[1, 3, 3], [1, 3, 3], [3, 3, 3], [3, 3, 3]],
           strides=[[1, 1, 1], [1, 2, 2], [1, 2, 2], [2, 2, 2]])
RAGGED = dict(patch=(16, 48, 40), features=(32, 64, 128, 256), kernels=[[1, 3, 3], [3, 3, 3], [3, 3, 3], [3, 3, 3]],
              strides=[[1, 1, 1], [1, 2, 2], [2, 2, 2], [2, 2, 2]])
SMALL = dict(patch=(32, 32, 32), features=(32, 64, 128))


def _edge_inputs(patch, seed=5):
    rng = np.random.default_rng(seed)
    vol = rng.standard_normal((1, patch[0] + 6, patch[1] + 5, patch[2] + 7)).astype(np.float32)
    return vol, [[0, 0, 0], [-3, 8, 10]]


@pytest.mark.parametrize("name,cfg", [("bca_1x3x3", BCA), ("ragged", RAGGED)])
def test_edge_geometries(ctx, name, cfg):
    geom, sd = _model(cfg["patch"], cfg["features"], 7, cfg.get("kernels"), cfg.get("strides"))
    vol, origins = _edge_inputs(cfg["patch"])
    rows, fails, cov = _case(ctx, name, geom, sd, vol, origins, [("fp32", [0, 1]), ("fp16", [0]), ("fp32_ref", [0])])
    assert not fails, fails
    if name == "bca_1x3x3":   # the K0 = 1 tap-paired loop (3 groups: one pair + the single last group) ran
        got, _ = cov["fp32"]
        assert any(LK[v["info"][0]] == "conv_ws" and v["info"][2] == 1 for k, v in got[0].items()
                   if "info" in v and k.startswith(("enc0", "enc1", "dec2"))), [(k, v["info"]) for k, v in got[0].items() if "info" in v]


@pytest.mark.parametrize("k", [6, 14])
def test_rescaled_pair(ctx, k):
    """up0 (weights and bias) x 2^-k and the up-channel half of dec0.conv0's weights x 2^k: the same function, with a transposed-conv
    output 2^-k as large -- the one raw (un-normalised) source of the stack.  Activations are split unscaled (x3_split4): below 2^-3
    the lo part is an fp16 subnormal, an absolute floor of 2^-25, which put dec0.conv0 at err/A 1.05e-4 for k = 14 (MI355X, bar
    9.5e-7).  Fixed at the cause: boa_net_load_weights folds a power of two g into the transposed conv (stored output g times the
    output) and 1 / g into the consumer's up-channel weights (x3_output_fold); the seam reports log2 g and takes it out again."""
    geom, sd = _model(SMALL["patch"], SMALL["features"], 5)
    sd = {kk: v.copy() for kk, v in sd.items()}
    sd["decoder.transpconvs.0.weight"] *= np.float32(2.0 ** -k)
    sd["decoder.transpconvs.0.bias"] = (sd["decoder.transpconvs.0.bias"] + np.float32(0.05)) * np.float32(2.0 ** -k)
    cup = sd["decoder.transpconvs.0.weight"].shape[1]
    sd["decoder.stages.0.convs.0.conv.weight"][:, :cup] *= np.float32(2.0 ** k)
    vol, origins = _edge_inputs(SMALL["patch"])
    rows, fails, cov = _case(ctx, f"rescaled k={k}", geom, sd, vol, origins, [("fp32", [0, 1])])
    assert not fails, fails
    fold = cov["fp32"][0][0]["up0"]["info"][2]
    assert abs(fold - k) <= 2, f"up0 output fold 2^{fold} for a 2^-{k} output"


# Two edges whose conv error (not their statistics) still exceeds the exact-mode bar: kept as strict xfails of the conv bar of the
# one layer they modify, while everything else of the same run -- every other layer's conv bar, the (scale, shift) of every layer
# including the modified one, the fp16 table -- must pass.  One GPU run per case, shared by the two tests.
_EDGE_RUNS = {}


def _channel_range_run(ctx, e):
    if ("chan", e) not in _EDGE_RUNS:
        geom, sd = _model(SMALL["patch"], SMALL["features"], 5)
        sd = {kk: v.copy() for kk, v in sd.items()}
        sd["encoder.stages.1.0.convs.1.conv.weight"][:4] *= np.float32(2.0 ** -e)
        vol, origins = _edge_inputs(SMALL["patch"])
        _EDGE_RUNS[("chan", e)] = _case(ctx, f"channels 2^-{e}", geom, sd, vol, origins, [("fp32", [0, 1])])[0]
    return _EDGE_RUNS[("chan", e)]


def _mean_offset_run(ctx):
    if "mean" not in _EDGE_RUNS:
        geom, sd = _model(SMALL["patch"], SMALL["features"], 5)
        sd = {kk: v.copy() for kk, v in sd.items()}
        for key in ("encoder.stages.1.0.convs.1.conv", "decoder.stages.0.convs.1.conv"):
            w = sd[key + ".weight"]
            std = np.sqrt((w.astype(np.float64) ** 2).reshape(w.shape[0], -1).sum(1) * 0.5)   # (inputs: lrelu of unit normals, E[y^2] ~ 1/2)
            sign = np.where(np.arange(w.shape[0]) % 2 == 0, 1.0, -1.0)
            sd[key + ".bias"] = (30.0 * std * sign).astype(np.float32)
        vol, origins = _edge_inputs(SMALL["patch"])
        _EDGE_RUNS["mean"] = _case(ctx, "mean offset", geom, sd, vol, origins, [("fp32", [0, 1]), ("fp16", [0])])[0]
    return _EDGE_RUNS["mean"]


def _all_but(rows, prec, layers):
    """Failures other than the conv bar of `layers` in precision `prec`."""
    return [r for r in rows if not r["stats_ok"] or (not r["conv_ok"] and not (f" {prec} " in r["tag"] and r["layer"] in layers))]


@pytest.mark.parametrize("e", [16, 24])
def test_channel_weight_range(ctx, e):
    """Output channels 0..3 of enc1.conv1 scaled by 2^-e relative to the rest: every check except enc1.conv1's conv bar passes."""
    rows = _channel_range_run(ctx, e)
    assert not _all_but(rows, "fp32", {"enc1.conv1"}), _all_but(rows, "fp32", {"enc1.conv1"})


@pytest.mark.xfail(strict=True, reason=(
    "open: x3_weight_scale is one power of two per layer.  enc1.conv1 measures err/A 1.8-2.0e-6 on MI355X at 2^-16 and 2^-24 (bar "
    "9.5e-7); the printed table gives the channel and voxel of the worst error.  Fix: one power-of-two weight scale per output "
    "channel, its inverse read next to the bias in the X3 epilogues (a kernel change)"))
@pytest.mark.parametrize("e", [16, 24])
def test_channel_weight_range_conv_bar(ctx, e):
    rows = _channel_range_run(ctx, e)
    bad = [r for r in rows if r["layer"] == "enc1.conv1" and not r["conv_ok"]]
    assert not bad, bad


def test_large_mean_offset(ctx):
    """Conv biases of ~30 standard deviations of the conv output on enc1.conv1 and dec0.conv1: E[c^2] - mean^2 in the statistics.
    The (scale, shift) bars, the fp16 table and every conv bar but the two biased layers' must pass."""
    rows = _mean_offset_run(ctx)
    assert max(r.get("mean/std", 0) for r in rows) > 15, "the offset did not reach the statistics"
    bad = _all_but(rows, "fp32", {"enc1.conv1", "dec0.conv1"})
    assert not bad, bad


@pytest.mark.xfail(strict=True, reason=(
    "open: the X3 accumulators start at bias * wscale, so with |bias| ~ 30 sigma each of the K / 16 fp32 MFMA accumulations rounds at "
    "the bias' magnitude: enc1.conv1 err/A 1.75e-6 on MI355X (bar 9.5e-7).  Fix: start from zero and add the bias in the epilogue "
    "(a kernel change)"))
def test_large_mean_offset_conv_bar(ctx):
    rows = _mean_offset_run(ctx)
    bad = [r for r in rows if " fp32 " in r["tag"] and r["layer"] in ("enc1.conv1", "dec0.conv1") and not r["conv_ok"]]
    assert not bad, bad
