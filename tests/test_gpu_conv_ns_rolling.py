"""k_conv_ns producers: fp64 parity of the stride-2 layers on the shapes a rolling commit / issue loop can get wrong.

The producer waves of k_conv_ns (csrc/conv_ns.hip) commit item j of chunk g + 1 to LDS and re-issue the load of item j of chunk g + 2
into the register that item leaves.  What such a loop can break is the bookkeeping between the chunk being committed and the chunk
in flight: the (scale, shift) words, the inside-the-tensor mask, the transform flag, the next tile's descriptor and addresses, and the
end of a workgroup's run, where nothing is issued.  Small synthetic nets (as tests/test_gpu_layer_parity.py builds them) put every
one of these on a few tiles:

  rm2  features (32, 64), patch (24, 20, 40): the 32 -> 64 stride-2 layer (k_conv_ns<2, 2, 2>) has a 12 x 10 x 20 output, a 3 x 3 x 3 tile
       grid ragged on two axes, and two chunks per tile -- every second interval issues across a tile boundary;
  rm4  features (32, 64, 128), patch (32, 40, 48): the second stride-2 layer is 64 -> 128 (k_conv_ns<2, 4, 4>) with an 8 x 10 x 12
       output and four chunks per tile.

Tiles: inside the volume, and overhanging it on two axes with a negative origin on the third (the zero padding switches the mask on
in some lanes of a chunk and not in others).  Batches N = 1, 3, 7: workgroup runs cross sample boundaries, so the (scale, shift) of
the chunk in flight belongs to another sample than the chunk being committed, and the last workgroup ends on a chunk with nothing
behind it.  Modes: fp16 and the exact mode (X3).

Every stride-2 layer's raw output and (scale, shift) are judged against the fp64 recomputation of tests/layer_reference.py from the
GPU's own inputs, with that file's bars unchanged; the layer info must name k_conv_ns.  The same tile at position 0 of N = 1 and at
the last position of N = 7 must give bit-identical raw output and (scale, shift) (a property of the kernel's batch-invariant tile
order; correctness is the fp64 bar, not this comparison)."""
import numpy as np
import pytest

import layer_reference as lr
import test_gpu_layer_parity as lp

pytestmark = pytest.mark.gpu

GEOMS = {"rm2": dict(patch=(24, 20, 40), features=(32, 64)), "rm4": dict(patch=(32, 40, 48), features=(32, 64, 128))}
INSIDE, INSIDE_B, INSIDE_C = [2, 3, 1], [6, 0, 7], [0, 5, 4]
EDGE, EDGE_B = [-3, 8, 10], [-1, 6, 9]           # (the volume is the patch + (6, 5, 7): _edge_inputs of the layer parity tests)
# origins of a batch, and the tiles judged against fp64
BATCHES = {1: ([INSIDE], [0]),
           3: ([INSIDE, EDGE, INSIDE_B], [0, 1, 2]),
           7: ([EDGE, INSIDE_B, EDGE_B, INSIDE_C, EDGE, INSIDE_B, INSIDE], [0, 6])}
CONV_NS = 4   # layer info: the kernel that ran (test_gpu_layer_parity.LK)


@pytest.fixture(scope="module")
def ctx():
    import torch
    from boa_hip.device import Context
    torch.set_num_threads(16)
    c = Context(0)
    yield c
    c.close()


_MODELS, _RUNS = {}, {}


def _model(name):
    if name not in _MODELS:
        cfg = GEOMS[name]
        geom, sd = lp._model(cfg["patch"], cfg["features"], 5)
        vol = np.random.default_rng(17).standard_normal((1, cfg["patch"][0] + 6, cfg["patch"][1] + 5, cfg["patch"][2] + 7)).astype(np.float32)
        walk = lr.layer_walk(geom)
        s2 = [L for L in walk if L.kind == 0 and tuple(L.stride) == (2, 2, 2)]
        assert len(s2) == len(cfg["features"]) - 1
        _MODELS[name] = (geom, sd, vol, {L.name: L for L in walk}, s2)
    return _MODELS[name]


def _run(ctx, name, prec, n):
    """One forward of batch n; per judged tile: the stride-2 layers and their sources as the GPU stored them."""
    if (name, prec, n) not in _RUNS:
        from boa_hip import plans
        from boa_hip.predictor import HipPredictor
        geom, sd, vol, layers, s2 = _model(name)
        origins, tiles = BATCHES[n]
        p = HipPredictor(ctx, geom, max_batch=len(origins), precision=prec)
        assert p.precision == prec, "no silent fall-back to another precision"
        p.set_parameters([plans.weight_blob_from_state_dict(geom, sd)])
        p.network_forward(vol, np.asarray(origins, dtype=np.int32))
        need = {nm for L in s2 for nm in [L.name] + L.sources}
        got = {t: {nm: lp._read(ctx, p, layers[nm], t, prec == "fp16") for nm in need} for t in tiles}
        p.close()
        _RUNS[(name, prec, n)] = got
    return _RUNS[(name, prec, n)]


def _judge(prec, sd, layers, L, got, tag):
    """lp._check for one layer: the conv error against tau * A and the (scale, shift) against the fp64 statistics."""
    d = got[L.name]
    assert d["info"][0] == CONV_NS, f"{tag} {L.name}: kernel {lp.LK.get(d['info'][0])}, not k_conv_ns"
    xin = np.concatenate([lp._consumer_input(prec, layers, L, s, got[s], d["info"]) for s in L.sources], 0)
    w, b = sd[L.wkey + ".weight"].astype(np.float32), sd[L.wkey + ".bias"].astype(np.float32)
    if prec == "fp16":
        w = w.astype(np.float16).astype(np.float32)
    c64 = lr.layer64(L, xin, w, b)
    A = lr.abs_bound(L, xin, w, b).astype(np.float64)
    c = d["raw"].astype(np.float64)
    assert c.shape == c64.shape, (L.name, c.shape, c64.shape)
    if prec == "fp16":
        bound = lr.TAU_FP16 * A + lr.FP16_STORE * np.abs(c64) + 2.0 ** -25
    else:
        bound = lr.tau_x3(L.K(sd)) * A
    worst = float((np.abs(c - c64) / bound).max())
    ss64, mean, var = lr.norm_reference(d["raw"], sd[L.normkey + ".weight"], sd[L.normkey + ".bias"])
    ssb, shb, _ = lr.ss_bars(d["raw"], d["ss"], ss64, mean, var, prec == "fp16")
    print(f"{tag:<22}{L.name:<11} K {L.K(sd):>5}  err/bar {worst:.3g}  ss/bar {ssb:.3g}  sh/bar {shb:.3g}")
    assert worst <= 1, f"{tag} {L.name}: conv error {worst:.3g} x its bar"
    assert ssb <= 1 and shb <= 1, f"{tag} {L.name}: (scale, shift) at {ssb:.3g} / {shb:.3g} of their bars"
    if prec == "fp16":
        assert np.array_equal(d["ss16"], lr.ss16_pack(d["ss"])), f"{tag} {L.name}: packed fp16 (scale, shift) table"


@pytest.mark.parametrize("n", [1, 3, 7])
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("name", ["rm2", "rm4"])
def test_stride2_layers_fp64(ctx, name, prec, n):
    geom, sd, vol, layers, s2 = _model(name)
    got = _run(ctx, name, prec, n)
    for t in BATCHES[n][1]:
        for L in s2:
            _judge(prec, sd, layers, L, got[t], f"{name} {prec} N={n} t{t}")


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("name", ["rm2", "rm4"])
def test_same_tile_first_of_1_last_of_7(ctx, name, prec):
    geom, sd, vol, layers, s2 = _model(name)
    assert BATCHES[1][0][0] == BATCHES[7][0][6]
    a, b = _run(ctx, name, prec, 1)[0], _run(ctx, name, prec, 7)[6]
    for L in s2:
        assert a[L.name]["info"][0] == CONV_NS and b[L.name]["info"][0] == CONV_NS
        assert np.array_equal(a[L.name]["raw"].view(np.uint32), b[L.name]["raw"].view(np.uint32)), f"{name} {prec} {L.name}: raw output"
        assert np.array_equal(a[L.name]["ss"].view(np.uint32), b[L.name]["ss"].view(np.uint32)), f"{name} {prec} {L.name}: (scale, shift)"
        if prec == "fp16":
            assert np.array_equal(a[L.name]["ss16"], b[L.name]["ss16"]), f"{name} {prec} {L.name}: packed (scale, shift)"
