"""The last layer's FALLBACK kernels, one launch form at a time (cases and references: tests/head_cases.py, proven on the CPU by
tests/test_head_cases_cpu.py):

  k_head<32,2>, k_head<32,1>, k_head<64,1>      fp16 mode off the matrix cores (more than 31 classes, P2 % 32 != 0, features[0] == 64),
  k_head_mfma<logits> + k_accumulate_tile       the MFMA logits with accumulators that are not 8-voxel aligned,      -> boa_head_tile
  k_head_x3, k_head_f32 (records / octet planes) the fp32-input heads                                                 -> boa_head_tile_f32
  and the class counts 31 / 32 / 33, at which the predictor changes heads.

Every case asserts
  (a) the logits-mode output against head64 (float64 on the exact inputs): |err| <= (F0 + 4) 2^-24 A for the fp32 fma chains (k_head,
      k_head_f32; A = sum |w| |y| + |b|; F0 + 1 terms, inputs with two roundings, one unit for second-order terms: derived, no margin),
      layer_reference.tau_x3(32) A for k_head_x3 (the project's measured bar of that kernel);
  (b) the accumulate seam bit for bit: three or more overlapping tiles, each with its own activation and (scale, shift), the last one flush
      against the far corner, with and without the Gaussian: accumulators and weight plane equal oracle.sliding_window.accumulate_tile on
      the tiles' logits-mode output (both modes of a kernel run the same fma chain per element);
  (c) containment: the accumulators lie between sentinel runs that must come back untouched;
and, from the launch counters, that the form the case is named for is the one that ran.
(The k_head_mfma<logits> + k_accumulate_tile case takes (b) and (c) only: that kernel rounds weights and (scale, shift) to fp16, its logit
values have their own bar in tests/test_gpu_head.py.)

Measured on MI355X, the largest err / A of each form over its cases, next to the bound it is held to (a record; the bound is the derived one):
  k_head<32,2>                 3.7e-7   (F0 + 4) 2^-24 = 2.15e-6
  k_head<32,1>                 2.8e-7   2.15e-6
  k_head<64,1>                 3.5e-7   4.05e-6          (3.5e-7 at 255 classes as well)
  k_head_f32, F0 = 8 / 32 / 64 2.8e-7 / 4.3e-7 / 4.1e-7   7.2e-7 / 2.15e-6 / 4.05e-6   (records and octet planes give identical logits)
  k_head_x3                    2.8e-7   tau_x3(32) = 9.5e-7
  k_head_mfma<logits>          6.1e-4   (fp16 weights and norm: not held to a bar here)
"""
import ctypes as C

import numpy as np
import pytest

import head_cases as hc
import layer_reference as lr

pytestmark = pytest.mark.gpu

KIND = {"x3": 12, "f32cl": 13, "f32oct": 13}       # BOA_LK_HEAD_X3 / BOA_LK_HEAD_F32


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


def _i3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


def _launch(ctx, case, d_act, stride, d_ss, d_w, d_b, logits=None, gauss=None, acc=None, n=None, start=None):
    from boa_hip._lib import check
    vp = lambda b: b.vp if b is not None else None
    tail = (_i3(case.P), case.C, d_w.vp, d_b.vp, hc.SLOPE, vp(logits), vp(gauss), vp(acc), vp(n),
            _i3(case.PV) if acc is not None else None, _i3(start) if acc is not None else None)
    if case.kind == "fp16":
        check(ctx.lib.boa_head_tile(ctx.h, d_act.vp, d_ss.vp, case.F0, *tail), "boa_head_tile")
    else:
        check(ctx.lib.boa_head_tile_f32(ctx.h, KIND[case.kind], d_act.vp, stride, d_ss.vp, case.F0, *tail), "boa_head_tile_f32")


def _expect_counters(case, form, cnt, launches):
    """the launch counters after `launches` launches of `form`"""
    want = dict(head_mfma=0, head_valu=0, x3=0, f32=0)
    if case.kind == "fp16":
        want["head_mfma" if form.startswith("k_head_mfma") else "head_valu"] = launches
    else:
        want["f32" if case.kind == "f32cl" else "x3"] = launches     # launch_head_f32 counts its octet layout with the split-precision kernels
    got = {k: cnt[k] for k in want}
    assert got == want and cnt["head_gather"] == 0, (case.name, form, cnt)


def _bound(case):
    return lr.tau_x3(32) if case.kind == "x3" else hc.logit_bound(case.F0)


def run_case(ctx, case):
    from boa_hip.device import BufferView
    w, b, tiles = hc.head_inputs(case)
    d_w, d_b = ctx.from_numpy(w), ctx.from_numpy(b)
    bufs = [d_w, d_b]
    dev = []
    for act, ss in tiles:
        packed, stride = hc.pack_act(case, act)
        dev.append((ctx.from_numpy(packed), stride, ctx.from_numpy(ss)))
        bufs += list(dev[-1][::2])
    try:
        # ---- logits mode, (a) --------------------------------------------------------------------------------------------------
        d_out = ctx.alloc(case.C * case.pv * 4)
        bufs.append(d_out)
        ctx.counters(reset=True)
        L, worst = [], 0.0
        for (d_act, stride, d_ss), (act, ss) in zip(dev, tiles):
            assert d_act.ptr % 256 == 0 and d_out.ptr % 256 == 0
            _launch(ctx, case, d_act, stride, d_ss, d_w, d_b, logits=d_out)
            L.append(d_out.download((case.C, *case.P), np.float32).copy())
            want, A = hc.head64(act, ss, w, b)
            assert np.isfinite(L[-1]).all() and (A > 0).all()
            worst = max(worst, float((np.abs(L[-1] - want) / A).max()))
        _expect_counters(case, case.logits_form, ctx.counters(), len(tiles))
        print(f"{case.name}: logits by {case.logits_form}, accumulate by {sorted(set(case.forms))}: max err/A {worst:.3g} (bound {_bound(case):.3g})")
        if not case.logits_form.startswith("k_head_mfma"):
            assert worst <= _bound(case), (case.name, worst, _bound(case))
        # ---- accumulate mode, (b) and (c) ----------------------------------------------------------------------------------------
        nv = int(np.prod(case.PV))
        for g16 in (None, hc.gaussian(case.P)):
            acc0, n0 = hc.initial_accumulators(case)
            G = hc.GUARD
            h_acc = np.concatenate([hc.sentinel(G, 1), acc0.view(np.uint16).reshape(-1), hc.sentinel(G, 2)])
            h_n = np.concatenate([hc.sentinel(G, 3), n0.view(np.uint16).reshape(-1), hc.sentinel(G, 4)])
            d_acc, d_n = ctx.from_numpy(h_acc), ctx.from_numpy(h_n)
            d_g = ctx.from_numpy(g16.view(np.uint16)) if g16 is not None else None
            assert d_acc.ptr % 256 == 0 and d_n.ptr % 256 == 0 and (d_g is None or d_g.ptr % 256 == 0)
            acc_v, n_v = BufferView(d_acc, 2 * G, case.C * nv * 2), BufferView(d_n, 2 * G, nv * 2)
            o_acc, o_n = acc0.copy(), n0.copy()
            try:
                for (d_act, stride, d_ss), s, form, Lt in zip(dev, case.starts, case.forms, L):
                    ctx.counters(reset=True)
                    _launch(ctx, case, d_act, stride, d_ss, d_w, d_b, gauss=d_g, acc=acc_v, n=n_v, start=s)
                    _expect_counters(case, form, ctx.counters(), 1)
                    hc.accumulate_tile(o_acc, o_n, Lt, g16, s)
                ctx.sync()
                got_acc, got_n = d_acc.download(h_acc.shape, np.uint16), d_n.download(h_n.shape, np.uint16)
            finally:
                for bf in (d_acc, d_n, d_g):
                    if bf is not None:
                        bf.free()
            tag = f"{case.name} {'gaussian' if g16 is not None else 'weight 1'}"
            np.testing.assert_array_equal(got_n[G:-G].reshape(case.PV), o_n.view(np.uint16), err_msg=tag + ": weight plane")
            np.testing.assert_array_equal(hc.canon_nan(got_acc[G:-G].reshape(case.C, *case.PV)), hc.canon_nan(o_acc.view(np.uint16)),
                                          err_msg=tag + ": accumulators")
            for got, host in ((got_acc, h_acc), (got_n, h_n)):                  # (c)
                np.testing.assert_array_equal(got[:G], host[:G], err_msg=tag + ": wrote in front of the buffer")
                np.testing.assert_array_equal(got[-G:], host[-G:], err_msg=tag + ": wrote behind the buffer")
            if case.scale > 1:
                f = o_acc.astype(np.float32)
                assert np.isinf(f).any() == (g16 is not None) and np.abs(f[np.isfinite(f)]).max() > 16384, tag
    finally:
        for bf in bufs:
            bf.free()
    return worst


@pytest.mark.parametrize("case", hc.fp16_cases(), ids=lambda c: c.name)
def test_fp16_fallback_heads(ctx, case):
    """k_head<32,2>, k_head<32,1>, k_head<64,1> and the MFMA logits + k_accumulate_tile through boa_head_tile.  `f64-C255-lds` asks for
    66812 bytes of LDS: launch_head raises k_head<64,1>'s limit above the default 64 KiB for it."""
    run_case(ctx, case)


@pytest.mark.parametrize("case", hc.x3_cases(), ids=lambda c: c.name)
def test_head_x3(ctx, case):
    """k_head_x3 up to C = 32 (all 32 D rows live), whole and partial waves and blocks, plane stride == and != the tile's voxel count."""
    run_case(ctx, case)


@pytest.mark.parametrize("case", hc.f32_cases(), ids=lambda c: c.name)
def test_head_f32(ctx, case):
    """k_head_f32: channels-last records and octet planes, F0 8 / 32 / 64, up to 118 classes."""
    run_case(ctx, case)


def test_head_refuses_what_does_not_fit_lds(ctx):
    """A class count whose weights exceed the LDS of a compute unit is refused with a message that names F0 and C, before any launch."""
    case = hc.HeadCase("too-large", "fp16", 64, 700, (2, 3, 5), (2, 3, 5), ((0, 0, 0),), ("k_head<64,1>",), "k_head<64,1>")
    assert hc.head_lds_bytes(64, 700) > 160 * 1024
    w, b, tiles = hc.head_inputs(case)
    bufs = [ctx.from_numpy(w), ctx.from_numpy(b), ctx.from_numpy(hc.planar16(tiles[0][0])), ctx.from_numpy(tiles[0][1]),
            ctx.alloc(case.C * case.pv * 4)]
    ctx.counters(reset=True)
    with pytest.raises(ValueError, match=r"features\[0\]=64 with 700 classes"):
        _launch(ctx, case, bufs[2], 0, bufs[3], bufs[0], bufs[1], logits=bufs[4])
    cnt = ctx.counters()
    assert cnt["head_valu"] == 0 and cnt["head_mfma"] == 0
    ctx.sync()
    for bf in bufs:
        bf.free()


# ---- class-count boundaries through the predictor ------------------------------------------------------------------------------------
def _head_kernel(p):
    """BOA_LK_* code of the scatter head of a predictor's network (boa_net_debug_layer, kind 3)."""
    from boa_hip._lib import check
    ch, dims, info = C.c_int(), (C.c_int * 3)(), (C.c_int * 3)()
    check(p.lib.boa_net_debug_layer(p._net, 3, 0, 0, 0, None, None, None, C.byref(ch), dims, info), "boa_net_debug_layer")
    return int(info[0])


def _boundary_case(ctx, patch, nc, precision):
    from boa_hip import plans, sliding_window as sw
    from boa_hip.predictor import HipPredictor
    from oracle import labels as olab
    from oracle import sliding_window as osw
    shape, step = (40, 36, 64), 0.5
    pj, dj = plans.synthetic_plans(patch=patch, features=(32, 64), num_classes=nc)
    geom = plans.model_config_from_plans(pj, dj).geometry
    p = HipPredictor(ctx, geom, tile_step_size=step, max_batch=3, precision=precision)
    p.set_parameters([plans.weight_blob_from_state_dict(geom, plans.synthetic_state_dict(geom, 7))])
    assert p.precision == precision
    x = np.random.default_rng(nc).standard_normal((1, *shape)).astype(np.float32)
    origins = np.asarray(sw.get_sliding_window_origins(list(shape), list(patch), step), dtype=np.int32)
    ctx.counters(reset=True)
    labels = p.predict_segmentation(x)
    c_lab = ctx.counters(reset=True)
    logits = p.predict_sliding_window_return_logits(x)
    c_log = ctx.counters(reset=True)
    kernel = _head_kernel(p)
    tiles = p.network_forward(x, origins)
    p.close()
    g = osw.compute_gaussian(tuple(patch), 1. / 8, 10)
    acc, n = np.zeros((nc, *shape), np.float16), np.zeros(shape, np.float16)
    for t, o in enumerate(origins):
        osw.accumulate_tile(acc, n, tiles[t], g, tuple(int(v) for v in o))
    want = osw.finalize_logits(acc, n)
    assert logits.dtype == np.float16 and len(np.unique(olab.argmax_labels(want))) >= 3
    np.testing.assert_array_equal(logits.view(np.uint16), want.view(np.uint16))
    np.testing.assert_array_equal(labels, olab.argmax_labels(want))
    return c_lab, c_log, kernel, len(origins)


@pytest.mark.parametrize("precision", ["fp16", "fp32", "fp32_ref"])
@pytest.mark.parametrize("nc", [31, 32, 33])
def test_class_count_boundaries(ctx, nc, precision):
    """31 / 32 / 33 classes flip the head between the matrix cores and the VALU, the gather and the scatter form, k_head_x3 and
    k_head_f32.  On either side the labels are the argmax, and the logits API's fp16 logits the quotient, of the oracle's tile loop over
    the device's own per-tile logits, bit for bit; the counters say which head ran:
               nc = 31      nc = 32             nc = 33
      fp16     gather       VALU scatter        VALU scatter
      fp32     gather (x3)  k_head_x3 scatter   k_head_f32 (octet planes)
      fp32_ref k_head_f32   k_head_f32          k_head_f32"""
    c_lab, c_log, kernel, nt = _boundary_case(ctx, (32, 32, 32), nc, precision)
    gather = precision != "fp32_ref" and nc == 31
    assert (c_lab["head_gather"] > 0) == gather and c_log["head_gather"] == 0, (c_lab, c_log)
    if precision == "fp16":
        assert kernel == 14
        assert c_lab["head_mfma"] == 0 and c_lab["head_valu"] == (0 if gather else nt), c_lab
        assert (c_log["head_mfma"], c_log["head_valu"]) == ((nt, 0) if nc == 31 else (0, nt)), c_log
        assert c_lab["x3"] == c_lab["f32"] == 0
    elif precision == "fp32":
        assert kernel == (12 if nc <= 32 else 13)
        for c in (c_lab, c_log):
            assert c["head_mfma"] == c["head_valu"] == c["f32"] == 0 and c["conv_x3"] > 0, c
        assert c_log["x3"] >= nt                                                      # the scatter loop's heads count with the x3 kernels
    else:
        assert kernel == 13
        for c in (c_lab, c_log):
            assert c["head_mfma"] == c["head_valu"] == c["x3"] == c["conv_x3"] == 0 and c["f32"] >= nt, c


def test_valu_head_through_the_patch_shape(ctx):
    """patch z = 48: P2 % 32 != 0 takes a 5-class fp16 network off the matrix cores (and off the gather form): k_head<32,2> per tile."""
    c_lab, c_log, kernel, nt = _boundary_case(ctx, (32, 32, 48), 5, "fp16")
    assert kernel == 14
    for c in (c_lab, c_log):
        assert c["head_gather"] == 0 and c["head_mfma"] == 0 and c["head_valu"] == nt, c
