"""The fp64 per-layer reference (tests/layer_reference.py) checked on the host, before any GPU is involved:
  * the z-slab fp64 conv equals one unslabbed torch fp64 conv (strides 1 / 2, kernels 3x3x3 / 1x3x3, ragged dims);
  * the layer walk, with its fp64 ops and InstanceNorm, reproduces every intermediate tensor of oracle.network (the fp32 torch
    PlainConvUNet) to fp32 precision: concat order, transposed-conv weight layout, padding and head are the oracle's;
  * the numpy model of the split-precision product stays under the exact-mode bar at the stack's K, and every mutant (a missing
    cross term, hi parts only, one lost 8-channel K-step) exceeds it at least 10x: the bar tests/test_gpu_layer_parity.py applies
    can see such a kernel bug;
  * the input transforms of the consumers are bit-exact against an exact-rational model on hand-picked cases (negative, fp16
    subnormal, overflow to inf, ties, an fp32 fma whose exact sum lies just off a rounding midpoint)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import layer_reference as lr


def _rng(seed=0):
    return np.random.default_rng(seed)


@pytest.mark.parametrize("shape,cin,cout,k,s", [
    ((9, 7, 11), 8, 16, (3, 3, 3), (1, 1, 1)),
    ((10, 9, 13), 8, 16, (3, 3, 3), (2, 2, 2)),
    ((5, 12, 10), 16, 8, (1, 3, 3), (1, 2, 2)),
    ((7, 6, 5), 4, 8, (3, 3, 3), (2, 1, 2)),
])
def test_slab_conv_equals_unslabbed(shape, cin, cout, k, s):
    rng = _rng(1)
    x = rng.standard_normal((cin,) + shape)
    w = rng.standard_normal((cout, cin) + k)
    b = rng.standard_normal(cout)
    pad = [(kk - 1) // 2 for kk in k]
    with torch.inference_mode():
        ref = torch.nn.functional.conv3d(torch.from_numpy(x)[None], torch.from_numpy(w), torch.from_numpy(b), s, pad)[0].numpy()
    # a budget that forces one output row per slab, and the default (one slab)
    for budget in (1.0, 1e9):
        got = lr.conv3d64(x, w, b, s, budget=budget)
        assert got.shape == ref.shape
        np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-12)


def _oracle_and_walk(patch, features, kernels=None, strides=None, classes=5, seed=3):
    from boa_hip import plans
    from oracle.network import build_from_arch
    pj, dj = plans.synthetic_plans(patch=patch, features=features, num_classes=classes, kernels=kernels, strides=strides)
    cfg = plans.model_config_from_plans(pj, dj)
    sd = plans.synthetic_state_dict(cfg.geometry, seed)
    net = build_from_arch(pj["configurations"]["3d_fullres"]["architecture"]["arch_kwargs"], 1, classes)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return cfg.geometry, sd, net.eval()


@pytest.mark.parametrize("patch,features,kernels,strides", [
    ((16, 16, 16), (32, 64, 128), None, None),
    ((8, 24, 20), (32, 64, 128), [[1, 3, 3], [3, 3, 3], [3, 3, 3]], [[1, 1, 1], [1, 2, 2], [2, 2, 2]]),
])
def test_walk_reproduces_oracle_activations(patch, features, kernels, strides):
    geom, sd, net = _oracle_and_walk(patch, features, kernels, strides)
    seen = {}

    def hook(name):
        def f(_m, _i, out):
            seen[name] = out.detach().numpy()[0].copy()
        return f

    for s, st in enumerate(net.encoder.stages):
        for i, blk in enumerate(st[0].convs):
            blk.conv.register_forward_hook(hook(f"enc{s}.conv{i}"))
            blk.register_forward_hook(hook(f"enc{s}.conv{i}.act"))
    for k, up in enumerate(net.decoder.transpconvs):
        up.register_forward_hook(hook(f"up{k}"))
    for k, st in enumerate(net.decoder.stages):
        for i, blk in enumerate(st.convs):
            blk.conv.register_forward_hook(hook(f"dec{k}.conv{i}"))
            blk.register_forward_hook(hook(f"dec{k}.conv{i}.act"))
    net.decoder.seg_layers[-1].register_forward_hook(hook("head"))
    x = _rng(7).standard_normal((1,) + tuple(patch)).astype(np.float32)
    with torch.inference_mode():
        net(torch.from_numpy(x)[None])
    walk = lr.layer_walk(geom)
    assert {L.name for L in walk} == {n for n in seen if not n.endswith(".act")}
    acts = {"input": x.astype(np.float64)}
    for L in walk:
        xin = np.concatenate([acts[s] for s in L.sources], 0)
        w, b = sd[L.wkey + ".weight"], sd[L.wkey + ".bias"]
        raw = lr.layer64(L, xin, w, b)
        ref = seen[L.name]
        A = lr.abs_bound(L, xin, w, b)
        assert raw.shape == ref.shape, L.name
        err = float((np.abs(raw - ref) / A).max())
        assert err < 1e-6, (L.name, err)    # fp32 (oneDNN) against fp64 on the same inputs: a few ulp of A, nothing structural
        if L.normkey:   # InstanceNorm + LeakyReLU from the fp64 statistics of the oracle's own raw output
            ss, _, _ = lr.norm_reference(ref, sd[L.normkey + ".weight"], sd[L.normkey + ".bias"])
            y = ref * ss[:, 0].reshape(-1, 1, 1, 1) + ss[:, 1].reshape(-1, 1, 1, 1)
            y = np.where(y > 0, y, 0.01 * y)
            aref = seen[L.name + ".act"]
            assert float(np.abs(y - aref).max()) < 1e-5 * max(1.0, float(np.abs(aref).max())), L.name
            acts[L.name] = aref.astype(np.float64)   # (the next layer reads the oracle's activation: every layer is checked alone)
        else:
            acts[L.name] = ref.astype(np.float64)
    # every weight of the state dict that the forward uses was used by the walk
    used = {L.wkey + ".weight" for L in walk}
    assert {k for k in sd if k.endswith("conv.weight") or k.startswith("decoder.transpconvs") and k.endswith("weight")} <= used


# ---- the split-precision product model ----------------------------------------------------------------------------------------
def _emu_case(cin, taps, seed=0, cout=64, J=256):
    rng = _rng(seed)
    K = cin * taps
    w = (rng.standard_normal((cout, K)) * np.sqrt(2.0 / K)).astype(np.float32)
    x = lr.lrelu32(rng.standard_normal((K, J)).astype(np.float32))
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    ref = w.astype(np.float64) @ x.astype(np.float64) + b.astype(np.float64)[:, None]
    A = np.abs(w).astype(np.float64) @ np.abs(x).astype(np.float64) + np.abs(b).astype(np.float64)[:, None]
    return w, x, b, ref, A


# K = 24 * 9 (a BCA-style 1x3x3 stage with 24 channels), 864 (32 x 27), 8640 (320 x 27), 17280 (the 640-channel decoder conv0)
EMU_K = [(24, 9), (32, 27), (320, 27), (640, 27)]


@pytest.mark.parametrize("cin,taps", EMU_K)
def test_x3_model_within_bar(cin, taps):
    w, x, b, ref, A = _emu_case(cin, taps)
    got = lr.x3_dot_emulate(w, x, b, taps=taps)
    r = float((np.abs(got - ref) / A).max())
    print(f"K={cin * taps}: x3 model max err/A {r:.3g}, bar {lr.tau_x3(cin * taps):.3g}")
    assert r <= lr.tau_x3(cin * taps)
    assert lr.tau_x3(cin * taps) <= lr.tau_x3_ceiling(cin * taps)


# (the lost K-step at the largest K only: there one octet is the smallest share of the sum)
@pytest.mark.parametrize("cin,taps,mutant", [ct + (m,) for m in ("no_WhXl", "no_WlXh", "hi_only") for ct in EMU_K]
                         + [EMU_K[-1] + ("drop_octet",)])
def test_x3_mutants_exceed_bar(cin, taps, mutant):
    w, x, b, ref, A = _emu_case(cin, taps)
    kw = {"no_WhXl": dict(terms=("hh", "lh")), "no_WlXh": dict(terms=("hh", "hl")), "hi_only": dict(terms=("hh",)),
          "drop_octet": dict(drop_octet=(taps // 2, cin // 16))}[mutant]
    got = lr.x3_dot_emulate(w, x, b, taps=taps, **kw)
    r = float((np.abs(got - ref) / A).max())
    print(f"K={cin * taps} {mutant}: max err/A {r:.3g} = {r / lr.tau_x3(cin * taps):.0f} x the bar")
    assert r >= 10 * lr.tau_x3(cin * taps)


def test_x3_weight_scale_matches_packer_rule():
    for m in (1e-3, 0.37, 1.0, 3.0, 1e4):
        w = np.array([m, -m / 3], np.float32)
        sc = lr.x3_weight_scale(w)
        assert 2 ** 13 <= m * sc < 2 ** 14
    assert lr.x3_weight_scale(np.zeros(4, np.float32)) == 1.0


# ---- input transforms, bit-exact against exact rationals --------------------------------------------------------------------
def _round_rational(q: Fraction, mant_bits: int, emin: int, emax: int) -> float:
    """Round-to-nearest-even of an exact rational into a binary format with `mant_bits` fraction bits (subnormals below 2^emin,
    overflow to inf above the largest finite)."""
    if q == 0:
        return 0.0
    sign = -1 if q < 0 else 1
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, emin)
    ulp = Fraction(2) ** (e - mant_bits)
    n, rem = divmod(a, ulp)
    if rem > ulp / 2 or (rem == ulp / 2 and n % 2 == 1):
        n += 1
    v = n * ulp
    if v >= Fraction(2) ** (emax + 1):
        return sign * float("inf")
    return sign * float(v)


def _f16(q):
    return _round_rational(Fraction(q), 10, -14, 15)


def _f32(q):
    return _round_rational(Fraction(q), 23, -126, 127)


def _pk_model(x, s, t, slope=0.01):
    y = _f16(Fraction(float(x)) * Fraction(float(s)) + Fraction(float(t)))
    if np.isinf(y):
        z = y
    else:
        z = _f16(Fraction(y) * Fraction(float(np.float16(np.float32(slope)))))
    return max(y, z)


PK_CASES = [
    (-2.0, 1.0, 0.0),                       # negative: the slope branch, y * half(0.01)
    (-2.0 ** -10, 1.0, 0.0),                # negative, slope product in the fp16 subnormal range
    (2.0 ** -14, 0.5, 0.0),                 # positive subnormal result
    (2.0 ** -24, 1.0, 0.0),                 # smallest subnormal passes through
    (60000.0, 2.0, 0.0),                    # overflow to +inf
    (-60000.0, 2.0, 0.0),                   # overflow to -inf (slope branch of -inf stays -inf)
    (1 + 2 ** -5, 1 + 2 ** -6, 0.0),        # exact product on an fp16 midpoint: ties to even (down)
    (1 + 2 ** -5, 1 + 2 ** -6, 2.0 ** -20), # the same midpoint plus a subnormal addend: rounds up (one rounding, not two)
    (1 + 2 ** -5, 1 + 2 ** -6, -2.0 ** -24),
    (3.0, -0.75, 2.25),                     # exact zero
    (1000.0, 0.0999755859375, -99.9375),    # cancellation
]


@pytest.mark.parametrize("x,s,t", PK_CASES)
def test_norm_act8_pk_bit_exact(x, s, t):
    raw = np.array([[x]], np.float16)
    ss16 = np.array([[s, t]], np.float16)
    got = lr.norm_act8_pk(raw, ss16)[0, 0]
    want = np.float16(_pk_model(np.float16(x), np.float16(s), np.float16(t)))
    assert got.view(np.uint16) == want.view(np.uint16) or (got == 0 and want == 0), (got, want)


F32_CASES = [
    (1 + 2 ** -12, 1 + 2 ** -12, 0.0),          # product 1 + 2^-11 + 2^-24: an fp32 midpoint, ties to even
    (1 + 2 ** -12, 1 + 2 ** -12, 2.0 ** -80),   # just above the midpoint: a sum in fp64 would lose the addend, fmaf rounds up
    (1 + 2 ** -12, 1 + 2 ** -12, -2.0 ** -80),
    (-3.5, 0.3, 0.5),                           # negative: the slope branch
    (1e-20, 1e-20, 0.0),                        # underflow to an fp32 subnormal / zero
    (3e38, 2.0, 0.0),                           # overflow
]


@pytest.mark.parametrize("x,s,t", F32_CASES)
def test_norm_act_x3_bit_exact(x, s, t):
    raw = np.array([[x]], np.float32)
    ss = np.array([[s, t]], np.float32)
    got = lr.norm_act_x3(raw, ss)[0, 0]
    f = _f32(Fraction(float(np.float32(x))) * Fraction(float(np.float32(s))) + Fraction(float(np.float32(t))))
    want = np.float32(f if f > 0 else (_f32(Fraction(f) * Fraction(float(np.float32(0.01)))) if np.isfinite(f) else f))
    assert got.view(np.uint32) == want.view(np.uint32) or (got == 0 and want == 0), (got, want)


def test_norm_act8_matches_pk_only_where_it_should():
    # the fp32-table form rounds once at the end; the packed form rounds (scale, shift) to fp16 first: they differ in general
    rng = _rng(4)
    raw = rng.standard_normal((8, 64)).astype(np.float16)
    ss = np.stack([rng.uniform(0.5, 2, 8), rng.uniform(-1, 1, 8)], 1).astype(np.float32)
    a = lr.norm_act8(raw, ss)
    b = lr.norm_act8_pk(raw, ss.astype(np.float16))
    assert a.dtype == b.dtype == np.float16
    assert np.abs(a.astype(np.float32) - b.astype(np.float32)).max() <= 4 * 2.0 ** -11 * np.abs(a.astype(np.float32)).max()


def test_ss16_pack_roundtrip():
    ss = np.array([[1.5, -0.25], [3e-6, 7.0], [70000.0, 1e-9], [-2.0, 0.1]], np.float32)
    words = lr.ss16_pack(ss)
    assert words.dtype == np.uint16 and words.shape == (8,)
    back = lr.ss16_unpack(words)
    np.testing.assert_array_equal(back.view(np.uint16), ss.astype(np.float16).view(np.uint16))
    # layout: {s_c, s_c+1, t_c, t_c+1} per channel pair
    assert words[1] == np.float16(3e-6).view(np.uint16) and words[2] == np.float16(-0.25).view(np.uint16)
