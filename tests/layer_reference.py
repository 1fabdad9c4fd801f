"""fp64 per-layer reference of the conv stack (host only; tests/test_layer_reference_cpu.py, tests/test_gpu_layer_parity.py).

Every layer is recomputed in float64 from the GPU's OWN stored inputs (raw outputs of the source layers + their (scale, shift)
tables, read back through boa_net_debug_layer), so a layer's error is its own and does not accumulate along the stack:

  * layer_walk(geom): the layers in forward order with the names of their input sources -- encoder chain; transposed conv of the
    deepest / previous decoder output; decoder conv0 = cat([up, skip]) in the order oracle.network and net_forward_stack_x3 use;
    head.  Weights / biases come from the state dict, in PyTorch layout.
  * norm_act_x3 / norm_act8_pk / norm_act8: the activation a consuming kernel builds from a stored raw tensor, bit for bit:
      exact mode (precision 2) : y = lrelu(fmaf(raw, scale, shift)) in fp32 (commit_items_x3, the k_convt_x3 / k_head_x3 staging)
      fp16 mode, packed        : norm_act8_pk: y = fp16 fma(raw16, s16, t16); y = max(y, y * half(0.01))   (k_conv_ws, k_conv_ns,
                                 k_convt_mfma_rw, k_convt_deep)
      fp16 mode, fp32 table    : norm_act8: y = half(lrelu(fmaf(float(raw16), scale, shift)))               (k_convt_mfma, k_conv_mfma)
      a transposed conv's output is consumed raw by both modes.
  * conv3d64 / convt64 / head64: torch float64 on the CPU, 3x3x3 convs in z-slabs so that the im2col buffer stays below ~1 GB;
    abs_bound(...): A = sum |w| |x| + |b| per output voxel (the same conv on absolute values, fp32: only a scale).
  * norm_reference(raw, gamma, beta): fp64 InstanceNorm statistics of the GPU's own raw output -> (scale, shift).
  * x3_dot_emulate(...): a numpy model of the split-precision product (hi / lo fp16 parts, fp32 accumulation per 16-product MFMA
    step) with switchable terms: the CPU tests show with it that the GPU bar can see a missing term.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

# ---- bars --------------------------------------------------------------------------------------------------------------------
# Exact mode: |c - c64| <= TAU_X3(K) * A.  Ceiling 2^-20 * max(1, sqrt(K / 4096)) is the fp32 class: an fp32 FMA chain measures
# 0.75-1.5e-7 of sum |a b| at K <= 1024 and 3.5e-7 at K = 4096; the split product carries 22 significant bits per operand.
def tau_x3_ceiling(K: int) -> float:
    return 2.0 ** -20 * max(1.0, float(np.sqrt(K / 4096.0)))


# the bar the tests apply (MI355X measurement x <= 2, never above the ceiling; DESIGN section 3 has the table).  Measured by the run of
# tests/test_gpu_layer_parity.py that introduced it (re-measure with `pytest -m gpu -s tests/test_gpu_layer_parity.py`): the largest per-layer
# max(err / A) of a conv / transposed conv over the production geometry and the edge geometries is 4.9e-7 (enc0.conv1, K = 864; the
# head 6.7e-7 at K = 32), rms 2-4e-8.  The max sits at voxels whose inputs are mostly small (the LeakyReLU's negative side): the lo
# part of an activation below 2^-3 is an fp16 subnormal, an absolute floor of 2^-25 per operand.  2^-20 = 9.5e-7 = 1.95 x 4.9e-7.
TAU_X3 = 2.0 ** -20


def tau_x3(K: int) -> float:
    return min(TAU_X3, tau_x3_ceiling(K))


# fp16 mode: fp16 operands replicated exactly (inputs through consumer_input, weights rounded to fp16 as pack_conv_weights does),
# so what remains is the fp32 accumulation -- the same class as the exact mode -- plus the fp16 storage rounding of the result
# (+ 2^-11 |c64|, added by the caller)
TAU_FP16 = 2.0 ** -22
FP16_STORE = 2.0 ** -11


# ---- layer walk --------------------------------------------------------------------------------------------------------------
@dataclass
class Layer:
    name: str
    kind: int             # boa_net_debug_layer addressing: 0 encoder conv, 1 transposed conv, 2 decoder conv, 3 head
    stage: int
    conv: int
    sources: List[str]    # "input" = the gathered tile; else layer names, concatenated in this order
    wkey: str             # state-dict prefix: <wkey>.weight / <wkey>.bias
    normkey: Optional[str]
    kernel: Tuple[int, int, int] = (1, 1, 1)
    stride: Tuple[int, int, int] = (1, 1, 1)
    transposed: bool = False
    first: bool = False
    meta: Dict = field(default_factory=dict)

    def K(self, sd) -> int:
        w = sd[self.wkey + ".weight"]
        if self.transposed:
            return int(w.shape[0])                      # each output voxel of a kernel == stride convT sees one tap
        return int(np.prod(w.shape[1:]))


def layer_walk(geom) -> List[Layer]:
    n = len(geom.features)
    out: List[Layer] = []
    prev = "input"
    enc_last = []
    for s in range(n):
        for i in range(geom.n_conv_enc[s]):
            name = f"enc{s}.conv{i}"
            key = f"encoder.stages.{s}.0.convs.{i}"
            out.append(Layer(name, 0, s, i, [prev], key + ".conv", key + ".norm", tuple(geom.kernels[s]),
                             tuple(geom.strides[s]) if i == 0 else (1, 1, 1), first=(s == 0 and i == 0)))
            prev = name
        enc_last.append(prev)
    for k in range(n - 1):
        sb = n - 1 - k
        up = f"up{k}"
        out.append(Layer(up, 1, k, 0, [prev], f"decoder.transpconvs.{k}", None, tuple(geom.strides[sb]),
                         tuple(geom.strides[sb]), transposed=True))
        for i in range(geom.n_conv_dec[k]):
            name = f"dec{k}.conv{i}"
            key = f"decoder.stages.{k}.convs.{i}"
            srcs = [up, enc_last[sb - 1]] if i == 0 else [prev]   # torch.cat((u, skips[-(s + 2)]), 1)
            out.append(Layer(name, 2, k, i, srcs, key + ".conv", key + ".norm", tuple(geom.kernels[sb - 1])))
            prev = name
    out.append(Layer("head", 3, 0, 0, [prev], f"decoder.seg_layers.{n - 2}", None))
    return out


# ---- consumer input reconstruction -------------------------------------------------------------------------------------------
def _round_fma(p: np.ndarray, t: np.ndarray, dtype) -> np.ndarray:
    """Correctly rounded p + t to `dtype` (float32 / float16) for float64 p, t where p is an exact product: fp64 TwoSum, then a
    result sitting exactly on a rounding boundary of `dtype` is moved by the sign of the TwoSum error (single rounding)."""
    s = p + t
    bb = s - p
    err = (p - (s - bb)) + (t - bb)
    r = s.astype(dtype)
    up = np.nextafter(s, np.inf).astype(dtype)
    dn = np.nextafter(s, -np.inf).astype(dtype)
    tie = (up != dn) & (err != 0)
    if tie.any():
        r = np.where(tie, np.where(err > 0, up, dn), r)
    return r


def fmaf32(x: np.ndarray, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """__builtin_fmaf on fp32 operands (one rounding)."""
    return _round_fma(x.astype(np.float64) * a.astype(np.float64), np.broadcast_to(b.astype(np.float64), np.broadcast_shapes(x.shape, a.shape, b.shape)), np.float32)


def fmaf16(x: np.ndarray, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Packed fp16 fma (v_pk_fma_f16: one rounding to fp16) on fp16 operands."""
    return _round_fma(x.astype(np.float64) * a.astype(np.float64), np.broadcast_to(b.astype(np.float64), np.broadcast_shapes(x.shape, a.shape, b.shape)), np.float16)


def lrelu32(f: np.ndarray, slope: float = 0.01) -> np.ndarray:
    f = f.astype(np.float32)
    return np.where(f > 0, f, f * np.float32(slope)).astype(np.float32)


def norm_act_x3(raw: np.ndarray, ss: np.ndarray, slope: float = 0.01) -> np.ndarray:
    """Exact mode: y = lrelu(fmaf(raw, scale, shift)) in fp32.  raw [C, ...] fp32, ss [C, 2] fp32."""
    sh = (-1,) + (1,) * (raw.ndim - 1)
    return lrelu32(fmaf32(raw, ss[:, 0].reshape(sh), ss[:, 1].reshape(sh)), slope)


def ss16_unpack(words: np.ndarray) -> np.ndarray:
    """boa_net_debug_layer's host_ss16 ([C/2][4] fp16 bits: s_c, s_c+1, t_c, t_c+1) -> [C, 2] float16."""
    q = np.asarray(words, dtype=np.uint16).reshape(-1, 4).view(np.float16)
    out = np.empty((q.shape[0] * 2, 2), np.float16)
    out[0::2, 0], out[1::2, 0], out[0::2, 1], out[1::2, 1] = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return out


def ss16_pack(ss: np.ndarray) -> np.ndarray:
    """What k_norm_finalize writes next to the fp32 table: fp16 roundings of (scale, shift), packed as ss16_unpack reads them."""
    h = ss.astype(np.float32).astype(np.float16)
    q = np.empty((h.shape[0] // 2, 4), np.float16)
    q[:, 0], q[:, 1], q[:, 2], q[:, 3] = h[0::2, 0], h[1::2, 0], h[0::2, 1], h[1::2, 1]
    return q.view(np.uint16).reshape(-1)


def norm_act8_pk(raw16: np.ndarray, ss16: np.ndarray, slope: float = 0.01) -> np.ndarray:
    """fp16 mode, packed form: y = fma16(x, s16, t16); y = max(y, y * half(slope)), all in fp16.  raw16 [C, ...] fp16."""
    sh = (-1,) + (1,) * (raw16.ndim - 1)
    y = fmaf16(raw16.astype(np.float16), ss16[:, 0].reshape(sh), ss16[:, 1].reshape(sh))
    z = (y * np.float16(np.float32(slope))).astype(np.float16)
    return np.maximum(y, z)


def norm_act8(raw16: np.ndarray, ss: np.ndarray, slope: float = 0.01) -> np.ndarray:
    """fp16 mode, fp32 table (norm_act8 of k_convt_mfma / k_conv_mfma): half(lrelu(fmaf(float(x), scale, shift)))."""
    sh = (-1,) + (1,) * (raw16.ndim - 1)
    f = fmaf32(raw16.astype(np.float32), ss[:, 0].reshape(sh), ss[:, 1].reshape(sh))
    return lrelu32(f, slope).astype(np.float16)


# ---- fp64 ops ----------------------------------------------------------------------------------------------------------------
def _slab_rows(cin: int, k, out_hw: int, budget: float = 1e9) -> int:
    return max(1, int(budget // (8.0 * cin * int(np.prod(k)) * out_hw)))


def conv3d64(x: np.ndarray, w: np.ndarray, b: Optional[np.ndarray], stride, budget: float = 1e9, dtype=torch.float64) -> np.ndarray:
    """Conv3d(k, stride, pad (k - 1) / 2) + bias of x [Cin, D, H, W] in `dtype`, output rows along D in slabs."""
    k = w.shape[2:]
    pad = [(kk - 1) // 2 for kk in k]
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)[None]
    xt = F.pad(xt, (pad[2], pad[2], pad[1], pad[1], pad[0], pad[0]))
    wt = torch.from_numpy(np.ascontiguousarray(w)).to(dtype)
    bt = None if b is None else torch.from_numpy(np.ascontiguousarray(b)).to(dtype)
    D, H, W = x.shape[1:]
    Do, Ho, Wo = [(n + 2 * p - kk) // s + 1 for n, p, kk, s in zip((D, H, W), pad, k, stride)]
    rows = _slab_rows(x.shape[0], k, Ho * Wo, budget)
    out = []
    with torch.inference_mode():
        for o0 in range(0, Do, rows):
            o1 = min(Do, o0 + rows)
            xi = xt[:, :, o0 * stride[0]:(o1 - 1) * stride[0] + k[0]]
            out.append(F.conv3d(xi, wt, bt, tuple(stride)))
    return torch.cat(out, 2)[0].numpy()


def convt64(x: np.ndarray, w: np.ndarray, b: Optional[np.ndarray], stride, dtype=torch.float64) -> np.ndarray:
    """ConvTranspose3d(kernel == stride) + bias; w [Cin, Cout, s0, s1, s2] (PyTorch layout)."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)[None]
    wt = torch.from_numpy(np.ascontiguousarray(w)).to(dtype)
    bt = None if b is None else torch.from_numpy(np.ascontiguousarray(b)).to(dtype)
    with torch.inference_mode():
        return F.conv_transpose3d(xt, wt, bt, tuple(stride))[0].numpy()


def head64(x: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
    """1x1x1 conv: w [C, F0, 1, 1, 1]."""
    return (np.einsum("cf,f...->c...", w.reshape(w.shape[0], -1).astype(np.float64), x.astype(np.float64))
            + b.astype(np.float64).reshape((-1,) + (1,) * (x.ndim - 1)))


def layer64(layer: Layer, x: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
    if layer.transposed:
        return convt64(x, w, b, layer.stride)
    if layer.kind == 3:
        return head64(x, w, b)
    return conv3d64(x, w, b, layer.stride)


def abs_bound(layer: Layer, x: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
    """A = sum |w| |x| + |b| per output voxel (fp32: a scale only)."""
    ax, aw, ab = np.abs(x).astype(np.float32), np.abs(w).astype(np.float32), np.abs(b).astype(np.float32)
    if layer.transposed:
        return convt64(ax, aw, ab, layer.stride, dtype=torch.float32)
    if layer.kind == 3:
        return head64(ax, aw, ab)
    return conv3d64(ax, aw, ab, layer.stride, budget=2e9, dtype=torch.float32)


def norm_reference(raw: np.ndarray, gamma: np.ndarray, beta: np.ndarray, eps: float = 1e-5):
    """fp64 InstanceNorm of the GPU's own raw output [C, ...]: (scale, shift) [C, 2] float64, plus mean and variance."""
    r = raw.reshape(raw.shape[0], -1).astype(np.float64)
    mean = r.mean(1)
    var = ((r - mean[:, None]) ** 2).mean(1)
    scale = gamma.astype(np.float64) / np.sqrt(var + eps)
    shift = beta.astype(np.float64) - mean * scale
    return np.stack([scale, shift], 1), mean, var


# InstanceNorm (scale, shift): the statistics are fp32 partial sums of (c, c^2) per conv-epilogue slot, reduced in fp64;
# var = E[c^2] - mean^2 amplifies the relative error eps_s of E[c^2] by E[c^2] / var = 1 + mean^2 / var, and scale = gamma / sqrt(var
# + eps) halves it: |d scale| / scale <= SS_EPS * (1 + mean^2 / var) / 2 + 2^-24 (its fp32 rounding).  SS_EPS = the relative error
# of an fp32-accumulated sum of positive terms (measured on MI355X: see DESIGN section 3).  The fp16 mode's statistics are
# those of the fp32 epilogue values, the stored raw output is their fp16 rounding: + 2^-11 / sqrt(n) of the rms for the mean.
SS_EPS = 2.0 ** -20


def ss_bars(raw: np.ndarray, ss: np.ndarray, ss64: np.ndarray, mean: np.ndarray, var: np.ndarray, fp16: bool):
    """A conv's (scale, shift) table `ss` [C, 2] against norm_reference's (ss64, mean, var) of its own raw output [C, ...]: the largest
    |d scale| / scale and |d shift| over their bars (<= 1 passes), and the largest |mean| / std."""
    r2 = raw.reshape(raw.shape[0], -1).astype(np.float64)
    n = r2.shape[1]
    amp = 1.0 + mean ** 2 / np.maximum(var, 1e-300)          # E[c^2] / var
    dmean = SS_EPS * np.abs(r2).mean(1)                        # fp32 sum of c: error relative to sum |c|
    rel = SS_EPS * amp / 2 + 2.0 ** -24
    if fp16:   # statistics of the fp32 epilogue values, not of their fp16 roundings: 4 sigma of the rounding noise
        rel = rel + (2.0 ** -24 + 4 * 2.0 ** -11 / np.sqrt(n)) * amp
        dmean = dmean + 4 * 2.0 ** -11 * np.sqrt((r2 ** 2).mean(1) / n)
    ds = np.abs(ss[:, 0] - ss64[:, 0]) / np.abs(ss64[:, 0])
    dt = np.abs(ss[:, 1] - ss64[:, 1])
    tol_t = 2.0 ** -24 * np.abs(ss64[:, 1]) + np.abs(ss64[:, 0]) * dmean + np.abs(mean * ss64[:, 0]) * rel
    return float((ds / rel).max()), float((dt / tol_t).max()), float((np.abs(mean) / np.sqrt(np.maximum(var, 1e-300))).max())


# ---- numpy model of the split-precision product ------------------------------------------------------------------------------
def x3_weight_scale(w: np.ndarray) -> float:
    """csrc/conv.hip x3_weight_scale: power of two that puts max |w| into [2^13, 2^14)."""
    m = float(np.max(np.abs(w.astype(np.float32))))
    if not (m > 0) or not np.isfinite(m):
        return 1.0
    _, e = np.frexp(m)
    return float(np.ldexp(1.0, max(-24, min(14 - int(e), 40))))


def split16(v: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """x3_split4: hi = half(v), lo = half(v - hi) (v - hi exact in fp32)."""
    v = v.astype(np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def x3_dot_emulate(w: np.ndarray, x: np.ndarray, b: np.ndarray, terms=("hh", "hl", "lh"), drop_octet: Optional[Tuple[int, int]] = None,
                   taps: int = 1) -> np.ndarray:
    """out[o] = sum_k w[o, k] x[k, j] + b[o] the way k_conv_ws<X3> forms it.  w [Cout, K] with K = taps * Cin ordered [tap][cin],
    x [K, J] fp32 activations, b [Cout].  The weights are scaled by the layer's power of two and split; so is x; `terms` picks
    the cross products (hh, hl = Wh Xl, lh = Wl Xh, ll); products are exact, every 16-product MFMA step (one 8-channel octet x
    two parts) is added to the fp32 accumulator with one rounding; the accumulator starts at b * wscale and is multiplied by
    1 / wscale at the end.  drop_octet = (tap, octet): leave that 8-channel group of one tap out (a lost K-step)."""
    ws = x3_weight_scale(w)
    wh, wl = split16(w.astype(np.float32) * np.float32(ws))
    xh, xl = split16(x)
    wh, wl, xh, xl = (a.astype(np.float64) for a in (wh, wl, xh, xl))
    K = w.shape[1]
    cin = K // taps
    acc = (b.astype(np.float32) * np.float32(ws)).astype(np.float32)[:, None] * np.ones((1, x.shape[1]), np.float32)
    for k0 in range(0, K, 8):
        if drop_octet is not None and k0 == drop_octet[0] * cin + 8 * drop_octet[1]:
            continue
        sl = slice(k0, k0 + 8)
        step = np.zeros(acc.shape, np.float64)
        if "hh" in terms:
            step += wh[:, sl] @ xh[sl]
        if "hl" in terms:
            step += wh[:, sl] @ xl[sl]
        if "lh" in terms:
            step += wl[:, sl] @ xh[sl]
        if "ll" in terms:
            step += wl[:, sl] @ xl[sl]
        acc = (acc.astype(np.float64) + step).astype(np.float32)
    return (acc * np.float32(1.0 / ws)).astype(np.float32)
