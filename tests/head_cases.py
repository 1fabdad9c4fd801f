"""Cases and numpy references for the last layer's fallback kernels (host only: tests/test_head_cases_cpu.py proves the set on the CPU,
tests/test_gpu_head_forms.py and tests/test_gpu_finalize_forms.py run it).

  * head64: y = lrelu(x * scale + shift), W y + b and A = sum |w| |y| + |b| in float64 from the exact fp16 / fp32 inputs.
  * planar16 / octet32 / channels_last: the three activation layouts the scatter heads read, with their inverses.
  * head_form / finalize_form: launch_head's dispatch (csrc/head.hip) and the vec8 predicate of boa_finalize_labels_planes (csrc/seg.hip)
    restated in Python, so that the CPU test can show that every case below reaches the kernel form it is named for.  The GPU tests
    assert the same branch through the launch counters.
  * finalize_ref: boa_finalize_labels_planes as statements of oracle.sliding_window / oracle.labels arithmetic: returns the new
    accumulator bits, the new fold bits, the labels and the inf flag (the oracle's finalize_logits raises instead of reporting).
  * canon_nan: bit patterns are compared with every NaN mapped to one pattern.  The sign and payload of a NaN that an fp32 operation
    produces (inf - inf, 0 / 0) differ between processors and are no part of the reference's arithmetic.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

import layer_reference as lr
from oracle import labels as olab
from oracle import sliding_window as osw

SLOPE = 0.01
GUARD = 64          # fp16 elements of sentinel in front of and behind an accumulator (128 bytes: keeps the 16-byte alignment)


# ---- references ----------------------------------------------------------------------------------------------------------------
def head64(act, ss, w, b, slope=SLOPE):
    """act [P0][P1][P2][F0] (fp16 or fp32), ss [F0][2] fp32, w [C][F0] fp32, b [C] fp32 -> (logits, A) float64 [C][P0][P1][P2]."""
    x = np.moveaxis(np.asarray(act).astype(np.float64), -1, 0)
    sh = (-1,) + (1,) * (x.ndim - 1)
    f = x * ss[:, 0].astype(np.float64).reshape(sh) + ss[:, 1].astype(np.float64).reshape(sh)
    y = np.where(f > 0, f, f * np.float64(np.float32(slope)))
    return lr.head64(y, w, b), lr.head64(np.abs(y), np.abs(w), np.abs(b))


def logit_bound(F0: int) -> float:
    """|err| <= (F0 + 4) 2^-24 A: an fp32 fma chain of F0 + 1 terms on inputs that carry two roundings (norm fma, slope multiply), one
    unit for the second-order terms."""
    return (F0 + 4) * 2.0 ** -24


def canon_nan(bits):
    b = np.asarray(bits, dtype=np.uint16)
    return np.where((b & 0x7FFF) > 0x7C00, np.uint16(0x7E00), b)


def accumulate_tile(acc, n, pred, gauss, start):
    """oracle.sliding_window.accumulate_tile without the overflow / invalid warnings of accumulators that reach inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        osw.accumulate_tile(acc, n, pred, gauss, tuple(int(v) for v in start))


# ---- layouts -------------------------------------------------------------------------------------------------------------------
def planar16(act, stride: Optional[int] = None):
    """channels-last [..., F0] -> the fp16 engine layout [F0/16][stride voxels][16] (tests/test_gpu_head._Head.planar for any F0)."""
    return _planes(act, 16, stride)


def octet32(act, stride: Optional[int] = None):
    """channels-last [..., F0] -> the split-precision layout [F0/8][stride voxels][8]."""
    return _planes(act, 8, stride)


def channels_last(act):
    """[..., F0] -> records [voxel][F0]."""
    return np.ascontiguousarray(act.reshape(-1, act.shape[-1]))


def _planes(act, g, stride):
    F0 = act.shape[-1]
    a = act.reshape(-1, F0)
    pv = a.shape[0]
    stride = pv if stride is None else stride
    assert F0 % g == 0 and stride >= pv
    out = np.zeros((F0 // g, stride, g), act.dtype)
    out[:, :pv] = a.reshape(pv, F0 // g, g).transpose(1, 0, 2)
    return out


def unplanes(planes, P):
    """inverse of planar16 / octet32: [F0/g][stride][g] -> [P0][P1][P2][F0]."""
    pv = int(np.prod(P))
    ng, _, g = planes.shape
    return np.ascontiguousarray(planes[:, :pv].transpose(1, 0, 2).reshape(*P, ng * g))


# ---- launch_head's dispatch ----------------------------------------------------------------------------------------------------------
def head_form(F0, P, C, logits, PV=None, start=None, act_align=0, acc_align=0, nacc_align=0, gauss_align=0, logits_align=0):
    """The kernel launch_head runs (csrc/head.hip).  *_align = the pointer's address modulo 16 (gauss_align None: no Gaussian)."""
    assert F0 in (32, 64)
    pair = P[2] % 2 == 0 and F0 == 32
    if not logits:
        pair = pair and PV[2] % 2 == 0 and start[2] % 2 == 0 and acc_align % 4 == 0
    mfma_shape = F0 == 32 and C <= 31 and P[2] % 32 == 0 and act_align == 0
    if not logits and mfma_shape and start[2] % 8 == 0 and PV[2] % 8 == 0 and acc_align == 0 and nacc_align == 0 and not gauss_align:
        return "k_head_mfma<acc>"
    if logits and mfma_shape and logits_align == 0:
        return "k_head_mfma<logits>"
    if not logits and mfma_shape:
        return "k_head_mfma<logits>+k_accumulate_tile"
    return "k_head<32,2>" if pair else "k_head<32,1>" if F0 == 32 else "k_head<64,1>"


def head_lds_bytes(F0, C):
    return (C * F0 + C + 2 * F0) * 4


def finalize_form(V, planes=None, acc_align=0, n_align=0, fold_align=0):
    """k_finalize_labels<8> or <1> (csrc/seg.hip): voxel count, first voxel and count of the plane range multiples of 8, pointers
    16-byte aligned (fold_align 0 also stands for no fold buffer)."""
    lo, hi = planes if planes is not None else (0, V[0])
    vtot, begin, count = V[0] * V[1] * V[2], lo * V[1] * V[2], (hi - lo) * V[1] * V[2]
    vec8 = vtot % 8 == 0 and begin % 8 == 0 and count % 8 == 0 and (acc_align | n_align | fold_align) % 16 == 0
    return 8 if vec8 else 1


# ---- the head cases ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class HeadCase:
    name: str
    kind: str                 # "fp16" (boa_head_tile) | "x3" | "f32cl" | "f32oct" (boa_head_tile_f32)
    F0: int
    C: int
    P: Tuple[int, int, int]
    PV: Tuple[int, int, int]
    starts: Tuple[Tuple[int, int, int], ...]
    forms: Tuple[str, ...]    # the accumulate-mode kernel of every tile
    logits_form: str
    scale: float = 1.0        # multiplies the (scale, shift) table ...
    wmul: float = 1.0         # ... and the head weights: 300 and 4 put the largest logits at ~1e4
    pad: int = 0              # plane / octet stride = pv + pad

    @property
    def pv(self):
        return int(np.prod(self.P))

    @property
    def far(self):
        return tuple(v - p for v, p in zip(self.PV, self.P))


def _starts(P, PV, zs):
    """three (or more) overlapping tiles: the origin corner, one step in, ..., the last one flush against the far corner of PV"""
    far = tuple(v - p for v, p in zip(PV, P))
    out = []
    for i, z in enumerate(zs):
        last = i == len(zs) - 1
        out.append(tuple(far[:2]) + (z,) if last else (min(i, far[0]), min(i, far[1]), z))
    assert out[-1] == far, (out, far)
    return tuple(out)


def _fp16_case(name, F0, C, P, PV, zs, scale=1.0, wmul=1.0):
    starts = _starts(P, PV, zs)
    forms = tuple(head_form(F0, P, C, False, PV, s) for s in starts)
    return HeadCase(name, "fp16", F0, C, tuple(P), tuple(PV), starts, forms, head_form(F0, P, C, True), scale, wmul)


def fp16_cases() -> List[HeadCase]:
    out = []
    # k_head<32,2>: P2, PV z and every start z even.  (3, 5, 32): P2 % 32 == 0, more than 31 classes alone keep it off the matrix cores
    for C in (32, 118):
        out.append(_fp16_case(f"pair-C{C}-P3x5x32", 32, C, (3, 5, 32), (5, 8, 40), (0, 4, 8)))
        out.append(_fp16_case(f"pair-C{C}-P2x3x6", 32, C, (2, 3, 6), (4, 5, 10), (0, 2, 4)))
    # k_head<32,1>: odd P2 whatever the accumulator geometry; even P2 with odd start z (the far-corner tile is even again: the pair form
    # next to the scalar one on the same accumulators) and with an odd PV z
    for C in (5, 33):
        out.append(_fp16_case(f"single-C{C}-P3x5x7", 32, C, (3, 5, 7), (5, 7, 11), (0, 1, 4)))
        out.append(_fp16_case(f"single-C{C}-P2x3x6-odd-start", 32, C, (2, 3, 6), (4, 5, 12), (1, 3, 5, 6)))
        out.append(_fp16_case(f"single-C{C}-P2x3x6-odd-PV", 32, C, (2, 3, 6), (4, 5, 13), (0, 2, 7)))
    # k_head<64,1>: 8-aligned and unaligned origins, a 32-voxel z extent and an odd one
    for C in (1, 7, 40):
        out.append(_fp16_case(f"f64-C{C}-P3x4x32", 64, C, (3, 4, 32), (5, 6, 40), (0, 3, 8)))
        out.append(_fp16_case(f"f64-C{C}-P2x3x5", 64, C, (2, 3, 5), (4, 5, 9), (0, 1, 4)))
    # the MFMA logits into a scratch buffer + k_accumulate_tile: z origins / extent that are no multiples of 8
    out.append(_fp16_case("mfma-logits-accumulate-C31", 32, 31, (2, 2, 32), (4, 4, 70), (3, 19, 38)))
    # logits of ~1e4: accumulators near the fp16 maximum, beyond it with the Gaussian (weight up to 10)
    out.append(_fp16_case("pair-large-C32", 32, 32, (3, 5, 32), (5, 8, 40), (0, 4, 8), scale=300.0, wmul=4.0))
    # 66812 bytes of LDS: above the 64 KiB a kernel gets by default
    out.append(_fp16_case("f64-C255-lds", 64, 255, (2, 3, 5), (4, 5, 9), (0, 1, 4)))
    return out


X3_SHAPES = {96: (1, 3, 32), 100: (4, 5, 5), 315: (7, 9, 5), 129: (1, 3, 43), 256: (2, 4, 32)}


def _f32_case(name, kind, F0, C, P, pad):
    PV = (P[0] + 2, P[1] + 2, P[2] + 9)
    zs = (0, 3, PV[2] - P[2])           # aligned, odd, far corner
    starts = _starts(P, PV, zs)
    k = "k_head_x3" if kind == "x3" else "k_head_f32"
    return HeadCase(name, kind, F0, C, tuple(P), PV, starts, (k,) * len(starts), k, 1.0, 1.0, pad)


def x3_cases() -> List[HeadCase]:
    """k_head_x3: one wave = 32 voxels, one block = 128.  pv = 96: whole waves, a partial block; 100: a partial wave; 315; 129: a wave
    with one valid lane and three waves whose lanes are all invalid; 256: whole blocks."""
    out = []
    for i, (C, pv) in enumerate(itertools.product((1, 4, 5, 31, 32), (96, 100, 315, 129, 256))):
        out.append(_f32_case(f"x3-C{C}-pv{pv}", "x3", 32, C, X3_SHAPES[pv], 5 * (i % 2)))
    return out


def f32_cases() -> List[HeadCase]:
    out = []
    for i, (F0, kind, C, pv) in enumerate(itertools.product((8, 32, 64), ("f32cl", "f32oct"), (1, 33, 118), (315, 512))):
        P = (7, 9, 5) if pv == 315 else (4, 4, 32)
        out.append(_f32_case(f"{kind}-F{F0}-C{C}-pv{pv}", kind, F0, C, P, 3 * (i % 2) if kind == "f32oct" else 0))
    return out


def head_inputs(case: HeadCase, seed: int = 0):
    """(w [C][F0], b [C], [(act [*P][F0], ss [F0][2]) per tile]); act fp16 for the fp16 heads, fp32 for the others."""
    rng = np.random.default_rng([seed, case.F0, case.C, case.pv])
    w = (rng.standard_normal((case.C, case.F0)) * 0.4 * case.wmul).astype(np.float32)
    b = (rng.standard_normal(case.C) * 0.5).astype(np.float32)
    tiles = []
    for _ in case.starts:
        act = rng.standard_normal((*case.P, case.F0)) * 1.5
        act = act.astype(np.float16 if case.kind == "fp16" else np.float32)
        ss = np.stack([rng.uniform(0.5, 1.5, case.F0), rng.normal(0, 0.3, case.F0)], axis=1) * case.scale
        tiles.append((act, ss.astype(np.float32)))
    return w, b, tiles


def pack_act(case: HeadCase, act):
    stride = case.pv + case.pad
    if case.kind == "fp16":
        return planar16(act), 0
    if case.kind == "f32cl":
        return channels_last(act), 0
    return octet32(act, stride), stride


def sentinel(n: int, salt: int = 0):
    """n fp16 bit patterns that no accumulation produces by chance"""
    return ((np.arange(n, dtype=np.uint32) * 40503 + 0x1235 + salt) & 0xFFFF).astype(np.uint16)


def initial_accumulators(case: HeadCase, seed: int = 1):
    """what the tiles are added to: small fp16 values (the read of the read-modify-write matters) and non-negative weights"""
    rng = np.random.default_rng([seed, case.C, *case.PV])
    acc = rng.uniform(-1, 1, (case.C, *case.PV)).astype(np.float16)
    n = rng.uniform(0, 1, case.PV).astype(np.float16)
    return acc, n


def gaussian(P):
    return np.ascontiguousarray(osw.compute_gaussian(tuple(P), 1. / 8, 10))


# ---- finalize ------------------------------------------------------------------------------------------------------------------------
def _f16(bits):
    return np.ascontiguousarray(bits, dtype=np.uint16).view(np.float16)


def finalize_ref(acc_bits, n_bits, fold_bits=None, fold_mode=0, n_folds_final=0, write_logits=1, lut=None, merge=0, labels_in=None,
                 crop=None, planes=None):
    """boa_finalize_labels_planes on fp16 bit patterns acc [C][V], n [V], fold [C][V] or None.  labels_in: the label volume before the
    call ([V], or crop[1] with crop = (offsets, dims)), None: no label output.  planes = (lo, hi) of axis 0, None: all.
    Returns (acc bits, fold bits or None, labels or None, inf flag) after the call.

      logits = acc / n                      oracle.sliding_window.finalize_logits: fp16 / fp16 in fp32, RTNE to fp16; inf sets the flag
      fold   = logits | fold + logits       ensemble_folds: fp16 + fp16 in fp32, RTNE; then / n_folds_final (fp32, RTNE) when > 1
      labels = lut[argmax]                  oracle.labels.argmax_labels (first maximum, the first NaN wins) of the folded logits, when the
                                            call is the last fold's (no fold buffer or n_folds_final > 0); merge: only where argmax != 0
    """
    acc_bits, n_bits = np.array(acc_bits, dtype=np.uint16), np.asarray(n_bits, dtype=np.uint16)
    V = n_bits.shape
    lo, hi = planes if planes is not None else (0, V[0])
    rng_ = slice(lo, hi)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        q = (_f16(acc_bits[:, rng_]).astype(np.float32) / _f16(n_bits[rng_]).astype(np.float32)[None]).astype(np.float16)
        inf = int(np.isinf(q).any())
        if write_logits:
            acc_bits[:, rng_] = q.view(np.uint16)
        fold_out = None
        if fold_bits is not None:
            fold_out = np.array(fold_bits, dtype=np.uint16)
            if fold_mode == 1:
                q = (_f16(fold_out[:, rng_]).astype(np.float32) + q.astype(np.float32)).astype(np.float16)
            if n_folds_final > 1:
                q = (q.astype(np.float32) / np.float32(n_folds_final)).astype(np.float16)
            fold_out[:, rng_] = q.view(np.uint16)
    labels = None
    if labels_in is not None and (fold_bits is None or n_folds_final > 0):
        labels = np.array(labels_in, dtype=np.uint8)
        idx = olab.argmax_labels(q)
        table = np.arange(256, dtype=np.uint8) if lut is None else np.asarray(lut, dtype=np.uint8)
        new = table[idx]
        off, dims = crop if crop is not None else ((0, 0, 0), V)
        assert labels.shape == tuple(dims)
        x0, x1 = max(lo, off[0]), min(hi, off[0] + dims[0])           # padded-grid planes of the range that fall into the crop box
        if x1 > x0:
            src = (slice(x0 - lo, x1 - lo), slice(off[1], off[1] + dims[1]), slice(off[2], off[2] + dims[2]))
            dst = labels[x0 - off[0]:x1 - off[0]]
            if merge:
                np.copyto(dst, new[src], where=idx[src] != 0)
            else:
                dst[...] = new[src]
    return acc_bits, fold_out, labels, inf


def fp16_patterns(rng, shape, special=False):
    """fp16 bit patterns: normals of every magnitude, subnormals, +-0 and (special) +-inf and NaN"""
    b = rng.integers(0, 0x7C00, shape, dtype=np.uint16)                       # every finite magnitude, subnormals included
    b = np.where(rng.random(shape) < 0.5, b, rng.integers(0x3000, 0x4800, shape, dtype=np.uint16))   # half of them of moderate size
    b = np.where(rng.random(shape) < 0.05, rng.integers(0, 0x0400, shape, dtype=np.uint16), b)       # subnormals
    b = np.where(rng.random(shape) < 0.03, np.uint16(0), b)
    if special:
        b = np.where(rng.random(shape) < 0.01, np.uint16(0x7C00), b)
        b = np.where(rng.random(shape) < 0.01, rng.integers(0x7C01, 0x8000, shape, dtype=np.uint16), b)
    return (b | (rng.integers(0, 2, shape, dtype=np.uint16) << 15)).astype(np.uint16)


@dataclass(frozen=True)
class FinalizeCase:
    name: str
    V: Tuple[int, int, int]
    C: int
    vec: int                                    # the kernel form of the whole-volume call with aligned pointers
    fold_mode: Optional[int] = None             # None: no fold buffer
    n_folds_final: int = 0
    write_logits: int = 1
    lut: bool = False
    merge: int = 0
    crop: Optional[Tuple[Tuple[int, int, int], Tuple[int, int, int]]] = None
    special: bool = False                       # +-inf / NaN among the inputs
    labels: bool = True


def finalize_inputs(case: FinalizeCase, seed: int = 0):
    """(acc bits [C][V], n bits [V], fold bits [C][V] | None, lut | None, labels before the call | None).  Exact ties for the first place on a third of
    the voxels; weights are positive and normal here (zero / subnormal ones have their own test)."""
    rng = np.random.default_rng([seed, case.C, *case.V])
    acc = fp16_patterns(rng, (case.C, *case.V), case.special)
    if case.C > 1:
        tie = rng.random(case.V) < 0.33                      # the maximum's bits into the next class row: a tie for the first place
        m = acc.view(np.float16).astype(np.float32).argmax(0)
        val = np.take_along_axis(acc, m[None], 0)[0]
        other = (m + 1) % case.C
        np.put_along_axis(acc, other[None], np.where(tie, val, np.take_along_axis(acc, other[None], 0)[0])[None], 0)
    n = rng.uniform(0.05, 20, case.V).astype(np.float16).view(np.uint16)
    fold = fp16_patterns(rng, (case.C, *case.V), case.special) if case.fold_mode is not None else None
    lut = None
    if case.lut:
        lut = ((np.arange(256) * 7 + 3) % 251).astype(np.uint8)
        lut[0] = 0
    shape = case.crop[1] if case.crop else case.V
    labels = rng.integers(200, 256, shape).astype(np.uint8) if case.labels else None
    return acc, n, fold, lut, labels


def finalize_cases() -> List[FinalizeCase]:
    """Form selection x class counts, then the options in combination: every option appears with and without every other one
    (test_head_cases_cpu checks the pairwise coverage)."""
    S, E = (3, 5, 7), (2, 4, 8)                # 105 voxels: scalar form; 64: vec8
    crop_s, crop_e = ((1, 2, 3), (2, 2, 3)), ((0, 1, 2), (2, 2, 5))
    F = FinalizeCase
    return [
        F("scalar-C1", S, 1, 1), F("scalar-C2", S, 2, 1), F("scalar-C255", S, 255, 1),
        F("vec8-C1", E, 1, 8), F("vec8-C2", E, 2, 8), F("vec8-C255", E, 255, 8, special=True),
        F("scalar-special", S, 7, 1, special=True), F("vec8-special", E, 7, 8, special=True),
    ] + _option_cases(S, E, crop_s, crop_e)


def _valid_option_rows():
    """every meaningful combination: n_folds_final goes with a fold buffer; a call that is not the last fold's writes no labels, so lut,
    merge and crop say nothing there"""
    rows = []
    for fm, nff, wr, lut, mg, cr in itertools.product((None, 0, 1), (0, 1, 3), (0, 1), (False, True), (0, 1), (False, True)):
        if fm is None and nff != 0:
            continue
        if fm is not None and nff == 0 and (lut or mg or cr):
            continue
        rows.append((fm, nff, wr, lut, mg, cr))
    return rows


def option_pairs(row):
    """the (dimension, value) pairs a row covers"""
    names = ("fold_mode", "n_folds_final", "write_logits", "lut", "merge", "crop")
    items = list(zip(names, row))
    return {(a, b) for a, b in itertools.combinations(items, 2)}


def _option_cases(S, E, crop_s, crop_e):
    """greedy pairwise cover of the valid combinations (deterministic: ties go to the first row in product order)"""
    rows = _valid_option_rows()
    todo = set().union(*(option_pairs(r) for r in rows))
    out = []
    while todo:
        best = max(rows, key=lambda r: len(option_pairs(r) & todo))
        todo -= option_pairs(best)
        i = len(out)
        fm, nff, wr, lut, mg, cr = best
        V, vec, crop = (S, 1, crop_s) if i % 2 == 0 else (E, 8, crop_e)
        labels = fm is None or nff > 0
        out.append(FinalizeCase(f"opt-{i}", V, (5, 6, 3, 9)[i % 4], vec, fm, nff, wr, lut, mg, crop if cr else None, special=(i % 3 == 2),
                                labels=labels))
    return out


def finalize_options(case: FinalizeCase):
    """the option values of a case, in the order option_pairs names them"""
    return (case.fold_mode, case.n_folds_final, case.write_logits, case.lut, case.merge, case.crop is not None)
