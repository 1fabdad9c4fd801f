"""Test-only model of the irreversible path of JPEG 2000 (dequantisation, inverse 9/7, sample conversion) in numpy float32,
following OpenJPEG's arithmetic operation by operation: it builds on j2k_reference.decode_block(with_last=True)
for tier-1 and consumes the host tables of boa_hip.jpeg2000.  Every product and every sum is rounded to float32 on its own
(numpy float32 arrays never fuse a multiply and an add), which is what csrc/j2k_dwt97.h does on the device and on the host."""
import numpy as np

import j2k_reference as R

F = np.float32
K_LOW, K_HIGH = F(1.230174105), F(1.625732422)          # the scales of the even (low-pass) and odd (high-pass) samples
LIFT = ((0, F(0.443506852)), (1, F(0.882911075)), (0, F(-0.052980118)), (1, F(-1.586134342)))   # (parity, c), in order


def quantised(v, last):
    """What tier-1 leaves (v: signed, the midpoint added for last >= 1; last: lowest coded plane, -1 not significant) ->
    the integer q = +-(2 m + 2^b_last) = +-(2 |v| + (b_last == 0))."""
    return np.sign(v) * (2 * np.abs(v) + (last == 0))


def block_plane(fr, passes=None):
    """A 9/7 boa_hip.jpeg2000.Frame -> (float32 [rows][cols] dequantised coefficients in Mallat layout, ok).  passes: the pass
    count of every block, where it is not the table's."""
    plane = np.zeros((fr.rows, fr.cols), dtype=F)
    off, ok = 0, True
    for k, (o, x0, y0, w, h, nbp, npass, ln) in enumerate(fr.blocks.tolist()):
        v, last, good = R.decode_block(fr.data, off, ln, w, h, o, nbp, npass if passes is None else int(passes[k]), with_last=True)
        ok = ok and good
        q = quantised(v, last)
        assert np.abs(q).max(initial=0) < 1 << 31
        plane[y0:y0 + h, x0:x0 + w] = q.astype(np.int32).astype(F) * (F(0.5) * fr.steps[fr.band[k]])
        off += ln
    return plane, ok


def idwt97_1d(y, axis):
    """Inverse 9/7 along `axis` of a float32 array in Mallat order (low half first), zero origin: interleave, scale, four
    lifting steps with whole-sample mirroring; a length-1 signal passes through unscaled."""
    y = np.moveaxis(np.asarray(y, dtype=F), axis, 0)
    n = y.shape[0]
    if n == 1:
        return np.moveaxis(y.copy(), 0, axis)
    nl = (n + 1) // 2
    x = np.empty_like(y)
    x[0::2] = y[:nl] * K_LOW
    x[1::2] = y[nl:] * K_HIGH
    idx = np.arange(n)
    left = np.where(idx - 1 < 0, 1, idx - 1)
    right = np.where(idx + 1 >= n, n - 2, idx + 1)
    for parity, c in LIFT:
        i = idx[parity::2]
        s = (x[left[i]] + x[right[i]]).astype(F)
        x[i] = (x[i] + (s * F(-c)).astype(F)).astype(F)
    return np.moveaxis(x, 0, axis)


def synthesise(plane, levels):
    """float32 coefficients in Mallat layout -> the inverse transform's output: per level rows, then columns."""
    plane = np.array(plane, dtype=F)
    rows, cols = plane.shape
    for r in range(1, levels + 1):
        d = levels - r
        hr, wr = -(-rows >> d), -(-cols >> d)
        reg = idwt97_1d(plane[:hr, :wr], 1)
        plane[:hr, :wr] = idwt97_1d(reg, 0)
    return plane


def reconstruct(fr, passes=None):
    """A 9/7 Frame -> (float32 [rows][cols], the inverse transform's output before rounding; ok)."""
    plane, ok = block_plane(fr, passes)
    return synthesise(plane, fr.levels), ok


def samples(plane, P, signed):
    """float32 -> uint16: round to nearest (ties to even), DC shift, clamp to the P-bit range; modulo 2^16."""
    v = np.rint(np.clip(plane, F(-131072.0), F(131072.0))).astype(np.int64)
    if signed:
        s = np.clip(v, -(1 << (P - 1)), (1 << (P - 1)) - 1)
    else:
        s = np.clip(v + (1 << (P - 1)), 0, (1 << P) - 1)
    return (s & 0xFFFF).astype(np.uint16)


def decode_frame(fr, passes=None):
    """A Frame of either transform -> (uint16 [rows][cols], ok)."""
    if fr.transform == 1:
        assert passes is None
        return R.decode_frame(fr)
    plane, ok = reconstruct(fr, passes)
    return samples(plane, fr.precision, fr.signed), ok
