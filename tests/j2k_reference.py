"""Test-only JPEG 2000 tier-1 (T.800 Annexes C and D: MQ decoder, the three coding passes) and inverse reversible 5/3 (Annex F)
in plain Python / numpy, written from the standard.  It consumes the host code-block table of boa_hip.jpeg2000 (parse_frame
and tier-2), so that the host side is proven on a machine without a GPU, and it is the model csrc/j2k.hip follows."""
import numpy as np

# Table C.2: Qe, NMPS, NLPS, SWITCH
MQ_TABLE = [
    (0x5601, 1, 1, 1), (0x3401, 2, 6, 0), (0x1801, 3, 9, 0), (0x0AC1, 4, 12, 0), (0x0521, 5, 29, 0), (0x0221, 38, 33, 0),
    (0x5601, 7, 6, 1), (0x5401, 8, 14, 0), (0x4801, 9, 14, 0), (0x3801, 10, 14, 0), (0x3001, 11, 17, 0), (0x2401, 12, 18, 0),
    (0x1C01, 13, 20, 0), (0x1601, 29, 21, 0), (0x5601, 15, 14, 1), (0x5401, 16, 14, 0), (0x5101, 17, 15, 0),
    (0x4801, 18, 16, 0), (0x3801, 19, 17, 0), (0x3401, 20, 18, 0), (0x3001, 21, 19, 0), (0x2801, 22, 19, 0),
    (0x2401, 23, 20, 0), (0x2201, 24, 21, 0), (0x1C01, 25, 22, 0), (0x1801, 26, 23, 0), (0x1601, 27, 24, 0),
    (0x1401, 28, 25, 0), (0x1201, 29, 26, 0), (0x1101, 30, 27, 0), (0x0AC1, 31, 28, 0), (0x09C1, 32, 29, 0),
    (0x08A1, 33, 30, 0), (0x0521, 34, 31, 0), (0x0441, 35, 32, 0), (0x02A1, 36, 33, 0), (0x0221, 37, 34, 0),
    (0x0141, 38, 35, 0), (0x0111, 39, 36, 0), (0x0085, 40, 37, 0), (0x0049, 41, 38, 0), (0x0025, 42, 39, 0),
    (0x0015, 43, 40, 0), (0x0009, 44, 41, 0), (0x0005, 45, 42, 0), (0x0001, 45, 43, 0), (0x5601, 46, 46, 0)]
CX_RL, CX_UNI = 17, 18

# flag word per coefficient (as in the kernel): neighbour significance NW N NE W E SW S SE = bits 0-7, signs of the N W E S
# neighbours = bits 8-11, own significance 12, visited in this plane's significance pass 13, refined 14, own sign 15
SIG, VIS, REF, NEG = 1 << 12, 1 << 13, 1 << 14, 1 << 15


def zc_context(nb, orient):
    """Table D.1: zero-coding context of the neighbour-significance bits, orientation 0 LL, 1 HL, 2 LH, 3 HH."""
    h = ((nb >> 3) & 1) + ((nb >> 4) & 1)
    v = ((nb >> 1) & 1) + ((nb >> 6) & 1)
    d = (nb & 1) + ((nb >> 2) & 1) + ((nb >> 5) & 1) + ((nb >> 7) & 1)
    if orient == 1:
        h, v = v, h
    if orient == 3:
        hv = h + v
        if d >= 3:
            return 8
        if d == 2:
            return 7 if hv >= 1 else 6
        if d == 1:
            return 5 if hv >= 2 else 4 if hv == 1 else 3
        return 2 if hv >= 2 else 1 if hv == 1 else 0
    if h == 2:
        return 8
    if h == 1:
        return 7 if v >= 1 else 6 if d >= 1 else 5
    if v == 2:
        return 4
    if v == 1:
        return 3
    return 2 if d >= 2 else 1 if d == 1 else 0


def sc_context(f):
    """Tables D.2 / D.3: (sign context, XOR bit) of a flag word."""
    def contrib(sig, neg):
        return 0 if not sig else (-1 if neg else 1)
    h = contrib(f >> 3 & 1, f >> 9 & 1) + contrib(f >> 4 & 1, f >> 10 & 1)
    v = contrib(f >> 1 & 1, f >> 8 & 1) + contrib(f >> 6 & 1, f >> 11 & 1)
    h, v = max(-1, min(1, h)), max(-1, min(1, v))
    if h < 0:
        h, v, x = -h, -v, 1
    else:
        x = 0
        if h == 0 and v < 0:
            v, x = 1, 1
    return {(1, 1): 13, (1, 0): 12, (1, -1): 11, (0, 1): 10, (0, 0): 9}[(h, v)], x


ZC = [[zc_context(nb, o) for nb in range(256)] for o in range(4)]
SC = [sc_context(f) for f in range(1 << 12)]


class MQ:
    """Annex C decoder (C.3, software conventions); bytes at or past `end` read as 0xFF."""

    def __init__(self, data, start, end):
        self.d, self.bp, self.end = data, start, end
        self.idx = [0] * 19
        self.mps = [0] * 19
        self.idx[0], self.idx[CX_RL], self.idx[CX_UNI] = 4, 3, 46
        self.c = self.byte(self.bp) << 16
        self.ct = 0
        self.bytein()
        self.c = (self.c << 7) & 0xFFFFFFFF
        self.ct -= 7
        self.a = 0x8000

    def byte(self, p):
        return self.d[p] if p < self.end else 0xFF

    def bytein(self):
        if self.byte(self.bp) == 0xFF:
            b1 = self.byte(self.bp + 1)
            if b1 > 0x8F:
                self.c += 0xFF00
                self.ct = 8
            else:
                self.bp += 1
                self.c += b1 << 9
                self.ct = 7
        else:
            self.bp += 1
            self.c += self.byte(self.bp) << 8
            self.ct = 8
        self.c &= 0xFFFFFFFF

    def decode(self, cx):
        qe, nmps, nlps, sw = MQ_TABLE[self.idx[cx]]
        self.a -= qe
        if (self.c >> 16) < qe:
            if self.a < qe:
                d = self.mps[cx]
                self.idx[cx] = nmps
            else:
                d = 1 - self.mps[cx]
                if sw:
                    self.mps[cx] = 1 - self.mps[cx]
                self.idx[cx] = nlps
            self.a = qe
        else:
            self.c -= qe << 16
            if self.a & 0x8000:
                return self.mps[cx]
            if self.a < qe:
                d = 1 - self.mps[cx]
                if sw:
                    self.mps[cx] = 1 - self.mps[cx]
                self.idx[cx] = nlps
            else:
                d = self.mps[cx]
                self.idx[cx] = nmps
        while True:                                   # RENORMD
            if self.ct == 0:
                self.bytein()
            self.a <<= 1
            self.c = (self.c << 1) & 0xFFFFFFFF
            self.ct -= 1
            if self.a & 0x8000:
                break
        return d


def decode_block(data, start, length, w, h, orient, numbps, passes, with_last=False):
    """One code block -> (int64 [h][w] signed coefficients, ok).  ok False: more passes than bit-planes, or beyond 30 bits.
    A block that stops before its last pass (passes < 3 * numbps - 2: a rate- or quality-limited layer) is reconstructed as
    OpenJPEG does: a significant coefficient whose lowest coded plane b_last (the plane where it became significant or was
    last refined) is >= 1 lies at the midpoint of what is left open, |v| = m + 2^(b_last - 1); b_last = 0 leaves m.
    with_last: (coefficients, b_last [h][w], -1 where not significant, ok)."""
    out = np.zeros((h, w), dtype=np.int64)
    if passes == 0:
        return (out, out - 1, True) if with_last else (out, True)
    if numbps < 1 or numbps > 30 or passes > 3 * numbps - 2:
        return (out, out - 1, False) if with_last else (out, False)
    W2 = w + 2
    F = [0] * (W2 * (h + 2))
    V = [0] * (W2 * (h + 2))
    B = [-1] * (W2 * (h + 2))                          # lowest plane at which the coefficient was coded
    mq = MQ(data, start, start + length)
    zc = ZC[orient]
    nbr = ((-W2 - 1, 1 << 7, 0), (-W2, 1 << 6, 1 << 11), (-W2 + 1, 1 << 5, 0), (-1, 1 << 4, 1 << 10), (1, 1 << 3, 1 << 9),
           (W2 - 1, 1 << 2, 0), (W2, 1 << 1, 1 << 8), (W2 + 1, 1, 0))

    def set_sig(i, neg):
        F[i] |= SIG | (NEG if neg else 0)
        for o, s, sg in nbr:
            F[i + o] |= s | (sg if neg else 0)

    def sign(i):
        ctx, x = SC[F[i] & 0xFFF]
        return mq.decode(ctx) ^ x

    for k in range(passes):
        kind = 2 if k == 0 else (k - 1) % 3            # 0 significance propagation, 1 refinement, 2 cleanup
        plane = numbps - 1 - (k + 2) // 3
        bit = 1 << plane
        for y0 in range(0, h, 4):
            y1 = min(y0 + 4, h)
            for x in range(w):
                y = y0
                if kind == 2 and y1 - y0 == 4:
                    i0 = (y0 + 1) * W2 + x + 1
                    if not any(F[i0 + j * W2] & (SIG | VIS | 0xFF) for j in range(4)):
                        if not mq.decode(CX_RL):
                            continue
                        r = mq.decode(CX_UNI) << 1
                        r |= mq.decode(CX_UNI)
                        i = i0 + r * W2
                        neg = sign(i)
                        set_sig(i, neg)
                        V[i] = -bit if neg else bit
                        B[i] = plane
                        y = y0 + r + 1
                for yy in range(y, y1):
                    i = (yy + 1) * W2 + x + 1
                    f = F[i]
                    if kind == 0:
                        if not f & SIG and f & 0xFF:
                            if mq.decode(zc[f & 0xFF]):
                                neg = sign(i)
                                set_sig(i, neg)
                                V[i] = -bit if neg else bit
                                B[i] = plane
                            F[i] |= VIS
                    elif kind == 1:
                        if f & SIG and not f & VIS:
                            ctx = 16 if f & REF else (15 if f & 0xFF else 14)
                            if mq.decode(ctx):
                                V[i] += -bit if V[i] < 0 else bit
                            B[i] = plane
                            F[i] |= REF
                    else:
                        if not f & (SIG | VIS):
                            if mq.decode(zc[f & 0xFF]):
                                neg = sign(i)
                                set_sig(i, neg)
                                V[i] = -bit if neg else bit
                                B[i] = plane
                        F[i] &= ~VIS
    out[:] = np.asarray(V, dtype=np.int64).reshape(h + 2, W2)[1:-1, 1:-1]
    last = np.asarray(B, dtype=np.int64).reshape(h + 2, W2)[1:-1, 1:-1]
    if passes < 3 * numbps - 2:
        half = np.where(last >= 1, 1 << np.maximum(last - 1, 0), 0)
        out += np.sign(out) * half
    return (out, last, True) if with_last else (out, True)


def idwt53_1d(y, axis):
    """Inverse reversible 5/3 along `axis` of an array in Mallat order (low half first), zero origin."""
    y = np.moveaxis(np.asarray(y, dtype=np.int64), axis, 0)
    n = y.shape[0]
    if n == 1:
        return np.moveaxis(y.copy(), 0, axis)
    nl, nh = (n + 1) // 2, n // 2
    L, H = y[:nl], y[nl:]
    k = np.arange(nl)
    he = (H[np.maximum(k - 1, 0)] + H[np.minimum(k, nh - 1)] + 2) >> 2
    X = np.empty_like(y)
    X[0::2] = L - he
    ko = np.arange(nh)
    X[1::2] = H + ((X[0::2][ko] + X[0::2][np.minimum(ko + 1, nl - 1)]) >> 1)
    return np.moveaxis(X, 0, axis)


def reconstruct(fr):
    """A boa_hip.jpeg2000.Frame -> (int64 [rows][cols], the inverse transform's output before the DC shift and the clamp; ok)."""
    plane = np.zeros((fr.rows, fr.cols), dtype=np.int64)
    data = fr.data
    off, ok = 0, True
    for o, x0, y0, w, h, nbp, npass, ln in fr.blocks.tolist():
        blk, good = decode_block(data, off, ln, w, h, o, nbp, npass)
        ok = ok and good
        plane[y0:y0 + h, x0:x0 + w] = blk
        off += ln
    for r in range(1, fr.levels + 1):
        d = fr.levels - r
        hr, wr = -(-fr.rows >> d), -(-fr.cols >> d)
        reg = idwt53_1d(plane[:hr, :wr], 1)
        plane[:hr, :wr] = idwt53_1d(reg, 0)
    return plane, ok


def decode_frame(fr):
    """A boa_hip.jpeg2000.Frame -> (uint16 [rows][cols], the sample modulo 2^16 after the clamp to its range; ok)."""
    plane, ok = reconstruct(fr)
    P = fr.precision
    if fr.signed:
        s = np.clip(plane, -(1 << (P - 1)), (1 << (P - 1)) - 1)
    else:
        s = np.clip(plane + (1 << (P - 1)), 0, (1 << P) - 1)
    return (s & 0xFFFF).astype(np.uint16), ok
