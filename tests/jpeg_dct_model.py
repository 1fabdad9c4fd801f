"""Numpy / plain-Python model of the sequential DCT JPEG decode (ITU T.81 Annex F.2.2, one component, Huffman) as libjpeg performs
it by default: the coefficient decode with its zig-zag state and DC prediction, dequantisation in wide integers, the `JDCT_ISLOW`
inverse DCT of jidctint.c (CONST_BITS 13, PASS1_BITS 2 at P = 8 and 1 at P = 12, DESCALE rounding half up), the level shift and
the range limit.  Written from T.81 and the published libjpeg sources; it shares no code with boa_hip/jpeg_dct.py.  Pinned
against libjpeg-turbo's pixels at both sample depths by tests/golden/jpeg_dct (tests/test_dicom_jpeg_dct_cpu.py)."""
import struct

import numpy as np

OK, TRUNCATED, INVALID_CODE, RUN_PAST_BLOCK, BAD_SSSS, TRAILING = 0, 1, 2, 3, 4, 5

# natural (row-major) index of the coefficient at zig-zag position k (T.81 figure A.6)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

CONST_BITS = 13
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def pass1_bits(P):
    return 2 if P == 8 else 1


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(v, shift):
    """One 1-D islow pass over the last axis of int64 [..., 8]."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (v[..., k] for k in range(8))
    z1 = (i2 + i6) * F_0_541
    tmp2 = z1 - i6 * F_1_847
    tmp3 = z1 + i2 * F_0_765
    tmp0 = (i0 + i4) << CONST_BITS
    tmp1 = (i0 - i4) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3], axis=-1)
    return _descale(out, shift)


def range_limit(x, P):
    """libjpeg's range-limit table, indexed by x & (4 MAX + 3) after the final descale (x: level shift not yet applied)."""
    mx = (1 << P) - 1
    centre = (mx + 1) // 2
    i = np.asarray(x, dtype=np.int64) & (4 * mx + 3)
    return np.where(i < centre, i + centre, np.where(i < 2 * (mx + 1), mx, np.where(i < 4 * (mx + 1) - centre, 0,
                                                                                   i - (4 * (mx + 1) - centre))))


def idct_blocks(coef, qt, P):
    """coef: int [n, 64] quantised coefficients in natural order, qt: [64] natural order -> samples int64 [n, 8, 8]."""
    pb = pass1_bits(P)
    w = (np.asarray(coef, dtype=np.int64) * np.asarray(qt, dtype=np.int64)).reshape(-1, 8, 8)
    ws = _pass(w.transpose(0, 2, 1), CONST_BITS - pb).transpose(0, 2, 1)      # pass 1: columns
    return range_limit(_pass(ws, CONST_BITS + pb + 3), P)                      # pass 2: rows


def assemble(blocks, rows, cols):
    """[n, 8, 8] blocks in raster order of the padded image -> [rows, cols]."""
    bh, bw = -(-rows // 8), -(-cols // 8)
    return blocks.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:rows, :cols]


def pixels(coef, qt, P, rows, cols):
    return assemble(idct_blocks(coef, qt, P), rows, cols).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------- the stream

def parse(stream):
    """A one-component, one-scan sequential stream -> dict(P, rows, cols, qt [64] natural order, dc / ac = (counts, values),
    ri, segments = the un-stuffed bytes of each restart interval, dht = every table as {(class, id): (counts, values)})."""
    b = bytes(stream)
    assert b[:2] == b"\xFF\xD8"
    pos, qts, dht, out = 2, {}, {}, {"ri": 0}
    while True:
        assert b[pos] == 0xFF
        m = b[pos + 1]
        ln = struct.unpack_from(">H", b, pos + 2)[0]
        body = b[pos + 4:pos + 2 + ln]
        pos += 2 + ln
        if m == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                n = 128 if pq else 64
                q = np.frombuffer(body[k + 1:k + 1 + n], dtype=">u2" if pq else np.uint8).astype(np.int64)
                nat = np.zeros(64, dtype=np.int64)
                nat[ZIGZAG] = q
                qts[tq] = nat
                k += 1 + n
        elif m == 0xC4:
            k = 0
            while k < len(body):
                counts = bytes(body[k + 1:k + 17])
                n = sum(counts)
                dht[(body[k] >> 4, body[k] & 15)] = (counts, bytes(body[k + 17:k + 17 + n]))
                k += 17 + n
        elif m in (0xC0, 0xC1):
            out["P"], out["rows"], out["cols"], nf = body[0], *struct.unpack_from(">HH", body, 1), body[5]
            assert nf == 1
            out["sof"] = m
            tq = body[8]
        elif m == 0xDD:
            out["ri"] = struct.unpack(">H", body)[0]
        elif m == 0xDA:
            td, ta = body[2] >> 4, body[2] & 15
            break
    out["qt"], out["dc"], out["ac"], out["dht"] = qts[tq], dht[(0, td)], dht[(1, ta)], dht
    segs, cur, i = [], bytearray(), pos
    while True:
        c = b[i]
        if c != 0xFF:
            cur.append(c)
            i += 1
        elif b[i + 1] == 0:
            cur.append(0xFF)
            i += 2
        elif 0xD0 <= b[i + 1] <= 0xD7:
            segs.append(bytes(cur))
            cur = bytearray()
            i += 2
        elif b[i + 1] == 0xFF:
            i += 1
        else:
            break
    segs.append(bytes(cur))
    out["segments"] = segs
    return out


def _codebook(counts, values):
    book, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            book[(length, code)] = values[k]
            code += 1
            k += 1
        code <<= 1
    return book


class _Bits:
    def __init__(self, data):
        self.d, self.n, self.pos = data, 8 * len(data), 0

    def peek(self, n):                      # n <= 16 bits at pos, 1 bits past the end
        by = self.pos >> 3
        w = int.from_bytes((self.d[by:by + 4] + b"\xFF\xFF\xFF\xFF")[:4], "big")
        return (w >> (32 - (self.pos & 7) - n)) & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n) if n else 0
        self.pos += n
        return v


def _symbol(br, book):
    """-> (symbol, status): the status tells a code cut off by the segment's end from one no table holds."""
    for length in range(1, 17):
        v = book.get((length, br.peek(length)))
        if v is not None:
            if br.pos + length > br.n:
                return None, TRUNCATED
            br.pos += length
            return v, OK
    return None, INVALID_CODE if br.pos + 16 <= br.n else TRUNCATED


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def decode_coefficients(p, steps=None):
    """parse() output -> (int32 [blocks, 64] natural-order quantised coefficients with the DC prediction undone, status).
    steps: a list that receives (segment, bit position, k, length, next k, zig-zag position written or -1, value) of every
    codeword, for the comparison with the device helpers' codeword step."""
    rows, cols, P = p["rows"], p["cols"], p["P"]
    nb = -(-rows // 8) * -(-cols // 8)
    ri = p["ri"] or nb
    coef = np.zeros((nb, 64), dtype=np.int32)
    dcb, acb = _codebook(*p["dc"]), _codebook(*p["ac"])
    dc_max, ac_max = (11, 10) if P == 8 else (15, 14)
    if len(p["segments"]) != -(-nb // ri):
        return coef, TRUNCATED
    for si, seg in enumerate(p["segments"]):
        br, pred = _Bits(seg), 0
        for blk in range(si * ri, min(si * ri + ri, nb)):
            k = 0
            while k < 64:
                at = br.pos
                sym, st = _symbol(br, acb if k else dcb)
                if st:
                    return coef, st
                if k == 0:
                    s, run, zz = sym, 0, 0
                    if s > dc_max:
                        return coef, BAD_SSSS
                else:
                    run, s = sym >> 4, sym & 15
                    if s > ac_max:
                        return coef, BAD_SSSS
                    if s == 0:
                        if run == 15:
                            if k + 16 > 64:
                                return coef, RUN_PAST_BLOCK
                            if steps is not None:
                                steps.append((si, at, k, br.pos - at, (k + 16) & 63, -1, 0))
                            k += 16
                            continue
                        if run:
                            return coef, INVALID_CODE          # EOBn belongs to the progressive processes
                        if steps is not None:
                            steps.append((si, at, k, br.pos - at, 0, -1, 0))
                        break
                    zz = k + run
                    if zz > 63:
                        return coef, RUN_PAST_BLOCK
                if br.pos + s > br.n:
                    return coef, TRUNCATED
                v = _extend(br.take(s), s)
                if k == 0:
                    pred += v
                    coef[blk, 0] = pred
                else:
                    coef[blk, ZIGZAG[zz]] = v
                if steps is not None:
                    steps.append((si, at, k, br.pos - at, (zz + 1) & 63, zz, v))
                k = zz + 1
        if br.n - br.pos >= 8:
            return coef, TRAILING
    return coef, OK


def decode(stream):
    """-> (uint16 [rows, cols] pixels as libjpeg decodes them, status)."""
    p = parse(stream)
    coef, st = decode_coefficients(p)
    return pixels(coef, p["qt"], p["P"], p["rows"], p["cols"]), st
