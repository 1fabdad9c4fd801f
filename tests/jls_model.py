"""Test-only JPEG-LS (ITU-T T.87) decoder in plain Python: the model of the decoding rule that boa_hip's kernels follow
(include/boa_hip.h, boa_jls_decode; csrc/jls_codes.h), written from the standard and pinned against CharLS (tests/golden/jls).
`decode_scan` takes the scan's bytes and the resolved parameters and returns the samples, the status and what the scan exercised
(escape codes, the highest RUNindex, C at a clamp, N at RESET); `decode_stream` reads the markers of a whole stream first."""
import struct

import numpy as np

OK, TRUNCATED, INVALID = 0, 1, 2
J = [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 9, 10, 11, 12, 13, 14, 15]


def _clamp_t(i, j, maxval):
    return j if (i > maxval or i < j) else i


def default_thresholds(maxval, near):
    """T.87 C.2.4.1.1.1 -> (T1, T2, T3)."""
    if maxval >= 128:
        f = (min(maxval, 4095) + 128) // 256
        t1 = _clamp_t(f * (3 - 2) + 2 + 3 * near, near + 1, maxval)
        t2 = _clamp_t(f * (7 - 3) + 3 + 5 * near, t1, maxval)
        t3 = _clamp_t(f * (21 - 4) + 4 + 7 * near, t2, maxval)
    else:
        f = 256 // (maxval + 1)
        t1 = _clamp_t(max(2, 3 // f + 3 * near), near + 1, maxval)
        t2 = _clamp_t(max(3, 7 // f + 5 * near), t1, maxval)
        t3 = _clamp_t(max(4, 21 // f + 7 * near), t2, maxval)
    return t1, t2, t3


class Params:
    def __init__(self, maxval, near=0, t1=0, t2=0, t3=0, reset=0):
        d = default_thresholds(maxval, near)
        self.maxval, self.near = maxval, near
        self.t1, self.t2, self.t3, self.reset = t1 or d[0], t2 or d[1], t3 or d[2], reset or 64
        self.step = 2 * near + 1
        self.range = (maxval + 2 * near) // self.step + 1
        self.qbpp = (self.range - 1).bit_length()
        self.bpp = max(2, maxval.bit_length())
        self.limit = 2 * (self.bpp + max(8, self.bpp))
        self.a0 = max(2, (self.range + 32) // 64)
        self.wrap = self.range * self.step

    def words(self):
        return [self.maxval, self.near, self.t1, self.t2, self.t3, self.reset]


class Bits:
    """The stuffed bit stream: after a 0xFF byte the next byte carries 7 bits, a byte >= 0x80 there ends the stream; zero bits
    behind the end, `over` once a read took one of them."""

    def __init__(self, scan: bytes):
        a = np.frombuffer(bytes(scan), dtype=np.uint8)
        after_ff = np.concatenate([[False], a[:-1] == 0xFF]) if len(a) else np.zeros(0, dtype=bool)
        marker = np.flatnonzero(after_ff & (a >= 0x80))
        if len(marker):
            a, after_ff = a[:marker[0]], after_ff[:marker[0]]
        bits = np.unpackbits(a).reshape(-1, 8)
        keep = np.ones_like(bits, dtype=bool)
        keep[after_ff, 0] = False
        flat = bits[keep]
        self.total = len(flat)
        self.buf = np.packbits(np.concatenate([flat, np.zeros(256, dtype=np.uint8)])).tobytes() + bytes(16)
        self.pos = 0
        self.over = False

    def peek64(self):
        i, s = self.pos >> 3, self.pos & 7
        if i + 9 > len(self.buf):
            return 0
        return (int.from_bytes(self.buf[i:i + 9], "big") >> (8 - s)) & 0xFFFFFFFFFFFFFFFF

    def skip(self, k):
        self.pos += k
        if self.pos > self.total:
            self.over = True

    def take(self, k):
        v = self.peek64() >> (64 - k) if k else 0
        self.skip(k)
        return v


def quantise(d, p):
    if d <= -p.t3:
        return -4
    if d <= -p.t2:
        return -3
    if d <= -p.t1:
        return -2
    if d < -p.near:
        return -1
    if d <= p.near:
        return 0
    if d < p.t1:
        return 1
    if d < p.t2:
        return 2
    if d < p.t3:
        return 3
    return 4


def fix(x, p):
    if x < -p.near:
        x += p.wrap
    elif x > p.maxval + p.near:
        x -= p.wrap
    return min(max(x, 0), p.maxval)


def golomb_k(n, a):
    k = 0
    while (n << k) < a:
        k += 1
    return k


class _Bad(Exception):
    pass


def _golomb(b, p, k, glimit, stats):
    qmax = glimit - p.qbpp - 1
    w = b.peek64()
    z = 64 - w.bit_length()
    if z > qmax:
        if b.total - b.pos < qmax + 1:
            b.over = True
        raise _Bad()
    b.skip(z + 1)
    if z == qmax:
        stats["escapes"] += 1
        v = b.take(p.qbpp) + 1
    else:
        v = (z << k) | b.take(k)
    if v > p.range:
        raise _Bad()
    return v


def decode_scan(scan: bytes, rows: int, cols: int, p: Params):
    """-> (uint16 [rows, cols], status, stats); the samples of a failed scan are what was decoded, zero filled."""
    b = Bits(scan)
    A = [p.a0] * 367
    B = [0] * 367
    C = [0] * 367
    N = [1] * 367
    stats = {"escapes": 0, "max_runindex": 0, "c_clamped": False, "n_reset": False, "runs": 0}
    out = np.zeros((rows, cols), dtype=np.uint16)
    ri, corner, bad = 0, 0, False
    prev = [0] * (cols + 1)
    near, reset, maxval, step = p.near, p.reset, p.maxval, p.step
    try:
        for r in range(rows):
            cur = [0] * (cols + 1)
            prev[cols] = prev[cols - 1]
            ra, rc, x = prev[0], corner, 0
            corner = prev[0]
            try:
                while x < cols:
                    rb, rd = prev[x], prev[x + 1]
                    d1, d2, d3 = rd - rb, rb - rc, rc - ra
                    if abs(d1) <= near and abs(d2) <= near and abs(d3) <= near:
                        stats["runs"] += 1
                        x0, more = x, True
                        while more and x < cols:
                            more = b.take(1) != 0
                            if more:
                                cnt = min(1 << J[ri], cols - x)
                                x += cnt
                                if cnt == 1 << J[ri] and ri < 31:
                                    ri += 1
                                    stats["max_runindex"] = max(stats["max_runindex"], ri)
                        if not more:
                            x += b.take(J[ri]) if J[ri] else 0
                            if x > cols:
                                cur[x0:cols] = [ra] * (cols - x0)
                                raise _Bad()
                        cur[x0:x] = [ra] * (x - x0)
                        if x >= cols:
                            break
                        rb = prev[x]
                        t = 1 if abs(ra - rb) <= near else 0
                        q = 365 + t
                        temp = A[q] + ((N[q] >> 1) if t else 0)
                        k = golomb_k(N[q], temp)
                        m = _golomb(b, p, k, p.limit - J[ri] - 1, stats)
                        tm = m + t
                        ea = (tm + 1) >> 1
                        e = -ea if ((k != 0 or 2 * B[q] >= N[q]) == bool(tm & 1)) else ea
                        if e < 0:
                            B[q] += 1
                        A[q] += (m + 1 - t) >> 1
                        if N[q] == reset:
                            A[q] >>= 1
                            B[q] >>= 1
                            N[q] >>= 1
                            stats["n_reset"] = True
                        N[q] += 1
                        rx = fix(ra + e * step, p) if t else fix(rb + (e if rb >= ra else -e) * step, p)
                        if ri > 0:
                            ri -= 1
                    else:
                        qs = 81 * quantise(d1, p) + 9 * quantise(d2, p) + quantise(d3, p)
                        sign, q = (-1, -qs) if qs < 0 else (1, qs)
                        px = min(ra, rb) if rc >= max(ra, rb) else max(ra, rb) if rc <= min(ra, rb) else ra + rb - rc
                        px = min(max(px + sign * C[q], 0), maxval)
                        k = golomb_k(N[q], A[q])
                        m = _golomb(b, p, k, p.limit, stats)
                        if near == 0 and k == 0 and 2 * B[q] <= -N[q]:
                            e = (m - 1) >> 1 if m & 1 else -(m >> 1) - 1
                        else:
                            e = -((m + 1) >> 1) if m & 1 else m >> 1
                        B[q] += e * step
                        A[q] += abs(e)
                        if N[q] == reset:
                            A[q] >>= 1
                            B[q] >>= 1
                            N[q] >>= 1
                            stats["n_reset"] = True
                        N[q] += 1
                        if B[q] <= -N[q]:
                            B[q] += N[q]
                            if C[q] > -128:
                                C[q] -= 1
                            if B[q] <= -N[q]:
                                B[q] = -N[q] + 1
                        elif B[q] > 0:
                            B[q] -= N[q]
                            if C[q] < 127:
                                C[q] += 1
                            if B[q] > 0:
                                B[q] = 0
                        if C[q] in (-128, 127):
                            stats["c_clamped"] = True
                        rx = fix(px + sign * e * step, p)
                    cur[x] = rx
                    ra, rc = rx, rb
                    x += 1
            finally:
                out[r] = cur[:cols]
            prev = cur
    except _Bad:
        bad = True
    return out, (TRUNCATED if b.over else INVALID if bad else OK), stats


def scan_of(stream: bytes):
    """A whole JPEG-LS stream -> (scan bytes, rows, cols, Params): the markers as a lenient reader takes them (test streams)."""
    pos, lse, sof, near = 2, {}, None, 0
    assert stream[:2] == b"\xFF\xD8"
    while True:
        assert stream[pos] == 0xFF
        m = stream[pos + 1]
        ln = struct.unpack_from(">H", stream, pos + 2)[0]
        body = stream[pos + 4:pos + 2 + ln]
        pos += 2 + ln
        if m == 0xF7:
            sof = (body[0],) + struct.unpack_from(">HH", body, 1)
        elif m == 0xF8 and body[0] == 1:
            lse = dict(zip(("maxval", "t1", "t2", "t3", "reset"), struct.unpack_from(">5H", body, 1)))
        elif m == 0xDA:
            near = body[1 + 2 * body[0]]
            break
    a = np.frombuffer(stream, dtype=np.uint8, offset=pos)
    end = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] >= 0x80))[0]
    p = Params(lse.get("maxval") or (1 << sof[0]) - 1, near, lse.get("t1", 0), lse.get("t2", 0), lse.get("t3", 0), lse.get("reset", 0))
    return stream[pos:pos + end], sof[1], sof[2], p


def decode_stream(stream: bytes):
    scan, rows, cols, p = scan_of(stream)
    return decode_scan(scan, rows, cols, p)
