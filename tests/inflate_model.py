"""Plain-Python restatement of the device inflate (csrc/inflate.hip, csrc/inflate_codes.h): the block-start test of the find pass, a
full inflate that records the true block boundaries, the chunk table with its chain walk, the decode of a chunk into 16-bit symbols
with markers for the unknown 32 KiB in front of it, and the chain of windows that turns them into bytes.  Also the streams that the
CPU and the GPU tests share.  Slow and obvious on purpose; zlib is the judge of the model, the model is the judge of the C code."""
import struct
import zlib

import numpy as np

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
WINDOW = 32768
NO_STOP = 1 << 64


class Invalid(Exception):
    """The stream is not deflate at this point (args[0]: "truncated", "invalid" or "far")."""


class Bits:
    def __init__(self, data, pos=0):
        self.data, self.pos, self.nbits = data, pos, 8 * len(data)

    def peek(self, n):                 # n <= 24; bits past the end read as zero
        i = self.pos >> 3
        return (int.from_bytes(self.data[i:i + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def get(self, n):
        v = self.peek(n)
        self.pos += n
        return v

    def check(self):
        if self.pos > self.nbits:
            raise Invalid("truncated")


def counts_ok(lens, allow_incomplete, allow_empty):
    """zlib's inflate_table on a set of code lengths: over-subscribed = invalid; incomplete = invalid unless it is one code of one
    bit (or, for the distance code, no code at all)."""
    count = [0] * 16
    for ln in lens:
        count[ln] += 1
    left, used = 1, sum(count[1:])
    for ln in range(1, 16):
        left = (left << 1) - count[ln]
        if left < 0:
            return False
    if left == 0:
        return True
    if used == 0:
        return allow_empty
    return allow_incomplete and used == 1 and count[1] == 1


def decode_table(lens):
    """(table indexed by the next `maxbits` stream bits -> (length, symbol) or None, maxbits) of a canonical code."""
    maxbits = max(max(lens), 1)
    table = [None] * (1 << maxbits)
    code, prev = 0, 0
    for ln, sym in sorted((ln, s) for s, ln in enumerate(lens) if ln):
        code <<= ln - prev
        prev = ln
        rev = int(format(code, f"0{ln}b")[::-1], 2)
        table[rev::1 << ln] = [(ln, sym)] * (1 << (maxbits - ln))
        code += 1
    return table, maxbits


def symbol(b, tm):
    table, maxbits = tm
    e = table[b.peek(maxbits)]
    if e is None:
        raise Invalid("invalid")
    b.pos += e[0]
    return e[1]


def dynamic_header(b):
    """The header of a dynamic block after its three block bits -> (literal/length lengths, distance lengths)."""
    hlit, hdist, hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
    if hlit > 286 or hdist > 30:
        raise Invalid("invalid")
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = b.get(3)
    b.check()
    if not counts_ok(cl, False, False):
        raise Invalid("invalid")
    tm = decode_table(cl)
    lens = []
    total = hlit + hdist
    while len(lens) < total:
        b.check()
        s = symbol(b, tm)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise Invalid("invalid")
            val, rep = lens[-1], 3 + b.get(2)
        elif s == 17:
            val, rep = 0, 3 + b.get(3)
        else:
            val, rep = 0, 11 + b.get(7)
        if len(lens) + rep > total:
            raise Invalid("invalid")
        lens += [val] * rep
    b.check()
    ll, d = lens[:hlit], lens[hlit:]
    if ll[256] == 0 or not counts_ok(ll, True, False) or not counts_ok(d, True, True):
        raise Invalid("invalid")
    return ll, d


def block_start(body, bit):
    """The find pass's test: a dynamic, non-final block header that the decoder accepts starts at `bit`."""
    if bit + 17 > 8 * len(body):
        return False
    b = Bits(body, bit)
    if b.get(3) != 4:
        return False
    try:
        dynamic_header(b)
    except Invalid:
        return False
    return True


FIXED = ([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30)


def decode(body, start=0, stop=NO_STOP, markers=False, boundaries=None):
    """Blocks of `body` from bit `start` until one ends at or beyond `stop` or the final block ends -> (output, end bit, final).
    markers=False: the output is a bytearray and a distance before the start is an error; markers=True: a list of 16-bit symbols,
    0x8000 | k for byte k of the 32 KiB in front of the start.  `boundaries` collects (bit, BTYPE, BFINAL) of every block."""
    b = Bits(body, start)
    out = [] if markers else bytearray()
    while True:
        if b.pos >= stop:
            return out, b.pos, False
        if b.pos + 3 > b.nbits:
            raise Invalid("truncated")
        if boundaries is not None:
            boundaries.append((b.pos, b.peek(3) >> 1, b.peek(3) & 1))
        hdr = b.get(3)
        btype = hdr >> 1
        if btype == 3:
            raise Invalid("invalid")
        if btype == 0:
            b.pos = (b.pos + 7) & ~7
            ln, nln = b.get(16), b.get(16)
            b.check()
            if ln != (~nln & 0xFFFF):
                raise Invalid("invalid")
            at = b.pos >> 3
            if at + ln > len(body):
                raise Invalid("truncated")
            out += body[at:at + ln]
            b.pos += 8 * ln
        else:
            ll, d = FIXED if btype == 1 else dynamic_header(b)
            tl, td = decode_table(ll), decode_table(d)
            while True:
                b.check()
                s = symbol(b, tl)
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                s -= 257
                if s >= 29:
                    raise Invalid("invalid")
                ln = LBASE[s] + b.get(LEXT[s])
                ds = symbol(b, td)
                if ds >= 30:
                    raise Invalid("invalid")
                dist = DBASE[ds] + b.get(DEXT[ds])
                b.check()
                n = len(out)
                if dist > n + (WINDOW if markers else 0):
                    raise Invalid("far")
                if dist <= n and dist >= ln:
                    out += out[n - dist:n - dist + ln]
                else:
                    for i in range(n, n + ln):
                        out.append(out[i - dist] if i >= dist else 0x8000 | (WINDOW - (dist - i)))
            b.check()
        if hdr & 1:
            return out, b.pos, True


def inflate(body):
    """-> (payload bytes, [(bit, BTYPE, BFINAL)] of every block)."""
    bounds = []
    out, end, final = decode(body, boundaries=bounds)
    if not final or (end + 7) >> 3 != len(body):
        raise Invalid("trailing")
    return bytes(out), bounds


def find_candidates(body, chunk_bytes):
    """start bit per chunk (None = no hit): chunk 0 at bit 0, chunk c the first accepted offset in [8 c chunk_bytes, 8 (c + 1) chunk_bytes)."""
    n = max(1, -(-len(body) // chunk_bytes))
    starts = [0]
    for c in range(1, n):
        lo, hi = 8 * c * chunk_bytes, min(8 * (c + 1) * chunk_bytes, 8 * len(body))
        starts.append(next((int(bit) for bit in _header_bits(body, lo, hi) if block_start(body, int(bit))), None))
    return starts


def _header_bits(body, lo, hi):
    """The offsets in [lo, hi) whose three block bits read BFINAL = 0, BTYPE = 2 (numpy: a prefilter for block_start, no verdict)."""
    bits = np.unpackbits(np.frombuffer(body, np.uint8, count=min(len(body), (hi >> 3) + 2) - (lo >> 3), offset=lo >> 3), bitorder="little")
    at = lo & 7
    n = min(hi - lo, len(bits) - at - 2)
    if n <= 0:
        return []
    w = bits[at:at + n + 2]
    return lo + np.flatnonzero((w[:n] == 0) & (w[1:n + 1] == 0) & (w[2:n + 2] == 1))


def chunked_inflate(body, chunk_bytes, starts=None):
    """The whole scheme -> (payload bytes, info).  The chain walk is the sequential form of inf_walk: a chunk whose start is not
    its true predecessor's end is a rejected candidate, and the predecessor's decode goes on in its place."""
    starts = find_candidates(body, chunk_bytes) if starts is None else starts
    live = [s for s in starts if s is not None]
    info = {"chunks": len(starts), "candidates": len(live) - 1, "rejected": 0}
    chain = []                       # (start, stop) of the chunks that decode in the end
    at = 0
    while True:
        nxt = [s for s in live if s > at]
        stop = nxt[0] if nxt else NO_STOP
        _, end, final = decode(body, at, stop, markers=True)
        chain.append((at, stop))
        info["rejected"] += sum(1 for s in nxt if s < end or final)
        if final:
            if (end + 7) >> 3 != len(body):
                raise Invalid("trailing")
            break
        at = end
    # store pass and window chain
    out = bytearray()
    for start, stop in chain:
        syms, _, _ = decode(body, start, stop, markers=True)
        window = bytes(out[-WINDOW:])
        base = WINDOW - len(window)
        for s in syms:
            if s & 0x8000:
                k = (s & 0x7FFF) - base
                if k < 0:
                    raise Invalid("far")
                out.append(window[k])
            else:
                out.append(s)
    info["live"] = len(chain)
    return bytes(out), info


# ---- the streams of the tests ----
def _deflate_raw(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None, every=3000):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if flush is None:
        return c.compress(payload) + c.flush()
    parts = []
    for lo in range(0, len(payload), every):
        parts.append(c.compress(payload[lo:lo + every]))
        parts.append(c.flush(flush))
    return b"".join(parts) + c.flush()


ENCODERS = {
    "level0": lambda p: _deflate_raw(p, 0),
    "level1": lambda p: _deflate_raw(p, 1),
    "level6": lambda p: _deflate_raw(p, 6),
    "level9": lambda p: _deflate_raw(p, 9),
    "fixed": lambda p: _deflate_raw(p, 6, zlib.Z_FIXED),
    "huffman_only": lambda p: _deflate_raw(p, 6, zlib.Z_HUFFMAN_ONLY),
    "rle": lambda p: _deflate_raw(p, 6, zlib.Z_RLE),
    "sync_flush": lambda p: _deflate_raw(p, 6, flush=zlib.Z_SYNC_FLUSH),
    "full_flush": lambda p: _deflate_raw(p, 6, flush=zlib.Z_FULL_FLUSH),
}


def _label_phantom():
    """Nested boxes of small labels in a 48 x 40 x 56 uint8 volume, as a label volume looks to a compressor."""
    v = np.zeros((48, 40, 56), np.uint8)
    rng = np.random.default_rng(3)
    for lab in range(1, 40):
        lo = rng.integers(0, (40, 32, 48))
        hi = lo + rng.integers(2, 16, 3)
        v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = lab
    return v.tobytes(order="F")


def payloads():
    from boa_hip.synthetic import ct_phantom
    rng = np.random.default_rng(17)
    block = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    return {
        "ct_phantom": ct_phantom((64, 64, 24), seed=5).tobytes(order="F"),
        "label_phantom": _label_phantom(),
        "empty": b"",
        "one_byte": b"\x2a",
        "random300k": rng.integers(0, 256, 300 * 1024, dtype=np.uint8).tobytes(),
        "zeros1m": bytes(1 << 20),
        "repeat32k": block * 12,               # distance 32768: beyond zlib's reach (32768 - 262), so zlib stores most of it
        "repeat16k": block[:16384] * 24,       # distance 16384: every match crosses the chunks, markers travel through copies of copies
    }


def gzip_wrap(body, payload, flags=0, extra=b"", name=b"", comment=b""):
    """One gzip member (RFC 1952) around a raw deflate body, with the optional header fields the flags ask for."""
    head = b"\x1f\x8b\x08" + bytes([flags]) + b"\x00\x00\x00\x00" + b"\x00\xff"
    if flags & 4:
        head += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        head += name + b"\x00"
    if flags & 16:
        head += comment + b"\x00"
    if flags & 2:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + body + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload) & 0xFFFFFFFF)


def planted_decoy():
    """(body, payload, bit offset of the decoy): incompressible data, which zlib emits as stored blocks, that holds a copy of the bytes
    of a byte-aligned dynamic non-final block (the first block after a Z_FULL_FLUSH of some compressible text)."""
    rng = np.random.default_rng(23)
    text = bytes(rng.choice(np.frombuffer(b"abcdefgh    eeeettaaoo\n", np.uint8), 6000))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    head = c.compress(text[:3000]) + c.flush(zlib.Z_FULL_FLUSH)
    tail = c.compress(text[3000:]) + c.flush(zlib.Z_FULL_FLUSH)      # a non-final dynamic block that starts on a byte
    noise = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    payload = noise[:9000] + tail + noise[9000:]
    body = _deflate_raw(payload, 6)
    at = body.find(tail[:64])
    assert at >= 0, "zlib did not store the noise"
    return body, payload, 8 * at
