"""The device deflate encoder (csrc/deflate.hip) restated on the CPU, numpy + zlib only, and a bit-level RFC 1951 reader.
  parse_blocks(body)    every block of a raw deflate stream: type, tokens, code lengths, header / payload bits, the bytes it makes
  encode_model(...)     the scheme itself: 16 KiB blocks, a greedy parse against two distances (a tie goes to the near one), per block
                        the smallest of the dynamic, fixed and stored forms (dynamic only where strictly smaller than both), an empty
                        stored block after every non-final block; code lengths of least cost within the limit (package-merge)
The helpers the GPU tests share (payloads, Huffman cost, the header's run-length rule) are here too."""
import heapq

import numpy as np

BLK = 16384
MAXLEN = 258
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


def len_symbol(length):
    """(symbol 257 .. 285, extra bits, extra value) of a match length."""
    for k in range(28, -1, -1):
        if length >= LBASE[k]:
            return 257 + k, LEXT[k], length - LBASE[k]
    raise ValueError(length)


def dist_symbol(dist):
    for k in range(29, -1, -1):
        if dist >= DBASE[k]:
            return k, DEXT[k], dist - DBASE[k]
    raise ValueError(dist)


def canonical_codes(lens):
    """RFC 1951 3.2.2: {symbol: code} of the non-zero lengths."""
    count = [0] * 17
    for ln in lens:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lens):
        if ln:
            out[s] = nxt[ln]
            nxt[ln] += 1
    return out


def kraft(lens):
    """Sum of 2^-length over the used symbols, in units of 2^-15."""
    return sum(1 << (15 - ln) for ln in lens if ln)


# ------------------------------------------------------------------------------------------------------------------ reader
class _Bits:
    def __init__(self, data):
        self.bits = np.unpackbits(np.frombuffer(bytes(data), np.uint8), bitorder="little").tolist()
        self.pos, self.n = 0, 8 * len(data)

    def take(self, k):
        assert self.pos + k <= self.n, "stream ends inside a block"
        v = 0
        for i, b in enumerate(self.bits[self.pos:self.pos + k]):
            v |= b << i
        self.pos += k
        return v


def _decoder(lens):
    """{(length, code): symbol}; an over-subscribed set of lengths is an error, an incomplete one is allowed (a single code)."""
    assert kraft(lens) <= 1 << 15, "over-subscribed code"
    return {(lens[s], c): s for s, c in canonical_codes(lens).items()}


def _symbol(bits, table):
    code = 0
    for ln in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (ln, code) in table:
            return table[(ln, code)]
    raise AssertionError("no such code")


def parse_blocks(body):
    """Every block of the raw deflate stream `body`, up to and including the final one: a list of dicts with
    type 0 / 1 / 2, final, tokens (an int per literal, (length, distance) per match), ll_lens / d_lens / cl_lens (dynamic: as the
    header gives them, HLIT / HDIST / 19 long), hlit, hdist, hclen, header_bits (everything before the first token), payload_bits
    (the tokens and the end-of-block code), start_bit / end_bit, data (the bytes the block makes)."""
    bits = _Bits(body)
    out, blocks, final = bytearray(), [], 0
    while not final:
        start = bits.pos
        final, btype = bits.take(1), bits.take(2)
        blk = {"type": btype, "final": final, "tokens": [], "start_bit": start}
        first = len(out)
        if btype == 0:
            bits.pos = (bits.pos + 7) & ~7
            ln = bits.take(16)
            assert bits.take(16) == ln ^ 0xFFFF
            lo = bits.pos // 8
            piece = bytes(body[lo:lo + ln])
            assert len(piece) == ln
            bits.pos += 8 * ln
            out += piece
            blk.update(tokens=list(piece), header_bits=bits.pos - 8 * ln - start, payload_bits=8 * ln)
        else:
            assert btype in (1, 2)
            if btype == 1:
                ll_lens, d_lens = FIXED_LL, FIXED_D
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl_lens = [0] * 19
                for k in range(hclen):
                    cl_lens[CL_ORDER[k]] = bits.take(3)
                assert kraft(cl_lens) == 1 << 15, "the code-length code must be complete"
                cl_tab, lens = _decoder(cl_lens), []
                while len(lens) < hlit + hdist:
                    s = _symbol(bits, cl_tab)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.take(2))
                    else:
                        lens += [0] * ((3 + bits.take(3)) if s == 17 else (11 + bits.take(7)))
                assert len(lens) == hlit + hdist
                ll_lens, d_lens = lens[:hlit], lens[hlit:]
                assert ll_lens[256], "no end-of-block code"
                blk.update(ll_lens=ll_lens, d_lens=d_lens, cl_lens=cl_lens, hlit=hlit, hdist=hdist, hclen=hclen)
            ll_tab = _decoder(list(ll_lens) + [0] * (288 - len(ll_lens)))
            d_tab = _decoder(list(d_lens)) if any(d_lens) else {}
            blk["header_bits"] = bits.pos - start
            tok_start = bits.pos
            while True:
                s = _symbol(bits, ll_tab)
                if s < 256:
                    out.append(s)
                    blk["tokens"].append(s)
                elif s == 256:
                    break
                else:
                    assert s <= 285
                    length = LBASE[s - 257] + bits.take(LEXT[s - 257])
                    d = _symbol(bits, d_tab)
                    assert d < 30
                    dist = DBASE[d] + bits.take(DEXT[d])
                    assert dist <= len(out), "distance before the start of the stream"
                    for _ in range(length):
                        out.append(out[-dist])
                    blk["tokens"].append((length, dist))
            blk["payload_bits"] = bits.pos - tok_start
        blk.update(end_bit=bits.pos, data=bytes(out[first:]))
        blocks.append(blk)
    assert (bits.pos + 7) // 8 == len(body), "bytes after the final block"
    return blocks


# ------------------------------------------------------------------------------------------------------------------ codes
def huffman_cost_and_depth(freqs):
    """(least cost sum f * length of a prefix code without a length limit, depth of the tree heapq builds) over the non-zero
    counts; one symbol costs one bit each.  The cost of an optimal code is unique, the depth is not."""
    f = [x for x in freqs if x]
    if len(f) == 1:
        return f[0], 1
    heap = [(x, 0) for x in f]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, da = heapq.heappop(heap)
        b, db = heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


def min_huffman_depth(freqs):
    """The least depth among the optimal unlimited codes' trees: merging the shallowest of equal weights first (Schwartz's rule,
    which the (weight, depth) heap order gives) minimises the maximum length."""
    return huffman_cost_and_depth(freqs)[1]


def limited_lengths(freqs, limit):
    """Code lengths of least cost sum f * length with every length <= limit (package-merge: Larmore & Hirschberg 1990); zero
    for the unused symbols, 1 for a single used one."""
    lens = [0] * len(freqs)
    leaves = sorted((f, s) for s, f in enumerate(freqs) if f)
    n = len(leaves)
    if n == 0:
        return lens
    if n == 1:
        lens[leaves[0][1]] = 1
        return lens
    assert (1 << limit) >= n
    cap = 2 * n - 2
    # an item is (weight, is package, index); level l = the leaves merged with the pairs of level l - 1, cut at 2 n - 2 items
    level = [(w, 0, j) for j, (w, _) in enumerate(leaves)]
    levels = [level]
    for _ in range(2, limit + 1):
        below = levels[-1]
        packs = [(below[2 * q][0] + below[2 * q + 1][0], 1, q) for q in range(len(below) // 2)]
        levels.append(sorted(level + packs)[:cap])
    take = cap
    for lv in reversed(levels):
        chosen = lv[:take]
        n_leaf = sum(1 for it in chosen if not it[1])
        for j in range(n_leaf):
            lens[leaves[j][1]] += 1
        take = 2 * (len(chosen) - n_leaf)
    assert take == 0
    return lens


def rle_lengths(seq):
    """The header's run-length code of the code lengths `seq` by zlib's greedy rule -> [(symbol, extra value)]."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        i += r
        if v:
            out.append((v, 0))
            r -= 1
        piece = 6 if v else 138
        while r >= 3:
            c = min(r, piece)
            out.append((16, c - 3) if v else (17, c - 3) if c <= 10 else (18, c - 11))
            r -= c
        out += [(v, 0)] * r
    return out


def header_plan(ll_lens, d_lens):
    """(hlit, hdist, hclen, cl_lens, rle, bits) of a dynamic block's header for these code lengths: trimmed to the last used symbol
    (HLIT >= 257, HDIST >= 1), the rule of rle_lengths over both alphabets as one sequence, the optimal 7-bit code for its symbols."""
    hlit = max(257, max(s for s, ln in enumerate(ll_lens) if ln) + 1)
    hdist = max([1] + [s + 1 for s, ln in enumerate(d_lens) if ln])
    rle = rle_lengths(list(ll_lens[:hlit]) + (list(d_lens) + [0])[:hdist])
    hist = [0] * 19
    for s, _ in rle:
        hist[s] += 1
    cl_lens = limited_lengths(hist, 7)
    hclen = max([4] + [k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]])
    bits = 3 + 5 + 5 + 4 + 3 * hclen + sum(hist[s] * (cl_lens[s] + CL_EXTRA.get(s, 0)) for s in range(19))
    return hlit, hdist, hclen, cl_lens, rle, bits


def histograms(tokens):
    ll, d, extra = [0] * 286, [0] * 30, 0
    ll[256] = 1
    for tok in tokens:
        if isinstance(tok, tuple):
            s, eb, _ = len_symbol(tok[0])
            ds, deb, _ = dist_symbol(tok[1])
            ll[s] += 1
            d[ds] += 1
            extra += eb + deb
        else:
            ll[tok] += 1
    return ll, d, extra


def fixed_bits(tokens):
    """3 header bits, the tokens in the fixed code, the 7-bit end of block."""
    ll, d, extra = histograms(tokens)
    return 3 + sum(f * FIXED_LL[s] for s, f in enumerate(ll)) + 5 * sum(d) + extra


def form_bytes(end_bit, final):
    """Bytes of a block that ends at `end_bit`: padded if final, else followed by an empty stored block (3 bits, padding, 4 bytes)."""
    return (end_bit + 7) // 8 if final else (end_bit + 3 + 7) // 8 + 4


# ------------------------------------------------------------------------------------------------------------------ the scheme
def _run_lengths(eq, block_end):
    """run[i] = number of consecutive True from i on, not past block_end[i]."""
    n = len(eq)
    stops = np.flatnonzero(~eq)
    nxt = np.full(n, n, np.int64)
    if len(stops):
        k = np.searchsorted(stops, np.arange(n))
        ok = k < len(stops)
        nxt[ok] = stops[k[ok]]
    return np.minimum(nxt, block_end) - np.arange(n)


def greedy_tokens(member, row_bytes, near_bytes):
    """The token list of every 16 KiB block of one member (bytes): at each position the longer of the matches at distance near_bytes
    and row_bytes (a tie goes to the near one), 3 .. 258 bytes, inside the block and not before the member's start; else a literal."""
    a = np.frombuffer(bytes(member), np.uint8)
    n = len(a)
    if n == 0:
        return [[]]
    idx = np.arange(n)
    block_end = np.minimum((idx // BLK + 1) * BLK, n)

    def cand(d):
        eq = np.zeros(n, bool)
        if 0 < d < n:
            eq[d:] = a[d:] == a[:-d]
        return np.minimum(_run_lengths(eq, block_end), MAXLEN)

    l1 = cand(near_bytes)
    lr = cand(row_bytes if 1 <= row_bytes <= 32768 else 0)
    far = l1 < lr
    length = np.where(far, lr, l1)
    length[length < 3] = 0
    length, far, raw = length.tolist(), far.tolist(), bytes(member)
    blocks = []
    for lo in range(0, n, BLK):
        hi, i, toks = min(lo + BLK, n), lo, []
        while i < hi:
            if length[i]:
                toks.append((length[i], row_bytes if far[i] else near_bytes))
                i += length[i]
            else:
                toks.append(raw[i])
                i += 1
        blocks.append(toks)
    return blocks


class _Writer:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        self.v |= value << self.n
        self.n += nbits

    def code(self, code, nbits):                      # Huffman codes go in most significant bit first
        self.put(int(format(code, f"0{nbits}b")[::-1], 2) if nbits else 0, nbits)

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def _write_tokens(w, tokens, ll_lens, d_lens):
    ll_codes, d_codes = canonical_codes(ll_lens), canonical_codes(d_lens)
    for tok in tokens:
        if isinstance(tok, tuple):
            s, eb, ev = len_symbol(tok[0])
            ds, deb, dev = dist_symbol(tok[1])
            w.code(ll_codes[s], ll_lens[s])
            w.put(ev, eb)
            w.code(d_codes[ds], d_lens[ds])
            w.put(dev, deb)
        else:
            w.code(ll_codes[tok], ll_lens[tok])
    w.code(ll_codes[256], ll_lens[256])


def encode_block(tokens, data, final, dynamic=True):
    """(bytes of the block in its smallest form, {"type", "fixed_bytes", "dynamic_bytes", "stored_bytes", "payload_bits",
    "header_bits"}): dynamic only where strictly smaller than both other forms, fixed only where smaller than stored."""
    ll, d, extra = histograms(tokens)
    ll_lens, d_lens = limited_lengths(ll, 15), limited_lengths(d, 15)
    hlit, hdist, hclen, cl_lens, rle, hdr = header_plan(ll_lens, d_lens)
    payload = sum(f * ln for f, ln in zip(ll, ll_lens)) + sum(f * ln for f, ln in zip(d, d_lens)) + extra
    sizes = {"fixed_bytes": form_bytes(fixed_bits(tokens), final), "dynamic_bytes": form_bytes(hdr + payload, final),
             "stored_bytes": 5 + len(data), "payload_bits": payload, "header_bits": hdr}
    w = _Writer()
    if dynamic and sizes["dynamic_bytes"] < sizes["fixed_bytes"] and sizes["dynamic_bytes"] < sizes["stored_bytes"]:
        sizes["type"] = 2
        w.put(final | 4, 3)
        w.put(hlit - 257, 5)
        w.put(hdist - 1, 5)
        w.put(hclen - 4, 4)
        for k in range(hclen):
            w.put(cl_lens[CL_ORDER[k]], 3)
        cl_codes = canonical_codes(cl_lens)
        for s, ev in rle:
            w.code(cl_codes[s], cl_lens[s])
            w.put(ev, CL_EXTRA.get(s, 0))
        _write_tokens(w, tokens, ll_lens, d_lens)
    elif sizes["fixed_bytes"] < sizes["stored_bytes"]:
        sizes["type"] = 1
        w.put(final | 2, 3)
        _write_tokens(w, tokens, FIXED_LL, FIXED_D)
    else:
        sizes["type"] = 0
        w.put(final, 8)
        w.put(len(data), 16)
        w.put(len(data) ^ 0xFFFF, 16)
        out = w.bytes() + bytes(data)
        assert len(out) == sizes["stored_bytes"]
        return out, sizes
    if not final:
        w.put(0, 3)
        w.align()
        w.put(0xFFFF0000, 32)
    out = w.bytes()
    assert len(out) == sizes["dynamic_bytes" if sizes["type"] == 2 else "fixed_bytes"]
    return out, sizes


def encode_model(payload, member_bytes, row_bytes, near_bytes=1, dynamic=True):
    """-> (the raw deflate stream of every member, the size record of every block, members in order)."""
    raw = bytes(payload)
    streams, records = [], []
    for lo in (range(0, len(raw), member_bytes) if raw else [0]):
        member = raw[lo:lo + member_bytes]
        toks = greedy_tokens(member, row_bytes, near_bytes)
        parts = []
        for b, t in enumerate(toks):
            data = member[b * BLK:(b + 1) * BLK]
            blob, rec = encode_block(t, data, int(b == len(toks) - 1), dynamic)
            rec["tokens"] = t
            parts.append(blob)
            records.append(rec)
        streams.append(b"".join(parts))
    return streams, records


# ------------------------------------------------------------------------------------------------------------------ payloads
IMG_W = 300


def prefix_image():
    """The image of tests/test_gpu_deflate.py: row k + 1 repeats the first L = 3 .. 258 bytes of row k."""
    rng = np.random.default_rng(11)
    rows = [rng.integers(0, 256, IMG_W, dtype=np.uint8)]
    for L in range(3, 259):
        r = rng.integers(0, 256, IMG_W, dtype=np.uint8)
        r[:L] = rows[-1][:L]
        r[L] = rows[-1][L] ^ 0x55
        r[-1] = rows[-1][-1] ^ 0xAA
        rows.append(r)
    rows += [rows[-1].copy(), rows[-1].copy()]
    return np.concatenate(rows)


def _cycle(a, n):
    return np.resize(a, n) if n else np.zeros(0, np.uint8)


def _regions_like(n):
    rng = np.random.default_rng(5)
    vals = rng.choice(np.array([0, 1, 2, 11, 143, 144, 200, 255, 255, 255], np.uint8), n // 8 + 2)
    lens = rng.choice(np.array([1, 1, 2, 3, 4, 17, 60, 300]), n // 8 + 2)
    return np.repeat(vals, lens)[:n]


CONTENTS = {
    "zeros": lambda n: np.zeros(n, np.uint8),
    "all255": lambda n: np.full(n, 255, np.uint8),
    "alternating": lambda n: (np.arange(n) & 1).astype(np.uint8),
    "random": lambda n: np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8),
    "random0to3": lambda n: np.random.default_rng(2).integers(0, 4, n, dtype=np.uint8),
    "prefix_image": lambda n: _cycle(prefix_image(), n),
    "regions_like": _regions_like,
}


def fibonacci_block():
    """6 763 bytes of 17 values with the counts 1, 2, 3, 5, .. 2584: with the end-of-block symbol (count 1) the block's histogram is
    the first 18 Fibonacci numbers, whose Huffman tree is a chain of depth 17 whatever the tie-breaking (17 Fibonacci counts next to
    the end-of-block symbol would not do: three counts of 1 let the tree split into two chains of half the depth).  No two equal
    bytes are adjacent, so there is no match at distance 1: the values are dealt out most frequent first onto the positions
    0, 2, 4, .. then 1, 3, 5, .. (the largest share is 38 %, less than one half)."""
    fib = [1, 2]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    vals = np.repeat(np.arange(17, dtype=np.uint8)[::-1] * 3 + 40, fib[::-1])
    n = len(vals)
    out = np.empty(n, np.uint8)
    order = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
    out[order] = vals
    assert (out[1:] != out[:-1]).all() and n == 6763
    return out
