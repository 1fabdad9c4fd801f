// The host-callable parts of the device inflate (inflate.hip): the bit reader, the validation of a dynamic block header and the
// construction of its decode tables (RFC 1951 section 3.2.7, with the verdicts of zlib's inflate_table), the decode of a chunk into
// a sink (a byte counter or the 16-bit symbol buffer), and the walk over a stream's chain of chunks.  Plain C++: the kernels call
// these functions, tools/inflate_codes_host.cpp runs them on the host under the sanitizers.  The bytes are untrusted: a read past the
// stream's end returns zero bits and ends the decode with a status, every loop consumes input or is bounded by a table.
#pragma once
#include <stdint.h>

#include "deflate_codes.h"

#define INF_OK 0
#define INF_TRUNCATED 1      // the stream ends inside a block
#define INF_INVALID 2        // an invalid code, block type, header or stored length
#define INF_FAR 3            // a distance that reaches more than 32 KiB before the chunk's start, or before the stream's first byte
#define INF_OVERRUN 4        // the store pass met more output than the count pass
#define INF_SIZE 5           // the stream's byte count is not the trailer's ISIZE
#define INF_CRC 6            // the stream's CRC-32 is not the trailer's
#define INF_REPAIR 7         // the chain of chunks did not settle within the repair rounds
#define INF_TRAILING 8       // the final block does not end in the stream's last byte, or no final block

#define INF_WINDOW 32768
#define INF_NO_STOP 0xffffffffffffffffull

struct InfBits {
    const uint8_t* p;      // the stream's first byte
    uint64_t nbytes;
    uint64_t next;         // the next byte to load (may pass nbytes: zero bits)
    uint64_t buf;
    int cnt;
};

BOA_HD void inf_refill(InfBits* b) {
    while (b->cnt <= 56) {
        const uint64_t v = b->next < b->nbytes ? b->p[b->next] : 0;
        b->buf |= v << b->cnt;
        ++b->next;
        b->cnt += 8;
    }
}

BOA_HD void inf_bits_init(InfBits* b, const uint8_t* p, uint64_t nbytes, uint64_t bit) {
    b->p = p;
    b->nbytes = nbytes;
    b->next = bit >> 3;
    b->buf = 0;
    b->cnt = 0;
    inf_refill(b);
    b->buf >>= (bit & 7);
    b->cnt -= (int)(bit & 7);
}

// the bit position of the next unread bit (beyond 8 nbytes once zero bits were handed out)
BOA_HD uint64_t inf_pos(const InfBits* b) { return b->next * 8 - (uint64_t)b->cnt; }

// the next n bits (n <= 32), first bit = bit 0
BOA_HD unsigned inf_get(InfBits* b, int n) {
    if (b->cnt < n) inf_refill(b);
    const unsigned v = (unsigned)(b->buf & ((1ull << n) - 1));
    b->buf >>= n;
    b->cnt -= n;
    return v;
}

// Decode tables of one block: per code the number of codes of every length and the symbols in canonical order.
struct InfTables {
    uint16_t lcount[16], lsym[288];
    uint16_t dcount[16], dsym[32];
    uint8_t lens[320];
};

// counts and canonical symbol order of the n code lengths `len`; the caller has judged the counts
BOA_HD void inf_construct(uint16_t* count, uint16_t* symbol, const uint8_t* len, int n) {
    uint16_t offs[16];
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) ++count[len[s] & 15];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int s = 0; s < n; ++s)
        if (len[s] & 15) symbol[offs[len[s] & 15]++] = (uint16_t)s;
}

// zlib's verdict on a set of code lengths given as counts per length (count[0] is not read): over-subscribed = invalid; incomplete =
// invalid unless the set is a single code of one bit (inflate_table: max == 1), or, with allow_empty, no code at all
BOA_HD bool inf_counts_ok(const uint16_t* count, bool allow_incomplete, bool allow_empty) {
    int left = 1, used = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - (int)count[l];
        if (left < 0) return false;
        used += count[l];
    }
    if (left == 0) return true;
    if (used == 0) return allow_empty;
    return allow_incomplete && used == 1 && count[1] == 1;
}

// one symbol of a canonical code, a bit at a time (at most 15); -1 = no such code (nothing is consumed then)
BOA_HD int inf_symbol(InfBits* b, const uint16_t* count, const uint16_t* symbol) {
    if (b->cnt < 15) inf_refill(b);
    uint64_t bits = b->buf;
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)(bits & 1);
        bits >>= 1;
        const int c = count[len];
        if (code - c < first) {
            b->buf >>= len;
            b->cnt -= len;
            return symbol[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// The header of a dynamic block, after its three block bits: HLIT, HDIST, HCLEN, the code-length code (which must be complete), the
// HLIT + 257 + HDIST + 1 lengths as one sequence, symbol 256 with a length, both codes judged by inf_counts_ok.  T != NULL: also
// builds the decode tables.  nbits = the stream's length in bits.
BOA_HD int inf_dynamic_header(InfBits* b, uint64_t nbits, InfTables* T) {
    const int hlit = (int)inf_get(b, 5) + 257, hdist = (int)inf_get(b, 5) + 1, hclen = (int)inf_get(b, 4) + 4;
    if (hlit > 286 || hdist > 30) return INF_INVALID;
    uint8_t cl[19];
    for (int k = 0; k < 19; ++k) cl[k] = 0;
    for (int k = 0; k < hclen; ++k) cl[dfl_cl_order(k)] = (uint8_t)inf_get(b, 3);
    if (inf_pos(b) > nbits) return INF_TRUNCATED;
    uint16_t ccount[16], csym[19];
    inf_construct(ccount, csym, cl, 19);
    if (!inf_counts_ok(ccount, false, false)) return INF_INVALID;
    uint16_t lc[16], dc[16];
    for (int l = 0; l < 16; ++l) lc[l] = dc[l] = 0;
    const int total = hlit + hdist;
    int i = 0, last = 0;
    bool has256 = false;
    while (i < total) {
        if (inf_pos(b) > nbits) return INF_TRUNCATED;
        const int sym = inf_symbol(b, ccount, csym);
        if (sym < 0) return INF_INVALID;
        int rep = 1, val = sym;
        if (sym == 16) {
            if (i == 0) return INF_INVALID;
            val = last;
            rep = 3 + (int)inf_get(b, 2);
        } else if (sym == 17) {
            val = 0;
            rep = 3 + (int)inf_get(b, 3);
        } else if (sym == 18) {
            val = 0;
            rep = 11 + (int)inf_get(b, 7);
        }
        if (i + rep > total) return INF_INVALID;
        for (; rep > 0; --rep, ++i) {
            if (T) T->lens[i] = (uint8_t)val;
            if (i < hlit) ++lc[val]; else ++dc[val];
            if (i == 256) has256 = val != 0;
        }
        last = val;
    }
    if (inf_pos(b) > nbits) return INF_TRUNCATED;
    if (!has256 || !inf_counts_ok(lc, true, false) || !inf_counts_ok(dc, true, true)) return INF_INVALID;
    if (T) {
        inf_construct(T->lcount, T->lsym, T->lens, hlit);
        inf_construct(T->dcount, T->dsym, T->lens + hlit, hdist);
    }
    return INF_OK;
}

// the tables of a fixed block (3.2.6): 288 literal/length codes (286 and 287 decode and are rejected as lengths), 30 distance codes
// of 5 bits (30 and 31 have no code)
BOA_HD void inf_fixed_tables(InfTables* T) {
    for (int s = 0; s < 288; ++s) T->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (int s = 0; s < 30; ++s) T->lens[288 + s] = 5;
    inf_construct(T->lcount, T->lsym, T->lens, 288);
    inf_construct(T->dcount, T->dsym, T->lens + 288, 30);
}

// The block-start test of the find pass: BFINAL = 0, BTYPE = 2 and a header that inf_dynamic_header accepts.
BOA_HD bool inf_block_start(const uint8_t* s, uint64_t nbytes, uint64_t bit) {
    const uint64_t nbits = nbytes * 8;
    if (bit + 17 > nbits) return false;
    InfBits b;
    inf_bits_init(&b, s, nbytes, bit);
    if (inf_get(&b, 3) != 4u) return false;
    return inf_dynamic_header(&b, nbits, nullptr) == INF_OK;
}

// length symbol 257 + s (s = 0 .. 28) and distance symbol d (0 .. 29): base value and extra bits
BOA_HD unsigned inf_len_base(int s, int* ebits) {
    if (s < 8 || s == 28) {
        *ebits = 0;
        return s == 28 ? 258u : 3u + (unsigned)s;
    }
    const int e = (s - 4) >> 2;
    *ebits = e;
    return 3u + ((4u + ((unsigned)s & 3u)) << e);
}

BOA_HD unsigned inf_dist_base(int d, int* ebits) {
    if (d < 4) {
        *ebits = 0;
        return (unsigned)d + 1u;
    }
    const int e = (d >> 1) - 1;
    *ebits = e;
    return 1u + ((2u + ((unsigned)d & 1u)) << e);
}

// ---- sinks of inf_decode_chunk ----
// the count pass: output bytes only
struct InfCount {
    uint64_t n = 0;
    BOA_HD int lit(unsigned) {
        ++n;
        return INF_OK;
    }
    BOA_HD int copy(unsigned len, unsigned dist) {
        if (dist > n + INF_WINDOW) return INF_FAR;
        n += len;
        return INF_OK;
    }
};

// the store pass: 16-bit symbols, 0 .. 255 = a literal byte, 0x8000 | k = byte k of the 32 KiB window in front of the chunk.  A copy
// copies symbols, so markers travel through transitive and overlapping matches; writes stay below `cap`, the counted length.
struct InfStore {
    uint16_t* out;
    uint64_t cap;
    uint64_t n = 0;
    BOA_HD int lit(unsigned v) {
        if (n >= cap) return INF_OVERRUN;
        out[n++] = (uint16_t)v;
        return INF_OK;
    }
    BOA_HD int copy(unsigned len, unsigned dist) {
        if (dist > n + INF_WINDOW) return INF_FAR;
        if (len > cap - n) return INF_OVERRUN;
        unsigned i = 0;
        if (dist <= n) {
            const uint16_t* src = out + (n - dist);
            uint16_t* dst = out + n;
            if (dist >= 4)
                for (; i + 4 <= len; i += 4) {      // four loads in flight before the stores (they do not overlap: dist >= 4)
                    const uint16_t a = src[i], b = src[i + 1], c = src[i + 2], d = src[i + 3];
                    dst[i] = a;
                    dst[i + 1] = b;
                    dst[i + 2] = c;
                    dst[i + 3] = d;
                }
            for (; i < len; ++i) dst[i] = src[i];
        } else {
            for (; i < len; ++i) {
                const uint64_t at = n + i;
                out[at] = at >= dist ? out[at - dist] : (uint16_t)(0x8000u | (unsigned)(INF_WINDOW - (dist - at)));
            }
        }
        n += len;
        return INF_OK;
    }
};

// Decodes the blocks of stream `s` (nbytes) from bit `start` until a block ends at or beyond bit `stop`, or the final block ends.
// *end_bit = where it stopped, *final = 1 after the BFINAL block.  T: the table space (one per decoding lane).
template <class Sink>
BOA_HD int inf_decode_chunk(const uint8_t* s, uint64_t nbytes, uint64_t start, uint64_t stop, InfTables* T, Sink& sink,
                            uint64_t* end_bit, int* final) {
    const uint64_t nbits = nbytes * 8;
    InfBits b;
    inf_bits_init(&b, s, nbytes, start);
    *final = 0;
    *end_bit = start;
    for (;;) {
        const uint64_t pos = inf_pos(&b);
        *end_bit = pos;
        if (pos >= stop) return INF_OK;
        if (pos + 3 > nbits) return INF_TRUNCATED;
        const unsigned hdr = inf_get(&b, 3);
        const unsigned type = hdr >> 1;
        if (type == 3) return INF_INVALID;
        if (type == 0) {
            inf_get(&b, (int)((0 - (pos + 3)) & 7));
            const unsigned len = inf_get(&b, 16), nlen = inf_get(&b, 16);
            const uint64_t at = inf_pos(&b);
            if (at > nbits) return INF_TRUNCATED;
            if (len != (~nlen & 0xffffu)) return INF_INVALID;
            const uint64_t byte = at >> 3;
            if (len > nbytes - byte) return INF_TRUNCATED;
            for (unsigned i = 0; i < len; ++i) {
                const int st = sink.lit(s[byte + i]);
                if (st) return st;
            }
            inf_bits_init(&b, s, nbytes, (byte + len) * 8);
        } else {
            if (type == 1)
                inf_fixed_tables(T);
            else {
                const int st = inf_dynamic_header(&b, nbits, T);
                if (st) return st;
            }
            for (;;) {
                if (inf_pos(&b) > nbits) return INF_TRUNCATED;
                int sym = inf_symbol(&b, T->lcount, T->lsym);
                if (sym < 0) return INF_INVALID;
                if (sym < 256) {
                    const int st = sink.lit((unsigned)sym);
                    if (st) return st;
                    continue;
                }
                if (sym == 256) break;
                sym -= 257;
                if (sym >= 29) return INF_INVALID;
                int eb;
                unsigned len = inf_len_base(sym, &eb);
                len += inf_get(&b, eb);
                const int ds = inf_symbol(&b, T->dcount, T->dsym);
                if (ds < 0 || ds >= 30) return INF_INVALID;
                unsigned dist = inf_dist_base(ds, &eb);
                dist += inf_get(&b, eb);
                if (inf_pos(&b) > nbits) return INF_TRUNCATED;
                const int st = sink.copy(len, dist);
                if (st) return st;
            }
            if (inf_pos(&b) > nbits) return INF_TRUNCATED;
        }
        if (hdr & 1) {
            *final = 1;
            *end_bit = inf_pos(&b);
            return INF_OK;
        }
    }
}

// ---- the chunk table and the walk over a stream's chain (host side of the count pass) ----
#define INF_F_LIVE 1u       // the chunk decodes
#define INF_F_REDO 2u       // the next count launch decodes it
#define INF_F_CAND 4u       // its start came from the find pass

struct InfChunk {
    uint64_t src_off, src_len;     // its stream in the source buffer
    uint64_t nominal;              // bit at which its search starts: 8 k chunk_bytes
    uint64_t search_end;           // bit at which its search ends
    uint64_t start, stop, end;     // bits
    uint64_t nbytes;               // output bytes
    uint64_t rel_off;              // output offset inside its stream
    uint64_t out_off;              // output offset in the whole buffer
    uint32_t stream, flags, status, final;
    uint32_t crc, pad;
};

struct InfWalk {
    int status = INF_OK;           // of the stream
    unsigned redo = 0;             // chunks flagged for another count launch
    unsigned rejected = 0;         // candidates dropped by this walk
};

// Walks the chunks [first, first + n) of one stream.  Chunk `first` starts at the stream's bit 0 and is therefore true; a chunk whose
// start equals the end of a true chunk is true.  Where a true chunk's end E is not the next live chunk's start, every live chunk that
// starts below E was a false candidate and is dropped, and unless the next one starts at E the first dropped slot is restarted at E
// (INF_F_REDO) with its stop at the next live start.  Behind a chunk that waits for its redo nothing is known: the walk goes on to
// hand out stops, but only a walk without any redo accepts the chain.  An error status of a true chunk is the stream's.
inline InfWalk inf_walk(InfChunk* ch, unsigned first, unsigned n) {
    InfWalk w;
    unsigned cur = first;
    const unsigned lim = first + n;
    bool known = true;             // cur's end is that of a true chunk
    for (;;) {
        InfChunk& c = ch[cur];
        unsigned f = cur + 1;
        if (c.flags & INF_F_REDO) {
            known = false;
            while (f < lim && !((ch[f].flags & INF_F_LIVE) && ch[f].start >= c.stop)) ++f;     // (its stop is the next live start)
            if (f >= lim) break;
            cur = f;
            continue;
        }
        if (known && c.status != INF_OK) {
            w.status = (int)c.status;
            return w;
        }
        if (!known) {              // stops only; the next walk judges
            while (f < lim && !(ch[f].flags & INF_F_LIVE)) ++f;
            if (f >= lim) break;
            cur = f;
            continue;
        }
        const uint64_t E = c.end;
        unsigned slot = lim;       // the first chunk dropped here
        while (f < lim && !((ch[f].flags & INF_F_LIVE) && ch[f].start >= E && !c.final)) {
            if (ch[f].flags & INF_F_LIVE) {
                if (ch[f].flags & INF_F_CAND) ++w.rejected;
                ch[f].flags = 0;
                if (slot == lim) slot = f;
            }
            ++f;
        }
        if (c.final) {
            if (((E + 7) >> 3) != c.src_len) w.status = INF_TRAILING;
            return w;
        }
        if (f < lim && ch[f].start == E) {
            cur = f;
            continue;
        }
        if (slot == lim) {         // no slot between the two: the chain cannot be repaired in place
            w.status = f < lim ? INF_REPAIR : INF_TRAILING;      // (no chunk left and no final block: the stream ends early)
            return w;
        }
        ch[slot].flags = INF_F_LIVE | INF_F_REDO;
        ch[slot].start = E;
        ch[slot].stop = f < lim ? ch[f].start : INF_NO_STOP;
        ++w.redo;
        cur = slot;
    }
    if (!w.redo && w.status == INF_OK) w.status = INF_TRAILING;      // the chain ended without a final block
    return w;
}
