// Token codes of a fixed-Huffman deflate block (RFC 1951 section 3.2.5 / 3.2.6), the symbols, canonical codes and header run-length
// code of a dynamic one (3.2.7) and the GF(2) arithmetic of CRC-32 (RFC 1952 section 8), shared by the kernels of deflate.hip, their
// host entry and tools/deflate_codes_host.cpp.  Plain C++: no table, every code is computed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BOA_HD __host__ __device__ __forceinline__
#else
#define BOA_HD inline
#endif

// the low `n` bits of `v` in reverse order (Huffman codes enter the stream most significant bit first)
BOA_HD unsigned dfl_rev(unsigned v, int n) {
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32 - n);
}

// literal byte `v` -> stream bits (first bit = bit 0); *nbits = 8 or 9
BOA_HD uint64_t dfl_literal(unsigned v, int* nbits) {
    if (v < 144) {
        *nbits = 8;
        return dfl_rev(0x30 + v, 8);
    }
    *nbits = 9;
    return dfl_rev(0x190 + (v - 144), 9);
}

// <length 3..258, distance 1..32768> -> stream bits: length code, its extra bits, 5-bit distance code, its extra bits (at most 31)
BOA_HD uint64_t dfl_match(unsigned len, unsigned dist, int* nbits) {
    unsigned l = len - 3, sym, e = 0;
    if (len == 258)
        sym = 285;
    else if (l < 8)
        sym = 257 + l;
    else {
        e = (31 - __builtin_clz(l)) - 2;          // codes 265..284: four per count of extra bits
        sym = 261 + 4 * e + ((l >> e) & 3);
    }
    int n;
    uint64_t bits;
    if (sym < 280) {
        bits = dfl_rev(sym - 256, 7);
        n = 7;
    } else {
        bits = dfl_rev(0xC0 + (sym - 280), 8);
        n = 8;
    }
    bits |= (uint64_t)(l & ((1u << e) - 1)) << n;
    n += e;
    unsigned dd = dist - 1, dc = dd, de = 0;
    if (dd >= 4) {
        const unsigned msb = 31 - __builtin_clz(dd);  // codes 4..29: two per count of extra bits
        de = msb - 1;
        dc = 2 * msb + ((dd >> de) & 1);
    }
    bits |= (uint64_t)(dfl_rev(dc, 5) | ((dd & ((1u << de) - 1)) << 5)) << n;
    *nbits = n + 5 + de;
    return bits;
}

// ---- dynamic-Huffman blocks (RFC 1951 section 3.2.7): symbols, canonical codes, the run-length code of the header ----
#define DFL_NLL 286      // literal/length symbols
#define DFL_ND 30        // distance symbols
#define DFL_NCL 19       // code-length symbols

// length 3..258 -> symbol 257..285; *ebits / *eval = its extra bits
BOA_HD unsigned dfl_len_symbol(unsigned len, int* ebits, unsigned* eval) {
    const unsigned l = len - 3;
    *ebits = 0;
    *eval = 0;
    if (len == 258) return 285;
    if (l < 8) return 257 + l;
    const unsigned e = (31 - __builtin_clz(l)) - 2;
    *ebits = (int)e;
    *eval = l & ((1u << e) - 1);
    return 261 + 4 * e + ((l >> e) & 3);
}

// distance 1..32768 -> symbol 0..29; *ebits / *eval = its extra bits
BOA_HD unsigned dfl_dist_symbol(unsigned dist, int* ebits, unsigned* eval) {
    const unsigned dd = dist - 1;
    *ebits = 0;
    *eval = 0;
    if (dd < 4) return dd;
    const unsigned msb = 31 - __builtin_clz(dd);
    *ebits = (int)(msb - 1);
    *eval = dd & ((1u << (msb - 1)) - 1);
    return 2 * msb + ((dd >> (msb - 1)) & 1);
}

// canonical code (RFC 1951 3.2.2) of symbol `sym` among the n code lengths `len` (0 = unused); len[sym] != 0.  Every shorter code
// in front of it takes 2^(L - its length) codes of length L, every equal-length symbol below it one.
BOA_HD unsigned dfl_canon_code(const unsigned char* len, int n, int sym) {
    const unsigned L = len[sym];
    unsigned code = 0;
    for (int s = 0; s < n; ++s) {
        const unsigned ls = len[s];
        if (ls && ls < L)
            code += 1u << (L - ls);
        else if (ls == L && s < sym)
            ++code;
    }
    return code;
}

// table entry of a symbol: its code as stream bits (reversed) | length << 16; 0 for an unused symbol
BOA_HD unsigned dfl_code_entry(const unsigned char* len, int n, int sym) {
    const unsigned L = len[sym];
    return L ? dfl_rev(dfl_canon_code(len, n, sym), (int)L) | (L << 16) : 0u;
}

// the order in which the header stores the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
BOA_HD unsigned dfl_cl_order(int k) {
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                        5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (unsigned)((k < 12 ? lo >> (5 * k) : hi >> (5 * (k - 12))) & 31u);
}

BOA_HD int dfl_cl_extra_bits(unsigned sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// Run-length code of the n code lengths `seq` (literal/length lengths, then distance lengths, as one sequence) by the greedy rule
// zlib uses: a run of zeros goes in pieces of at most 138, a piece of 11..138 as symbol 18, of 3..10 as 17; a run of a non-zero
// length is written once, then repeated in pieces of at most 6, a piece of 3..6 as symbol 16; pieces below 3 are written out.
// out[k] = symbol | extra value << 8 (at most n entries); hist[19] counts the symbols (zeroed by the caller).  Returns the count.
BOA_HD int dfl_rle_lengths(const unsigned char* seq, int n, unsigned short* out, unsigned* hist) {
    int k = 0;
    for (int i = 0; i < n;) {
        const unsigned v = seq[i];
        int r = 1;
        while (i + r < n && seq[i + r] == v) ++r;
        i += r;
        if (v) {                     // the length itself
            out[k++] = (unsigned short)v;
            ++hist[v];
            --r;
        }
        const int piece = v ? 6 : 138;
        while (r >= 3) {
            const int c = r < piece ? r : piece;
            const unsigned sym = v ? 16 : c <= 10 ? 17 : 18;
            out[k++] = (unsigned short)(sym | (unsigned)(c - (sym == 18 ? 11 : 3)) << 8);
            ++hist[sym];
            r -= c;
        }
        for (; r > 0; --r) {
            out[k++] = (unsigned short)v;
            ++hist[v];
        }
    }
    return k;
}

// ---- CRC-32 as polynomials over GF(2) modulo P, reflected: bit 31 = x^0 ----
#define DFL_CRC_POLY 0xEDB88320u

BOA_HD unsigned dfl_gf2_mul(unsigned a, unsigned b) {
    unsigned p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & 0x80000000u) p ^= b;
        a <<= 1;
        b = (b >> 1) ^ ((b & 1) ? DFL_CRC_POLY : 0u);
    }
    return p;
}

struct DflCrcPow {
    unsigned x[40];   // x[k] = x^(8 * 2^k) mod P: appending 2^k bytes multiplies a CRC by x[k]
};

inline void dfl_crc_pow_init(DflCrcPow* t) {
    t->x[0] = 0x00800000u;   // x^8
    for (int k = 1; k < 40; ++k) t->x[k] = dfl_gf2_mul(t->x[k - 1], t->x[k - 1]);
}

// x^(8 * bytes) mod P; x = DflCrcPow::x
BOA_HD unsigned dfl_crc_xpow(const unsigned* x, unsigned long long bytes) {
    unsigned p = 0x80000000u;
    for (int k = 0; k < 40 && (bytes >> k); ++k)
        if ((bytes >> k) & 1) p = dfl_gf2_mul(x[k], p);
    return p;
}

// crc32(A || B) from crc32(A), crc32(B) and the byte length of B
BOA_HD unsigned dfl_crc_combine(const unsigned* x, unsigned crc_a, unsigned crc_b, unsigned long long len_b) {
    return dfl_gf2_mul(dfl_crc_xpow(x, len_b), crc_a) ^ crc_b;
}
