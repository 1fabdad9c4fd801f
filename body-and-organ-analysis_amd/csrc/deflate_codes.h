// Token codes of a fixed-Huffman deflate block (RFC 1951 section 3.2.5 / 3.2.6) and the GF(2) arithmetic of CRC-32
// (RFC 1952 section 8), shared by the kernels of deflate.hip and their host entry.  Plain C++: no table, every code is computed.
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
