// Sequential DCT JPEG (ITU T.81 Annex F.2.2, Huffman, one component), the parts the kernels of jpeg_dct.hip and the stand-alone
// program tools/jpeg_dct_host.cpp share: one codeword step of the coefficient decode (DC and AC), the zig-zag table, and the
// reconstruction of a block as libjpeg performs it by default (JDCT_ISLOW, jidctint.c): dequantisation in wide integers, the
// two islow passes, the level shift and the range limit.  The IDCT is not normative in T.81; libjpeg's pixels are the bar.
#pragma once
#include "jpeg_huff.h"

#define JD_ST_OK 0
#define JD_ST_TRUNCATED 1          // the segment ends inside a codeword or before its last block
#define JD_ST_INVALID_CODE 2       // bits no code of the table is a prefix of (or an AC symbol RRRR/0 other than EOB and ZRL)
#define JD_ST_RUN_PAST_BLOCK 3     // a zero run that carries the zig-zag index past 63
#define JD_ST_BAD_SSSS 4           // SSSS above 11 (DC) / 10 (AC) at P = 8, 15 / 14 at P = 12
#define JD_ST_TRAILING 5           // a whole byte or more left after the segment's last block

// natural (row-major) index of the coefficient at zig-zag position k (T.81 figure A.6)
JH_HD int jd_natural(int k) {
    constexpr unsigned char Z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return Z[k & 63];
}

// One codeword = a Huffman code and its SSSS extra bits.  k: the zig-zag index of the next coefficient (0: the codeword is a DC
// code); zz: the position written (-1: none, for EOB and ZRL), val: the DC difference or the AC coefficient; knext: the index
// after the codeword, 0 when it completes the block.
struct JdStep {
    int len, knext, zz, val;
};

// win: >= 33 stream bits from the codeword's first (bits past the segment's end read as 1), avail: bits left in the segment.
// Returns JD_ST_OK or the reason the codeword does not decode.
JH_HD int jd_step(const unsigned* Tdc, const unsigned* Tac, unsigned long long win, int k, int P, unsigned avail, JdStep& o) {
    int sym;
    const int len = jh_symbol(k ? Tac : Tdc, (unsigned)(win >> 32), sym);
    if (!len) return avail >= 16u ? JD_ST_INVALID_CODE : JD_ST_TRUNCATED;
    if ((unsigned)len > avail) return JD_ST_TRUNCATED;
    int s, zz;
    if (k == 0) {
        s = sym;
        zz = 0;
        if (s > (P == 8 ? 11 : 15)) return JD_ST_BAD_SSSS;
    } else {
        const int run = sym >> 4;
        s = sym & 15;
        if (s > (P == 8 ? 10 : 14)) return JD_ST_BAD_SSSS;
        if (s == 0) {
            if (run == 15) {                            // ZRL: sixteen zeros
                if (k + 16 > 64) return JD_ST_RUN_PAST_BLOCK;
                o = JdStep{len, (k + 16) & 63, -1, 0};
                return JD_ST_OK;
            }
            if (run) return JD_ST_INVALID_CODE;         // EOBn: the progressive processes'
            o = JdStep{len, 0, -1, 0};                  // EOB
            return JD_ST_OK;
        }
        zz = k + run;
        if (zz > 63) return JD_ST_RUN_PAST_BLOCK;
    }
    if ((unsigned)(len + s) > avail) return JD_ST_TRUNCATED;
    int v = 0;
    if (s) {
        const unsigned u = (unsigned)((win << len) >> (64 - s));
        v = u < (1u << (s - 1)) ? (int)u - (1 << s) + 1 : (int)u;      // T.81 F.2.2.1 EXTEND
    }
    o = JdStep{len + s, (zz + 1) & 63, zz, v};
    return JD_ST_OK;
}

// ---- libjpeg's JDCT_ISLOW (jidctint.c): CONST_BITS 13, PASS1_BITS 2 at P = 8 and 1 at P = 12, DESCALE rounds half up
#define JD_CONST_BITS 13
JH_HD int jd_pass1_bits(int P) { return P == 8 ? 2 : 1; }

// one 1-D pass over v[0], v[stride], ..., v[7 stride] in place, results descaled by `shift` bits
JH_HD void jd_islow_1d(long long* v, int stride, int shift) {
    const long long i0 = v[0], i1 = v[stride], i2 = v[2 * stride], i3 = v[3 * stride], i4 = v[4 * stride], i5 = v[5 * stride],
                    i6 = v[6 * stride], i7 = v[7 * stride];
    long long z1 = (i2 + i6) * 4433;                    // FIX(0.541196100)
    const long long e2 = z1 - i6 * 15137;               // FIX(1.847759065)
    const long long e3 = z1 + i2 * 6270;                // FIX(0.765366865)
    const long long e0 = (i0 + i4) * (1 << JD_CONST_BITS), e1 = (i0 - i4) * (1 << JD_CONST_BITS);
    const long long t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    long long t0 = i7, t1 = i5, t2 = i3, t3 = i1;
    z1 = t0 + t3;
    long long z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const long long z5 = (z3 + z4) * 9633;              // FIX(1.175875602)
    t0 *= 2446;                                         // FIX(0.298631336)
    t1 *= 16819;                                        // FIX(2.053119869)
    t2 *= 25172;                                        // FIX(3.072711026)
    t3 *= 12299;                                        // FIX(1.501321110)
    z1 *= -7373;                                        // FIX(0.899976223)
    z2 *= -20995;                                       // FIX(2.562915447)
    z3 = z3 * -16069 + z5;                              // FIX(1.961570560)
    z4 = z4 * -3196 + z5;                               // FIX(0.390180644)
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    const long long r = 1ll << (shift - 1);
    v[0] = (t10 + t3 + r) >> shift;
    v[7 * stride] = (t10 - t3 + r) >> shift;
    v[stride] = (t11 + t2 + r) >> shift;
    v[6 * stride] = (t11 - t2 + r) >> shift;
    v[2 * stride] = (t12 + t1 + r) >> shift;
    v[5 * stride] = (t12 - t1 + r) >> shift;
    v[3 * stride] = (t13 + t0 + r) >> shift;
    v[4 * stride] = (t13 - t0 + r) >> shift;
}

// libjpeg's range-limit table read at x & (4 MAX + 3), x = a result of the second pass: the level shift (+ centre) and the clamp
// to 0 .. MAX, with the table's wrap for values far outside
JH_HD int jd_range_limit(long long x, int P) {
    const int mx = (1 << P) - 1, centre = (mx + 1) >> 1;
    const int i = (int)(x & (long long)(4 * mx + 3));
    if (i < centre) return i + centre;
    if (i < 2 * (mx + 1)) return mx;
    if (i < 4 * (mx + 1) - centre) return 0;
    return i - (4 * (mx + 1) - centre);
}

// A block: coef[64] quantised coefficients and q[64] the quantisation table, both in natural order -> px[64] samples
JH_HD void jd_block(const short* coef, const unsigned short* q, int P, unsigned short* px) {
    long long w[64];
    for (int i = 0; i < 64; ++i) w[i] = (long long)coef[i] * (long long)q[i];
    const int pb = jd_pass1_bits(P);
    for (int c = 0; c < 8; ++c) jd_islow_1d(w + c, 8, JD_CONST_BITS - pb);             // pass 1: columns
    for (int r = 0; r < 8; ++r) jd_islow_1d(w + 8 * r, 1, JD_CONST_BITS + pb + 3);     // pass 2: rows
    for (int i = 0; i < 64; ++i) px[i] = (unsigned short)jd_range_limit(w[i], P);
}
