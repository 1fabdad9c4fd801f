// What the two Huffman JPEG decoders (jpeg_ll.hip: lossless Process 14; jpeg_dct.hip: sequential DCT) share: the bit window
// over one restart interval of un-stuffed entropy-coded data and the lookup of one Huffman code in an expanded DHT table
// (layout: include/boa_hip.h, boa_ljpeg_decode).  Host-callable: tools/jpeg_dct_host.cpp runs the same code under the host
// compiler's sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JH_HD __host__ __device__ __forceinline__
#else
#define JH_HD inline
#endif

#define JH_LB 9                    // bits of the direct lookup (codes of up to JH_LB bits: one read)
#define JH_T_MAXCODE 256
#define JH_T_VALOFF 274
#define JH_T_HUFFVAL 292

// stream word k (bytes 4k .. 4k+3 of the frame, big-endian); bytes at or past `end` (the segment's end) read as 0xff, and the
// load itself happens only when the word starts below `end` (the frame's bytes are padded to a multiple of 4 on the host)
JH_HD unsigned lj_word(const unsigned* w, unsigned end, unsigned k) {
    const unsigned b = 4u * k;
    if (b >= end) return ~0u;
    unsigned v = __builtin_bswap32(w[k]);
    if (b + 4u > end) v |= ~0u >> (8u * (end - b));
    return v;
}

// 64-bit window over the bit stream of one segment, refilled a word at a time
struct BitReader {
    const unsigned* w;
    unsigned end;      // segment end (byte, relative to the frame)
    unsigned wi;       // index of the word in the high half of `ab` (~0: nothing loaded)
    unsigned long long ab;
    JH_HD BitReader(const unsigned char* frame, unsigned end_byte) : w((const unsigned*)frame), end(end_byte), wi(~0u), ab(0) {}
    // 64 - (pos & 31) >= 33 valid bits starting at bit `pos` (a codeword is at most 16 + 15 = 31 bits)
    JH_HD unsigned long long peek(unsigned pos) {
        const unsigned k = pos >> 5;
        if (k != wi) {
            if (k == wi + 1u && wi != ~0u) ab = (ab << 32) | lj_word(w, end, k + 1u);
            else ab = ((unsigned long long)lj_word(w, end, k) << 32) | lj_word(w, end, k + 1u);
            wi = k;
        }
        return ab << (pos & 31u);
    }
};

// The Huffman code at the head of `top` (the next 32 stream bits): returns its length in bits (0 = no code of the table is a
// prefix of these bits) and the value coded.  T: table words (LDS or global).
JH_HD int jh_symbol(const unsigned* T, unsigned top, int& sym) {
    const unsigned li = top >> (32 - JH_LB);
    const unsigned e = (T[li >> 1] >> ((li & 1u) * 16u)) & 0xffffu;
    if (e) {
        sym = (int)(e & 0xffu);
        return (int)(e >> 8);
    }
    for (int l = JH_LB + 1; l <= 16; ++l) {        // canonical codes: the first length whose maxcode bounds the prefix
        const int code = (int)(top >> (32 - l));
        if (code <= (int)T[JH_T_MAXCODE + l]) {
            const unsigned vi = (unsigned)((int)T[JH_T_VALOFF + l] + code) & 255u;
            sym = (int)((T[JH_T_HUFFVAL + (vi >> 2)] >> ((vi & 3u) * 8u)) & 0xffu);
            return l;
        }
    }
    sym = 0;
    return 0;
}
