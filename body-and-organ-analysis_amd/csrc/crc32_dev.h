// CRC-32 (RFC 1952 section 8) on the device, shared by deflate.hip (the encoder's members) and inflate.hip (the decoder's check):
// the byte-wise table, built in LDS by 256 threads, the update over a run of bytes, and the table of x^(8 2^k) that the combine
// steps of deflate_codes.h read.
#pragma once
#include "deflate_codes.h"

// entry t of the byte-wise table (t = 0 .. 255)
__device__ __forceinline__ unsigned crc32_table_entry(unsigned t) {
    unsigned c = t;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? DFL_CRC_POLY : 0u);
    return c;
}

// the register of a CRC (initial value 0xffffffff, final XOR by the caller) after the bytes p[lo .. hi)
template <class I>
__device__ __forceinline__ unsigned crc32_update(const unsigned* tab, unsigned c, const unsigned char* p, I lo, I hi) {
    for (I i = lo; i < hi; ++i) c = tab[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return c;
}

inline const DflCrcPow& crc_pow() {
    static const DflCrcPow t = [] {
        DflCrcPow p;
        dfl_crc_pow_init(&p);
        return p;
    }();
    return t;
}
