// The per-voxel arithmetic of the class-probability pass (prob.hip): apply_inference_nonlin's `logits.float()` and
// `torch.softmax(x, 0)` in fp32 (NN/utilities/label_handling/label_handling.py:128-141) and the first-maximum argmax of the
// PROBABILITIES of convert_probabilities_to_segmentation (:144-183).  Plain C++: the kernels call these functions per voxel,
// tools/softmax_host.cpp calls them on the host under the sanitizers.
//
// One column of C fp16 logits x_c:
//   m   = max x_c                      (fp32 of the fp16 values: exact)
//   e_c = expf(x_c - m)                (the accurate expf, one rounded subtraction)
//   s   = e_0 + e_1 + ... + e_{C-1}    (ascending class order)
//   p_c = e_c / s                      (IEEE division)
//   label = the first c with p_c == max p
// For every class with p64 > 2^-100:  |p - p64| <= (C + 110) 2^-24 p64, else |p - p64| <= 2^-99  (DESIGN 4.14).
// A NaN logit makes s NaN, hence every p_c of the column NaN and the label 0 (no comparison with a NaN holds).  The maximum e_c is
// expf(0) = 1, so s >= 1 and nothing divides by zero or overflows, whatever finite fp16 values come in.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if !defined(BOA_HD)
#if defined(__HIPCC__)
#define BOA_HD __host__ __device__ __forceinline__
#else
#define BOA_HD inline
#endif
#endif

#define SMX_MAX_CLASSES 255

// fp16 bits -> fp32, exact (subnormals, infinities and NaNs included)
BOA_HD float smx_half_bits_to_float(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __half2float(__ushort_as_half(h));
#else
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t ex = (h >> 10) & 0x1fu, man = h & 0x3ffu, u;
    if (ex == 0x1fu) {
        u = sign | 0x7f800000u | (man << 13);
    } else if (ex != 0) {
        u = sign | ((ex + 112u) << 23) | (man << 13);
    } else if (man == 0) {
        u = sign;
    } else {                       // subnormal: man * 2^-24, normalised
        int sh = 0;
        while (!(man & 0x400u)) {
            man <<= 1;
            ++sh;
        }
        u = sign | ((uint32_t)(113 - sh) << 23) | ((man & 0x3ffu) << 13);
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}

// the running maximum: a NaN that comes first stays, one that comes later is passed over (the sum catches it)
BOA_HD float smx_max(float m, float x) { return x > m ? x : m; }
BOA_HD float smx_exp(float x, float m) { return expf(x - m); }
BOA_HD float smx_div(float e, float s) { return e / s; }
// the running first maximum of the probabilities: (best, label) updated with class c
BOA_HD void smx_first_max(float p, int c, float& best, int& label) {
    if (c == 0) {
        best = p;
        label = 0;
    } else if (p > best) {
        best = p;
        label = c;
    }
}

// The whole column: x(c) gives the fp16 bits of class c (asked for twice), p gets C values `pstride` apart and holds the exponentials
// between the sum and the division.  Returns the label.  (k_prob_rows does the same with the classes spread over registers; this is
// the form the host program and the per-voxel kernel call.)
template <typename X>
BOA_HD int smx_column_of(X x, int C, float* p, size_t pstride) {
    float m = smx_half_bits_to_float(x(0));
    for (int c = 1; c < C; ++c) m = smx_max(m, smx_half_bits_to_float(x(c)));
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
        const float e = smx_exp(smx_half_bits_to_float(x(c)), m);
        p[(size_t)c * pstride] = e;
        s += e;
    }
    float best = 0.f;
    int label = 0;
    for (int c = 0; c < C; ++c) {
        const float q = smx_div(p[(size_t)c * pstride], s);
        p[(size_t)c * pstride] = q;
        smx_first_max(q, c, best, label);
    }
    return label;
}

// ... of logits in memory, the classes `stride` elements apart
BOA_HD int smx_column(const uint16_t* x, size_t stride, int C, float* p, size_t pstride) {
    return smx_column_of([=](int c) { return x[(size_t)c * stride]; }, C, p, pstride);
}
