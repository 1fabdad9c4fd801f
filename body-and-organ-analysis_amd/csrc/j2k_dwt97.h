// The arithmetic of the irreversible path of the JPEG 2000 decoder (j2k.hip): dequantisation of what tier-1 decodes, the
// one-dimensional inverse 9/7 synthesis and the conversion of its output to a sample.  Plain C++: the kernels call these
// functions per thread, tools/j2k_dwt97_host.cpp calls them on the host under the sanitizers.
//
// This is OpenJPEG's arithmetic, operation by operation, so that a stream decodes to the very pixels OpenJPEG gives (a float64
// model with T.800's constants differs by +-1 on about 2 % of samples): float32 throughout, one rounding per multiply and per
// add.  Nothing here may be contracted into a fused multiply-add: both the library and the host program are built with
// -ffp-contract=off.
//
//   coefficient  float(q) * (0.5f * step_b),  q = +-(2 m + 2^b_last): m the decoded magnitude bits, b_last the lowest plane at
//                which the coefficient was coded (0 in a complete block), step_b = (1 + mu_b / 2048) 2^(P - eps_b); zero stays 0.0f.
//   synthesis    of n > 1 interleaved samples (even = low-pass): even samples *= K_LOW, odd samples *= K_HIGH, then four lifting
//                steps x[i] += (x[i-1] + x[i+1]) * -c, over the even i with c = DELTA, the odd i with GAMMA, the even i with
//                BETA, the odd i with ALPHA; a neighbour outside [0, n) is the whole-sample mirror image.  n = 1 passes through.
//   sample       rintf (ties to even), DC level shift, clamp to the P-bit range.
//
// A lifting step is symmetric in its two neighbours and float addition commutes, so the mirrored extension of the signal stays
// the mirror image, bit for bit, through every step: a sample may be computed from its own +-4 window of the extended signal,
// independently of all others, and equals what the in-place sweeps over the whole array give.  j2k97_pair does that for the
// samples 2k and 2k + 1 from the window 2k - 3 .. 2k + 5 (9 loads, 9 multiplies, 20 adds).
#pragma once
#include <math.h>
#include <stdint.h>

#if !defined(BOA_HD)
#if defined(__HIPCC__)
#define BOA_HD __host__ __device__ __forceinline__
#else
#define BOA_HD inline
#endif
#endif

#define J2K97_K_LOW 1.230174105f
#define J2K97_K_HIGH 1.625732422f
#define J2K97_DELTA 0.443506852f
#define J2K97_GAMMA 0.882911075f
#define J2K97_BETA (-0.052980118f)
#define J2K97_ALPHA (-1.586134342f)

// The lowest plane at which a significant coefficient of magnitude bits m was coded, in a block whose last pass is of kind kf
// (0 significance propagation, 1 magnitude refinement, 2 cleanup) at plane bf: bf, or bf + 1 where a significance pass left the
// coefficient waiting for its refinement (it was significant before: bit bf of m is not set by this pass).
BOA_HD int j2k_b_last(int m, int kf, int bf) { return kf == 0 && !(m & (1 << bf)) ? bf + 1 : bf; }

// t: the signed magnitude bits (|t| < 2^30, its bits below b_last zero), b_last 0 .. 30 -> the dequantised coefficient
BOA_HD float j2k97_dequant(int t, int b_last, float step_half) {
    if (t == 0) return 0.0f;
    const unsigned m = t < 0 ? 0u - (unsigned)t : (unsigned)t;
    const int q = (int)(2u * m + (1u << b_last));          // below 2^31
    return (float)(t < 0 ? -q : q) * step_half;
}

// whole-sample mirror image of index a in a signal of n >= 2 samples
BOA_HD int j2k97_mirror(int a, int n) {
    if ((unsigned)a < (unsigned)n) return a;               // (all but the windows at the two ends: no division)
    const int p = 2 * (n - 1);
    a %= p;
    if (a < 0) a += p;
    return a < n ? a : p - a;
}

// Samples 2k (-> even) and 2k + 1 (-> odd; meaningful where 2k + 1 < n) of the synthesis of n >= 1 samples, 0 <= 2k < n.
// in(i), 0 <= i < n: the subband sample at interleaved position i (even i: low-pass sample i / 2, odd i: high-pass sample i / 2).
template <class In>
BOA_HD void j2k97_pair(In in, int k, int n, float& even, float& odd) {
    if (n == 1) {
        even = in(0);
        odd = 0.0f;
        return;
    }
    float w[9];                                     // positions 2k - 3 .. 2k + 5: w[j] at an even position for odd j
    for (int j = 0; j < 9; ++j) w[j] = in(j2k97_mirror(2 * k - 3 + j, n)) * ((j & 1) ? J2K97_K_LOW : J2K97_K_HIGH);
    for (int j = 1; j <= 7; j += 2) w[j] = w[j] + (w[j - 1] + w[j + 1]) * -J2K97_DELTA;
    for (int j = 2; j <= 6; j += 2) w[j] = w[j] + (w[j - 1] + w[j + 1]) * -J2K97_GAMMA;
    for (int j = 3; j <= 5; j += 2) w[j] = w[j] + (w[j - 1] + w[j + 1]) * -J2K97_BETA;
    w[4] = w[4] + (w[3] + w[5]) * -J2K97_ALPHA;
    even = w[3];
    odd = w[4];
}

// The synthesis' output -> the sample modulo 2^16.  The float is clamped before its conversion (far outside any sample range,
// so that the result is the same), which keeps the conversion defined for whatever a corrupt stream makes of the coefficients;
// a NaN goes to the low end.
BOA_HD unsigned short j2k97_sample(float v, int P, int sgn) {
    int s = (int)fminf(fmaxf(rintf(v), -131072.0f), 131072.0f);
    const int half = 1 << (P - 1);
    if (sgn) s = s < -half ? -half : (s > half - 1 ? half - 1 : s);
    else { s += half; s = s < 0 ? 0 : (s > 2 * half - 1 ? 2 * half - 1 : s); }
    return (unsigned short)(s & 0xFFFF);
}
