// fp16 transposed conv, kernel == stride, on f16 MFMA: out[o] = sum_ci y[o / s][ci] * W[ci][co][o % s] + b, with the producer's
// InstanceNorm + LeakyReLU applied while staging.  Three kernels (convt_mfma_form picks one) that share their index paths, their
// epilogue and its LDS slab: k_convt_mfma (any Cin), k_convt_mfma_rw (weights in registers), k_convt_deep (weights by LDS-DMA).
#include <algorithm>

#include "conv.h"

// ---- the transposed convs' per-wave LDS slab (D fragments -> 16-byte pieces of the output voxels' records) -------------------------
// Logical layout [plane][output voxel ov = l31 * TZ + t][16 couts]: lane (l31, kh) writes the 8-byte piece q = 2 (gq & 1) + kh of its
// voxel's 32-byte record, the wave then reads 16-byte pieces `lane + 64 k` and stores 1 KiB runs.  With TZ = 2 the writing lanes sit
// 64 bytes apart: every 16-lane group of the ds_write_b64 fell on two banks' worth of one 128-byte row -- 8-way conflicts, 72 - 76 % of
// the kernels' LDS cycles (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE, profiles/r05_pmc_lds.txt).  Physical layout for TZ = 2: record
// (t, l31) at t * 32 + (l31 ^ 4 t) (lanes 32 bytes apart; the xor keeps the two taps of a voxel pair off the same bank row for the
// reads), piece q at q ^ ((l31 >> 2) & 3) (the four lanes of a group that share a 32-byte window take its four pieces): writes and
// reads are conflict-free; a reader whose record has an odd swizzle finds the two 8-byte pieces of its half swapped and swaps them back.
template <int TZ>
__device__ __forceinline__ int convt_slab_waddr(int gq, int l31, int t, int kh) {
    if constexpr (TZ == 2) {
        const int rec = t * 32 + (l31 ^ (4 * t));
        const int q = ((gq & 1) * 2 + kh) ^ ((l31 >> 2) & 3);
        return ((gq >> 1) * 64 + rec) * 32 + q * 8;
    } else {
        return ((gq >> 1) * 32 * TZ + l31 * TZ + t) * 32 + (8 * (gq & 1) + 4 * kh) * 2;
    }
}
template <int TZ>
__device__ __forceinline__ uint4 convt_slab_read(const unsigned char* slab, int pl, int piece) {
    if constexpr (TZ == 2) {
        const int ov = piece >> 1, h = piece & 1;
        const int j = ov >> 1, tz = ov & 1;
        const int sw = (j >> 2) & 3;
        const uint4 d = *(const uint4*)(slab + (pl * 64 + tz * 32 + (j ^ (4 * tz))) * 32 + (h ^ (sw >> 1)) * 16);
        return (sw & 1) ? make_uint4(d.z, d.w, d.x, d.y) : d;
    } else {
        return *(const uint4*)(slab + pl * 32 * TZ * 32 + piece * 16);
    }
}

struct ConvTArgs {
    const __half* src;
    const float* ss;
    const unsigned* ss16;  // packed fp16 (scale, shift) pairs of the input's deferred norm (preferred), or NULL
    int Cin, Cout, N, Di, Hi, Wi, s0, s1, s2;
    const __half* wpk;  // [tap][Cin/16][2][Cout][8]
    const float* bias;
    __half* out;
    float slope;
};

// One wave = 32 consecutive (flattened) input voxels.  Per (tx, ty, cout chunk) it computes BOTH z taps (TZ = s2
// accumulators): in the chunk-planar output the voxels 2 iz and 2 iz + 1 of a row are neighbours, so the wave's result for
// one 16-cout plane is one run of 2 KiB (TZ = 2) of consecutive bytes.  The D fragments go through a per-wave LDS slab
// [2 planes][32 TZ voxels][16 couts] and leave as 16-byte pieces, lane L taking pieces L, L + 64, ...: every store
// instruction writes 1 KiB of consecutive bytes (the one-tap-per-pass form wrote 32-byte pieces 64 bytes apart).
typedef _Float16 ct_h2 __attribute__((ext_vector_type(2)));

// deferred InstanceNorm + LeakyReLU on 8 channels in packed fp16 (the same one-rounding evaluation as k_conv_ws's producers):
// w = 4 x {packed scales, packed shifts} of the four channel pairs
__device__ __forceinline__ uint4 convt_norm_act8_pk(uint4 raw, const uint4& w0, const uint4& w1, unsigned slope2) {
    union {
        uint4 u;
        ct_h2 v[4];
    } x;
    union {
        unsigned u;
        ct_h2 v;
    } s, t, sl;
    const unsigned w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    x.u = raw;
    sl.u = slope2;
    ct_h2 y[4], z[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s.u = w[2 * i];
        t.u = w[2 * i + 1];
        y[i] = __builtin_elementwise_fma(x.v[i], s.v, t.v);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = y[i] * sl.v;
#pragma unroll
    for (int i = 0; i < 4; ++i) x.v[i] = __builtin_elementwise_max(y[i], z[i]);
    return x.u;
}

// ---- the pieces the three kernels share ------------------------------------------------------------------------------------------------
// (the helpers get scalars and this small struct BY VALUE: handed a reference to the kernel's ConvTArgs, hipcc re-loaded the kernel
//  arguments and re-scheduled every prologue)
struct ConvTGeo {
    // (32-bit index arithmetic: N * in_vox < 2^31, checked on the host -- the 64-bit divisions of the first version were ~40 % of
    //  k_convt_mfma's instructions; the kernel is instruction-bound: with every memory access switched off it still took half of its time)
    unsigned in_vox, total;  // input voxels per sample, of all samples
    int Hi, Wi, s0, s1, s2, Ho, Wo;
    size_t ovox;             // output voxels per sample
    int planes;              // 16-cout planes of the output
    int nco, npasses;        // cout chunks; (x tap, y tap, cout chunk) passes -- every pass covers the TZ = s2 z taps
};
__device__ __forceinline__ ConvTGeo convt_geo(int N, int Di, int Hi, int Wi, int s0, int s1, int s2, int Cout) {
    ConvTGeo q;
    q.in_vox = (unsigned)(Di * Hi * Wi);
    q.total = (unsigned)N * q.in_vox;
    q.Hi = Hi; q.Wi = Wi; q.s0 = s0; q.s1 = s1; q.s2 = s2;
    q.Ho = Hi * s1; q.Wo = Wi * s2;
    q.ovox = (size_t)(Di * s0) * q.Ho * q.Wo;
    q.planes = Cout / 16;
    q.nco = Cout / 32;
    q.npasses = s0 * s1 * q.nco;
    return q;
}

// pass -> its x / y tap, its cout chunk and its first tap (the z taps follow)
struct ConvTPass {
    int tx, ty, co, tap0;
};
__device__ __forceinline__ ConvTPass convt_pass(const ConvTGeo q, int pr) {
    const int txy = pr / q.nco, co = pr - txy * q.nco;
    const int ty = txy % q.s1, tx = txy / q.s1;
    return ConvTPass{tx, ty, co, (tx * q.s1 + ty) * q.s2};
}
// the bytes a pass adds to a store pointer (wave-uniform; plane pl adds ovox * 32)
__device__ __forceinline__ size_t convt_pass_off(const ConvTGeo q, const ConvTPass ps) {
    return ((size_t)(ps.co * 2) * q.ovox + ((size_t)ps.tx * q.Ho + ps.ty) * q.Wo) * 32;
}

// the packed pair (slope, slope) of convt_norm_act8_pk
__device__ __forceinline__ unsigned convt_slope2(float slope) {
    union {
        unsigned u;
        ct_h2 v;
    } sl2;
    sl2.v = ct_h2{(_Float16)slope, (_Float16)slope};
    return sl2.u;
}

// flattened (n, voxel) index -> sample and voxel within it; an index past the last voxel maps to voxel 0 of sample 0 (its lane stages zeros
// and stores nothing).  (The staging step built on it -- load a chunk's octet, convt_norm_act8_pk, zero if invalid -- stays written out in
// the kernels: as a function it changed the code of k_convt_mfma_rw when its argument came by value and that of k_convt_deep when it came
// by reference, profiles/convt_split_ab.txt.)
struct ConvTVox {
    bool valid;
    unsigned n, vi;
};
__device__ __forceinline__ ConvTVox convt_vox(const ConvTGeo q, unsigned gv) {
    ConvTVox v;
    v.valid = gv < q.total;
    v.n = v.valid ? gv / q.in_vox : 0;
    v.vi = v.valid ? gv - v.n * q.in_vox : 0;
    return v;
}

// Store side of a 32-voxel group that starts at the flattened (n, voxel) index g0.  The slab of one plane holds 32 * TZ output voxels =
// 64 * TZ pieces of 16 bytes; a lane takes pieces lane + 64 k (k < TZ) of each plane: output voxel ov = piece / 2 -> input voxel j = ov / TZ
// of the group, z tap ov % TZ.  *optr: the lane's piece k in plane 0 of its sample at tap (0, 0) -- a pass adds convt_pass_off();
// returns whether that voxel exists.
template <int TZ>
__device__ __forceinline__ bool convt_piece_ptr(const ConvTGeo q, __half* out, unsigned g0, int lane, int k, unsigned char** optr) {
    const int ov = (lane + 64 * k) >> 1;
    const int j = ov / TZ, tz = ov % TZ;
    const ConvTVox v = convt_vox(q, g0 + j);
    const unsigned r2 = v.vi / (unsigned)q.Wi;
    const int iz = (int)(v.vi - r2 * (unsigned)q.Wi);
    const int ix = (int)(r2 / (unsigned)q.Hi), iy = (int)(r2 - (unsigned)ix * (unsigned)q.Hi);
    const size_t ospat = ((size_t)(ix * q.s0) * q.Ho + (size_t)(iy * q.s1)) * q.Wo + (size_t)(iz * q.s2 + tz);
    *optr = (unsigned char*)out + ((size_t)v.n * q.planes * q.ovox + ospat) * 32 + 16 * (lane & 1);
    return v.valid;
}

// one (gq, t) quad of an accumulator + bias -> fp16 (RTNE) -> slab: lane (voxel l31, kh) holds couts 8 gq + 4 kh + e -> plane gq / 2,
// offset 8 (gq % 2) + 4 kh
template <int TZ>
__device__ __forceinline__ void convt_slab_put(unsigned char* slab, int gq, int t, int l31, int kh, const f32x16& acc, const f32x16& bias) {
    union {
        uint2 u;
        __half h[4];
    } pk;
    pk.h[0] = __float2half_rn(acc[gq * 4 + 0] + bias[gq * 4 + 0]);
    pk.h[1] = __float2half_rn(acc[gq * 4 + 1] + bias[gq * 4 + 1]);
    pk.h[2] = __float2half_rn(acc[gq * 4 + 2] + bias[gq * 4 + 2]);
    pk.h[3] = __float2half_rn(acc[gq * 4 + 3] + bias[gq * 4 + 3]);
    *(uint2*)(slab + convt_slab_waddr<TZ>(gq, l31, t, kh)) = pk.u;
}

// slab -> the group's guarded 16-byte stores (bit k of `ok`: piece k's voxel exists); the wave barriers order them against the slab writes
// before and after
template <int TZ>
__device__ __forceinline__ void convt_slab_store(const unsigned char* slab, int lane, unsigned char* const* optr, unsigned ok, size_t poff,
                                                 size_t ovox) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int k = 0; k < TZ; ++k) {
            const int piece = lane + 64 * k;
            const uint4 d = convt_slab_read<TZ>(slab, pl, piece);
            if ((ok >> k) & 1u) *(uint4*)(optr[k] + poff + (size_t)pl * ovox * 32) = d;
        }
    __builtin_amdgcn_wave_barrier();
}

// this lane's 16 biases of cout chunk co: entry 4 gq + e <-> cout 8 gq + 4 kh + e, as in the accumulators
__device__ __forceinline__ f32x16 convt_bias(const float* bias, int co, int kh) {
    f32x16 b;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const float4 bq = *(const float4*)(bias + co * 32 + 8 * gq + 4 * kh);
        b[gq * 4 + 0] = bq.x; b[gq * 4 + 1] = bq.y; b[gq * 4 + 2] = bq.z; b[gq * 4 + 3] = bq.w;
    }
    return b;
}

template <int TZ>
__global__ __launch_bounds__(256) void k_convt_mfma(ConvTArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int kh = lane >> 5;
    const int ncc = p.Cin / 16;
    const ConvTGeo q = convt_geo(p.N, p.Di, p.Hi, p.Wi, p.s0, p.s1, p.s2, p.Cout);
    constexpr int SLAB = 2 * 32 * TZ * 32;  // bytes: [2 planes][32 * TZ output voxels][16 halves]
    unsigned char* lds = smem + (size_t)wave * (ncc * 1024 + SLAB);  // [cc][khalf][32 voxels][8 halves] + slab
    unsigned char* slab = lds + ncc * 1024;
    const unsigned g0 = ((unsigned)blockIdx.x * 4 + wave) * 32;  // first flattened (n, voxel) of this wave
    // stage this wave's 32 voxels: lane (l31, kh) moves octet kh of every 16-channel chunk; loads batched by 4
    {
        const unsigned sl2 = convt_slope2(p.slope);
        const ConvTVox v = convt_vox(q, g0 + l31);
        const __half* src_l = p.src + ((size_t)v.n * ncc * q.in_vox + v.vi) * 16 + kh * 8;   // + cc * in_vox * 16 per chunk
        const unsigned* ss16_l = p.ss16 ? p.ss16 + ((size_t)v.n * p.Cin + kh * 8) : nullptr;  // + cc * 16 words per chunk
        for (int c0 = 0; c0 < ncc; c0 += 4) {
            uint4 val[4], w0[4], w1[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int cc = min(c0 + b, ncc - 1);
                val[b] = *(const uint4*)(src_l + (size_t)cc * q.in_vox * 16);  // chunk-planar
                if (ss16_l) {
                    w0[b] = *(const uint4*)(ss16_l + cc * 16);
                    w1[b] = *(const uint4*)(ss16_l + cc * 16 + 4);
                }
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int cc = min(c0 + b, ncc - 1);
                uint4 o = val[b];
                if (ss16_l) {
                    o = convt_norm_act8_pk(o, w0[b], w1[b], sl2);
                } else if (p.ss) {  // (callers without the packed table: fp32 evaluation)
                    float sc[8], sh[8];
                    const float* ss = p.ss + ((size_t)v.n * p.Cin + cc * 16 + kh * 8) * 2;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        sc[j] = ss[2 * j];
                        sh[j] = ss[2 * j + 1];
                    }
                    o = norm_act8(o, sc, sh, p.slope);
                }
                if (!v.valid) o = make_uint4(0, 0, 0, 0);
                *(uint4*)(lds + ((cc * 2 + kh) * 32 + l31) * 16) = o;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    unsigned char* optr[TZ];
    unsigned ovalid = 0;
#pragma unroll
    for (int k = 0; k < TZ; ++k) ovalid |= convt_piece_ptr<TZ>(q, p.out, g0, lane, k, &optr[k]) ? (1u << k) : 0u;
    // weights: wave-uniform part of the address per (tap, chunk, cout chunk) + this lane's (kh, cout) offset
    const unsigned char* wbase = (const unsigned char*)p.wpk;
    const unsigned wlane = ((unsigned)kh * (unsigned)p.Cout + (unsigned)l31) * 16u;
    const unsigned wstep_cc = 2u * (unsigned)p.Cout * 16u;  // bytes per (tap, chunk)
    const unsigned char* bfrag = lds + (kh * 32 + l31) * 16;  // + cc * 1024
    int bias_co = -1;
    f32x16 biasv;
#pragma unroll
    for (int i = 0; i < 16; ++i) biasv[i] = 0.f;
    for (int pr = blockIdx.y; pr < q.npasses; pr += gridDim.y) {
        const ConvTPass ps = convt_pass(q, pr);
        if (ps.co != bias_co) {
            bias_co = ps.co;
            biasv = convt_bias(p.bias, ps.co, kh);
        }
        f32x16 acc[TZ];
        const unsigned char* wpass = wbase + ((size_t)ps.tap0 * ncc * wstep_cc + (size_t)ps.co * 32 * 16);  // uniform
        // groups of 4 chunks: the group's TZ x 4 weight fragments are loaded as one batch (the thin deep layers wait on L2 for
        // them: 8 loads in flight per wave), then 4 x TZ MFMAs.  The very first MFMA takes an inline-zero C operand instead
        // of zeroed accumulators.
        const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        auto group = [&](int c0, bool first) {
            f16x8 a[TZ][4];
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int t = 0; t < TZ; ++t)
                    a[t][b] = *(const f16x8*)(wpass + (size_t)(t * ncc + min(c0 + b, ncc - 1)) * wstep_cc + wlane);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (b == 0 || c0 + b < ncc) {  // (wave-uniform)
                    const f16x8 bf = *(const f16x8*)(bfrag + (c0 + b) * 1024);
#pragma unroll
                    for (int t = 0; t < TZ; ++t)
                        acc[t] = (first && b == 0) ? __builtin_amdgcn_mfma_f32_32x32x16_f16(a[t][b], bf, zero, 0, 0, 0)
                                                   : __builtin_amdgcn_mfma_f32_32x32x16_f16(a[t][b], bf, acc[t], 0, 0, 0);
                }
            }
        };
        group(0, true);
        for (int c0 = 4; c0 < ncc; c0 += 4) group(c0, false);
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
#pragma unroll
            for (int t = 0; t < TZ; ++t) convt_slab_put<TZ>(slab, gq, t, l31, kh, acc[t], biasv);
        convt_slab_store<TZ>(slab, lane, optr, ovalid, convt_pass_off(q, ps), q.ovox);
    }
}

// Register-weights variant for Cin = 16 NCC <= 128 (the 32^3 -> 64^3 and 64^3 -> 128^3 transposed convs, 75 % of the class's
// time): a wave covers G groups of 32 input voxels, staged once into its LDS slice, and per (x tap, y tap, cout chunk) pass loads
// the pass's TZ x NCC weight fragments ONCE into registers for all G groups.  k_convt_mfma re-reads them from L2 for every 32
// voxels: 1 KiB of weights per input voxel of the 64 -> 32 layer against 640 bytes of activations moved -- the kernel was bound
// by L2 -> CU weight traffic, not by HBM.  Same arithmetic, same output order.
template <int TZ, int NCC, int G>
__global__ __launch_bounds__(256) void k_convt_mfma_rw(ConvTArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int kh = lane >> 5;
    const ConvTGeo q = convt_geo(p.N, p.Di, p.Hi, p.Wi, p.s0, p.s1, p.s2, p.Cout);
    constexpr int SLAB = 2 * 32 * TZ * 32;  // bytes: [2 planes][32 * TZ output voxels][16 halves]
    unsigned char* lds = smem + (size_t)wave * (G * NCC * 1024 + SLAB);  // [g][cc][khalf][32 voxels][8 halves] + slab
    unsigned char* slab = lds + G * NCC * 1024;
    const unsigned g0 = ((unsigned)blockIdx.x * 4 + wave) * (32 * G);  // first flattened (n, voxel) of this wave
    const unsigned sl2 = convt_slope2(p.slope);
    // stage the wave's G x 32 voxels with the deferred norm applied
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const ConvTVox v = convt_vox(q, g0 + 32 * g + l31);
        const __half* src_l = p.src + ((size_t)v.n * NCC * q.in_vox + v.vi) * 16 + kh * 8;
        const unsigned* ss16_l = p.ss16 ? p.ss16 + ((size_t)v.n * p.Cin + kh * 8) : nullptr;
        uint4 val[NCC];
#pragma unroll
        for (int cc = 0; cc < NCC; ++cc) val[cc] = *(const uint4*)(src_l + (size_t)cc * q.in_vox * 16);
#pragma unroll
        for (int cc = 0; cc < NCC; ++cc) {
            uint4 o = val[cc];
            if (ss16_l) {
                const uint4 w0 = *(const uint4*)(ss16_l + cc * 16), w1 = *(const uint4*)(ss16_l + cc * 16 + 4);
                o = convt_norm_act8_pk(o, w0, w1, sl2);
            }
            if (!v.valid) o = make_uint4(0, 0, 0, 0);
            *(uint4*)(lds + (((g * NCC + cc) * 2 + kh) * 32 + l31) * 16) = o;
        }
    }
    __builtin_amdgcn_wave_barrier();
    unsigned char* optr[G][TZ];
    unsigned ovalid = 0;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int k = 0; k < TZ; ++k)
            ovalid |= convt_piece_ptr<TZ>(q, p.out, g0 + 32 * g, lane, k, &optr[g][k]) ? (1u << (g * TZ + k)) : 0u;
    const unsigned char* wbase = (const unsigned char*)p.wpk;
    const unsigned wlane = ((unsigned)kh * (unsigned)p.Cout + (unsigned)l31) * 16u;
    const unsigned wstep_cc = 2u * (unsigned)p.Cout * 16u;  // bytes per (tap, chunk)
    const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int pr = blockIdx.y; pr < q.npasses; pr += gridDim.y) {
        const ConvTPass ps = convt_pass(q, pr);
        const f32x16 biasv = convt_bias(p.bias, ps.co, kh);
        const unsigned char* wpass = wbase + ((size_t)ps.tap0 * NCC * wstep_cc + (size_t)ps.co * 32 * 16);  // uniform
        f16x8 a[TZ][NCC];   // the pass's weights, once for all G groups
#pragma unroll
        for (int t = 0; t < TZ; ++t)
#pragma unroll
            for (int cc = 0; cc < NCC; ++cc) a[t][cc] = *(const f16x8*)(wpass + (size_t)(t * NCC + cc) * wstep_cc + wlane);
        const size_t poff = convt_pass_off(q, ps);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            f32x16 acc[TZ];
            const unsigned char* bfrag = lds + ((g * NCC * 2 + kh) * 32 + l31) * 16;  // + cc * 1024
#pragma unroll
            for (int cc = 0; cc < NCC; ++cc) {
                const f16x8 bf = *(const f16x8*)(bfrag + cc * 1024);
#pragma unroll
                for (int t = 0; t < TZ; ++t)
                    acc[t] = cc == 0 ? __builtin_amdgcn_mfma_f32_32x32x16_f16(a[t][cc], bf, zero, 0, 0, 0)
                                     : __builtin_amdgcn_mfma_f32_32x32x16_f16(a[t][cc], bf, acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
#pragma unroll
                for (int t = 0; t < TZ; ++t) convt_slab_put<TZ>(slab, gq, t, l31, kh, acc[t], biasv);
            convt_slab_store<TZ>(slab, lane, optr[g], ovalid >> (g * TZ), poff, q.ovox);
        }
    }
}

// Deep transposed convs (Cin = 16 NCC >= 256: 4^3 ... 16^3 inputs, round 4).  These layers are not HBM-bound at all -- a pass's
// weights (2 NCC KiB per (x tap, y tap, cout chunk)) outweigh the activations, and k_convt_mfma streams them from L2 once per WAVE:
// 230 / 138 / 41 us per 25 tiles for 84 / 19 / 3 MB of tensor traffic.  Here the block shares them: a wave keeps the B fragments of
// its MT x 32 input voxels (deferred norm applied) in REGISTERS for the whole kernel (one wave per SIMD: 512 VGPRs), the pass's
// weight fragments are moved L2 -> LDS once per BLOCK by LDS-DMA (double-buffered: the next pass's weights arrive under this
// pass's MFMAs) and every wave reads its A fragments from LDS: 0.5 KiB of LDS reads per MFMA, no weight traffic per wave.
// Same arithmetic as k_convt_mfma (chunk order, fp32 accumulation, bias add, RTNE to fp16), same slab interleave for the stores.
template <int NCC>
__global__ __launch_bounds__(256) void k_convt_deep(ConvTArgs p) {
    constexpr int TZ = 2, MT = 2;
    constexpr int WB = TZ * NCC * 1024;          // bytes of one pass's weights in LDS
    constexpr int SLAB = 2 * 32 * TZ * 32;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [weights 0][weights 1][4 slabs]
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, kh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const ConvTGeo q = convt_geo(p.N, p.Di, p.Hi, p.Wi, p.s0, p.s1, p.s2, p.Cout);
    unsigned char* slab = smem + 2 * WB + wave * SLAB;
    float* lbias = (float*)(smem + 2 * WB + 4 * SLAB);   // the bias vector in LDS: a global load inside the pass loop would make hipcc wait
    for (int i = tid; i < p.Cout; i += 256) lbias[i] = p.bias[i];   // with vmcnt(0) -- i.e. also for the next pass's weight DMA
    const unsigned lds_w = __builtin_amdgcn_readfirstlane((unsigned)(size_t)smem);
    // weights of pass `pr` -> LDS buffer `buf`: fragment f = tz * NCC + cc is one wave-wide LDS-DMA (64 lanes x 16 B: k-half
    // lane / 32, cout lane % 32); the four waves take f = wave, wave + 4, ...
    const unsigned wvoff = ((unsigned)kh * (unsigned)p.Cout + (unsigned)l31) * 16u;
    auto dma_pass = [&](int pr, int buf) {
        const ConvTPass ps = convt_pass(q, pr);
        for (int f = wave; f < TZ * NCC; f += 4) {
            const int t = f / NCC, cc = f - t * NCC;
            const size_t woff = ((size_t)((ps.tap0 + t) * NCC + cc) * 2 * p.Cout + (size_t)ps.co * 32) * 16;
            // (wave-uniform by construction; readfirstlane makes it so for the compiler: the SGPR operands of the DMA)
            const unsigned wlo = __builtin_amdgcn_readfirstlane((unsigned)woff), whi = __builtin_amdgcn_readfirstlane((unsigned)(woff >> 32));
            const unsigned char* src = (const unsigned char*)p.wpk + (((size_t)whi << 32) | wlo);
            const unsigned m0v = __builtin_amdgcn_readfirstlane(lds_w + (unsigned)(buf * WB + f * 1024));
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(wvoff), "s"(src), "s"(m0v) : "memory");
        }
    };
    int pr = blockIdx.y;
    if (pr < q.npasses) dma_pass(pr, 0);
    // this wave's B fragments (registers) and store pointers
    const unsigned sl2 = convt_slope2(p.slope);
    const unsigned g0 = ((unsigned)blockIdx.x * 4 + wave) * (32 * MT);
    f16x8 b[MT][NCC];
    unsigned char* optr[MT][TZ];
    unsigned ovalid = 0;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const ConvTVox v = convt_vox(q, g0 + 32 * m + l31);
        const __half* src_l = p.src + ((size_t)v.n * NCC * q.in_vox + v.vi) * 16 + kh * 8;
        const unsigned* ss16_l = p.ss16 + ((size_t)v.n * p.Cin + kh * 8);   // (convt_mfma_form: only sources with a packed table come here)
#pragma unroll
        for (int cc = 0; cc < NCC; ++cc) {
            uint4 o = *(const uint4*)(src_l + (size_t)cc * q.in_vox * 16);
            const uint4 w0 = *(const uint4*)(ss16_l + cc * 16), w1 = *(const uint4*)(ss16_l + cc * 16 + 4);
            o = convt_norm_act8_pk(o, w0, w1, sl2);
            if (!v.valid) o = make_uint4(0, 0, 0, 0);
            union {
                uint4 u;
                f16x8 f;
            } cv;
            cv.u = o;
            b[m][cc] = cv.f;
        }
#pragma unroll
        for (int k = 0; k < TZ; ++k)
            ovalid |= convt_piece_ptr<TZ>(q, p.out, g0 + 32 * m, lane, k, &optr[m][k]) ? (1u << (m * TZ + k)) : 0u;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int it = 0; pr < q.npasses; pr += gridDim.y, ++it) {
        const int buf = it & 1;
        if (pr + (int)gridDim.y < q.npasses) dma_pass(pr + (int)gridDim.y, buf ^ 1);
        const ConvTPass ps = convt_pass(q, pr);
        const f32x16 biasv = convt_bias(lbias, ps.co, kh);
        const unsigned char* wl = smem + buf * WB + (kh * 32 + l31) * 16;
        f32x16 acc[MT][TZ];
#pragma unroll
        for (int cc = 0; cc < NCC; ++cc)
#pragma unroll
            for (int t = 0; t < TZ; ++t) {
                const f16x8 a = *(const f16x8*)(wl + (t * NCC + cc) * 1024);
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    acc[m][t] = cc == 0 ? __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b[m][cc], zero, 0, 0, 0)
                                        : __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b[m][cc], acc[m][t], 0, 0, 0);
            }
        const size_t poff = convt_pass_off(q, ps);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
#pragma unroll
                for (int t = 0; t < TZ; ++t) convt_slab_put<TZ>(slab, gq, t, l31, kh, acc[m][t], biasv);
            convt_slab_store<TZ>(slab, lane, optr[m], ovalid >> (m * TZ), poff, q.ovox);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next pass's weights have landed (and this pass's stores are out)
        __syncthreads();
    }
}

int convt_mfma_form(int Cin, const int s[3], bool norm_src) {
    if (s[0] == 2 && s[1] == 2 && s[2] == 2 && norm_src && (Cin == 256 || Cin == 320)) return 2;
    if (s[2] == 2 && norm_src && (Cin == 64 || Cin == 128)) return 1;
    return 0;
}

int launch_convt_mfma(boa_ctx* ctx, const ActSrc& src, int N, const int din[3], const int s[3], int Cout,
                      const __half* wpk, const float* bias, float slope, __half* out) {
    BOA_REQUIRE(src.C % 16 == 0 && Cout % 32 == 0, "convT: channels %d -> %d unsupported", src.C, Cout);
    ConvTArgs a;
    a.src = src.data; a.ss = src.ss; a.ss16 = src.ss16; a.Cin = src.C; a.Cout = Cout; a.N = N;
    a.Di = din[0]; a.Hi = din[1]; a.Wi = din[2]; a.s0 = s[0]; a.s1 = s[1]; a.s2 = s[2];
    a.wpk = wpk; a.bias = bias; a.out = out; a.slope = slope;
    const int gy_mult = 2;  // (8 and 32 measured slower: every y-slice re-stages the block's input voxels)
    size_t total = (size_t)N * din[0] * din[1] * din[2];
    int gx = (int)((total + 127) / 128);
    // split the (tap, cout-chunk) pairs over gridDim.y only as far as needed to fill the chip: every y-slice
    // re-stages the block's input voxels
    BOA_REQUIRE(s[2] == 1 || s[2] == 2, "convT: stride %d along the contiguous axis is not instantiated (1 or 2)", s[2]);
    BOA_REQUIRE((double)total < 2147483648.0 - 256.0, "convT: %zu input voxels exceed the 32-bit index range", total);
    const int npairs = s[0] * s[1] * (Cout / 32);   // (tx, ty, cout chunk); a pair covers the s2 z taps
    int gy = std::min(npairs, std::max(1, ceil_div(gy_mult * ctx->cu_count, gx)));
    size_t lds = (size_t)4 * ((src.C / 16) * 1024 + 2 * 32 * s[2] * 32);
    BOA_REQUIRE(lds <= 160 * 1024, "convT: Cin=%d needs %zu bytes of LDS", src.C, lds);
    static bool once = (hipFuncSetAttribute((const void*)k_convt_mfma<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                        hipFuncSetAttribute((const void*)k_convt_mfma<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), true);
    (void)once;
    const double taps = (double)s[0] * s[1] * s[2];
    KernelTimer tm(ctx, BOA_K_CONVT, 2.0 * total * taps * src.C * Cout, 2.0 * total * (src.C + taps * Cout));
    const int form = convt_mfma_form(src.C, s, src.ss16 != nullptr);
    const bool rw = form == 1, deep = form == 2;
    if (deep) {
        const int ncc = src.C / 16;
        const int gxd = (int)((total + 255) / 256);    // 4 waves x 2 M-tiles x 32 voxels per block
        // the (x tap, y tap, cout chunk) passes are spread over gridDim.y until there is about one block per CU (one fits: 64-80 KiB of
        // weight buffers), at least two passes per block so that the weight DMA overlaps (measured at 25 tiles: 16^3 124 / 140 / 151 /
        // 189 us at 1 / 2 / 4 / 8 slices, 8^3 139 / 81 / 48 / 58, 4^3 166 / 94 / 52 / 34 and 22 at 20)
        const int gyd = std::max(1, std::min(npairs / 2, ctx->cu_count / std::max(gxd, 1)));
        const size_t ldsd = (size_t)2 * 2 * ncc * 1024 + 4 * (2 * 32 * 2 * 32) + (size_t)Cout * sizeof(float);
        static bool od = (hipFuncSetAttribute((const void*)k_convt_deep<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                          hipFuncSetAttribute((const void*)k_convt_deep<20>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), true);
        (void)od;
        if (ncc == 16)
            hipLaunchKernelGGL(k_convt_deep<16>, dim3(gxd, gyd), dim3(256), ldsd, ctx->stream, a);
        else
            hipLaunchKernelGGL(k_convt_deep<20>, dim3(gxd, gyd), dim3(256), ldsd, ctx->stream, a);
    } else if (rw) {
        // register-weights variant: G groups of 32 voxels per wave (G x 128 voxels per block)
        const int G = 2;   // (32^3 -> 64^3: 125 -> 105 us per 8 tiles: two workgroups per CU)
        const int gxr = (int)((total + 128 * G - 1) / (128 * G));
        const int gyr = std::min(npairs, std::max(1, ceil_div(gy_mult * ctx->cu_count, gxr)));
        const size_t ldsr = (size_t)4 * ((size_t)G * (src.C / 16) * 1024 + 2 * 32 * 2 * 32);
        static bool o1 = (hipFuncSetAttribute((const void*)k_convt_mfma_rw<2, 4, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                          hipFuncSetAttribute((const void*)k_convt_mfma_rw<2, 8, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), true);
        (void)o1;
        if (src.C == 64)
            hipLaunchKernelGGL((k_convt_mfma_rw<2, 4, 2>), dim3(gxr, gyr), dim3(256), ldsr, ctx->stream, a);
        else
            hipLaunchKernelGGL((k_convt_mfma_rw<2, 8, 2>), dim3(gxr, gyr), dim3(256), ldsr, ctx->stream, a);
    } else if (s[2] == 2)
        hipLaunchKernelGGL(k_convt_mfma<2>, dim3(gx, gy), dim3(256), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL(k_convt_mfma<1>, dim3(gx, gy), dim3(256), lds, ctx->stream, a);
    tm.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}
