// 1x1x1 head on the last decoder activation (+ Gaussian weighting + fp16 accumulate), scatter form: k_head_mfma on the matrix cores
// (F0 == 32, at most 31 classes, 32-voxel rows) and the fp32 VALU k_head.  (The gather form is head_gather.hip.)
#include <algorithm>

#include "conv.h"

struct HeadArgs {
    const __half* act;
    const float* ss;
    int F0, P0, P1, P2, C;
    const float* w;  // [C][F0]
    const float* bias;
    float slope;
    float* logits;
    const unsigned short* gauss;
    unsigned short* acc;
    unsigned short* nacc;
    int V0, V1, V2, s0, s1, s2;
    size_t plane_stride;  // voxels between the 16-channel planes of `act` (the tile's voxel count; a stash: its own)
};

template <int F0, int VPT>
__global__ __launch_bounds__(256) void k_head(HeadArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* lw = (float*)smem;        // [C][F0]
    float* lb = lw + p.C * F0;       // [C]
    float* lss = lb + p.C;           // [F0][2]
    for (int i = threadIdx.x; i < p.C * F0; i += 256) lw[i] = p.w[i];
    for (int i = threadIdx.x; i < p.C; i += 256) lb[i] = p.bias[i];
    for (int i = threadIdx.x; i < 2 * F0; i += 256) lss[i] = p.ss[i];
    __syncthreads();
    const size_t pv = (size_t)p.P0 * p.P1 * p.P2;
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * VPT;  // first of VPT consecutive voxels along z
    if (i >= pv) return;
    float y[VPT][F0];
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
#pragma unroll
        for (int v = 0; v < F0 / 8; ++v) {
            union {
                uint4 u4;
                __half h[8];
            } x;
            x.u4 = *(const uint4*)(p.act + ((size_t)(v >> 1) * p.plane_stride + (i + u)) * 16 + 8 * (v & 1));  // chunk-planar
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int c = v * 8 + j;
                float f = __builtin_fmaf(__half2float(x.h[j]), lss[2 * c], lss[2 * c + 1]);
                y[u][c] = f > 0.f ? f : f * p.slope;
            }
        }
    }
    if (p.logits) {
        for (int c = 0; c < p.C; ++c) {
#pragma unroll
            for (int u = 0; u < VPT; ++u) {
                float sum = lb[c];
#pragma unroll
                for (int k = 0; k < F0; ++k) sum = __builtin_fmaf(lw[c * F0 + k], y[u][k], sum);
                p.logits[(size_t)c * pv + i + u] = sum;
            }
        }
        return;
    }
    const int p2 = (int)(i % p.P2);
    const int p1 = (int)((i / p.P2) % p.P1);
    const int p0 = (int)(i / ((size_t)p.P2 * p.P1));
    const size_t vv = (size_t)p.V0 * p.V1 * p.V2;
    const size_t vi = ((size_t)(p.s0 + p0) * p.V1 + (p.s1 + p1)) * p.V2 + (p.s2 + p2);
    float g[VPT];
#pragma unroll
    for (int u = 0; u < VPT; ++u) g[u] = p.gauss ? us2f(p.gauss[i + u]) : 1.0f;
    for (int c = 0; c < p.C; ++c) {
        float sum[VPT];
#pragma unroll
        for (int u = 0; u < VPT; ++u) sum[u] = lb[c];
#pragma unroll
        for (int k = 0; k < F0; ++k) {
            const float wk = lw[c * F0 + k];
#pragma unroll
            for (int u = 0; u < VPT; ++u) sum[u] = __builtin_fmaf(wk, y[u][k], sum[u]);
        }
        unsigned short* ap = p.acc + (size_t)c * vv + vi;
        if (VPT == 2) {
            union {
                unsigned u32;
                unsigned short h[2];
            } a;
            a.u32 = *(const unsigned*)ap;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float pr = p.gauss ? sum[u] * g[u] : sum[u];  // prediction *= gaussian (fp32)
                a.h[u] = f2us(us2f(a.h[u]) + pr);             // fp16 += fp32 (fp32 add, RTNE to fp16)
            }
            *(unsigned*)ap = a.u32;
        } else {
            float pr = p.gauss ? sum[0] * g[0] : sum[0];
            *ap = f2us(us2f(*ap) + pr);
        }
    }
#pragma unroll
    for (int u = 0; u < VPT; ++u) p.nacc[vi + u] = f2us(us2f(p.nacc[vi + u]) + g[u]);
}

// Head on the matrix cores (F0 == 32, C <= 32, accumulate mode): per 32 consecutive z voxels two
// v_mfma_f32_32x32x16_f16 (K = 32 channels) replace 32 x C fp32 FMAs per voxel.  B fragments are the voxels' channel
// records straight from global memory (16 B per lane and step) with the deferred InstanceNorm + LeakyReLU applied in
// packed fp16, A = the head weights in registers.  D[class][voxel] -> + bias, x Gaussian (fp32), fp16 `+=` into the
// accumulators exactly as k_head does it (fp32 add, one RTNE rounding): lanes 0-31 / 32-63 update two classes of the
// same 32 voxels per instruction (64 contiguous bytes each).
typedef _Float16 hh2_t __attribute__((ext_vector_type(2)));

// LOGITS = true: the same MFMA / bias / transpose path, but the fp32 logits [C][P0][P1][P2] are written out instead of
// being accumulated (boa_net_forward, and the seam that proves the accumulate arithmetic of THIS kernel bit-exact: the
// logits it writes are the values its accumulate mode multiplies by the Gaussian and adds).
template <bool LOGITS>
__global__ __launch_bounds__(256, 5) void k_head_mfma(HeadArgs p) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, kh = lane >> 5;
    f16x8 a0, a1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        a0[i] = l31 < p.C ? (_Float16)p.w[l31 * 32 + 8 * kh + i] : (_Float16)0.f;
        a1[i] = l31 < p.C ? (_Float16)p.w[l31 * 32 + 16 + 8 * kh + i] : (_Float16)0.f;
    }
    // The per-lane constants -- packed (scale, shift) of this lane's 16 input channels and the 16 biases of its D rows --
    // depend on the k-half only; they live in LDS (2 x 32 words) and are re-read per M-tile instead of occupying 32 VGPRs:
    // the kernel waits on HBM round trips, and 114 -> ~80 VGPRs doubles the waves in flight (3 -> 6 per SIMD).
    __shared__ __attribute__((aligned(16))) unsigned s_ss[2][16];   // [kh][step 0: sc x4, sh x4 | step 1: sc x4, sh x4]
    __shared__ __attribute__((aligned(16))) float s_bz[2][16];
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        union {
            unsigned u;
            hh2_t v;
        } cv;
        for (int i = 0; i < 4; ++i) {
            const int c0 = 8 * k + 2 * i, c1 = 16 + 8 * k + 2 * i;
            cv.v = hh2_t{(_Float16)p.ss[2 * c0], (_Float16)p.ss[2 * c0 + 2]};
            s_ss[k][i] = cv.u;
            cv.v = hh2_t{(_Float16)p.ss[2 * c0 + 1], (_Float16)p.ss[2 * c0 + 3]};
            s_ss[k][4 + i] = cv.u;
            cv.v = hh2_t{(_Float16)p.ss[2 * c1], (_Float16)p.ss[2 * c1 + 2]};
            s_ss[k][8 + i] = cv.u;
            cv.v = hh2_t{(_Float16)p.ss[2 * c1 + 1], (_Float16)p.ss[2 * c1 + 3]};
            s_ss[k][12 + i] = cv.u;
        }
        for (int i = 0; i < 16; ++i) {
            const int c = 8 * (i >> 2) + 4 * k + (i & 3);
            s_bz[k][i] = c < p.C ? p.bias[c] : 0.f;
        }
    }
    __syncthreads();
    const hh2_t sl = hh2_t{(_Float16)p.slope, (_Float16)p.slope};
    auto xform = [&](uint4 raw, int step) {
        union {
            uint4 u;
            hh2_t v[4];
            f16x8 f;
        } x, sc, sh;
        x.u = raw;
        sc.u = *(const uint4*)&s_ss[kh][8 * step];
        sh.u = *(const uint4*)&s_ss[kh][8 * step + 4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const hh2_t y = __builtin_elementwise_fma(x.v[i], sc.v[i], sh.v[i]);
            x.v[i] = __builtin_elementwise_max(y, y * sl);
        }
        return x.f;
    };
    // per-wave LDS slab for the [class][voxel] transpose: 33 rows (32 classes + pad) x 36 floats (16-byte aligned rows)
    __shared__ __attribute__((aligned(16))) float slab_all[4][32 * 36];
    float* slab = slab_all[threadIdx.x >> 6];
    const int mpr = p.P2 / 32;                     // M-tiles per (x, y) row
    const int n_mt = p.P0 * p.P1 * mpr;
    const size_t vv = (size_t)p.V0 * p.V1 * p.V2;
    const size_t pv = (size_t)p.P0 * p.P1 * p.P2;
    const int gw = (int)((blockIdx.x * 256 + threadIdx.x) >> 6), nw = (int)(gridDim.x * 4);
    const int n_items = LOGITS ? p.C * 4 : (p.C + 1) * 4;  // (class, group of 8 voxels); class index C = the n_predictions row
    for (int mt = gw; mt < n_mt; mt += nw) {
        const int zb = (mt % mpr) * 32, row = mt / mpr, p1 = row % p.P1, p0 = row / p.P1;
        const size_t t0 = ((size_t)p0 * p.P1 + p1) * p.P2 + zb;       // first voxel of the M-tile within the tile
        const size_t v0 = ((size_t)(p.s0 + p0) * p.V1 + (p.s1 + p1)) * p.V2 + (p.s2 + zb);  // ... within the volume
        // chunk-planar: plane 0 = channels 0-15 (MFMA step 0 takes its octet kh), plane 1 = channels 16-31 (step 1); a wave
        // reads 1 KiB of consecutive bytes per plane
        const uint4 r0 = *(const uint4*)(p.act + (t0 + l31) * 16 + kh * 8);
        const uint4 r1 = *(const uint4*)(p.act + (p.plane_stride + t0 + l31) * 16 + kh * 8);
        // the RMW operands of this lane's items: issued before the MFMAs so that their latency overlaps
        uint4 gq8[2], old8[2];
        if (!LOGITS) {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int item = lane + 64 * it;
                const int c = item >> 2, grp = item & 3;
                gq8[it] = make_uint4(0x3c003c00u, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u);  // 1.0 (no Gaussian)
                old8[it] = make_uint4(0, 0, 0, 0);
                if (item < n_items) {
                    if (p.gauss) gq8[it] = *(const uint4*)(p.gauss + t0 + 8 * grp);
                    const unsigned short* src = (c < p.C ? p.acc + (size_t)c * vv : p.nacc) + v0 + 8 * grp;
                    old8[it] = *(const uint4*)src;
                }
            }
        }
        const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        f32x16 d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, xform(r0, 0), zero, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, xform(r1, 1), d, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) slab[(8 * (i >> 2) + 4 * kh + (i & 3)) * 36 + l31] = d[i] + s_bz[kh][i];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int item = lane + 64 * it;
            const int c = item >> 2, grp = item & 3;
            if (item < n_items) {
                float4 lo = make_float4(1.f, 1.f, 1.f, 1.f), hi = lo;  // the n_predictions row adds the Gaussian itself
                if (c < p.C) {
                    lo = *(const float4*)(slab + c * 36 + 8 * grp);
                    hi = *(const float4*)(slab + c * 36 + 8 * grp + 4);
                }
                if (LOGITS) {
                    float* dst = p.logits + (size_t)c * pv + t0 + 8 * grp;
                    *(float4*)dst = lo;
                    *(float4*)(dst + 4) = hi;
                } else {
                    union {
                        uint4 u;
                        unsigned short h[8];
                    } g, o;
                    g.u = gq8[it];
                    o.u = old8[it];
                    const float sum[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float gg = us2f(g.h[e]);
                        const float pr = (p.gauss || c >= p.C) ? sum[e] * gg : sum[e];  // prediction *= gaussian (fp32); n += g
                        o.h[e] = f2us(us2f(o.h[e]) + pr);                               // fp16 += fp32 (fp32 add, RTNE)
                    }
                    unsigned short* dst = (c < p.C ? p.acc + (size_t)c * vv : p.nacc) + v0 + 8 * grp;
                    *(uint4*)dst = o.u;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

int launch_head(boa_ctx* ctx, const __half* act, const float* ss, int F0, const int P[3], int C, const float* w,
                const float* bias, float slope, float* logits_out, const uint16_t* gauss, uint16_t* acc,
                uint16_t* nacc, const int PV[3], const int start[3], size_t plane_stride) {
    BOA_REQUIRE(F0 == 32 || F0 == 64, "head: features[0]=%d unsupported (32 or 64)", F0);
    HeadArgs a;
    a.act = act; a.ss = ss; a.F0 = F0; a.P0 = P[0]; a.P1 = P[1]; a.P2 = P[2]; a.C = C; a.w = w; a.bias = bias;
    a.slope = slope; a.logits = logits_out; a.gauss = gauss; a.acc = acc; a.nacc = nacc;
    a.plane_stride = plane_stride ? plane_stride : (size_t)P[0] * P[1] * P[2];
    bool pair = (P[2] % 2 == 0) && F0 == 32;
    if (!logits_out) {
        for (int d = 0; d < 3; ++d)
            BOA_REQUIRE(start[d] >= 0 && start[d] + P[d] <= PV[d], "head: tile [%d,%d) outside accumulator dim %d (%d)",
                        start[d], start[d] + P[d], d, PV[d]);
        a.V0 = PV[0]; a.V1 = PV[1]; a.V2 = PV[2]; a.s0 = start[0]; a.s1 = start[1]; a.s2 = start[2];
        pair = pair && (PV[2] % 2 == 0) && (start[2] % 2 == 0) && (((uintptr_t)acc) % 4 == 0);
    } else {
        a.V0 = a.V1 = a.V2 = a.s0 = a.s1 = a.s2 = 0;
    }
    size_t pv = (size_t)P[0] * P[1] * P[2];
    size_t lds = ((size_t)C * F0 + C + 2 * F0) * 4;
    // the VALU head keeps the weights of every class in LDS: more than the 64 KiB a kernel gets by default from 251 classes on at F0 = 64
    // (k_head<64, 1>; boa_finalize_labels takes 255 at most, 33 KiB at F0 = 32), so that kernel's limit is raised for such a launch
    BOA_REQUIRE(lds <= (F0 == 64 ? 160 : 64) * 1024, "head: features[0]=%d with %d classes needs %zu bytes of LDS", F0, C, lds);
    if (lds > 64 * 1024)
        BOA_HIP_TRY(hipFuncSetAttribute((const void*)k_head<64, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    double bytes = (double)pv * (2.0 * F0 + (logits_out ? 4.0 * C : (4.0 * (C + 1) + 2.0)));
    KernelTimer tm(ctx, BOA_K_HEAD_ACCUM, 2.0 * pv * F0 * C, bytes);
    const bool mfma_shape = F0 == 32 && C <= 31 && P[2] % 32 == 0 && ((uintptr_t)act) % 16 == 0;
    const unsigned mfma_grid = (unsigned)std::min<size_t>(std::max<size_t>(pv / 32 / 4, 1), (size_t)ctx->cu_count * 8);
    // 16-byte accumulator accesses: the tile's z origin, the volume's z extent and the buffers must be 8-voxel aligned
    if (!logits_out && mfma_shape && start[2] % 8 == 0 && PV[2] % 8 == 0 && ((uintptr_t)acc) % 16 == 0 &&
        ((uintptr_t)nacc) % 16 == 0 && (!gauss || ((uintptr_t)gauss) % 16 == 0)) {
        hipLaunchKernelGGL(k_head_mfma<false>, dim3(mfma_grid), dim3(256), 0, ctx->stream, a);
        ctx->counters[BOA_CNT_HEAD_MFMA]++;
    } else if (logits_out && mfma_shape && ((uintptr_t)logits_out) % 16 == 0) {
        hipLaunchKernelGGL(k_head_mfma<true>, dim3(mfma_grid), dim3(256), 0, ctx->stream, a);
        ctx->counters[BOA_CNT_HEAD_MFMA]++;
    } else if (!logits_out && mfma_shape) {
        // accumulators that do not allow the 16-byte read-modify-write (tile z origin / volume z extent not 8-aligned: the common
        // case for real CT sizes): the SAME MFMA logits (logits mode) into a scratch buffer, then the reference's accumulate step on
        // them (k_accumulate_tile: identical arithmetic, tests/test_gpu_head.py) -- so that every tile's logits come from the same
        // kernel whatever its alignment, and the logits API agrees bit for bit with the label path (gather head).  (Round 2 fell
        // back to an fp32 VALU head here, whose logits differ in the last bits.)
        float* tmp = nullptr;
        if (boa_malloc(ctx, (size_t)C * pv * sizeof(float), (void**)&tmp) != BOA_OK) {
            tm.stop();
            return BOA_ENOMEM;
        }
        HeadArgs al = a;
        al.logits = tmp;
        hipLaunchKernelGGL(k_head_mfma<true>, dim3(mfma_grid), dim3(256), 0, ctx->stream, al);
        tm.stop();
        ctx->counters[BOA_CNT_HEAD_MFMA]++;
        const int rc = boa_accumulate_tile(ctx, tmp, gauss, acc, nacc, C, P, PV, start);
        boa_free(ctx, tmp);
        if (rc) return rc;
        BOA_HIP_TRY(hipGetLastError());
        return BOA_OK;
    } else {
        if (pair)
            hipLaunchKernelGGL((k_head<32, 2>), dim3((unsigned)((pv / 2 + 255) / 256)), dim3(256), lds, ctx->stream, a);
        else if (F0 == 32)
            hipLaunchKernelGGL((k_head<32, 1>), dim3((unsigned)((pv + 255) / 256)), dim3(256), lds, ctx->stream, a);
        else
            hipLaunchKernelGGL((k_head<64, 1>), dim3((unsigned)((pv + 255) / 256)), dim3(256), lds, ctx->stream, a);
        ctx->counters[BOA_CNT_HEAD_VALU]++;
    }
    tm.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}
