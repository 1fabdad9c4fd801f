// Class probabilities from the fold-mean fp16 logits (boa_logits_to_probabilities): the device form of
// convert_predicted_logits_to_segmentation_with_correct_shape(..., return_probabilities=True)
// (NN/inference/export_prediction.py:14-71) -- order-1 resampling of the logits (resample_logits.h, the arithmetic of
// boa_resize_logits_argmax), fp32 softmax and the first-maximum argmax of the probabilities (softmax_codes.h), the crop revert
// with background (1, 0, ..., 0) outside the box (label_handling.py:197-220) and the transpose_backward, in one pass.
//
// Two kernels.  k_prob_rows is the pass every shipped plan takes (identity perm, no resampling): HBM-bound, lanes along the
// fastest axis, one coalesced read per class plane with the exponentials of up to 32 classes held in registers, C fp32 planes and
// the label plane written with whole lines.  More than 32 classes: three loops over the classes (maximum, sum, quotient) that
// re-read the logits, which the first loop left in L2.  k_prob_voxel takes everything else (resampling, the five other
// permutations): one thread per output voxel, the column kept in the output planes between the sum and the division.
#include "common.h"
#include "resample_logits.h"
#include "softmax_codes.h"

struct ProbArgs {
    LogitsResizeGeom g;   // g.O: the dims of the box that is inserted (== g.I without resampling)
    int resample;
    int lo[3], F[3];      // where the box goes in the pre-crop grid, and that grid
    int perm[3], D[3];    // output axis i is axis perm[i] of the pre-crop grid: D[i] = F[perm[i]]
    float* prob;          // [C][D0][D1][D2]
    unsigned char* labels;  // [D0][D1][D2] or NULL
    unsigned char lut[256];
};

template <int VEC>
__device__ __forceinline__ void load_half_vec(const unsigned short* p, unsigned short v[VEC]) {
    if (VEC == 4) {
        *(uint2*)v = *(const uint2*)p;
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = p[j];
    }
}

template <int VEC>
__device__ __forceinline__ void store_float_vec(float* p, const float v[VEC]) {
    if (VEC == 4) {
        // nobody reads the planes again in this pass: streaming stores (still one 16-byte store per lane) left the L2 to the logits
        // and measured 0.66 against 0.74 ms at C = 25 on 256^3
        __builtin_nontemporal_store(v[0], p);
        __builtin_nontemporal_store(v[1], p + 1);
        __builtin_nontemporal_store(v[2], p + 2);
        __builtin_nontemporal_store(v[3], p + 3);
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) p[j] = v[j];
    }
}

// VEC voxels of one row per thread (VEC == 4: every fastest extent and offset is a multiple of 4, so the four share one side of
// the box and every access is one aligned 8 / 16 / 4 byte word).  CR > 0: C <= CR classes in registers; CR == 0: the class loops.
template <int VEC, int CR>
__global__ __launch_bounds__(256) void k_prob_rows(ProbArgs a) {
    const unsigned rowv = (unsigned)a.F[2] / VEC;
    const size_t nvec = (size_t)a.F[0] * a.F[1] * rowv;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nvec) return;
    const unsigned u = (unsigned)t;                 // F0 F1 F2 < 2^31 (checked by the host entry)
    const unsigned r = u / rowv;
    const int z = (int)(u - r * rowv) * VEC, x = (int)(r / (unsigned)a.F[1]), y = (int)(r - (unsigned)x * (unsigned)a.F[1]);
    const size_t fv = (size_t)a.F[0] * a.F[1] * a.F[2];
    const size_t oi = ((size_t)x * a.F[1] + y) * a.F[2] + z;
    float* out = a.prob + oi;
    const int bx = x - a.lo[0], by = y - a.lo[1], bz = z - a.lo[2];
    const int C = a.g.C;
    int label[VEC];
    if (bx < 0 || by < 0 || bz < 0 || bx >= a.g.O[0] || by >= a.g.O[1] || bz >= a.g.O[2]) {
        // revert_cropping_on_probabilities: zeros, channel 0 set to 1
        float v[VEC];
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = c == 0 ? 1.f : 0.f;
            store_float_vec<VEC>(out + (size_t)c * fv, v);
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) label[j] = 0;
    } else {
        const size_t lv = (size_t)a.g.L[0] * a.g.L[1] * a.g.L[2];
        const unsigned short* src = a.g.logits + ((size_t)(bx + a.g.off[0]) * a.g.L[1] + (by + a.g.off[1])) * a.g.L[2] + (bz + a.g.off[2]);
        float m[VEC], s[VEC], best[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            s[j] = 0.f;
            best[j] = 0.f;
            label[j] = 0;
        }
        if (CR > 0) {
            float e[CR > 0 ? CR : 1][VEC];
#pragma unroll
            for (int c = 0; c < CR; ++c)
                if (c < C) {
                    unsigned short h[VEC];
                    load_half_vec<VEC>(src + (size_t)c * lv, h);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        e[c][j] = smx_half_bits_to_float(h[j]);
                        m[j] = c == 0 ? e[c][j] : smx_max(m[j], e[c][j]);
                    }
                }
#pragma unroll
            for (int c = 0; c < CR; ++c)
                if (c < C) {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        e[c][j] = smx_exp(e[c][j], m[j]);
                        s[j] += e[c][j];
                    }
                }
#pragma unroll
            for (int c = 0; c < CR; ++c)
                if (c < C) {
                    float p[VEC];
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        p[j] = smx_div(e[c][j], s[j]);
                        smx_first_max(p[j], c, best[j], label[j]);
                    }
                    store_float_vec<VEC>(out + (size_t)c * fv, p);
                }
        } else {
            unsigned short h[VEC];
            for (int c = 0; c < C; ++c) {
                load_half_vec<VEC>(src + (size_t)c * lv, h);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float f = smx_half_bits_to_float(h[j]);
                    m[j] = c == 0 ? f : smx_max(m[j], f);
                }
            }
            for (int c = 0; c < C; ++c) {
                load_half_vec<VEC>(src + (size_t)c * lv, h);
#pragma unroll
                for (int j = 0; j < VEC; ++j) s[j] += smx_exp(smx_half_bits_to_float(h[j]), m[j]);
            }
            for (int c = 0; c < C; ++c) {
                load_half_vec<VEC>(src + (size_t)c * lv, h);
                float p[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    p[j] = smx_div(smx_exp(smx_half_bits_to_float(h[j]), m[j]), s[j]);   // the same expf of the same operands as in the sum
                    smx_first_max(p[j], c, best[j], label[j]);
                }
                store_float_vec<VEC>(out + (size_t)c * fv, p);
            }
        }
    }
    if (a.labels) {
        if (VEC == 4) {
            *(uchar4*)(a.labels + oi) = make_uchar4(a.lut[label[0]], a.lut[label[1]], a.lut[label[2]], a.lut[label[3]]);
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) a.labels[oi + j] = a.lut[label[j]];
        }
    }
}

// one output voxel per thread: any permutation, with or without resampling
__global__ __launch_bounds__(256) void k_prob_voxel(ProbArgs a) {
    const size_t dv = (size_t)a.D[0] * a.D[1] * a.D[2];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= dv) return;
    int o[3], q[3], b[3];
    idx3(i, a.D[1], a.D[2], o[0], o[1], o[2]);
#pragma unroll
    for (int d = 0; d < 3; ++d) {      // (no dynamic index into q: it stays in registers)
        if (a.perm[d] == 0) q[0] = o[d];
        if (a.perm[d] == 1) q[1] = o[d];
        if (a.perm[d] == 2) q[2] = o[d];
    }
    bool inside = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        b[d] = q[d] - a.lo[d];
        inside = inside && b[d] >= 0 && b[d] < a.g.O[d];
    }
    float* out = a.prob + i;
    const int C = a.g.C;
    int label = 0;
    if (!inside) {
        for (int c = 0; c < C; ++c) out[(size_t)c * dv] = c == 0 ? 1.f : 0.f;
    } else if (a.resample) {
        LogitsTaps t;
        logits_taps(a.g, b, t);
        label = smx_column_of([&](int c) { return logits_resampled(a.g, t, c); }, C, out, dv);
    } else {
        const size_t lv = (size_t)a.g.L[0] * a.g.L[1] * a.g.L[2];
        const unsigned short* src = a.g.logits + ((size_t)(b[0] + a.g.off[0]) * a.g.L[1] + (b[1] + a.g.off[1])) * a.g.L[2] + (b[2] + a.g.off[2]);
        label = smx_column(src, lv, C, out, dv);
    }
    if (a.labels) a.labels[i] = a.lut[label];
}

template <int VEC>
static void launch_rows(boa_ctx* c, const ProbArgs& a) {
    const size_t nvec = (size_t)a.F[0] * a.F[1] * (a.F[2] / VEC);
    const dim3 grid((unsigned)((nvec + 255) / 256)), block(256);
    const int C = a.g.C;
    if (C <= 4) hipLaunchKernelGGL((k_prob_rows<VEC, 4>), grid, block, 0, c->stream, a);
    else if (C <= 8) hipLaunchKernelGGL((k_prob_rows<VEC, 8>), grid, block, 0, c->stream, a);
    else if (C <= 16) hipLaunchKernelGGL((k_prob_rows<VEC, 16>), grid, block, 0, c->stream, a);
    else if (C <= 32) hipLaunchKernelGGL((k_prob_rows<VEC, 32>), grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL((k_prob_rows<VEC, 0>), grid, block, 0, c->stream, a);
}

extern "C" int boa_logits_to_probabilities(boa_ctx* c, const uint16_t* dev_logits, int C, const int grid_dims[3], const int* crop_off,
                                           const int* crop_dims, const int* out_dims, int slice_axis, const int bbox_lo[3],
                                           const int full_dims[3], const int perm[3], float* dev_prob, const uint8_t* host_lut,
                                           uint8_t* dev_labels) {
    BOA_REQUIRE(c && dev_logits && grid_dims && bbox_lo && full_dims && perm && dev_prob, "boa_logits_to_probabilities: NULL argument");
    BOA_REQUIRE(C >= 1 && C <= SMX_MAX_CLASSES, "boa_logits_to_probabilities: C=%d out of range", C);
    BOA_REQUIRE(slice_axis >= -1 && slice_axis <= 2, "boa_logits_to_probabilities: slice_axis %d", slice_axis);
    ProbArgs a;
    int bad = 0;
    const int* box = crop_dims ? crop_dims : grid_dims;
    BOA_REQUIRE(logits_resize_geom(&a.g, dev_logits, C, grid_dims, crop_off, crop_dims, out_dims ? out_dims : box, slice_axis, &bad),
                "boa_logits_to_probabilities: bad geometry on axis %d", bad);
    a.resample = 0;
    int seen = 0;
    for (int d = 0; d < 3; ++d) {
        a.resample |= a.g.O[d] != a.g.I[d];
        a.lo[d] = bbox_lo[d];
        a.F[d] = full_dims[d];
        BOA_REQUIRE(a.F[d] >= 1 && a.lo[d] >= 0 && a.lo[d] <= a.F[d] && a.g.O[d] <= a.F[d] - a.lo[d],
                    "boa_logits_to_probabilities: the box [%d, %d + %d) leaves the grid of %d on axis %d", a.lo[d], a.lo[d], a.g.O[d], a.F[d], d);
        BOA_REQUIRE(perm[d] >= 0 && perm[d] <= 2, "boa_logits_to_probabilities: perm[%d] = %d", d, perm[d]);
        seen |= 1 << perm[d];
        a.perm[d] = perm[d];
    }
    BOA_REQUIRE(seen == 7, "boa_logits_to_probabilities: perm (%d, %d, %d) is not a permutation", perm[0], perm[1], perm[2]);
    for (int d = 0; d < 3; ++d) a.D[d] = a.F[a.perm[d]];
    const long long lim = 1ll << 31;
    const long long lv = (long long)a.g.L[0] * a.g.L[1], fv = (long long)a.F[0] * a.F[1];
    BOA_REQUIRE(lv < lim && lv * a.g.L[2] < lim && fv < lim && fv * a.F[2] < lim, "boa_logits_to_probabilities: a class plane has 2^31 voxels or more");
    a.prob = dev_prob;
    a.labels = dev_labels;
    for (int i = 0; i < 256; ++i) a.lut[i] = host_lut ? host_lut[i] : (unsigned char)i;
    const size_t nfull = (size_t)(fv * a.F[2]), nbox = (size_t)a.g.O[0] * a.g.O[1] * a.g.O[2];
    KernelTimer t(c, BOA_K_ARGMAX, 0, (double)nbox * 2.0 * C + (double)nfull * (4.0 * C + (dev_labels ? 1.0 : 0.0)));
    const bool ident = a.perm[0] == 0 && a.perm[1] == 1 && a.perm[2] == 2;
    if (ident && !a.resample) {
        const bool vec4 = ((a.F[2] | a.g.L[2] | a.g.O[2] | a.lo[2] | a.g.off[2]) & 3) == 0 && ((uintptr_t)dev_logits & 7) == 0 &&
                          ((uintptr_t)dev_prob & 15) == 0 && ((uintptr_t)dev_labels & 3) == 0;
        if (vec4) launch_rows<4>(c, a);
        else launch_rows<1>(c, a);
    } else {
        hipLaunchKernelGGL(k_prob_voxel, dim3((unsigned)((nfull + 255) / 256)), dim3(256), 0, c->stream, a);
    }
    t.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}
