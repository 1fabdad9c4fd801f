// 3-D convolution stack for gfx950: implicit-GEMM 3x3x3 / strided conv on f16 MFMA (32x32x16) with the
// producer's InstanceNorm+LeakyReLU applied while staging the LDS halo tile, InstanceNorm statistics reduced in
// the epilogue (deterministic per-block partials).  This file: the weight packers, tile selection, the variant-0 conv
// k_conv_mfma, the InstanceNorm finalize and the layout helpers.  The other kernel families have files of their own:
// conv_ws.hip / conv_ns.hip (the producer/consumer and N-split convs), conv_first.hip (first layer, tiles read out of the
// resident volume), convt.hip (transposed conv, kernel == stride), head.hip (1x1x1 head + Gaussian fp16 accumulation).
//
// Replaces `self.network(x)` (NN/inference/predict_from_raw_data.py:543), i.e. dynamic_network_architectures'
// PlainConvUNet as configured by NN/utilities/plans_handling/plans_handler.py:59-92.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "conv.h"


// ======================================================================================================
// host-side weight packing
// A-operand image for v_mfma_f32_32x32x16_f16: lane l holds A[i = l & 31][k = 8 * (l >> 5) + j], j = 0..7, so a
// (tap, 16-channel chunk, k-half) fragment is 32 couts x 8 halves = 512 contiguous bytes.
// conv:  [cc = Cin/16][tap][khalf][Cout][8]
size_t conv_wpk_halves(int Cin_total, int Cout, const int k[3]) {
    return (size_t)(Cin_total / 16) * k[0] * k[1] * k[2] * 2 * Cout * 8;
}

void pack_conv_weights(const float* w, int Cin, int Cout, const int k[3], __half* dst) {
    const int taps = k[0] * k[1] * k[2];
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int t = 0; t < taps; ++t) {
                int cc = ci / 16, kh = (ci % 16) / 8, j = ci % 8;
                size_t o = ((((size_t)cc * taps + t) * 2 + kh) * Cout + co) * 8 + j;
                dst[o] = __float2half_rn(w[((size_t)co * Cin + ci) * taps + t]);
            }
}

// convT: [tap][cc = Cin/16][khalf][Cout][8]
size_t convt_wpk_halves(int Cin, int Cout, const int s[3]) { return (size_t)s[0] * s[1] * s[2] * Cin * Cout; }

void pack_convt_weights(const float* w, int Cin, int Cout, const int s[3], __half* dst) {
    const int taps = s[0] * s[1] * s[2];
    const int ncc = Cin / 16;
    for (int ci = 0; ci < Cin; ++ci)
        for (int co = 0; co < Cout; ++co)
            for (int t = 0; t < taps; ++t) {
                int cc = ci / 16, kh = (ci % 16) / 8, j = ci % 8;
                size_t o = ((((size_t)t * ncc + cc) * 2 + kh) * Cout + co) * 8 + j;
                dst[o] = __float2half_rn(w[((size_t)ci * Cout + co) * taps + t]);
            }
}

// ---- split-precision mode (precision 2) --------------------------------------------------------------
// One K = 16 MFMA step covers 8 real input channels: conv [cc = Cin/8][tap][part: hi, lo][Cout][8], convT
// [tap][cc = Cin/8][part][Cout][8]; every weight is scaled by `scale` (a power of two chosen per layer so that the largest
// magnitude sits just below 2^14: the lo parts of typical weights then stay out of the fp16 subnormal range) and split as
// hi = half(w s), lo = half(w s - hi).
float x3_weight_scale(const float* w, size_t n) {
    float m = 0.f;
    for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(w[i]));
    if (!(m > 0.f) || !std::isfinite(m)) return 1.f;
    int e;
    std::frexp(m, &e);               // m = f * 2^e, f in [0.5, 1)
    return std::ldexp(1.f, std::max(-24, std::min(14 - e, 40)));   // m * scale in [2^13, 2^14)
}

float x3_output_fold(const float* w, size_t n, int cin, const float* bias, int cout) {
    // output scale of a transposed conv fed with O(1) activations: sqrt(Cin) rms(w), or the largest bias if that is larger
    double q = 0.0, bmax = 0.0;
    for (size_t i = 0; i < n; ++i) q += (double)w[i] * w[i];
    for (int i = 0; i < cout; ++i) bmax = std::max(bmax, (double)std::fabs(bias[i]));
    const double mag = std::max(std::sqrt(q / std::max<size_t>(n, 1) * cin), bmax);
    if (!(mag > 0.0) || !std::isfinite(mag)) return 1.f;
    const int e = (int)std::lround(-std::log2(mag));
    // within [-2, 2] the fold changes nothing worth a different rounding of the consumer's weights: keep the bits of the unfolded net
    return (e >= -2 && e <= 2) ? 1.f : std::ldexp(1.f, std::max(-30, std::min(e, 30)));
}

static inline void x3_split(float v, __half* hi, __half* lo) {
    const __half h = __float2half_rn(v);
    *hi = h;
    *lo = __float2half_rn(v - __half2float(h));
}

size_t conv_wpk_halves_x3(int Cin_total, int Cout, const int k[3]) { return (size_t)(Cin_total / 8) * k[0] * k[1] * k[2] * 2 * Cout * 8; }

void pack_conv_weights_x3(const float* w, int Cin, int Cout, const int k[3], float scale, __half* dst) {
    const int taps = k[0] * k[1] * k[2];
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int t = 0; t < taps; ++t) {
                const int cc = ci / 8, j = ci % 8;
                const size_t o = ((((size_t)cc * taps + t) * 2 + 0) * Cout + co) * 8 + j;
                x3_split(w[((size_t)co * Cin + ci) * taps + t] * scale, &dst[o], &dst[o + (size_t)Cout * 8]);
            }
}

size_t convt_wpk_halves_x3(int Cin, int Cout, const int s[3]) { return (size_t)s[0] * s[1] * s[2] * Cin * Cout * 2; }

void pack_convt_weights_x3(const float* w, int Cin, int Cout, const int s[3], float scale, __half* dst) {
    const int taps = s[0] * s[1] * s[2];
    const int ncc = Cin / 8;
    for (int ci = 0; ci < Cin; ++ci)
        for (int co = 0; co < Cout; ++co)
            for (int t = 0; t < taps; ++t) {
                const int cc = ci / 8, j = ci % 8;
                const size_t o = ((((size_t)t * ncc + cc) * 2 + 0) * Cout + co) * 8 + j;
                x3_split(w[((size_t)ci * Cout + co) * taps + t] * scale, &dst[o], &dst[o + (size_t)Cout * 8]);
            }
}

// ======================================================================================================
// tile selection
static int next_pow2(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

static size_t conv_lds_bytes(int HV, int taps) {
    size_t plane = (size_t)HV * 16 + 64;
    return 2 * plane + (size_t)taps * 1024 + (size_t)HV * 4 + 1024;
}

size_t conv_ws_lds_bytes(int HV, int taps, int ncc, int Cout);
bool conv_ws_supported(const int k[3], int HV);
bool conv_ws_resident(int HV, int taps, int ncc, int Cout);

// Completes a candidate (variant 0 / 1, R, w, b) for the geometry: halo h, padded plane stride xs, block tiles per axis and the LDS
// bytes; *hv_out = the halo voxels the kernel stages (variant 1: the padded planes).  false: the kernel does not take the candidate
// (conv_ws_supported, the LDS limit).  Shared by choose_conv_tile's search and the plan query / plan override of the test seams
// (net_debug.hip), so that an overridden plan is completed and refused exactly as the search would.
bool conv_tile_complete(const ConvGeom& g, bool x3, ConvTile* t, long long* hv_out) {
    const int dims[3] = {g.Do, g.Ho, g.Wo};
    const int taps = g.k[0] * g.k[1] * g.k[2];
    const int ncc = x3 ? g.Cin / 8 : g.Cin / 16;
    const int variant = t->variant;
    const int* w = t->w;
    int* h = t->h;
    long long HV = 1;
    for (int d = 0; d < 3; ++d) {
        const int ext = t->b[d] * w[d];
        h[d] = (ext - 1) * g.s[d] + g.k[d];
        t->tiles[d] = ceil_div(dims[d], ext);
        HV *= h[d];
    }
    // k_conv_ws, M-tiles that span several x-planes (w0 > 1, rows of w2 = 8 / 16 lanes: the 16^3 ... 4^3 layers):
    // lane row lx sits xs voxels = xs * 16 bytes behind row lx - 1, and with xs = h1 * h2 (180 / 100 at the 16^3 / 8^3
    // layers: = 64 bytes mod 256) the rows of a ds_read_b128 lane group overlapped on the banks -- 35 - 44 % of these
    // launches' LDS cycles were conflicts (profiles/r05_pmc_lds.txt).  The planes are padded to xs = w2 (mod 16): the
    // rows of every lane group then tile a 256-byte bank row.  HV below counts the padded planes.
    int xs = h[1] * h[2];
    if (variant == 1 && w[0] > 1 && w[1] == 1 && w[2] >= 8 && w[2] <= 16 && g.s[0] == 1 && g.s[2] == 1)
        while (xs % 16 != w[2] % 16) ++xs;
    if (variant == 1) HV = (long long)h[0] * xs;
    if (variant == 1 && !conv_ws_supported(g.k, (int)HV)) return false;
    const size_t lds = variant == 1 ? conv_ws_lds_bytes((int)HV, taps, ncc, g.Cout) : conv_lds_bytes((int)HV, taps);
    if (lds > 160 * 1024 - 2048) return false;   // (2 KiB stay free for the split-precision kernel's bias table)
    t->xs = xs;
    t->lds_bytes = lds;
    if (hv_out) *hv_out = HV;
    return true;
}

// Pick the wave M-tile shape, the block tile and the kernel variant.  Cost model (cycles per 32-voxel M-tile):
//   variant 1 (k_conv_ws): chunk time = max(MFMA time of the consumers, staging time of the producers) + barrier;
//   variant 0 (k_conv_mfma): MFMA and staging serialised inside a block, partly hidden by the second block on the CU.
bool choose_conv_tile(const ConvGeom& g, int cu_count, ConvTile* out, bool x3) {
    const int dims[3] = {g.Do, g.Ho, g.Wo};
    const int taps = g.k[0] * g.k[1] * g.k[2];
    const int ncc = x3 ? g.Cin / 8 : g.Cin / 16;   // split-precision mode: 8 real channels per staged chunk, two MFMAs per tap
    double best_cost = 1e30;
    bool found = false;
    if (conv_ns_applicable(g)) {  // N-split kernel (conv_ns.hip): stride-2 layers (split-precision mode too), fixed tile shape
        conv_ns_tile(g, out);
        return true;
    }
    // wave M-tile shapes: 32 voxels = w0 x w1 x w2 (powers of two), contiguous axis as long as possible first
    // (second pass: extents so small that no wave tile fits without overhang -- e.g. a last axis of 2 -- take any shape; the
    // kernels mask the overhang)
    for (int relax = 0; relax < 2 && !found; ++relax)
    for (int w2 = 32; w2 >= 4; w2 >>= 1) {
        if (!relax && w2 > next_pow2(dims[2])) continue;
        for (int w1 = 1; w1 * w2 <= 32; w1 <<= 1) {
            const int w0 = 32 / (w2 * w1);
            if (!relax && (w1 > next_pow2(dims[1]) || w0 > next_pow2(dims[0]))) continue;
            const int w[3] = {w0, w1, w2};
            for (int variant : {1, 0}) {
                if (x3 && variant != 1) continue;
                for (int R : {4, 2, 1}) {
                    const int M = 4 * R;
                    for (int b0 = 1; b0 <= M; b0 *= 2)
                        for (int b1 = 1; b0 * b1 <= M; b1 *= 2) {
                            const int b2 = M / (b0 * b1);
                            if (b0 * b1 * b2 != M) continue;
                            const int b[3] = {b0, b1, b2};
                            ConvTile c;
                            c.variant = variant;
                            c.R = R;
                            for (int d = 0; d < 3; ++d) {
                                c.w[d] = w[d];
                                c.b[d] = b[d];
                            }
                            long long HV;
                            if (!conv_tile_complete(g, x3, &c, &HV)) continue;
                            const int* h = c.h;
                            const int* tl = c.tiles;
                            const size_t lds = c.lds_bytes;
                            long long covered = 1, tiles = 1;
                            for (int d = 0; d < 3; ++d) {
                                covered *= (long long)tl[d] * b[d] * w[d];
                                tiles *= tl[d];
                            }
                            const long long nblocks = tiles * (g.Cout / 32) * g.N;
                            const double valid = (double)dims[0] * dims[1] * dims[2];
                            const double waste = (double)covered / valid;
                            // LDS fragment reads are conflict-free when a wave row is contiguous (w2 lanes at the
                            // stride of the conv); short rows / strided rows cost extra LDS cycles
                            // (measured: an 8x8x8 block tile of 4x1x8 wave tiles stages 26 % fewer halo voxels than 4x4x32 of 1x1x32 wave
                            // tiles and is still 2-4 % slower: rows shorter than 32 lanes cost fragment-read conflicts)
                            const double lds_pen = (g.s[2] > 1 ? 1.25 : 1.0) * (w2 < 16 ? 1.3 : (w2 < 32 ? 1.15 : 1.0));
                            const double t_mfma = (double)taps * R * 32.0 * lds_pen * (x3 ? 2.0 : 1.0);
                            double t_chunk;
                            const double slots = cu_count;
                            if (variant == 1) {
                                const bool res = conv_ws_resident((int)HV, taps, ncc, g.Cout);
                                // measured (s_memtime stamps, 32->32 @128^3): a 1360-voxel chunk costs the producers ~6500
                                // cycles next to the consumers' MFMA stream -> ~4.3 cycles per halo voxel + fixed part
                                const double t_prod = (double)h[0] * h[1] * h[2] * 4.3 + (res ? 0.0 : taps * 64.0 / 256.0 * 60.0) + 800.0;   // (the halo's voxels, not the padded planes)
                                t_chunk = std::max(t_mfma * 1.15, t_prod * (g.s[2] > 1 ? 1.0 : lds_pen)) + 500.0;
                            } else {
                                const double items = (2.0 * HV + taps * 64.0) / 256.0;
                                const int bpc = lds <= 78 * 1024 ? 2 : 1;
                                t_chunk = (taps * R * 200.0 + items * 1500.0 + 400.0) / (bpc == 2 ? 1.8 : 1.0);
                            }
                            // epilogue + tile turnaround amortised over the chunks of a tile
                            const double t_tile = t_chunk * ncc + (variant == 1 ? 3000.0 : 6000.0);
                            const double rounds = std::ceil((double)nblocks / slots);
                            const double cost = t_tile * rounds * waste / (double)M * (slots / (double)nblocks);
                            if (cost < best_cost) {
                                best_cost = cost;
                                found = true;
                                *out = c;
                            }
                        }
                }
            }
        }
    }
    return found;
}

// number of per-(n, cout) partial-statistics entries the conv kernel writes
int conv_nblk(const ConvTile& t, int cu_count, int Cout) {
    const int spatial = t.tiles[0] * t.tiles[1] * t.tiles[2];
    if (t.variant == 2) return conv_ws_nslots(spatial * conv_ns_ncy(Cout), cu_count);
    return t.variant == 1 ? conv_ws_nslots(spatial * (Cout / 32), cu_count) : spatial;
}

// ======================================================================================================
// MFMA conv kernel
template <int R>
__global__ __launch_bounds__(256) void k_conv_mfma(ConvArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int kh = lane >> 5;
    const int taps = p.k0 * p.k1 * p.k2;
    const int HV = p.h0 * p.h1 * p.h2;
    const int plane = HV * 16 + 64;
    unsigned char* lds_in = smem;
    unsigned char* lds_w = smem + 2 * plane;
    int* lds_tab = (int*)(lds_w + taps * 1024);
    float* lds_red = (float*)(lds_tab + HV);

    const int n = blockIdx.z;
    const int cout0 = blockIdx.y * 32;
    int bt = blockIdx.x;
    const int tz = bt % p.t2;
    bt /= p.t2;
    const int ty = bt % p.t1;
    const int tx = bt / p.t1;
    const int ox0 = tx * p.b0 * p.w0, oy0 = ty * p.b1 * p.w1, oz0 = tz * p.b2 * p.w2;
    const int ix0 = ox0 * p.s0 - p.p0, iy0 = oy0 * p.s1 - p.p1, iz0 = oz0 * p.s2 - p.p2;

    // halo voxel -> input voxel index table (-1 = zero padding), reused by every channel chunk
    for (int v = tid; v < HV; v += 256) {
        int hz = v % p.h2;
        int t = v / p.h2;
        int hy = t % p.h1;
        int hx = t / p.h1;
        int ix = ix0 + hx, iy = iy0 + hy, iz = iz0 + hz;
        bool inb = ix >= 0 && ix < p.Di && iy >= 0 && iy < p.Hi && iz >= 0 && iz < p.Wi;
        lds_tab[v] = inb ? (ix * p.Hi + iy) * p.Wi + iz : -1;
    }

    // per-lane voxel of each of this wave's M-tiles
    const int lz = l31 % p.w2;
    const int ly = (l31 / p.w2) % p.w1;
    const int lx = l31 / (p.w2 * p.w1);
    int hoff[R];
    int ovox[R];  // output voxel index or -1
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int m = wave * R + r;
        int mz = m % p.b2;
        int t = m / p.b2;
        int my = t % p.b1;
        int mx = t / p.b1;
        int tx_ = mx * p.w0 + lx, ty_ = my * p.w1 + ly, tz_ = mz * p.w2 + lz;
        hoff[r] = ((tx_ * p.s0) * p.h1 + ty_ * p.s1) * p.h2 + tz_ * p.s2;
        int ox = ox0 + tx_, oy = oy0 + ty_, oz = oz0 + tz_;
        ovox[r] = (ox < p.Do && oy < p.Ho && oz < p.Wo) ? (ox * p.Ho + oy) * p.Wo + oz : -1;
    }

    f32x16 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[r][i] = 0.f;

    const size_t in_vox = (size_t)p.Di * p.Hi * p.Wi;
    const int ncc = (p.C0 + p.C1) / 16;
    const int oct = tid & 1;  // this thread always stages the same channel octet of a chunk

    for (int cc = 0; cc < ncc; ++cc) {
        __syncthreads();  // previous chunk fully consumed (also orders the table writes before first use)
        // ---- stage the halo tile of 16 channels, applying the producer's norm + LeakyReLU -------------
        {
            int cg = cc * 16 + oct * 8;
            const __half* base;
            const float* ss;
            int C;
            // chunk-planar activations [N][C/16][voxel][16]: plane of this chunk + this thread's octet
            if (cg < p.C0) {
                base = p.src0 + ((size_t)n * p.C0 + (cg & ~15)) * in_vox + (cg & 15);
                ss = p.ss0 ? p.ss0 + ((size_t)n * p.C0 + cg) * 2 : nullptr;
                C = p.C0;
            } else {
                cg -= p.C0;
                base = p.src1 + ((size_t)n * p.C1 + (cg & ~15)) * in_vox + (cg & 15);
                ss = p.ss1 ? p.ss1 + ((size_t)n * p.C1 + cg) * 2 : nullptr;
                C = p.C1;
            }
            (void)C;
            float sc[8], sh[8];
            if (ss) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    sc[j] = ss[2 * j];
                    sh[j] = ss[2 * j + 1];
                }
            }
            unsigned char* dstp = lds_in + oct * plane;
            for (int i = tid; i < 2 * HV; i += 256) {
                int v = i >> 1;
                int gi = lds_tab[v];
                uint4 val = make_uint4(0, 0, 0, 0);
                if (gi >= 0) {
                    val = *(const uint4*)(base + (size_t)gi * 16);
                    if (ss) val = norm_act8(val, sc, sh, p.slope);
                }
                *(uint4*)(dstp + v * 16) = val;
            }
        }
        // ---- stage this chunk's weights for the block's 32 output channels ----------------------------
        {
            const __half* wsrc = p.wpk + ((size_t)cc * taps * 2) * p.Cout * 8;
            for (int i = tid; i < taps * 64; i += 256) {
                int seg = i >> 5, co = i & 31;
                *(uint4*)(lds_w + i * 16) = *(const uint4*)(wsrc + ((size_t)seg * p.Cout + cout0 + co) * 8);
            }
        }
        __syncthreads();
        // ---- MFMA over the taps -----------------------------------------------------------------------
        const unsigned char* bbase = lds_in + kh * plane;
        const unsigned char* abase = lds_w + (kh * 32 + l31) * 16;
        int tap = 0;
        for (int dx = 0; dx < p.k0; ++dx)
            for (int dy = 0; dy < p.k1; ++dy) {
                const int rowoff = (dx * p.h1 + dy) * p.h2;
#pragma unroll 3
                for (int dz = 0; dz < p.k2; ++dz, ++tap) {
                    f16x8 a = *(const f16x8*)(abase + tap * 1024);
                    const int toff = rowoff + dz;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        f16x8 b = *(const f16x8*)(bbase + (hoff[r] + toff) * 16);
                        acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[r], 0, 0, 0);
                    }
                }
            }
    }

    // ---- epilogue: + bias, fp16 store, InstanceNorm partial statistics ------------------------------
    // D layout: lane holds column (voxel) l31, rows (couts) (i & 3) + 8 * (i >> 2) + 4 * kh
    float s[16], q[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = q[i] = 0.f;
    float bv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) bv[i] = p.bias[cout0 + (i & 3) + 8 * (i >> 2) + 4 * kh];
    const size_t out_vox = (size_t)p.Do * p.Ho * p.Wo;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (ovox[r] < 0) continue;
        // couts cout0 + 8 g + 4 kh + j -> plane cout0 / 16 + g / 2, offset 8 (g % 2) + 4 kh + j
        __half* op = p.out + ((size_t)n * p.Cout + cout0) * out_vox + (size_t)ovox[r] * 16 + 4 * kh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            union {
                uint2 u;
                __half h[4];
            } pk;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v = acc[r][g * 4 + j] + bv[g * 4 + j];
                __half hv = __float2half_rn(v);
                pk.h[j] = hv;
                float vr = __half2float(hv);
                s[g * 4 + j] += vr;
                q[g * 4 + j] = __builtin_fmaf(vr, vr, q[g * 4 + j]);
            }
            *(uint2*)(op + (size_t)(g >> 1) * 16 * out_vox + 8 * (g & 1)) = pk.u;
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
#pragma unroll
        for (int m = 1; m < 32; m <<= 1) {
            s[i] += __shfl_xor(s[i], m);
            q[i] += __shfl_xor(q[i], m);
        }
    }
    __syncthreads();
    if (l31 == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            int row = (i & 3) + 8 * (i >> 2) + 4 * kh;
            lds_red[(wave * 32 + row) * 2 + 0] = s[i];
            lds_red[(wave * 32 + row) * 2 + 1] = q[i];
        }
    }
    __syncthreads();
    if (tid < 64) {
        int row = tid >> 1, j = tid & 1;
        float v = lds_red[(0 * 32 + row) * 2 + j] + lds_red[(1 * 32 + row) * 2 + j];
        v += lds_red[(2 * 32 + row) * 2 + j];
        v += lds_red[(3 * 32 + row) * 2 + j];
        const int nblk = gridDim.x;
        p.partials[(((size_t)n * p.Cout + cout0 + row) * 2 + j) * nblk + blockIdx.x] = v;
    }
}

// the ConvArgs of a conv's geometry, tile, weights and output (the sources are the caller's: their channel units differ)
static ConvArgs conv_args(const ConvGeom& g, const ConvTile& t, const __half* wpk, const float* bias, float slope, __half* out,
                          float* partials) {
    ConvArgs a;
    a.N = g.N; a.Di = g.Di; a.Hi = g.Hi; a.Wi = g.Wi; a.Do = g.Do; a.Ho = g.Ho; a.Wo = g.Wo; a.Cout = g.Cout;
    a.k0 = g.k[0]; a.k1 = g.k[1]; a.k2 = g.k[2]; a.s0 = g.s[0]; a.s1 = g.s[1]; a.s2 = g.s[2];
    a.p0 = (g.k[0] - 1) / 2; a.p1 = (g.k[1] - 1) / 2; a.p2 = (g.k[2] - 1) / 2;
    a.w0 = t.w[0]; a.w1 = t.w[1]; a.w2 = t.w[2]; a.b0 = t.b[0]; a.b1 = t.b[1]; a.b2 = t.b[2];
    a.h0 = t.h[0]; a.h1 = t.h[1]; a.h2 = t.h[2]; a.t0 = t.tiles[0]; a.t1 = t.tiles[1]; a.t2 = t.tiles[2];
    a.xs = t.xs > 0 ? t.xs : t.h[1] * t.h[2];
    auto ilog2 = [](int v) { int l = 0; while ((1 << l) < v) ++l; return l; };
    a.lw1 = ilog2(t.w[1]); a.lw2 = ilog2(t.w[2]); a.lb1 = ilog2(t.b[1]); a.lb2 = ilog2(t.b[2]);
    a.wpk = wpk; a.bias = bias; a.out = out; a.partials = partials; a.slope = slope;
    return a;
}

template <int R>
static void launch_conv_mfma_r(boa_ctx* ctx, dim3 grid, size_t lds_bytes, const ConvArgs& a) {
    static bool once = (hipFuncSetAttribute((const void*)k_conv_mfma<R>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), true);
    (void)once;
    hipLaunchKernelGGL(k_conv_mfma<R>, grid, dim3(256), lds_bytes, ctx->stream, a);
}

int launch_conv_mfma(boa_ctx* ctx, const ActSrc& s0, const ActSrc& s1, const ConvGeom& g, const ConvTile& t,
                     const __half* wpk, const float* bias, float slope, __half* out, float* partials) {
    BOA_REQUIRE(s0.C % 16 == 0 && s1.C % 16 == 0 && s0.C > 0, "conv: input channels (%d,%d) must be multiples of 16",
                s0.C, s1.C);
    BOA_REQUIRE(g.Cout % 32 == 0, "conv: Cout=%d must be a multiple of 32", g.Cout);
    BOA_REQUIRE((s0.ss == nullptr) == (s0.ss16 == nullptr) && (s1.ss == nullptr) == (s1.ss16 == nullptr),
                "conv: ss and ss16 must be given together");
    ConvArgs a = conv_args(g, t, wpk, bias, slope, out, partials);
    a.src0 = s0.data; a.src1 = s1.data; a.ss0 = s0.ss; a.ss1 = s1.ss; a.C0 = s0.C; a.C1 = s1.C;
    a.ss16_0 = s0.ss16; a.ss16_1 = s1.ss16;
    dim3 grid(t.tiles[0] * t.tiles[1] * t.tiles[2], g.Cout / 32, g.N);
    const int taps = g.k[0] * g.k[1] * g.k[2];
    const double vox = (double)g.N * g.Do * g.Ho * g.Wo;
    const double flops = 2.0 * vox * taps * (s0.C + s1.C) * g.Cout;
    const double bytes = 2.0 * ((double)g.N * g.Di * g.Hi * g.Wi * (s0.C + s1.C) + vox * g.Cout);
    if (t.variant == 2) return launch_conv_ns(ctx, a, t, flops, bytes);
    if (t.variant == 1) return launch_conv_ws(ctx, a, t, flops, bytes);
    ctx->counters[BOA_CNT_CONV_SIMPLE]++;
    KernelTimer tm(ctx, BOA_K_CONV_MFMA, flops, bytes);
    switch (t.R) {
        case 4: launch_conv_mfma_r<4>(ctx, grid, t.lds_bytes, a); break;
        case 2: launch_conv_mfma_r<2>(ctx, grid, t.lds_bytes, a); break;
        case 1: launch_conv_mfma_r<1>(ctx, grid, t.lds_bytes, a); break;
        default:
            boa_set_error("conv: unsupported R=%d", t.R);
            return BOA_EINVAL;
    }
    tm.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}

// split-precision conv (precision 2): k_conv_ws<..., X3>.  Sources / output are fp32 octet planes [N][C/8][voxel][8]; `ss` the
// producer's fp32 (scale, shift) table [N][C][2] or nullptr (raw source).  The kernel sees 2-byte channel units (2 C).
int launch_conv_x3(boa_ctx* ctx, const float* src0, const float* ss0, int C0, const float* src1, const float* ss1, int C1,
                   const ConvGeom& g, const ConvTile& t, const __half* wpk, float wscale, const float* bias, float slope, float* out,
                   float* partials) {
    BOA_REQUIRE(C0 % 8 == 0 && C1 % 8 == 0 && C0 > 0, "conv_x3: input channels (%d,%d) must be multiples of 8", C0, C1);
    BOA_REQUIRE(g.Cout % 32 == 0, "conv_x3: Cout=%d must be a multiple of 32", g.Cout);
    BOA_REQUIRE(t.variant == 1 || t.variant == 2, "conv_x3: tile variant %d", t.variant);
    ConvArgs a = conv_args(g, t, wpk, bias, slope, (__half*)out, partials);
    a.src0 = (const __half*)src0; a.src1 = (const __half*)src1; a.ss0 = ss0; a.ss1 = ss1; a.C0 = 2 * C0; a.C1 = 2 * C1;
    a.ss16_0 = (const unsigned*)ss0; a.ss16_1 = (const unsigned*)ss1;   // read as 16 fp32 words per 8-channel chunk
    a.wscale = wscale; a.winv = 1.0f / wscale;
    const int taps = g.k[0] * g.k[1] * g.k[2];
    const double vox = (double)g.N * g.Do * g.Ho * g.Wo;
    const double flops = 2.0 * vox * taps * (C0 + C1) * g.Cout;
    const double bytes = 4.0 * ((double)g.N * g.Di * g.Hi * g.Wi * (C0 + C1) + vox * g.Cout);
    if (t.variant == 2) return launch_conv_ns(ctx, a, t, flops, bytes, true);
    return launch_conv_ws(ctx, a, t, flops, bytes, true);
}

// ======================================================================================================
// InstanceNorm finalize: deterministic fp64 reduction of the per-block partials
// T = 256: one block per (n, c).  T = 64 (layers with at most 64 slots per (n, c): the 8^3 / 4^3 layers, whose N x 320 blocks of 256 mostly
// idle threads took four rounds of dependent HBM round trips to get through the CUs): one wave per (n, c) -- the same additions in the same
// order (with <= 64 slots only wave 0 of the 256-thread form holds non-zero terms), so the same bits.
template <int T>
__global__ __launch_bounds__(T) void k_norm_finalize(float* __restrict__ partials, int nblk, int C, double count, int clear,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float eps, float* __restrict__ ss,
                                                    unsigned short* __restrict__ ss16) {
    const int c = blockIdx.x, n = blockIdx.y;
    float* ps = partials + (((size_t)n * C + c) * 2 + 0) * nblk;
    float* pq = partials + (((size_t)n * C + c) * 2 + 1) * nblk;
    __shared__ double red[8];
    // (loaded up front: behind the reduction they were one more dependent round trip per block)
    const float gam = gamma[c], bet = beta[c];
    double s = 0.0, q = 0.0;
    // (four slots per thread in flight: the loop was a chain of dependent global round trips -- 16 for the 4 096 slots of a 128^3
    //  layer; the additions keep their order)
    int i = threadIdx.x;
    for (; i + 768 < nblk; i += 1024) {
        const float a0 = ps[i], a1 = ps[i + 256], a2 = ps[i + 512], a3 = ps[i + 768];
        const float b0 = pq[i], b1 = pq[i + 256], b2 = pq[i + 512], b3 = pq[i + 768];
        s += (double)a0; q += (double)b0;
        s += (double)a1; q += (double)b1;
        s += (double)a2; q += (double)b2;
        s += (double)a3; q += (double)b3;
        if (clear) {  // k_conv_ws only writes the slots of waves that worked on (n, c): leave the table zeroed for the next launch
            ps[i] = 0.f; ps[i + 256] = 0.f; ps[i + 512] = 0.f; ps[i + 768] = 0.f;
            pq[i] = 0.f; pq[i + 256] = 0.f; pq[i + 512] = 0.f; pq[i + 768] = 0.f;
        }
    }
    for (; i < nblk; i += 256) {
        s += (double)ps[i];
        q += (double)pq[i];
        if (clear) {
            ps[i] = 0.f;
            pq[i] = 0.f;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        s += __shfl_xor(s, m);
        q += __shfl_xor(q, m);
    }
    if (T > 64) {
        if ((threadIdx.x & 63) == 0) {
            red[(threadIdx.x >> 6) * 2] = s;
            red[(threadIdx.x >> 6) * 2 + 1] = q;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (T > 64) {
            s = (red[0] + red[2]) + (red[4] + red[6]);  // fixed order: deterministic
            q = (red[1] + red[3]) + (red[5] + red[7]);
        }
        double mean = s / count;
        double var = q / count - mean * mean;
        if (var < 0.0) var = 0.0;
        double inv = 1.0 / sqrt(var + (double)eps);
        float scale = (float)((double)gam * inv);
        float shift = (float)((double)bet - mean * (double)gam * inv);
        ss[((size_t)n * C + c) * 2 + 0] = scale;
        ss[((size_t)n * C + c) * 2 + 1] = shift;
        if (ss16) {  // packed fp16 copy for k_conv_ws: per channel pair {s_c, s_c+1, t_c, t_c+1}
            unsigned short* q16 = ss16 + ((size_t)n * C + (c & ~1)) * 2;
            q16[c & 1] = f2us(scale);
            q16[2 + (c & 1)] = f2us(shift);
        }
    }
}

int launch_norm_finalize(boa_ctx* ctx, float* partials, int nblk, int N, int C, double count,
                         const float* gamma, const float* beta, float eps, float* ss_out, unsigned* ss16_out, int clear) {
    KernelTimer tm(ctx, BOA_K_NORM_FINALIZE, 0, (double)N * C * nblk * 8.0);
    if (nblk <= 64)
        hipLaunchKernelGGL(k_norm_finalize<64>, dim3(C, N), dim3(64), 0, ctx->stream, partials, nblk, C, count, clear, gamma,
                           beta, eps, ss_out, (unsigned short*)ss16_out);
    else
        hipLaunchKernelGGL(k_norm_finalize<256>, dim3(C, N), dim3(256), 0, ctx->stream, partials, nblk, C, count, clear, gamma,
                           beta, eps, ss_out, (unsigned short*)ss16_out);
    tm.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}

// ======================================================================================================
// layout helpers
// PyTorch [N][C][vox] fp32 -> the engine's chunk-planar fp16 layout [N][C/16][vox][16]
__global__ void k_nchw_to_ndhwc_f16(const float* __restrict__ in, int C, size_t vox, __half* __restrict__ out) {
    const int n = blockIdx.y;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // over C * vox in the output order
    if (i >= vox * C) return;
    const int j = (int)(i % 16);
    const size_t v = (i / 16) % vox;
    const int c = (int)(i / (16 * vox)) * 16 + j;
    out[(size_t)n * vox * C + i] = __float2half_rn(in[((size_t)n * C + c) * vox + v]);
}

int launch_nchw_to_ndhwc_f16(boa_ctx* ctx, const float* in, int N, int C, size_t vox, __half* out) {
    size_t tot = vox * C;
    hipLaunchKernelGGL(k_nchw_to_ndhwc_f16, dim3((unsigned)((tot + 255) / 256), N), dim3(256), 0, ctx->stream, in, C,
                       vox, out);
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}

__global__ void k_ndhwc_to_nchw_f32(const __half* __restrict__ in, const float* __restrict__ ss, float slope, int C,
                                    size_t vox, float* __restrict__ out) {
    const int n = blockIdx.y;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // over C * vox, voxel fastest
    if (i >= vox * C) return;
    size_t v = i % vox;
    int c = (int)(i / vox);
    float f = __half2float(in[(((size_t)n * (C / 16) + c / 16) * vox + v) * 16 + (c & 15)]);  // chunk-planar
    if (ss) {
        f = __builtin_fmaf(f, ss[((size_t)n * C + c) * 2], ss[((size_t)n * C + c) * 2 + 1]);
        f = f > 0.f ? f : f * slope;
    }
    out[((size_t)n * C + c) * vox + v] = f;
}

int launch_ndhwc_to_nchw_f32(boa_ctx* ctx, const __half* in, const float* ss, float slope, int N, int C, size_t vox,
                             float* out) {
    size_t tot = vox * C;
    hipLaunchKernelGGL(k_ndhwc_to_nchw_f32, dim3((unsigned)((tot + 255) / 256), N), dim3(256), 0, ctx->stream, in, ss,
                       slope, C, vox, out);
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}
