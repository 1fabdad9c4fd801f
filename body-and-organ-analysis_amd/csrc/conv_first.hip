// First conv of the network, reading its tiles out of the resident fp32 volume: k_conv_first_mfma on the matrix cores (Cin == 1, 3x3x3,
// Cout == 32, patch a multiple of the block tile) and the general fp32 VALU pair k_gather_patches + k_conv_first.
#include <algorithm>

#include "conv.h"

// ======================================================================================================
// first conv: fp32 VALU, tiles gathered from the resident volume
// Stage 1: k_gather_patches copies the N tiles out of the resident volume into a zero-padded dense fp32 buffer
// [N][Cin][PX][PY][PZ] (conv padding + pad_nd_image zeros + tile overhang), so that stage 2 has no bounds logic.
// Stage 2: k_conv_first<K0,K1,K2>: each thread computes FV consecutive voxels along the contiguous axis x 32 output
// channels, so one LDS read of a weight quad feeds 4 * FV FMAs and one input value feeds up to 3 taps x 32
// channels.  Weights live in LDS ([Cin][tap][32] floats, broadcast reads); a block covers FT0 x FT1 x FT2 voxels.
#define FT0 4
#define FT1 4
#define FT2 64
#define FV 4

__global__ __launch_bounds__(256) void k_gather_patches(const float* __restrict__ vol, const int* __restrict__ origins,
                                                        int V0, int V1, int V2, int o0, int o1, int o2, int Cin, int P0,
                                                        int P1, int P2, int pad0, int pad1, int pad2, int PX, int PY, int PZ,
                                                        int flip, float* __restrict__ out) {
    const int n = blockIdx.z, ci = blockIdx.y;
    const unsigned pvol = (unsigned)(PX * PY * PZ);  // (a padded tile is far below 2^31 voxels: 32-bit index divisions)
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pvol) return;
    const unsigned r = i / (unsigned)PZ;
    const int z = (int)(i - r * (unsigned)PZ), x = (int)(r / (unsigned)PY), y = (int)(r - (unsigned)x * (unsigned)PY);
    const int px = x - pad0, py = y - pad1, pz = z - pad2;  // patch coordinates
    float v = 0.f;
    if (px >= 0 && px < P0 && py >= 0 && py < P1 && pz >= 0 && pz < P2) {
        // test-time mirroring (predict_from_raw_data.py:541-557): the network sees torch.flip(tile, axes)
        const int qx = (flip & 1) ? P0 - 1 - px : px, qy = (flip & 2) ? P1 - 1 - py : py, qz = (flip & 4) ? P2 - 1 - pz : pz;
        const int vx = origins[n * 3 + 0] + qx - o0, vy = origins[n * 3 + 1] + qy - o1, vz = origins[n * 3 + 2] + qz - o2;
        if (vx >= 0 && vx < V0 && vy >= 0 && vy < V1 && vz >= 0 && vz < V2)
            v = vol[(size_t)ci * V0 * V1 * V2 + ((size_t)vx * V1 + vy) * V2 + vz];
    }
    out[((size_t)n * Cin + ci) * pvol + i] = v;
}

struct FirstArgs {
    const float* padded;  // [N][Cin][PX][PY][PZ]
    int PX, PY, PZ;
    int N, Cin, P0, P1, P2, Cout;
    const float* w;  // [Cin][taps][Cout]
    const float* bias;
    __half* out;
    float* partials;
    int t0, t1, t2;
    int nblk;  // stride of the partials table (>= number of entries a launch writes)
    float* out32;  // F32OUT: fp32 octet planes [N][Cout/8][voxel][8] (split-precision mode)
};

template <int K0, int K1, int K2, bool F32OUT>
__global__ __launch_bounds__(256) void k_conv_first(FirstArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int cout0 = blockIdx.y * 32;
    int bt = blockIdx.x;
    const int tz = bt % p.t2;
    bt /= p.t2;
    const int ty = bt % p.t1;
    const int tx = bt / p.t1;
    constexpr int h0 = FT0 + K0 - 1, h1 = FT1 + K1 - 1, h2 = FT2 + K2 - 1;
    constexpr int HV = h0 * h1 * h2;
    constexpr int taps = K0 * K1 * K2;
    float* lds_w = (float*)smem;                // [Cin][taps][32]
    float* lds_in = lds_w + p.Cin * taps * 32;  // [Cin][HV]
    float* lds_red = lds_in + ((p.Cin * HV + 3) & ~3);
    for (int i = tid; i < p.Cin * taps * 32; i += 256) lds_w[i] = p.w[(size_t)(i >> 5) * p.Cout + cout0 + (i & 31)];
    {
        // halo tile from the padded buffer: always in bounds, compile-time index arithmetic, 4 loads in flight
        const size_t pvol = (size_t)p.PX * p.PY * p.PZ;
        const float* src = p.padded + (size_t)n * p.Cin * pvol;
        const int total = p.Cin * HV;
        for (int i0 = tid; i0 < total; i0 += 256 * 4) {
            float v[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int i = min(i0 + b * 256, total - 1);
                const int ci = i / HV, r = i % HV;
                const int hz = r % h2, hy = (r / h2) % h1, hx = r / (h2 * h1);
                v[b] = src[(size_t)ci * pvol + ((size_t)(tx * FT0 + hx) * p.PY + (ty * FT1 + hy)) * p.PZ + tz * FT2 + hz];
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) lds_in[min(i0 + b * 256, total - 1)] = v[b];
        }
    }
    __syncthreads();
    const int lzq = tid % (FT2 / FV);
    const int ly = (tid / (FT2 / FV)) % FT1;
    const int lx = tid / ((FT2 / FV) * FT1);
    const int lz = lzq * FV;
    const int ox = tx * FT0 + lx, oy = ty * FT1 + ly, oz = tz * FT2 + lz;
    float acc[FV][32];
#pragma unroll
    for (int c = 0; c < 32; ++c) {
        const float b = p.bias[cout0 + c];
#pragma unroll
        for (int v = 0; v < FV; ++v) acc[v][c] = b;
    }
    // The weight reads are wave-uniform; hipcc would scalarise all 27 x 32 of them (v_readfirstlane into SGPRs,
    // ~2700 SGPR spills, occupancy 1).  A lane-opaque zero keeps them as plain broadcast LDS reads.
    int lane_zero = 0;
    asm volatile("" : "+v"(lane_zero));
    for (int ci = 0; ci < p.Cin; ++ci) {
        for (int dx = 0; dx < K0; ++dx)
            for (int dy = 0; dy < K1; ++dy) {
                const float* row = lds_in + ci * HV + ((lx + dx) * h1 + (ly + dy)) * h2 + lz;
                float xin[FV + K2 - 1];
#pragma unroll
                for (int j = 0; j < FV + K2 - 1; ++j) xin[j] = row[j];
                const float* wrow = lds_w + ((ci * taps) + (dx * K1 + dy) * K2) * 32 + lane_zero;
#pragma unroll
                for (int dz = 0; dz < K2; ++dz) {
#pragma unroll
                    for (int c4 = 0; c4 < 8; ++c4) {
                        const float4 w4 = *(const float4*)(wrow + dz * 32 + c4 * 4);  // broadcast read
#pragma unroll
                        for (int v = 0; v < FV; ++v) {
                            acc[v][c4 * 4 + 0] = __builtin_fmaf(xin[v + dz], w4.x, acc[v][c4 * 4 + 0]);
                            acc[v][c4 * 4 + 1] = __builtin_fmaf(xin[v + dz], w4.y, acc[v][c4 * 4 + 1]);
                            acc[v][c4 * 4 + 2] = __builtin_fmaf(xin[v + dz], w4.z, acc[v][c4 * 4 + 2]);
                            acc[v][c4 * 4 + 3] = __builtin_fmaf(xin[v + dz], w4.w, acc[v][c4 * 4 + 3]);
                        }
                    }
                }
            }
    }
    float s[32], q[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) s[c] = q[c] = 0.f;
#pragma unroll
    for (int v = 0; v < FV; ++v) {
        if (F32OUT && ox < p.P0 && oy < p.P1 && oz + v < p.P2) {
            // split-precision mode: the fp32 sums are stored as they are (statistics of the stored values)
            const size_t pvox = (size_t)p.P0 * p.P1 * p.P2;
            float* op = p.out32 + ((size_t)n * p.Cout + cout0) * pvox + ((((size_t)ox) * p.P1 + oy) * (size_t)p.P2 + (oz + v)) * 8;
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                s[c] += acc[v][c];
                q[c] = __builtin_fmaf(acc[v][c], acc[v][c], q[c]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                *(float4*)(op + (size_t)(j >> 1) * 8 * pvox + 4 * (j & 1)) = make_float4(acc[v][4 * j], acc[v][4 * j + 1], acc[v][4 * j + 2], acc[v][4 * j + 3]);
        } else if (!F32OUT && ox < p.P0 && oy < p.P1 && oz + v < p.P2) {
            const size_t pvox = (size_t)p.P0 * p.P1 * p.P2;
            __half* op = p.out + ((size_t)n * p.Cout + cout0) * pvox + ((((size_t)ox) * p.P1 + oy) * (size_t)p.P2 + (oz + v)) * 16;
            union {
                uint4 u[4];
                __half h[32];
            } pk;
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                __half hv = __float2half_rn(acc[v][c]);
                pk.h[c] = hv;
                float vr = __half2float(hv);
                s[c] += vr;
                q[c] = __builtin_fmaf(vr, vr, q[c]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) *(uint4*)(op + (size_t)(j >> 1) * 16 * pvox + 8 * (j & 1)) = pk.u[j];  // chunk-planar
        }
    }
    // recursive-halving reduction over the wave: after step m a lane keeps half of its channels, summed with its
    // partner's copy; 16 + 8 + ... shuffles per quantity instead of 6 x 32.  Lane l ends up owning channel
    // 16*b0 + 8*b1 + 4*b2 + 2*b3 + b4 (b_i = bit i of the lane id).
    const int lane_ = tid & 63;
#define HALVE_STEP(M, HALF)                                                                  \
    {                                                                                        \
        const bool up = (lane_ & (M)) != 0;                                                  \
        _Pragma("unroll") for (int i = 0; i < (HALF); ++i) {                                 \
            const float ks = up ? s[i + (HALF)] : s[i], ss_ = up ? s[i] : s[i + (HALF)];     \
            const float kq = up ? q[i + (HALF)] : q[i], sq_ = up ? q[i] : q[i + (HALF)];     \
            s[i] = ks + __shfl_xor(ss_, (M));                                                \
            q[i] = kq + __shfl_xor(sq_, (M));                                                \
        }                                                                                    \
    }
    HALVE_STEP(1, 16)
    HALVE_STEP(2, 8)
    HALVE_STEP(4, 4)
    HALVE_STEP(8, 2)
    HALVE_STEP(16, 1)
#undef HALVE_STEP
    s[0] += __shfl_xor(s[0], 32);
    q[0] += __shfl_xor(q[0], 32);
    const int wave = tid >> 6;
    if (lane_ < 32) {
        const int c = ((lane_ & 1) << 4) | ((lane_ & 2) << 2) | (lane_ & 4) | ((lane_ & 8) >> 2) | ((lane_ & 16) >> 4);
        lds_red[(wave * 32 + c) * 2 + 0] = s[0];
        lds_red[(wave * 32 + c) * 2 + 1] = q[0];
    }
    __syncthreads();
    if (tid < 64) {
        int row = tid >> 1, j = tid & 1;
        float v = lds_red[(0 * 32 + row) * 2 + j] + lds_red[(1 * 32 + row) * 2 + j];
        v += lds_red[(2 * 32 + row) * 2 + j];
        v += lds_red[(3 * 32 + row) * 2 + j];
        p.partials[(((size_t)n * p.Cout + cout0 + row) * 2 + j) * p.nblk + blockIdx.x] = v;
    }
}

// ------------------------------------------------------------------------------------------------------
// First conv on the matrix cores (Cin == 1, 3x3x3, Cout == 32): the 27 taps are the K dimension (padded to 32 = two
// v_mfma_f32_32x32x16_f16 steps).  A = weights [cout][k] in registers for the whole kernel, B = im2col fragment gathered
// from an fp16 halo tile in LDS (lane (voxel z, k-half) reads its 8 taps with 2-byte LDS loads), D[cout][voxel] goes
// through the same epilogue as k_conv_ws (bias, fp32 InstanceNorm partial sums, v_permlane32_swap transpose, two 16-byte
// stores per lane).  864 fp32 FMAs per voxel become 2 MFMAs per 32 voxels: the kernel is bound by the 64 B/voxel store.
// Persistent blocks walk block tiles of MF0 x MF1 x 32 voxels; M-tile = 32 consecutive z at fixed (x, y).
#define MF0 4
#define MF1 8
#define MF2 32

struct FirstMfmaArgs {
    int N, P0, P1, P2;
    const float* w;  // [27][32] fp32
    const float* bias;
    __half* out;      // [N][P0][P1][P2][32]
    float* partials;  // [N][32][2][nslots]
    int nslots;
    int t0, t1, t2;  // block tiles per axis
    int vw;          // virtual workgroups per sample
    // fused tile gather: the halo is read straight out of the resident volume -- tile origin, pad_nd_image zeros, conv padding,
    // tile overhang and the test-time flip resolved per element -- instead of from the dense padded copy that k_gather_patches
    // makes for the VALU kernel (one kernel and a 4.3 B / voxel round trip less per batch)
    const float* vol;
    const int* origins;  // [N][3]
    int V0, V1, V2, o0, o1, o2, flip;
    float* out32;        // X3: fp32 octet planes [N][4][voxel][8]
    float wscale, winv;  // X3: power-of-two scale of the split weights
};

// X3 (split-precision mode): the fp32 input is staged as hi / lo fp16 halo tiles, a K step covers 8 taps ([Wh | Wh] x [Xh ; Xl] +
// [Wl | Wl] x [Xh ; Xl], 4 steps = 8 MFMAs per 32 voxels), the epilogue stores fp32 octet planes (128 B per voxel: the kernel
// stays store-bound).
template <bool X3>
__global__ __launch_bounds__(256) void k_conv_first_mfma(FirstMfmaArgs p) {
    constexpr int H0 = MF0 + 2, H1 = MF1 + 2, H2 = MF2 + 2, HV = H0 * H1 * H2;
    __shared__ _Float16 halo[X3 ? 4 : 2][HV + 8];   // [buffer][X3: hi, lo]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    // A fragments: lane (cout = l31, kh) holds k = 8 kh + i (step 0) and 16 + 8 kh + i (step 1); taps >= 27 are zero
    f16x8 a0, a1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k0 = 8 * kh + i, k1 = 16 + 8 * kh + i;
        a0[i] = (_Float16)p.w[k0 * 32 + l31];
        a1[i] = k1 < 27 ? (_Float16)p.w[k1 * 32 + l31] : (_Float16)0.f;
    }
    f16x8 xah[X3 ? 4 : 1], xal[X3 ? 4 : 1];
    if constexpr (X3) {
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = 8 * st + i;
                const float wv = k < 27 ? p.w[k * 32 + l31] * p.wscale : 0.f;
                const _Float16 h = (_Float16)wv;
                xah[st][i] = h;
                xal[st][i] = (_Float16)(wv - (float)h);
            }
    }
    // MFMA column (lane l31) <-> voxel lv of the 32-voxel row: even lanes take voxels 0-15, odd lanes 16-31, so that after the
    // register transpose the lane pair (2m, 2m + 1) can exchange one 16-byte piece and ONE store instruction writes the complete
    // 32-byte records of voxels 0-15 (the next one 16-31): whole 64-byte lines per instruction in this write-bound kernel
    // (column = voxel made every instruction write bytes [0, 16) or [16, 32) of all 32 records)
    const int lv = X3 ? l31 : (l31 >> 1) + ((l31 & 1) << 4);   // (X3: column = voxel, 16-byte stores of a half-wave are 1 KiB contiguous)
    const bool odd = (l31 & 1) != 0;
    // LDS offsets (in halves) of this lane's 16 taps relative to the M-tile's first halo voxel
    int toff[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        int t = (i < 8 ? 8 * kh + i : 16 + 8 * kh + (i - 8));
        t = t < 27 ? t : 26;  // padded taps: any finite value (their weights are zero)
        toff[i] = ((t / 9) * H1 + (t / 3) % 3) * H2 + t % 3 + lv;
    }
    int xoff[X3 ? 32 : 1];   // X3: taps 8 st + i for both k-halves (the k-half selects the hi / lo tile)
    if constexpr (X3) {
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int t = i < 27 ? i : 26;
            xoff[i] = ((t / 9) * H1 + (t / 3) % 3) * H2 + t % 3 + lv;
        }
    }
    float4 bq[4];
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) bq[gq] = *(const float4*)(p.bias + 8 * gq + 4 * kh);
    float st_s[16], st_q[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) st_s[i] = st_q[i] = 0.f;
    int st_n = -1;
    auto flush = [&](int slot) {
        if (st_n < 0) return;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
#pragma unroll
            for (int mm = 1; mm < 32; mm <<= 1) {
                st_s[i] += __shfl_xor(st_s[i], mm);
                st_q[i] += __shfl_xor(st_q[i], mm);
            }
        }
        if (l31 == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = 8 * (i >> 2) + 4 * kh + (i & 3);
                float* pp = p.partials + (((size_t)st_n * 32 + row) * 2) * p.nslots + slot;
                pp[0] = st_s[i];
                pp[p.nslots] = st_q[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) st_s[i] = st_q[i] = 0.f;
    };
    const int nsp = p.t0 * p.t1 * p.t2;
    const size_t ovox = (size_t)p.P0 * p.P1 * p.P2;
    // Tile sequence: the spatial tiles of ONE sample are dealt out to vw = min(nsp, CUs) virtual workgroups (j takes
    // sp = j, j + vw, ...), whose partial sums go to statistics slot 4 j + wave of that sample -- a function of the sample
    // alone, not of the batch it shares the launch with (batch-invariant results, as in k_conv_ws).  Physical workgroup b
    // executes the virtual workgroups b, b + G, ...
    const int vw = p.vw, nvirt = p.N * vw;
    struct Seq {
        int v, n, j, sp;
    };
    auto seq_valid = [&](const Seq& q) { return q.v < nvirt; };
    auto seq_first = [&]() {
        Seq q;
        q.v = (int)blockIdx.x;
        q.n = q.v / vw;
        q.j = q.v - q.n * vw;
        q.sp = q.j;
        return q;
    };
    auto seq_next = [&](Seq q) {
        q.sp += vw;
        if (q.sp >= nsp) {
            q.v += (int)gridDim.x;
            q.n = q.v / vw;
            q.j = q.v - q.n * vw;
            q.sp = q.j;
        }
        return q;
    };
    // halo staging is split in two halves so that the global round trip of the NEXT tile overlaps this tile's compute:
    // fetch() issues the loads into registers, commit() converts and writes them to the other LDS buffer afterwards
    constexpr int NPRE = (HV + 255) / 256;
    float pre[NPRE];
    // this thread's halo voxels (tile independent): packed coordinates x | y << 8 | z << 16 and the voxel's linear offset in the
    // volume relative to the halo origin -- the per-tile gather is then three range tests and one add per element (the first
    // version decomposed the index and rebuilt a 64-bit address per element and tile: ~80 instructions each, as much as the
    // tile's MFMA + epilogue work)
    int hc[NPRE], hrel[NPRE];
#pragma unroll
    for (int j = 0; j < NPRE; ++j) {
        const int i = min(tid + 256 * j, HV - 1);
        const int z = i % H2, r = i / H2, y = r % H1, x = r / H1;
        hc[j] = x | (y << 8) | (z << 16);
        hrel[j] = (x * p.V1 + y) * p.V2 + z;
    }
    auto fetch = [&](const Seq& q) {
        int sp = q.sp;
        const int tz = sp % p.t2;
        sp /= p.t2;
        const int ty = sp % p.t1, tx = sp / p.t1;
        if (p.flip == 0) {
            // halo origin in patch coordinates (conv padding 1) and in the volume; valid halo range per axis: inside the patch
            // (conv / tile padding reads zero) and inside the volume (pad_nd_image zeros)
            const int bx = tx * MF0 - 1, by = ty * MF1 - 1, bz = tz * MF2 - 1;
            const int ox = p.origins[q.n * 3 + 0] - p.o0 + bx, oy = p.origins[q.n * 3 + 1] - p.o1 + by, oz = p.origins[q.n * 3 + 2] - p.o2 + bz;
            const int xl = max(-bx, -ox), xh = min(p.P0 - bx, p.V0 - ox);      // halo x valid iff xl <= x < xh
            const int yl = max(-by, -oy), yh = min(p.P1 - by, p.V1 - oy);
            const int zl = max(-bz, -oz), zh = min(p.P2 - bz, p.V2 - oz);
            const float* base = p.vol + ((ptrdiff_t)ox * p.V1 + oy) * p.V2 + oz;
#pragma unroll
            for (int j = 0; j < NPRE; ++j) {
                const int x = hc[j] & 255, y = (hc[j] >> 8) & 255, z = hc[j] >> 16;
                const bool ok = (unsigned)(x - xl) < (unsigned)max(xh - xl, 0) && (unsigned)(y - yl) < (unsigned)max(yh - yl, 0) &&
                                (unsigned)(z - zl) < (unsigned)max(zh - zl, 0);
                pre[j] = ok ? base[hrel[j]] : 0.f;
            }
            return;
        }
        // patch coordinates of the halo origin (conv padding 1) and the tile's position in the volume
        const int bx = tx * MF0 - 1, by = ty * MF1 - 1, bz = tz * MF2 - 1;
        const int ox = p.origins[q.n * 3 + 0] - p.o0, oy = p.origins[q.n * 3 + 1] - p.o1, oz = p.origins[q.n * 3 + 2] - p.o2;
#pragma unroll
        for (int j = 0; j < NPRE; ++j) {
            const int i = min(tid + 256 * j, HV - 1);
            const int z = i % H2, r = i / H2, y = r % H1, x = r / H1;
            const int px = bx + x, py = by + y, pz = bz + z;
            float v = 0.f;
            if ((unsigned)px < (unsigned)p.P0 && (unsigned)py < (unsigned)p.P1 && (unsigned)pz < (unsigned)p.P2) {
                // test-time mirroring (predict_from_raw_data.py:541-557): the network sees torch.flip(tile, axes)
                const int qx = (p.flip & 1) ? p.P0 - 1 - px : px, qy = (p.flip & 2) ? p.P1 - 1 - py : py,
                          qz = (p.flip & 4) ? p.P2 - 1 - pz : pz;
                const int vx = ox + qx, vy = oy + qy, vz = oz + qz;
                if ((unsigned)vx < (unsigned)p.V0 && (unsigned)vy < (unsigned)p.V1 && (unsigned)vz < (unsigned)p.V2)
                    v = p.vol[((size_t)vx * p.V1 + vy) * p.V2 + vz];
            }
            pre[j] = v;
        }
    };
    auto commit = [&](int buf) {
#pragma unroll
        for (int j = 0; j < NPRE; ++j) {
            const int i = tid + 256 * j;
            if constexpr (X3) {
                if (i < HV) {
                    const _Float16 h = (_Float16)pre[j];
                    halo[2 * buf][i] = h;
                    halo[2 * buf + 1][i] = (_Float16)(pre[j] - (float)h);
                }
            } else {
                if (i < HV) halo[buf][i] = (_Float16)pre[j];
            }
        }
    };
    Seq cur = seq_first();
    if (seq_valid(cur)) {
        fetch(cur);
        commit(0);
    }
    __syncthreads();
    int st_v = -1, slot = 0;
    for (int it = 0; seq_valid(cur); ++it) {
        const int buf = it & 1;
        const Seq nxt = seq_next(cur);
        const bool more = seq_valid(nxt);
        if (more) fetch(nxt);
        const int n = cur.n;
        int sp = cur.sp;
        const int tz = sp % p.t2;
        sp /= p.t2;
        const int ty = sp % p.t1, tx = sp / p.t1;
        if (cur.v != st_v) {
            flush(slot);
            st_v = cur.v;
            st_n = n;
            slot = cur.j * 4 + wave;
        }
        const _Float16* hb = X3 ? halo[2 * buf + kh] : halo[buf];
#pragma unroll 2
        for (int r = 0; r < (MF0 * MF1) / 4; ++r) {
            const int row = wave * ((MF0 * MF1) / 4) + r;  // (x, y) row of the block tile
            const int x = row / MF1, y = row % MF1;
            const _Float16* hr = hb + (x * H1 + y) * H2;
            const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            f32x16 acc;
            if constexpr (X3) {
                acc = zero;
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    f16x8 b;
#pragma unroll
                    for (int i = 0; i < 8; ++i) b[i] = hr[xoff[8 * st + i]];
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(xah[st], b, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(xal[st], b, acc, 0, 0, 0);
                }
            } else {
                f16x8 b0, b1;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    b0[i] = hr[toff[i]];
                    b1[i] = hr[toff[8 + i]];
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, zero, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc, 0, 0, 0);
            }
            float v[16];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                v[gq * 4 + 0] = (X3 ? acc[gq * 4 + 0] * p.winv : acc[gq * 4 + 0]) + bq[gq].x;
                v[gq * 4 + 1] = (X3 ? acc[gq * 4 + 1] * p.winv : acc[gq * 4 + 1]) + bq[gq].y;
                v[gq * 4 + 2] = (X3 ? acc[gq * 4 + 2] * p.winv : acc[gq * 4 + 2]) + bq[gq].z;
                v[gq * 4 + 3] = (X3 ? acc[gq * 4 + 3] * p.winv : acc[gq * 4 + 3]) + bq[gq].w;
            }
            // packed fp32 statistics (v_pk_add_f32 / v_pk_fma_f32: the same operations per entry, two entries per instruction)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                typedef float cf2 __attribute__((ext_vector_type(2)));
                const cf2 vv = cf2{v[2 * i], v[2 * i + 1]};
                cf2 s2 = cf2{st_s[2 * i], st_s[2 * i + 1]}, q2 = cf2{st_q[2 * i], st_q[2 * i + 1]};
                s2 = s2 + vv;
                q2 = __builtin_elementwise_fma(vv, vv, q2);
                st_s[2 * i] = s2.x; st_s[2 * i + 1] = s2.y;
                st_q[2 * i] = q2.x; st_q[2 * i + 1] = q2.y;
            }
            if constexpr (X3) {
                // fp32 octet planes [N][4][voxel][8]: entries 4 gq .. + 3 = couts 8 gq + 4 kh .. + 3 of voxel l31
                float* dst32 = p.out32 + ((size_t)n * 32 * ovox + (((size_t)(tx * MF0 + x) * p.P1 + ty * MF1 + y) * p.P2 + tz * MF2 + l31) * 8) + 4 * kh;
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) *(float4*)(dst32 + (size_t)gq * 8 * ovox) = make_float4(v[4 * gq], v[4 * gq + 1], v[4 * gq + 2], v[4 * gq + 3]);
                continue;
            }
            unsigned w8[8];
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                float lo4[4], hi4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[pr * 4 + e]), __float_as_uint(v[(pr + 2) * 4 + e]), false, false);
                    lo4[e] = __uint_as_float(sw[0]);
                    hi4[e] = __uint_as_float(sw[1]);
                }
                // one v_cvt_pk_f16_f32 (RTNE, same rounding as __float2half_rn) per output word
                typedef float cvf2 __attribute__((ext_vector_type(2)));
                typedef _Float16 cvh2 __attribute__((ext_vector_type(2)));
                auto pk = [](float a, float b) {
                    union {
                        cvh2 v;
                        unsigned u;
                    } c;
                    c.v = __builtin_convertvector(cvf2{a, b}, cvh2);
                    return c.u;
                };
                w8[pr * 4 + 0] = pk(lo4[0], lo4[1]);
                w8[pr * 4 + 1] = pk(lo4[2], lo4[3]);
                w8[pr * 4 + 2] = pk(hi4[0], hi4[1]);
                w8[pr * 4 + 3] = pk(hi4[2], hi4[3]);
            }
            // chunk-planar [N][2][voxel][16]: lane pair (2m, 2m + 1) of plane kh writes voxel m's record, then voxel 16 + m's
            unsigned wa[4], wb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned n0 = (unsigned)__builtin_amdgcn_mov_dpp((int)w8[i], 0xB1, 0xF, 0xF, true);       // neighbour's piece 0
                const unsigned n1 = (unsigned)__builtin_amdgcn_mov_dpp((int)w8[4 + i], 0xB1, 0xF, 0xF, true);   // neighbour's piece 1
                wa[i] = odd ? n1 : w8[i];
                wb[i] = odd ? w8[4 + i] : n0;
            }
            __half* dst = p.out + ((size_t)(n * 2 + kh) * ovox + ((size_t)(tx * MF0 + x) * p.P1 + ty * MF1 + y) * p.P2 + tz * MF2 + (l31 >> 1)) * 16 + (odd ? 8 : 0);
            // (streaming `nt` stores were measured: 0 ... -10 %)
            *(uint4*)dst = make_uint4(wa[0], wa[1], wa[2], wa[3]);
            *(uint4*)(dst + 16 * 16) = make_uint4(wb[0], wb[1], wb[2], wb[3]);
        }
        if (more) commit(buf ^ 1);
        __syncthreads();
        cur = nxt;
    }
    flush(slot);
}

bool first_mfma_ok(int Cin, const int P[3], const int k[3], int Cout) {
    return Cin == 1 && Cout == 32 && k[0] == 3 && k[1] == 3 && k[2] == 3 && P[0] % MF0 == 0 && P[1] % MF1 == 0 && P[2] % MF2 == 0;
}

int conv_first_nblk(const int P[3], int cu_count) {
    return std::max(ceil_div(P[0], FT0) * ceil_div(P[1], FT1) * ceil_div(P[2], FT2), cu_count * 4);
}

// dims of the zero-padded gather buffer for a patch P and kernel k
void conv_first_padded_dims(const int P[3], const int k[3], int out[3]) {
    const int ft[3] = {FT0, FT1, FT2};
    for (int a = 0; a < 3; ++a) out[a] = ceil_div(P[a], ft[a]) * ft[a] + (k[a] - 1);
}

int launch_conv_first(boa_ctx* ctx, const float* volume, const int V[3], const int vol_off[3], const int* dev_origins,
                      int N, int Cin, const int P[3], const int k[3], int Cout, const float* w, const float* bias,
                      float* padded_scratch, __half* out, float* partials, int* nblk_out, int flip_mask, float* out32) {
    BOA_REQUIRE(Cout % 32 == 0, "first conv: Cout=%d must be a multiple of 32", Cout);
    BOA_REQUIRE(Cin >= 1 && Cin <= 4, "first conv: Cin=%d unsupported (1..4)", Cin);
    const bool k333 = k[0] == 3 && k[1] == 3 && k[2] == 3, k133 = k[0] == 1 && k[1] == 3 && k[2] == 3;
    BOA_REQUIRE(k333 || k133, "first conv: kernel %dx%dx%d not instantiated", k[0], k[1], k[2]);
    BOA_REQUIRE(volume && dev_origins, "first conv: needs the resident volume and the tile origins");
    int PD[3];
    conv_first_padded_dims(P, k, PD);
    const size_t pvol = (size_t)PD[0] * PD[1] * PD[2];
    const double vox = (double)N * P[0] * P[1] * P[2];
    KernelTimer tm(ctx, BOA_K_CONV_FIRST, 2.0 * vox * k[0] * k[1] * k[2] * Cin * Cout, vox * (4.0 * Cin + 2.0 * Cout));
    const int nblk_tab = conv_first_nblk(P, ctx->cu_count);
    if (nblk_out) *nblk_out = nblk_tab;
    if (first_mfma_ok(Cin, P, k, Cout)) {
        FirstMfmaArgs m;
        m.out32 = out32;
        m.wscale = X3_HEAD_WSCALE;   // (first-conv weights are O(0.1 .. 1) like the head's: one fixed power of two)
        m.winv = 1.0f / X3_HEAD_WSCALE;
        m.vol = volume; m.origins = dev_origins; m.flip = flip_mask;
        m.V0 = V[0]; m.V1 = V[1]; m.V2 = V[2];
        m.o0 = vol_off ? vol_off[0] : 0; m.o1 = vol_off ? vol_off[1] : 0; m.o2 = vol_off ? vol_off[2] : 0;
        m.N = N; m.P0 = P[0]; m.P1 = P[1]; m.P2 = P[2];
        m.w = w; m.bias = bias; m.out = out; m.partials = partials; m.nslots = nblk_tab;
        m.t0 = P[0] / MF0; m.t1 = P[1] / MF1; m.t2 = P[2] / MF2;
        m.vw = std::min(m.t0 * m.t1 * m.t2, ctx->cu_count);
        // (physical workgroup b runs the virtual workgroups b, b + G, ...: any G gives the same results; more than one workgroup
        //  per CU hides the halo gather's and the stores' latency -- the kernel is a 3.4 GB write per 25 tiles)
        const dim3 fgrid((unsigned)std::min<long long>((long long)m.vw * N, (long long)ctx->cu_count * 4));
        if (out32) {
            hipLaunchKernelGGL(k_conv_first_mfma<true>, fgrid, dim3(256), 0, ctx->stream, m);
            ctx->counters[BOA_CNT_X3]++;
        } else {
            hipLaunchKernelGGL(k_conv_first_mfma<false>, fgrid, dim3(256), 0, ctx->stream, m);
            ctx->counters[BOA_CNT_FIRST_MFMA]++;
        }
        tm.stop();
        BOA_HIP_TRY(hipGetLastError());
        return BOA_OK;
    }
    // (the MFMA kernel gathers its halo from the volume itself; the VALU kernel reads a zero-padded copy)
    hipLaunchKernelGGL(k_gather_patches, dim3((unsigned)((pvol + 255) / 256), Cin, N), dim3(256), 0, ctx->stream, volume,
                       dev_origins, V[0], V[1], V[2], vol_off ? vol_off[0] : 0, vol_off ? vol_off[1] : 0,
                       vol_off ? vol_off[2] : 0, Cin, P[0], P[1], P[2], (k[0] - 1) / 2, (k[1] - 1) / 2, (k[2] - 1) / 2, PD[0],
                       PD[1], PD[2], flip_mask, padded_scratch);
    FirstArgs a;
    a.nblk = nblk_tab;
    a.padded = padded_scratch; a.PX = PD[0]; a.PY = PD[1]; a.PZ = PD[2];
    a.N = N; a.Cin = Cin; a.P0 = P[0]; a.P1 = P[1]; a.P2 = P[2]; a.Cout = Cout;
    a.w = w; a.bias = bias; a.out = out; a.partials = partials; a.out32 = out32;
    a.t0 = ceil_div(P[0], FT0); a.t1 = ceil_div(P[1], FT1); a.t2 = ceil_div(P[2], FT2);
    const int nblk = a.t0 * a.t1 * a.t2;
    const int HV = (FT0 + k[0] - 1) * (FT1 + k[1] - 1) * (FT2 + k[2] - 1);
    const size_t lds = ((size_t)Cin * k[0] * k[1] * k[2] * 32 + (((size_t)Cin * HV + 3) & ~(size_t)3)) * 4 + 1024;
    if (out32) {
        if (k333)
            hipLaunchKernelGGL((k_conv_first<3, 3, 3, true>), dim3(nblk, Cout / 32, N), dim3(256), lds, ctx->stream, a);
        else
            hipLaunchKernelGGL((k_conv_first<1, 3, 3, true>), dim3(nblk, Cout / 32, N), dim3(256), lds, ctx->stream, a);
        ctx->counters[BOA_CNT_X3]++;
    } else {
        if (k333)
            hipLaunchKernelGGL((k_conv_first<3, 3, 3, false>), dim3(nblk, Cout / 32, N), dim3(256), lds, ctx->stream, a);
        else
            hipLaunchKernelGGL((k_conv_first<1, 3, 3, false>), dim3(nblk, Cout / 32, N), dim3(256), lds, ctx->stream, a);
        ctx->counters[BOA_CNT_FIRST_VALU]++;
    }
    tm.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}
