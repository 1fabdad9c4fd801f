// JPEG 2000 with the reversible 5/3 transform (lossless, or stopped early by its layers) or the irreversible 9/7 transform with
// scalar quantisation (ITU T.800, one component, one tile):
// tier-1 and the inverse wavelet transform of a batch of frames (the compressed slices of a DICOM series, transfer syntaxes 1.2.840.10008.1.2.4.90 / .91) in one call.
//
// The host (boa_hip/jpeg2000.py) parses the codestream and runs tier-2, and hands over a flat table of code blocks: frame,
// subband orientation, position and size in the frame's coefficient plane (Mallat layout), number of magnitude bit-planes,
// number of coding passes, and the block's data (its contributions of all layers, one codeword segment: code-block style 0);
// for a 9/7 frame also half the quantisation step of the block's subband.  The frames of a batch may mix both transforms.
//
// k_j2k_t1: one lane per code block, all blocks of a chunk of frames in one launch (T.800 Annexes C and D).  The MQ decoder's
// registers stay in the lane's registers, its 19 context states in LDS (a byte per context and lane).  Each coefficient has a
// 16-bit flag word in a device scratch buffer (significance of the eight neighbours, signs of the four horizontal / vertical
// ones, own significance / visited / refined / sign), so that a context is one load; a coefficient that becomes significant
// updates its neighbours' words.  The words of the blocks are interleaved (word k of the lane's block at k * n_lanes + lane),
// so that lanes stepping through blocks of one size in lockstep touch neighbouring addresses.  Coefficients are written signed
// into the frame's int32 plane as they are decoded.  A block whose passes stop before the last bit-plane (a .91 stream with
// rate- or quality-limited layers) gets one more sweep that moves every significant coefficient to the midpoint of its
// undecoded planes, so that such streams reconstruct exactly as OpenJPEG reconstructs them; complete blocks skip it.
// The host orders the blocks by passes x area, longest first.
// k_j2k_idwt_h / k_j2k_idwt_v: inverse 5/3 lifting (Annex F.3.8, symmetric extension, all origins zero so that every level
// starts at an even coordinate; a length-1 signal passes through) of one level of every frame, rows then columns (2D_SR);
// the last column pass of a frame adds the DC level shift, clamps to the sample range (as OpenJPEG does) and writes the uint16
// output.  k_j2k_store does the same for frames without a decomposition.  Launches: 1 + 2 x (levels) per chunk and transform.
// 9/7 frames (j2k_dwt97.h holds the arithmetic, which is OpenJPEG's, float32 operation by operation, so that the pixels are its
// pixels): k_j2k_t1 ends a block with a sweep that turns every significant coefficient into float(+-(2 m + 2^b_last)) * step / 2,
// whose bits take the coefficient's place in the plane (4 bytes per sample either way: workspace and chunks are the same);
// k_j2k_idwt97_h / k_j2k_idwt97_v follow the step schedule of the 5/3 kernels, each kernel skipping the other transform's frames:
// every thread recomputes the +-4 window of a pair of neighbouring samples (scaling, four lifting steps, whole-sample mirroring),
// which gives each output the operations of the in-place sweeps in their order; the last column pass rounds (ties to even), adds
// the DC level shift, clamps and writes the uint16 output.
//
// Malformed input never faults: the host entry validates every table field against the buffers before anything is copied,
// the MQ decoder reads only inside [block start, block end) and feeds 0xFF past it (C.3.4), every loop is bounded by the
// table, and a block with more passes than its bit-planes allow or magnitudes beyond 30 bits sets the frame's status.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "j2k_dwt97.h"

namespace {

constexpr int NT_T1 = 64;                         // lanes (code blocks) per workgroup of k_j2k_t1
constexpr int NT_DWT = 256;
constexpr size_t WS_CAP = size_t(1) << 30;       // workspace of one chunk of frames: int32 planes + flag words
constexpr int CX_RL = 17, CX_UNI = 18, N_CX = 19;
constexpr unsigned SIG = 1u << 12, VIS = 1u << 13, REF = 1u << 14, NEG = 1u << 15;

// Table C.2, packed: Qe | NMPS << 16 | NLPS << 22 | SWITCH << 28
#define MQ_E(q, n, l, s) ((q) | ((n) << 16) | ((l) << 22) | ((s) << 28))
__constant__ unsigned c_mq[47] = {
    MQ_E(0x5601, 1, 1, 1), MQ_E(0x3401, 2, 6, 0), MQ_E(0x1801, 3, 9, 0), MQ_E(0x0AC1, 4, 12, 0), MQ_E(0x0521, 5, 29, 0),
    MQ_E(0x0221, 38, 33, 0), MQ_E(0x5601, 7, 6, 1), MQ_E(0x5401, 8, 14, 0), MQ_E(0x4801, 9, 14, 0), MQ_E(0x3801, 10, 14, 0),
    MQ_E(0x3001, 11, 17, 0), MQ_E(0x2401, 12, 18, 0), MQ_E(0x1C01, 13, 20, 0), MQ_E(0x1601, 29, 21, 0), MQ_E(0x5601, 15, 14, 1),
    MQ_E(0x5401, 16, 14, 0), MQ_E(0x5101, 17, 15, 0), MQ_E(0x4801, 18, 16, 0), MQ_E(0x3801, 19, 17, 0), MQ_E(0x3401, 20, 18, 0),
    MQ_E(0x3001, 21, 19, 0), MQ_E(0x2801, 22, 19, 0), MQ_E(0x2401, 23, 20, 0), MQ_E(0x2201, 24, 21, 0), MQ_E(0x1C01, 25, 22, 0),
    MQ_E(0x1801, 26, 23, 0), MQ_E(0x1601, 27, 24, 0), MQ_E(0x1401, 28, 25, 0), MQ_E(0x1201, 29, 26, 0), MQ_E(0x1101, 30, 27, 0),
    MQ_E(0x0AC1, 31, 28, 0), MQ_E(0x09C1, 32, 29, 0), MQ_E(0x08A1, 33, 30, 0), MQ_E(0x0521, 34, 31, 0), MQ_E(0x0441, 35, 32, 0),
    MQ_E(0x02A1, 36, 33, 0), MQ_E(0x0221, 37, 34, 0), MQ_E(0x0141, 38, 35, 0), MQ_E(0x0111, 39, 36, 0), MQ_E(0x0085, 40, 37, 0),
    MQ_E(0x0049, 41, 38, 0), MQ_E(0x0025, 42, 39, 0), MQ_E(0x0015, 43, 40, 0), MQ_E(0x0009, 44, 41, 0), MQ_E(0x0005, 45, 42, 0),
    MQ_E(0x0001, 45, 43, 0), MQ_E(0x5601, 46, 46, 0)};
#undef MQ_E

__device__ __forceinline__ long long frame_out(const int* F) {
    return (long long)(((unsigned long long)(unsigned)F[BOA_J2K_F_OUT_HI] << 32) | (unsigned)F[BOA_J2K_F_OUT_LO]);
}

// size of a signal of length n after d halvings (zero origin): ceil(n / 2^d), n < 2^16
__device__ __host__ __forceinline__ int ceil_shift(int n, int d) { return d >= 16 ? 1 : (n + (1 << d) - 1) >> d; }

struct MQDec {
    const unsigned char* d;
    unsigned len, bp, a, c;
    int ct;
    unsigned char* cx;      // this lane's context states in LDS: cx[k * NT_T1], index | mps << 7
    const unsigned* tab;

    __device__ __forceinline__ unsigned byte(unsigned p) const { return p < len ? d[p] : 0xFFu; }
    __device__ __forceinline__ void bytein() {
        if (byte(bp) == 0xFFu) {
            const unsigned b1 = byte(bp + 1);
            if (b1 > 0x8Fu) { c += 0xFF00u; ct = 8; }
            else { ++bp; c += b1 << 9; ct = 7; }
        } else {
            ++bp;
            c += byte(bp) << 8;
            ct = 8;
        }
    }
    __device__ __forceinline__ void init() {
        bp = 0;
        c = byte(0) << 16;
        bytein();
        c <<= 7;
        ct -= 7;
        a = 0x8000u;
    }
    __device__ __forceinline__ int decode(int k) {
        unsigned s = cx[k * NT_T1];
        const unsigned e = tab[s & 63u], qe = e & 0xFFFFu;
        int mps = (int)(s >> 7), d;
        a -= qe;
        if ((c >> 16) < qe) {
            if (a < qe) { d = mps; s = (e >> 16) & 63u; }
            else { d = 1 - mps; if (e >> 28) mps = 1 - mps; s = (e >> 22) & 63u; }
            a = qe;
        } else {
            c -= qe << 16;
            if (a & 0x8000u) return mps;
            if (a < qe) { d = 1 - mps; if (e >> 28) mps = 1 - mps; s = (e >> 22) & 63u; }
            else { d = mps; s = (e >> 16) & 63u; }
        }
        cx[k * NT_T1] = (unsigned char)(s | ((unsigned)mps << 7));
        do {
            if (ct == 0) bytein();
            a <<= 1;
            c <<= 1;
            --ct;
        } while (!(a & 0x8000u));
        return d;
    }
};

// Table D.1: zero-coding context of the neighbour-significance bits (NW N NE W E SW S SE = bits 0-7)
__device__ __forceinline__ int zc_ctx(unsigned nb, int orient) {
    int h = ((nb >> 3) & 1) + ((nb >> 4) & 1), v = ((nb >> 1) & 1) + ((nb >> 6) & 1);
    const int dg = (nb & 1) + ((nb >> 2) & 1) + ((nb >> 5) & 1) + ((nb >> 7) & 1);
    if (orient == 1) { const int t = h; h = v; v = t; }
    if (orient == 3) {
        const int hv = h + v;
        if (dg >= 3) return 8;
        if (dg == 2) return hv >= 1 ? 7 : 6;
        if (dg == 1) return hv >= 2 ? 5 : (hv == 1 ? 4 : 3);
        return hv >= 2 ? 2 : hv;
    }
    if (h == 2) return 8;
    if (h == 1) return v >= 1 ? 7 : (dg >= 1 ? 6 : 5);
    if (v == 2) return 4;
    if (v == 1) return 3;
    return dg >= 2 ? 2 : dg;
}

// Tables D.2 / D.3: sign context (9..13) and XOR bit of a flag word (signs of N W E S = bits 8-11)
__device__ __forceinline__ int sc_ctx(unsigned f, int& x) {
    auto contrib = [](unsigned sig, unsigned neg) { return sig ? (neg ? -1 : 1) : 0; };
    int h = contrib((f >> 3) & 1, (f >> 9) & 1) + contrib((f >> 4) & 1, (f >> 10) & 1);
    int v = contrib((f >> 1) & 1, (f >> 8) & 1) + contrib((f >> 6) & 1, (f >> 11) & 1);
    h = h < -1 ? -1 : (h > 1 ? 1 : h);
    v = v < -1 ? -1 : (v > 1 ? 1 : v);
    x = 0;
    if (h < 0) { h = 1; v = -v; x = 1; }
    else if (h == 0 && v < 0) { v = 1; x = 1; }
    return h == 0 ? 9 + v : 12 + v;      // (0,0) 9, (0,1) 10, (1,1) 13, (1,0) 12, (1,-1) 11
}

__global__ void __launch_bounds__(NT_T1) k_j2k_t1(const unsigned char* __restrict__ data, const int* __restrict__ frames,
                                                 const int* __restrict__ blocks, const int* __restrict__ perm, int n_blk,
                                                 long long base, int* __restrict__ plane, unsigned short* __restrict__ flags,
                                                 int* __restrict__ status) {
    __shared__ unsigned s_mq[47];
    __shared__ unsigned char s_cx[N_CX * NT_T1];
    for (int i = threadIdx.x; i < 47; i += NT_T1) s_mq[i] = c_mq[i];
    __syncthreads();
    const int lane = blockIdx.x * NT_T1 + threadIdx.x;
    if (lane >= n_blk) return;
    const int* B = blocks + (size_t)perm[lane] * BOA_J2K_BLOCK_WORDS;
    const int f = B[BOA_J2K_B_FRAME], orient = B[BOA_J2K_B_ORIENT], w = B[BOA_J2K_B_W], h = B[BOA_J2K_B_H];
    const int nbp = B[BOA_J2K_B_NUMBPS], passes = B[BOA_J2K_B_PASSES];
    if (passes == 0) return;
    if (nbp < 1 || nbp > 30 || passes > 3 * nbp - 2) {
        atomicCAS(status + f, 0, BOA_J2K_INVALID);
        return;
    }
    const int* F = frames + (size_t)f * BOA_J2K_FRAME_WORDS;
    const int cols = F[BOA_J2K_F_COLS];
    int* V = plane + (frame_out(F) - base) + (size_t)B[BOA_J2K_B_Y0] * cols + B[BOA_J2K_B_X0];
    const unsigned long long off = ((unsigned long long)(unsigned)B[BOA_J2K_B_OFF_HI] << 32) | (unsigned)B[BOA_J2K_B_OFF_LO];
    unsigned char* cx = s_cx + threadIdx.x;
    for (int k = 0; k < N_CX; ++k) cx[k * NT_T1] = 0;
    cx[0] = 4;
    cx[CX_RL * NT_T1] = 3;
    cx[CX_UNI * NT_T1] = 46;
    MQDec mq{data + off, (unsigned)B[BOA_J2K_B_LEN], 0, 0, 0, 0, cx, s_mq};
    mq.init();
    const size_t S = (size_t)n_blk;                   // interleave stride of the flag words
    unsigned short* Fl = flags + lane;
    const int W2 = w + 2;
    auto fl = [&](int i) -> unsigned short& { return Fl[(size_t)i * S]; };
    auto set_sig = [&](int i, int neg) {
        fl(i) |= (unsigned short)(SIG | (neg ? NEG : 0u));
        fl(i - W2 - 1) |= 1u << 7;
        fl(i - W2) |= (unsigned short)((1u << 6) | (neg ? 1u << 11 : 0u));
        fl(i - W2 + 1) |= 1u << 5;
        fl(i - 1) |= (unsigned short)((1u << 4) | (neg ? 1u << 10 : 0u));
        fl(i + 1) |= (unsigned short)((1u << 3) | (neg ? 1u << 9 : 0u));
        fl(i + W2 - 1) |= 1u << 2;
        fl(i + W2) |= (unsigned short)((1u << 1) | (neg ? 1u << 8 : 0u));
        fl(i + W2 + 1) |= 1u;
    };
    auto sign = [&](int i) {
        int x;
        const int k = sc_ctx(fl(i), x);
        return mq.decode(k) ^ x;
    };
    for (int p = 0; p < passes; ++p) {
        const int kind = p == 0 ? 2 : (p - 1) % 3;    // 0 significance propagation, 1 magnitude refinement, 2 cleanup
        const int bit = 1 << (nbp - 1 - (p + 2) / 3);
        for (int y0 = 0; y0 < h; y0 += 4) {
            const int y1 = min(y0 + 4, h);
            for (int x = 0; x < w; ++x) {
                int y = y0;
                if (kind == 2 && y1 - y0 == 4) {
                    const int i0 = (y0 + 1) * W2 + x + 1;
                    const unsigned any = fl(i0) | fl(i0 + W2) | fl(i0 + 2 * W2) | fl(i0 + 3 * W2);
                    if (!(any & (SIG | VIS | 0xFFu))) {
                        if (!mq.decode(CX_RL)) continue;
                        int r = mq.decode(CX_UNI) << 1;
                        r |= mq.decode(CX_UNI);
                        const int i = i0 + r * W2;
                        const int neg = sign(i);
                        set_sig(i, neg);
                        V[(size_t)(y0 + r) * cols + x] = neg ? -bit : bit;
                        y = y0 + r + 1;
                    }
                }
                for (; y < y1; ++y) {
                    const int i = (y + 1) * W2 + x + 1;
                    const unsigned f0 = fl(i);
                    int* v = V + (size_t)y * cols + x;
                    if (kind == 0) {
                        if (!(f0 & SIG) && (f0 & 0xFFu)) {
                            if (mq.decode(zc_ctx(f0 & 0xFFu, orient))) {
                                const int neg = sign(i);
                                set_sig(i, neg);
                                *v = neg ? -bit : bit;
                            }
                            fl(i) |= (unsigned short)VIS;
                        }
                    } else if (kind == 1) {
                        if ((f0 & SIG) && !(f0 & VIS)) {
                            if (mq.decode((f0 & REF) ? 16 : ((f0 & 0xFFu) ? 15 : 14))) {
                                const int t = *v;
                                *v = t < 0 ? t - bit : t + bit;
                            }
                            fl(i) = (unsigned short)(f0 | REF);
                        }
                    } else {
                        if (!(f0 & (SIG | VIS))) {
                            if (mq.decode(zc_ctx(f0 & 0xFFu, orient))) {
                                const int neg = sign(i);
                                set_sig(i, neg);
                                *v = neg ? -bit : bit;
                            }
                        }
                        fl(i) &= (unsigned short)~VIS;
                    }
                }
            }
        }
    }
    if (F[BOA_J2K_F_TRANSFORM] == BOA_J2K_T_97) {
        // A block of a 9/7 frame: every significant coefficient becomes float(+-(2 m + 2^b_last)) * step / 2 (j2k_dwt97.h), the
        // bits of the float32 in the plane; b_last by the rule below, 0 throughout a complete block.
        const int pl = passes - 1, kf = pl == 0 ? 2 : (pl - 1) % 3, bf = nbp - 1 - (pl + 2) / 3;
        const float step_half = __int_as_float(B[BOA_J2K_B_STEP]);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                int* v = V + (size_t)y * cols + x;
                const int t = *v;
                if (t != 0) *v = __float_as_int(j2k97_dequant(t, j2k_b_last(t < 0 ? -t : t, kf, bf), step_half));
            }
        return;
    }
    if (passes == 3 * nbp - 2) return;
    // A block that stops early (a rate- or quality-limited layer): as OpenJPEG does, a significant coefficient goes to the
    // midpoint of what its undecoded planes leave open, |v| += 2^(b_last - 1) where b_last >= 1 is the lowest plane at which
    // it was coded.  After a cleanup or refinement pass at plane bf that is bf for every significant coefficient; after a
    // significance pass it is bf for those that pass made significant (bit bf of |v| set) and bf + 1 for the others, which
    // wait for their refinement.  bf + 1 <= nbp - 1, so |v| stays below 2^30.
    const int pl = passes - 1, kf = pl == 0 ? 2 : (pl - 1) % 3, bf = nbp - 1 - (pl + 2) / 3;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int* v = V + (size_t)y * cols + x;
            const int t = *v;
            if (t == 0) continue;
            const int m = t < 0 ? -t : t;
            const int bl = kf == 0 && !(m & (1 << bf)) ? bf + 1 : bf;
            if (bl >= 1) *v = t < 0 ? t - (1 << (bl - 1)) : t + (1 << (bl - 1));
        }
}

__device__ __forceinline__ unsigned short j2k_sample(int v, int P, int sgn) {
    if (sgn) v = max(-(1 << (P - 1)), min((1 << (P - 1)) - 1, v));
    else v = max(0, min((1 << P) - 1, v + (1 << (P - 1))));
    return (unsigned short)(v & 0xFFFF);
}

// the level a frame reconstructs at `step` (frames with fewer levels start later, all finish at step max_levels); 0 = none
__device__ __forceinline__ int frame_level(const int* F, int step, int max_levels) {
    return step - (max_levels - F[BOA_J2K_F_LEVELS]);
}

// rows of resolution r: every row's low half [0, wl) and high half [wl, w_r) of A -> interleaved in B
__global__ void __launch_bounds__(NT_DWT) k_j2k_idwt_h(const int* __restrict__ frames, int f0, long long base, int step,
                                                      int max_levels, const int* __restrict__ A, int* __restrict__ Bp) {
    const int* F = frames + (size_t)(f0 + blockIdx.y) * BOA_J2K_FRAME_WORDS;
    const int r = frame_level(F, step, max_levels);
    if (r < 1 || F[BOA_J2K_F_TRANSFORM] != BOA_J2K_T_53) return;
    const int rows = F[BOA_J2K_F_ROWS], cols = F[BOA_J2K_F_COLS], d = F[BOA_J2K_F_LEVELS] - r;
    const int wr = ceil_shift(cols, d), hr = ceil_shift(rows, d), wl = ceil_shift(cols, d + 1), nh = wr - wl;
    const int idx = blockIdx.x * NT_DWT + threadIdx.x;
    if (idx >= hr * wl) return;
    const int y = idx / wl, k = idx - y * wl;
    const size_t o = (size_t)(frame_out(F) - base) + (size_t)y * cols;
    const int* row = A + o;
    int* out = Bp + o;
    if (nh == 0) { out[0] = row[0]; return; }
    const int hk = row[wl + min(k, nh - 1)];
    const int xe = row[k] - ((row[wl + max(k - 1, 0)] + hk + 2) >> 2);
    out[2 * k] = xe;
    if (k < nh) {
        const int xe1 = k + 1 < wl ? row[k + 1] - ((hk + row[wl + min(k + 1, nh - 1)] + 2) >> 2) : xe;
        out[2 * k + 1] = hk + ((xe + xe1) >> 1);
    }
}

// columns of resolution r: low rows [0, hl) and high rows [hl, h_r) of B -> interleaved in A, or (the frame's last level)
// the shifted, clamped uint16 samples in out
__global__ void __launch_bounds__(NT_DWT) k_j2k_idwt_v(const int* __restrict__ frames, int f0, long long base, int step,
                                                      int max_levels, const int* __restrict__ Bp, int* __restrict__ A,
                                                      unsigned short* __restrict__ out) {
    const int* F = frames + (size_t)(f0 + blockIdx.y) * BOA_J2K_FRAME_WORDS;
    const int r = frame_level(F, step, max_levels);
    if (r < 1 || F[BOA_J2K_F_TRANSFORM] != BOA_J2K_T_53) return;
    const int rows = F[BOA_J2K_F_ROWS], cols = F[BOA_J2K_F_COLS], L = F[BOA_J2K_F_LEVELS], d = L - r;
    const int wr = ceil_shift(cols, d), hr = ceil_shift(rows, d), hl = ceil_shift(rows, d + 1), nh = hr - hl;
    const int idx = blockIdx.x * NT_DWT + threadIdx.x;
    if (idx >= wr * hl) return;
    const int k = idx / wr, x = idx - k * wr;
    const long long fo = frame_out(F);
    const size_t o = (size_t)(fo - base) + x;
    const int* col = Bp + o;
    auto at = [&](int i) { return col[(size_t)i * cols]; };
    int v0, v1 = 0;
    if (nh == 0) {
        v0 = at(0);
    } else {
        const int hk = at(hl + min(k, nh - 1));
        v0 = at(k) - ((at(hl + max(k - 1, 0)) + hk + 2) >> 2);
        if (k < nh) {
            const int xe1 = k + 1 < hl ? at(k + 1) - ((hk + at(hl + min(k + 1, nh - 1)) + 2) >> 2) : v0;
            v1 = hk + ((v0 + xe1) >> 1);
        }
    }
    const bool last = r == L, two = nh > 0 && k < nh;
    if (last) {
        const int P = F[BOA_J2K_F_P], sg = F[BOA_J2K_F_SIGNED];
        unsigned short* po = out + fo + x;
        po[(size_t)(2 * k) * cols] = j2k_sample(v0, P, sg);
        if (two) po[(size_t)(2 * k + 1) * cols] = j2k_sample(v1, P, sg);
    } else {
        int* pa = A + o;
        pa[(size_t)(2 * k) * cols] = v0;
        if (two) pa[(size_t)(2 * k + 1) * cols] = v1;
    }
}

// The 9/7 frames' row pass of resolution r (j2k_dwt97.h): one thread per pair of neighbouring samples, each from its own window
// of the row's low half [0, wl) and high half [wl, w_r) of A (the float32 coefficients) -> interleaved in B.
__global__ void __launch_bounds__(NT_DWT) k_j2k_idwt97_h(const int* __restrict__ frames, int f0, long long base, int step,
                                                        int max_levels, const float* __restrict__ A, float* __restrict__ Bp) {
    const int* F = frames + (size_t)(f0 + blockIdx.y) * BOA_J2K_FRAME_WORDS;
    const int r = frame_level(F, step, max_levels);
    if (r < 1 || F[BOA_J2K_F_TRANSFORM] != BOA_J2K_T_97) return;
    const int rows = F[BOA_J2K_F_ROWS], cols = F[BOA_J2K_F_COLS], d = F[BOA_J2K_F_LEVELS] - r;
    const int wr = ceil_shift(cols, d), hr = ceil_shift(rows, d), wl = ceil_shift(cols, d + 1);
    const int idx = blockIdx.x * NT_DWT + threadIdx.x;
    if (idx >= hr * wl) return;
    const int y = idx / wl, k = idx - y * wl;
    const size_t o = (size_t)(frame_out(F) - base) + (size_t)y * cols;
    const float* row = A + o;
    float v0, v1;
    j2k97_pair([&](int i) { return row[(i & 1) ? wl + (i >> 1) : (i >> 1)]; }, k, wr, v0, v1);
    Bp[o + 2 * k] = v0;
    if (2 * k + 1 < wr) Bp[o + 2 * k + 1] = v1;
}

// The 9/7 frames' column pass: low rows [0, hl) and high rows [hl, h_r) of B -> interleaved in A, or (the frame's last level)
// the rounded, shifted, clamped uint16 samples in out
__global__ void __launch_bounds__(NT_DWT) k_j2k_idwt97_v(const int* __restrict__ frames, int f0, long long base, int step,
                                                        int max_levels, const float* __restrict__ Bp, float* __restrict__ A,
                                                        unsigned short* __restrict__ out) {
    const int* F = frames + (size_t)(f0 + blockIdx.y) * BOA_J2K_FRAME_WORDS;
    const int r = frame_level(F, step, max_levels);
    if (r < 1 || F[BOA_J2K_F_TRANSFORM] != BOA_J2K_T_97) return;
    const int rows = F[BOA_J2K_F_ROWS], cols = F[BOA_J2K_F_COLS], L = F[BOA_J2K_F_LEVELS], d = L - r;
    const int wr = ceil_shift(cols, d), hr = ceil_shift(rows, d), hl = ceil_shift(rows, d + 1);
    const int idx = blockIdx.x * NT_DWT + threadIdx.x;
    if (idx >= wr * hl) return;
    const int k = idx / wr, x = idx - k * wr;
    const long long fo = frame_out(F);
    const size_t o = (size_t)(fo - base) + x;
    const float* col = Bp + o;
    float v0, v1;
    j2k97_pair([&](int i) { return col[(size_t)((i & 1) ? hl + (i >> 1) : (i >> 1)) * cols]; }, k, hr, v0, v1);
    const bool two = 2 * k + 1 < hr;
    if (r == L) {
        const int P = F[BOA_J2K_F_P], sg = F[BOA_J2K_F_SIGNED];
        unsigned short* po = out + fo + x;
        po[(size_t)(2 * k) * cols] = j2k97_sample(v0, P, sg);
        if (two) po[(size_t)(2 * k + 1) * cols] = j2k97_sample(v1, P, sg);
    } else {
        float* pa = A + o;
        pa[(size_t)(2 * k) * cols] = v0;
        if (two) pa[(size_t)(2 * k + 1) * cols] = v1;
    }
}

// frames without a decomposition level: plane -> shifted, clamped uint16 samples (a 9/7 frame's plane holds float32: rounded first)
__global__ void __launch_bounds__(NT_DWT) k_j2k_store(const int* __restrict__ frames, int f0, long long base,
                                                     const int* __restrict__ A, unsigned short* __restrict__ out) {
    const int* F = frames + (size_t)(f0 + blockIdx.y) * BOA_J2K_FRAME_WORDS;
    if (F[BOA_J2K_F_LEVELS] != 0) return;
    const int n = F[BOA_J2K_F_ROWS] * F[BOA_J2K_F_COLS];
    const int P = F[BOA_J2K_F_P], sg = F[BOA_J2K_F_SIGNED];
    const long long fo = frame_out(F);
    const bool irr = F[BOA_J2K_F_TRANSFORM] == BOA_J2K_T_97;
    for (int i = blockIdx.x * NT_DWT + threadIdx.x; i < n; i += gridDim.x * NT_DWT) {
        const int v = A[fo - base + i];
        out[fo + i] = irr ? j2k97_sample(__int_as_float(v), P, sg) : j2k_sample(v, P, sg);
    }
}

}  // namespace

extern "C" int boa_j2k_decode(boa_ctx* c, const uint8_t* dev_data, size_t data_bytes, int n_frames, const int* frames,
                              int n_blocks, const int* blocks, uint16_t* dev_out, int* host_status) {
    BOA_REQUIRE(c && dev_data && frames && dev_out && host_status && (blocks || n_blocks == 0), "boa_j2k_decode: NULL argument");
    BOA_REQUIRE(n_frames > 0 && n_blocks >= 0, "boa_j2k_decode: %d frames, %d blocks", n_frames, n_blocks);
    // every field the kernels follow is checked here, on the host, before anything reaches the device
    long long out_total = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int* F = frames + (size_t)f * BOA_J2K_FRAME_WORDS;
        const long long fo = (long long)(((unsigned long long)(unsigned)F[BOA_J2K_F_OUT_HI] << 32) | (unsigned)F[BOA_J2K_F_OUT_LO]);
        const int rows = F[BOA_J2K_F_ROWS], cols = F[BOA_J2K_F_COLS], L = F[BOA_J2K_F_LEVELS], P = F[BOA_J2K_F_P];
        BOA_REQUIRE(rows >= 1 && rows <= 65535 && cols >= 1 && cols <= 65535, "boa_j2k_decode: frame %d: size %d x %d", f, rows, cols);
        BOA_REQUIRE(L >= 0 && L <= 32 && P >= 1 && P <= 16 && (F[BOA_J2K_F_SIGNED] & ~1) == 0,
                    "boa_j2k_decode: frame %d: %d levels, precision %d, signed %d", f, L, P, F[BOA_J2K_F_SIGNED]);
        const int T = F[BOA_J2K_F_TRANSFORM];
        BOA_REQUIRE(T == BOA_J2K_T_97 || T == BOA_J2K_T_53, "boa_j2k_decode: frame %d: wavelet transform %d (0 = 9/7, 1 = 5/3)", f, T);
        BOA_REQUIRE(fo == out_total, "boa_j2k_decode: frame %d: output offset %lld, %lld expected (frames packed in order)", f, fo, out_total);
        out_total += (long long)rows * cols;
        const int bf = F[BOA_J2K_F_BLOCK_FIRST], nb = F[BOA_J2K_F_N_BLOCKS];
        BOA_REQUIRE(nb >= 0 && bf >= 0 && bf <= n_blocks - nb && (f == 0 ? bf == 0 : bf == frames[(size_t)(f - 1) * BOA_J2K_FRAME_WORDS + BOA_J2K_F_BLOCK_FIRST]
                                                                                  + frames[(size_t)(f - 1) * BOA_J2K_FRAME_WORDS + BOA_J2K_F_N_BLOCKS]),
                    "boa_j2k_decode: frame %d: blocks [%d, +%d) (blocks grouped by frame, in order)", f, bf, nb);
        for (int b = bf; b < bf + nb; ++b) {
            const int* B = blocks + (size_t)b * BOA_J2K_BLOCK_WORDS;
            const int x0 = B[BOA_J2K_B_X0], y0 = B[BOA_J2K_B_Y0], w = B[BOA_J2K_B_W], h = B[BOA_J2K_B_H];
            const unsigned long long off = ((unsigned long long)(unsigned)B[BOA_J2K_B_OFF_HI] << 32) | (unsigned)B[BOA_J2K_B_OFF_LO];
            const long long len = B[BOA_J2K_B_LEN];
            BOA_REQUIRE(B[BOA_J2K_B_FRAME] == f && B[BOA_J2K_B_ORIENT] >= 0 && B[BOA_J2K_B_ORIENT] <= 3,
                        "boa_j2k_decode: block %d: frame %d, orientation %d", b, B[BOA_J2K_B_FRAME], B[BOA_J2K_B_ORIENT]);
            BOA_REQUIRE(w >= 1 && h >= 1 && w <= 1024 && h <= 1024 && w * h <= 4096 && x0 >= 0 && y0 >= 0 && x0 <= cols - w && y0 <= rows - h,
                        "boa_j2k_decode: block %d: %d x %d at (%d, %d) outside its %d x %d frame", b, w, h, x0, y0, rows, cols);
            BOA_REQUIRE(B[BOA_J2K_B_PASSES] >= 0 && len >= 0 && off + (unsigned long long)len <= data_bytes,
                        "boa_j2k_decode: block %d: %d passes, bytes [%llu, +%lld) outside the %zu-byte buffer", b, B[BOA_J2K_B_PASSES], off, len, data_bytes);
            if (T == BOA_J2K_T_97) {
                float sh;
                memcpy(&sh, B + BOA_J2K_B_STEP, 4);
                BOA_REQUIRE(std::isfinite(sh) && sh > 0.0f, "boa_j2k_decode: block %d: half quantisation step %g (finite, positive)", b, (double)sh);
            }
        }
    }
    BOA_REQUIRE((n_frames == 0 ? 0 : frames[(size_t)(n_frames - 1) * BOA_J2K_FRAME_WORDS + BOA_J2K_F_BLOCK_FIRST]
                 + frames[(size_t)(n_frames - 1) * BOA_J2K_FRAME_WORDS + BOA_J2K_F_N_BLOCKS]) == n_blocks,
                "boa_j2k_decode: the frames do not cover the %d blocks", n_blocks);

    // chunks of frames whose planes (A: coefficients, B: the row pass) and flag words fit WS_CAP; in each chunk the blocks are
    // ordered by passes x area, longest first
    struct Chunk { int f0, nf, b0, nb, pad, max_levels; long long base, samples; };
    std::vector<Chunk> chunks;
    std::vector<int> perm(std::max(n_blocks, 1));
    size_t ws_max = 0;
    auto pad_of = [&](int b) {
        const int* B = blocks + (size_t)b * BOA_J2K_BLOCK_WORDS;
        return (B[BOA_J2K_B_W] + 2) * (B[BOA_J2K_B_H] + 2);
    };
    for (int f = 0; f < n_frames;) {
        Chunk k{f, 0, frames[(size_t)f * BOA_J2K_FRAME_WORDS + BOA_J2K_F_BLOCK_FIRST], 0, 1, 0, 0, 0};
        k.base = (long long)(((unsigned long long)(unsigned)frames[(size_t)f * BOA_J2K_FRAME_WORDS + BOA_J2K_F_OUT_HI] << 32)
                             | (unsigned)frames[(size_t)f * BOA_J2K_FRAME_WORDS + BOA_J2K_F_OUT_LO]);
        while (f < n_frames && k.nf < 65535) {
            const int* F = frames + (size_t)f * BOA_J2K_FRAME_WORDS;
            int pad = k.pad;
            for (int b = F[BOA_J2K_F_BLOCK_FIRST]; b < F[BOA_J2K_F_BLOCK_FIRST] + F[BOA_J2K_F_N_BLOCKS]; ++b) pad = std::max(pad, pad_of(b));
            const long long s = k.samples + (long long)F[BOA_J2K_F_ROWS] * F[BOA_J2K_F_COLS];
            const size_t ws = (size_t)s * 8 + (size_t)(k.nb + F[BOA_J2K_F_N_BLOCKS]) * pad * 2;
            if (k.nf > 0 && ws > WS_CAP) break;
            k.samples = s;
            k.pad = pad;
            k.nb += F[BOA_J2K_F_N_BLOCKS];
            k.max_levels = std::max(k.max_levels, F[BOA_J2K_F_LEVELS]);
            ++k.nf;
            ++f;
        }
        ws_max = std::max(ws_max, (size_t)k.samples * 8 + (size_t)k.nb * k.pad * 2);
        for (int i = 0; i < k.nb; ++i) perm[k.b0 + i] = k.b0 + i;
        std::stable_sort(perm.begin() + k.b0, perm.begin() + k.b0 + k.nb, [&](int a, int b) {
            const int* A = blocks + (size_t)a * BOA_J2K_BLOCK_WORDS;
            const int* B = blocks + (size_t)b * BOA_J2K_BLOCK_WORDS;
            return (long long)A[BOA_J2K_B_PASSES] * A[BOA_J2K_B_W] * A[BOA_J2K_B_H] > (long long)B[BOA_J2K_B_PASSES] * B[BOA_J2K_B_W] * B[BOA_J2K_B_H];
        });
        chunks.push_back(k);
    }

    const size_t fb = (size_t)n_frames * BOA_J2K_FRAME_WORDS * 4, bb = (size_t)n_blocks * BOA_J2K_BLOCK_WORDS * 4;
    const size_t pb = perm.size() * 4, stb = (size_t)n_frames * 4;
    const size_t tab_bytes = (fb + bb + pb + stb + 255) & ~size_t(255);
    unsigned char* blk = nullptr;
    BOA_TRY(boa_malloc(c, tab_bytes + ws_max, (void**)&blk));
    int* d_frames = (int*)blk;
    int* d_blocks = (int*)(blk + fb);
    int* d_perm = (int*)(blk + fb + bb);
    int* d_status = (int*)(blk + fb + bb + pb);
    unsigned char* ws = blk + tab_bytes;
    hipError_t e = hipMemcpyAsync(d_frames, frames, fb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && bb) e = hipMemcpyAsync(d_blocks, blocks, bb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_perm, perm.data(), pb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_status, 0, stb, c->stream);
    for (const Chunk& k : chunks) {
        if (e != hipSuccess) break;
        int* A = (int*)ws;
        int* Bp = A + k.samples;
        unsigned short* flags = (unsigned short*)(Bp + k.samples);
        e = hipMemsetAsync(A, 0, (size_t)k.samples * 4, c->stream);
        if (e == hipSuccess && k.nb) e = hipMemsetAsync(flags, 0, (size_t)k.nb * k.pad * 2, c->stream);
        if (e != hipSuccess) break;
        c->prof_break = true;
        KernelTimer t(c, BOA_K_OTHER, 0, (double)data_bytes + (double)k.samples * 18);
        if (k.nb)
            hipLaunchKernelGGL(k_j2k_t1, dim3((k.nb + NT_T1 - 1) / NT_T1), dim3(NT_T1), 0, c->stream, dev_data, d_frames, d_blocks,
                               d_perm + k.b0, k.nb, k.base, A, flags, d_status);
        bool any_flat = false, any[2] = {false, false};       // any[T]: the chunk holds frames of transform T
        for (int f = k.f0; f < k.f0 + k.nf; ++f) {
            any_flat |= frames[(size_t)f * BOA_J2K_FRAME_WORDS + BOA_J2K_F_LEVELS] == 0;
            any[frames[(size_t)f * BOA_J2K_FRAME_WORDS + BOA_J2K_F_TRANSFORM]] = true;
        }
        for (int step = 1; step <= k.max_levels; ++step) {
            long long nh[2] = {1, 1}, nv[2] = {1, 1};   // per transform: the largest row-pass / column-pass work of a frame at this step
            for (int f = k.f0; f < k.f0 + k.nf; ++f) {
                const int* F = frames + (size_t)f * BOA_J2K_FRAME_WORDS;
                const int r = step - (k.max_levels - F[BOA_J2K_F_LEVELS]), T = F[BOA_J2K_F_TRANSFORM];
                if (r < 1) continue;
                const int d = F[BOA_J2K_F_LEVELS] - r;
                nh[T] = std::max(nh[T], (long long)ceil_shift(F[BOA_J2K_F_ROWS], d) * ceil_shift(F[BOA_J2K_F_COLS], d + 1));
                nv[T] = std::max(nv[T], (long long)ceil_shift(F[BOA_J2K_F_COLS], d) * ceil_shift(F[BOA_J2K_F_ROWS], d + 1));
            }
            // both transforms follow one step schedule; a kernel leaves the other transform's frames alone
            if (any[BOA_J2K_T_53]) {
                hipLaunchKernelGGL(k_j2k_idwt_h, dim3((unsigned)((nh[BOA_J2K_T_53] + NT_DWT - 1) / NT_DWT), k.nf), dim3(NT_DWT), 0,
                                   c->stream, d_frames, k.f0, k.base, step, k.max_levels, A, Bp);
                hipLaunchKernelGGL(k_j2k_idwt_v, dim3((unsigned)((nv[BOA_J2K_T_53] + NT_DWT - 1) / NT_DWT), k.nf), dim3(NT_DWT), 0,
                                   c->stream, d_frames, k.f0, k.base, step, k.max_levels, Bp, A, dev_out);
            }
            if (any[BOA_J2K_T_97]) {
                hipLaunchKernelGGL(k_j2k_idwt97_h, dim3((unsigned)((nh[BOA_J2K_T_97] + NT_DWT - 1) / NT_DWT), k.nf), dim3(NT_DWT), 0,
                                   c->stream, d_frames, k.f0, k.base, step, k.max_levels, (const float*)A, (float*)Bp);
                hipLaunchKernelGGL(k_j2k_idwt97_v, dim3((unsigned)((nv[BOA_J2K_T_97] + NT_DWT - 1) / NT_DWT), k.nf), dim3(NT_DWT), 0,
                                   c->stream, d_frames, k.f0, k.base, step, k.max_levels, (const float*)Bp, (float*)A, dev_out);
            }
        }
        if (any_flat)
            hipLaunchKernelGGL(k_j2k_store, dim3(64, k.nf), dim3(NT_DWT), 0, c->stream, d_frames, k.f0, k.base, A, dev_out);
        t.stop();
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host_status, d_status, stb, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    boa_free(c, blk);
    BOA_HIP_TRY(e);
    return BOA_OK;
}
