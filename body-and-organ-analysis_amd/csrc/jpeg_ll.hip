// JPEG Lossless, Process 14 (ITU T.81 Annex H), one component: the entropy decode and the reconstruction of a batch of
// frames (the compressed slices of a DICOM series, transfer syntaxes 1.2.840.10008.1.2.4.57 / .70) in one launch.
//
// The host (boa_hip/jpeg_lossless.py) parses the markers, removes the byte stuffing (FF 00) and the RSTn markers, and hands
// over per frame the restart intervals ("segments", each a bit stream of its own starting on a byte boundary) and a split of
// every segment into subsequences of a few dozen to a few hundred bytes.  Huffman tables arrive expanded (include/boa_hip.h).
//
// k_lj_parallel: one workgroup per frame, self-synchronising parallel Huffman decoding (Klein & Wiseman 2003; Weissenberger &
// Schmidt, ICPP 2018).  A codeword is the Huffman code of SSSS followed by its SSSS extra bits.
//   A  every subsequence is decoded speculatively from its first bit up to its end: exit position (the first codeword that
//      starts at or after the end) and codeword count;
//   B  every subsequence is decoded again from the exit of its predecessor until no start changes (sweeps over two exit
//      buffers; a thread owns a contiguous block of subsequences and hands exits on within its block in the same sweep, so a
//      correction crosses a whole block per sweep).  The first subsequence of a segment is exact from the start, so every sweep
//      makes at least one more subsequence exact: at most as many sweeps as subsequences, usually two or three (decoding
//      resynchronises within a few codewords).  A subsequence whose
//      predecessor's exit is BAD keeps its state: handing BAD on would travel one subsequence per sweep to the segment's end;
//   C  exclusive scans of the counts (= index of every subsequence's first difference within its segment) and of the BAD exits;
//   D  verified pass: each subsequence decodes from its verified start and writes its differences.  Only here is an invalid
//      code an error (speculation from a wrong start meets invalid codes as a matter of course).  Subsequences behind a BAD
//      exit of their segment are skipped: the first one reports the error, or its failure lies past the segment's last sample;
//   E  reconstruction (T.81 H.1.2, modulo 2^16): predictor 1 = wave scans down column 0 per restart interval, then along
//      the rows; predictor 2 = row scan of each interval's first row, then column sums; predictors 3-7 (6 and 7 are
//      nonlinear in Ra) = anti-diagonal wavefront.  The output is shifted left by Pt at the end.
// k_lj_serial: one lane per frame, the plain sequential T.81 decoder (reference path for the tests and the measurement).
//
// Malformed input never faults: the host entry validates every table offset against the buffers before anything is copied,
// stream bytes are read only below the segment's end (bytes past it read as 1 bits), every loop has a bound, and decoding
// errors are reported per frame in the status array (no trap / assert on the device).
#include <algorithm>

#include "common.h"
#include "jpeg_huff.h"

namespace {

constexpr int LB = JH_LB;                    // bits of the direct lookup (codes of up to LB bits: one LDS read)
constexpr int TW = BOA_LJ_TABLE_WORDS;
constexpr int T_MAXCODE = JH_T_MAXCODE, T_HUFFVAL = JH_T_HUFFVAL;
constexpr unsigned BAD = 0xffffffffu;        // exit of a subsequence whose decode met an invalid code or ran past its segment
constexpr int NT = 256;

__device__ __forceinline__ void set_status(int* st, int code) { atomicCAS(st, 0, code); }

// status of a codeword that could not be decoded at `pos`: a prefix that reaches the segment's end was cut off
__device__ __forceinline__ int lj_fail(int L, unsigned pos, unsigned seg_bits) {
    return (!L && pos + 16u <= seg_bits) ? BOA_LJ_INVALID_CODE : BOA_LJ_TRUNCATED;
}

// One codeword at the head of `win`: returns its length in bits (0 = invalid code) and the difference (T.81 H.1.2.2, table
// H.2: SSSS 16 carries no extra bits and means 32768).  T: table words (LDS or global).
__device__ __forceinline__ int lj_decode(const unsigned* T, unsigned long long win, int& diff) {
    int s;
    const int len = jh_symbol(T, (unsigned)(win >> 32), s);
    if (!len) return 0;
    if (s == 0) {
        diff = 0;
        return len;
    }
    if (s >= 16) {
        diff = 32768;
        return len;
    }
    const unsigned v = (unsigned)((win << len) >> (64 - s));
    diff = v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v;
    return len + s;
}

// decode codewords from `pos` while they start below `stop` (bits): returns the count, `pos` = the exit (BAD on an invalid
// code or a codeword running past the segment end `seg_bits`).  At most stop - pos iterations (a codeword has >= 1 bit).
__device__ __forceinline__ unsigned lj_run(const unsigned* T, BitReader& br, unsigned& pos, unsigned stop, unsigned seg_bits) {
    unsigned n = 0;
    while (pos < stop) {
        int d;
        const int L = lj_decode(T, br.peek(pos), d);
        if (!L || pos + (unsigned)L > seg_bits) {
            pos = BAD;
            return n;
        }
        pos += (unsigned)L;
        ++n;
    }
    return n;
}

// T.81 H.1.2.1: the predictor of sample (r, c); `first` = first row of the image or of a restart interval
__device__ __forceinline__ int lj_predict(int pred, const unsigned short* img, int r, int c, int cols, bool first, int init) {
    if (first) return c == 0 ? init : (int)img[(size_t)r * cols + c - 1];
    if (c == 0) return (int)img[(size_t)(r - 1) * cols];
    const int Ra = img[(size_t)r * cols + c - 1], Rb = img[(size_t)(r - 1) * cols + c], Rc = img[(size_t)(r - 1) * cols + c - 1];
    switch (pred) {
        case 1: return Ra;
        case 2: return Rb;
        case 3: return Rc;
        case 4: return Ra + Rb - Rc;
        case 5: return Ra + ((Rb - Rc) >> 1);
        case 6: return Rb + ((Ra - Rc) >> 1);
        default: return (Ra + Rb) >> 1;
    }
}

struct FrameView {
    const unsigned char* data;
    int len, rows, cols, P, Pt, pred, R, table, seg_first, n_seg, sub_first, n_sub;
    __device__ __forceinline__ FrameView(const unsigned char* d, const int* F) {
        const long long off = (long long)(((unsigned long long)(unsigned)F[BOA_LJ_F_OFF_HI] << 32) | (unsigned)F[BOA_LJ_F_OFF_LO]);
        data = d + off;
        len = F[BOA_LJ_F_LEN];
        rows = F[BOA_LJ_F_ROWS];
        cols = F[BOA_LJ_F_COLS];
        P = F[BOA_LJ_F_P];
        Pt = F[BOA_LJ_F_PT];
        pred = F[BOA_LJ_F_PRED];
        R = F[BOA_LJ_F_RESTART_ROWS] > 0 ? F[BOA_LJ_F_RESTART_ROWS] : F[BOA_LJ_F_ROWS];
        table = F[BOA_LJ_F_TABLE];
        seg_first = F[BOA_LJ_F_SEG_FIRST];
        n_seg = F[BOA_LJ_F_N_SEG];
        sub_first = F[BOA_LJ_F_SUB_FIRST];
        n_sub = F[BOA_LJ_F_N_SUB];
    }
};

// inclusive sum over the 64 lanes
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v, int lane) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const unsigned t = __shfl_up(v, k, 64);
        if (lane >= k) v += t;
    }
    return v;
}

// in-place inclusive prefix sum (mod 2^16) of n elements `stride` apart, plus `carry`, by one wave
__device__ __forceinline__ void wave_scan_inplace(unsigned short* a, int n, size_t stride, unsigned carry, int lane) {
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int c = c0 + lane;
        unsigned v = c < n ? (unsigned)a[c * stride] : 0u;
        v = wave_incl_scan(v, lane) + carry;
        if (c < n) a[c * stride] = (unsigned short)v;
        carry = __shfl(v, 63, 64);
    }
}

// out[i] = sum of get(k) for s0 <= k < i, i in [s0, s1), by the whole workgroup
template <class F>
__device__ __forceinline__ void block_excl_scan(F get, unsigned* out, int s0, int s1, unsigned* wsum, int tid) {
    const int lane = tid & 63, wid = tid >> 6;
    unsigned carry = 0;
    for (int b = s0; b < s1; b += NT) {
        const int i = b + tid;
        const unsigned v = i < s1 ? get(i) : 0u;
        const unsigned incl = wave_incl_scan(v, lane);
        if (lane == 63) wsum[wid] = incl;
        __syncthreads();
        unsigned woff = 0, tot = 0;
        for (int w = 0; w < NT / 64; ++w) {
            woff += w < wid ? wsum[w] : 0u;
            tot += wsum[w];
        }
        if (i < s1) out[i] = carry + woff + incl - v;
        carry += tot;
        __syncthreads();
    }
}

// end (bits) of subsequence i: the next subsequence's start within the same segment, else the segment's end
__device__ __forceinline__ unsigned sub_stop(const int* subs, const int* S, int i, int last) {
    const int seg = subs[2 * i + 1];
    return (i < last && subs[2 * (i + 1) + 1] == seg) ? 8u * (unsigned)subs[2 * (i + 1)] : 8u * (unsigned)S[4 * seg + 1];
}

__global__ __launch_bounds__(NT) void k_lj_parallel(const unsigned char* __restrict__ data, const int* __restrict__ frames,
                                                    const int* __restrict__ segs, const int* __restrict__ subs,
                                                    const unsigned* __restrict__ tables, unsigned short* __restrict__ out,
                                                    int* __restrict__ status, unsigned* __restrict__ scratch, int n_subs) {
    __shared__ unsigned T[TW];
    __shared__ unsigned wsum[NT / 64];
    __shared__ int flag;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const FrameView fv(data, frames + (size_t)f * BOA_LJ_FRAME_WORDS);
    for (int i = tid; i < TW; i += NT) T[i] = tables[(size_t)fv.table * TW + i];
    unsigned* ex0 = scratch;                         // exit positions, two buffers of the Jacobi sweeps
    unsigned* ex1 = scratch + n_subs;
    unsigned* su = scratch + 2 * (size_t)n_subs;     // start each subsequence was last decoded from
    unsigned* cnt = scratch + 3 * (size_t)n_subs;    // codewords from that start up to the subsequence's end
    unsigned* fs = scratch + 4 * (size_t)n_subs;     // exclusive scan of cnt over the frame's subsequences
    const int s0 = fv.sub_first, s1 = fv.sub_first + fv.n_sub, last = s1 - 1;
    __syncthreads();

    // A: speculative decode of every subsequence from its own first bit
    for (int i = s0 + tid; i < s1; i += NT) {
        const int* S = segs + 4 * subs[2 * i + 1];
        BitReader br(fv.data, (unsigned)S[1]);
        unsigned pos = 8u * (unsigned)subs[2 * i];
        su[i] = pos;
        cnt[i] = lj_run(T, br, pos, sub_stop(subs, segs, i, last), 8u * (unsigned)S[1]);
        ex0[i] = pos;
    }
    __syncthreads();

    // B: hand the exits over until no start changes
    const int m = (fv.n_sub + NT - 1) / NT, b0 = s0 + tid * m, b1 = min(b0 + m, s1);
    int p = 0;
    bool converged = false;
    for (int it = 0; it <= fv.n_sub; ++it) {
        if (tid == 0) flag = 0;
        __syncthreads();
        const unsigned* rd = p ? ex1 : ex0;
        unsigned* wr = p ? ex0 : ex1;
        unsigned prev = (b0 > s0 && b0 < s1) ? rd[b0 - 1] : 0u;   // the previous block's exit from the last sweep
        for (int i = b0; i < b1; ++i) {
            const int* S = segs + 4 * subs[2 * i + 1];
            unsigned e = rd[i];
            if (subs[2 * i] != S[0]) {               // not the first subsequence of its segment
                const unsigned s = prev;
                if (s != su[i] && s != BAD) {
                    su[i] = s;
                    BitReader br(fv.data, (unsigned)S[1]);
                    e = s;
                    cnt[i] = lj_run(T, br, e, sub_stop(subs, segs, i, last), 8u * (unsigned)S[1]);
                    flag = 1;
                }
            }
            wr[i] = e;
            prev = e;
        }
        __syncthreads();
        const int changed = flag;
        __syncthreads();
        p ^= 1;
        if (!changed) {
            converged = true;
            break;
        }
    }
    if (!converged) {                                 // (cannot happen: sweep t fixes subsequence t)
        if (tid == 0) set_status(status + f, BOA_LJ_INVALID_CODE);
        return;
    }
    const unsigned* exf = p ? ex1 : ex0;              // the exits of the last sweep

    // C: exclusive scans of the counts and of the BAD exits (into the other exit buffer, free now)
    unsigned* nbad = p ? ex0 : ex1;
    block_excl_scan([&](int i) { return cnt[i]; }, fs, s0, s1, wsum, tid);
    block_excl_scan([&](int i) { return exf[i] == BAD ? 1u : 0u; }, nbad, s0, s1, wsum, tid);

    // D: verified decode, differences written to the frame's output
    unsigned short* img = out + (size_t)f * fv.rows * fv.cols;
    for (int i = s0 + tid; i < s1; i += NT) {
        const int* S = segs + 4 * subs[2 * i + 1];
        const int r0 = S[2];
        const unsigned n = (unsigned)(min(fv.R, fv.rows - r0)) * (unsigned)fv.cols;
        const unsigned j0 = fs[i] - fs[S[3]];
        if (j0 >= n) continue;                        // past the segment's last sample (padding or trailing garbage)
        if (nbad[i] != nbad[S[3]]) continue;          // start unknown: a predecessor failed (the first one reports it)
        const unsigned s = su[i];
        const unsigned seg_bits = 8u * (unsigned)S[1], stop = sub_stop(subs, segs, i, last);
        BitReader br(fv.data, (unsigned)S[1]);
        unsigned short* o = img + (size_t)r0 * fv.cols;
        unsigned pos = s, j = j0;
        int err = 0;
        while (pos < stop && j < n) {
            int d;
            const int L = lj_decode(T, br.peek(pos), d);
            if (!L || pos + (unsigned)L > seg_bits) { err = lj_fail(L, pos, seg_bits); break; }
            o[j++] = (unsigned short)d;
            pos += (unsigned)L;
        }
        if (!err) {
            if (j == n && seg_bits - pos >= 8u) err = BOA_LJ_TRAILING_GARBAGE;   // more than the last byte's padding left
            else if (j < n && stop == seg_bits) err = BOA_LJ_TRUNCATED;            // the segment ended before its last sample
        }
        if (err) set_status(status + f, err);
    }
    __syncthreads();

    // E: reconstruction
    const int rows = fv.rows, cols = fv.cols, R = fv.R, n_int = fv.n_seg;
    const int init = 1 << (fv.P - fv.Pt - 1);
    if (fv.pred <= 2) {
        for (int q = wid; q < n_int; q += NT / 64)    // column 0: Rb, from 2^(P-Pt-1) at the interval's first sample
            wave_scan_inplace(img + (size_t)q * R * cols, min(R, rows - q * R), cols, (unsigned)init, lane);
        __syncthreads();
        for (int r = wid; r < rows; r += NT / 64)     // Ra along the row: every row (predictor 1), the interval's first (2)
            if (fv.pred == 1 || r % R == 0) wave_scan_inplace(img + (size_t)r * cols, cols, 1, 0u, lane);
        __syncthreads();
        if (fv.pred == 2 && cols > 1) {               // Rb down the columns below the interval's first row
            for (int t = tid; t < n_int * (cols - 1); t += NT) {
                const int q = t / (cols - 1), c = 1 + t % (cols - 1);
                unsigned a = img[(size_t)q * R * cols + c];
                for (int r = q * R + 1, r1 = min(q * R + R, rows); r < r1; ++r) {
                    a += img[(size_t)r * cols + c];
                    img[(size_t)r * cols + c] = (unsigned short)a;
                }
            }
        }
    } else {
        for (int dg = 0; dg < rows + cols - 1; ++dg) {   // anti-diagonal wavefront: (r, c) needs (r, c-1), (r-1, c), (r-1, c-1)
            for (int r = max(0, dg - cols + 1) + tid, r1 = min(rows - 1, dg); r <= r1; r += NT) {
                const int c = dg - r;
                const size_t k = (size_t)r * cols + c;
                img[k] = (unsigned short)(lj_predict(fv.pred, img, r, c, cols, r % R == 0, init) + (int)img[k]);
            }
            __syncthreads();
        }
    }
    if (fv.Pt) {
        __syncthreads();
        for (size_t k = tid; k < (size_t)rows * cols; k += NT) img[k] = (unsigned short)(img[k] << fv.Pt);
    }
}

__global__ __launch_bounds__(64) void k_lj_serial(const unsigned char* __restrict__ data, const int* __restrict__ frames,
                                                  const int* __restrict__ segs, const unsigned* __restrict__ tables,
                                                  unsigned short* __restrict__ out, int* __restrict__ status, int n_frames) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= n_frames) return;
    const FrameView fv(data, frames + (size_t)f * BOA_LJ_FRAME_WORDS);
    const unsigned* T = tables + (size_t)fv.table * TW;
    const int rows = fv.rows, cols = fv.cols;
    const int init = 1 << (fv.P - fv.Pt - 1);
    unsigned short* img = out + (size_t)f * rows * cols;
    int err = 0;
    for (int k = 0; k < fv.n_seg && !err; ++k) {
        const int* S = segs + 4 * (fv.seg_first + k);
        const int r0 = S[2], r1 = min(r0 + fv.R, rows);
        const unsigned seg_bits = 8u * (unsigned)S[1];
        BitReader br(fv.data, (unsigned)S[1]);
        unsigned pos = 8u * (unsigned)S[0];
        for (int r = r0; r < r1 && !err; ++r) {
            for (int c = 0; c < cols; ++c) {
                int d;
                const int L = lj_decode(T, br.peek(pos), d);
                if (!L || pos + (unsigned)L > seg_bits) { err = lj_fail(L, pos, seg_bits); break; }
                pos += (unsigned)L;
                img[(size_t)r * cols + c] = (unsigned short)(lj_predict(fv.pred, img, r, c, cols, r == r0, init) + d);
            }
        }
        if (!err && seg_bits - pos >= 8u) err = BOA_LJ_TRAILING_GARBAGE;
    }
    if (err) set_status(status + f, err);
    if (fv.Pt)
        for (size_t k = 0; k < (size_t)rows * cols; ++k) img[k] = (unsigned short)(img[k] << fv.Pt);
}

}  // namespace

extern "C" int boa_ljpeg_decode(boa_ctx* c, const uint8_t* dev_data, size_t data_bytes, int n_frames, const int* frames,
                                int n_segs, const int* segs, int n_subs, const int* subs, int n_tables, const uint32_t* tables,
                                uint16_t* dev_out, int* host_status, int serial) {
    BOA_REQUIRE(c && dev_data && frames && segs && subs && tables && dev_out && host_status, "boa_ljpeg_decode: NULL argument");
    BOA_REQUIRE((uintptr_t)dev_data % 4 == 0, "boa_ljpeg_decode: dev_data not 4-byte aligned");
    BOA_REQUIRE(n_frames > 0 && n_segs > 0 && n_subs > 0 && n_tables > 0, "boa_ljpeg_decode: empty batch or tables");
    const int rows = frames[BOA_LJ_F_ROWS], cols = frames[BOA_LJ_F_COLS];
    BOA_REQUIRE(rows >= 1 && rows <= 65535 && cols >= 1 && cols <= 65535, "boa_ljpeg_decode: frame size %d x %d", rows, cols);
    // every offset the kernels follow is checked here, on the host, before anything reaches the device
    for (int f = 0; f < n_frames; ++f) {
        const int* F = frames + (size_t)f * BOA_LJ_FRAME_WORDS;
        const unsigned long long off = ((unsigned long long)(unsigned)F[BOA_LJ_F_OFF_HI] << 32) | (unsigned)F[BOA_LJ_F_OFF_LO];
        const long long len = F[BOA_LJ_F_LEN];
        BOA_REQUIRE(off % 4 == 0 && len >= 0 && len < (1 << 28) && off + (((unsigned long long)len + 3) & ~3ull) <= data_bytes,
                    "boa_ljpeg_decode: frame %d: bytes [%llu, +%lld) outside the %zu-byte buffer (or not 4-aligned)", f, off, len, data_bytes);
        BOA_REQUIRE(F[BOA_LJ_F_ROWS] == rows && F[BOA_LJ_F_COLS] == cols, "boa_ljpeg_decode: frame %d: size differs within the batch", f);
        const int P = F[BOA_LJ_F_P], Pt = F[BOA_LJ_F_PT], pred = F[BOA_LJ_F_PRED], Rr = F[BOA_LJ_F_RESTART_ROWS];
        BOA_REQUIRE(P >= 2 && P <= 16 && Pt >= 0 && Pt < P && pred >= 1 && pred <= 7 && Rr >= 0,
                    "boa_ljpeg_decode: frame %d: P %d, Pt %d, predictor %d, restart rows %d", f, P, Pt, pred, Rr);
        BOA_REQUIRE(F[BOA_LJ_F_TABLE] >= 0 && F[BOA_LJ_F_TABLE] < n_tables, "boa_ljpeg_decode: frame %d: table %d", f, F[BOA_LJ_F_TABLE]);
        const int R = Rr > 0 ? std::min(Rr, rows) : rows, n_seg = (rows + R - 1) / R;
        const int sf = F[BOA_LJ_F_SEG_FIRST], bf = F[BOA_LJ_F_SUB_FIRST], nb = F[BOA_LJ_F_N_SUB];
        BOA_REQUIRE(F[BOA_LJ_F_N_SEG] == n_seg && sf >= 0 && sf <= n_segs - n_seg && bf >= 0 && nb >= n_seg && bf <= n_subs - nb,
                    "boa_ljpeg_decode: frame %d: segment / subsequence ranges", f);
        BOA_REQUIRE(Rr == 0 || Rr <= rows, "boa_ljpeg_decode: frame %d: restart interval of %d rows", f, Rr);
        int i = bf;
        for (int k = 0; k < n_seg; ++k) {
            const int* S = segs + 4 * (size_t)(sf + k);
            BOA_REQUIRE(S[0] >= 0 && S[0] <= S[1] && S[1] <= len && S[2] == k * R && S[3] == i,
                        "boa_ljpeg_decode: frame %d segment %d: bytes [%d, %d), first row %d, first subsequence %d", f, k, S[0], S[1], S[2], S[3]);
            BOA_REQUIRE(i < bf + nb && subs[2 * i] == S[0] && subs[2 * i + 1] == sf + k,
                        "boa_ljpeg_decode: frame %d segment %d: first subsequence", f, k);
            for (++i; i < bf + nb && subs[2 * i + 1] == sf + k; ++i)
                BOA_REQUIRE(subs[2 * i] > subs[2 * i - 2] && subs[2 * i] < S[1], "boa_ljpeg_decode: frame %d: subsequence %d start", f, i);
        }
        BOA_REQUIRE(i == bf + nb, "boa_ljpeg_decode: frame %d: subsequences outside its segments", f);
    }
    for (int t = 0; t < n_tables; ++t) {
        const uint32_t* T = tables + (size_t)t * BOA_LJ_TABLE_WORDS;
        for (int li = 0; li < (1 << LB); ++li) {
            const unsigned e = (T[li >> 1] >> ((li & 1) * 16)) & 0xffffu, len = e >> 8, s = e & 0xffu;
            BOA_REQUIRE(e == 0 || (len >= 1 && len <= (unsigned)LB && s <= 16), "boa_ljpeg_decode: table %d: lookup entry %d", t, li);
        }
        for (int l = 0; l < 18; ++l)
            BOA_REQUIRE((int)T[T_MAXCODE + l] >= -1 && (int)T[T_MAXCODE + l] < (1 << std::min(l, 17)), "boa_ljpeg_decode: table %d: maxcode", t);
        for (int v = 0; v < 256; ++v)
            BOA_REQUIRE(((T[T_HUFFVAL + (v >> 2)] >> ((v & 3) * 8)) & 0xffu) <= 16, "boa_ljpeg_decode: table %d: SSSS > 16", t);
    }

    const size_t fb = (size_t)n_frames * BOA_LJ_FRAME_WORDS * 4, sb = (size_t)n_segs * 16, bb = (size_t)n_subs * 8;
    const size_t tb = (size_t)n_tables * BOA_LJ_TABLE_WORDS * 4, stb = (size_t)n_frames * 4, scb = serial ? 0 : (size_t)n_subs * 20;
    unsigned char* blk = nullptr;
    BOA_TRY(boa_malloc(c, fb + sb + bb + tb + stb + scb, (void**)&blk));
    int* d_frames = (int*)blk;
    int* d_segs = (int*)(blk + fb);
    int* d_subs = (int*)(blk + fb + sb);
    unsigned* d_tables = (unsigned*)(blk + fb + sb + bb);
    int* d_status = (int*)(blk + fb + sb + bb + tb);
    unsigned* d_scratch = (unsigned*)(blk + fb + sb + bb + tb + stb);
    hipError_t e = hipMemcpyAsync(d_frames, frames, fb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_segs, segs, sb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_subs, subs, bb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tables, tables, tb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_status, 0, stb, c->stream);
    if (e == hipSuccess) {
        c->prof_break = true;
        KernelTimer t(c, BOA_K_OTHER, 0, (double)data_bytes + (double)n_frames * rows * cols * 2);
        if (serial)
            hipLaunchKernelGGL(k_lj_serial, dim3((n_frames + 63) / 64), dim3(64), 0, c->stream, dev_data, d_frames, d_segs, d_tables,
                               dev_out, d_status, n_frames);
        else
            hipLaunchKernelGGL(k_lj_parallel, dim3(n_frames), dim3(NT), 0, c->stream, dev_data, d_frames, d_segs, d_subs, d_tables,
                               dev_out, d_status, d_scratch, n_subs);
        t.stop();
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host_status, d_status, stb, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    boa_free(c, blk);
    BOA_HIP_TRY(e);
    return BOA_OK;
}
