// Sequential DCT JPEG (ITU T.81 baseline Process 1 and extended Process 2 / 4, Huffman, one component, P = 8 or 12): the
// entropy decode and the reconstruction of a batch of frames (the compressed slices of a DICOM series, transfer syntaxes
// 1.2.840.10008.1.2.4.50 / .51) on the device.
//
// The host (boa_hip/jpeg_dct.py) parses the markers, removes the byte stuffing (FF 00) and the RSTn markers, and hands over per
// frame the restart intervals ("segments", each a bit stream of its own starting on a byte boundary, holding Ri blocks: one MCU
// is one 8 x 8 block here) and a split of every segment into subsequences.  Huffman tables arrive expanded as for jpeg_ll.hip,
// quantisation tables as uint16 [64] in natural order.
//
// k_jd_parallel: one workgroup per frame, the self-synchronising parallel Huffman decode of jpeg_ll.hip (Weissenberger & Schmidt,
// ICPP 2018) with the decoder state widened to (bit position, zig-zag index k): k = 0 means the next codeword is a DC code, and
// a codeword is a Huffman code plus its SSSS extra bits (jpeg_dct_codes.h: jd_step).
//   A  every subsequence is decoded speculatively from its first bit at k = 0 up to its end: exit state and blocks completed;
//   B  every subsequence is decoded again from the exit state of its predecessor until no start changes (both parts of the
//      state must match for a subsequence to count as synchronised); sweeps as in k_lj_parallel;
//   C  exclusive scans of the blocks completed (= the block in progress at every subsequence's start; a block may straddle
//      subsequences) and of the BAD exits;
//   D  verified pass: each subsequence decodes from its verified start and writes the non-zero coefficients, de-zig-zagged, into
//      the zeroed int16 [block][64] workspace, the DC difference in place of the DC.  Only here is a codeword that does not
//      decode an error;
//   E  a prefix sum per restart interval turns the DC differences into DC values (predictor 0 at every interval's start).
// k_jd_serial: one lane per frame, the plain loop of T.81 F.2.2 (reference path for the tests and the measurement).
// k_jd_idct: one thread per block: dequantisation, libjpeg's islow inverse DCT, level shift and range limit (jd_block), and the
// crop of the partial blocks at the right and bottom edges into the uint16 [rows][cols] output.
//
// Malformed input never faults: the host entry validates every table field against the buffers before anything is copied,
// stream bytes are read only below the segment's end (bytes past it read as 1 bits), every loop has a bound, coefficient
// positions are bounded by jd_step (zz <= 63) and block indices by the segment's block count, and decoding errors are reported
// per frame in the status array (no trap / assert on the device).
#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "jpeg_dct_codes.h"

namespace {

constexpr int TW = BOA_LJ_TABLE_WORDS;
constexpr unsigned long long BAD = ~0ull;    // exit of a subsequence whose decode met a codeword that does not decode
constexpr int NT = 256;

// coefficient workspace of one chunk of frames: 1 GiB, or BOA_JDCT_WS_KB KiB (read at every call; small values let a test reach
// the chunking with small frames)
size_t ws_cap() {
    const char* v = getenv("BOA_JDCT_WS_KB");
    const long kb = v ? atol(v) : 0;
    return kb > 0 ? (size_t)kb << 10 : size_t(1) << 30;
}

// The status word of a frame starts as NO_ERROR and keeps the error of the EARLIEST restart interval that failed (interval << 8 |
// code, by atomic minimum), so that both entropy decoders report the same error whatever the order their threads run in; the
// host entry turns the word into the code.
constexpr unsigned NO_ERROR = 0xffffffffu;
__device__ __forceinline__ void set_status(int* st, int interval, int code) {
    atomicMin((unsigned*)st, ((unsigned)interval << 8) | (unsigned)code);
}

__device__ __forceinline__ unsigned long long pack(unsigned pos, int k) { return ((unsigned long long)pos << 6) | (unsigned)k; }

struct FrameView {
    const unsigned char* data;
    int len, P, R, dc, ac, qt, seg_first, n_seg, sub_first, n_sub;
    __device__ __forceinline__ FrameView(const unsigned char* d, const int* F, int n_blocks) {
        const long long off = (long long)(((unsigned long long)(unsigned)F[BOA_JD_F_OFF_HI] << 32) | (unsigned)F[BOA_JD_F_OFF_LO]);
        data = d + off;
        len = F[BOA_JD_F_LEN];
        P = F[BOA_JD_F_P];
        R = F[BOA_JD_F_RESTART] > 0 ? F[BOA_JD_F_RESTART] : n_blocks;
        dc = F[BOA_JD_F_DC_TABLE];
        ac = F[BOA_JD_F_AC_TABLE];
        qt = F[BOA_JD_F_QTABLE];
        seg_first = F[BOA_JD_F_SEG_FIRST];
        n_seg = F[BOA_JD_F_N_SEG];
        sub_first = F[BOA_JD_F_SUB_FIRST];
        n_sub = F[BOA_JD_F_N_SUB];
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

// decode codewords from state (pos, k) while they start below `stop` (bits): returns the blocks completed; the state becomes
// the exit (BAD on a codeword that does not decode).  At most stop - pos iterations (a codeword has >= 1 bit).
__device__ __forceinline__ unsigned jd_run(const unsigned* Tdc, const unsigned* Tac, BitReader& br, unsigned long long& state,
                                           unsigned stop, unsigned seg_bits, int P) {
    unsigned pos = (unsigned)(state >> 6), n = 0;
    int k = (int)(state & 63u);
    while (pos < stop) {
        JdStep s;
        if (jd_step(Tdc, Tac, br.peek(pos), k, P, seg_bits - pos, s)) {
            state = BAD;
            return n;
        }
        pos += (unsigned)s.len;
        k = s.knext;
        n += k == 0;
    }
    state = pack(pos, k);
    return n;
}

__global__ __launch_bounds__(NT) void k_jd_parallel(const unsigned char* __restrict__ data, const int* __restrict__ frames,
                                                    const int* __restrict__ segs, const int* __restrict__ subs,
                                                    const unsigned* __restrict__ tables, short* __restrict__ coef,
                                                    int* __restrict__ status, unsigned long long* __restrict__ ex,
                                                    unsigned* __restrict__ cn, int n_subs, int f0, int n_blocks) {
    __shared__ unsigned Tdc[TW], Tac[TW];
    __shared__ unsigned wsum[NT / 64];
    __shared__ int flag;
    const int f = f0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const FrameView fv(data, frames + (size_t)f * BOA_JD_FRAME_WORDS, n_blocks);
    for (int i = tid; i < TW; i += NT) {
        Tdc[i] = tables[(size_t)fv.dc * TW + i];
        Tac[i] = tables[(size_t)fv.ac * TW + i];
    }
    unsigned long long* ex0 = ex;                         // exit states, two buffers of the Jacobi sweeps
    unsigned long long* ex1 = ex + n_subs;
    unsigned long long* su = ex + 2 * (size_t)n_subs;     // state each subsequence was last decoded from
    unsigned* cnt = cn;                                   // blocks completed from that state up to the subsequence's end
    unsigned* fs = cn + n_subs;                           // exclusive scan of cnt over the frame's subsequences
    unsigned* nbad = cn + 2 * (size_t)n_subs;             // exclusive scan of the BAD exits
    const int s0 = fv.sub_first, s1 = fv.sub_first + fv.n_sub, last = s1 - 1;
    const int P = fv.P;
    __syncthreads();

    // A: speculative decode of every subsequence from its own first bit, as if a block began there
    for (int i = s0 + tid; i < s1; i += NT) {
        const int* S = segs + 4 * subs[2 * i + 1];
        BitReader br(fv.data, (unsigned)S[1]);
        unsigned long long st = pack(8u * (unsigned)subs[2 * i], 0);
        su[i] = st;
        cnt[i] = jd_run(Tdc, Tac, br, st, sub_stop(subs, segs, i, last), 8u * (unsigned)S[1], P);
        ex0[i] = st;
    }
    __syncthreads();

    // B: hand the exit states over until no start changes
    const int m = (fv.n_sub + NT - 1) / NT, b0 = s0 + tid * m, b1 = min(b0 + m, s1);
    int p = 0;
    bool converged = false;
    for (int it = 0; it <= fv.n_sub; ++it) {
        if (tid == 0) flag = 0;
        __syncthreads();
        const unsigned long long* rd = p ? ex1 : ex0;
        unsigned long long* wr = p ? ex0 : ex1;
        unsigned long long prev = (b0 > s0 && b0 < s1) ? rd[b0 - 1] : 0ull;   // the previous block's exit from the last sweep
        for (int i = b0; i < b1; ++i) {
            const int* S = segs + 4 * subs[2 * i + 1];
            unsigned long long e = rd[i];
            if (subs[2 * i] != S[0]) {               // not the first subsequence of its segment
                const unsigned long long s = prev;
                if (s != su[i] && s != BAD) {
                    su[i] = s;
                    BitReader br(fv.data, (unsigned)S[1]);
                    e = s;
                    cnt[i] = jd_run(Tdc, Tac, br, e, sub_stop(subs, segs, i, last), 8u * (unsigned)S[1], P);
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
        if (tid == 0) set_status(status + f, 0, JD_ST_INVALID_CODE);
        return;
    }
    const unsigned long long* exf = p ? ex1 : ex0;    // the exits of the last sweep

    // C: exclusive scans of the counts and of the BAD exits
    block_excl_scan([&](int i) { return cnt[i]; }, fs, s0, s1, wsum, tid);
    block_excl_scan([&](int i) { return exf[i] == BAD ? 1u : 0u; }, nbad, s0, s1, wsum, tid);

    // D: verified decode, coefficients written to the frame's workspace
    short* cf = coef + (size_t)blockIdx.x * n_blocks * 64;
    for (int i = s0 + tid; i < s1; i += NT) {
        const int* S = segs + 4 * subs[2 * i + 1];
        const unsigned blk0 = (unsigned)S[2];
        const unsigned n = (unsigned)min(fv.R, n_blocks - S[2]);
        const unsigned j0 = fs[i] - fs[S[3]];
        if (j0 >= n) continue;                        // past the segment's last block (padding or trailing data)
        if (nbad[i] != nbad[S[3]]) continue;          // start unknown: a predecessor failed (the first one reports it)
        const unsigned seg_bits = 8u * (unsigned)S[1], stop = sub_stop(subs, segs, i, last);
        BitReader br(fv.data, (unsigned)S[1]);
        unsigned pos = (unsigned)(su[i] >> 6), j = j0;
        int k = (int)(su[i] & 63u), err = 0;
        while (pos < stop && j < n) {
            JdStep s;
            err = jd_step(Tdc, Tac, br.peek(pos), k, P, seg_bits - pos, s);
            if (err) break;
            if (s.zz >= 0 && s.val) cf[(size_t)(blk0 + j) * 64 + jd_natural(s.zz)] = (short)s.val;
            pos += (unsigned)s.len;
            k = s.knext;
            j += k == 0;
        }
        if (!err) {
            if (j == n && seg_bits - pos >= 8u) err = JD_ST_TRAILING;              // more than the last byte's padding left
            else if (j < n && stop == seg_bits) err = JD_ST_TRUNCATED;             // the segment ended before its last block
        }
        if (err) set_status(status + f, subs[2 * i + 1] - fv.seg_first, err);
    }
    __syncthreads();

    // E: DC differences -> DC values, modulo 2^16 as the int16 coefficient holds them; one wave per restart interval
    for (int q = wid; q < fv.n_seg; q += NT / 64) {
        const int b0q = q * fv.R, nq = min(fv.R, n_blocks - b0q);
        unsigned carry = 0;
        for (int c0 = 0; c0 < nq; c0 += 64) {
            const int c = c0 + lane;
            short* a = cf + (size_t)(b0q + c) * 64;
            unsigned v = c < nq ? (unsigned)(unsigned short)*a : 0u;
            v = wave_incl_scan(v, lane) + carry;
            if (c < nq) *a = (short)(unsigned short)v;
            carry = __shfl(v, 63, 64);
        }
    }
}

__global__ __launch_bounds__(64) void k_jd_serial(const unsigned char* __restrict__ data, const int* __restrict__ frames,
                                                  const int* __restrict__ segs, const unsigned* __restrict__ tables,
                                                  short* __restrict__ coef, int* __restrict__ status, int f0, int n_chunk,
                                                  int n_blocks) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= n_chunk) return;
    const int f = f0 + g;
    const FrameView fv(data, frames + (size_t)f * BOA_JD_FRAME_WORDS, n_blocks);
    const unsigned* Tdc = tables + (size_t)fv.dc * TW;
    const unsigned* Tac = tables + (size_t)fv.ac * TW;
    short* cf = coef + (size_t)g * n_blocks * 64;
    int err = 0, q = 0;
    for (; q < fv.n_seg; ++q) {
        const int* S = segs + 4 * (fv.seg_first + q);
        const int b0 = S[2], b1 = min(b0 + fv.R, n_blocks);
        const unsigned seg_bits = 8u * (unsigned)S[1];
        BitReader br(fv.data, (unsigned)S[1]);
        unsigned pos = 8u * (unsigned)S[0];
        int pred = 0;
        for (int b = b0; b < b1 && !err; ++b) {
            int k = 0;
            do {                                      // at most 64 codewords: every one but ZRL moves k on, and ZRL by 16
                JdStep s;
                err = pos >= seg_bits ? JD_ST_TRUNCATED : jd_step(Tdc, Tac, br.peek(pos), k, fv.P, seg_bits - pos, s);
                if (err) break;
                if (k == 0) {
                    pred += s.val;
                    cf[(size_t)b * 64] = (short)pred;
                } else if (s.zz >= 0 && s.val) {
                    cf[(size_t)b * 64 + jd_natural(s.zz)] = (short)s.val;
                }
                pos += (unsigned)s.len;
                k = s.knext;
            } while (k);
        }
        if (!err && seg_bits - pos >= 8u) err = JD_ST_TRAILING;
        if (err) break;
    }
    if (err) set_status(status + f, q, err);
}

__global__ __launch_bounds__(NT) void k_jd_idct(const short* __restrict__ coef, const int* __restrict__ frames,
                                                const unsigned short* __restrict__ qtables, unsigned short* __restrict__ out,
                                                int f0, int n_chunk, int rows, int cols, int bw, int n_blocks) {
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t >= (long long)n_chunk * n_blocks) return;
    const int g = (int)(t / n_blocks), b = (int)(t % n_blocks);
    const int* F = frames + (size_t)(f0 + g) * BOA_JD_FRAME_WORDS;
    unsigned short px[64];
    jd_block(coef + (size_t)t * 64, qtables + (size_t)F[BOA_JD_F_QTABLE] * 64, F[BOA_JD_F_P], px);
    const int y0 = (b / bw) * 8, x0 = (b % bw) * 8;
    unsigned short* o = out + (size_t)(f0 + g) * rows * cols;
    for (int y = 0; y < 8 && y0 + y < rows; ++y)
        for (int x = 0; x < 8 && x0 + x < cols; ++x) o[(size_t)(y0 + y) * cols + x0 + x] = px[8 * y + x];
}

}  // namespace

extern "C" int boa_jdct_decode(boa_ctx* c, const uint8_t* dev_data, size_t data_bytes, int n_frames, const int* frames, int rows,
                               int cols, int n_segs, const int* segs, int n_subs, const int* subs, int n_tables,
                               const uint32_t* tables, int n_qtables, const uint16_t* qtables, uint16_t* dev_out,
                               int* host_status, int serial) {
    BOA_REQUIRE(c && dev_data && frames && segs && subs && tables && qtables && dev_out && host_status,
                "boa_jdct_decode: NULL argument");
    BOA_REQUIRE((uintptr_t)dev_data % 4 == 0, "boa_jdct_decode: dev_data not 4-byte aligned");
    BOA_REQUIRE(n_frames > 0 && n_segs > 0 && n_subs > 0 && n_tables > 0 && n_qtables > 0, "boa_jdct_decode: empty batch or tables");
    BOA_REQUIRE(rows >= 1 && rows <= 65535 && cols >= 1 && cols <= 65535, "boa_jdct_decode: frame size %d x %d", rows, cols);
    const int bw = (cols + 7) / 8, bh = (rows + 7) / 8;
    BOA_REQUIRE((long long)bw * bh < (1 << 24), "boa_jdct_decode: %d x %d blocks in a frame", bh, bw);
    const int n_blocks = bw * bh;
    // every offset the kernels follow is checked here, on the host, before anything reaches the device
    for (int f = 0; f < n_frames; ++f) {
        const int* F = frames + (size_t)f * BOA_JD_FRAME_WORDS;
        const unsigned long long off = ((unsigned long long)(unsigned)F[BOA_JD_F_OFF_HI] << 32) | (unsigned)F[BOA_JD_F_OFF_LO];
        const long long len = F[BOA_JD_F_LEN];
        BOA_REQUIRE(off % 4 == 0 && len >= 0 && len < (1 << 28) && off <= data_bytes &&
                        (((unsigned long long)len + 3) & ~3ull) <= data_bytes - off,
                    "boa_jdct_decode: frame %d: bytes [%llu, +%lld) outside the %zu-byte buffer (or not 4-aligned)", f, off, len, data_bytes);
        const int P = F[BOA_JD_F_P], Ri = F[BOA_JD_F_RESTART];
        BOA_REQUIRE((P == 8 || P == 12) && Ri >= 0 && Ri <= 65535, "boa_jdct_decode: frame %d: P %d, restart interval %d", f, P, Ri);
        BOA_REQUIRE(F[BOA_JD_F_DC_TABLE] >= 0 && F[BOA_JD_F_DC_TABLE] < n_tables && F[BOA_JD_F_AC_TABLE] >= 0 &&
                        F[BOA_JD_F_AC_TABLE] < n_tables && F[BOA_JD_F_QTABLE] >= 0 && F[BOA_JD_F_QTABLE] < n_qtables,
                    "boa_jdct_decode: frame %d: tables %d / %d / %d", f, F[BOA_JD_F_DC_TABLE], F[BOA_JD_F_AC_TABLE], F[BOA_JD_F_QTABLE]);
        const int R = Ri > 0 ? Ri : n_blocks, n_seg = (n_blocks + R - 1) / R;
        const int sf = F[BOA_JD_F_SEG_FIRST], bf = F[BOA_JD_F_SUB_FIRST], nb = F[BOA_JD_F_N_SUB];
        BOA_REQUIRE(F[BOA_JD_F_N_SEG] == n_seg && sf >= 0 && sf <= n_segs - n_seg && bf >= 0 && nb >= n_seg && bf <= n_subs - nb,
                    "boa_jdct_decode: frame %d: segment / subsequence ranges", f);
        int i = bf;
        for (int k = 0; k < n_seg; ++k) {
            const int* S = segs + 4 * (size_t)(sf + k);
            BOA_REQUIRE(S[0] >= 0 && S[0] <= S[1] && S[1] <= len && (long long)S[2] == (long long)k * R && S[3] == i,
                        "boa_jdct_decode: frame %d segment %d: bytes [%d, %d), first block %d, first subsequence %d", f, k, S[0], S[1], S[2], S[3]);
            BOA_REQUIRE(i < bf + nb && subs[2 * i] == S[0] && subs[2 * i + 1] == sf + k,
                        "boa_jdct_decode: frame %d segment %d: first subsequence", f, k);
            for (++i; i < bf + nb && subs[2 * i + 1] == sf + k; ++i)
                BOA_REQUIRE(subs[2 * i] > subs[2 * i - 2] && subs[2 * i] < S[1], "boa_jdct_decode: frame %d: subsequence %d start", f, i);
        }
        BOA_REQUIRE(i == bf + nb, "boa_jdct_decode: frame %d: subsequences outside its segments", f);
    }
    for (int t = 0; t < n_tables; ++t) {
        const uint32_t* T = tables + (size_t)t * BOA_LJ_TABLE_WORDS;
        for (int li = 0; li < (1 << JH_LB); ++li) {
            const unsigned e = (T[li >> 1] >> ((li & 1) * 16)) & 0xffffu, len = e >> 8;
            BOA_REQUIRE(e == 0 || (len >= 1 && len <= (unsigned)JH_LB), "boa_jdct_decode: table %d: lookup entry %d", t, li);
        }
        for (int l = 0; l < 18; ++l)
            BOA_REQUIRE((int)T[JH_T_MAXCODE + l] >= -1 && (int)T[JH_T_MAXCODE + l] < (1 << std::min(l, 17)), "boa_jdct_decode: table %d: maxcode", t);
    }

    // frames per chunk: the coefficient workspace (2 B per padded sample) stays below the cap
    const size_t per_frame = (size_t)n_blocks * 128;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_frames, ws_cap() / per_frame));
    const size_t fb = (size_t)n_frames * BOA_JD_FRAME_WORDS * 4, sb = (size_t)n_segs * 16, bb = (size_t)n_subs * 8;
    const size_t tb = (size_t)n_tables * BOA_LJ_TABLE_WORDS * 4, qb = (size_t)n_qtables * 128, stb = (size_t)n_frames * 4;
    const size_t exb = serial ? 0 : (size_t)n_subs * 24, cnb = serial ? 0 : (size_t)n_subs * 12;
    const size_t head = (fb + sb + bb + tb + qb + stb + 7) & ~size_t(7);
    unsigned char* blk = nullptr;
    short* d_coef = nullptr;
    BOA_TRY(boa_malloc(c, head + exb + cnb, (void**)&blk));
    const int rc = boa_malloc(c, (size_t)chunk * per_frame, (void**)&d_coef);
    if (rc != BOA_OK) {
        boa_free(c, blk);
        return rc;
    }
    int* d_frames = (int*)blk;
    int* d_segs = (int*)(blk + fb);
    int* d_subs = (int*)(blk + fb + sb);
    unsigned* d_tables = (unsigned*)(blk + fb + sb + bb);
    unsigned short* d_q = (unsigned short*)(blk + fb + sb + bb + tb);
    int* d_status = (int*)(blk + fb + sb + bb + tb + qb);
    unsigned long long* d_ex = (unsigned long long*)(blk + head);
    unsigned* d_cn = (unsigned*)(blk + head + exb);
    hipError_t e = hipMemcpyAsync(d_frames, frames, fb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_segs, segs, sb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_subs, subs, bb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tables, tables, tb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_q, qtables, qb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_status, 0xff, stb, c->stream);
    for (int f0 = 0; f0 < n_frames && e == hipSuccess; f0 += chunk) {
        const int nc = std::min(chunk, n_frames - f0);
        e = hipMemsetAsync(d_coef, 0, (size_t)nc * per_frame, c->stream);
        if (e != hipSuccess) break;
        c->prof_break = true;
        KernelTimer t(c, BOA_K_OTHER, 0, (double)data_bytes * nc / n_frames + (double)nc * per_frame * 2 + (double)nc * rows * cols * 2);
        if (serial)
            hipLaunchKernelGGL(k_jd_serial, dim3((nc + 63) / 64), dim3(64), 0, c->stream, dev_data, d_frames, d_segs, d_tables, d_coef,
                               d_status, f0, nc, n_blocks);
        else
            hipLaunchKernelGGL(k_jd_parallel, dim3(nc), dim3(NT), 0, c->stream, dev_data, d_frames, d_segs, d_subs, d_tables, d_coef,
                               d_status, d_ex, d_cn, n_subs, f0, n_blocks);
        const long long nthr = (long long)nc * n_blocks;
        hipLaunchKernelGGL(k_jd_idct, dim3((unsigned)((nthr + NT - 1) / NT)), dim3(NT), 0, c->stream, d_coef, d_frames, d_q, dev_out,
                           f0, nc, rows, cols, bw, n_blocks);
        t.stop();
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host_status, d_status, stb, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    boa_free(c, d_coef);
    boa_free(c, blk);
    BOA_HIP_TRY(e);
    for (int f = 0; f < n_frames; ++f) host_status[f] = (unsigned)host_status[f] == NO_ERROR ? BOA_JD_OK : (host_status[f] & 0xff);
    return BOA_OK;
}
