// JPEG-LS (ITU-T T.87) decoding rules shared by the kernels of jls.hip and the host program tools/jls_codes_host.cpp (which runs
// them under the address and undefined-behaviour sanitizers): the parameter derivation, the stuffed bit stream, the limited
// Golomb code, gradient quantisation, prediction, error mapping, the context update and the run mode.  One scan is one chain:
// jls_row decodes a row through a row policy (where the row above is read, where samples and run fills go), so the one-lane
// kernel, the one-wave kernel and the host program run the same chain.  Every loop is bounded by a constant or by the row.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JLS_HD __host__ __device__
#else
#define JLS_HD
#endif

#define JLS_CONTEXTS 367          // 365 regular (index |81 Q1 + 9 Q2 + Q3|, 0 unused) and the two run-interruption contexts
#define JLS_ST_OK 0
#define JLS_ST_TRUNCATED 1
#define JLS_ST_INVALID 2

struct JlsParams {
    int maxval, near_, t1, t2, t3, reset;             // as the frame header / LSE give them, defaults resolved
    int range, qbpp, bpp, limit, a0, step, wrap;      // derived: step = 2 NEAR + 1, wrap = RANGE * step
};

struct JlsCtx {                  // one context record; a run-interruption context keeps Nn in B
    int A, B, C, N;
};

JLS_HD inline int jls_ceil_log2(unsigned v) {
    int b = 0;
    while (b < 31 && (1u << b) < v) ++b;
    return b;
}

JLS_HD inline int jls_clamp_t(int i, int j, int maxval) { return (i > maxval || i < j) ? j : i; }

// T.87 C.2.4.1.1.1: the default thresholds
JLS_HD inline void jls_default_thresholds(int maxval, int near_, int* t1, int* t2, int* t3) {
    if (maxval >= 128) {
        const int f = ((maxval < 4095 ? maxval : 4095) + 128) >> 8;
        *t1 = jls_clamp_t(f * (3 - 2) + 2 + 3 * near_, near_ + 1, maxval);
        *t2 = jls_clamp_t(f * (7 - 3) + 3 + 5 * near_, *t1, maxval);
        *t3 = jls_clamp_t(f * (21 - 4) + 4 + 7 * near_, *t2, maxval);
    } else {
        const int f = 256 / (maxval + 1);
        const int a = 3 / f + 3 * near_, b = 7 / f + 5 * near_, c = 21 / f + 7 * near_;
        *t1 = jls_clamp_t(a > 2 ? a : 2, near_ + 1, maxval);
        *t2 = jls_clamp_t(b > 3 ? b : 3, *t1, maxval);
        *t3 = jls_clamp_t(c > 4 ? c : 4, *t2, maxval);
    }
}

// T.87 C.2.4.1.1: the ranges of resolved parameters
JLS_HD inline bool jls_params_valid(int maxval, int near_, int t1, int t2, int t3, int reset) {
    if (maxval < 1 || maxval > 65535) return false;
    if (near_ < 0 || near_ > 255 || near_ > maxval / 2) return false;
    if (t1 < near_ + 1 || t1 > maxval || t2 < t1 || t2 > maxval || t3 < t2 || t3 > maxval) return false;
    return reset >= 3 && reset <= (maxval > 255 ? maxval : 255);
}

JLS_HD inline JlsParams jls_derive(int maxval, int near_, int t1, int t2, int t3, int reset) {
    JlsParams p;
    p.maxval = maxval, p.near_ = near_, p.t1 = t1, p.t2 = t2, p.t3 = t3, p.reset = reset;
    p.step = 2 * near_ + 1;
    p.range = (maxval + 2 * near_) / p.step + 1;
    p.qbpp = jls_ceil_log2((unsigned)p.range);
    const int b = jls_ceil_log2((unsigned)maxval + 1u);
    p.bpp = b > 2 ? b : 2;
    p.limit = 2 * (p.bpp + (p.bpp > 8 ? p.bpp : 8));
    const int a = (p.range + 32) >> 6;
    p.a0 = a > 2 ? a : 2;
    p.wrap = p.range * p.step;
    return p;
}

JLS_HD inline JlsCtx jls_ctx_init(const JlsParams& p) { return JlsCtx{p.a0, 0, 0, 1}; }

// the run-length orders J
JLS_HD inline int jls_J(int runindex) {
    // 0 0 0 0 1 1 1 1 2 2 2 2 3 3 3 3 4 4 5 5 6 6 7 7 8 9 10 11 12 13 14 15
    return runindex < 16 ? runindex >> 2 : runindex < 24 ? 4 + ((runindex - 16) >> 1) : runindex - 16;
}

// a value every lane of the wave holds alike, moved to the scalar side (U: the one-wave kernel)
template <bool U>
JLS_HD inline int jls_uni(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (U) return __builtin_amdgcn_readfirstlane(v);
#endif
    return v;
}

JLS_HD inline int jls_clz64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return v ? __clzll((long long)v) : 64;
#else
    return v ? __builtin_clzll(v) : 64;
#endif
}

// ---------------------------------------------------------------------------------------------------- the stuffed bit stream
// The scan's bytes as aligned little-endian words (byte i = bits 8 (i & 3) .. of word i / 4).  After a 0xFF byte the next byte
// carries 7 bits; a byte >= 0x80 there is a marker and ends the stream.  Behind the end zero bits are fed; `real` counts the bits
// of the accumulator that came from the stream, and a read that takes more sets `over`.
// The one-wave kernel (U) keeps a window of 64 words in a register, lane l word l of it, and the window behind it in a second one,
// loaded when the first was entered: a word is then a lane read, and the memory latency is off the chain.  Nothing on the chain may
// branch on the lane: a divergent branch makes the compiler treat what joins behind it as divergent, and the chain leaves the
// scalar side.
struct JlsBits {
    const uint32_t* w;
    uint32_t len, pos;
    uint64_t acc;                // next bit = bit 63
    int n, real;
    bool ff, over;
    uint32_t n_words, win_base, win0, win1;
};

template <bool U>
JLS_HD inline JlsBits jls_bits_open(const uint32_t* words, uint32_t len) {
    JlsBits b{words, len, 0u, 0ull, 0, 0, false, false, (len + 3u) >> 2, 0u, 0u, 0u};
#if defined(__HIP_DEVICE_COMPILE__)
    if (U && b.n_words) {                        // (no lane takes a branch of its own: an index behind the end reads the last word)
        const uint32_t last = b.n_words - 1u, i = threadIdx.x;
        b.win0 = words[i < last ? i : last];
        b.win1 = words[i + 64u < last ? i + 64u : last];
    }
#endif
    return b;
}

// word dw of the stream; the positions advance byte by byte, so a window is left for the one behind it
template <bool U>
JLS_HD inline uint32_t jls_word(JlsBits& b, uint32_t dw) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (U) {
        if (dw - b.win_base >= 64u) {
            b.win_base += 64u;
            b.win0 = b.win1;
            const uint32_t i = b.win_base + 64u + threadIdx.x, last = b.n_words - 1u;
            b.win1 = b.w[i < last ? i : last];
        }
        return (uint32_t)__builtin_amdgcn_readlane((int)b.win0, (int)(dw & 63u));
    }
#endif
    return b.w[dw];
}

// at least 57 bits in the accumulator afterwards
template <bool U>
JLS_HD inline void jls_refill(JlsBits& b) {
    for (int i = 0; i < 10 && b.n <= 56; ++i) {
        if (b.pos < b.len) {
            const uint32_t word = jls_word<U>(b, b.pos >> 2);
            const uint32_t byte = (word >> (8u * (b.pos & 3u))) & 0xFFu;
            if (b.ff && (byte & 0x80u)) {
                b.len = b.pos;                     // a marker
                continue;
            }
            const int width = b.ff ? 7 : 8;
            b.acc |= (uint64_t)byte << (64 - b.n - width);
            b.n += width;
            b.real += width;
            b.ff = byte == 0xFFu;
            ++b.pos;
        } else {
            b.n += 8;
        }
    }
}

JLS_HD inline void jls_skip(JlsBits& b, int k) {          // 0 .. 63 bits, all in the accumulator
    b.acc <<= k;
    b.n -= k;
    b.real -= k;
    if (b.real < 0) {
        b.over = true;
        b.real = 0;
    }
}

JLS_HD inline uint32_t jls_take(JlsBits& b, int k) {      // 0 .. 32 bits, all in the accumulator
    const uint32_t v = k ? (uint32_t)(b.acc >> (64 - k)) : 0u;
    jls_skip(b, k);
    return v;
}

// The limited Golomb code (T.87 A.5.3): up to qmax = glimit - qbpp - 1 zeros and a one, then k bits; qmax zeros escape to qbpp
// bits of the value minus one.  More zeros, or a value above RANGE (no encoder writes one), set *bad.
template <bool U>
JLS_HD inline uint32_t jls_golomb(JlsBits& b, const JlsParams& p, int k, int glimit, int* bad) {
    jls_refill<U>(b);
    const int qmax = glimit - p.qbpp - 1;
    const int z = jls_clz64(b.acc);
    if (z > qmax) {
        if (b.real < qmax + 1) b.over = true;
        *bad = 1;
        return 0u;
    }
    jls_skip(b, z + 1);
    jls_refill<U>(b);
    const uint64_t v = z == qmax ? (uint64_t)jls_take(b, p.qbpp) + 1u : ((uint64_t)z << k) | jls_take(b, k);
    if (v > (uint64_t)p.range) {
        *bad = 1;
        return 0u;
    }
    return (uint32_t)v;
}

// ---------------------------------------------------------------------------------------------------- the sample rules
JLS_HD inline int jls_quantise(int d, const JlsParams& p) {
    if (d <= -p.t3) return -4;
    if (d <= -p.t2) return -3;
    if (d <= -p.t1) return -2;
    if (d < -p.near_) return -1;
    if (d <= p.near_) return 0;
    if (d < p.t1) return 1;
    if (d < p.t2) return 2;
    if (d < p.t3) return 3;
    return 4;
}

// what a sample's context owes to the row above alone: (81 Q(Rd - Rb) + 9 Q(Rb - Rc)) << 16 | Rb; the upper half is 0 exactly
// where the row above is flat (the run precondition)
JLS_HD inline uint32_t jls_pre_word(int Rb, int Rc, int Rd, const JlsParams& p) {
    const int q12 = 81 * jls_quantise(Rd - Rb, p) + 9 * jls_quantise(Rb - Rc, p);
    return ((uint32_t)(uint16_t)(int16_t)q12 << 16) | (uint32_t)Rb;
}

JLS_HD inline int jls_predict(int Ra, int Rb, int Rc) {
    const int lo = Ra < Rb ? Ra : Rb, hi = Ra < Rb ? Rb : Ra;
    return Rc >= hi ? lo : Rc <= lo ? hi : Ra + Rb - Rc;
}

JLS_HD inline int jls_k(int N, uint32_t A) {
    // the smallest k with N << k >= A (N >= 1): the difference of the bit lengths, or one more
    const int d = jls_clz64((uint64_t)(uint32_t)N) - jls_clz64((uint64_t)A), k = d > 0 ? d : 0;
    return k + (((uint64_t)(uint32_t)N << k) < (uint64_t)A ? 1 : 0);
}

// modulo RANGE (2 NEAR + 1), then clamped to [0, MAXVAL]
JLS_HD inline int jls_fix(int x, const JlsParams& p) {
    if (x < -p.near_) x += p.wrap;
    else if (x > p.maxval + p.near_) x -= p.wrap;
    return x < 0 ? 0 : x > p.maxval ? p.maxval : x;
}

JLS_HD inline int jls_unmap(uint32_t m, int k, const JlsCtx& c, const JlsParams& p) {
    if (p.near_ == 0 && k == 0 && 2 * c.B <= -c.N) return (m & 1u) ? (int)((m - 1u) >> 1) : -(int)(m >> 1) - 1;
    return (m & 1u) ? -(int)((m + 1u) >> 1) : (int)(m >> 1);
}

// T.87 A.6.1 - A.6.3: A, B, the halving at RESET, N, then the bias with C in [-128, 127]
JLS_HD inline void jls_update(JlsCtx& c, int e, const JlsParams& p) {
    c.B += e * p.step;
    c.A = (int)((uint32_t)c.A + (uint32_t)(e < 0 ? -e : e));
    if (c.N == p.reset) {
        c.A = (int)((uint32_t)c.A >> 1);
        c.B >>= 1;
        c.N >>= 1;
    }
    c.N += 1;
    if (c.B <= -c.N) {
        c.B += c.N;
        if (c.C > -128) --c.C;
        if (c.B <= -c.N) c.B = -c.N + 1;
    } else if (c.B > 0) {
        c.B -= c.N;
        if (c.C < 127) ++c.C;
        if (c.B > 0) c.B = 0;
    }
}

template <bool U, class CtxPtr>
JLS_HD inline JlsCtx jls_ctx_load(CtxPtr ctx, int i) {
    const JlsCtx c = ctx[i];
    return JlsCtx{jls_uni<U>(c.A), jls_uni<U>(c.B), jls_uni<U>(c.C), jls_uni<U>(c.N)};
}

template <bool U, class CtxPtr>
JLS_HD inline int jls_regular(JlsBits& b, const JlsParams& p, CtxPtr ctx, int qs, int Ra, int Rb, int Rc, int* bad) {
    const int sign = qs < 0 ? -1 : 1, q = qs < 0 ? -qs : qs;
    JlsCtx c = jls_ctx_load<U>(ctx, q);
    int px = jls_predict(Ra, Rb, Rc) + sign * c.C;
    px = px < 0 ? 0 : px > p.maxval ? p.maxval : px;
    const int k = jls_k(c.N, (uint32_t)c.A);
    const uint32_t m = jls_golomb<U>(b, p, k, p.limit, bad);
    if (*bad) return 0;
    int e = jls_unmap(m, k, c, p);
    jls_update(c, e, p);
    ctx[q] = c;
    e *= p.step;
    return jls_fix(px + (sign < 0 ? -e : e), p);
}

// T.87 A.7.2: the sample that ends a run
template <bool U, class CtxPtr>
JLS_HD inline int jls_run_interruption(JlsBits& b, const JlsParams& p, CtxPtr ctx, int Ra, int Rb, int runindex, int* bad) {
    const int d = Ra - Rb, type = (d < 0 ? -d : d) <= p.near_ ? 1 : 0;
    JlsCtx c = jls_ctx_load<U>(ctx, 365 + type);
    const uint32_t temp = (uint32_t)c.A + (type ? (uint32_t)(c.N >> 1) : 0u);
    const int k = jls_k(c.N, temp);
    const uint32_t m = jls_golomb<U>(b, p, k, p.limit - jls_J(runindex) - 1, bad);
    if (*bad) return 0;
    const uint32_t t = m + (uint32_t)type;
    const bool map = t & 1u, cond = k != 0 || 2 * c.B >= c.N;
    const int ea = (int)((t + 1u) >> 1), e = cond == map ? -ea : ea;
    if (e < 0) c.B += 1;
    c.A = (int)((uint32_t)c.A + ((m + 1u - (uint32_t)type) >> 1));
    if (c.N == p.reset) {
        c.A = (int)((uint32_t)c.A >> 1);
        c.B >>= 1;
        c.N >>= 1;
    }
    c.N += 1;
    ctx[365 + type] = c;
    if (type) return jls_fix(Ra + e * p.step, p);
    return jls_fix(Rb + (Rb >= Ra ? e : -e) * p.step, p);
}

// ---------------------------------------------------------------------------------------------------- one row of the chain
// Row policy R: look(x, Rc, &Rb) -> the pre word of sample x (jls_pre_word), above(x) -> Rb at x, put(x, v), fill(x0, x1, v).
// Ra0: the row above's first sample (0 for the first row), corner: the Ra0 of the row above.  Returns non-zero where the stream
// is invalid; *runindex persists over the rows of a scan.
template <bool U, class R, class CtxPtr>
JLS_HD inline int jls_row(JlsBits& b, const JlsParams& p, CtxPtr ctx, R& row, int cols, int Ra0, int corner, int* runindex) {
    int x = 0, Ra = Ra0, Rc = corner, bad = 0;
    while (x < cols) {
        int Rb;
        const uint32_t w = row.look(x, Rc, &Rb);
        const int q12 = (int)(int16_t)(uint16_t)(w >> 16), d3 = Rc - Ra;
        if (q12 == 0 && (d3 < 0 ? -d3 : d3) <= p.near_) {
            const int x0 = x;
            bool more = true;
            while (more && x < cols) {                      // every one bit moves x on: at most `cols` rounds
                jls_refill<U>(b);
                more = jls_take(b, 1) != 0u;
                if (more) {
                    const int full = 1 << jls_J(*runindex), cnt = full < cols - x ? full : cols - x;
                    x += cnt;
                    if (cnt == full && *runindex < 31) ++*runindex;
                }
            }
            if (!more) {
                const int j = jls_J(*runindex);
                x += j ? (int)jls_take(b, j) : 0;
                if (x > cols) {
                    row.fill(x0, cols, Ra);
                    return 1;
                }
            }
            row.fill(x0, x, Ra);
            if (x >= cols) break;
            Rb = row.above(x);
            const int Rx = jls_run_interruption<U>(b, p, ctx, Ra, Rb, *runindex, &bad);
            if (bad) return 1;
            row.put(x, Rx);
            if (*runindex > 0) --*runindex;
            Ra = Rx;
        } else {
            const int Rx = jls_regular<U>(b, p, ctx, q12 + jls_quantise(d3, p), Ra, Rb, Rc, &bad);
            if (bad) return 1;
            row.put(x, Rx);
            Ra = Rx;
        }
        Rc = Rb;
        ++x;
    }
    return 0;
}

JLS_HD inline int jls_status(const JlsBits& b, int bad) { return b.over ? JLS_ST_TRUNCATED : bad ? JLS_ST_INVALID : JLS_ST_OK; }

// ---------------------------------------------------------------------------------------------------- the plain loop
// The row above is read where the samples were written (out, rows x cols); the first row sees zeros.
struct JlsPlainRow {
    const uint16_t* prev;        // NULL: the first row
    uint16_t* cur;
    int cols;
    const JlsParams* p;
    JLS_HD int above(int x) const { return prev ? (int)prev[x < cols ? x : cols - 1] : 0; }
    JLS_HD uint32_t look(int x, int Rc, int* Rb) const {
        *Rb = above(x);
        return jls_pre_word(*Rb, Rc, above(x + 1), *p);
    }
    JLS_HD void put(int x, int v) { cur[x] = (uint16_t)v; }
    JLS_HD void fill(int x0, int x1, int v) {
        for (int i = x0; i < x1; ++i) cur[i] = (uint16_t)v;
    }
};

// one scan, one caller: ctx = JLS_CONTEXTS records of scratch
JLS_HD inline int jls_decode_plain(const uint32_t* words, uint32_t len, const JlsParams& p, int rows, int cols, uint16_t* out,
                                   JlsCtx* ctx) {
    for (int i = 0; i < JLS_CONTEXTS; ++i) ctx[i] = jls_ctx_init(p);
    JlsBits b = jls_bits_open<false>(words, len);
    int runindex = 0, corner = 0, bad = 0;
    for (int r = 0; r < rows && !bad; ++r) {
        JlsPlainRow row{r ? out + (size_t)(r - 1) * cols : nullptr, out + (size_t)r * cols, cols, &p};
        const int Ra0 = row.above(0);
        bad = jls_row<false>(b, p, ctx, row, cols, Ra0, corner, &runindex);
        corner = Ra0;
    }
    return jls_status(b, bad);
}
