// Deflate encoder for label volumes (boa_deflate_members): the payload of a .nii.gz is cut into gzip members, every member into
// deflate blocks of DFL_BLK input bytes, one workgroup per block.  RFC 1951 (the stream), RFC 1952 (CRC-32 of each member).
//   k_deflate_block    match lengths against a near distance (1 .. 16) and distance row_bytes, greedy parse by pointer jumping, fixed-Huffman
//                      bit assembly in LDS (or a stored block where that is not smaller), the block's CRC-32; one slot per block.
//                      <true>: also counts the block's symbols, builds optimal length-limited codes and writes a dynamic-Huffman
//                      block where that is smaller than both other forms
//   k_deflate_scan     block sizes -> byte offsets; CRCs of the blocks -> CRC of each member
//   k_deflate_compact  slots -> one contiguous body per member
// Every block ends on a byte boundary (an empty stored block after a non-final fixed block, as pigz does), so bodies concatenate
// by byte copy.  A match never reaches before its member's first byte nor past its block's last, so a member inflates alone.
// boa_deflate_label_pairs runs the same three kernels over a list of (label, member) pairs of a label volume: a pair takes the
// place of the member, and k_deflate_block<., true> fills LDS with (byte == label) instead of the byte, so the mask exists in LDS only.
#include <algorithm>

#include "common.h"
#include "crc32_dev.h"
#include "deflate_codes.h"

namespace {

constexpr int DFL_BLK = 16384;                 // input bytes per deflate block
constexpr int DFL_NT = 1024;                   // threads per block workgroup
constexpr int DFL_PIECE = DFL_BLK / DFL_NT;    // positions per thread (16: one uint4 of payload, one half mark word)
constexpr int DFL_SLOT = DFL_BLK + 16;         // bytes of a block's slot in the workspace (a stored block is 5 + DFL_BLK)
constexpr int DFL_MAXLEN = 258;
constexpr int DFL_MAXROW = 32768;
constexpr int DFL_LOOK = (DFL_MAXLEN + DFL_PIECE - 1) / DFL_PIECE;   // pieces a run is followed into
static_assert(DFL_PIECE == 16, "the match scan reads one uint4 per thread");

// LDS carve (bytes).  s_next is reused for the assembled bits once the parse is known.
constexpr int OFF_NEXT = 0;                                    // uint16 [DFL_BLK + 8]
constexpr int OFF_TOK = OFF_NEXT + (DFL_BLK + 8) * 2;          // uint16 [DFL_BLK]: match length (0 = literal) | 0x8000 if the row distance
constexpr int OFF_MARK = OFF_TOK + DFL_BLK * 2;                // uint32 [DFL_BLK / 32 + 4]: bit i = position i starts a token
constexpr int OFF_TAB = OFF_MARK + (DFL_BLK / 32 + 4) * 4;     // uint32 [256]: byte-wise CRC table
constexpr int OFF_LEAD = OFF_TAB + 1024;                       // uint8 [2][DFL_NT]: leading equal positions of each piece
constexpr int OFF_MISC = OFF_LEAD + 2 * DFL_NT;                // uint32 [32]
constexpr int OFF_DATA = OFF_MISC + 128;                       // uint8 [hist + DFL_BLK + 16]: history, then the block
static_assert(OFF_DATA % 16 == 0 && OFF_TOK % 16 == 0 && OFF_MARK % 16 == 0, "LDS carve alignment");
static_assert(OFF_DATA >= DFL_MAXROW + 16, "a row candidate of an early piece reads below s_d, inside the carve");

// What a launch encodes: every member of the payload in file order (first == nullptr), or a list of pairs.  Pair p is member
// member[p] of the mask (payload == label[p]); its blocks are [first[p], first[p + 1]) of the grid.
struct DflPairs {
    const unsigned* first;           // [n + 1]
    const unsigned* member;          // [n]
    const unsigned char* label;      // [n]
    unsigned n;
};

// four bytes of w -> 1 where the byte equals the label (lab4 = the label in every byte), else 0
__device__ __forceinline__ unsigned eq_label4(unsigned w, unsigned lab4) {
    const unsigned x = w ^ lab4;
    const unsigned nz = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;      // bit 7 of a byte = that byte of x is not zero
    return (~nz >> 7) & 0x01010101u;
}

// bit k = (block byte p0 + k equals the byte `d` before it); 16 positions.  Reads LDS words only; the caller masks what is invalid.
__device__ __forceinline__ unsigned eq_mask16(const unsigned char* s_d, int a, const uint4 own) {
    const unsigned* w = (const unsigned*)(s_d + (a & ~3));
    const int sh = (a & 3) * 8;
    unsigned v[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) v[j] = w[j];
    const unsigned o[4] = {own.x, own.y, own.z, own.w};
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned b = sh ? (v[j] >> sh) | (v[j + 1] << (32 - sh)) : v[j];
        const unsigned x = b ^ o[j];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (((x >> (8 * q)) & 0xffu) == 0) mask |= 1u << (4 * j + q);
    }
    return mask;
}

__device__ __forceinline__ void or_bits(unsigned* words, unsigned bit_off, uint64_t bits) {
    const uint64_t v = bits << (bit_off & 31);
    const unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    if (lo) atomicOr(&words[bit_off >> 5], lo);
    if (hi) atomicOr(&words[(bit_off >> 5) + 1], hi);
}

// ---- dynamic-Huffman blocks: work arrays inside the s_next region, which is dead once the parse is known.  What the bit assembly
// still reads (DW_*) lies above the words s_out can use: a block is written dynamic only where that is smaller than stored, so
// s_out ends below DFL_BLK + 16 bytes.  The scratch of the code construction (DS_*) lies below and is dead before s_out is zeroed.
constexpr int DW_KEEP = OFF_NEXT + DFL_BLK + 32;
constexpr int DW_HLL = DW_KEEP;                    // uint32 [288]: literal/length counts
constexpr int DW_HD = DW_HLL + 288 * 4;            // uint32 [32]: distance counts
constexpr int DW_HCL = DW_HD + 32 * 4;             // uint32 [32]: code-length symbol counts
constexpr int DW_CNT = DW_HCL + 32 * 4;            // uint32 [16]: scalars (DC_*)
constexpr int DW_ZERO_WORDS = 288 + 32 + 32 + 16;  // the four above are zeroed together
constexpr int DW_TLL = DW_CNT + 16 * 4;            // uint32 [288]: stream bits | length << 16 per literal/length symbol
constexpr int DW_TD = DW_TLL + 288 * 4;            // uint32 [32]
constexpr int DW_TCL = DW_TD + 32 * 4;             // uint32 [32]
constexpr int DW_LLL = DW_TCL + 32 * 4;            // uint8 [288]: code lengths
constexpr int DW_LD = DW_LLL + 288;                // uint8 [32]
constexpr int DW_LCL = DW_LD + 32;                 // uint8 [32]
constexpr int DW_SEQ = DW_LCL + 32;                // uint8 [320]: the lengths the header codes, HLIT then HDIST of them
constexpr int DW_HSYM = DW_SEQ + 320;              // uint16 [320]: their run-length code
constexpr int DW_END = DW_HSYM + 320 * 2;
constexpr int DS_CUR = OFF_NEXT;                   // uint32 [2][576]: item weights of the last two levels
constexpr int DS_LEAFW = DS_CUR + 2 * 576 * 4;     // uint32 [288]: counts of the used symbols, sorted
constexpr int DS_LEAFS = DS_LEAFW + 288 * 4;       // uint16 [288]: their symbols
constexpr int DS_PKPOS = DS_LEAFS + 288 * 2;       // uint16 [16][288]: position of every package in its level
constexpr int DS_LEV = DS_PKPOS + 16 * 288 * 2;    // uint32 [2][16]: packages of a level; leaves taken from a level
static_assert(DS_LEV + 32 * 4 <= DW_KEEP && DW_END <= OFF_TOK && DW_KEEP % 16 == 0, "dynamic-code carve");
static_assert(DW_KEEP - OFF_NEXT >= ((5 + DFL_BLK + 3) / 4 + 1) * 4, "s_out of a block smaller than stored ends below the kept arrays");
enum { DC_LL_USED = 0, DC_LL_LAST, DC_D_USED, DC_D_LAST, DC_CL_USED, DC_CL_LAST, DC_EXTRA, DC_TOKBITS, DC_HDRBITS, DC_NHSYM, DC_HCLEN };

// Code lengths of at most `limit` bits with the least total cost for the counts freq[0 .. nsym) (0 = unused symbol -> length 0), by
// package-merge, the whole workgroup at work; one used symbol gets length 1.  cnt[0] / cnt[1] (zero on entry) return the number of
// used symbols and the last one + 1.  The leaves are sorted by (count, symbol) with a rank count.  Level 1 is the leaves; level l
// merges the leaves with the packages (pairs in order) of level l - 1, every item finding its place by a binary search in the other
// list (a tie puts the leaf first), cut at 2 n - 2 items.  The first 2 n - 2 items of the last level are the solution: the packages
// among them stand for twice as many items of the level below, and a symbol's length is the number of levels that take its leaf.
// nsym <= 286, 2^limit >= nsym; ends with a barrier.
__device__ void dfl_limited_lengths(const unsigned* freq, int nsym, int limit, unsigned char* len, unsigned* cnt, unsigned char* smem, int t) {
    unsigned* cur = (unsigned*)(smem + DS_CUR);
    unsigned* leafw = (unsigned*)(smem + DS_LEAFW);
    unsigned short* leafs = (unsigned short*)(smem + DS_LEAFS);
    unsigned short* pkpos = (unsigned short*)(smem + DS_PKPOS);
    unsigned* lev = (unsigned*)(smem + DS_LEV);
    if (t < nsym) {
        const unsigned f = freq[t];
        len[t] = 0;
        if (f) {
            int rank = 0;
            for (int s = 0; s < nsym; ++s) {
                const unsigned fs = freq[s];
                rank += (fs && (fs < f || (fs == f && s < t))) ? 1 : 0;
            }
            leafw[rank] = f;
            leafs[rank] = (unsigned short)t;
            atomicAdd(&cnt[0], 1u);
            atomicMax(&cnt[1], (unsigned)t + 1);
        }
    }
    __syncthreads();
    const int n = (int)cnt[0];
    if (n < 2) {
        if (n == 1 && t == 0) len[leafs[0]] = 1;
        __syncthreads();
        return;
    }
    const int cap = 2 * n - 2;
    if (t < n) cur[t] = leafw[t];
    int m = n;                                               // items of the level below
    __syncthreads();
    for (int l = 2; l <= limit; ++l) {
        const unsigned* below = cur + ((l & 1) ? 576 : 0);
        unsigned* here = cur + ((l & 1) ? 0 : 576);
        const int np = m >> 1;
        if (t < n) {
            const unsigned w = leafw[t];
            int lo = 0, hi = np;                             // the packages lighter than this leaf
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (below[2 * mid] + below[2 * mid + 1] < w) lo = mid + 1; else hi = mid;
            }
            if (t + lo < cap) here[t + lo] = w;
        } else if (t >= 512 && t - 512 < np) {
            const int q = t - 512;
            const unsigned w = below[2 * q] + below[2 * q + 1];
            int lo = 0, hi = n;                              // the leaves that are not heavier than this package
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (leafw[mid] <= w) lo = mid + 1; else hi = mid;
            }
            const int pos = q + lo;
            pkpos[l * 288 + q] = (unsigned short)(pos < cap ? pos : cap);
            if (pos < cap) here[pos] = w;
        }
        if (t == 0) lev[l] = (unsigned)np;
        m = n + np < cap ? n + np : cap;
        __syncthreads();
    }
    if (t == 0) {
        int take = cap;                                      // items taken from the level
        for (int l = limit; l >= 2; --l) {
            int lo = 0, hi = (int)lev[l];                    // the packages among them
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pkpos[l * 288 + mid] < take) lo = mid + 1; else hi = mid;
            }
            lev[16 + l] = (unsigned)(take - lo);
            take = 2 * lo;
        }
        lev[16 + 1] = (unsigned)take;
    }
    __syncthreads();
    if (t < n) {
        unsigned L = 0;
        for (int l = 1; l <= limit; ++l) L += (unsigned)t < lev[16 + l] ? 1u : 0u;
        len[leafs[t]] = (unsigned char)L;
    }
    __syncthreads();
}

// f(position, token) for every token start of a thread's piece
template <class F>
__device__ __forceinline__ void for_each_token(unsigned starts, int p0, const unsigned short* s_tok, F f) {
    for (unsigned m = starts; m; m &= m - 1) {
        const int i = p0 + __builtin_ctz(m);
        f(i, (unsigned)s_tok[i]);
    }
}

// grid = blocks of all members in file order; dynamic LDS = OFF_DATA + hist + DFL_BLK + 16.  DYN: also try a dynamic-Huffman block
// (BTYPE = 10) and take it where it is smaller than both other forms; near = the short candidate distance (1 without DYN).
// PAIRS: grid = the blocks of the pairs of `pr` in list order; the payload of a pair's block is (src byte == label) ? 1 : 0.
template <bool DYN, bool PAIRS>
__global__ __launch_bounds__(DFL_NT) void k_deflate_block(const unsigned char* __restrict__ src, size_t n, unsigned member_bytes,
                                                          unsigned bpm, int row, int hist, int near_arg, const unsigned* __restrict__ pw,
                                                          unsigned* __restrict__ ws, unsigned* __restrict__ blk_size, unsigned* __restrict__ blk_crc,
                                                          const DflPairs pr) {
    const int near = DYN ? near_arg : 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned short* s_next = (unsigned short*)(smem + OFF_NEXT);
    unsigned* s_out = (unsigned*)(smem + OFF_NEXT);
    unsigned short* s_tok = (unsigned short*)(smem + OFF_TOK);
    unsigned* s_mark = (unsigned*)(smem + OFF_MARK);
    unsigned* s_tab = (unsigned*)(smem + OFF_TAB);
    unsigned char* s_lead = smem + OFF_LEAD;
    unsigned* s_misc = (unsigned*)(smem + OFF_MISC);
    unsigned char* s_d = smem + OFF_DATA;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t g = blockIdx.x;
    size_t moff;
    unsigned boff;                                                                    // block start inside its member
    unsigned lab4 = 0;
    if constexpr (PAIRS) {
        unsigned lo = 0, hi = pr.n;                                                   // the last pair whose first block is not after g
        while (hi - lo > 1) {
            const unsigned mid = (lo + hi) >> 1;
            if (pr.first[mid] <= g) lo = mid; else hi = mid;
        }
        moff = pr.member[lo] * (size_t)member_bytes;
        boff = ((unsigned)g - pr.first[lo]) * DFL_BLK;
        lab4 = pr.label[lo] * 0x01010101u;
    } else {
        moff = (g / bpm) * (size_t)member_bytes;
        boff = (unsigned)(g % bpm) * DFL_BLK;
    }
    const size_t mlen = n - moff < member_bytes ? n - moff : member_bytes;            // 0 only for the empty payload
    const int blen = (int)(mlen - boff < (size_t)DFL_BLK ? mlen - boff : DFL_BLK);
    const bool bfinal = boff + (size_t)blen == mlen;
    const int avail = boff < (unsigned)hist ? (int)boff : hist;                       // history bytes of the same member (multiple of 16)
    const int H = hist;

    // ---- payload -> LDS, CRC table, marks ----
    {
        const unsigned char* gsrc = src + moff + boff - avail;
        unsigned char* ldst = s_d + H - avail;
        const int total = avail + blen;
        const int n16 = ((uintptr_t)gsrc & 15) == 0 ? total >> 4 : 0;
        if constexpr (PAIRS) {
            // the mask is made here and nowhere else: history, CRC, matches and the stored form all read LDS
            for (int i = t; i < n16; i += DFL_NT) {
                const uint4 v = ((const uint4*)gsrc)[i];
                ((uint4*)ldst)[i] = make_uint4(eq_label4(v.x, lab4), eq_label4(v.y, lab4), eq_label4(v.z, lab4), eq_label4(v.w, lab4));
            }
            for (int i = n16 * 16 + t; i < total; i += DFL_NT) ldst[i] = gsrc[i] == (lab4 & 0xffu) ? 1 : 0;
        } else {
            for (int i = t; i < n16; i += DFL_NT) ((uint4*)ldst)[i] = ((const uint4*)gsrc)[i];
            for (int i = n16 * 16 + t; i < total; i += DFL_NT) ldst[i] = gsrc[i];
        }
    }
    if (t < 256) s_tab[t] = crc32_table_entry((unsigned)t);
    for (int i = t; i < DFL_BLK / 32 + 4; i += DFL_NT) s_mark[i] = (i == 0 && blen > 0) ? 1u : 0u;
    __syncthreads();

    // ---- CRC-32: pieces of 16 bytes aligned to the block's END (the first may be short or empty: crc32("") = 0), combined in
    // a tree inside each wave, then across the 16 waves ----
    {
        const int hi = blen - DFL_PIECE * (DFL_NT - 1 - t);
        const unsigned c0 = crc32_update(s_tab, 0xffffffffu, s_d + H, hi - DFL_PIECE > 0 ? hi - DFL_PIECE : 0, hi);
        unsigned c = c0 ^ 0xffffffffu;
#pragma unroll
        for (int k = 0; k < 6; ++k) {        // after step k the lanes that are multiples of 2^(k+1) hold 2^(k+1) pieces
            const unsigned right = __shfl_down(c, 1 << k, 64);
            c = dfl_gf2_mul(pw[4 + k], c) ^ right;
        }
        if (lane == 0) s_misc[wave] = c;     // 1 KiB each
        __syncthreads();
        if (wave == 0) {
            unsigned v = 0;
            if (lane < DFL_NT / 64) v = dfl_gf2_mul(dfl_crc_xpow(pw, 1024ull * (DFL_NT / 64 - 1 - lane)), s_misc[lane]);
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) v ^= __shfl_xor(v, k, 64);
            if (lane == 0) blk_crc[g] = v;
        }
        __syncthreads();
    }

    // ---- match lengths.  Thread t owns positions [16 t, 16 t + 16). ----
    const int p0 = t * DFL_PIECE;
    unsigned eq1 = 0, eqr = 0;
    {
        const uint4 own = *(const uint4*)(s_d + H + p0);
        const int inside = blen - p0;                                             // positions of this piece inside the block
        const unsigned in_mask = inside >= DFL_PIECE ? 0xffffu : inside > 0 ? (1u << inside) - 1 : 0u;
        if (in_mask) {
            const int first1 = near - avail - p0;                                 // first k whose source byte is in the member
            const unsigned m1 = in_mask & (first1 <= 0 ? 0xffffu : first1 >= DFL_PIECE ? 0u : 0xffffu << first1);
            if (m1) eq1 = eq_mask16(s_d, H + p0 - near, own) & m1;
            if (row > 0) {
                const int firstr = row - avail - p0;
                const unsigned mr = in_mask & (firstr <= 0 ? 0xffffu : firstr >= DFL_PIECE ? 0u : 0xffffu << firstr);
                if (mr) eqr = eq_mask16(s_d, H + p0 - row, own) & mr;
            }
        }
        s_lead[t] = (unsigned char)__builtin_ctz(~eq1 & 0x1ffffu);
        s_lead[DFL_NT + t] = (unsigned char)__builtin_ctz(~eqr & 0x1ffffu);
    }
    __syncthreads();
    {
        // the runs that leave this piece: full pieces behind it, then the lead of the first that is not
        int run1 = 0, runr = 0;
        for (int k = 1; k <= DFL_LOOK && t + k < DFL_NT; ++k) {
            const int l = s_lead[t + k];
            run1 += l;
            if (l < DFL_PIECE) break;
        }
        for (int k = 1; k <= DFL_LOOK && t + k < DFL_NT; ++k) {
            const int l = s_lead[DFL_NT + t + k];
            runr += l;
            if (l < DFL_PIECE) break;
        }
        unsigned tok[8], nxt[8];
#pragma unroll
        for (int k = DFL_PIECE - 1; k >= 0; --k) {
            run1 = (eq1 >> k) & 1 ? run1 + 1 : 0;
            runr = (eqr >> k) & 1 ? runr + 1 : 0;
            const int l1 = run1 < DFL_MAXLEN ? run1 : DFL_MAXLEN, lr = runr < DFL_MAXLEN ? runr : DFL_MAXLEN;
            int L = l1 >= lr ? l1 : lr;                    // a tie goes to the near distance: no or fewer extra distance bits
            const unsigned far = l1 >= lr ? 0u : 0x8000u;
            if (L < 3) L = 0;
            const int i = p0 + k;
            const unsigned tv = (unsigned)L | (L ? far : 0u);
            const unsigned nv = i < blen ? (unsigned)(i + (L ? L : 1)) : (unsigned)blen;
            if (k & 1) {
                tok[k >> 1] = tv << 16;
                nxt[k >> 1] = nv << 16;
            } else {
                tok[k >> 1] |= tv;
                nxt[k >> 1] |= nv;
            }
        }
        uint4* pt = (uint4*)(s_tok + p0);
        uint4* pn = (uint4*)(s_next + p0);
        pt[0] = make_uint4(tok[0], tok[1], tok[2], tok[3]);
        pt[1] = make_uint4(tok[4], tok[5], tok[6], tok[7]);
        pn[0] = make_uint4(nxt[0], nxt[1], nxt[2], nxt[3]);
        pn[1] = make_uint4(nxt[4], nxt[5], nxt[6], nxt[7]);
        if (t == 0) s_next[DFL_BLK] = (unsigned short)blen;
    }
    __syncthreads();

    // ---- greedy parse: the token starts are the orbit of 0 under next[].  After round r, next[] jumps 2^r tokens and the first
    // 2^r tokens are marked; every marked position then marks its image.  Position blen is the fixed point. ----
    {
        int rounds = 0;
        while ((1 << rounds) < blen) ++rounds;               // at most log2(DFL_BLK)
        for (int r = 0; r < rounds; ++r) {
            unsigned pair[DFL_PIECE];
            unsigned marked = 0;
#pragma unroll
            for (int j = 0; j < DFL_PIECE; ++j) {
                const int i = t + DFL_NT * j;
                const unsigned nx = s_next[i];
                pair[j] = nx | ((unsigned)s_next[nx] << 16);
                marked |= ((s_mark[i >> 5] >> (i & 31)) & 1u) << j;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < DFL_PIECE; ++j) {
                const int i = t + DFL_NT * j;
                const unsigned nx = pair[j] & 0xffffu;
                if ((marked >> j) & 1) atomicOr(&s_mark[nx >> 5], 1u << (nx & 31));
                s_next[i] = (unsigned short)(pair[j] >> 16);
            }
            __syncthreads();
        }
    }

    // ---- token bit lengths -> bit offsets ----
    const int inside = blen - p0;
    const unsigned starts = (s_mark[p0 >> 5] >> (p0 & 31)) & (inside >= DFL_PIECE ? 0xffffu : inside > 0 ? (1u << inside) - 1 : 0u);
    const int far_dist = row;
    unsigned my_bits = 0;
    for (unsigned m = starts; m; m &= m - 1) {
        const int i = p0 + __builtin_ctz(m);
        const unsigned tv = s_tok[i];
        int nb;
        if (tv & 0x7fffu)
            dfl_match(tv & 0x7fffu, (tv & 0x8000u) ? far_dist : near, &nb);
        else
            dfl_literal(s_d[H + i], &nb);
        my_bits += nb;
    }
    unsigned incl = my_bits;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const unsigned up = __shfl_up(incl, k, 64);
        if (lane >= k) incl += up;
    }
    if (lane == 63) s_misc[wave] = incl;
    __syncthreads();                                            // (also: s_next is dead from here on, s_out may be written)
    unsigned before = 0, tok_bits = 0;
    for (int w = 0; w < DFL_NT / 64; ++w) {
        const unsigned v = s_misc[w];
        if (w < wave) before += v;
        tok_bits += v;
    }
    // 3 header bits, the tokens, 7 bits of end-of-block; a non-final block then gets 3 header bits of an empty stored block,
    // padding to a byte and 00 00 FF FF; the final block is only padded
    const unsigned end_bit = 3 + tok_bits + 7;
    const unsigned sync_byte = (end_bit + 3 + 7) >> 3;
    const unsigned fixed_bytes = bfinal ? (end_bit + 7) >> 3 : sync_byte + 4;
    const unsigned stored_bytes = 5 + blen;
    const bool fixed = fixed_bytes < stored_bytes;
    const unsigned out_bytes = fixed ? fixed_bytes : stored_bytes;
    const unsigned out_words = (out_bytes + 3) >> 2;            // <= DFL_SLOT / 4
    unsigned* slot = ws + g * (size_t)(DFL_SLOT / 4);
    if constexpr (DYN) {
        unsigned* h_ll = (unsigned*)(smem + DW_HLL);
        unsigned* h_d = (unsigned*)(smem + DW_HD);
        unsigned* h_cl = (unsigned*)(smem + DW_HCL);
        unsigned* cnt = (unsigned*)(smem + DW_CNT);
        unsigned* t_ll = (unsigned*)(smem + DW_TLL);
        unsigned* t_d = (unsigned*)(smem + DW_TD);
        unsigned* t_cl = (unsigned*)(smem + DW_TCL);
        unsigned char* l_ll = smem + DW_LLL;
        unsigned char* l_d = smem + DW_LD;
        unsigned char* l_cl = smem + DW_LCL;
        unsigned char* seq = smem + DW_SEQ;
        unsigned short* hsym = (unsigned short*)(smem + DW_HSYM);
        int near_eb, far_eb = 0;
        unsigned near_ev, far_ev = 0, far_sym = 0;
        const unsigned near_sym = dfl_dist_symbol((unsigned)near, &near_eb, &near_ev);
        if (far_dist > 0) far_sym = dfl_dist_symbol((unsigned)far_dist, &far_eb, &far_ev);

        // ---- counts of the literal/length and distance symbols over the token starts; a thread adds runs of one symbol at once ----
        for (int i = t; i < DW_ZERO_WORDS; i += DFL_NT) h_ll[i] = 0;
        __syncthreads();
        {
            unsigned extra = 0, n_near = 0, n_far = 0, run = 0, cur = 0;
            for_each_token(starts, p0, s_tok, [&](int i, unsigned tv) {
                unsigned sym;
                if (tv & 0x7fffu) {
                    int eb;
                    unsigned ev;
                    sym = dfl_len_symbol(tv & 0x7fffu, &eb, &ev);
                    extra += (unsigned)eb;
                    if (tv & 0x8000u) ++n_far; else ++n_near;
                } else
                    sym = s_d[H + i];
                if (run && sym != cur) {
                    atomicAdd(&h_ll[cur], run);
                    run = 0;
                }
                cur = sym;
                ++run;
            });
            if (run) atomicAdd(&h_ll[cur], run);
            if (n_near) atomicAdd(&h_d[near_sym], n_near);
            if (n_far) atomicAdd(&h_d[far_sym], n_far);
            extra += n_near * (unsigned)near_eb + n_far * (unsigned)far_eb;
            if (extra) atomicAdd(&cnt[DC_EXTRA], extra);
            if (t == 0) h_ll[256] = 1;                      // end of block (no token counts it)
        }
        __syncthreads();

        // ---- code lengths, the header's run-length code and its code lengths ----
        dfl_limited_lengths(h_ll, DFL_NLL, 15, l_ll, cnt + DC_LL_USED, smem, t);
        dfl_limited_lengths(h_d, DFL_ND, 15, l_d, cnt + DC_D_USED, smem, t);
        const int hlit = (int)cnt[DC_LL_LAST];                                  // >= 257: the end-of-block symbol is in use
        const int hdist = cnt[DC_D_LAST] ? (int)cnt[DC_D_LAST] : 1;             // no match at all: one distance code of length zero
        if (t < hlit) seq[t] = l_ll[t];
        else if (t < hlit + hdist) seq[t] = l_d[t - hlit];
        __syncthreads();
        if (t == 0) cnt[DC_NHSYM] = (unsigned)dfl_rle_lengths(seq, hlit + hdist, hsym, h_cl);
        __syncthreads();
        dfl_limited_lengths(h_cl, DFL_NCL, 7, l_cl, cnt + DC_CL_USED, smem, t);

        // ---- code tables; the size of the dynamic form ----
        {
            unsigned bits = 0;
            if (t < DFL_NLL) {
                t_ll[t] = dfl_code_entry(l_ll, DFL_NLL, t);
                bits = h_ll[t] * l_ll[t];
            } else if (t >= 320 && t < 320 + DFL_ND) {
                t_d[t - 320] = dfl_code_entry(l_d, DFL_ND, t - 320);
                bits = h_d[t - 320] * l_d[t - 320];
            } else if (t >= 384 && t < 384 + DFL_NCL) {
                t_cl[t - 384] = dfl_code_entry(l_cl, DFL_NCL, t - 384);
                const unsigned hb = h_cl[t - 384] * (l_cl[t - 384] + (unsigned)dfl_cl_extra_bits(t - 384));
                if (hb) atomicAdd(&cnt[DC_HDRBITS], hb);
            } else if (t == 448) {
                int k = DFL_NCL;
                while (k > 4 && l_cl[dfl_cl_order(k - 1)] == 0) --k;
                cnt[DC_HCLEN] = (unsigned)k;
            }
            if (bits) atomicAdd(&cnt[DC_TOKBITS], bits);
        }
        __syncthreads();
        const unsigned hclen = cnt[DC_HCLEN];
        const unsigned hdr_bits = 3 + 5 + 5 + 4 + 3 * hclen + cnt[DC_HDRBITS];
        const unsigned dyn_end = hdr_bits + cnt[DC_TOKBITS] + cnt[DC_EXTRA];    // (the end-of-block code is in DC_TOKBITS)
        const unsigned dyn_sync = (dyn_end + 3 + 7) >> 3;
        const unsigned dyn_bytes = bfinal ? (dyn_end + 7) >> 3 : dyn_sync + 4;
        if (dyn_bytes < fixed_bytes && dyn_bytes < stored_bytes) {
            // ---- bit offsets from the table's lengths, then the assembly as in the fixed form ----
            unsigned dbits = 0;
            for_each_token(starts, p0, s_tok, [&](int i, unsigned tv) {
                if (tv & 0x7fffu) {
                    int eb;
                    unsigned ev;
                    const unsigned sym = dfl_len_symbol(tv & 0x7fffu, &eb, &ev);
                    dbits += (t_ll[sym] >> 16) + (unsigned)eb;
                    dbits += (tv & 0x8000u) ? (t_d[far_sym] >> 16) + (unsigned)far_eb : (t_d[near_sym] >> 16) + (unsigned)near_eb;
                } else
                    dbits += t_ll[s_d[H + i]] >> 16;
            });
            unsigned dincl = dbits;
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {
                const unsigned up = __shfl_up(dincl, k, 64);
                if (lane >= k) dincl += up;
            }
            if (lane == 63) s_misc[wave] = dincl;
            const unsigned dyn_words = (dyn_bytes + 3) >> 2;
            for (unsigned w = t; w < dyn_words + 1; w += DFL_NT) s_out[w] = 0;
            __syncthreads();
            unsigned off = hdr_bits + (dincl - dbits);
            for (int w = 0; w < wave; ++w) off += s_misc[w];
            for_each_token(starts, p0, s_tok, [&](int i, unsigned tv) {
                if (tv & 0x7fffu) {
                    int eb;
                    unsigned ev;
                    const unsigned e = t_ll[dfl_len_symbol(tv & 0x7fffu, &eb, &ev)];
                    or_bits(s_out, off, (e & 0xffffu) | (uint64_t)ev << (e >> 16));
                    off += (e >> 16) + (unsigned)eb;
                    const bool is_far = (tv & 0x8000u) != 0;
                    const unsigned d = t_d[is_far ? far_sym : near_sym];
                    or_bits(s_out, off, (d & 0xffffu) | (uint64_t)(is_far ? far_ev : near_ev) << (d >> 16));
                    off += (d >> 16) + (unsigned)(is_far ? far_eb : near_eb);
                } else {
                    const unsigned e = t_ll[s_d[H + i]];
                    or_bits(s_out, off, e & 0xffffu);
                    off += e >> 16;
                }
            });
            if (t == 0) {
                // BFINAL, BTYPE = 10, HLIT, HDIST, HCLEN, the code-length code's lengths, the coded lengths; then the end of block
                unsigned o = 0;
                auto put = [&](unsigned v, unsigned nb) {
                    or_bits(s_out, o, v);
                    o += nb;
                };
                put((bfinal ? 1u : 0u) | 4u, 3);
                put((unsigned)hlit - 257, 5);
                put((unsigned)hdist - 1, 5);
                put(hclen - 4, 4);
                for (unsigned k = 0; k < hclen; ++k) put(l_cl[dfl_cl_order((int)k)], 3);
                const unsigned nh = cnt[DC_NHSYM];
                for (unsigned k = 0; k < nh; ++k) {
                    const unsigned hs = hsym[k], e = t_cl[hs & 0xffu];
                    put(e & 0xffffu, e >> 16);
                    put(hs >> 8, (unsigned)dfl_cl_extra_bits(hs & 0xffu));
                }
                or_bits(s_out, dyn_end - (t_ll[256] >> 16), t_ll[256] & 0xffffu);
                if (!bfinal) {
                    atomicOr(&s_out[(dyn_sync + 2) >> 2], 0xffu << (((dyn_sync + 2) & 3) * 8));
                    atomicOr(&s_out[(dyn_sync + 3) >> 2], 0xffu << (((dyn_sync + 3) & 3) * 8));
                }
            }
            __syncthreads();
            for (unsigned w = t; w < dyn_words; w += DFL_NT) slot[w] = s_out[w];
            if (t == 0) blk_size[g] = dyn_bytes;
            return;
        }
        __syncthreads();      // (the fixed form zeroes s_out next: every read of the arrays above is done)
    }
    if (fixed) {
        for (unsigned w = t; w < out_words + 1; w += DFL_NT) s_out[w] = 0;
        __syncthreads();
        unsigned off = 3 + before + (incl - my_bits);
        for (unsigned m = starts; m; m &= m - 1) {
            const int i = p0 + __builtin_ctz(m);
            const unsigned tv = s_tok[i];
            int nb;
            const uint64_t bits = (tv & 0x7fffu) ? dfl_match(tv & 0x7fffu, (tv & 0x8000u) ? far_dist : near, &nb) : dfl_literal(s_d[H + i], &nb);
            or_bits(s_out, off, bits);
            off += nb;
        }
        if (t == 0) {
            atomicOr(&s_out[0], (bfinal ? 1u : 0u) | 2u);       // BFINAL, BTYPE = 01
            if (!bfinal) {
                atomicOr(&s_out[(sync_byte + 2) >> 2], 0xffu << (((sync_byte + 2) & 3) * 8));
                atomicOr(&s_out[(sync_byte + 3) >> 2], 0xffu << (((sync_byte + 3) & 3) * 8));
            }
        }
        __syncthreads();
        for (unsigned w = t; w < out_words; w += DFL_NT) slot[w] = s_out[w];
    } else {
        // stored block: BFINAL + BTYPE = 00 in one byte (the block starts on a byte boundary), LEN, ~LEN, the bytes
        const unsigned head[5] = {bfinal ? 1u : 0u, (unsigned)blen & 0xffu, (unsigned)blen >> 8, ~(unsigned)blen & 0xffu, (~(unsigned)blen >> 8) & 0xffu};
        for (unsigned w = t; w < out_words; w += DFL_NT) {
            unsigned v = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned b = 4 * w + q;
                const unsigned byte = b < 5 ? head[b] : b < stored_bytes ? s_d[H + b - 5] : 0u;
                v |= byte << (8 * q);
            }
            slot[w] = v;
        }
    }
    if (t == 0) blk_size[g] = out_bytes;
}

// one workgroup: exclusive scan of the block sizes (members are consecutive runs of blocks), then one thread per member -- or per
// pair of `pr` (nmem = pr.n), which has the payload length of its member and its own run of blocks
__global__ __launch_bounds__(DFL_NT) void k_deflate_scan(const unsigned* __restrict__ blk_size, const unsigned* __restrict__ blk_crc,
                                                         unsigned nblocks, unsigned bpm, unsigned nmem, size_t n, unsigned member_bytes,
                                                         const unsigned* __restrict__ pw, unsigned long long* __restrict__ blk_off,
                                                         unsigned long long* __restrict__ mem_off, unsigned* __restrict__ mem_crc,
                                                         const DflPairs pr) {
    __shared__ unsigned long long s_wave[DFL_NT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long carry = 0;
    for (unsigned base = 0; base < nblocks; base += DFL_NT) {
        const unsigned i = base + t;
        const unsigned long long v = i < nblocks ? blk_size[i] : 0;
        unsigned long long incl = v;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const unsigned long long up = __shfl_up(incl, k, 64);
            if (lane >= k) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, total = 0;
        for (int w = 0; w < DFL_NT / 64; ++w) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        if (i < nblocks) blk_off[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    for (unsigned m = t; m < nmem; m += DFL_NT) {
        const size_t moff = (size_t)(pr.first ? pr.member[m] : m) * member_bytes;
        const size_t mlen = n - moff < member_bytes ? n - moff : member_bytes;
        const unsigned first = pr.first ? pr.first[m] : m * bpm;
        const unsigned nb = pr.first ? pr.first[m + 1] - first : m + 1 < nmem ? bpm : nblocks - first;
        unsigned c = 0;
        for (unsigned k = 0; k < nb; ++k) {
            const size_t left = mlen - (size_t)k * DFL_BLK;
            c = dfl_crc_combine(pw, c, blk_crc[first + k], left < (size_t)DFL_BLK ? left : DFL_BLK);
        }
        mem_off[m] = blk_off[first];
        mem_crc[m] = c;
    }
    if (t == 0) mem_off[nmem] = carry;
}

__device__ __forceinline__ unsigned slot_byte(const unsigned* w, unsigned i) { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }

// grid = blocks; the slot of block g -> dst + blk_off[g], whole words where the destination allows
__global__ __launch_bounds__(256) void k_deflate_compact(const unsigned* __restrict__ ws, const unsigned* __restrict__ blk_size,
                                                         const unsigned long long* __restrict__ blk_off, unsigned char* __restrict__ dst) {
    const size_t g = blockIdx.x;
    const unsigned* w = ws + g * (size_t)(DFL_SLOT / 4);
    const unsigned sz = blk_size[g];
    unsigned char* d = dst + blk_off[g];
    unsigned head = (unsigned)((4 - ((uintptr_t)d & 3)) & 3);
    if (head > sz) head = sz;
    const unsigned nw = (sz - head) >> 2;
    const int t = threadIdx.x;
    if ((unsigned)t < head) d[t] = (unsigned char)slot_byte(w, t);
    unsigned* dw = (unsigned*)(d + head);
    const unsigned sh = (head & 3) * 8;
    for (unsigned k = t; k < nw; k += 256) {
        const unsigned s = (head + 4 * k) >> 2;
        dw[k] = sh ? (w[s] >> sh) | (w[s + 1] << (32 - sh)) : w[s];      // w[s + 1] holds byte head + 4 k + 3 < sz: inside the slot
    }
    const unsigned tail = head + 4 * nw;
    if (tail + t < sz) d[tail + t] = (unsigned char)slot_byte(w, tail + t);
}

// (members, blocks per full member, blocks in all) of n payload bytes; the empty payload is one member of one empty block
void deflate_shape(size_t n, size_t member_bytes, size_t* nmem, size_t* bpm, size_t* nblocks) {
    *bpm = (member_bytes + DFL_BLK - 1) / DFL_BLK;
    if (n == 0) {
        *nmem = *nblocks = 1;
        return;
    }
    *nmem = (n + member_bytes - 1) / member_bytes;
    const size_t last = n - (*nmem - 1) * member_bytes;
    *nblocks = (*nmem - 1) * *bpm + (last + DFL_BLK - 1) / DFL_BLK;
}

constexpr size_t DFL_MAX_N = (size_t)1 << 40;
constexpr size_t DFL_MAX_MEMBER = (size_t)1 << 30;

// The three kernels over `nblocks` blocks of `nmem` members -- or pairs, where pair_first (host, nmem + 1: the first block of every
// pair), pair_member and pair_label (host, nmem) are given -- and the download of the offset and CRC tables.  Arguments are checked.
int deflate_run(boa_ctx* c, const uint8_t* dev_src, size_t n, size_t member_bytes, size_t nmem, size_t bpm, size_t nblocks, int row_bytes,
                int near_bytes, bool dyn, const unsigned* pair_first, const uint32_t* pair_member, const uint8_t* pair_label,
                uint8_t* dev_out, size_t* host_offsets, uint32_t* host_crc32) {
    const bool pairs = pair_first != nullptr;
    const int row = (row_bytes >= 1 && row_bytes <= DFL_MAXROW) ? row_bytes : 0;      // anything else: no row candidate
    const int hist = std::max(16, (row + 15) & ~15);
    const size_t lds = (size_t)OFF_DATA + hist + DFL_BLK + 16;

    // workspace: [slots][block offsets u64][member offsets u64][block sizes][block CRCs][member CRCs][x^(8 2^k) table]
    //            [first block of every pair][member of every pair][label of every pair]
    const size_t slots_b = nblocks * (size_t)DFL_SLOT;
    const size_t boff_b = nblocks * 8, moff_b = (nmem + 1) * 8, bsz_b = nblocks * 4, bcrc_b = nblocks * 4, mcrc_b = nmem * 4;
    const size_t pfirst_b = pairs ? (nmem + 1) * 4 : 0, pmem_b = pairs ? nmem * 4 : 0, plab_b = pairs ? nmem : 0;
    const size_t fixed_b = slots_b + boff_b + moff_b + bsz_b + bcrc_b + mcrc_b + sizeof(DflCrcPow);
    unsigned char* blk = nullptr;
    BOA_TRY(boa_malloc(c, fixed_b + pfirst_b + pmem_b + plab_b, (void**)&blk));
    unsigned* d_slots = (unsigned*)blk;
    unsigned long long* d_boff = (unsigned long long*)(blk + slots_b);
    unsigned long long* d_moff = (unsigned long long*)(blk + slots_b + boff_b);
    unsigned* d_bsz = (unsigned*)(blk + slots_b + boff_b + moff_b);
    unsigned* d_bcrc = (unsigned*)(blk + slots_b + boff_b + moff_b + bsz_b);
    unsigned* d_mcrc = (unsigned*)(blk + slots_b + boff_b + moff_b + bsz_b + bcrc_b);
    unsigned* d_pw = (unsigned*)(blk + slots_b + boff_b + moff_b + bsz_b + bcrc_b + mcrc_b);
    DflPairs pr = {nullptr, nullptr, nullptr, 0};
    if (pairs) pr = {(const unsigned*)(blk + fixed_b), (const unsigned*)(blk + fixed_b + pfirst_b), blk + fixed_b + pfirst_b + pmem_b, (unsigned)nmem};

    static bool once = (hipFuncSetAttribute((const void*)k_deflate_block<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                        hipFuncSetAttribute((const void*)k_deflate_block<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                        hipFuncSetAttribute((const void*)k_deflate_block<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                        hipFuncSetAttribute((const void*)k_deflate_block<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), true);
    (void)once;
    std::vector<unsigned long long> offs(nmem + 1);
    hipError_t e = hipMemcpyAsync(d_pw, crc_pow().x, sizeof(DflCrcPow), hipMemcpyHostToDevice, c->stream);
    if (pairs) {
        if (e == hipSuccess) e = hipMemcpyAsync((void*)pr.first, pair_first, pfirst_b, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync((void*)pr.member, pair_member, pmem_b, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync((void*)pr.label, pair_label, plab_b, hipMemcpyHostToDevice, c->stream);
    }
    if (e != hipSuccess) {
        hipStreamSynchronize(c->stream);
        boa_free(c, blk);
        BOA_HIP_TRY(e);
    }
    c->prof_break = true;
    KernelTimer t(c, BOA_K_OTHER, 0, (double)(pairs ? nblocks * (size_t)DFL_BLK : n) * 2 + (double)nblocks * 16);
    const dim3 grid((unsigned)nblocks), wg(DFL_NT);
    const unsigned mb = (unsigned)member_bytes, ubpm = (unsigned)bpm;
    if (pairs && dyn)
        hipLaunchKernelGGL((k_deflate_block<true, true>), grid, wg, lds, c->stream, dev_src, n, mb, ubpm, row, hist, near_bytes, d_pw, d_slots, d_bsz, d_bcrc, pr);
    else if (pairs)
        hipLaunchKernelGGL((k_deflate_block<false, true>), grid, wg, lds, c->stream, dev_src, n, mb, ubpm, row, hist, near_bytes, d_pw, d_slots, d_bsz, d_bcrc, pr);
    else if (dyn)
        hipLaunchKernelGGL((k_deflate_block<true, false>), grid, wg, lds, c->stream, dev_src, n, mb, ubpm, row, hist, near_bytes, d_pw, d_slots, d_bsz, d_bcrc, pr);
    else
        hipLaunchKernelGGL((k_deflate_block<false, false>), grid, wg, lds, c->stream, dev_src, n, mb, ubpm, row, hist, near_bytes, d_pw, d_slots, d_bsz, d_bcrc, pr);
    hipLaunchKernelGGL(k_deflate_scan, dim3(1), dim3(DFL_NT), 0, c->stream, d_bsz, d_bcrc, (unsigned)nblocks, ubpm, (unsigned)nmem, n, mb, d_pw,
                       d_boff, d_moff, d_mcrc, pr);
    hipLaunchKernelGGL(k_deflate_compact, grid, dim3(256), 0, c->stream, d_slots, d_bsz, d_boff, dev_out);
    t.stop();
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(offs.data(), d_moff, moff_b, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(host_crc32, d_mcrc, mcrc_b, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    boa_free(c, blk);
    BOA_HIP_TRY(e);
    for (size_t m = 0; m <= nmem; ++m) host_offsets[m] = (size_t)offs[m];
    return BOA_OK;
}

}  // namespace

extern "C" size_t boa_deflate_bound(size_t n, size_t member_bytes) {
    if (member_bytes < 1 || member_bytes > DFL_MAX_MEMBER || n > DFL_MAX_N) return 0;
    size_t nmem, bpm, nblocks;
    deflate_shape(n, member_bytes, &nmem, &bpm, &nblocks);
    return n + 5 * nblocks;      // every block as a stored block: 5 bytes of header each
}

extern "C" int boa_deflate_members2(boa_ctx* c, const uint8_t* dev_src, size_t n, size_t member_bytes, int row_bytes, int near_bytes, int flags,
                                    uint8_t* dev_out, size_t out_capacity, size_t* host_offsets, uint32_t* host_crc32) {
    BOA_REQUIRE(c && dev_out && host_offsets && host_crc32 && (dev_src || n == 0), "boa_deflate_members: NULL argument");
    BOA_REQUIRE(member_bytes >= 1 && member_bytes <= DFL_MAX_MEMBER, "boa_deflate_members: member_bytes %zu outside [1, 2^30]", member_bytes);
    BOA_REQUIRE(n <= DFL_MAX_N, "boa_deflate_members: %zu payload bytes (at most 2^40)", n);
    BOA_REQUIRE(near_bytes >= 1 && near_bytes <= 16, "boa_deflate_members: near_bytes %d outside [1, 16]", near_bytes);
    BOA_REQUIRE((flags & ~BOA_DEFLATE_DYNAMIC) == 0, "boa_deflate_members: unknown flags 0x%x", (unsigned)flags);
    const bool dyn = (flags & BOA_DEFLATE_DYNAMIC) != 0;
    BOA_REQUIRE(dyn || near_bytes == 1, "boa_deflate_members: near_bytes %d without BOA_DEFLATE_DYNAMIC (the fixed-code kernel has distance 1)", near_bytes);
    size_t nmem, bpm, nblocks;
    deflate_shape(n, member_bytes, &nmem, &bpm, &nblocks);
    BOA_REQUIRE(nblocks <= 0x7fffffffu && nmem <= 0x7fffffffu, "boa_deflate_members: %zu blocks in %zu members", nblocks, nmem);
    const size_t bound = n + 5 * nblocks;
    BOA_REQUIRE(out_capacity >= bound, "boa_deflate_members: out_capacity %zu below boa_deflate_bound = %zu", out_capacity, bound);
    return deflate_run(c, dev_src, n, member_bytes, nmem, bpm, nblocks, row_bytes, near_bytes, dyn, nullptr, nullptr, nullptr, dev_out, host_offsets,
                       host_crc32);
}

extern "C" int boa_deflate_members(boa_ctx* c, const uint8_t* dev_src, size_t n, size_t member_bytes, int row_bytes, uint8_t* dev_out,
                                   size_t out_capacity, size_t* host_offsets, uint32_t* host_crc32) {
    return boa_deflate_members2(c, dev_src, n, member_bytes, row_bytes, 1, 0, dev_out, out_capacity, host_offsets, host_crc32);
}

extern "C" int boa_deflate_label_pairs(boa_ctx* c, const uint8_t* dev_labels, size_t n, size_t member_bytes, int row_bytes, int flags,
                                       const uint8_t* host_pair_label, const uint32_t* host_pair_member, int n_pairs, uint8_t* dev_out,
                                       size_t out_capacity, size_t* host_offsets, uint32_t* host_crc32) {
    BOA_REQUIRE(c && host_offsets && (dev_labels || n == 0), "boa_deflate_label_pairs: NULL argument");
    BOA_REQUIRE(n_pairs >= 0, "boa_deflate_label_pairs: n_pairs %d", n_pairs);
    BOA_REQUIRE(n_pairs == 0 || (dev_out && host_crc32 && host_pair_label && host_pair_member), "boa_deflate_label_pairs: NULL argument");
    BOA_REQUIRE(member_bytes >= 1 && member_bytes <= DFL_MAX_MEMBER, "boa_deflate_label_pairs: member_bytes %zu outside [1, 2^30]", member_bytes);
    BOA_REQUIRE(n <= DFL_MAX_N, "boa_deflate_label_pairs: %zu payload bytes (at most 2^40)", n);
    BOA_REQUIRE((flags & ~BOA_DEFLATE_DYNAMIC) == 0, "boa_deflate_label_pairs: unknown flags 0x%x", (unsigned)flags);
    size_t nmem, bpm, all_blocks;
    deflate_shape(n, member_bytes, &nmem, &bpm, &all_blocks);
    const size_t last_len = n - (nmem - 1) * member_bytes;                         // (0 only for the empty payload)
    const size_t last_blocks = std::max<size_t>(1, (last_len + DFL_BLK - 1) / DFL_BLK);
    std::vector<unsigned> first((size_t)n_pairs + 1);
    size_t nblocks = 0, bound = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const size_t m = host_pair_member[p];
        BOA_REQUIRE(m < nmem, "boa_deflate_label_pairs: pair %d names member %zu of %zu", p, m, nmem);
        first[p] = (unsigned)nblocks;
        const size_t nb = m + 1 < nmem ? bpm : last_blocks;
        nblocks += nb;
        bound += (m + 1 < nmem ? member_bytes : last_len) + 5 * nb;                // every block stored
        BOA_REQUIRE(nblocks <= 0x7fffffffu, "boa_deflate_label_pairs: more than 2^31 - 1 blocks in %d pairs", n_pairs);
    }
    first[n_pairs] = (unsigned)nblocks;
    BOA_REQUIRE(out_capacity >= bound, "boa_deflate_label_pairs: out_capacity %zu below the pairs' bound = %zu", out_capacity, bound);
    if (n_pairs == 0) {
        host_offsets[0] = 0;
        return BOA_OK;
    }
    return deflate_run(c, dev_labels, n, member_bytes, (size_t)n_pairs, bpm, nblocks, row_bytes, 1, (flags & BOA_DEFLATE_DYNAMIC) != 0, first.data(),
                       host_pair_member, host_pair_label, dev_out, host_offsets, host_crc32);
}
