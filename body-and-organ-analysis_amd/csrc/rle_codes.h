// The index logic of the device RLE Lossless decoder (rle.hip; DICOM PS3.5 Annex G = byte-plane PackBits): the control step, the
// entry map of a chunk of a segment, the walk over a segment's chain of chunks, the marking of a chunk's live runs and the lookup
// of the run that covers an output byte.  Plain C++: the kernels call these functions with (lane, lanes of the workgroup),
// tools/rle_codes_host.cpp calls them with (0, 1) on the host under the sanitizers.  The bytes are untrusted: every read is of a
// position below the bound the caller passes, every loop is bounded by the chunk size or by a table.
//
// A control byte c at position p: c < 128 copies the next c + 1 bytes, c > 128 repeats the next byte 257 - c times, c == 128 does
// nothing.  A control whose operand bytes are not all inside the segment produces nothing and ends the decode.  A step advances p
// by 1 .. 129 bytes, so a chunk of chunk_bytes >= 129 can be entered at the offsets 0 .. 128 only, and is left at the offsets
// 0 .. 128 of the next one: the chain is resolved exactly from the 129 answers of every chunk.
#pragma once
#include <stdint.h>

#if !defined(BOA_HD)
#if defined(__HIPCC__)
#define BOA_HD __host__ __device__ __forceinline__
#else
#define BOA_HD inline
#endif
#endif

#define RLE_MAX_STEP 129u        // the largest advance of one control (c = 127: the control and 128 literals)
#define RLE_ENTRIES 129u         // entry offsets 0 .. 128 of a chunk
#define RLE_CHUNK_MIN 256u       // chunk_bytes: a power of two in RLE_CHUNK_MIN .. RLE_CHUNK_MAX
#define RLE_CHUNK_MAX 4096u
#define RLE_NOT_LIVE 0xffffffffu

// A node word: the position reached (low 13 bits: at most chunk_bytes + 129 < 8192) and the bytes produced on the way (high 19
// bits: at most 128 per two bytes of the chunk, 64 chunk_bytes <= 2^18).  The nodes of a chunk are its positions 0 .. chunk_bytes +
// 128 (those at or beyond the chunk's length are fixed points that produce nothing) and one more, `dead`, where a control whose
// operands overrun the segment leads: also a fixed point.
#define RLE_POS_BITS 13
#define RLE_POS_MASK 0x1fffu
BOA_HD uint32_t rle_word(uint32_t pos, uint32_t count) { return pos | (count << RLE_POS_BITS); }
BOA_HD uint32_t rle_pos(uint32_t w) { return w & RLE_POS_MASK; }
BOA_HD uint32_t rle_count(uint32_t w) { return w >> RLE_POS_BITS; }
BOA_HD uint32_t rle_nodes(uint32_t chunk_bytes) { return chunk_bytes + RLE_ENTRIES + 1; }
BOA_HD int rle_rounds(uint32_t chunk_bytes) {      // log2: 2^rounds steps of at least one byte each leave the chunk
    int r = 0;
    while ((1u << r) < chunk_bytes) ++r;
    return r;
}

// A table word (one per entry offset of a chunk): bytes produced (low 20 bits), exit offset into the next chunk (bits 20 .. 27),
// RLE_T_DEAD: the decode ended inside the chunk at a control whose operands overrun the segment.
#define RLE_T_COUNT_MASK 0xfffffu
#define RLE_T_EXIT_SHIFT 20
#define RLE_T_DEAD 0x80000000u

// the control step: bytes consumed (the control and its operands) and bytes produced
BOA_HD void rle_step(uint32_t c, uint32_t* advance, uint32_t* produced) {
    if (c < 128u) {
        *advance = c + 2u;
        *produced = c + 1u;
    } else if (c > 128u) {
        *advance = 2u;
        *produced = 257u - c;
    } else {
        *advance = 1u;
        *produced = 0u;
    }
}

// Node p of a chunk after one step.  chunk: the chunk's first byte; rest: the bytes from there to the segment's end (only
// chunk[0 .. min(rest, len)) is read); len: the chunk's length = min(chunk_bytes, rest); dead: the index of the dead node.
BOA_HD uint32_t rle_node(const uint8_t* chunk, uint32_t rest, uint32_t len, uint32_t dead, uint32_t p) {
    if (p >= len) return rle_word(p, 0u);
    uint32_t adv, out;
    rle_step(chunk[p], &adv, &out);
    if (p + adv > rest) return rle_word(dead, 0u);
    return rle_word(p + adv, out);
}

// One round of pointer doubling over the n nodes: dst[i] = src[i] followed by src at the node it reaches.  Lane `lane` of
// `lanes`; the caller separates the rounds (a barrier on the device) and swaps src and dst.
BOA_HD void rle_double_round(const uint32_t* src, uint32_t* dst, uint32_t n, uint32_t lane, uint32_t lanes) {
    for (uint32_t i = lane; i < n; i += lanes) {
        const uint32_t a = src[i], b = src[rle_pos(a)];
        dst[i] = rle_word(rle_pos(b), rle_count(a) + rle_count(b));
    }
}

// the table word of an entry offset from its node after rle_rounds(chunk_bytes) rounds
BOA_HD uint32_t rle_table_word(uint32_t w, uint32_t len, uint32_t dead) {
    const uint32_t pos = rle_pos(w);
    if (pos == dead) return RLE_T_DEAD | rle_count(w);
    return rle_count(w) | ((pos - len) << RLE_T_EXIT_SHIFT);
}

// The entry map of chunk k of a segment, on one lane (the host's form of k_rle_chunk_map): table[RLE_ENTRIES].  a, b: two buffers
// of rle_nodes(chunk_bytes) words.
BOA_HD void rle_entry_map(const uint8_t* seg, uint32_t seg_len, uint32_t k, uint32_t chunk_bytes, uint32_t* a, uint32_t* b,
                          uint32_t* table) {
    const uint32_t n = rle_nodes(chunk_bytes), start = k * chunk_bytes, rest = seg_len - start;
    const uint32_t len = rest < chunk_bytes ? rest : chunk_bytes;
    for (uint32_t i = 0; i < n; ++i) a[i] = rle_node(seg + start, rest, len, n - 1u, i);
    for (int r = rle_rounds(chunk_bytes); r > 0; --r) {
        rle_double_round(a, b, n, 0u, 1u);
        uint32_t* t = a;
        a = b;
        b = t;
    }
    for (uint32_t e = 0; e < RLE_ENTRIES; ++e) table[e] = rle_table_word(a[e], len, n - 1u);
}

// The walk over a segment's chain of chunks from entry 0 of its first: per chunk the entry offset (RLE_NOT_LIVE for the chunks
// behind the one where `wanted` bytes are reached or the decode ended) and the output offset of its first byte.  Returns the bytes
// produced, counted up to the chunk that reaches `wanted`: less than `wanted` = the segment is truncated.
BOA_HD uint64_t rle_chain(const uint32_t* table, uint32_t n_chunks, uint32_t wanted, uint32_t* entry, uint32_t* base) {
    uint64_t total = 0;
    uint32_t e = 0;
    bool live = true;
    for (uint32_t k = 0; k < n_chunks; ++k) {
        live = live && total < wanted;
        entry[k] = live ? e : RLE_NOT_LIVE;
        base[k] = live ? (uint32_t)total : 0u;
        if (!live) continue;
        const uint32_t t = table[(uint64_t)k * RLE_ENTRIES + e];
        total += t & RLE_T_COUNT_MASK;
        if (t & RLE_T_DEAD) live = false;
        e = (t >> RLE_T_EXIT_SHIFT) & 0xffu;
    }
    return total;
}

// One round of marking the nodes on the chain from a chunk's entry, run BEFORE the rle_double_round of the same words: with the
// words holding jumps of 2^r steps and the nodes at less than 2^r steps from the entry marked, it marks those at less than 2^(r+1).
// mark[i] = the bytes produced between the entry and node i, RLE_NOT_LIVE off the chain.  Every value written to a node is that
// node's one offset, so the order in which lanes read and write within a round does not change the result.
BOA_HD void rle_mark_round(const uint32_t* words, uint32_t* mark, uint32_t n, uint32_t lane, uint32_t lanes) {
    for (uint32_t i = lane; i < n; i += lanes) {
        const uint32_t m = mark[i];
        if (m == RLE_NOT_LIVE) continue;
        const uint32_t w = words[i];
        mark[rle_pos(w)] = m + rle_count(w);
    }
}

// Position p of a chunk starts a run of the chunk's output: it is on the chain, inside the chunk, and its control produces bytes.
// Returns the run word (position, offset of its first byte in the chunk's output) or RLE_NOT_LIVE.
BOA_HD uint32_t rle_run_at(const uint8_t* chunk, uint32_t rest, uint32_t len, uint32_t dead, const uint32_t* mark, uint32_t p) {
    if (p >= len || mark[p] == RLE_NOT_LIVE) return RLE_NOT_LIVE;
    const uint32_t w = rle_node(chunk, rest, len, dead, p);
    if (rle_pos(w) == dead || rle_count(w) == 0u) return RLE_NOT_LIVE;
    return rle_word(p, mark[p]);
}

// the run that covers output byte o of the chunk: the last of the n_runs >= 1 run words (ascending) whose offset is <= o
BOA_HD uint32_t rle_find_run(const uint32_t* runs, uint32_t n_runs, uint32_t o) {
    uint32_t lo = 0, hi = n_runs;              // runs[lo] <= o < runs[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rle_count(runs[mid]) <= o) lo = mid;
        else hi = mid;
    }
    return runs[lo];
}

// output byte o of the chunk, which `run` covers
BOA_HD uint8_t rle_run_byte(const uint8_t* chunk, uint32_t run, uint32_t o) {
    const uint32_t p = rle_pos(run);
    return chunk[p] < 128u ? chunk[p + 1u + (o - rle_count(run))] : chunk[p + 1u];
}

// the plain loop over a segment: up to `wanted` bytes into out; returns the bytes produced (a run that crosses `wanted` is clipped)
BOA_HD uint32_t rle_decode_serial(const uint8_t* seg, uint32_t seg_len, uint8_t* out, uint32_t wanted) {
    uint32_t p = 0, n = 0;
    while (n < wanted && p < seg_len) {
        uint32_t adv, cnt;
        const uint32_t c = seg[p];
        rle_step(c, &adv, &cnt);
        if (p + adv > seg_len) break;
        if (cnt > wanted - n) cnt = wanted - n;
        for (uint32_t i = 0; i < cnt; ++i) out[n + i] = c < 128u ? seg[p + 1u + i] : seg[p + 1u];
        n += cnt;
        p += adv;
    }
    return n;
}
