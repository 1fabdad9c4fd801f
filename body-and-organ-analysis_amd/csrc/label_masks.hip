// Which labels occur in which gzip member of a label volume (boa_label_member_presence): the table that lets the per-structure mask
// writer (boa_deflate_label_pairs, deflate.hip) encode only the (label, member) pairs that hold a voxel.
//   k_label_presence   one pass over the volume with 16-byte loads.  A workgroup owns PRS_CHUNK consecutive bytes; where they lie in
//                      at most PRS_ROWS members it ORs into 256-bit rows in LDS and flushes them once, else (members of a few bytes)
//                      every lane ORs straight into the table.  Labels are spatially coherent: a lane whose 16 bytes are the label
//                      it recorded last, in the same member, does nothing.
// The table is zeroed first and only ever ORed into, so the result does not depend on the order of the workgroups.
#include "common.h"

namespace {

constexpr int PRS_NT = 256;                            // threads per workgroup
constexpr int PRS_ITER = 8;                            // 16-byte vectors per thread
constexpr int PRS_CHUNK = PRS_NT * PRS_ITER * 16;      // bytes per workgroup (32 KiB)
constexpr int PRS_ROWS = 16;                           // member rows a workgroup keeps in LDS
constexpr size_t PRS_MAX_N = (size_t)1 << 40;
constexpr size_t PRS_MAX_MEMBER = (size_t)1 << 30;

// Positions are counted from the 16-byte boundary at or below src (`shift` bytes before it), so that every vector load is aligned
// whatever the pointer: the volume is v in [shift, shift + n), chunk k is v in [k PRS_CHUNK, (k + 1) PRS_CHUNK).
__global__ __launch_bounds__(PRS_NT) void k_label_presence(const unsigned char* __restrict__ src, size_t n, unsigned member_bytes, unsigned shift,
                                                           unsigned* __restrict__ bits) {
    __shared__ unsigned s_bits[PRS_ROWS * 8];
    const int t = threadIdx.x;
    const unsigned char* base = src - shift;
    const size_t v_lo = (size_t)blockIdx.x * PRS_CHUNK, v_end = (size_t)shift + n;
    const size_t c_lo = v_lo > shift ? v_lo : (size_t)shift;                          // the chunk's part of the volume, [c_lo, c_hi)
    const size_t c_hi = v_lo + PRS_CHUNK < v_end ? v_lo + PRS_CHUNK : v_end;
    if (c_lo >= c_hi) return;                                                         // (whole workgroup)
    const size_t m_first = (c_lo - shift) / member_bytes;
    const unsigned nrows = (unsigned)((c_hi - 1 - shift) / member_bytes - m_first) + 1;
    const bool in_lds = nrows <= (unsigned)PRS_ROWS;
    // byte offset of position v_lo from the start of member m_first; negative only in chunk 0 (before the volume), never used there
    const long long rel0 = (long long)v_lo - (long long)shift - (long long)(m_first * (size_t)member_bytes);
    if (in_lds) {
        if (t < PRS_ROWS * 8) s_bits[t] = 0;
        __syncthreads();
    }
    unsigned* rows = bits + m_first * 8;

    unsigned last = 0xffffffffu;                                                      // row << 8 | label recorded last
    auto record = [&](unsigned row, unsigned label) {
        const unsigned key = row << 8 | label;
        if (key == last) return;
        last = key;
        atomicOr(in_lds ? &s_bits[row * 8 + (label >> 5)] : &rows[(size_t)row * 8 + (label >> 5)], 1u << (label & 31));
    };
    // the member row (from m_first) of the byte at chunk offset o; o + rel0 < member_bytes + PRS_CHUNK fits 32 bits
    auto row_of = [&](unsigned o) { return nrows == 1 ? 0u : (unsigned)(o + rel0) / member_bytes; };

#pragma unroll 2
    for (int it = 0; it < PRS_ITER; ++it) {
        const unsigned o = (unsigned)(it * PRS_NT + t) * 16;                          // chunk offset of this lane's vector
        const size_t v = v_lo + o;
        if (v >= c_lo && v + 16 <= c_hi) {
            const uint4 q = *(const uint4*)(base + v);
            const unsigned r0 = row_of(o), r1 = row_of(o + 15);
            const unsigned rep = (q.x & 0xffu) * 0x01010101u;
            if (r0 == r1 && q.x == rep && q.y == rep && q.z == rep && q.w == rep) {
                record(r0, q.x & 0xffu);
                continue;
            }
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) record(r0 == r1 ? r0 : row_of(o + j), (w[j >> 2] >> (8 * (j & 3))) & 0xffu);
        } else {
            for (int j = 0; j < 16; ++j)                                              // the ragged ends of the volume
                if (v + j >= c_lo && v + j < c_hi) record(row_of(o + j), base[v + j]);
        }
    }
    if (in_lds) {
        __syncthreads();
        if (t < (int)nrows * 8 && s_bits[t]) atomicOr(&rows[t], s_bits[t]);            // (neighbouring workgroups share a member's row)
    }
}

}  // namespace

extern "C" int boa_label_member_presence(boa_ctx* c, const uint8_t* dev_labels, size_t n, size_t member_bytes, uint32_t* host_bits) {
    BOA_REQUIRE(c && host_bits && (dev_labels || n == 0), "boa_label_member_presence: NULL argument");
    BOA_REQUIRE(member_bytes >= 1 && member_bytes <= PRS_MAX_MEMBER, "boa_label_member_presence: member_bytes %zu outside [1, 2^30]", member_bytes);
    BOA_REQUIRE(n <= PRS_MAX_N, "boa_label_member_presence: %zu bytes (at most 2^40)", n);
    const size_t nmem = n == 0 ? 1 : (n + member_bytes - 1) / member_bytes;
    BOA_REQUIRE(nmem <= 0x7fffffffu, "boa_label_member_presence: %zu members", nmem);
    if (n == 0) {
        for (int k = 0; k < 8; ++k) host_bits[k] = 0;
        return BOA_OK;
    }
    unsigned* d_bits = nullptr;
    BOA_TRY(boa_malloc(c, nmem * 32, (void**)&d_bits));
    const unsigned shift = (unsigned)((uintptr_t)dev_labels & 15);
    const size_t chunks = (shift + n + PRS_CHUNK - 1) / PRS_CHUNK;                    // <= 2^25 + 1
    hipError_t e = hipMemsetAsync(d_bits, 0, nmem * 32, c->stream);
    if (e == hipSuccess) {
        c->prof_break = true;
        KernelTimer t(c, BOA_K_OTHER, 0, (double)n);
        hipLaunchKernelGGL(k_label_presence, dim3((unsigned)chunks), dim3(PRS_NT), 0, c->stream, dev_labels, n, (unsigned)member_bytes, shift, d_bits);
        t.stop();
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host_bits, d_bits, nmem * 32, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    boa_free(c, d_bits);
    BOA_HIP_TRY(e);
    return BOA_OK;
}
