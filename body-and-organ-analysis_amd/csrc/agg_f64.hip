// Voxel statistics of CT values held as float64 (what `get_fdata()` returns for float-valued, scaled or out-of-int16-range CTs):
// per-group exact order statistics by radix select, count / sum / centred sum of squares.  (The float form of the tissue pass is an
// instantiation of k_tissue_aggregate, agg.hip.)
// The int16 path (agg.hip) reads order statistics off a (label, HU) histogram; doubles have no such histogram.
#include <string.h>

#include <algorithm>

#include "common.h"

// ------------------------------------------------------------------------------------------------------
// Radix select.  A double is mapped to a 64-bit key whose unsigned order is the order of the values (sign bit flipped for
// non-negative values, all bits flipped for negative ones; -0.0 sorts directly below +0.0, which `==` cannot tell apart).  The key is
// consumed in eight 8-bit digits from the top.  Per group, GS_SLOTS ranks are resolved together: rank 0 (min), floor and ceil of
// (count-1)*q for q = 1/4, 1/2, 3/4, and rank count-1 (max).  Pass p counts, for every (group, slot), the voxels whose key agrees
// with the slot's prefix (the p digits found so far) by their next digit; a one-block-per-group step then walks the 256 counts to
// the digit that holds the slot's rank.  Of the slots that still share a prefix only the first (the "leader") is counted, the
// others read its row -- leaders have distinct prefixes, so a voxel matches at most one: one table entry per voxel and pass.
// Each pass reads 9 B per voxel; pass 0 also sums the values, pass 1 the squared deviations from the mean.
//
// The table of a pass is (group, slot, digit) = up to 256 x 8 x 256 counters: too large for LDS as a dense array, and sparse in
// practice (the top digits of a CT take a handful of values; in later passes few voxels match a prefix at all).  As in
// k_label_hist (agg.hip) each workgroup counts into an open-addressing hash table in LDS and sends one device-scope atomic per
// DISTINCT key to the global table when its table fills up and at the end; waves whose voxels all carry one key (air around
// the patient: 30 % of a CT at one value) issue a single LDS atomic, runs of equal keys inside a lane are merged first.
#define GS_SLOTS 8
#define GS_SENT 0xFFFFFFFFFFFFFFFFull   // prefix that no voxel matches (prefixes of passes 1..7 have at most 56 bits)
#define GS_NONE 0xFFFFFFFFu             // key of a voxel that is not counted; also the empty mark of the LDS table
#define GS_LOG2 12
#define GS_TAB (1 << GS_LOG2)
#define GS_FLUSH (GS_TAB * 2 / 3)
#define GS_HT 512

__device__ __forceinline__ unsigned long long f64_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double f64_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double((long long)b);
}

struct Lut256F {
    unsigned char v[256];
};

// MODE 0: first digit of every voxel of a group (no prefix yet), acc[g] += v
// MODE 1: prefix-restricted count,                               acc[g] += (v - mean[g])^2
// MODE 2: prefix-restricted count only
template <int VEC, int MODE>
__global__ __launch_bounds__(GS_HT) void k_group_select(const double* __restrict__ ct, const unsigned char* __restrict__ labels, size_t n,
                                                        Lut256F lut, int shift, const unsigned long long* __restrict__ lpref,
                                                        const double* __restrict__ mean, unsigned int* __restrict__ tab,
                                                        double* __restrict__ acc, size_t vec_per_block) {
    __shared__ unsigned int keys[GS_TAB];
    __shared__ unsigned int cnts[GS_TAB];
    __shared__ unsigned long long s_pref[MODE == 0 ? 1 : 256 * GS_SLOTS];
    __shared__ double s_acc[MODE == 2 ? 1 : 256];
    __shared__ double s_mean[MODE == 1 ? 256 : 1];
    __shared__ unsigned char s_lut[256];
    __shared__ int nkeys;
    const int tid = threadIdx.x;
    for (int i = tid; i < GS_TAB; i += GS_HT) {
        keys[i] = GS_NONE;
        cnts[i] = 0u;
    }
    if (tid < 256) {
        s_lut[tid] = lut.v[tid];
        if (MODE != 2) s_acc[tid] = 0.0;
        if (MODE == 1) s_mean[tid] = mean[tid];
    }
    if (MODE != 0)
        for (int i = tid; i < 256 * GS_SLOTS; i += GS_HT) s_pref[i] = lpref[i];
    if (tid == 0) nkeys = 0;
    __syncthreads();

    auto key_of = [&](double v, unsigned g) -> unsigned {   // g < 256
        const unsigned long long k = f64_key(v);
        if (MODE == 0) return (g << 11) | (unsigned)(k >> 56);
        const unsigned long long pfx = k >> (shift + 8);
        int slot = -1;
#pragma unroll
        for (int s = 0; s < GS_SLOTS; ++s) slot = (s_pref[g * GS_SLOTS + s] == pfx) ? s : slot;   // leaders have distinct prefixes
        return slot < 0 ? GS_NONE : ((g << 11) | ((unsigned)slot << 8) | (unsigned)((k >> shift) & 0xFFu));
    };
    auto term = [&](double v, unsigned g) -> double {
        if (MODE == 0) return v;
        const double d = v - s_mean[g];
        return d * d;
    };
    auto count = [&](unsigned key, unsigned c) {
        unsigned h = (key * 2654435761u) >> (32 - GS_LOG2);
#pragma unroll 1
        for (int probe = 0; probe < 16; ++probe, h = (h + 1) & (GS_TAB - 1)) {
            unsigned k = keys[h];
            if (k == GS_NONE) {
                k = atomicCAS(&keys[h], GS_NONE, key);
                if (k == GS_NONE) {
                    atomicAdd(&nkeys, 1);
                    k = key;
                }
            }
            if (k == key) {
                atomicAdd(&cnts[h], c);
                return;
            }
        }
        atomicAdd(&tab[key], c);   // a long probe chain: straight to the global table
    };
    auto flush = [&]() {  // whole workgroup
        for (int i = tid; i < GS_TAB; i += GS_HT) {
            const unsigned k = keys[i];
            if (k != GS_NONE) {
                atomicAdd(&tab[k], cnts[i]);
                keys[i] = GS_NONE;
                cnts[i] = 0u;
            }
        }
        __syncthreads();
        if (tid == 0) nkeys = 0;
        __syncthreads();
    };

    const size_t nvec = n / VEC;
    const size_t v_begin = (size_t)blockIdx.x * vec_per_block;
    const size_t v_end = v_begin + vec_per_block < nvec ? v_begin + vec_per_block : nvec;
    for (size_t base = v_begin; base < v_end; base += GS_HT) {   // (same trip count in every thread: the loop holds barriers)
        const size_t i = base + tid;
        const bool live = i < v_end;
        unsigned key[VEC], grp[VEC];
        double val[VEC];
        if (live) {
            unsigned char lb[VEC] __attribute__((aligned(8)));
            if (VEC == 8) {
                *(uint2*)lb = *(const uint2*)(labels + i * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) *(double2*)(val + 2 * j) = *(const double2*)(ct + i * 8 + 2 * j);
            } else {
                lb[0] = labels[i];
                val[0] = ct[i];
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                grp[j] = s_lut[lb[j]];
                key[j] = grp[j] == 0xFFu ? GS_NONE : key_of(val[j], grp[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                grp[j] = 0xFFu;
                key[j] = GS_NONE;
                val[j] = 0.0;
            }
        }
        // ---- counts: a wave on one key issues one LDS atomic (or none); otherwise one per run of equal keys in a lane
        {
            bool uni = true;
#pragma unroll
            for (int j = 1; j < VEC; ++j) uni = uni && key[j] == key[0];
            const unsigned k0 = __builtin_amdgcn_readfirstlane(key[0]);
            if (__builtin_amdgcn_ballot_w64(!(uni && key[0] == k0)) == 0) {
                if (k0 != GS_NONE && (tid & 63) == 0) count(k0, (unsigned)VEC * 64u);
            } else {
                unsigned run = 1;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    if (j + 1 < VEC && key[j + 1] == key[j]) {
                        ++run;
                    } else {
                        if (key[j] != GS_NONE) count(key[j], run);
                        run = 1;
                    }
                }
            }
        }
        // ---- sums: a wave on one group reduces through shuffles to one LDS atomic; otherwise one per run of equal groups in a lane
        if (MODE != 2) {
            bool uni = true;
#pragma unroll
            for (int j = 1; j < VEC; ++j) uni = uni && grp[j] == grp[0];
            const unsigned g0 = __builtin_amdgcn_readfirstlane(grp[0]);
            if (__builtin_amdgcn_ballot_w64(!(uni && grp[0] == g0)) == 0) {
                if (g0 != 0xFFu) {
                    double s = 0.0;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) s += term(val[j], g0);
#pragma unroll
                    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
                    if ((tid & 63) == 0) atomicAdd(&s_acc[g0], s);
                }
            } else {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    if (grp[j] != 0xFFu) s += term(val[j], grp[j]);
                    if (j + 1 == VEC || grp[j + 1] != grp[j]) {
                        if (grp[j] != 0xFFu) atomicAdd(&s_acc[grp[j]], s);
                        s = 0.0;
                    }
                }
            }
        }
        // The flush decision must be the same in every wave (flush() holds barriers and empties slots): the first barrier ends this
        // iteration's inserts, so all threads latch the same nkeys; the second keeps the next iteration's inserts behind those reads.
        __syncthreads();
        const bool full = nkeys > GS_FLUSH;
        __syncthreads();
        if (full) flush();
    }
    // the n % VEC voxels at the end, one by one straight into the global tables
    if (blockIdx.x == 0 && tid < (int)(n - nvec * VEC)) {
        const size_t i = nvec * VEC + tid;
        const unsigned g = s_lut[labels[i]];
        if (g != 0xFFu) {
            const unsigned k = key_of(ct[i], g);
            if (k != GS_NONE) atomicAdd(&tab[k], 1u);
            if (MODE != 2) atomicAdd(&acc[g], term(ct[i], g));
        }
    }
    __syncthreads();
    flush();
    if (MODE != 2 && tid < 256 && s_acc[tid] != 0.0) atomicAdd(&acc[tid], s_acc[tid]);
}

// One block per group, after pass `pass`: the digit that holds every slot's rank extends the slot's prefix; the rank becomes
// the rank among the voxels of that digit; the group's rows are cleared for the next pass.  After pass 0 the row of slot 0 is
// the group's whole histogram of top digits: its total is the voxel count, from which the ranks and the mean follow.
__global__ __launch_bounds__(256) void k_group_select_step(int pass, unsigned int* __restrict__ tab, unsigned long long* __restrict__ pref,
                                                           unsigned long long* __restrict__ lpref, unsigned long long* __restrict__ rank,
                                                           unsigned long long* __restrict__ count, const double* __restrict__ sum,
                                                           double* __restrict__ mean, double* __restrict__ out) {
    __shared__ unsigned int rows[GS_SLOTS][256];
    __shared__ int lead[GS_SLOTS];
    __shared__ unsigned long long s_rank[GS_SLOTS], s_new[GS_SLOTS];
    __shared__ unsigned long long s_count;
    const int g = blockIdx.x, tid = threadIdx.x;
#pragma unroll
    for (int s = 0; s < GS_SLOTS; ++s) {
        unsigned int* p = tab + ((size_t)g * GS_SLOTS + s) * 256 + tid;
        rows[s][tid] = *p;
        *p = 0u;
    }
    __syncthreads();
    if (tid == 0) {
        if (pass == 0) {
            unsigned long long c = 0;
            for (int d = 0; d < 256; ++d) c += rows[0][d];
            count[g] = c;
            mean[g] = c ? sum[g] / (double)c : 0.0;
            const unsigned long long m = c ? c - 1 : 0;
            // floor / ceil of (count-1) * q for q = 1/4, 1/2, 3/4 in integers
            const unsigned long long r[GS_SLOTS] = {0, m / 4, (m + 3) / 4, m / 2, (m + 1) / 2, 3 * m / 4, (3 * m + 3) / 4, m};
            for (int s = 0; s < GS_SLOTS; ++s) {
                s_rank[s] = r[s];
                lead[s] = 0;
            }
            s_count = c;
        } else {
            for (int s = 0; s < GS_SLOTS; ++s) {
                s_rank[s] = rank[g * GS_SLOTS + s];
                lead[s] = s;      // the first slot with this prefix (ranks are not monotone in the slot index for small counts)
                for (int q = s - 1; q >= 0; --q)
                    if (pref[g * GS_SLOTS + q] == pref[g * GS_SLOTS + s]) lead[s] = q;
            }
            s_count = count[g];
        }
    }
    __syncthreads();
    if (tid < GS_SLOTS && s_count) {
        const unsigned int* row = rows[lead[tid]];
        const unsigned long long r = s_rank[tid];
        unsigned long long cum = 0;
        int d = 0;
        for (; d < 255; ++d) {
            if (r < cum + row[d]) break;
            cum += row[d];
        }
        s_new[tid] = (pass == 0 ? 0ull : (pref[g * GS_SLOTS + tid] << 8)) | (unsigned long long)d;
        rank[g * GS_SLOTS + tid] = r - cum;
    }
    __syncthreads();
    if (tid < GS_SLOTS) {
        const int i = g * GS_SLOTS + tid;
        if (s_count) {
            pref[i] = s_new[tid];
            bool first = true;
            for (int q = 0; q < tid; ++q) first = first && s_new[q] != s_new[tid];
            lpref[i] = first ? s_new[tid] : GS_SENT;
            if (pass == 7) out[i] = f64_unkey(s_new[tid]);
        } else {
            lpref[i] = GS_SENT;
            if (pass == 7) out[i] = 0.0;
        }
    }
}

template <int VEC>
static void group_select_pass(boa_ctx* c, int pass, unsigned grid, const double* ct, const uint8_t* labels, size_t n, const Lut256F& lut,
                              const unsigned long long* lpref, const double* mean, unsigned int* tab, double* sum, double* m2, size_t vpb) {
    const int shift = 56 - 8 * pass;
    if (pass == 0)
        hipLaunchKernelGGL((k_group_select<VEC, 0>), dim3(grid), dim3(GS_HT), 0, c->stream, ct, labels, n, lut, shift, lpref, mean, tab, sum, vpb);
    else if (pass == 1)
        hipLaunchKernelGGL((k_group_select<VEC, 1>), dim3(grid), dim3(GS_HT), 0, c->stream, ct, labels, n, lut, shift, lpref, mean, tab, m2, vpb);
    else
        hipLaunchKernelGGL((k_group_select<VEC, 2>), dim3(grid), dim3(GS_HT), 0, c->stream, ct, labels, n, lut, shift, lpref, mean, tab, m2, vpb);
}

extern "C" int boa_group_stats_f64(boa_ctx* c, const double* dev_ct, const uint8_t* dev_labels, size_t n, const uint8_t* host_lut,
                                   int n_groups, uint64_t* host_count, double* host_stats) {
    BOA_REQUIRE(c && host_lut && host_count && host_stats && (n == 0 || (dev_ct && dev_labels)), "boa_group_stats_f64: NULL argument");
    BOA_REQUIRE(n_groups >= 1 && n_groups <= 255, "boa_group_stats_f64: %d groups (1..255)", n_groups);
    BOA_REQUIRE(n < (1ull << 32), "boa_group_stats_f64: %zu voxels (the counters hold 32 bits)", n);
    Lut256F lut;
    memcpy(lut.v, host_lut, 256);
    for (int i = 0; i < 256; ++i)
        BOA_REQUIRE(lut.v[i] == 0xFF || lut.v[i] < n_groups, "boa_group_stats_f64: lut[%d] = %d with %d groups", i, lut.v[i], n_groups);
    memset(host_count, 0, sizeof(uint64_t) * n_groups);
    memset(host_stats, 0, sizeof(double) * BOA_GROUP_STATS_F64_COLS * n_groups);
    if (n == 0) return BOA_OK;
    // device state; the kernels index 256 groups whatever n_groups is
    const size_t b_tab = (size_t)256 * GS_SLOTS * 256 * 4, b_slot = (size_t)256 * GS_SLOTS * 8, b_grp = (size_t)256 * 8;
    const size_t total = b_tab + 4 * b_slot + 4 * b_grp;
    unsigned char* d = nullptr;
    BOA_TRY(boa_malloc(c, total, (void**)&d));
    unsigned int* tab = (unsigned int*)d;
    unsigned long long* pref = (unsigned long long*)(d + b_tab);
    unsigned long long* lpref = pref + 256 * GS_SLOTS;
    unsigned long long* rank = lpref + 256 * GS_SLOTS;
    double* out = (double*)(rank + 256 * GS_SLOTS);
    unsigned long long* count = (unsigned long long*)(out + 256 * GS_SLOTS);
    double* sum = (double*)(count + 256);
    double* mean = sum + 256;
    double* m2 = mean + 256;
    hipError_t e = hipMemsetAsync(d, 0, total, c->stream);
    if (e != hipSuccess) {
        boa_free(c, d);
        BOA_HIP_TRY(e);
    }
    c->prof_break = true;
    // 16-byte loads of the values and 8-byte loads of the labels, or one voxel at a time for views that start anywhere
    const bool vec8 = ((uintptr_t)dev_ct % 16 == 0) && ((uintptr_t)dev_labels % 8 == 0);
    const size_t nvec = vec8 ? n / 8 : n;
    const size_t iters = (nvec + GS_HT - 1) / GS_HT;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(iters, (size_t)c->cu_count * 3));   // 52 KiB of LDS: three workgroups per CU
    const size_t vpb = (iters + grid - 1) / grid * GS_HT;
    for (int pass = 0; pass < 8; ++pass) {
        KernelTimer t(c, BOA_K_AGG, 0, (double)n * 9.0);
        if (vec8)
            group_select_pass<8>(c, pass, grid, dev_ct, dev_labels, n, lut, lpref, mean, tab, sum, m2, vpb);
        else
            group_select_pass<1>(c, pass, grid, dev_ct, dev_labels, n, lut, lpref, mean, tab, sum, m2, vpb);
        hipLaunchKernelGGL(k_group_select_step, dim3(256), dim3(256), 0, c->stream, pass, tab, pref, lpref, rank, count, sum, mean, out);
        t.stop();
    }
    std::vector<unsigned long long> h_count(256);
    std::vector<double> h_out(256 * GS_SLOTS), h_sum(256), h_m2(256);
    c->prof_break = true;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_count.data(), count, 256 * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_out.data(), out, 256 * GS_SLOTS * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_sum.data(), sum, 256 * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_m2.data(), m2, 256 * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    boa_free(c, d);
    BOA_HIP_TRY(e);
    for (int g = 0; g < n_groups; ++g) {
        host_count[g] = h_count[g];
        if (!h_count[g]) continue;
        double* r = host_stats + (size_t)g * BOA_GROUP_STATS_F64_COLS;
        r[0] = h_out[g * GS_SLOTS + 0];
        r[1] = h_out[g * GS_SLOTS + 7];
        r[2] = h_sum[g];
        r[3] = h_m2[g];
        for (int k = 0; k < 6; ++k) r[4 + k] = h_out[g * GS_SLOTS + 1 + k];
    }
    return BOA_OK;
}
