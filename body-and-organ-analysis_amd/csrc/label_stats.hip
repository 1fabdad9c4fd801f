// Per-label basic statistics of a label volume over a CT in ONE pass (get_basic_statistics, TS/statistics.py:76-141: the reference
// makes three full-volume numpy passes per label -- `seg == k`, touches_border, np.average -- 117 times), and the label look-up
// table pass behind `roi_subset` (TS/nnunet.py:707-709).
#include "common.h"

// Everything here is integer: counts, int64 sums, OR-ed flags, integer min / max.  The table does not depend on the order in which
// lanes, waves and workgroups arrive and is bitwise reproducible.
//
// A lane reads 16 consecutive voxels (one 16-byte load of labels, two or four of CT values) and keeps ONE open run {label, count,
// sum, touches} in registers, across iterations: labels are spatially coherent, so inside an organ or the background nothing leaves
// the registers.  When the label changes the run is handed to the wave: the first pending lane's label is broadcast, the lanes that
// share it are balloted, their counts and sums are reduced across the wave and one lane adds the result to the workgroup's table in
// LDS (64-bit adds); after LS_ROUNDS distinct labels the lanes still pending add their own run (salt-and-pepper labels: up to 64
// distinct labels in a wave).  The workgroup sends the non-empty rows of its table to the global one at the end: one barrier, then
// one flush -- no row is emptied while another wave may still add to it.
//
// The border test needs (i0, i1, i2) of a voxel: one decomposition per 16 voxels, then the column walks along the innermost axis and
// carries into the row.  `i < border || i >= dim - border` in signed arithmetic is numpy's `mask[:border]` / `mask[-border:]` also
// for dim < 2 * border (the slabs overlap) and dim < border (both are the whole axis).
#define LS_THREADS 256
#define LS_ROUNDS 4

struct LsTable {
    unsigned long long cnt[256];
    long long sum[256];
    unsigned int touch[256];
    int vmin, vmax;
};

__device__ __forceinline__ void ls_add(LsTable& t, unsigned label, unsigned cnt, long long sum, unsigned touch) {
    atomicAdd(&t.cnt[label], (unsigned long long)cnt);
    atomicAdd((unsigned long long*)&t.sum[label], (unsigned long long)sum);      // (two's complement: the signed sum)
    if (touch) atomicOr(&t.touch[label], 1u);
}

// Hands the runs of the lanes with `p` to the LDS table.  Called by the whole wave (wave-uniform control flow).
__device__ __forceinline__ void ls_emit(LsTable& t, bool p, unsigned label, unsigned cnt, long long sum, unsigned touch) {
    unsigned long long todo = __builtin_amdgcn_ballot_w64(p);
#pragma unroll 1
    for (int round = 0; todo != 0ull && round < LS_ROUNDS; ++round) {
        const int leader = __builtin_ctzll(todo);
        const unsigned l0 = (unsigned)__builtin_amdgcn_readlane((int)label, leader);
        const bool mine = p && label == l0;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(mine);
        unsigned c = mine ? cnt : 0u;
        long long s = mine ? sum : 0ll;
        if ((m & (m - 1ull)) != 0ull) {          // more than one lane: reduce over the wave (the other lanes carry zeros)
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                c += (unsigned)__shfl_xor((int)c, d, 64);
                s += __shfl_xor(s, d, 64);
            }
        }
        const bool tch = __builtin_amdgcn_ballot_w64(mine && touch != 0u) != 0ull;
        if ((int)(threadIdx.x & 63) == leader) ls_add(t, l0, c, s, tch ? 1u : 0u);
        p = p && !mine;
        todo &= ~m;
    }
    if (p) ls_add(t, label, cnt, sum, touch);
}

template <typename CT>
__global__ __launch_bounds__(LS_THREADS) void k_label_stats(const CT* __restrict__ ct, const unsigned char* __restrict__ labels, size_t n,
                                                            int d0, int d1, int d2, int border, size_t iters_per_block,
                                                            unsigned long long* __restrict__ out) {
    constexpr int CV = 16 * (int)sizeof(CT) / 16;      // 16-byte loads of CT values per 16 voxels
    __shared__ LsTable tab;
    const int tid = threadIdx.x;
    tab.cnt[tid] = 0ull;
    tab.sum[tid] = 0ll;
    tab.touch[tid] = 0u;
    if (tid == 0) {
        tab.vmin = 0x7fffffff;
        tab.vmax = -0x7fffffff - 1;
    }
    __syncthreads();
    const size_t n16 = n / 16;
    const int hi0 = d0 - border, hi1 = d1 - border, hi2 = d2 - border;
    auto row_touches = [&](int i0, int i1) { return i0 < border || i0 >= hi0 || i1 < border || i1 >= hi1; };
    int vmin = 0x7fffffff, vmax = -0x7fffffff - 1;
    unsigned cur = 0u, cnt = 0u, tch = 0u;       // the lane's open run (cnt == 0: none)
    long long sum = 0ll;
    union LabV {
        uint4 u;
        unsigned char b[16];
    };
    union CtV {
        uint4 u[CV];
        CT v[16];
    };
#pragma unroll 1
    for (size_t it = 0; it < iters_per_block; ++it) {
        const size_t g = ((size_t)blockIdx.x * iters_per_block + it) * LS_THREADS + tid;
        const bool live = g < n16;
        LabV lb;
        CtV cv;
        lb.u = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int k = 0; k < CV; ++k) cv.u[k] = make_uint4(0, 0, 0, 0);
        int i0 = 0, i1 = 0, col = 0;
        if (live) {
            lb.u = *(const uint4*)(labels + g * 16);
#pragma unroll
            for (int k = 0; k < CV; ++k) cv.u[k] = *((const uint4*)(ct + g * 16) + k);
            idx3(g * 16, d1, d2, i0, i1, col);
        }
        bool rowt = row_touches(i0, i1);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const unsigned l = lb.b[i];
            const int v = (int)cv.v[i];
            const bool differs = live && cnt != 0u && l != cur;
            if (__builtin_amdgcn_ballot_w64(differs) != 0ull) {
                ls_emit(tab, differs, cur, cnt, sum, tch);
                if (differs) {
                    cnt = 0u;
                    sum = 0ll;
                    tch = 0u;
                }
            }
            if (live) {
                cur = l;
                cnt += 1u;
                sum += (long long)v;
                tch |= (rowt || col < border || col >= hi2) ? 1u : 0u;
                vmin = min(vmin, v);
                vmax = max(vmax, v);
                if (++col == d2) {
                    col = 0;
                    if (++i1 == d1) {
                        i1 = 0;
                        ++i0;
                    }
                    rowt = row_touches(i0, i1);
                }
            }
        }
    }
    ls_emit(tab, cnt != 0u, cur, cnt, sum, tch);
    // the last n % 16 voxels, one lane each
    if (blockIdx.x == 0 && (size_t)tid < n - n16 * 16) {
        const size_t i = n16 * 16 + (size_t)tid;
        int i0, i1, col;
        idx3(i, d1, d2, i0, i1, col);
        const int v = (int)ct[i];
        ls_add(tab, labels[i], 1u, (long long)v, (row_touches(i0, i1) || col < border || col >= hi2) ? 1u : 0u);
        vmin = min(vmin, v);
        vmax = max(vmax, v);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        vmin = min(vmin, __shfl_xor(vmin, d, 64));
        vmax = max(vmax, __shfl_xor(vmax, d, 64));
    }
    if ((tid & 63) == 0) {
        atomicMin(&tab.vmin, vmin);
        atomicMax(&tab.vmax, vmax);
    }
    __syncthreads();       // every add of every wave is in the table: the one flush of this workgroup
    const unsigned long long c = tab.cnt[tid];
    if (c != 0ull) {
        atomicAdd(&out[tid], c);
        atomicAdd(&out[256 + tid], (unsigned long long)tab.sum[tid]);
        if (tab.touch[tid]) atomicOr(&out[512 + tid], 1ull);
    }
    if (tid == 0 && tab.vmin <= tab.vmax) {
        atomicMin((long long*)&out[768], (long long)tab.vmin);
        atomicMax((long long*)&out[769], (long long)tab.vmax);
    }
}

__global__ __launch_bounds__(256) void k_label_stats_init(unsigned long long* __restrict__ out) {
    for (int i = threadIdx.x; i < BOA_LABEL_STATS_WORDS; i += 256)
        out[i] = i == 768 ? 0x7fffffffffffffffull : (i == 769 ? 0x8000000000000000ull : 0ull);
}

extern "C" int boa_label_basic_stats(boa_ctx* c, const void* dev_ct, int ct_dtype, const uint8_t* dev_labels, const int dims[3],
                                     int border, uint64_t* dev_out) {
    BOA_REQUIRE(c && dev_ct && dev_labels && dims && dev_out, "boa_label_basic_stats: NULL argument");
    BOA_REQUIRE(ct_dtype == 1 || ct_dtype == 2, "boa_label_basic_stats: ct dtype %d (1 int16, 2 int32)", ct_dtype);
    BOA_REQUIRE(dims[0] >= 0 && dims[1] >= 0 && dims[2] >= 0 && border >= 0, "boa_label_basic_stats: negative dims or border");
    BOA_REQUIRE((((uintptr_t)dev_ct | (uintptr_t)dev_labels) & 15) == 0 && ((uintptr_t)dev_out & 7) == 0,
                "boa_label_basic_stats: the arrays must be 16-byte aligned");
    const size_t n = (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2];
    hipLaunchKernelGGL(k_label_stats_init, dim3(1), dim3(256), 0, c->stream, (unsigned long long*)dev_out);
    BOA_HIP_TRY(hipGetLastError());
    if (n == 0) return BOA_OK;
    // contiguous voxel ranges per workgroup (few labels each, long runs per lane): up to 8 workgroups per CU
    const size_t iters = (n / 16 + LS_THREADS - 1) / LS_THREADS;
    const size_t blocks = std::max<size_t>(1, std::min<size_t>(iters, (size_t)c->cu_count * 8));
    const size_t ipb = (iters + blocks - 1) / blocks;
    const unsigned grid = (unsigned)std::max<size_t>(1, (iters + std::max<size_t>(ipb, 1) - 1) / std::max<size_t>(ipb, 1));
    KernelTimer t(c, BOA_K_AGG, 0, (double)n * (ct_dtype == 1 ? 3.0 : 5.0));
    if (ct_dtype == 1)
        hipLaunchKernelGGL(k_label_stats<short>, dim3(grid), dim3(LS_THREADS), 0, c->stream, (const short*)dev_ct, dev_labels, n, dims[0],
                           dims[1], dims[2], border, ipb, (unsigned long long*)dev_out);
    else
        hipLaunchKernelGGL(k_label_stats<int>, dim3(grid), dim3(LS_THREADS), 0, c->stream, (const int*)dev_ct, dev_labels, n, dims[0],
                           dims[1], dims[2], border, ipb, (unsigned long long*)dev_out);
    t.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}

// ------------------------------------------------------------------------------------------------------
struct LsLut {
    unsigned char v[256];
};

__global__ __launch_bounds__(256) void k_label_apply_lut(const unsigned char* in, LsLut lut, size_t n, size_t head,
                                                         size_t n16, unsigned char* out) {   // (in == out is allowed)
    // voxels [head, head + 16 n16) in 16-byte vectors, the others one by one
    const size_t stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t g = t0; g < n16; g += stride) {
        union {
            uint4 u;
            unsigned char b[16];
        } x;
        x.u = *(const uint4*)(in + head + g * 16);
#pragma unroll
        for (int i = 0; i < 16; ++i) x.b[i] = lut.v[x.b[i]];
        *(uint4*)(out + head + g * 16) = x.u;
    }
    for (size_t k = t0; k < n - n16 * 16; k += stride) {
        const size_t i = k < head ? k : k + n16 * 16;
        out[i] = lut.v[in[i]];
    }
}

extern "C" int boa_label_apply_lut(boa_ctx* c, const uint8_t* dev_labels, size_t n, const uint8_t host_lut[256], uint8_t* dev_out) {
    BOA_REQUIRE(c && dev_labels && host_lut && dev_out, "boa_label_apply_lut: NULL argument");
    if (n == 0) return BOA_OK;
    LsLut lut;
    for (int i = 0; i < 256; ++i) lut.v[i] = host_lut[i];
    size_t head = (size_t)((16 - ((uintptr_t)dev_labels & 15)) & 15);
    if (head > n) head = n;
    // (arrays that cannot be aligned together are processed one voxel at a time)
    const size_t n16 = (((uintptr_t)dev_out + head) & 15) == 0 ? (n - head) / 16 : 0;
    const size_t work = std::max(n16, n - n16 * 16);
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((work + 255) / 256, (size_t)c->cu_count * 16));
    KernelTimer t(c, BOA_K_AGG, 0, 2.0 * (double)n);
    hipLaunchKernelGGL(k_label_apply_lut, dim3(grid), dim3(256), 0, c->stream, dev_labels, lut, n, head, n16, dev_out);
    t.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}
