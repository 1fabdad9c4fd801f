// 26-connected component labelling of BYTE masks by atomic union-find (roots = smallest linear index of each component), the filters
// on its per-voxel roots and sizes, and the helpers of the z-slab sharded labelling.  The product path of boa_hip/agg_shard.py and
// what the BCA post-processing falls back to (BOA_MORPH_BYTES, slices too large for the LDS fill); ccl_bits.hip is the bit-mask form.
#include <string.h>

#include <algorithm>

#include "common.h"
#include "ccl_tile.h"

__global__ __launch_bounds__(256) void k_ccl_local(const unsigned char* __restrict__ mask, int Z, int Y, int X, int tiles_x, int tiles_y,
                                                   int* __restrict__ L, unsigned int* __restrict__ sizes) {
    __shared__ int lab[CCL_TILE];  // union-find parents; reused for the component sizes once every voxel knows its root
    __shared__ unsigned int rowbits[CCL_TY * CCL_TZ];  // bit lx of word (lz, ly): voxel is foreground
    const int tid = threadIdx.x;
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, tz = t / tiles_y;
    const int x0 = tx * CCL_TX, y0 = ty * CCL_TY, z0 = tz * CCL_TZ;
    // one wave-wide ballot per row pair: lane (row r of the pair, lx)
    for (int r2 = tid >> 5; r2 < CCL_TY * CCL_TZ; r2 += 8) {
        const int lx = tid & 31, ly = r2 % CCL_TY, lz = r2 / CCL_TY;
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        const bool fg = x < X && y < Y && z < Z && mask[((size_t)z * Y + y) * X + x] != 0;
        const unsigned long long b = __ballot(fg);
        if (lx == 0) rowbits[r2] = (unsigned int)(b >> (32 * ((tid >> 5) & 1)));
    }
    __syncthreads();
    // uniform tiles (all background, or a full tile of foreground: one component rooted at its first voxel) skip the union-find:
    // body-sized masks and their inverses are mostly such tiles.  Same forest as the general path (root = smallest index).
    {
        unsigned int w_and = 0xffffffffu, w_or = 0u;
        for (int r2 = tid; r2 < CCL_TY * CCL_TZ; r2 += 256) {
            w_and &= rowbits[r2];
            w_or |= rowbits[r2];
        }
        const int all0 = __syncthreads_and(w_or == 0u);
        const int all1 = __syncthreads_and(w_and == 0xffffffffu);
        if (all0 || all1) {
            const int root = (int)(((size_t)z0 * Y + y0) * X + x0);
#pragma unroll
            for (int k = 0; k < CCL_TILE / 256; ++k) {
                const int r2 = (tid >> 5) + 8 * k, lx = tid & 31, ly = r2 % CCL_TY, lz = r2 / CCL_TY;
                const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
                if (x >= X || y >= Y || z >= Z) continue;   // (all1 implies the tile lies inside the volume)
                const size_t gi = ((size_t)z * Y + y) * X + x;
                L[gi] = all1 ? root : -1;
                sizes[gi] = (all1 && r2 == 0 && lx == 0) ? (unsigned int)CCL_TILE : 0u;
            }
            return;
        }
    }
    // the tile's own labelling (ccl_tile.h): run starts, one union per pair of touching runs, roots, counts
    ccl_tile_init_runs(rowbits, lab, tid);
    __syncthreads();
    ccl_tile_union_rows(rowbits, lab, tid);
    __syncthreads();
    int myroot[CCL_TILE / 256];
    ccl_tile_roots(rowbits, lab, tid, myroot);
    __syncthreads();
    unsigned int* cnt = (unsigned int*)lab;
#pragma unroll
    for (int k = 0; k < CCL_TILE / 256; ++k) cnt[tid + 256 * k] = 0;
    __syncthreads();
    ccl_tile_count_runs(cnt, tid, myroot);
    __syncthreads();
    // global labels: the tile-local root's linear index in the volume
#pragma unroll
    for (int k = 0; k < CCL_TILE / 256; ++k) {
        const int r2 = (tid >> 5) + 8 * k, lx = tid & 31, ly = r2 % CCL_TY, lz = r2 / CCL_TY;
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        if (x >= X || y >= Y || z >= Z) continue;
        int out = -1;
        if (myroot[k] >= 0) {
            const int rt = myroot[k];
            const int rx = rt % CCL_TX, rr = rt / CCL_TX;
            out = (int)(((size_t)(z0 + rr / CCL_TY) * Y + (y0 + rr % CCL_TY)) * X + (x0 + rx));
        }
        const size_t gi = ((size_t)z * Y + y) * X + x;
        L[gi] = out;
        sizes[gi] = cnt[r2 * CCL_TX + lx];  // > 0 only at tile-local roots (every voxel is written: no memset of `sizes`)
    }
}

// the last pass: roots and sizes as documented (ccl_resolve_voxel in ccl_tile.h)
__global__ __launch_bounds__(256) void k_ccl_resolve(size_t n, int* L, unsigned int* sizes, int* n_comp) {
    ccl_resolve_voxel((size_t)blockIdx.x * 256 + threadIdx.x, n, L, sizes, n_comp);
}

// unions across tile faces only, per voxel and on the byte mask (the rule: "unions across tile faces" in ccl_tile.h)
__device__ __forceinline__ void ccl_border_voxel(const unsigned char* __restrict__ mask, int Z, int Y, int X, int* L, int x, int y, int z) {
    const size_t i = ((size_t)z * Y + y) * X + x;
    const int lx = x % CCL_TX, ly = y % CCL_TY, lz = z % CCL_TZ;
    if (!mask[i]) return;
    if (lx == CCL_TX - 1 && x + 1 < X && mask[i + 1]) uf_union(L, (int)i, (int)(i + 1));
    const bool left = x > 0 && mask[i - 1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int dz = r == 0 ? 0 : 1, dy = r == 0 ? 1 : r - 2;
        const int zz = z + dz, yy = y + dy;
        if (zz >= Z || yy < 0 || yy >= Y) continue;
        const bool row_other = (dz && lz == CCL_TZ - 1) || (dy == 1 && ly == CCL_TY - 1) || (dy == -1 && ly == 0);
        const size_t row = ((size_t)zz * Y + yy) * X;
        const bool m0 = x > 0 && mask[row + x - 1], m1 = mask[row + x] != 0, m2 = x + 1 < X && mask[row + x + 1];
        if (row_other) {   // the whole row lies in another tile
            if (!left) {
                if (m1) {
                    uf_union(L, (int)i, (int)(row + x));
                } else {
                    if (m0) uf_union(L, (int)i, (int)(row + x - 1));
                    if (m2) uf_union(L, (int)i, (int)(row + x + 1));
                }
            } else if (m2 && !m1) {
                uf_union(L, (int)i, (int)(row + x + 1));
            }
        } else if (!m1) {   // a row of this tile: only its x - 1 / x + 1 voxels in the x-neighbour tiles
            if (m0 && lx == 0) uf_union(L, (int)i, (int)(row + x - 1));
            if (m2 && lx == CCL_TX - 1) uf_union(L, (int)i, (int)(row + x + 1));
        }
    }
}

// The face voxels are enumerated directly (23 % of the volume; the first version launched over every voxel and returned for the
// rest: 1.9 of the 5.5 ms of a 512^3 mask).  mode 0: whole rows of the planes lz = TZ-1 (grid: x blocks, Y, planes);
// mode 1: the rows ly = 0 and ly = TY-1 of the other planes (grid: x blocks, 2 rows per y tile, Z);
// mode 2: the x-face voxels lx = 0 / TX-1 of the remaining rows (thread <-> (x tile, face, y), grid: blocks, 1, Z).
__global__ __launch_bounds__(256) void k_ccl_border(const unsigned char* __restrict__ mask, int Z, int Y, int X, int* L, int mode) {
    if (mode == 0) {
        const int x = (int)blockIdx.x * 256 + (int)threadIdx.x, y = (int)blockIdx.y, z = (int)blockIdx.z * CCL_TZ + CCL_TZ - 1;
        if (x >= X || z >= Z) return;
        ccl_border_voxel(mask, Z, Y, X, L, x, y, z);
    } else if (mode == 1) {
        const int x = (int)blockIdx.x * 256 + (int)threadIdx.x, z = (int)blockIdx.z;
        const int y = ((int)blockIdx.y >> 1) * CCL_TY + (((int)blockIdx.y & 1) ? CCL_TY - 1 : 0);
        if (x >= X || y >= Y || (z % CCL_TZ) == CCL_TZ - 1) return;
        ccl_border_voxel(mask, Z, Y, X, L, x, y, z);
    } else {
        const int tiles_x = (X + CCL_TX - 1) / CCL_TX;
        const int t = (int)blockIdx.x * 256 + (int)threadIdx.x, z = (int)blockIdx.z;
        const int f = t % (2 * tiles_x), y = t / (2 * tiles_x);
        const int x = (f >> 1) * CCL_TX + ((f & 1) ? CCL_TX - 1 : 0);
        if (y >= Y || x >= X) return;
        const int ly = y % CCL_TY;
        if ((z % CCL_TZ) == CCL_TZ - 1 || ly == 0 || ly == CCL_TY - 1) return;   // rows of modes 0 / 1
        ccl_border_voxel(mask, Z, Y, X, L, x, y, z);
    }
}

extern "C" int boa_ccl26(boa_ctx* c, const uint8_t* dev_mask, int Z, int Y, int X, int32_t* dev_roots,
                         uint32_t* dev_sizes, int* host_n_components) {
    BOA_REQUIRE(c && dev_mask && dev_roots && dev_sizes && Z > 0 && Y > 0 && X > 0, "boa_ccl26: bad argument");
    const size_t n = (size_t)Z * Y * X;
    BOA_REQUIRE(n < (1ull << 31), "boa_ccl26: volume too large for int32 indices");
    // the component counter: a pooled 4-byte block; without host_n_components nothing is copied back and the call does not
    // synchronise (the BCA post-processing chains 16 of these per volume)
    int* d_count = nullptr;
    BOA_TRY(boa_malloc(c, sizeof(int), (void**)&d_count));
    {   // (an early return must hand the pooled counter back)
        const hipError_t e0 = hipMemsetAsync(d_count, 0, sizeof(int), c->stream);
        if (e0 != hipSuccess) {
            boa_free(c, d_count);
            BOA_HIP_TRY(e0);
        }
    }
    unsigned grid = (unsigned)((n + 255) / 256);
    KernelTimer t(c, BOA_K_MORPH, 0, (double)n * 14.0);
    const int tx = (X + CCL_TX - 1) / CCL_TX, ty = (Y + CCL_TY - 1) / CCL_TY, tz = (Z + CCL_TZ - 1) / CCL_TZ;
    hipLaunchKernelGGL(k_ccl_local, dim3((unsigned)((size_t)tx * ty * tz)), dim3(256), 0, c->stream, dev_mask, Z, Y, X, tx, ty, dev_roots,
                       dev_sizes);
    hipLaunchKernelGGL(k_ccl_border, dim3((unsigned)((X + 255) / 256), (unsigned)Y, (unsigned)tz), dim3(256), 0, c->stream, dev_mask, Z, Y, X,
                       dev_roots, 0);
    hipLaunchKernelGGL(k_ccl_border, dim3((unsigned)((X + 255) / 256), (unsigned)(2 * ty), (unsigned)Z), dim3(256), 0, c->stream, dev_mask, Z,
                       Y, X, dev_roots, 1);
    hipLaunchKernelGGL(k_ccl_border, dim3((unsigned)(((size_t)2 * tx * Y + 255) / 256), 1, (unsigned)Z), dim3(256), 0, c->stream, dev_mask, Z, Y,
                       X, dev_roots, 2);
    hipLaunchKernelGGL(k_ccl_resolve, dim3(grid), dim3(256), 0, c->stream, n, dev_roots, dev_sizes, d_count);
    t.stop();
    hipError_t e = hipGetLastError();
    if (host_n_components && e == hipSuccess) {
        int cnt = 0;
        e = hipMemcpyAsync(&cnt, d_count, sizeof(int), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        *host_n_components = cnt;
    }
    boa_free(c, d_count);  // (stream-ordered: the block is reused only by work queued after the kernels above)
    BOA_HIP_TRY(e);
    return BOA_OK;
}

__global__ __launch_bounds__(256) void k_ccl_best(const unsigned int* __restrict__ sizes, size_t n,
                                                  unsigned long long* best) {
    // grid-stride, one atomic per wave of a few thousand (one per 64 voxels was 2 M atomics on one word: 1.8 ms per 512^3 volume)
    unsigned long long key = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned int sz = sizes[i];
        if (sz) {
            const unsigned long long k = ((unsigned long long)sz << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
            key = k > key ? k : key;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        unsigned long long o = __shfl_xor(key, m);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0 && key) atomicMax(best, key);
}

__global__ __launch_bounds__(256) void k_ccl_apply_largest(const int* __restrict__ roots, size_t n,
                                                           const unsigned long long* best, unsigned char* seg, int fill) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long b = *best;
    if (!b) return;
    const int best_root = (int)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFull));
    const int r = roots[i];
    if (r >= 0 && r != best_root) seg[i] = (unsigned char)fill;
}

extern "C" int boa_ccl_filter_largest(boa_ctx* c, const int32_t* dev_roots, const uint32_t* dev_sizes, size_t n,
                                      uint8_t* dev_seg, int fill_value) {
    BOA_REQUIRE(c && dev_roots && dev_sizes && dev_seg, "boa_ccl_filter_largest: NULL argument");
    if (n == 0) return BOA_OK;
    unsigned long long* d_best = nullptr;
    BOA_TRY(boa_malloc(c, sizeof(unsigned long long), (void**)&d_best));   // (pooled: no synchronisation around the two kernels)
    {
        const hipError_t e0 = hipMemsetAsync(d_best, 0, sizeof(unsigned long long), c->stream);
        if (e0 != hipSuccess) {   // (an early return must hand the pooled block back)
            boa_free(c, d_best);
            BOA_HIP_TRY(e0);
        }
    }
    unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_ccl_best, dim3(std::min<unsigned>(grid, (unsigned)c->cu_count * 8)), dim3(256), 0, c->stream, dev_sizes, n, d_best);
    hipLaunchKernelGGL(k_ccl_apply_largest, dim3(grid), dim3(256), 0, c->stream, dev_roots, n, d_best, dev_seg,
                       fill_value);
    hipError_t e = hipGetLastError();
    boa_free(c, d_best);
    BOA_HIP_TRY(e);
    return BOA_OK;
}

__global__ __launch_bounds__(256) void k_ccl_remove_small(const int* __restrict__ roots, const unsigned int* __restrict__ sizes,
                                                          size_t n, unsigned int max_size, unsigned char* mask) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = roots[i];
    if (r >= 0 && sizes[r] <= max_size) mask[i] = 0;
}

extern "C" int boa_ccl_remove_small(boa_ctx* c, const int32_t* dev_roots, const uint32_t* dev_sizes, size_t n,
                                    uint32_t max_size, uint8_t* dev_mask_inout) {
    BOA_REQUIRE(c && dev_roots && dev_sizes && dev_mask_inout, "boa_ccl_remove_small: NULL argument");
    if (n == 0) return BOA_OK;
    unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_ccl_remove_small, dim3(grid), dim3(256), 0, c->stream, dev_roots, dev_sizes, n, max_size,
                       dev_mask_inout);
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}


// ------------------------------------------------------------------------------------------------------
// z-slab sharded connected components (SURVEY 8e "aggregation stages"): each rank labels its slab with boa_ccl26; the
// components that touch a slab interface are merged on the host over the exchanged boundary planes (boa_hip/agg_shard.py).
// These helpers move the small per-component tables between the device and the host.
__global__ __launch_bounds__(256) void k_ccl_list(const unsigned int* __restrict__ sizes, size_t n, int max_out, int* __restrict__ roots_out,
                                                  unsigned int* __restrict__ sizes_out, int* __restrict__ count) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned s = sizes[i];
    if (s == 0) return;
    const int k = atomicAdd(count, 1);
    if (k < max_out) {
        roots_out[k] = (int)i;
        sizes_out[k] = s;
    }
}

extern "C" int boa_ccl_list_components(boa_ctx* c, const uint32_t* dev_sizes, size_t n, int max_out, int32_t* host_roots,
                                       uint32_t* host_sizes, int* host_count) {
    BOA_REQUIRE(c && dev_sizes && host_roots && host_sizes && host_count && max_out >= 0, "boa_ccl_list_components: bad argument");
    int* d_cnt = nullptr;
    int* d_roots = nullptr;
    unsigned* d_sz = nullptr;
    BOA_TRY(boa_malloc(c, sizeof(int), (void**)&d_cnt));
    int rc = boa_malloc(c, (size_t)std::max(max_out, 1) * 4, (void**)&d_roots);
    if (!rc) rc = boa_malloc(c, (size_t)std::max(max_out, 1) * 4, (void**)&d_sz);
    if (!rc) {
        hipMemsetAsync(d_cnt, 0, sizeof(int), c->stream);
        if (n) hipLaunchKernelGGL(k_ccl_list, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, dev_sizes, n, max_out, d_roots, d_sz, d_cnt);
        c->prof_break = true;
        hipError_t e = hipMemcpyAsync(host_count, d_cnt, sizeof(int), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        const int m = std::min(*host_count, max_out);
        if (e == hipSuccess && m > 0) e = hipMemcpy(host_roots, d_roots, (size_t)m * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && m > 0) e = hipMemcpy(host_sizes, d_sz, (size_t)m * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            boa_set_error("boa_ccl_list_components: %s", hipGetErrorString(e));
            rc = BOA_EHIP;
        }
    }
    boa_free(c, d_cnt);
    if (d_roots) boa_free(c, d_roots);
    if (d_sz) boa_free(c, d_sz);
    return rc;
}

__global__ __launch_bounds__(256) void k_scatter_u32(const int* __restrict__ idx, const unsigned int* __restrict__ val, int m,
                                                     unsigned int* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) dst[idx[i]] = val[i];
}

extern "C" int boa_scatter_u32(boa_ctx* c, uint32_t* dev_dst, const int32_t* host_idx, const uint32_t* host_val, int m) {
    BOA_REQUIRE(c && dev_dst && (m == 0 || (host_idx && host_val)) && m >= 0, "boa_scatter_u32: bad argument");
    if (m == 0) return BOA_OK;
    int* d_i = nullptr;
    unsigned* d_v = nullptr;
    BOA_TRY(boa_malloc(c, (size_t)m * 4, (void**)&d_i));
    int rc = boa_malloc(c, (size_t)m * 4, (void**)&d_v);
    if (!rc) {
        c->prof_break = true;
        // (stream-ordered copies: d_i / d_v may be recycled blocks whose previous user still has work queued on the stream)
        hipError_t e = hipMemcpyAsync(d_i, host_idx, (size_t)m * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_v, host_val, (size_t)m * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_scatter_u32, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, d_i, d_v, m, dev_dst);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the host arrays are borrowed for the duration of the call
        if (e != hipSuccess) {
            boa_set_error("boa_scatter_u32: %s", hipGetErrorString(e));
            rc = BOA_EHIP;
        }
    }
    boa_free(c, d_i);
    if (d_v) boa_free(c, d_v);
    return rc;
}

__global__ __launch_bounds__(256) void k_ccl_fill_unmarked(const int* __restrict__ roots, const unsigned int* __restrict__ sizes, size_t n,
                                                           unsigned int mark, unsigned char* __restrict__ seg, int fill) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = roots[i];
    if (r >= 0 && sizes[r] != mark) seg[i] = (unsigned char)fill;
}

extern "C" int boa_ccl_fill_unmarked(boa_ctx* c, const int32_t* dev_roots, const uint32_t* dev_sizes, size_t n, uint32_t mark,
                                     uint8_t* dev_seg, int fill_value) {
    BOA_REQUIRE(c && dev_roots && dev_sizes && dev_seg, "boa_ccl_fill_unmarked: NULL argument");
    if (n == 0) return BOA_OK;
    KernelTimer t(c, BOA_K_MORPH, 0, (double)n * 6.0);
    hipLaunchKernelGGL(k_ccl_fill_unmarked, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, dev_roots, dev_sizes, n, mark,
                       dev_seg, fill_value);
    t.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}
