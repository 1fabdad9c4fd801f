// 6-connected component labelling of a uint8 LABEL volume, all labels in one run: a component is a maximal face-connected set of
// voxels of the same non-zero value (what scipy.ndimage.label(data == v) finds, label by label, in TS/postprocessing.py:13-98), and
// the two blob filters on its per-voxel roots and sizes.  Same two-level scheme and the same forest invariant as ccl_bytes.hip (root
// = smallest linear index = first voxel in raster order): a 32 x 16 x 16 tile is labelled in LDS, unions across tile faces go
// through global memory.  What differs from the binary kernels: runs are maximal x-runs of EQUAL label, rows are joined only at
// equal lx (faces, no edges or corners) and only where the labels are equal, and every voxel of a tile may be its own component
// (8 192 per tile), so the parents and sizes are per voxel as in ccl_bytes.hip: int32 + uint32 = 8 bytes per voxel of work space.
#include <algorithm>

#include "common.h"
#include "ccl_tile.h"

__global__ __launch_bounds__(256) void k_lb_local(const unsigned char* __restrict__ labels, int D0, int D1, int D2, int tiles_x, int tiles_y,
                                                  int* __restrict__ L, unsigned int* __restrict__ sizes) {
    __shared__ int lab[CCL_TILE];                       // union-find parents; reused for the component sizes once every voxel knows its root
    __shared__ unsigned char val[CCL_TILE];             // the tile's labels (0 outside the volume)
    __shared__ unsigned int rowstart[CCL_TY * CCL_TZ];  // bit lx of word (lz, ly): the voxel is the first of its run of equal labels
    const int tid = threadIdx.x, lx = tid & 31;
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, tz = t / tiles_y;
    const int x0 = tx * CCL_TX, y0 = ty * CCL_TY, z0 = tz * CCL_TZ;
    // a wave holds two rows: the ballot of the run starts is split per row; the parents start at the first voxel of the voxel's run
    // (the runs of a row are its components: no unions along x at all)
    unsigned int vmin = 255u, vmax = 0u;
    for (int r2 = tid >> 5; r2 < CCL_TY * CCL_TZ; r2 += 8) {
        const int ly = r2 % CCL_TY, lz = r2 / CCL_TY;
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        const unsigned int v = (x < D2 && y < D1 && z < D0) ? labels[((size_t)z * D1 + y) * D2 + x] : 0u;
        const unsigned int prev = __shfl_up(v, 1);
        const unsigned long long b = __ballot(lx == 0 || prev != v);
        const unsigned int starts = (unsigned int)(b >> (32 * ((tid >> 5) & 1)));   // this row's half of the wave
        const unsigned int upto = starts & (0xffffffffu >> (31 - lx));              // run starts at or left of lx (bit 0 is always set)
        if (lx == 0) rowstart[r2] = starts;
        val[r2 * CCL_TX + lx] = (unsigned char)v;
        lab[r2 * CCL_TX + lx] = v ? r2 * CCL_TX + (31 - __clz((int)upto)) : -1;
        vmin = v < vmin ? v : vmin;
        vmax = v > vmax ? v : vmax;
    }
    __syncthreads();
    // uniform tiles (all background, or a full tile of one label: one component rooted at its first voxel) skip the union-find:
    // organ-sized structures and the background around them are mostly such tiles.  Same forest as the general path.
    {
        const unsigned int v0 = val[0];
        if (__syncthreads_and(vmin == v0 && vmax == v0)) {
            const int root = (int)(((size_t)z0 * D1 + y0) * D2 + x0);
#pragma unroll
            for (int k = 0; k < CCL_TILE / 256; ++k) {
                const int r2 = (tid >> 5) + 8 * k, ly = r2 % CCL_TY, lz = r2 / CCL_TY;
                const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
                if (x >= D2 || y >= D1 || z >= D0) continue;   // (a non-zero v0 implies the tile lies inside the volume)
                const size_t gi = ((size_t)z * D1 + y) * D2 + x;
                L[gi] = v0 ? root : -1;
                sizes[gi] = (v0 && r2 == 0 && lx == 0) ? (unsigned int)CCL_TILE : 0u;
            }
            return;
        }
    }
    // unions with the rows (dy, dz) = (1, 0) and (0, 1) at equal lx and equal label: ONE union per pair of touching runs -- where either
    // run starts (at any other voxel of the overlap the pair to the left joins the same two runs)
    for (int r2 = tid >> 5; r2 < CCL_TY * CCL_TZ; r2 += 8) {
        const int ly = r2 % CCL_TY, lz = r2 / CCL_TY;
        const int i = r2 * CCL_TX + lx;
        const unsigned int v = val[i];
        if (!v) continue;
        const bool s_me = (rowstart[r2] >> lx) & 1u;
        if (ly + 1 < CCL_TY && val[i + CCL_TX] == v && (s_me || ((rowstart[r2 + 1] >> lx) & 1u))) lds_union(lab, i, i + CCL_TX);
        if (lz + 1 < CCL_TZ && val[i + CCL_TX * CCL_TY] == v && (s_me || ((rowstart[r2 + CCL_TY] >> lx) & 1u)))
            lds_union(lab, i, i + CCL_TX * CCL_TY);
    }
    __syncthreads();
    int myroot[CCL_TILE / 256];
#pragma unroll
    for (int k = 0; k < CCL_TILE / 256; ++k) {
        const int i = ((tid >> 5) + 8 * k) * CCL_TX + lx;
        myroot[k] = val[i] ? lds_find(lab, i) : -1;
    }
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
        const int r2 = (tid >> 5) + 8 * k, ly = r2 % CCL_TY, lz = r2 / CCL_TY;
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        if (x >= D2 || y >= D1 || z >= D0) continue;
        int out = -1;
        if (myroot[k] >= 0) {
            const int rt = myroot[k];
            const int rx = rt % CCL_TX, rr = rt / CCL_TX;
            out = (int)(((size_t)(z0 + rr / CCL_TY) * D1 + (y0 + rr % CCL_TY)) * D2 + (x0 + rx));
        }
        const size_t gi = ((size_t)z * D1 + y) * D2 + x;
        L[gi] = out;
        sizes[gi] = cnt[r2 * CCL_TX + lx];  // > 0 only at tile-local roots (every voxel is written: no memset of `sizes`)
    }
}

// Unions across tile faces, one launch per face direction over exactly the face voxels that have a neighbour beyond the face:
//   mode 0: the planes lz = TZ - 1 (grid: x blocks, D1, planes), neighbour z + 1;
//   mode 1: the rows ly = TY - 1 (grid: x blocks, rows, D0), neighbour y + 1;
//   mode 2: the voxels lx = TX - 1 (thread <-> (x face, y), grid: blocks, 1, D0), neighbour x + 1.
// Modes 0 / 1 make one union per pair of touching runs as the tile pass does: not where the pair to the left has the same two labels
// (it is linked to both voxels along x, inside its tile or by mode 2).
__global__ __launch_bounds__(256) void k_lb_border(const unsigned char* __restrict__ labels, int D0, int D1, int D2, int* L, int mode) {
    if (mode == 2) {
        const int faces = (D2 - 1) / CCL_TX;   // faces x = 32 f + 31 with x + 1 < D2
        const int t = (int)blockIdx.x * 256 + (int)threadIdx.x, z = (int)blockIdx.z;
        const int y = t / faces, x = (t % faces) * CCL_TX + CCL_TX - 1;
        if (y >= D1) return;
        const size_t i = ((size_t)z * D1 + y) * D2 + x;
        const unsigned char v = labels[i];
        if (v && labels[i + 1] == v) uf_union(L, (int)i, (int)(i + 1));
        return;
    }
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (x >= D2) return;
    int y, z;
    size_t step;
    if (mode == 0) {
        y = (int)blockIdx.y;
        z = (int)blockIdx.z * CCL_TZ + CCL_TZ - 1;
        if (z + 1 >= D0) return;
        step = (size_t)D1 * D2;
    } else {
        y = (int)blockIdx.y * CCL_TY + CCL_TY - 1;
        z = (int)blockIdx.z;
        if (y + 1 >= D1) return;
        step = (size_t)D2;
    }
    const size_t i = ((size_t)z * D1 + y) * D2 + x, j = i + step;
    const unsigned char v = labels[i];
    if (!v || labels[j] != v) return;
    if (x > 0 && labels[i - 1] == v && labels[j - 1] == v) return;
    uf_union(L, (int)i, (int)j);
}

__global__ __launch_bounds__(256) void k_lb_resolve(size_t n, int* L, unsigned int* sizes, int* n_comp) {
    ccl_resolve_voxel((size_t)blockIdx.x * 256 + threadIdx.x, n, L, sizes, n_comp);
}

extern "C" int boa_label_blobs6(boa_ctx* c, const uint8_t* dev_labels, int D0, int D1, int D2, int32_t* dev_roots, uint32_t* dev_sizes,
                                int* host_n_components) {
    BOA_REQUIRE(c, "boa_label_blobs6: ctx is NULL");
    BOA_REQUIRE(dev_labels, "boa_label_blobs6: dev_labels is NULL");
    BOA_REQUIRE(dev_roots, "boa_label_blobs6: dev_roots is NULL");
    BOA_REQUIRE(dev_sizes, "boa_label_blobs6: dev_sizes is NULL");
    BOA_REQUIRE(D0 > 0 && D1 > 0 && D2 > 0, "boa_label_blobs6: D0, D1, D2 = %d, %d, %d must be positive", D0, D1, D2);
    BOA_REQUIRE(D0 <= 65535 && D1 <= 65535, "boa_label_blobs6: D0, D1 = %d, %d exceed 65535", D0, D1);
    const size_t n = (size_t)D0 * D1 * D2;
    BOA_REQUIRE(n < (1ull << 31), "boa_label_blobs6: D0 * D1 * D2 too large for int32 indices");
    // the component counter: a pooled 4-byte block; without host_n_components nothing is copied back and the call does not synchronise
    int* d_count = nullptr;
    BOA_TRY(boa_malloc(c, sizeof(int), (void**)&d_count));
    {   // (an early return must hand the pooled counter back)
        const hipError_t e0 = hipMemsetAsync(d_count, 0, sizeof(int), c->stream);
        if (e0 != hipSuccess) {
            boa_free(c, d_count);
            BOA_HIP_TRY(e0);
        }
    }
    KernelTimer t(c, BOA_K_MORPH, 0, (double)n * 22.0);
    const int tx = (D2 + CCL_TX - 1) / CCL_TX, ty = (D1 + CCL_TY - 1) / CCL_TY, tz = (D0 + CCL_TZ - 1) / CCL_TZ;
    const unsigned xb = (unsigned)((D2 + 255) / 256);
    const int planes = (D0 - 1) / CCL_TZ, rows = (D1 - 1) / CCL_TY, faces = (D2 - 1) / CCL_TX;   // those with a neighbour beyond them
    hipLaunchKernelGGL(k_lb_local, dim3((unsigned)((size_t)tx * ty * tz)), dim3(256), 0, c->stream, dev_labels, D0, D1, D2, tx, ty, dev_roots,
                       dev_sizes);
    if (planes) hipLaunchKernelGGL(k_lb_border, dim3(xb, (unsigned)D1, (unsigned)planes), dim3(256), 0, c->stream, dev_labels, D0, D1, D2, dev_roots, 0);
    if (rows) hipLaunchKernelGGL(k_lb_border, dim3(xb, (unsigned)rows, (unsigned)D0), dim3(256), 0, c->stream, dev_labels, D0, D1, D2, dev_roots, 1);
    if (faces)
        hipLaunchKernelGGL(k_lb_border, dim3((unsigned)(((size_t)faces * D1 + 255) / 256), 1, (unsigned)D0), dim3(256), 0, c->stream, dev_labels, D0,
                           D1, D2, dev_roots, 2);
    hipLaunchKernelGGL(k_lb_resolve, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, dev_roots, dev_sizes, d_count);
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

// ---- the filters ---------------------------------------------------------------------------------------------------------------------
struct LbModes {
    unsigned char m[256];
};

// per label of mode 2: the largest component as max of (size << 32) | ~root, so that a tie goes to the smallest root.  Roots are
// reduced in an LDS table first (speckle has millions of them), then one global atomic per (block, label present).
__global__ __launch_bounds__(256) void k_lb_best(const unsigned char* __restrict__ labels, const unsigned int* __restrict__ sizes, size_t n,
                                                 LbModes modes, unsigned long long* __restrict__ best) {
    __shared__ unsigned long long sbest[256];
    sbest[threadIdx.x] = 0ull;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned int sz = sizes[i];
        if (!sz) continue;   // not a root
        const unsigned int v = labels[i];
        if (modes.m[v] != 2) continue;
        atomicMax(&sbest[v], ((unsigned long long)sz << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i));
    }
    __syncthreads();
    const unsigned long long k = sbest[threadIdx.x];
    if (k) atomicMax(&best[threadIdx.x], k);
}

__global__ __launch_bounds__(256) void k_lb_apply(const int* __restrict__ roots, const unsigned int* __restrict__ sizes, size_t n, LbModes modes,
                                                  unsigned int lo, unsigned int hi, const unsigned long long* __restrict__ best,
                                                  unsigned char* labels) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = roots[i];
    if (r < 0) return;
    const unsigned int v = labels[i];   // (0 where an earlier filter call cleared the voxel)
    if (!v) return;
    const unsigned int m = modes.m[v];
    bool clear = false;
    if (m == 1) {
        const unsigned int s = sizes[r];
        clear = s <= lo || s > hi;
    } else if (m == 2) {
        clear = r != (int)(0xFFFFFFFFu - (unsigned)(best[v] & 0xFFFFFFFFull));
    }
    if (clear) labels[i] = 0;
}

extern "C" int boa_label_blobs_filter(boa_ctx* c, const int32_t* dev_roots, const uint32_t* dev_sizes, size_t n, const uint8_t host_mode[256],
                                      uint32_t lo, uint32_t hi, uint8_t* dev_labels_inout) {
    BOA_REQUIRE(c, "boa_label_blobs_filter: ctx is NULL");
    BOA_REQUIRE(dev_roots, "boa_label_blobs_filter: dev_roots is NULL");
    BOA_REQUIRE(dev_sizes, "boa_label_blobs_filter: dev_sizes is NULL");
    BOA_REQUIRE(host_mode, "boa_label_blobs_filter: host_mode is NULL");
    BOA_REQUIRE(dev_labels_inout, "boa_label_blobs_filter: dev_labels_inout is NULL");
    BOA_REQUIRE(n < (1ull << 31), "boa_label_blobs_filter: n too large for int32 indices");
    LbModes modes;
    bool any = false, any_largest = false;
    for (int v = 0; v < 256; ++v) {
        BOA_REQUIRE(host_mode[v] <= 2, "boa_label_blobs_filter: host_mode[%d] = %d is not 0, 1 or 2", v, (int)host_mode[v]);
        modes.m[v] = v ? host_mode[v] : 0;   // (background has no components)
        any |= modes.m[v] != 0;
        any_largest |= modes.m[v] == 2;
    }
    if (n == 0 || !any) return BOA_OK;
    unsigned long long* d_best = nullptr;
    BOA_TRY(boa_malloc(c, 256 * sizeof(unsigned long long), (void**)&d_best));   // (pooled: no synchronisation around the kernels)
    if (any_largest) {
        const hipError_t e0 = hipMemsetAsync(d_best, 0, 256 * sizeof(unsigned long long), c->stream);
        if (e0 != hipSuccess) {   // (an early return must hand the pooled block back)
            boa_free(c, d_best);
            BOA_HIP_TRY(e0);
        }
    }
    const unsigned grid = (unsigned)((n + 255) / 256);
    KernelTimer t(c, BOA_K_MORPH, 0, (double)n * 10.0);
    if (any_largest)
        hipLaunchKernelGGL(k_lb_best, dim3(std::min<unsigned>(grid, (unsigned)c->cu_count * 8)), dim3(256), 0, c->stream, dev_labels_inout, dev_sizes,
                           n, modes, d_best);
    hipLaunchKernelGGL(k_lb_apply, dim3(grid), dim3(256), 0, c->stream, dev_roots, dev_sizes, n, modes, lo, hi, d_best, dev_labels_inout);
    const hipError_t e = hipGetLastError();
    t.stop();
    boa_free(c, d_best);
    BOA_HIP_TRY(e);
    return BOA_OK;
}
