// Shared pieces of the connected-component kernels (ccl_bytes.hip, ccl_bits.hip, ccl_labels.hip) and of the background union-find of
// the byte fill (morph.hip): the atomic union-find on global memory, its LDS form, the labelling of one 32 x 16 x 16 tile in LDS (the
// binary form; ccl_labels.hip has its own run and row rules and shares the union-find, the counting and the last pass).
// Forest invariant everywhere: parent index <= own index, root = smallest linear index of the component.
#pragma once
#include <hip/hip_runtime.h>

#define AGENT_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// ---- union-find on global memory ------------------------------------------------------------------------------------------------
// HALVE = false stores nothing during a find (the per-voxel background union-find of morph.hip walks read-only).
template <bool HALVE = true>
__device__ __forceinline__ int uf_find(int* L, int i) {
    // path halving: every node on the way is re-pointed to its grandparent (parents only ever move towards the root, so a racing
    // walker at worst takes the longer way).  The store is an agent-scope atomic store like every other access to L in the
    // union kernels: a plain store stays dirty in the L2 of the XCD that issued it, and when that line is written back it can
    // take stale copies of NEIGHBOURING words with it -- words that another XCD's atomicMin has meanwhile changed at the
    // memory side.  Measured: with plain stores 1 labelling in ~200 lost one union (a voxel keeps a root that was merged away)
    // whenever a second stream kept the GPU busy (tools/ccl_stress.py, tests/test_gpu_lanes.py); with atomic stores 0 in 2 400.
    int p = AGENT_LOAD(&L[i]);
    while (p != i) {
        const int gp = AGENT_LOAD(&L[p]);
        if (HALVE && gp != p) __hip_atomic_store(&L[i], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        i = p;
        p = gp;
    }
    return i;
}

template <bool HALVE = true>
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
    while (true) {
        a = uf_find<HALVE>(L, a);
        b = uf_find<HALVE>(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&L[a], b);  // link the larger root under the smaller
        if (old == a) return;
        a = old;
    }
}

// ---- the same on LDS words -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(volatile int* L, int i) {
    int p = L[i];
    while (p != i) {
        const int gp = L[p];
        if (gp != p) L[i] = gp;  // path halving (a racing walker at worst takes the longer way)
        i = p;
        p = gp;
    }
    return i;
}

__device__ __forceinline__ void lds_union(int* L, int a, int b) {
    while (true) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}

// ---- two-level labelling: tiles of CCL_TX x CCL_TY x CCL_TZ voxels (one 32-bit mask word per row) are labelled in LDS first, then
// only the unions that cross a tile face go through global memory.  A per-voxel version (uf_union on every voxel) spent its time in
// device-scope atomics and pointer chasing through HBM (5.7 ms per 512^3 mask); inside a tile the same union-find runs on LDS words.
#define CCL_TX 32
#define CCL_TY 16
#define CCL_TZ 16
#define CCL_TILE (CCL_TX * CCL_TY * CCL_TZ)

// The tile kernels run 256 threads: thread tid owns the voxels (row r2 = (tid >> 5) + 8 k, lx = tid & 31), k < CCL_TILE / 256, so a wave
// holds two whole rows.  rowbits[CCL_TY * CCL_TZ]: bit lx of word r2 = lz * CCL_TY + ly is set for a foreground voxel; lab[CCL_TILE]:
// the parents, then (as `cnt`) the voxel counts at the tile-local roots.  The helpers hold no barrier: the kernel puts one after each.

// parents start at the first voxel of the voxel's x-run (the runs of a row are its components: no unions along x at all)
__device__ __forceinline__ void ccl_tile_init_runs(const unsigned int* rowbits, int* lab, int tid) {
    for (int r2 = tid >> 5; r2 < CCL_TY * CCL_TZ; r2 += 8) {
        const int lx = tid & 31;
        const unsigned int me = rowbits[r2];
        const unsigned int starts = me & ~(me << 1);                       // first voxel of every run
        const unsigned int upto = starts & (0xffffffffu >> (31 - lx));     // run starts at or left of lx
        lab[r2 * CCL_TX + lx] = ((me >> lx) & 1u) ? r2 * CCL_TX + (31 - __clz((int)upto)) : -1;
    }
}

// unions between the runs of neighbouring rows (the four forward rows (dz, dy) = (0, 1), (1, -1), (1, 0), (1, 1)): ONE union per
// pair of touching runs -- at the first voxel where both rows are set, or, for runs that only touch diagonally, at the run end
// facing the other run.  (The first version linked every voxel to the voxel below it: ~5 LDS union-finds per voxel.)
// (measured and not kept: one neighbour-row class per phase with a pointer-jumping pass in between -- 42.8 -> 50.6 ms on the 512^3
//  noise labels of the bit path: the chains are short, the extra passes are not)
__device__ __forceinline__ void ccl_tile_union_rows(const unsigned int* rowbits, int* lab, int tid) {
    for (int r2 = tid >> 5; r2 < CCL_TY * CCL_TZ; r2 += 8) {
        const int lx = tid & 31, ly = r2 % CCL_TY, lz = r2 / CCL_TY;
        const unsigned int me = rowbits[r2];
        if (!((me >> lx) & 1u)) continue;
        const int i = r2 * CCL_TX + lx;
        const bool a_l = lx > 0 && ((me >> (lx - 1)) & 1u), a_r = lx + 1 < CCL_TX && ((me >> (lx + 1)) & 1u);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int dz = r == 0 ? 0 : 1, dy = r == 0 ? 1 : r - 2;
            const int zz = lz + dz, yy = ly + dy;
            if (zz >= CCL_TZ || yy < 0 || yy >= CCL_TY) continue;
            const int rr = zz * CCL_TY + yy;
            const unsigned int w = rowbits[rr];
            const bool m0 = lx > 0 && ((w >> (lx - 1)) & 1u), m1 = (w >> lx) & 1u, m2 = lx + 1 < CCL_TX && ((w >> (lx + 1)) & 1u);
            const int row = rr * CCL_TX;
            if (m1) {
                if (!(a_l && m0)) lds_union(lab, i, row + lx);          // first voxel of the overlap of the two runs
            } else {
                if (m2 && !a_r) lds_union(lab, i, row + lx + 1);        // my run ends here, the other starts diagonally
                if (m0 && !a_l) lds_union(lab, i, row + lx - 1);        // my run starts here, the other ends diagonally
            }
        }
    }
}

// the tile-local root (an index into the tile) of each of the thread's voxels, -1 for background
__device__ __forceinline__ void ccl_tile_roots(const unsigned int* rowbits, int* lab, int tid, int (&myroot)[CCL_TILE / 256]) {
#pragma unroll
    for (int k = 0; k < CCL_TILE / 256; ++k) {
        const int r2 = (tid >> 5) + 8 * k, lx = tid & 31;
        myroot[k] = -1;
        if ((rowbits[r2] >> lx) & 1u) myroot[k] = lds_find(lab, r2 * CCL_TX + lx);
    }
}

// voxel counts of the local components into cnt (= lab, zeroed by the kernel once every voxel knows its root; a second 32 KiB array
// halved the occupancy: 2.1 -> 4.0 ms per 512^3 mask).  LDS atomics: the per-voxel global atomics of the one-level version were its
// second most expensive part.
__device__ __forceinline__ void ccl_tile_count_runs(unsigned int* cnt, int tid, const int (&myroot)[CCL_TILE / 256]) {
#pragma unroll
    for (int k = 0; k < CCL_TILE / 256; ++k) {
        const int lx = tid & 31;
        // one LDS atomic per run of equal roots in the row (a solid tile would otherwise put 8 192 atomics on one word)
        const int prev = __shfl_up(myroot[k], 1);
        const bool lead = lx == 0 || prev != myroot[k];
        const unsigned int leads = (unsigned int)(__ballot(lead) >> (32 * ((tid >> 5) & 1)));  // this row's half of the wave
        if (lead && myroot[k] >= 0) {
            const unsigned int after = lx == 31 ? 0u : (leads >> (lx + 1));
            const int len = after ? __ffs((int)after) : 32 - lx;
            atomicAdd(&cnt[myroot[k]], (unsigned int)len);
        }
    }
}

// ---- the last pass of a labelling (boa_ccl26, boa_label_blobs6), one thread per voxel i of a 256-thread block -----------------
// after the border unions: every voxel points at its global root; a tile-local root that is not the global root hands its count
// over (one global atomic per tile-local component instead of one per voxel)
__device__ __forceinline__ void ccl_resolve_voxel(size_t i, size_t n, int* L, unsigned int* sizes, int* n_comp) {
    int is_root = 0;
    unsigned int pend_c = 0u;
    int pend_root = 0;
    if (i < n) {
        const int p0 = L[i];
        if (p0 >= 0) {
            int root = p0, p = L[root];
            while (p != root) {
                root = p;
                p = L[root];
            }
            if (root != p0) L[i] = root;
            if (root == (int)i) {
                is_root = 1;
            } else {
                const unsigned int c = sizes[i];
                if (c) {
                    pend_c = c;
                    pend_root = root;
                    // (agent-scope store, not a plain one: the same line may hold a root's count that other XCDs are adding to)
                    __hip_atomic_store(&sizes[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
    // hand the counts over: body-sized masks are ONE giant component, so nearly every tile-local root of the volume adds to the same
    // word -- a device-scope atomic per tile-local component serialises at that address (resolve took 0.2 ms on a mask of scattered
    // specks and 2 ms on a solid one).  Two rounds of wave-level aggregation on the most common root of the wave, then the rest one
    // by one.
    {
        const int lane = threadIdx.x & 63;
#pragma unroll 1
        for (int round = 0; round < 2; ++round) {
            const unsigned long long act = __ballot(pend_c != 0u);
            if (!act) break;
            const int leader = __ffsll((long long)act) - 1;
            const int r0 = __shfl(pend_root, leader);
            const bool mine = pend_c != 0u && pend_root == r0;
            unsigned int sum = mine ? pend_c : 0u;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
            if (lane == leader) atomicAdd(&sizes[r0], sum);
            if (mine) pend_c = 0u;
        }
        if (pend_c) atomicAdd(&sizes[pend_root], pend_c);
    }
    const unsigned long long b = __ballot(is_root);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_comp, __popcll(b));
}

// ---- unions across tile faces (ccl_border_voxel on bytes, cb_border_voxel on mask words and component ids) -----------------------
// The tile pass has made every link between two voxels of one tile, so a voxel only owes the links to its FORWARD neighbours (x + 1 in
// its row, x - 1 / x / x + 1 in the four forward rows) that lie in another tile: voxels on the faces x = 0 (its x - 1 neighbours in
// the later rows), x = TX - 1, y = 0 (the (dz, dy) = (1, -1) row), y = TY - 1 and z = TZ - 1.  Per forward row:
//   * the whole row lies in another tile (z face, or the y face the row is on): a foreground left neighbour sits on the same face and
//     runs this rule too, and has linked itself to x - 2, x - 1, x of that row already, so only x + 1 is new (and only when x is
//     background there: otherwise that row's own x / x + 1 link joins them).  Without a left neighbour one link is enough when
//     consecutive voxels of that row are foreground: x if set, else x - 1 and x + 1 (which then are separate runs of that row);
//   * a row of this tile: its x voxel was linked in LDS and x - 1 / x + 1 hang on it through that row's own links; only when x is
//     background there do x - 1 (from lx = 0) and x + 1 (from lx = TX - 1), which lie in the x-neighbour tiles, need a link.
