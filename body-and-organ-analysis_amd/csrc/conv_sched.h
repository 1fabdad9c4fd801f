// Tile schedule of the persistent convs (k_conv_ws, k_conv_ns): the host-side arithmetic and the tables conv_sched.hip keeps per context.
// A sample's tiles (decode_tile's order, conv_ws_dev.h) are cut into `vw` contiguous runs, one per virtual workgroup; `grid` physical
// workgroups execute the N * vw virtual ones b, b + grid, ... and read their tile sequence from a descriptor row.  Plain C++17 without
// HIP, so that tools/conv_sched_host.cpp runs it under the host compiler's sanitizers (tests/test_conv_sched_host_cpu.py): a
// descriptor row shorter than a workgroup's tile count is otherwise caught only by the host check of a launch on the GPU.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <array>
#include <deque>
#include <vector>

// virtual workgroups per sample (a function of the layer geometry only) and the statistics slots of a layer: one per (virtual
// workgroup, consumer wave) -- sized per layer, so that k_norm_finalize reads and re-zeroes 4 vw entries per (n, cout), not 4 x CUs
// (the deep layers have 10-64 tiles per sample)
inline int conv_ws_vw(int tiles_per_sample, int cu_count) { return std::min(tiles_per_sample, cu_count); }
inline int conv_ws_nslots(int tiles_per_sample, int cu_count) { return conv_ws_vw(tiles_per_sample, cu_count) * 4; }

// physical workgroups of a launch of N samples
inline int conv_sched_grid(int vw, int N, int cu_count) { return (int)std::min<long long>((long long)vw * N, cu_count); }

// what the tile order depends on: spatial tiles per axis, a tile's output extent per axis, cout groups per spatial tile and whether the
// cout group is the fastest index (ConvArgs: t*, b* x w*, ncy, cy_fast)
struct ConvSchedGeom {
    int t[3], ext[3], ncy, cy_fast;
};

// Run table of a layer: the tiles of ONE sample (decode_tile's order) cut into vw contiguous runs, 8 XCD ranges first
// (virtual workgroup j <-> XCD j % 8) and then the virtual workgroups of an XCD; entry j = {count, cy, sp, ox0, oy0, oz0, -, -}
// of the run's first tile.  A function of the layer geometry only (never of the batch size).
inline std::vector<int> conv_sched_runs(const ConvSchedGeom& g, int tiles_per_sample, int vw) {
    std::vector<int> tab((size_t)vw * 8, 0);
    const int nsp = g.t[0] * g.t[1] * g.t[2];
    for (int j = 0; j < vw; ++j) {
        int first, count;
        if (vw % 8 != 0) {
            const int q = tiles_per_sample / vw, r = tiles_per_sample % vw;
            first = j * q + std::min(j, r);
            count = q + (j < r ? 1 : 0);
        } else {
            const int xcd = j & 7, slot = j >> 3, per = vw >> 3;
            const int q = tiles_per_sample / 8, rem = tiles_per_sample % 8;
            const int lo = xcd * q + std::min(xcd, rem), len = q + (xcd < rem ? 1 : 0);
            const int cq = len / per, cr = len % per;
            first = lo + slot * cq + std::min(slot, cr);
            count = cq + (slot < cr ? 1 : 0);
        }
        const int cy = g.cy_fast ? first % g.ncy : first / nsp, sp = g.cy_fast ? first / g.ncy : first % nsp;
        const int tx = sp % g.t[0], tz = sp / g.t[0] % g.t[2], ty = sp / g.t[0] / g.t[2];
        int* e = &tab[(size_t)j * 8];
        e[0] = count; e[1] = cy; e[2] = sp; e[3] = tx * g.ext[0]; e[4] = ty * g.ext[1]; e[5] = tz * g.ext[2];
    }
    return tab;
}

// Entries (of 8 ints) of a descriptor row: entry 0 + an upper bound of a workgroup's tiles.  A run has at most tiles_per_sample / vw + 2
// tiles (the 8 XCD ranges differ by one tile, the runs inside a range by one more) and a workgroup executes ceil(N vw / grid) runs.
inline int conv_sched_desc_row(int N, int vw, int grid, int tiles_per_sample) {
    return (N * vw + grid - 1) / grid * (tiles_per_sample / vw + 2) + 1;
}

// tiles physical workgroup b walks: the runs of the virtual workgroups b, b + grid, ... (the loop of k_ws_build_desc)
inline long long conv_sched_wg_tiles(const std::vector<int>& runs, int vw, int N, int grid, int b) {
    long long my = 0;
    for (long long v = b; v < (long long)N * vw; v += grid) my += runs[(size_t)(v % vw) * 8];
    return my;
}

// ---- the tables of a context (built, looked up and released by conv_sched.hip alone) ---------------------------------------------------
// one per layer geometry, kept for the life of the context
struct ConvRunTable {
    std::array<int, 13> key;
    std::vector<int> host;
    int* dev;
};
// one per (layer geometry, batch, grid): the tail batches of differently sized volumes keep adding some, boa_trim releases them
struct ConvDescTable {
    const ConvRunTable* runs;   // its layer geometry (entries of a deque: never moved)
    std::array<int, 18> key;    // batch, grid and what the descriptors hold beyond the run table's key
    int* dev;
    size_t bytes;
};
struct ConvSchedTables {
    std::deque<ConvRunTable> runs;
    std::vector<ConvDescTable> desc;
};
