// Host-side index logic of the stash-based sliding windows (net_stash.hip): the tile grid of a fold, the gather head's walk table, the
// byte layout of a stash and the deferral plan of a tile-sharded call.  Plain C++17 without HIP, so that tools/tile_grid_host.cpp runs
// it under the host compiler's sanitizers (tests/test_tile_grid_host_cpu.py): an off-by-one here lets k_gather_head read a
// neighbouring tile's records.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <vector>

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Tile origins [n][3] = the full cartesian grid of per-axis steps in canonical (x outer, z inner) order, fewer than 256 steps per
// axis?  Leaves the steps per axis in `steps`.
inline bool grid_origins(const int* o, int n, std::vector<int> (&steps)[3]) {
    for (int a = 0; a < 3; ++a) steps[a].clear();
    if (n < 1) return false;
    // canonical order: the last axis varies fastest
    for (int t = 0; t < n && (t == 0 || o[t * 3 + 2] > o[(t - 1) * 3 + 2]); ++t) steps[2].push_back(o[t * 3 + 2]);
    const int n2 = (int)steps[2].size();
    if (n % n2) return false;
    for (int t = 0; t < n; t += n2) {
        if (t > 0 && o[t * 3 + 1] <= o[(t - n2) * 3 + 1]) break;
        steps[1].push_back(o[t * 3 + 1]);
    }
    const int n1 = (int)steps[1].size();
    if (n % (n1 * n2)) return false;
    for (int t = 0; t < n; t += n1 * n2) steps[0].push_back(o[t * 3]);
    const int n0 = (int)steps[0].size();
    if ((long long)n0 * n1 * n2 != n) return false;
    for (int a = 0; a < 3; ++a)
        for (size_t i = 1; i < steps[a].size(); ++i)
            if (steps[a][i] <= steps[a][i - 1]) return false;
    for (int t = 0; t < n; ++t) {
        const int iz = t % n2, iy = (t / n2) % n1, ix = t / (n1 * n2);
        if (o[t * 3] != steps[0][ix] || o[t * 3 + 1] != steps[1][iy] || o[t * 3 + 2] != steps[2][iz]) return false;
    }
    return n0 < 256 && n1 < 256 && n2 < 256;
}

// ints of the walk table of n0 x n1 x n2 tiles in a padded volume PV
inline size_t walk_table_ints(int n0, int n1, int n2, const int PV[3]) {
    return (size_t)n0 + n1 + n2 + PV[0] + PV[1] + (PV[2] + 31) / 32;
}

// The gather head's walk table: the tile origins per axis, then per coordinate the first covering tile and the count (x, y), per
// 32-voxel z run the tiles that intersect the run, as `first | count << 8` (a tile at origin o covers [o, o + ext[a]) along axis a)
inline std::vector<int> walk_table(const std::vector<int>& s0, const std::vector<int>& s1, const std::vector<int>& s2, const int ext[3],
                                   const int PV[3]) {
    const std::vector<int>* steps[3] = {&s0, &s1, &s2};
    std::vector<int> tab;
    for (const std::vector<int>* s : steps) tab.insert(tab.end(), s->begin(), s->end());
    auto cover = [&](int a, int lo, int hi) {
        const std::vector<int>& st = *steps[a];
        int first = 0, cnt = 0;
        for (size_t i = 0; i < st.size(); ++i)
            if (st[i] <= hi && st[i] + ext[a] > lo) {
                if (!cnt) first = (int)i;
                ++cnt;
            }
        return first | (cnt << 8);
    };
    for (int x = 0; x < PV[0]; ++x) tab.push_back(cover(0, x, x));
    for (int y = 0; y < PV[1]; ++y) tab.push_back(cover(1, y, y));
    for (int zb = 0; zb < PV[2]; zb += 32) tab.push_back(cover(2, zb, std::min(zb + 31, PV[2] - 1)));
    return tab;
}

// byte offsets of a gather-head stash's sub-buffers after act_bytes of activations -- fp32 (scale, shift), their fp16 form as the conv
// stack packs it (only when `ss16`), the head's packed table, the walk table -- and its size
struct StashOffsets {
    size_t ss, ss16, ssp, tab, bytes;
};

inline StashOffsets stash_offsets(size_t act_bytes, int n_tiles, int F, bool ss16, size_t tab_ints) {
    StashOffsets o;
    o.ss = align256(act_bytes);
    o.ss16 = align256(o.ss + (size_t)n_tiles * F * 2 * sizeof(float));
    o.ssp = ss16 ? align256(o.ss16 + (size_t)n_tiles * F * sizeof(unsigned)) : o.ss16;
    o.tab = align256(o.ssp + (size_t)n_tiles * 32 * sizeof(unsigned));
    o.bytes = align256(o.tab + tab_ints * sizeof(int));
    return o;
}

// The deferral pattern of a tile-sharded call (defer[i] leading axis-0 planes of tile i wait for the lower rank), as the gather form
// needs it.  dp0 = the deepest deferral (the block's first row, at x0); rows that start further up defer fewer planes -- actual steps
// below half a patch make the block's second row reach the lower block's last row too.  `consistent`: every deferring tile ends its
// deferral at the same plane x_split, none starts below x0, and every tile defers exactly its planes below x_split; the launch over
// [x_split, x_end) then leaves exactly the deferred planes out.
struct DeferPlan {
    int x0 = 0, x_split = -1, x_end = 0, dp0 = 0, n_def = 0;
    std::vector<int> def_rows;   // origins of the tile rows that defer, ascending in a consistent pattern
    bool consistent = true;
};

inline DeferPlan defer_plan(const int* origins, const int* defer, int n_tiles, int patch0) {
    DeferPlan p;
    if (n_tiles < 1) return p;
    int x_first = origins[0];
    for (int i = 0; i < n_tiles; ++i) {
        const int xo = origins[(size_t)i * 3], dpi = defer[i];
        x_first = std::min(x_first, xo);
        p.x_end = std::max(p.x_end, xo + patch0);
        if (dpi > 0) {
            if (p.n_def == 0) {
                p.dp0 = dpi;
                p.x0 = xo;
                p.x_split = xo + dpi;
            }
            p.consistent = p.consistent && xo + dpi == p.x_split && xo >= p.x0;   // all end at the same plane (canonical order: x0 first)
            if (p.def_rows.empty() || p.def_rows.back() != xo) p.def_rows.push_back(xo);
            ++p.n_def;
        }
    }
    if (p.x_split < 0) p.x_split = x_first;
    for (int i = 0; i < n_tiles; ++i) {   // every tile that reaches below x_split defers exactly its planes below x_split
        const int below = std::max(0, std::min(p.x_split - origins[(size_t)i * 3], patch0));
        p.consistent = p.consistent && defer[i] == below;
    }
    return p;
}
