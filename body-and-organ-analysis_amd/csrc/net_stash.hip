// The two sliding windows that keep last decoder activations in a stash for the gather head (head_gather.hip): the fused label path
// (boa_net_predict_labels_fold) and the tile-sharded "deferred" path (boa_net_predict_sliding_window_deferred / boa_net_apply_deferred).
// The index logic -- tile grid, walk table, stash layout, deferral plan -- is tile_grid.h.
#include <stdlib.h>

#include <memory>

#include "net.h"

// One gather-head stash: [activations][fp32 ss][packed ss16 of the conv stack][head ss table][walk table] at the offsets `o` from
// `base`.  The context's stash holds every tile of a fold (TileStash), a boa_stash the planes a tile-sharded call kept back.
struct StashView {
    unsigned char* base = nullptr;   // the activations: fp16 chunk planes (fp32 octet planes in the split-precision mode)
    StashOffsets o{};
    int ntile[3] = {0, 0, 0};
    bool x3 = false;                 // split-precision mode: the head reads the fp32 (scale, shift)
    float* ss() const { return (float*)(base + o.ss); }            // [tile][F0][2] fp32 (scale, shift) of the last InstanceNorm
    unsigned* ss16() const { return (unsigned*)(base + o.ss16); }  // the same as the fp16 conv stack packs them
    unsigned* ssp() const { return (unsigned*)(base + o.ssp); }    // [tile][2][16] packed fp16 (scale, shift): the fp16 head's table
    int* tab() const { return (int*)(base + o.tab); }              // walk table (device)
    int tiles() const { return ntile[0] * ntile[1] * ntile[2]; }
    size_t tab_ints(const int PV[3]) const { return walk_table_ints(ntile[0], ntile[1], ntile[2], PV); }
};

// the gather head over a stash of tiles of extent P: everything but what the pass does with the sums
static GatherHead gather_head_on(const boa_net* net, const StashView& v, const int P[3], const int PV[3], const float* w, const float* b,
                                 const uint16_t* gauss) {
    GatherHead g;
    g.act = (const __half*)v.base; g.ssp = v.x3 ? (const unsigned*)v.ss() : v.ssp(); g.dev_tab = v.tab();
    g.tiles_total = v.tiles(); g.x3 = v.x3;
    g.w = w; g.bias = b; g.gauss = gauss; g.C = net->d.num_classes; g.slope = net->d.lrelu_slope;
    for (int a = 0; a < 3; ++a) g.ntile[a] = v.ntile[a], g.P[a] = P[a], g.PV[a] = PV[a];
    return g;
}

// The last decoder activation of EVERY tile of a fold, kept in the context's stash for the gather head (k_gather_head)
struct TileStash {
    StashView v;
    std::vector<int> steps[3];   // tile origins per axis
};

// Keeps the context's tile stash out of boa_trim's reach (an allocation that fails under memory pressure trims, and a trim frees an
// idle stash) from before the tiles are written until the LAST consumer of the TileStash pointers -- the deferred planes' copies, the
// gather head launch -- is queued on the stream; a later trim synchronises the stream before it frees anything.
struct StashHold {
    boa_ctx* c;
    explicit StashHold(boa_ctx* ctx) : c(ctx) { c->stash_busy = true; }
    ~StashHold() { c->stash_busy = false; }
    StashHold(const StashHold&) = delete;
    StashHold& operator=(const StashHold&) = delete;
};

// makes the context's stash at least `need` bytes; BOA_ENOMEM when that does not fit
static int reserve_ctx_stash(boa_ctx* c, size_t need) {
    if (c->stash_bytes >= need) return BOA_OK;
    BOA_HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->stash) hipFree(c->stash);
    c->stash = nullptr;
    c->stash_bytes = 0;
    boa_trim(c);
    // The stash may take a bounded share of what is free NOW ($BOA_STASH_FRAC, default 0.6): what follows the network on this
    // context and on the GPU's other contexts -- fold buffers, post-processing volumes, the second lane, RCCL buffers -- has no
    // fallback of its own, the tile loop has one (BOA_ENOMEM here sends the caller to the scatter form, which needs
    // (C + 1) fp16 planes instead of a tile stash).
    static const double frac = getenv("BOA_STASH_FRAC") ? atof(getenv("BOA_STASH_FRAC")) : 0.6;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && (double)need > frac * (double)fr) {
        boa_set_error("fused sliding window: stash of %zu bytes exceeds %.2f of the %zu free bytes", need, frac, fr);
        return BOA_ENOMEM;
    }
    if (hipMalloc(&c->stash, need) != hipSuccess) {
        (void)hipGetLastError();
        c->stash = nullptr;
        boa_set_error("fused sliding window: %zu bytes of stash do not fit", need);
        return BOA_ENOMEM;
    }
    c->stash_bytes = need;
    return BOA_OK;
}

// runs the conv stack over all tiles (batches of max_batch), the last decoder conv writing straight into the stash slots of its tiles, and
// builds the gather head's walk table.  BOA_ENOMEM when the stash does not fit (the caller falls back to the scatter form).
// (the caller holds c->stash_busy -- StashHold -- until every use of the returned pointers has been queued: boa_trim must not
//  release the stash while tiles are being written into it, nor between this call and the caller's copies / gather launch)
static int net_forward_into_stash(boa_net* net, const float* dev_volume, const int V[3], const int PV[3], const int* off, const int* host_origins,
                                  int n_tiles, TileStash& ts) {
    boa_ctx* c = net->ctx;
    const boa_net_desc& d = net->d;
    grid_origins(host_origins, n_tiles, ts.steps);
    StashView& v = ts.v;
    for (int a = 0; a < 3; ++a) v.ntile[a] = (int)ts.steps[a].size();
    const int F0 = d.features[0];
    const size_t pv = (size_t)d.patch[0] * d.patch[1] * d.patch[2];
    const ActLayout lay = act_layout(net->mode, F0);
    v.o = stash_offsets(lay.tile(n_tiles, pv), n_tiles, F0, true, v.tab_ints(PV));
    BOA_TRY(reserve_ctx_stash(c, v.o.bytes));
    v.base = (unsigned char*)c->stash;
    v.x3 = lay.esz == 4;   // split-precision mode: the stash holds the fp32 octet planes
    ConvLayer& last = net->dec.back().back();
    void* keep_act = last.act;
    float* keep_ss = last.ss;
    unsigned* keep_ss16 = last.ss16;
    int rc = BOA_OK;
    for (int t0 = 0; t0 < n_tiles && rc == BOA_OK; t0 += net->maxN) {
        const int nb = std::min(net->maxN, n_tiles - t0);
        // the last decoder conv of this batch writes straight into the stash slots of its tiles
        last.act = v.base + lay.tile(t0, pv);
        last.ss = v.ss() + (size_t)t0 * F0 * 2;
        last.ss16 = keep_ss16 ? v.ss16() + (size_t)t0 * F0 : nullptr;
        rc = net_forward_stack(net, dev_volume, V, off, host_origins + (size_t)t0 * 3, nb);
    }
    last.act = keep_act;
    last.ss = keep_ss;
    last.ss16 = keep_ss16;
    if (rc) return rc;
    if (!v.x3) BOA_TRY(launch_pack_head_ss(c, v.ss(), v.ssp(), n_tiles));
    const std::vector<int> tab = walk_table(ts.steps[0], ts.steps[1], ts.steps[2], d.patch, PV);
    BOA_REQUIRE(tab.size() == v.tab_ints(PV), "walk table: %zu ints, %zu reserved", tab.size(), v.tab_ints(PV));
    BOA_HIP_TRY(hipMemcpyAsync(v.tab(), tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    BOA_HIP_TRY(hipStreamSynchronize(c->stream));   // (the table is a stack-lifetime host vector)
    c->prof_break = true;
    return BOA_OK;
}

// ------------------------------------------------------------------------------------------------------
// Fused sliding window -> labels (head_gather.hip): the conv stack writes the last decoder activation of EVERY tile of the
// volume into the context's stash, then one gather pass per fold walks the volume.  Conditions (else the caller uses
// boa_net_predict_sliding_window + boa_finalize_labels): production or split-precision mode, no test-time mirroring, features[0] == 32,
// <= 32 classes, tile origins = the full cartesian grid of per-axis steps in canonical (x outer, z inner) order.
extern "C" int boa_net_labels_supported(boa_net* net, const int* host_origins, int n_tiles) {
    if (!net || !host_origins) return 0;
    // (record planes -- not fp32_ref's channels-last records --, patch z extent a multiple of 32 and <= 31 classes: the shapes for which
    //  the scatter loop's head runs on the matrix cores too, so that the label path and the logits API share one head arithmetic)
    if (!act_layout(net->mode, net->d.features[0]).planar || net->mirror_mask != 0 || net->d.features[0] != 32 || net->d.num_classes > 31 || net->d.patch[2] % 32 != 0) return 0;
    std::vector<int> steps[3];
    return grid_origins(host_origins, n_tiles, steps) ? 1 : 0;
}

extern "C" int boa_net_predict_labels_fold(boa_net* net, const float* dev_volume, const int V[3], const int PV[3], const int* vol_off,
                                           const int* host_origins, int n_tiles, const uint16_t* dev_gauss, uint16_t* dev_fold,
                                           int fold_index, int n_folds, const uint8_t* host_lut, int merge, uint8_t* dev_labels_out,
                                           const int* crop_off, const int* crop_dims, int* dev_inf_flag) {
    BOA_REQUIRE(net && dev_volume && V && PV && host_origins && dev_inf_flag, "boa_net_predict_labels_fold: NULL argument");
    BOA_REQUIRE(boa_net_labels_supported(net, host_origins, n_tiles), "boa_net_predict_labels_fold: unsupported network / tile layout");
    BOA_TRY(net_bind_arena(net));
    BOA_REQUIRE(n_folds >= 1 && fold_index >= 0 && fold_index < n_folds && (n_folds == 1 || dev_fold), "boa_net_predict_labels_fold: folds");
    BOA_REQUIRE(fold_index + 1 < n_folds || dev_labels_out, "boa_net_predict_labels_fold: the last fold needs the label buffer");
    const int zero[3] = {0, 0, 0};
    const int* off = vol_off ? vol_off : zero;
    BOA_TRY(check_padded(net, V, PV, off, "fused sliding window"));
    TileStash ts;
    StashHold hold(net->ctx);   // until launch_gather_head below is queued
    BOA_TRY(net_forward_into_stash(net, dev_volume, V, PV, off, host_origins, n_tiles, ts));
    GatherHead g = gather_head_on(net, ts.v, net->d.patch, PV, net->head_w, net->head_b, dev_gauss);
    g.fold_mode = n_folds == 1 ? FoldMode::Single : fold_index == 0 ? FoldMode::First : fold_index + 1 == n_folds ? FoldMode::Last : FoldMode::Middle;
    g.n_folds = n_folds; g.fold = dev_fold; g.inf_flag = dev_inf_flag;
    g.host_lut = host_lut; g.merge = merge; g.labels = dev_labels_out; g.crop_off = crop_off; g.crop_dims = crop_dims;
    return launch_gather_head(net->ctx, g);
}

// ------------------------------------------------------------------------------------------------------
// tile-sharded sliding window (several GPUs on one volume): the rank that owns tile rows [b0, b1) along
// axis 0 cannot add the first `defer` planes of its row-b0 tiles before the lower rank's partial sums for those
// planes have arrived (the reference's fp16 `+=` runs in ascending tile order per voxel).  The head input of those
// planes is kept in a stash and applied afterwards; everything else is accumulated at once.
struct boa_stash {
    boa_ctx* ctx = nullptr;
    unsigned char* arena = nullptr;
    // head weights of the weight set that produced the stashed activations: the stash may be applied after the network has
    // switched to the next fold's weights (the exchange of fold f overlaps the tiles of fold f + 1); the sets are cached device
    // arenas (boa_net::wsets), so the pointers outlive the switch
    const float* head_w = nullptr;
    const float* head_b = nullptr;
    // scatter form: per deferring tile its first `planes` planes and its (scale, shift) table, applied by one scatter head each
    struct Item {
        size_t act_off, ss_off;
        int planes;
        int start[3];
    };
    std::vector<Item> items;
    // gather form (the call ran the gather head): the first dp planes of every deferring tile (the block's first tile row; with steps
    // below half a patch also the rows behind it, which defer fewer planes) as a gather-head stash `v` of tiles of dp planes in the
    // arena, so that boa_net_apply_deferred is ONE more k_gather_head launch over planes [x0, x_split), started from the lower rank's sums
    bool gather = false;
    StashView v;
    int dp = 0, x0 = 0, x_split = 0;
};

extern "C" void boa_stash_destroy(boa_stash* st) {
    if (!st) return;
    if (st->arena) boa_free(st->ctx, st->arena);
    delete st;
}

// what one deferred call shares between its two forms
struct DeferredCall {
    boa_net* net;
    const float* volume;
    const int *V, *PV, *off, *origins;
    int n_tiles;
    const uint16_t* gauss;
    uint16_t *acc, *nacc;
    const int* defer;   // planes to keep back, per tile
};

// the deferred planes of the stashed tiles `ts` in the gather head's layout, in st.arena: every deferring tile keeps dp0 planes (the later
// rows more than they defer: valid planes of the tile, never visited by the launch over [x0, x_split))
static int keep_deferred_planes(const DeferredCall& k, const DeferPlan& plan, const TileStash& ts, boa_stash& st) {
    boa_net* net = k.net;
    boa_ctx* c = net->ctx;
    const boa_net_desc& d = net->d;
    const int F = d.features[0], n_def = plan.n_def;
    const size_t plane = (size_t)d.patch[1] * d.patch[2], pv = d.patch[0] * plane;
    const ActLayout lay = act_layout(net->mode, F);
    StashView& v = st.v;
    BOA_TRY(boa_malloc(c, v.o.bytes, (void**)&st.arena));
    v.base = st.arena;
    BOA_REQUIRE(n_def == v.tiles(), "deferred sliding window: %d deferred tiles in %d rows of %d x %d", n_def, v.ntile[0], v.ntile[1], v.ntile[2]);
    const size_t item_act = lay.bytes((size_t)plan.dp0 * plane);
    bool ok_copy = true;
    int item = 0;
    for (int i = 0; i < k.n_tiles && ok_copy; ++i) {
        if (k.defer[i] == 0) continue;
        ok_copy = lay.copy_head(v.base + (size_t)item * item_act, ts.v.base + lay.tile(i, pv), plan.dp0, plane, pv, c->stream) == hipSuccess;
        ok_copy = ok_copy && hipMemcpyAsync(v.ss() + (size_t)item * F * 2, ts.v.ss() + (size_t)i * F * 2, (size_t)F * 2 * sizeof(float),
                                            hipMemcpyDeviceToDevice, c->stream) == hipSuccess;
        ++item;
    }
    if (!ok_copy) {
        boa_set_error("deferred sliding window: stash copy failed");
        return BOA_EHIP;
    }
    if (!v.x3) BOA_TRY(launch_pack_head_ss(c, v.ss(), v.ssp(), n_def));
    // walk table of the deferring tile rows with dp0 planes per tile
    const int ext[3] = {plan.dp0, d.patch[1], d.patch[2]};
    const std::vector<int> tab = walk_table(plan.def_rows, ts.steps[1], ts.steps[2], ext, k.PV);
    BOA_REQUIRE(tab.size() == v.tab_ints(k.PV), "walk table: %zu ints, %zu reserved", tab.size(), v.tab_ints(k.PV));
    if (hipMemcpyAsync(v.tab(), tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {   // (the table is a stack-lifetime host vector)
        boa_set_error("deferred sliding window: walk table copy failed");
        return BOA_EHIP;
    }
    return BOA_OK;
}

// Gather form (the product path when the network / tile grid allow it, as in boa_net_predict_labels_fold): every tile's last
// activation goes to the context's stash, the planes to defer are copied out of it, and ONE k_gather_head launch in raw mode
// writes the partial sums of all other planes of this rank -- [x_split, end of its last row) -- instead of one accumulator
// read-modify-write per covering tile.  The planes below x_split are exactly the deferred ones (plan.consistent) and all belong to
// the block's first tile rows: they stay untouched until boa_net_apply_deferred adds them, with the same kernel, on top of the
// lower rank's sums.  Same head arithmetic for every tile (the matrix-core head), whatever the tile origins' alignment.
// *done = false (and BOA_OK) when the stash does not fit or the pattern is unusual: the caller runs the scatter form.
static int deferred_gather(const DeferredCall& k, const DeferPlan& plan, boa_stash& st, bool* done) {
    boa_net* net = k.net;
    boa_ctx* c = net->ctx;
    const boa_net_desc& d = net->d;
    *done = false;
    TileStash ts;
    StashHold hold(c);   // across the arena allocation (it may trim), the stash copies and the raw gather launch
    const int grc = plan.consistent ? net_forward_into_stash(net, k.volume, k.V, k.PV, k.off, k.origins, k.n_tiles, ts) : BOA_ENOMEM;
    if (grc != BOA_OK) return grc == BOA_ENOMEM ? BOA_OK : grc;
    st.gather = true; st.dp = plan.dp0; st.x0 = plan.x0; st.x_split = plan.x_split;
    StashView& v = st.v;
    v.x3 = ts.v.x3;
    v.ntile[0] = (int)plan.def_rows.size(); v.ntile[1] = ts.v.ntile[1]; v.ntile[2] = ts.v.ntile[2];
    v.o = stash_offsets((size_t)plan.n_def * act_layout(net->mode, d.features[0]).bytes((size_t)plan.dp0 * d.patch[1] * d.patch[2]), plan.n_def,
                        d.features[0], false, v.tab_ints(k.PV));
    if (plan.n_def > 0) BOA_TRY(keep_deferred_planes(k, plan, ts, st));
    c->prof_break = true;
    GatherHead g = gather_head_on(net, ts.v, d.patch, k.PV, net->head_w, net->head_b, k.gauss);
    g.fold_mode = FoldMode::Raw; g.fold = k.acc; g.raw_n = k.nacc;
    g.x_lo = plan.x_split; g.x_hi = std::min(plan.x_end, k.PV[0]);
    BOA_TRY(launch_gather_head(c, g));
    *done = true;
    return BOA_OK;
}

// Scatter form: per batch the conv stack, then per tile the copy of its deferred planes into st.items' slots and the scatter head on the rest
static int deferred_scatter(const DeferredCall& k, boa_stash& st, size_t bytes) {
    boa_net* net = k.net;
    boa_ctx* c = net->ctx;
    const boa_net_desc& d = net->d;
    const int F = d.features[0];
    const size_t plane = (size_t)d.patch[1] * d.patch[2], pv = d.patch[0] * plane;
    const ActLayout lay = act_layout(net->mode, F);
    if (bytes) BOA_TRY(boa_malloc(c, bytes, (void**)&st.arena));
    size_t item = 0;
    for (int t0 = 0; t0 < k.n_tiles; t0 += net->maxN) {
        const int nb = std::min(net->maxN, k.n_tiles - t0);
        BOA_TRY(net_forward_stack(net, k.volume, k.V, k.off, k.origins + (size_t)t0 * 3, nb));
        const ConvLayer& last = net->dec.back().back();
        for (int i = 0; i < nb; ++i) {
            const int* stt = k.origins + (size_t)(t0 + i) * 3;
            const int dp = k.defer[t0 + i];
            if (dp > 0) {
                const boa_stash::Item& it = st.items[item++];
                // the first dp axis-0 planes in the stash, with its own plane stride (dp * plane voxels)
                if (lay.copy_head(st.arena + it.act_off, (const unsigned char*)last.act + lay.tile(i, pv), dp, plane, pv, c->stream) != hipSuccess ||
                    hipMemcpyAsync(st.arena + it.ss_off, last.ss + (size_t)i * F * 2, (size_t)F * 2 * 4, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) {
                    boa_set_error("deferred sliding window: stash copy failed");
                    return BOA_EHIP;
                }
                c->prof_break = true;
            }
            if (dp < d.patch[0]) {
                const int P[3] = {d.patch[0] - dp, d.patch[1], d.patch[2]};
                const int s2[3] = {stt[0] + dp, stt[1], stt[2]};
                BOA_TRY(net_head(net, i, P, dp, nullptr, k.gauss ? k.gauss + (size_t)dp * plane : nullptr, k.acc, k.nacc, k.PV, s2));
            }
        }
    }
    return BOA_OK;
}

extern "C" int boa_net_predict_sliding_window_deferred(boa_net* net, const float* dev_volume, const int V[3], const int PV[3], const int* vol_off,
                                                       const int* host_origins, int n_tiles, const uint16_t* dev_gauss, uint16_t* dev_acc,
                                                       uint16_t* dev_n, const int* host_defer_planes, boa_stash** stash_out) {
    BOA_REQUIRE(net && dev_volume && V && PV && host_origins && dev_acc && dev_n && host_defer_planes && stash_out,
                "boa_net_predict_sliding_window_deferred: NULL argument");
    BOA_TRY(net_bind_arena(net));
    const boa_net_desc& d = net->d;
    BOA_REQUIRE(net->mirror_mask == 0, "deferred sliding window (tile sharding) is not available with test-time mirroring");
    const int zero[3] = {0, 0, 0};
    const int* off = vol_off ? vol_off : zero;
    BOA_TRY(check_padded(net, V, PV, off, "sliding window"));
    const int F = d.features[0];
    const size_t plane = (size_t)d.patch[1] * d.patch[2];
    const ActLayout lay = act_layout(net->mode, F);
    std::unique_ptr<boa_stash, void (*)(boa_stash*)> st(new boa_stash, boa_stash_destroy);
    st->ctx = net->ctx;
    st->head_w = net->head_w;
    st->head_b = net->head_b;
    size_t bytes = 0;   // of the scatter form's arena
    for (int i = 0; i < n_tiles; ++i) {
        const int dp = host_defer_planes[i];
        BOA_REQUIRE(dp >= 0 && dp <= d.patch[0], "deferred sliding window: tile %d defers %d planes of %d", i, dp, d.patch[0]);
        if (dp == 0) continue;
        boa_stash::Item it;
        it.act_off = bytes;
        bytes += align256(lay.bytes((size_t)dp * plane));
        it.ss_off = bytes;
        bytes += 256 * ((F * 2 * 4 + 255) / 256);
        it.planes = dp;
        for (int a = 0; a < 3; ++a) it.start[a] = host_origins[(size_t)i * 3 + a];
        st->items.push_back(it);
    }
    const DeferredCall k{net, dev_volume, V, PV, off, host_origins, n_tiles, dev_gauss, dev_acc, dev_n, host_defer_planes};
    bool done = false;
    if (n_tiles > 0 && boa_net_labels_supported(net, host_origins, n_tiles))
        BOA_TRY(deferred_gather(k, defer_plan(host_origins, host_defer_planes, n_tiles, d.patch[0]), *st, &done));
    if (!done) BOA_TRY(deferred_scatter(k, *st, bytes));
    *stash_out = st.release();
    return BOA_OK;
}

extern "C" int boa_net_apply_deferred(boa_net* net, const boa_stash* st, const uint16_t* dev_gauss, uint16_t* dev_acc,
                                      uint16_t* dev_n, const int PV[3]) {
    BOA_REQUIRE(net && st && dev_acc && dev_n && PV, "boa_net_apply_deferred: NULL argument");
    const boa_net_desc& d = net->d;
    if (st->gather) {
        if (st->v.tiles() == 0) return BOA_OK;
        const int P[3] = {st->dp, d.patch[1], d.patch[2]};
        GatherHead g = gather_head_on(net, st->v, P, PV, st->head_w, st->head_b, dev_gauss);
        g.fold_mode = FoldMode::Raw; g.fold = dev_acc; g.raw_n = dev_n; g.raw_init = 1;
        g.x_lo = st->x0; g.x_hi = std::min(st->x_split, PV[0]);
        return launch_gather_head(net->ctx, g);
    }
    const ActLayout lay = act_layout(net->mode, d.features[0]);
    for (const boa_stash::Item& it : st->items) {  // the stash keeps the canonical tile order
        int P[3] = {it.planes, d.patch[1], d.patch[2]};
        BOA_TRY(scatter_head(net, st->arena + it.act_off, (const float*)(st->arena + it.ss_off), P,
                             lay.plane_stride((size_t)it.planes * d.patch[1] * d.patch[2]), st->head_w, st->head_b, nullptr, dev_gauss,
                             dev_acc, dev_n, PV, it.start));
    }
    return BOA_OK;
}
