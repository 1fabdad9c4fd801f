// Tile schedule of a k_conv_ws / k_conv_ns launch: the launchers' shared prologue (conv_sched_prepare), the per-context cache of run and
// descriptor tables with the kernel that builds the latter, and the BOA_WS_TRACE buffer.  The arithmetic and the table types are
// conv_sched.h; the device-side walk is conv_ws_dev.h.
#include <stdlib.h>

#include "conv.h"
#include "conv_ws_dev.h"

// Builds the descriptor rows of a launch: thread b walks physical workgroup b's tile sequence with the kernels' own code.
__global__ __launch_bounds__(64) void k_ws_build_desc(ConvArgs p, int grid, int row, int* __restrict__ out) {
    const int b = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (b >= grid) return;
    int* r = out + (size_t)b * row * 8;
    int my = 0;
    for (int v = b; v < p.N * p.vw; v += grid) my += p.runs[(v % p.vw) * 8];
    if (my > row - 1) my = row - 1;   // (unreachable: desc_table checks every workgroup's tile count against the row length on the host before the launch)
    r[0] = my;
    for (int i = 1; i < 8; ++i) r[i] = 0;
    TileSeq s;
    s.n = s.left = s.j = 0;
    for (int k = 0; k < my; ++k) {
        bool new_run = true;
        if (k == 0)
            seq_first_of(p, s, b);
        else
            new_run = seq_next(p, s);
        const TileDesc d = make_desc(p, s, new_run);
        int* e = r + (size_t)(k + 1) * 8;
        e[0] = d.tc.n; e[1] = d.tc.cy; e[2] = d.tc.ox0; e[3] = d.tc.oy0; e[4] = d.tc.oz0; e[5] = d.flags; e[6] = d.vo; e[7] = d.ibase;
    }
}

// ---- the cache ------------------------------------------------------------------------------------------------------------------------
// Both kinds are allocated with boa_malloc_raw BEFORE they enter the cache and with no reference into `desc` held: a failed allocation
// trims the context, which releases every descriptor table.
size_t conv_sched_desc_bytes(const boa_ctx* c) {
    size_t n = 0;
    for (const ConvDescTable& e : c->sched.desc) n += e.bytes;
    return n;
}

void conv_sched_release_desc(boa_ctx* c) {
    for (ConvDescTable& e : c->sched.desc) hipFree(e.dev);
    c->sched.desc.clear();
}

void conv_sched_destroy(boa_ctx* c) {
    conv_sched_release_desc(c);
    for (ConvRunTable& e : c->sched.runs) hipFree(e.dev);
    c->sched.runs.clear();
}

// the run table of a's layer geometry (a.ncy, a.cy_fast and vw set); the copy is synchronous: the table is complete on return
static const ConvRunTable* run_table(boa_ctx* ctx, const ConvArgs& a, int tiles_per_sample, int vw) {
    const std::array<int, 13> key = {a.t0, a.t1, a.t2, a.b0, a.b1, a.b2, a.w0, a.w1, a.w2, a.Cout, a.cy_fast, vw, a.ncy};
    for (const ConvRunTable& e : ctx->sched.runs)
        if (e.key == key) return &e;
    const ConvSchedGeom g = {{a.t0, a.t1, a.t2}, {a.b0 * a.w0, a.b1 * a.w1, a.b2 * a.w2}, a.ncy, a.cy_fast};
    std::vector<int> tab = conv_sched_runs(g, tiles_per_sample, vw);
    void* dev = nullptr;
    if (boa_malloc_raw(ctx, tab.size() * sizeof(int), &dev) != BOA_OK) return nullptr;
    if (hipMemcpy(dev, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(dev);
        return nullptr;
    }
    ctx->sched.runs.push_back({key, std::move(tab), (int*)dev});
    return &ctx->sched.runs.back();
}

// Descriptor table of a launch (WS_DESC): a function of the layer geometry, the batch and the grid; built once per key on the device by
// k_ws_build_desc, on ctx->stream ahead of the conv (8 samples of the 128^3 layers: 32 768 tiles = 1 MiB; <= ~150 MB for every batch
// size 1 .. 25 of one net geometry).  a.runs / a.vw are set: the builder walks them.
static const int* desc_table(boa_ctx* ctx, const ConvArgs& a, const ConvRunTable* rt, int tiles_per_sample, int grid, int row, const char* what) {
    const std::array<int, 18> key = {a.N, grid, a.Do, a.Ho, a.Wo, a.Di, a.Hi, a.Wi, a.s0, a.s1, a.s2, a.p0, a.p1, a.p2, a.h0, a.h1, a.h2, a.xs};
    for (const ConvDescTable& e : ctx->sched.desc)
        if (e.runs == rt && e.key == key) return e.dev;
    // the row length is an upper bound of every workgroup's tile count: checked here against the host copy of the run table, so the
    // builder kernel can neither truncate a row nor write past it (an error return instead of a device trap)
    for (int b = 0; b < grid; ++b) {
        const long long my = conv_sched_wg_tiles(rt->host, a.vw, a.N, grid, b);
        if (my > row - 1) {
            boa_set_error("%s: workgroup %d walks %lld tiles, descriptor rows hold %d", what, b, my, row - 1);
            return nullptr;
        }
    }
    void* dev = nullptr;
    const size_t bytes = (size_t)grid * row * 8 * sizeof(int);
    if (boa_malloc_raw(ctx, bytes, &dev) != BOA_OK) {
        boa_set_error("%s: could not allocate the tile descriptor table", what);
        return nullptr;
    }
    hipLaunchKernelGGL(k_ws_build_desc, dim3((grid + 63) / 64), dim3(64), 0, ctx->stream, a, grid, row, (int*)dev);
    ctx->sched.desc.push_back({rt, key, (int*)dev, bytes});
    return (const int*)dev;
}

// ---- BOA_WS_TRACE (traced build only) -------------------------------------------------------------------------------------------------
#ifdef WS_WITH_TRACE
static void trace_arm(boa_ctx* ctx, ConvArgs& a, int grid) {
    static const char* env = getenv("BOA_WS_TRACE");
    if (!env || hipMalloc(&a.trace, WS_TRACE_SLOTS * 8) != hipSuccess) return;
    hipMemsetAsync(a.trace, 0, WS_TRACE_SLOTS * 8, ctx->stream);
    const unsigned long long blk = (unsigned long long)std::min(std::max(atoi(env), 0), grid - 1);
    hipMemcpyAsync(a.trace + WS_TRACE_SLOTS - 5, &blk, 8, hipMemcpyHostToDevice, ctx->stream);
    hipStreamSynchronize(ctx->stream);
}

// per-event deltas (cycles) of the traced block: consumer wave 0, then producer wave 4
static void trace_row(const unsigned long long* h, int lo, int hi) {
    for (int i = lo; i < hi && h[i]; ++i)
        fprintf(stderr, " %d:%llu", (int)(h[i] >> 56), (h[i] & 0x00ffffffffffffffull) - (h[i - 1] & 0x00ffffffffffffffull));
}

void conv_sched_trace_dump(boa_ctx* ctx, const ConvArgs& a, const ConvSched& s, int tiles_per_sample, int R) {
    if (!a.trace) return;
    static unsigned long long host[WS_TRACE_SLOTS];
    hipStreamSynchronize(ctx->stream);
    hipMemcpy(host, a.trace, sizeof(host), hipMemcpyDeviceToHost);
    hipFree(a.trace);
    const unsigned long long* hp = host + WS_TRACE_SLOTS / 2;
    const int cin = a.C0 + a.C1;
    if (R == 0) {
        fprintf(stderr, "[ns-trace] Cin=%d Cout=%d in=%d s=%d:", cin, a.Cout, a.Di, a.s0);
        trace_row(host, 1, 80);
        fprintf(stderr, "\n[ns-trace] producer:");
        trace_row(hp, 41, 110);
        fprintf(stderr, "\n");
        return;
    }
    const unsigned long long cyc = host[WS_TRACE_SLOTS - 2] - host[WS_TRACE_SLOTS - 4], t10ns = host[WS_TRACE_SLOTS - 1] - host[WS_TRACE_SLOTS - 3];
    fprintf(stderr, "[ws-clock] Cin=%d Cout=%d in=%d: %llu cycles in %llu x10ns -> %.3f GHz, %d tiles per block\n", cin, a.Cout, a.Di, cyc, t10ns,
            (double)cyc / (10.0 * (double)t10ns), (tiles_per_sample * a.N + s.grid - 1) / s.grid);
    fprintf(stderr, "[ws-trace] consumer Cin=%d Cout=%d in=%d R=%d:", cin, a.Cout, a.Di, R);
    trace_row(host, 40, 120);
    fprintf(stderr, "\n[ws-trace] producer Cin=%d Cout=%d in=%d R=%d:", cin, a.Cout, a.Di, R);
    trace_row(hp, 40, 90);
    fprintf(stderr, "\n");
}
#endif

// ---- the launchers' prologue ------------------------------------------------------------------------------------------------------------
int conv_sched_prepare(boa_ctx* ctx, ConvArgs& a, int tiles_per_sample, const char* what, ConvSched* out) {
    BOA_REQUIRE((double)a.Di * a.Hi * a.Wi <= 16777216.0 && std::max(a.C0, a.C1) * 2 < 16777216,
                "%s: more than 2^24 input voxels per sample (24-bit offset multiply)", what);
    BOA_REQUIRE((double)a.Di * a.Hi * a.Wi * std::max(a.C0, a.C1) * 2.0 < 4294967296.0,
                "%s: one sample of the input exceeds 4 GiB (32-bit voxel offsets)", what);
    // the tools set BOA_WS_DBG before the process starts
    static const int dbg = getenv("BOA_WS_DBG") ? atoi(getenv("BOA_WS_DBG")) : 0;
    // virtual workgroups of a sample (batch-invariant statistics, see conv_ws_dev.h) and the physical grid
    const int vw = conv_ws_vw(tiles_per_sample, ctx->cu_count);
    const int grid = conv_sched_grid(vw, a.N, ctx->cu_count);
    // statistics slots: one per (virtual workgroup, consumer wave) = conv_nblk: the stride the caller allocated and k_norm_finalize
    // reads; waves that never touch an (n, cout chunk) leave zeros.  a.partials must be all zero on entry: the callers zero it once
    // (allocation / test seam) and k_norm_finalize clears what it has read, so no per-launch memset is needed
    a.nslots = conv_ws_nslots(tiles_per_sample, ctx->cu_count);
    a.vw = vw;
    a.vstep_n = grid / vw;
    a.vstep_j = grid % vw;
    const ConvRunTable* rt = run_table(ctx, a, tiles_per_sample, vw);
    BOA_REQUIRE(rt != nullptr, "%s: could not allocate the run table", what);
    a.runs = rt->dev;
    a.trace = nullptr;
    out->grid = grid;
    out->dbg = dbg;
    out->desc_row = conv_sched_desc_row(a.N, vw, grid, tiles_per_sample);
    out->desc = desc_table(ctx, a, rt, tiles_per_sample, grid, out->desc_row, what);
    if (!out->desc) return BOA_EINVAL;   // (desc_table has set the error)
#ifdef WS_WITH_TRACE
    trace_arm(ctx, a, grid);
#else
    static const bool trace_note = getenv("BOA_WS_TRACE") != nullptr && (fprintf(stderr, "[boa_hip] BOA_WS_TRACE needs a library built with -DWS_WITH_TRACE (tools/build_alt.sh trace -DWS_WITH_TRACE)\n"), true);
    (void)trace_note;
#endif
    return BOA_OK;
}
