// Unit-test seams of the network driver: single conv / transposed conv / head launches on caller data, and the stored activations,
// (scale, shift) tables and kernel choices of a network's layers.
#include "net.h"

// one step of a seam's straight-line body; later steps are skipped after a failure, the buffers are freed either way
#define T_(x) do { if (rc == BOA_OK) rc = (x); } while (0)

extern "C" int boa_conv_block_test(boa_ctx* ctx, const float* dev_in, int N, int Cin, const int dims[3],
                                   const float* host_w, const float* host_b, const float* host_gamma,
                                   const float* host_beta, int Cout, const int kernel[3], const int stride[3],
                                   int with_norm_act, int impl, float* dev_out) {
    BOA_REQUIRE(ctx && dev_in && dims && host_w && host_b && kernel && stride && dev_out, "conv test: NULL argument");
    BOA_REQUIRE(impl == 0, "conv test: impl %d not available", impl);
    ConvGeom g;
    g.N = N; g.Di = dims[0]; g.Hi = dims[1]; g.Wi = dims[2]; g.Cout = Cout; g.Cin = Cin;
    int dout[3];
    for (int a = 0; a < 3; ++a) {
        g.k[a] = kernel[a];
        g.s[a] = stride[a];
        dout[a] = (dims[a] + 2 * ((kernel[a] - 1) / 2) - kernel[a]) / stride[a] + 1;
    }
    g.Do = dout[0]; g.Ho = dout[1]; g.Wo = dout[2];
    ConvTile t;
    ConvGeom gref = g;
    gref.N = TILE_REF_BATCH;  // as the network does: the tile shape must not depend on the batch size
    BOA_REQUIRE(choose_conv_tile(gref, ctx->cu_count, &t), "conv test: no tile configuration");
    size_t vin = (size_t)dims[0] * dims[1] * dims[2], vout = (size_t)dout[0] * dout[1] * dout[2];
    __half *in16 = nullptr, *out16 = nullptr, *wpk = nullptr;
    float *bias = nullptr, *gamma = nullptr, *beta = nullptr, *partials = nullptr, *ss = nullptr;
    int nblk = conv_nblk(t, ctx->cu_count, Cout);
    std::vector<__half> tmp(conv_wpk_halves(Cin, Cout, kernel));
    pack_conv_weights(host_w, Cin, Cout, kernel, tmp.data());
    std::vector<float> ones(Cout, 1.f), zeros(Cout, 0.f);
    int rc = BOA_OK;
    T_(boa_malloc(ctx, (size_t)N * vin * Cin * 2, (void**)&in16));
    T_(boa_malloc(ctx, (size_t)N * vout * Cout * 2, (void**)&out16));
    T_(boa_malloc(ctx, tmp.size() * 2, (void**)&wpk));
    T_(boa_malloc(ctx, Cout * 4, (void**)&bias));
    T_(boa_malloc(ctx, Cout * 4, (void**)&gamma));
    T_(boa_malloc(ctx, Cout * 4, (void**)&beta));
    T_(boa_malloc(ctx, (size_t)N * Cout * 2 * nblk * 4, (void**)&partials));
    T_(boa_memset(ctx, partials, 0, (size_t)N * Cout * 2 * nblk * 4));
    T_(boa_malloc(ctx, (size_t)N * Cout * 2 * 4, (void**)&ss));
    T_(boa_h2d(ctx, wpk, tmp.data(), tmp.size() * 2));
    T_(boa_h2d(ctx, bias, host_b, Cout * 4));
    T_(boa_h2d(ctx, gamma, host_gamma ? host_gamma : ones.data(), Cout * 4));
    T_(boa_h2d(ctx, beta, host_beta ? host_beta : zeros.data(), Cout * 4));
    T_(launch_nchw_to_ndhwc_f16(ctx, dev_in, N, Cin, vin, in16));
    ActSrc a, none;
    a.data = in16; a.ss = nullptr; a.C = Cin;
    T_(launch_conv_mfma(ctx, a, none, g, t, wpk, bias, 0.01f, out16, partials));
    T_(launch_norm_finalize(ctx, partials, nblk, N, Cout, (double)vout, gamma, beta, 1e-5f, ss, nullptr, 1));
    T_(launch_ndhwc_to_nchw_f32(ctx, out16, with_norm_act ? ss : nullptr, 0.01f, N, Cout, vout, dev_out));
    if (rc == BOA_OK) rc = boa_sync(ctx);
    boa_free(ctx, in16); boa_free(ctx, out16); boa_free(ctx, wpk); boa_free(ctx, bias); boa_free(ctx, gamma);
    boa_free(ctx, beta); boa_free(ctx, partials); boa_free(ctx, ss);
    return rc;
}

extern "C" int boa_convtranspose_test(boa_ctx* ctx, const float* dev_in, int N, int Cin, const int dims[3],
                                      const float* host_w, const float* host_b, int Cout, const int stride[3],
                                      float* dev_out) {
    BOA_REQUIRE(ctx && dev_in && dims && host_w && host_b && stride && dev_out, "convT test: NULL argument");
    size_t vin = (size_t)dims[0] * dims[1] * dims[2];
    size_t vout = vin * stride[0] * stride[1] * stride[2];
    __half *in16 = nullptr, *out16 = nullptr, *wpk = nullptr;
    float* bias = nullptr;
    std::vector<__half> tmp(convt_wpk_halves(Cin, Cout, stride));
    pack_convt_weights(host_w, Cin, Cout, stride, tmp.data());
    int rc = BOA_OK;
    T_(boa_malloc(ctx, (size_t)N * vin * Cin * 2, (void**)&in16));
    T_(boa_malloc(ctx, (size_t)N * vout * Cout * 2, (void**)&out16));
    T_(boa_malloc(ctx, tmp.size() * 2, (void**)&wpk));
    T_(boa_malloc(ctx, Cout * 4, (void**)&bias));
    T_(boa_h2d(ctx, wpk, tmp.data(), tmp.size() * 2));
    T_(boa_h2d(ctx, bias, host_b, Cout * 4));
    T_(launch_nchw_to_ndhwc_f16(ctx, dev_in, N, Cin, vin, in16));
    ActSrc a;
    a.data = in16; a.ss = nullptr; a.C = Cin;
    T_(launch_convt_mfma(ctx, a, N, dims, stride, Cout, wpk, bias, 0.01f, out16));
    T_(launch_ndhwc_to_nchw_f32(ctx, out16, nullptr, 0.01f, N, Cout, vout, dev_out));
    if (rc == BOA_OK) rc = boa_sync(ctx);
    boa_free(ctx, in16); boa_free(ctx, out16); boa_free(ctx, wpk); boa_free(ctx, bias);
    return rc;
}
#undef T_

extern "C" int boa_head_tile(boa_ctx* ctx, const uint16_t* dev_act, const float* dev_ss, int F0, const int P[3], int C,
                             const float* dev_w, const float* dev_b, float slope, float* dev_logits_out,
                             const uint16_t* dev_gauss, uint16_t* dev_acc, uint16_t* dev_n, const int PV[3],
                             const int start[3]) {
    BOA_REQUIRE(ctx && dev_act && dev_ss && P && dev_w && dev_b, "boa_head_tile: NULL argument");
    BOA_REQUIRE(dev_logits_out || (dev_acc && dev_n && PV && start), "boa_head_tile: neither logits_out nor accumulators given");
    return launch_head(ctx, (const __half*)dev_act, dev_ss, F0, P, C, dev_w, dev_b, slope, dev_logits_out, dev_gauss, dev_acc,
                       dev_n, PV, start);
}

// fp32 NCDHW of one stored tile for the debug seams, with a transposed conv's output fold taken out again (x / fold is exact): through
// the conversion's (scale, shift) path with scale 1 / fold, shift 0 and slope 1 (LeakyReLU with slope 1 is the identity)
static int debug_to_nchw(boa_net* net, const ActLayout& lay, const void* tile, const float* ss, float fold, size_t vox, float* out) {
    if (fold == 1.f) return lay.to_nchw(net->ctx, tile, ss, net->d.lrelu_slope, vox, out);
    std::vector<float> tab((size_t)lay.C * 2);
    for (int i = 0; i < lay.C; ++i) {
        tab[2 * i] = 1.f / fold;
        tab[2 * i + 1] = 0.f;
    }
    float* dss = nullptr;
    BOA_TRY(boa_malloc(net->ctx, tab.size() * sizeof(float), (void**)&dss));
    int rc = boa_h2d(net->ctx, dss, tab.data(), tab.size() * sizeof(float));
    if (rc == BOA_OK) rc = lay.to_nchw(net->ctx, tile, dss, 1.f, vox, out);
    if (rc == BOA_OK) rc = boa_sync(net->ctx);
    boa_free(net->ctx, dss);
    return rc;
}

// a stored layer output: kind 0 / 2 = conv `conv` of encoder / decoder stage `stage` (L), kind 1 = transposed conv `stage` (U)
struct LayerRef {
    const ConvLayer* L = nullptr;
    const UpLayer* U = nullptr;
    const void* act = nullptr;
    float fold = 1.f;   // a split-precision transposed conv stores fold * output
    int C = 0, dims[3] = {0, 0, 0};
    size_t vox() const { return (size_t)dims[0] * dims[1] * dims[2]; }
    const void* tile(NetMode m, int i) const { return (const unsigned char*)act + act_layout(m, C).tile(i, vox()); }
};

static int find_layer(boa_net* net, const char* who, int kind, int stage, int conv, LayerRef* r) {
    if (kind == 1) {
        BOA_REQUIRE(stage >= 0 && stage < (int)net->up.size(), "%s: no transposed conv %d", who, stage);
        const UpLayer& U = net->up[stage];
        r->U = &U;
        r->C = U.Cout;
        for (int a = 0; a < 3; ++a) r->dims[a] = U.din[a] * U.s[a];
        r->act = U.act;
        r->fold = U.fold;
        return BOA_OK;
    }
    auto& stages = kind == 0 ? net->enc : net->dec;
    BOA_REQUIRE((kind == 0 || kind == 2) && stage >= 0 && stage < (int)stages.size() && conv >= 0 && conv < (int)stages[stage].size(),
                "%s: no layer (kind %d, stage %d, conv %d)", who, kind, stage, conv);
    const ConvLayer& L = stages[stage][conv];
    r->L = &L;
    r->C = L.g.Cout;
    r->dims[0] = L.g.Do; r->dims[1] = L.g.Ho; r->dims[2] = L.g.Wo;
    r->act = L.act;
    return BOA_OK;
}

extern "C" int boa_net_debug_activation(boa_net* net, int kind, int stage, int conv, int tile, float* dev_out, int* channels_out,
                                        int dims_out[3]) {
    BOA_REQUIRE(net && channels_out && dims_out, "boa_net_debug_activation: NULL argument");
    BOA_REQUIRE(tile >= 0 && tile < net->maxN, "boa_net_debug_activation: tile %d outside the batch", tile);
    BOA_TRY(net_bind_arena(net));
    LayerRef r;
    BOA_TRY(find_layer(net, "boa_net_debug_activation", kind, stage, conv, &r));
    *channels_out = r.C;
    for (int a = 0; a < 3; ++a) dims_out[a] = r.dims[a];
    if (!dev_out) return BOA_OK;  // size query
    const float* ss = r.L ? r.L->ss + (size_t)tile * r.C * 2 : nullptr;
    return debug_to_nchw(net, act_layout(net->mode, r.C), r.tile(net->mode, tile), ss, r.fold, r.vox(), dev_out);
}

extern "C" int boa_net_debug_layer(boa_net* net, int kind, int stage, int conv, int tile, float* dev_raw, float* host_ss,
                                   uint16_t* host_ss16, int* channels_out, int dims_out[3], int* host_info) {
    BOA_REQUIRE(net && channels_out && dims_out, "boa_net_debug_layer: NULL argument");
    BOA_REQUIRE(tile >= 0 && tile < net->maxN, "boa_net_debug_layer: tile %d outside the batch", tile);
    BOA_TRY(net_bind_arena(net));
    const boa_net_desc& d = net->d;
    if (kind == 3) {   // the head: which kernel net_head launches (its output is the logits of boa_net_forward, nothing is stored)
        BOA_REQUIRE(!dev_raw && !host_ss && !host_ss16, "boa_net_debug_layer: the head stores no output (kind 3 reports the kernel only)");
        *channels_out = d.num_classes;
        for (int a = 0; a < 3; ++a) dims_out[a] = d.patch[a];
        if (host_info) {
            host_info[0] = head_kernel(net);
            host_info[1] = host_info[2] = 0;
        }
        return BOA_OK;
    }
    LayerRef r;
    BOA_TRY(find_layer(net, "boa_net_debug_layer", kind, stage, conv, &r));
    const ConvLayer* L = r.L;
    const int Cc = r.C;
    int info[3] = {0, 0, 0};
    if (L) conv_kernel_info(net, *L, info);
    else convt_kernel_info(net, *r.U, info);
    *channels_out = Cc;
    for (int a = 0; a < 3; ++a) dims_out[a] = r.dims[a];
    if (host_info)
        for (int i = 0; i < 3; ++i) host_info[i] = info[i];
    if (host_ss) {
        if (L) {
            BOA_TRY(boa_sync(net->ctx));
            BOA_HIP_TRY(hipMemcpy(host_ss, L->ss + (size_t)tile * Cc * 2, (size_t)Cc * 2 * sizeof(float), hipMemcpyDeviceToHost));
        } else {
            for (int i = 0; i < 2 * Cc; ++i) host_ss[i] = i & 1 ? 0.f : 1.f;   // (raw source: identity)
        }
    }
    if (host_ss16) {
        BOA_REQUIRE(L && L->ss16, "boa_net_debug_layer: fp16 (scale, shift) exist for the convs of the fp16 mode only");
        BOA_TRY(boa_sync(net->ctx));
        BOA_HIP_TRY(hipMemcpy(host_ss16, L->ss16 + (size_t)tile * Cc, (size_t)Cc * sizeof(unsigned), hipMemcpyDeviceToHost));
    }
    if (!dev_raw) return BOA_OK;
    return debug_to_nchw(net, act_layout(net->mode, Cc), r.tile(net->mode, tile), nullptr, r.fold, r.vox(), dev_raw);
}
