// Unit-test seams of the network driver: single conv / transposed conv / head launches on caller data, and the stored activations,
// (scale, shift) tables and kernel choices of a network's layers.
#include <string.h>

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

// ---- host-only plan queries (no GPU touched) and the layer seams that launch ONE layer the way the network does -------------------------
// A plan is everything that selects code for a layer.  The queries call what setup_conv and the launchers call (choose_conv_tile with
// TILE_REF_BATCH, conv_tile_complete, conv_ws_row_reuse, conv_ws_resident, conv_ws_cy_fast, conv_ws_vw, conv_nblk, convt_mfma_form,
// convt_x3_mt); nothing is restated here.
static void plan_geom(ConvGeom* g, int Cin, const int dims[3], int Cout, const int k[3], const int s[3]) {
    g->N = TILE_REF_BATCH;   // as the network does: the tile shape must not depend on the batch size
    g->Di = dims[0]; g->Hi = dims[1]; g->Wi = dims[2]; g->Cout = Cout; g->Cin = Cin;
    int dout[3];
    for (int a = 0; a < 3; ++a) {
        g->k[a] = k[a];
        g->s[a] = s[a];
        dout[a] = (dims[a] + 2 * ((k[a] - 1) / 2) - k[a]) / s[a] + 1;
    }
    g->Do = dout[0]; g->Ho = dout[1]; g->Wo = dout[2];
}

static bool pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }

// the tile of a layer: the planner's, or the override {variant, R, w[3], b[3]} completed and checked as the planner's candidates are
static int plan_tile(const ConvGeom& g, int cu_count, bool x3, const int* ov, ConvTile* t) {
    if (!ov) {
        BOA_REQUIRE(choose_conv_tile(g, cu_count, t, x3), "conv plan: no tile configuration");
        return BOA_OK;
    }
    const int variant = ov[0], R = ov[1];
    BOA_REQUIRE(variant >= 0 && variant <= 2 && (R == 1 || R == 2 || R == 4), "conv plan: override variant %d, R %d", variant, R);
    BOA_REQUIRE(!x3 || variant != 0, "conv plan: the split-precision mode has no variant 0");
    if (variant == 2) {
        BOA_REQUIRE(conv_ns_applicable(g), "conv plan: k_conv_ns does not take this layer");
        conv_ns_tile(g, t);
        bool same = t->R == R;
        for (int d = 0; d < 3; ++d) same = same && t->w[d] == ov[2 + d] && t->b[d] == ov[5 + d];
        BOA_REQUIRE(same, "conv plan: k_conv_ns has one tile shape");
        return BOA_OK;
    }
    t->variant = variant;
    t->R = R;
    for (int d = 0; d < 3; ++d) {
        t->w[d] = ov[2 + d];
        t->b[d] = ov[5 + d];
    }
    BOA_REQUIRE(pow2_in(t->w[0], 1, 8) && pow2_in(t->w[1], 1, 8) && pow2_in(t->w[2], 4, 32) && t->w[0] * t->w[1] * t->w[2] == 32,
                "conv plan: wave tile %dx%dx%d", t->w[0], t->w[1], t->w[2]);
    BOA_REQUIRE(pow2_in(t->b[0], 1, 16) && pow2_in(t->b[1], 1, 16) && pow2_in(t->b[2], 1, 16) && t->b[0] * t->b[1] * t->b[2] == 4 * R,
                "conv plan: block tile %dx%dx%d for R %d", t->b[0], t->b[1], t->b[2], R);
    BOA_REQUIRE(conv_tile_complete(g, x3, t), "conv plan: the override fails conv_ws_supported or the LDS limit");
    return BOA_OK;
}

static void plan_words(const ConvGeom& g, const ConvTile& t, int cu_count, bool x3, int* out) {
    for (int i = 0; i < BOA_PLAN_WORDS; ++i) out[i] = 0;
    out[0] = t.variant; out[1] = t.R;
    for (int d = 0; d < 3; ++d) {
        out[2 + d] = t.w[d]; out[5 + d] = t.b[d]; out[8 + d] = t.h[d]; out[12 + d] = t.tiles[d];
    }
    out[11] = t.xs > 0 ? t.xs : t.h[1] * t.h[2];
    out[15] = (int)t.lds_bytes;
    const int taps = g.k[0] * g.k[1] * g.k[2], ncc = x3 ? g.Cin / 8 : g.Cin / 16, spatial = t.tiles[0] * t.tiles[1] * t.tiles[2];
    if (t.variant == 1) {
        out[16] = conv_ws_row_reuse(t.R, g.k[1], g.s[1], t.w[1], t.b[1], t.b[2]) ? 1 : 0;
        out[17] = conv_ws_resident(t.h[0] * out[11], taps, ncc, g.Cout) ? 1 : 0;
        out[18] = conv_ws_cy_fast(x3 ? 2 * g.Cin : g.Cin, g.Cout, t.R) ? 1 : 0;
        out[22] = g.Cout / 32;
    } else if (t.variant == 2) {
        out[21] = conv_ns_wn(g.Cout);
        out[22] = conv_ns_ncy(g.Cout);
    }
    if (t.variant != 0) out[19] = conv_ws_vw(spatial * out[22], cu_count);
    out[20] = t.variant != 0 ? conv_ws_nslots(spatial * out[22], cu_count) : 0;
    out[23] = conv_nblk(t, cu_count, g.Cout);
    out[24] = g.Do; out[25] = g.Ho; out[26] = g.Wo;
    out[27] = t.variant == 2 ? BOA_LK_CONV_NS : t.variant == 1 ? BOA_LK_CONV_WS : BOA_LK_CONV_MFMA;
    out[28] = x3 ? 1 : 0;
}

static int plan_mode(int mode, bool* x3) {
    BOA_REQUIRE(mode == (int)NetMode::F16 || mode == (int)NetMode::Split, "plan: mode %d (0 = fp16, 2 = split precision)", mode);
    *x3 = mode == (int)NetMode::Split;
    return BOA_OK;
}

static int conv_plan(int Cin0, int Cin1, const int dims[3], int Cout, const int k[3], const int s[3], int cu_count, int mode,
                     const int* ov, ConvGeom* g, ConvTile* t, int* plan_out) {
    bool x3 = false;
    BOA_TRY(plan_mode(mode, &x3));
    const int gran = x3 ? 8 : 16;
    BOA_REQUIRE(Cin0 > 0 && Cin1 >= 0 && Cin0 % gran == 0 && Cin1 % gran == 0 && Cout > 0 && Cout % 32 == 0 && cu_count > 0,
                "conv plan: channels %d+%d -> %d (multiples of %d in, 32 out)", Cin0, Cin1, Cout, gran);
    for (int a = 0; a < 3; ++a)
        BOA_REQUIRE(dims[a] >= 1 && k[a] >= 1 && (k[a] & 1) && s[a] >= 1, "conv plan: dims / kernel / stride of axis %d", a);
    plan_geom(g, Cin0 + Cin1, dims, Cout, k, s);
    BOA_REQUIRE(g->Do >= 1 && g->Ho >= 1 && g->Wo >= 1, "conv plan: empty output");
    BOA_TRY(plan_tile(*g, cu_count, x3, ov, t));
    if (plan_out) plan_words(*g, *t, cu_count, x3, plan_out);
    return BOA_OK;
}

extern "C" int boa_conv_plan(int Cin0, int Cin1, const int dims[3], int Cout, const int kernel[3], const int stride[3], int cu_count,
                             int mode, const int* plan_override, int* plan_out) {
    BOA_REQUIRE(dims && kernel && stride && plan_out, "boa_conv_plan: NULL argument");
    ConvGeom g;
    ConvTile t;
    return conv_plan(Cin0, Cin1, dims, Cout, kernel, stride, cu_count, mode, plan_override, &g, &t, plan_out);
}

static int convt_plan(int Cin, const int dims[3], int Cout, const int s[3], int mode, int norm_src, int* out) {
    bool x3 = false;
    BOA_TRY(plan_mode(mode, &x3));
    BOA_REQUIRE(Cin > 0 && Cin % (x3 ? 8 : 16) == 0 && Cout > 0 && Cout % 32 == 0, "convT plan: channels %d -> %d", Cin, Cout);
    for (int a = 0; a < 3; ++a) BOA_REQUIRE(dims[a] >= 1 && s[a] >= 1, "convT plan: dims / stride of axis %d", a);
    for (int i = 0; i < BOA_PLAN_WORDS; ++i) out[i] = 0;
    if (x3) {
        out[0] = -1;
        out[1] = convt_x3_mt((size_t)dims[0] * dims[1] * dims[2]);
        out[2] = BOA_LK_CONVT_X3;
    } else {
        out[0] = convt_mfma_form(Cin, s, norm_src != 0);
        out[2] = out[0] == 2 ? BOA_LK_CONVT_DEEP : out[0] == 1 ? BOA_LK_CONVT_RW : BOA_LK_CONVT_MFMA;
    }
    out[3] = s[2];
    out[4] = Cin / 16;
    for (int a = 0; a < 3; ++a) out[5 + a] = dims[a] * s[a];
    return BOA_OK;
}

extern "C" int boa_convt_plan(int Cin, const int dims[3], int Cout, const int stride[3], int cu_count, int mode, int norm_src,
                              int* plan_out) {
    BOA_REQUIRE(dims && stride && plan_out && cu_count > 0, "boa_convt_plan: NULL argument");
    return convt_plan(Cin, dims, Cout, stride, mode, norm_src, plan_out);
}

// fp32 NCDHW -> the mode's activation layout (fp16 chunk planes / fp32 octet planes), in a fresh buffer
static int seam_source(boa_ctx* ctx, bool x3, const float* dev_in, int N, int C, size_t vox, void** out) {
    BOA_TRY(boa_malloc(ctx, (size_t)N * vox * C * (x3 ? 4 : 2), out));
    if (x3) return launch_nchw_to_octet_f32(ctx, dev_in, N, C, vox, (float*)*out);
    return launch_nchw_to_ndhwc_f16(ctx, dev_in, N, C, vox, (__half*)*out);
}

extern "C" int boa_conv_layer_test(boa_ctx* ctx, int mode, int N, const int dims[3], const float* dev_src0, int C0, const float* dev_ss0,
                                   const uint32_t* dev_ss16_0, const float* dev_src1, int C1, const float* dev_ss1,
                                   const uint32_t* dev_ss16_1, const float* host_w, const float* host_b, const float* host_gamma,
                                   const float* host_beta, int Cout, const int kernel[3], const int stride[3], const int* plan_override,
                                   void* dev_raw, float* dev_ss, uint32_t* dev_ss16, float* dev_partials, int* host_plan) {
    BOA_REQUIRE(ctx && dims && dev_src0 && host_w && host_b && host_gamma && host_beta && kernel && stride && dev_raw && dev_ss && dev_partials,
                "conv layer test: NULL argument");
    BOA_REQUIRE(N >= 1 && (C1 == 0) == (dev_src1 == nullptr), "conv layer test: batch %d, second source of %d channels", N, C1);
    ConvGeom g;
    ConvTile t;
    int plan[BOA_PLAN_WORDS];
    BOA_TRY(conv_plan(C0, C1, dims, Cout, kernel, stride, ctx->cu_count, mode, plan_override, &g, &t, plan));
    const bool x3 = mode == (int)NetMode::Split;
    // the tables come as the producer's k_norm_finalize leaves them: fp16 consumers read the fp32 and the packed fp16 table
    BOA_REQUIRE(x3 ? (!dev_ss16_0 && !dev_ss16_1 && !dev_ss16) : ((dev_ss0 == nullptr) == (dev_ss16_0 == nullptr) &&
                                                                  (dev_ss1 == nullptr) == (dev_ss16_1 == nullptr) && dev_ss16),
                "conv layer test: fp16 sources take ss and ss16 together, split-precision ones ss only");
    BOA_REQUIRE(C1 > 0 || (!dev_ss1 && !dev_ss16_1), "conv layer test: table without a second source");
    if (host_plan) memcpy(host_plan, plan, sizeof(plan));
    g.N = N;
    const int Cin = C0 + C1, nblk = plan[23];
    const size_t vin = (size_t)dims[0] * dims[1] * dims[2], vout = (size_t)g.Do * g.Ho * g.Wo;
    void *in0 = nullptr, *in1 = nullptr;
    __half* wpk = nullptr;
    float *bias = nullptr, *gamma = nullptr, *beta = nullptr;
    float wscale = 1.f;
    std::vector<__half> tmp(x3 ? conv_wpk_halves_x3(Cin, Cout, kernel) : conv_wpk_halves(Cin, Cout, kernel));
    if (x3) {
        wscale = x3_weight_scale(host_w, (size_t)Cout * Cin * kernel[0] * kernel[1] * kernel[2]);
        pack_conv_weights_x3(host_w, Cin, Cout, kernel, wscale, tmp.data());
    } else {
        pack_conv_weights(host_w, Cin, Cout, kernel, tmp.data());
    }
    int rc = BOA_OK;
    T_(boa_malloc(ctx, tmp.size() * 2, (void**)&wpk));
    T_(boa_malloc(ctx, Cout * 4, (void**)&bias));
    T_(boa_malloc(ctx, Cout * 4, (void**)&gamma));
    T_(boa_malloc(ctx, Cout * 4, (void**)&beta));
    T_(boa_h2d(ctx, wpk, tmp.data(), tmp.size() * 2));
    T_(boa_h2d(ctx, bias, host_b, Cout * 4));
    T_(boa_h2d(ctx, gamma, host_gamma, Cout * 4));
    T_(boa_h2d(ctx, beta, host_beta, Cout * 4));
    T_(seam_source(ctx, x3, dev_src0, N, C0, vin, &in0));
    if (C1) T_(seam_source(ctx, x3, dev_src1, N, C1, vin, &in1));
    if (x3) {
        T_(launch_conv_x3(ctx, (const float*)in0, dev_ss0, C0, (const float*)in1, dev_ss1, C1, g, t, wpk, wscale, bias, 0.01f, (float*)dev_raw,
                          dev_partials));
    } else {
        ActSrc a, b;
        a.data = (const __half*)in0; a.ss = dev_ss0; a.ss16 = dev_ss16_0; a.C = C0;
        b.data = (const __half*)in1; b.ss = dev_ss1; b.ss16 = dev_ss16_1; b.C = C1;
        T_(launch_conv_mfma(ctx, a, b, g, t, wpk, bias, 0.01f, (__half*)dev_raw, dev_partials));
    }
    T_(launch_norm_finalize(ctx, dev_partials, nblk, N, Cout, (double)vout, gamma, beta, 1e-5f, dev_ss, dev_ss16, 1));
    if (rc == BOA_OK) rc = boa_sync(ctx);
    boa_free(ctx, in0); boa_free(ctx, in1); boa_free(ctx, wpk); boa_free(ctx, bias); boa_free(ctx, gamma); boa_free(ctx, beta);
    return rc;
}

extern "C" int boa_convt_layer_test(boa_ctx* ctx, int mode, int N, const int dims[3], const float* dev_src, int Cin, const float* dev_ss,
                                    const uint32_t* dev_ss16, const float* host_w, const float* host_b, int Cout, const int stride[3],
                                    void* dev_raw, int* host_plan) {
    BOA_REQUIRE(ctx && dims && dev_src && host_w && host_b && stride && dev_raw && N >= 1, "convT layer test: NULL argument");
    int plan[BOA_PLAN_WORDS];
    BOA_TRY(convt_plan(Cin, dims, Cout, stride, mode, dev_ss16 != nullptr, plan));
    const bool x3 = mode == (int)NetMode::Split;
    // (fp16: the network passes both tables and the kernels read the packed one; ss alone reaches k_convt_mfma's fp32-table transform)
    BOA_REQUIRE(x3 ? !dev_ss16 : (dev_ss != nullptr || dev_ss16 == nullptr),
                "convT layer test: the packed fp16 table comes with the fp32 one, a split-precision source takes ss only");
    if (host_plan) memcpy(host_plan, plan, sizeof(plan));
    const size_t vin = (size_t)dims[0] * dims[1] * dims[2];
    void* in = nullptr;
    __half* wpk = nullptr;
    float* bias = nullptr;
    float wscale = 1.f;
    std::vector<__half> tmp(x3 ? convt_wpk_halves_x3(Cin, Cout, stride) : convt_wpk_halves(Cin, Cout, stride));
    if (x3) {
        wscale = x3_weight_scale(host_w, (size_t)Cin * Cout * stride[0] * stride[1] * stride[2]);
        pack_convt_weights_x3(host_w, Cin, Cout, stride, wscale, tmp.data());
    } else {
        pack_convt_weights(host_w, Cin, Cout, stride, tmp.data());
    }
    int rc = BOA_OK;
    T_(boa_malloc(ctx, tmp.size() * 2, (void**)&wpk));
    T_(boa_malloc(ctx, Cout * 4, (void**)&bias));
    T_(boa_h2d(ctx, wpk, tmp.data(), tmp.size() * 2));
    T_(boa_h2d(ctx, bias, host_b, Cout * 4));
    T_(seam_source(ctx, x3, dev_src, N, Cin, vin, &in));
    if (x3) {
        T_(launch_convt_x3(ctx, (const float*)in, dev_ss, Cin, N, dims, stride, Cout, wpk, wscale, bias, 0.01f, (float*)dev_raw));
    } else {
        ActSrc a;
        a.data = (const __half*)in; a.ss = dev_ss; a.ss16 = dev_ss16; a.C = Cin;
        T_(launch_convt_mfma(ctx, a, N, dims, stride, Cout, wpk, bias, 0.01f, (__half*)dev_raw));
    }
    if (rc == BOA_OK) rc = boa_sync(ctx);
    boa_free(ctx, in); boa_free(ctx, wpk); boa_free(ctx, bias);
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

extern "C" int boa_head_tile_f32(boa_ctx* ctx, int kind, const float* dev_act_f32, size_t stride, const float* dev_ss, int F0,
                                 const int P[3], int C, const float* dev_w, const float* dev_b, float slope, float* dev_logits_out,
                                 const uint16_t* dev_gauss, uint16_t* dev_acc, uint16_t* dev_n, const int PV[3], const int start[3]) {
    BOA_REQUIRE(ctx && dev_act_f32 && dev_ss && P && dev_w && dev_b, "boa_head_tile_f32: NULL argument");
    BOA_REQUIRE(dev_logits_out || (dev_acc && dev_n && PV && start), "boa_head_tile_f32: neither logits_out nor accumulators given");
    BOA_REQUIRE(kind == BOA_LK_HEAD_X3 || kind == BOA_LK_HEAD_F32, "boa_head_tile_f32: kind %d (12 = k_head_x3, 13 = k_head_f32)", kind);
    if (kind == BOA_LK_HEAD_X3)
        return launch_head_x3(ctx, dev_act_f32, dev_ss, F0, P, C, dev_w, dev_b, slope, dev_logits_out, dev_gauss, dev_acc, dev_n, PV, start,
                              stride);
    return launch_head_f32(ctx, dev_act_f32, dev_ss, F0, P, C, dev_w, dev_b, slope, dev_logits_out, dev_gauss, dev_acc, dev_n, PV, start,
                           stride);
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
