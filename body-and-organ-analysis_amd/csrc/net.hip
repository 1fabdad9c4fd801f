// PlainConvUNet on device + the sliding-window tile loop
// (NN/inference/predict_from_raw_data.py:543,560-631; architecture per NN/utilities/plans_handling/plans_handler.py:59-92).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "net.h"

namespace {

// input channels per staged MFMA chunk of a conv and of a transposed conv: 16 fp16 channels, 8 split-precision channels; the
// fp32_ref kernels take any count (0)
int in_granule(NetMode m) { return m == NetMode::F16 ? 16 : m == NetMode::Split ? 8 : 0; }

// The pieces of a weight set in blob order, each in the device form its kernel reads.
enum class Piece {
    FirstW,    // first conv of the fp16 / split-precision modes: fp32 [Cin][taps][Cout]
    ConvW16,   // packed fp16 (pack_conv_weights)
    ConvWX3,   // split precision: hi / lo fp16 parts of w * 2^e (pack_conv_weights_x3)
    ConvW32,   // fp32_ref: fp32 [taps][Cin][Cout]
    Bias, Gamma, Beta,
    UpW16,     // transposed conv: packed fp16 (pack_convt_weights)
    UpWX3,     // split precision (pack_convt_weights_x3)
    UpW32,     // fp32_ref: fp32 [taps][Cin][Cout]
    UpBias,
    HeadW, HeadB,
};

Piece conv_weight_piece(NetMode m, bool first) {
    if (m == NetMode::F32Ref) return Piece::ConvW32;
    if (first) return Piece::FirstW;
    return m == NetMode::Split ? Piece::ConvWX3 : Piece::ConvW16;
}

Piece convt_weight_piece(NetMode m) { return m == NetMode::F32Ref ? Piece::UpW32 : m == NetMode::Split ? Piece::UpWX3 : Piece::UpW16; }

}  // namespace

static int net_alloc(boa_net* net, size_t bytes, void** out) {
    BOA_TRY(boa_malloc_raw(net->ctx, bytes, out));   // (long-lived: not through the caching allocator; freed with hipFree)
    net->allocs.push_back(*out);
    return BOA_OK;
}

// an activation buffer: a slice of the context's shared arena (bound by net_bind_arena)
static int net_alloc_act(boa_net* net, size_t bytes, void** out) {
    *out = nullptr;
    net->act_slots.push_back({out, net->act_need});
    net->act_need += (bytes + 255) & ~(size_t)255;
    return BOA_OK;
}

// make the arena large enough for this network (re-allocating it if another, smaller network sized it) and point the layers at it
int net_bind_arena(boa_net* net) {
    boa_ctx* c = net->ctx;
    if (net->act_slots.empty()) return BOA_OK;
    if (c->act_bytes < net->act_need) {
        BOA_HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->act_arena) hipFree(c->act_arena);
        c->act_arena = nullptr;
        c->act_bytes = 0;
        BOA_TRY(boa_malloc_raw(c, net->act_need, &c->act_arena));
        c->act_bytes = net->act_need;
        c->act_gen++;
    }
    if (net->act_gen_seen != c->act_gen) {
        for (auto& sl : net->act_slots) *sl.where = (unsigned char*)c->act_arena + sl.offset;
        net->act_gen_seen = c->act_gen;
    }
    return BOA_OK;
}

static bool desc_ok(const boa_net_desc* d) {
    if (!d || d->n_stages < 2 || d->n_stages > BOA_MAX_STAGES || d->in_channels < 1 || d->num_classes < 1) return false;
    for (int s = 0; s < d->n_stages; ++s) {
        if (d->features[s] <= 0 || d->n_conv_enc[s] < 1) return false;
        for (int a = 0; a < 3; ++a)
            if ((d->kernel[s][a] != 1 && d->kernel[s][a] != 3) || d->stride[s][a] < 1 || d->stride[s][a] > 2) return false;
    }
    for (int s = 0; s < d->n_stages - 1; ++s)
        if (d->n_conv_dec[s] < 1) return false;
    return true;
}

extern "C" size_t boa_net_weight_count(const boa_net_desc* d) {
    if (!desc_ok(d)) return 0;
    size_t n = 0;
    int cin = d->in_channels;
    for (int s = 0; s < d->n_stages; ++s) {
        int taps = d->kernel[s][0] * d->kernel[s][1] * d->kernel[s][2];
        for (int i = 0; i < d->n_conv_enc[s]; ++i) {
            n += (size_t)d->features[s] * cin * taps + 3 * (size_t)d->features[s];
            cin = d->features[s];
        }
    }
    for (int k = 0; k < d->n_stages - 1; ++k) {
        int sb = d->n_stages - 1 - k;  // stage below
        int below = d->features[sb], skip = d->features[sb - 1];
        int st = d->stride[sb][0] * d->stride[sb][1] * d->stride[sb][2];
        n += (size_t)below * skip * st + skip;
        int taps = d->kernel[sb - 1][0] * d->kernel[sb - 1][1] * d->kernel[sb - 1][2];
        int ci = 2 * skip;
        for (int i = 0; i < d->n_conv_dec[k]; ++i) {
            n += (size_t)skip * ci * taps + 3 * (size_t)skip;
            ci = skip;
        }
    }
    n += (size_t)d->num_classes * d->features[0] + d->num_classes;
    return n;
}

static int setup_conv(boa_net* net, ConvLayer& L, int N, const int din[3], int cin0, int cin1, int cout, const int k[3],
                      const int s[3], bool first) {
    L.first = first;
    L.Cin0 = cin0;
    L.Cin1 = cin1;
    L.g.N = N;
    L.g.Di = din[0]; L.g.Hi = din[1]; L.g.Wi = din[2];
    L.g.Cout = cout;
    L.g.Cin = cin0 + cin1;
    int dout[3];
    for (int a = 0; a < 3; ++a) {
        L.g.k[a] = k[a];
        L.g.s[a] = s[a];
        int p = (k[a] - 1) / 2;
        dout[a] = (din[a] + 2 * p - k[a]) / s[a] + 1;
    }
    L.g.Do = dout[0]; L.g.Ho = dout[1]; L.g.Wo = dout[2];
    const int taps = k[0] * k[1] * k[2];
    L.w_elems = (size_t)cout * (cin0 + cin1) * taps;
    const int gran = in_granule(net->mode);
    if (gran == 0) {   // fp32_ref: statistics from the stored output (launch_stats_f32), no partial sums
        BOA_REQUIRE(cout % 32 == 0, "conv %d+%d -> %d: Cout must be a multiple of 32", cin0, cin1, cout);
    } else if (first) {
        BOA_REQUIRE(s[0] == 1 && s[1] == 1 && s[2] == 1, "first conv must have stride 1");
        // (what launch_conv_first takes; refused here already, so that the split-precision caller can fall back to fp32_ref)
        BOA_REQUIRE(cout % 32 == 0 && cin0 >= 1 && cin0 <= 4, "first conv %d -> %d unsupported", cin0, cout);
        L.nblk = conv_first_nblk(dout, net->ctx->cu_count);
    } else {
        BOA_REQUIRE((cin0 % gran) == 0 && (cin1 % gran) == 0 && (cout % 32) == 0,
                    "conv %d+%d -> %d: channel counts must be multiples of %d (in) / 32 (out)", cin0, cin1, cout, gran);
        // the tile shape fixes the fp32 summation order inside the conv and the grouping of the InstanceNorm partial sums:
        // it is chosen for a nominal batch (TILE_REF_BATCH), never for the actual max_batch, so that a tile's result does not
        // depend on the batch size the network was created with
        ConvGeom gref = L.g;
        gref.N = TILE_REF_BATCH;
        BOA_REQUIRE(choose_conv_tile(gref, net->ctx->cu_count, &L.t, gran == 8), "no tile configuration fits conv %dx%dx%d k=%dx%dx%d",
                    din[0], din[1], din[2], k[0], k[1], k[2]);
        L.nblk = conv_nblk(L.t, net->ctx->cu_count, cout);
    }
    const ActLayout lay = act_layout(net->mode, cout);
    BOA_TRY(net_alloc_act(net, N * lay.bytes((size_t)dout[0] * dout[1] * dout[2]), &L.act));
    if (gran) {
        BOA_TRY(net_alloc(net, (size_t)N * cout * 2 * L.nblk * sizeof(float), (void**)&L.partials));
        BOA_HIP_TRY(hipMemsetAsync(L.partials, 0, (size_t)N * cout * 2 * L.nblk * sizeof(float), net->ctx->stream));
    }
    BOA_TRY(net_alloc(net, (size_t)N * cout * 2 * sizeof(float), (void**)&L.ss));
    if (lay.esz == 2)   // fp16 consumers read the (scale, shift) table packed to fp16 as well
        BOA_TRY(net_alloc(net, (size_t)N * cout * sizeof(unsigned), (void**)&L.ss16));
    return BOA_OK;
}

// Device layout of one weight set: every tensor of the blob, in blob order, at a 256-byte aligned offset of one arena.
// `visit(piece, layer pointers..., byte size)` is called in blob order; used both to size / fill the arena and
// to point the layers at it.
template <typename F>
static void for_each_weight_piece(boa_net* net, F&& f) {
    auto conv = [&](ConvLayer& L) {
        const int cin = L.Cin0 + L.Cin1, cout = L.g.Cout;
        const Piece w = conv_weight_piece(net->mode, L.first);
        f(w, &L, nullptr, w == Piece::ConvWX3   ? conv_wpk_halves_x3(cin, cout, L.g.k) * sizeof(__half)
                          : w == Piece::ConvW16 ? conv_wpk_halves(cin, cout, L.g.k) * sizeof(__half)
                                                : L.w_elems * sizeof(float));
        f(Piece::Bias, &L, nullptr, cout * sizeof(float));
        f(Piece::Gamma, &L, nullptr, cout * sizeof(float));
        f(Piece::Beta, &L, nullptr, cout * sizeof(float));
    };
    for (auto& st : net->enc)
        for (auto& L : st) conv(L);
    for (size_t k = 0; k < net->up.size(); ++k) {
        UpLayer& U = net->up[k];
        const Piece w = convt_weight_piece(net->mode);
        f(w, nullptr, &U, w == Piece::UpWX3   ? convt_wpk_halves_x3(U.Cin, U.Cout, U.s) * sizeof(__half)
                          : w == Piece::UpW16 ? convt_wpk_halves(U.Cin, U.Cout, U.s) * sizeof(__half)
                                              : (size_t)U.Cin * U.Cout * U.s[0] * U.s[1] * U.s[2] * sizeof(float));
        f(Piece::UpBias, nullptr, &U, U.Cout * sizeof(float));
        for (auto& L : net->dec[k]) conv(L);
    }
    f(Piece::HeadW, nullptr, nullptr, (size_t)net->d.num_classes * net->d.features[0] * sizeof(float));
    f(Piece::HeadB, nullptr, nullptr, net->d.num_classes * sizeof(float));
}

static void point_layers_at(boa_net* net, unsigned char* arena, const std::vector<float>& scales) {
    size_t off = 0, si = 0;
    for_each_weight_piece(net, [&](Piece piece, ConvLayer* L, UpLayer* U, size_t bytes) {
        void* p = arena + off;
        switch (piece) {
            case Piece::FirstW: L->wfirst = (float*)p; break;
            case Piece::ConvW16: L->wpk = (__half*)p; break;
            case Piece::ConvWX3: L->wpk = (__half*)p; L->wscale = scales[si++]; break;
            case Piece::ConvW32: L->w32 = (float*)p; break;
            case Piece::Bias: L->bias = (float*)p; break;
            case Piece::Gamma: L->gamma = (float*)p; break;
            case Piece::Beta: L->beta = (float*)p; break;
            case Piece::UpW16: U->wpk = (__half*)p; break;
            case Piece::UpWX3: U->wpk = (__half*)p; U->wscale = scales[si++]; U->fold = scales[si++]; break;
            case Piece::UpW32: U->w32 = (float*)p; break;
            case Piece::UpBias: U->bias = (float*)p; break;
            case Piece::HeadW: net->head_w = (float*)p; break;
            case Piece::HeadB: net->head_b = (float*)p; break;
        }
        off += align256(bytes);
    });
}

extern "C" int boa_net_load_weights(boa_net* net, const float* w, size_t n_floats) {
    BOA_REQUIRE(net && w, "boa_net_load_weights: NULL argument");
    size_t expect = boa_net_weight_count(&net->d);
    BOA_REQUIRE(n_floats == expect, "weight blob has %zu floats, geometry needs %zu", n_floats, expect);
    boa_ctx* c = net->ctx;
    // cached set of the same host blob (fold switching in predict_logits_from_preprocessed_data, :483-489)?
    unsigned long long hsh = 1469598103934665603ull;
    {
        const size_t step = n_floats > 4096 ? n_floats / 4096 : 1;
        for (size_t i = 0; i < n_floats; i += step) {
            unsigned u;
            memcpy(&u, w + i, 4);
            hsh = (hsh ^ u) * 1099511628211ull;
        }
    }
    for (auto& ws : net->wsets)
        if (ws.key == w && ws.n == n_floats && ws.sample_hash == hsh) {
            point_layers_at(net, ws.arena, ws.scales);  // (host-side pointers of later launches only: queued work keeps its own)
            return BOA_OK;
        }
    BOA_HIP_TRY(hipStreamSynchronize(c->stream));
    size_t total = 0;
    for_each_weight_piece(net, [&](Piece, ConvLayer*, UpLayer*, size_t bytes) { total += align256(bytes); });
    std::vector<unsigned char> stage(total, 0);
    std::vector<float> scales;
    const float* p = w;
    size_t off = 0;
    // Split-precision mode: activations are split unscaled (x3_split4), so the lo part of a value below 2^-3 is an fp16 subnormal with
    // an absolute floor of 2^-25.  Normalised activations are O(1), but a transposed conv's output is the one raw source of the stack:
    // its magnitude is whatever its weights make it.  A power of two g, chosen here from the weights so that the output lands near 1,
    // is folded into the transposed conv (stored output = g * output: winv and bias times g) and 1 / g into the up-channel weights of
    // the decoder conv that consumes it -- exact in binary, no instruction on the hot path.  (g = 1 for the usual Kaiming weights.)
    float up_fold = 1.f;
    const ConvLayer* fold_target = nullptr;
    for_each_weight_piece(net, [&](Piece piece, ConvLayer* L, UpLayer* U, size_t bytes) {
        unsigned char* dst = stage.data() + off;
        switch (piece) {
            case Piece::FirstW: {  // [cout][cin][taps] -> [cin][taps][cout] fp32
                const int cin = L->Cin0 + L->Cin1, cout = L->g.Cout, taps = L->g.k[0] * L->g.k[1] * L->g.k[2];
                float* wf = (float*)dst;
                for (int co = 0; co < cout; ++co)
                    for (int ci = 0; ci < cin; ++ci)
                        for (int t = 0; t < taps; ++t) wf[((size_t)ci * taps + t) * cout + co] = p[((size_t)co * cin + ci) * taps + t];
                p += L->w_elems;
                break;
            }
            case Piece::ConvW16:
                pack_conv_weights(p, L->Cin0 + L->Cin1, L->g.Cout, L->g.k, (__half*)dst);
                p += L->w_elems;
                break;
            case Piece::UpW16:
                pack_convt_weights(p, U->Cin, U->Cout, U->s, (__half*)dst);
                p += (size_t)U->Cin * U->Cout * U->s[0] * U->s[1] * U->s[2];
                break;
            case Piece::ConvWX3: {
                const float* wl = p;
                std::vector<float> folded;
                if (L == fold_target && up_fold != 1.f) {   // [Cout][Cin0 + Cin1][taps]: the first Cin0 inputs are the transposed conv's
                    const int cin = L->Cin0 + L->Cin1, taps = L->g.k[0] * L->g.k[1] * L->g.k[2];
                    folded.assign(p, p + L->w_elems);
                    for (int co = 0; co < L->g.Cout; ++co)
                        for (size_t i = 0; i < (size_t)L->Cin0 * taps; ++i) folded[(size_t)co * cin * taps + i] /= up_fold;
                    wl = folded.data();
                }
                const float sc = x3_weight_scale(wl, L->w_elems);
                scales.push_back(sc);
                pack_conv_weights_x3(wl, L->Cin0 + L->Cin1, L->g.Cout, L->g.k, sc, (__half*)dst);
                p += L->w_elems;
                break;
            }
            case Piece::UpWX3: {
                const size_t ne = (size_t)U->Cin * U->Cout * U->s[0] * U->s[1] * U->s[2];
                const float sc = x3_weight_scale(p, ne);
                up_fold = x3_output_fold(p, ne, U->Cin, p + ne, U->Cout);   // (the bias follows the weights in the blob)
                fold_target = &net->dec[U - net->up.data()][0];
                scales.push_back(sc / up_fold);   // winv = 1 / wscale = fold / sc
                scales.push_back(up_fold);
                pack_convt_weights_x3(p, U->Cin, U->Cout, U->s, sc, (__half*)dst);
                p += ne;
                break;
            }
            case Piece::UpBias:   // (times the output fold of the split-precision mode)
                memcpy(dst, p, bytes);
                if (up_fold != 1.f)
                    for (int i = 0; i < U->Cout; ++i) ((float*)dst)[i] *= up_fold;
                p += bytes / sizeof(float);
                break;
            case Piece::ConvW32: {  // [cout][cin][taps] -> [tap][cin][cout]
                const int cin = L->Cin0 + L->Cin1, cout = L->g.Cout, taps = L->g.k[0] * L->g.k[1] * L->g.k[2];
                float* wf = (float*)dst;
                for (int co = 0; co < cout; ++co)
                    for (int ci = 0; ci < cin; ++ci)
                        for (int t = 0; t < taps; ++t) wf[((size_t)t * cin + ci) * cout + co] = p[((size_t)co * cin + ci) * taps + t];
                p += L->w_elems;
                break;
            }
            case Piece::UpW32: {  // [cin][cout][taps] -> [tap][cin][cout]
                const int taps = U->s[0] * U->s[1] * U->s[2];
                float* wf = (float*)dst;
                for (int ci = 0; ci < U->Cin; ++ci)
                    for (int co = 0; co < U->Cout; ++co)
                        for (int t = 0; t < taps; ++t) wf[((size_t)t * U->Cin + ci) * U->Cout + co] = p[((size_t)ci * U->Cout + co) * taps + t];
                p += (size_t)U->Cin * U->Cout * taps;
                break;
            }
            case Piece::Bias:
            case Piece::Gamma:
            case Piece::Beta:
            case Piece::HeadW:
            case Piece::HeadB:  // fp32 vectors / head matrix, copied as they are
                memcpy(dst, p, bytes);
                p += bytes / sizeof(float);
                break;
        }
        off += align256(bytes);
    });
    BOA_REQUIRE((size_t)(p - w) == expect, "internal: weight cursor mismatch");
    if (net->wsets.size() >= 8) {  // bounded cache: drop the oldest set
        hipFree(net->wsets.front().arena);
        net->wsets.erase(net->wsets.begin());
    }
    unsigned char* arena = nullptr;
    BOA_TRY(boa_malloc_raw(c, total, (void**)&arena));
    hipError_t e = hipMemcpy(arena, stage.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(arena);
        BOA_HIP_TRY(e);
    }
    net->wsets.push_back({w, n_floats, hsh, arena, scales});
    point_layers_at(net, arena, scales);
    return BOA_OK;
}

extern "C" void boa_net_destroy(boa_net* net) {
    if (!net) return;
    hipStreamSynchronize(net->ctx->stream);
    for (void* a : net->allocs) hipFree(a);
    for (auto& ws : net->wsets) hipFree(ws.arena);
    delete net;
}

extern "C" int boa_net_create(boa_ctx* ctx, const boa_net_desc* desc, const float* host_weights, size_t n_floats,
                              int max_batch, int precision, boa_net** out) {
    BOA_REQUIRE(ctx && desc && out, "boa_net_create: NULL argument");
    BOA_REQUIRE(desc_ok(desc), "boa_net_create: invalid network geometry");
    BOA_REQUIRE(precision >= 0 && precision <= 2,
                "boa_net_create: precision %d not supported (0 = f16 MFMA / fp32 accumulate, 1 = fp32 reference mode, 2 = split-precision fp32)",
                precision);
    BOA_REQUIRE(max_batch >= 1 && max_batch <= 64, "boa_net_create: max_batch %d out of range", max_batch);
    BOA_HIP_TRY(hipSetDevice(ctx->device));
    boa_net* net = new boa_net();
    net->ctx = ctx;
    net->d = *desc;
    if (net->d.norm_eps <= 0.f) net->d.norm_eps = 1e-5f;
    if (net->d.lrelu_slope == 0.f) net->d.lrelu_slope = 0.01f;
    net->maxN = max_batch;
    net->mode = (NetMode)precision;
    const boa_net_desc& d = net->d;
    int rc = BOA_OK;
    auto fail = [&](int r) {
        boa_net_destroy(net);
        return r;
    };
    // encoder
    int din[3] = {d.patch[0], d.patch[1], d.patch[2]};
    int cin = d.in_channels;
    net->enc.resize(d.n_stages);
    for (int s = 0; s < d.n_stages; ++s) {
        net->enc[s].resize(d.n_conv_enc[s]);
        for (int i = 0; i < d.n_conv_enc[s]; ++i) {
            int one[3] = {1, 1, 1};
            const int* st = (i == 0) ? d.stride[s] : one;
            bool first = (s == 0 && i == 0);
            rc = setup_conv(net, net->enc[s][i], max_batch, din, cin, 0, d.features[s], d.kernel[s], st, first);
            if (rc) return fail(rc);
            const ConvGeom& g = net->enc[s][i].g;
            din[0] = g.Do; din[1] = g.Ho; din[2] = g.Wo;
            cin = d.features[s];
        }
        net->dims[s][0] = din[0]; net->dims[s][1] = din[1]; net->dims[s][2] = din[2];
    }
    // decoder
    net->up.resize(d.n_stages - 1);
    net->dec.resize(d.n_stages - 1);
    for (int k = 0; k < d.n_stages - 1; ++k) {
        int sb = d.n_stages - 1 - k;
        UpLayer& U = net->up[k];
        U.Cin = d.features[sb];
        U.Cout = d.features[sb - 1];
        for (int a = 0; a < 3; ++a) {
            U.s[a] = d.stride[sb][a];
            U.din[a] = net->dims[sb][a];
        }
        int dup[3] = {U.din[0] * U.s[0], U.din[1] * U.s[1], U.din[2] * U.s[2]};
        for (int a = 0; a < 3; ++a)
            if (dup[a] != net->dims[sb - 1][a]) {
                boa_set_error("decoder %d: upsampled dim %d (%d) != skip dim (%d); patch not divisible by strides", k, a,
                              dup[a], net->dims[sb - 1][a]);
                return fail(BOA_EINVAL);
            }
        const int gran = in_granule(net->mode);
        if ((gran && U.Cin % gran) || U.Cout % 32) {
            boa_set_error("transposed conv %d -> %d: unsupported channel counts", U.Cin, U.Cout);
            return fail(BOA_EINVAL);
        }
        if ((rc = net_alloc_act(net, max_batch * act_layout(net->mode, U.Cout).bytes((size_t)dup[0] * dup[1] * dup[2]), &U.act)))
            return fail(rc);
        net->dec[k].resize(d.n_conv_dec[k]);
        int one[3] = {1, 1, 1};
        for (int i = 0; i < d.n_conv_dec[k]; ++i) {
            int c0 = U.Cout, c1 = (i == 0) ? U.Cout : 0;
            rc = setup_conv(net, net->dec[k][i], max_batch, dup, c0, c1, U.Cout, d.kernel[sb - 1], one, false);
            if (rc) return fail(rc);
        }
    }
    if ((rc = net_alloc(net, (size_t)max_batch * 3 * sizeof(int), (void**)&net->dev_origins))) return fail(rc);
    if (net->mode == NetMode::F32Ref) {   // input of the forward's first conv: tiles gathered before the walk (net_forward_stack)
        if ((rc = net_alloc_act(net, (size_t)max_batch * d.in_channels * d.patch[0] * d.patch[1] * d.patch[2] * sizeof(float),
                                (void**)&net->tiles32)))
            return fail(rc);
    } else {
        int PD[3];
        conv_first_padded_dims(d.patch, d.kernel[0], PD);
        if ((rc = net_alloc_act(net, (size_t)max_batch * d.in_channels * PD[0] * PD[1] * PD[2] * sizeof(float),
                                (void**)&net->first_padded)))
            return fail(rc);
    }
    if ((rc = net_bind_arena(net))) return fail(rc);
    if (host_weights) {
        rc = boa_net_load_weights(net, host_weights, n_floats);
        if (rc) return fail(rc);
    }
    *out = net;
    return BOA_OK;
}

// ------------------------------------------------------------------------------------------------------
// The forward: ONE walk over the U-Net -- encoder, then per decoder stage the transposed conv and the convs on its output and the
// skip -- in which conv_step / convt_step launch every layer the way the network's mode does.

// inputs of one forward of N tiles
struct Fwd {
    const float* volume;
    const int* V;
    const int* vol_off;
    int N, flip_mask;
};

// BOA_LAYER_PROF: device time of every layer of the forward on stderr, one "[layer]" line each (tools/ab_layers.sh parses them);
// BOA_LAYER_PROF_REPEAT=n [BOA_LAYER_PROF_MATCH=Di,Cin,Cout]: a conv's launch n more times, timed as one block (sustained clocks;
// tools/power_sample.sh samples the socket power meanwhile)
struct LayerProf {
    boa_ctx* c;
    int N;
    const char* tag;   // after "[layer] ": "x3 " for split precision, "f32 " for fp32_ref
    bool variant;      // fp16 lines name the tile variant
    static bool on() {
        static const bool v = getenv("BOA_LAYER_PROF") != nullptr;
        return v;
    }
    void begin() const {
        if (on()) hipEventRecord(c->t0[7], c->stream);
    }
    float elapsed_ms() const {
        hipEventRecord(c->t1[7], c->stream);
        hipEventSynchronize(c->t1[7]);
        float ms = 0.f;
        hipEventElapsedTime(&ms, c->t0[7], c->t1[7]);
        return ms;
    }
    void end(const char* what, const int* din, int cin, int cout, const int* k, const int* s, double flops, const ConvTile* t) const {
        if (!on()) return;
        const float ms = elapsed_ms();
        fprintf(stderr, "[layer] %s%-6s N=%d in=%dx%dx%d cin=%d cout=%d k=%d%d%d s=%d%d%d ", tag, what, N, din[0], din[1], din[2], cin, cout,
                k[0], k[1], k[2], s[0], s[1], s[2]);
        if (t && variant) fprintf(stderr, "var=%d ", t->variant);
        if (t)
            fprintf(stderr, "R=%d w=%d,%d,%d b=%d,%d,%d tiles=%d lds=%zu ", t->R, t->w[0], t->w[1], t->w[2], t->b[0], t->b[1], t->b[2],
                    t->tiles[0] * t->tiles[1] * t->tiles[2], t->lds_bytes);
        fprintf(stderr, "%.1f us %.1f TFLOP/s\n", ms * 1e3, flops / (ms * 1e-3) / 1e12);
    }
    // after the timed launch of a conv: `launch` n more times as one timed block, then once more for end()
    template <typename F>
    int repeat(const ConvGeom& g, int cin, F&& launch) const {
        static const int n = getenv("BOA_LAYER_PROF_REPEAT") ? atoi(getenv("BOA_LAYER_PROF_REPEAT")) : 0;
        static int m_di = -1, m_ci = -1, m_co = -1;
        static const bool has_match = getenv("BOA_LAYER_PROF_MATCH") && sscanf(getenv("BOA_LAYER_PROF_MATCH"), "%d,%d,%d", &m_di, &m_ci, &m_co) == 3;
        if (!on() || n <= 0 || (has_match && (g.Di != m_di || cin != m_ci || g.Cout != m_co))) return BOA_OK;
        begin();
        for (int rep = 0; rep < n; ++rep) BOA_TRY(launch());
        const float ms = elapsed_ms();
        fprintf(stderr, "[repeat] in=%d cin=%d cout=%d: %d launches, %.1f us each, %.3f s\n", g.Di, cin, g.Cout, n, ms * 1e3 / n, ms * 1e-3);
        begin();
        return launch();
    }
};

// One conv of the walk (a, b: its two sources), then the (scale, shift) table of its InstanceNorm.  fp16: k_conv_first / the MFMA
// convs, statistics from the conv epilogues; split precision: the same with fp32 octet planes (k_conv_first<F32OUT>, k_conv_ws<X3>);
// fp32_ref: net_f32.hip's conv and statistics kernels.
static int conv_step(boa_net* net, const Fwd& f, const LayerProf& prof, ConvLayer& L, const ActSrc& a, const ActSrc& b) {
    boa_ctx* c = net->ctx;
    const boa_net_desc& d = net->d;
    ConvGeom g = L.g;
    g.N = f.N;
    int nblk = 0;
    auto launch = [&]() -> int {
        switch (net->mode) {
            case NetMode::F16:
                if (L.first)
                    return launch_conv_first(c, f.volume, f.V, f.vol_off, net->dev_origins, f.N, d.in_channels, d.patch, g.k, g.Cout, L.wfirst,
                                             L.bias, net->first_padded, (__half*)L.act, L.partials, &nblk, f.flip_mask);
                return launch_conv_mfma(c, a, b, g, L.t, L.wpk, L.bias, d.lrelu_slope, (__half*)L.act, L.partials);
            case NetMode::Split:
                if (L.first)
                    return launch_conv_first(c, f.volume, f.V, f.vol_off, net->dev_origins, f.N, d.in_channels, d.patch, g.k, g.Cout, L.wfirst,
                                             L.bias, net->first_padded, nullptr, L.partials, &nblk, f.flip_mask, (float*)L.act);
                return launch_conv_x3(c, (const float*)a.data, a.ss, a.C, (const float*)b.data, b.ss, b.C, g, L.t, L.wpk, L.wscale, L.bias,
                                      d.lrelu_slope, (float*)L.act, L.partials);
            case NetMode::F32Ref: {
                const int din[3] = {g.Di, g.Hi, g.Wi}, dout[3] = {g.Do, g.Ho, g.Wo};
                return launch_conv_f32(c, (const float*)a.data, a.ss, a.C, (const float*)b.data, b.ss, b.C, f.N, din, dout, g.k, g.s, g.Cout,
                                       L.w32, L.bias, d.lrelu_slope, (float*)L.act);
            }
        }
        return BOA_EINVAL;
    };
    const int cin = L.Cin0 + L.Cin1, din[3] = {g.Di, g.Hi, g.Wi};
    prof.begin();
    BOA_TRY(launch());
    if (!L.first) BOA_TRY(prof.repeat(g, cin, launch));
    prof.end(L.first ? "first" : "conv", din, cin, g.Cout, g.k, g.s, 2.0 * f.N * (double)g.Do * g.Ho * g.Wo * g.k[0] * g.k[1] * g.k[2] * cin * g.Cout,
             L.t.R ? &L.t : nullptr);   // (the first conv and fp32_ref have no MFMA tile)
    const double vox = (double)g.Do * g.Ho * g.Wo;
    if (net->mode == NetMode::F32Ref)
        return launch_stats_f32(c, (const float*)L.act, f.N, (size_t)vox, g.Cout, L.gamma, L.beta, d.norm_eps, L.ss);
    return launch_norm_finalize(c, L.partials, L.nblk, f.N, g.Cout, vox, L.gamma, L.beta, d.norm_eps, L.ss, L.ss16, 1);
}

// One transposed conv of the walk (src: the normalised output of the stage below).
static int convt_step(boa_net* net, const Fwd& f, const LayerProf& prof, UpLayer& U, const ActSrc& src) {
    boa_ctx* c = net->ctx;
    const float slope = net->d.lrelu_slope;
    prof.begin();
    switch (net->mode) {
        case NetMode::F16:
            BOA_TRY(launch_convt_mfma(c, src, f.N, U.din, U.s, U.Cout, U.wpk, U.bias, slope, (__half*)U.act));
            break;
        case NetMode::Split:
            BOA_TRY(launch_convt_x3(c, (const float*)src.data, src.ss, U.Cin, f.N, U.din, U.s, U.Cout, U.wpk, U.wscale, U.bias, slope,
                                    (float*)U.act));
            break;
        case NetMode::F32Ref:
            BOA_TRY(launch_convt_f32(c, (const float*)src.data, src.ss, U.Cin, f.N, U.din, U.s, U.Cout, U.w32, U.bias, slope, (float*)U.act));
            break;
    }
    prof.end("convT", U.din, U.Cin, U.Cout, U.s, U.s, 2.0 * f.N * (double)U.din[0] * U.din[1] * U.din[2] * U.s[0] * U.s[1] * U.s[2] * U.Cin * U.Cout,
             nullptr);
    return BOA_OK;
}

// what conv_step / convt_step launch for a layer, as boa_net_debug_layer reports it: {BOA_LK_* kernel, R (MT of k_convt_x3), row reuse
// of k_conv_ws (log2 of a split-precision transposed conv's output fold)}
void conv_kernel_info(const boa_net* net, const ConvLayer& L, int info[3]) {
    if (net->mode == NetMode::F32Ref) {
        info[0] = BOA_LK_CONV_F32;
    } else if (L.first) {
        info[0] = first_mfma_ok(net->d.in_channels, net->d.patch, L.g.k, L.g.Cout) ? BOA_LK_FIRST_MFMA : BOA_LK_FIRST_VALU;
    } else {
        const ConvTile& t = L.t;
        info[0] = t.variant == 2 ? BOA_LK_CONV_NS : t.variant == 1 ? BOA_LK_CONV_WS : BOA_LK_CONV_MFMA;
        info[1] = t.R;
        info[2] = t.variant == 1 && conv_ws_row_reuse(t.R, L.g.k[1], L.g.s[1], t.w[1], t.b[1], t.b[2]) ? 1 : 0;
    }
}

void convt_kernel_info(const boa_net* net, const UpLayer& U, int info[3]) {
    switch (net->mode) {
        case NetMode::F16: {
            const int form = convt_mfma_form(U.Cin, U.s, true);   // (the source of a transposed conv is always a normalised conv output)
            info[0] = form == 2 ? BOA_LK_CONVT_DEEP : form == 1 ? BOA_LK_CONVT_RW : BOA_LK_CONVT_MFMA;
            break;
        }
        case NetMode::Split:
            info[0] = BOA_LK_CONVT_X3;
            info[1] = convt_x3_mt((size_t)U.din[0] * U.din[1] * U.din[2]);
            info[2] = (int)std::lround(std::log2((double)U.fold));
            break;
        case NetMode::F32Ref:
            info[0] = BOA_LK_CONVT_F32;
            break;
    }
}

// run the conv stack for N tiles; leaves the last decoder activation (+ its ss) in net->dec.back().back()
int net_forward_stack(boa_net* net, const float* volume, const int V[3], const int vol_off[3], const int* host_origins, int N, int flip_mask) {
    boa_ctx* c = net->ctx;
    const boa_net_desc& d = net->d;
    BOA_REQUIRE(N >= 1 && N <= net->maxN, "forward: batch %d exceeds max_batch %d", N, net->maxN);
    BOA_HIP_TRY(hipMemcpyAsync(net->dev_origins, host_origins, (size_t)N * 3 * sizeof(int), hipMemcpyHostToDevice,
                               c->stream));
    // (the fp16 mode sets no profiling break after the upload, the others do: bench.py's per-class times depend on that)
    if (net->mode != NetMode::F16) c->prof_break = true;
    // fp32_ref's first conv reads the tiles gathered here, the other modes' first conv reads the volume itself
    if (net->mode == NetMode::F32Ref)
        BOA_TRY(launch_gather_tiles_f32(c, volume, V, vol_off, net->dev_origins, N, d.in_channels, d.patch, net->tiles32, flip_mask));
    const Fwd f{volume, V, vol_off, N, flip_mask};
    const LayerProf prof{c, N, net->mode == NetMode::Split ? "x3 " : net->mode == NetMode::F32Ref ? "f32 " : "", net->mode == NetMode::F16};
    auto out_of = [](const ConvLayer& L) {
        ActSrc s;
        s.data = (const __half*)L.act;
        s.ss = L.ss;
        s.ss16 = L.ss16;
        s.C = L.g.Cout;
        return s;
    };
    ActSrc cur, none;
    cur.data = (const __half*)net->tiles32;
    cur.C = d.in_channels;
    for (int s = 0; s < d.n_stages; ++s)
        for (ConvLayer& L : net->enc[s]) {
            BOA_TRY(conv_step(net, f, prof, L, cur, none));
            cur = out_of(L);
        }
    for (int k = 0; k < d.n_stages - 1; ++k) {
        UpLayer& U = net->up[k];
        BOA_TRY(convt_step(net, f, prof, U, cur));
        ActSrc up;
        up.data = (const __half*)U.act;
        up.C = U.Cout;
        const ActSrc skip = out_of(net->enc[d.n_stages - 2 - k].back());
        for (size_t i = 0; i < net->dec[k].size(); ++i) {
            ConvLayer& L = net->dec[k][i];
            BOA_TRY(i == 0 ? conv_step(net, f, prof, L, up, skip) : conv_step(net, f, prof, L, cur, none));
            cur = out_of(L);
        }
    }
    return BOA_OK;
}

// The scatter-form head (one launch per tile) of a network, as its BOA_LK_* code: fp16 -> the MFMA head; split precision -> k_head_x3
// (the gather head's arithmetic: label path == logits API, bit for bit) for F0 = 32 and up to 32 classes, else the fp32 head;
// fp32_ref -> the fp32 head.
int head_kernel(const boa_net* net) {
    const boa_net_desc& d = net->d;
    if (net->mode == NetMode::F16) return BOA_LK_HEAD_MFMA;
    return net->mode == NetMode::Split && d.features[0] == 32 && d.num_classes <= 32 ? BOA_LK_HEAD_X3 : BOA_LK_HEAD_F32;
}

// runs it on one tile: `act` at the first record it reads, `plane_stride` as ActLayout::plane_stride
int scatter_head(const boa_net* net, const void* act, const float* ss, const int P[3], size_t plane_stride, const float* w, const float* b,
                 float* logits_out, const uint16_t* gauss, uint16_t* acc, uint16_t* nacc, const int PV[3], const int start[3]) {
    const boa_net_desc& d = net->d;
    switch (head_kernel(net)) {
        case BOA_LK_HEAD_MFMA:
            return launch_head(net->ctx, (const __half*)act, ss, d.features[0], P, d.num_classes, w, b, d.lrelu_slope, logits_out, gauss, acc,
                               nacc, PV, start, plane_stride);
        case BOA_LK_HEAD_X3:
            return launch_head_x3(net->ctx, (const float*)act, ss, d.features[0], P, d.num_classes, w, b, d.lrelu_slope, logits_out, gauss,
                                  acc, nacc, PV, start, plane_stride);
        default:
            return launch_head_f32(net->ctx, (const float*)act, ss, d.features[0], P, d.num_classes, w, b, d.lrelu_slope, logits_out, gauss,
                                   acc, nacc, PV, start, plane_stride);
    }
}

// head of tile i of the current batch without its first plane_skip axis-0 planes
int net_head(boa_net* net, int i, const int P[3], int plane_skip, float* logits_out, const uint16_t* gauss, uint16_t* acc, uint16_t* nacc,
             const int PV[3], const int start[3]) {
    const boa_net_desc& d = net->d;
    const ConvLayer& last = net->dec.back().back();
    const ActLayout lay = act_layout(net->mode, d.features[0]);
    const size_t plane = (size_t)d.patch[1] * d.patch[2], pv = d.patch[0] * plane;
    return scatter_head(net, (const unsigned char*)last.act + lay.tile(i, pv) + lay.skip(plane_skip, plane), last.ss + (size_t)i * d.features[0] * 2,
                        P, lay.plane_stride(pv), net->head_w, net->head_b, logits_out, gauss, acc, nacc, PV, start);
}

// `_internal_maybe_mirror_and_predict` (predict_from_raw_data.py:541-557) for the nb tiles of one batch: the fp32 logits of
// the plain forward plus, for every non-empty combination of the allowed mirror axes (itertools.combinations order: single
// axes, pairs, the triple), the logits of the flipped tile flipped back, divided by the number of variants.  Result in
// net->mirror_sum [nb][C][P].
static int net_mirrored_logits(boa_net* net, const float* volume, const int V[3], const int vol_off[3], const int* host_origins, int nb) {
    const boa_net_desc& d = net->d;
    const size_t pv = (size_t)d.patch[0] * d.patch[1] * d.patch[2], per = (size_t)d.num_classes * pv;
    if (!net->mirror_tmp) {
        BOA_TRY(net_alloc(net, (size_t)net->maxN * per * sizeof(float), (void**)&net->mirror_tmp));
        BOA_TRY(net_alloc(net, (size_t)net->maxN * per * sizeof(float), (void**)&net->mirror_sum));
    }
    std::vector<int> combos = {0};
    int axes[3], na = 0;
    for (int a = 0; a < 3; ++a)
        if (net->mirror_mask & (1 << a)) axes[na++] = a;
    for (int size = 1; size <= na; ++size)
        for (int m = 1; m < (1 << na); ++m) {   // subsets of `size` axes in lexicographic order of their axis tuples
            if (__builtin_popcount(m) != size) continue;
            combos.push_back(m);
        }
    // lexicographic order of tuples: for size 1: (a0), (a1), (a2); size 2: (a0,a1), (a0,a2), (a1,a2) = ascending bit masks
    // 3, 5, 6 -- the ascending-mask enumeration above already yields that order for up to three axes
    for (size_t k = 0; k < combos.size(); ++k) {
        int flip = 0;
        for (int j = 0; j < na; ++j)
            if (combos[k] & (1 << j)) flip |= 1 << axes[j];
        BOA_TRY(net_forward_stack(net, volume, V, vol_off, host_origins, nb, flip));
        const bool last = k + 1 == combos.size();
        for (int i = 0; i < nb; ++i) {
            BOA_TRY(net_head(net, i, d.patch, 0, net->mirror_tmp + (size_t)i * per, nullptr, nullptr, nullptr, nullptr, nullptr));
            BOA_TRY(launch_flip_accumulate(net->ctx, net->mirror_tmp + (size_t)i * per, net->mirror_sum + (size_t)i * per, d.num_classes,
                                           d.patch, flip, k > 0, last ? (float)combos.size() : 1.0f));
        }
    }
    return BOA_OK;
}

extern "C" int boa_net_set_mirroring(boa_net* net, int axes_mask) {
    BOA_REQUIRE(net && axes_mask >= 0 && axes_mask < 8, "boa_net_set_mirroring: axes mask %d", axes_mask);
    net->mirror_mask = axes_mask;
    return BOA_OK;
}

extern "C" int boa_net_forward(boa_net* net, const float* dev_volume, const int V[3], const int* host_origins,
                               int n_tiles, float* dev_logits_out) {
    BOA_REQUIRE(net && dev_volume && V && host_origins && dev_logits_out, "boa_net_forward: NULL argument");
    BOA_TRY(net_bind_arena(net));
    const boa_net_desc& d = net->d;
    const size_t pv = (size_t)d.patch[0] * d.patch[1] * d.patch[2];
    const int zero[3] = {0, 0, 0};
    for (int t0 = 0; t0 < n_tiles; t0 += net->maxN) {
        int nb = std::min(net->maxN, n_tiles - t0);
        if (net->mirror_mask) {
            BOA_TRY(net_mirrored_logits(net, dev_volume, V, zero, host_origins + (size_t)t0 * 3, nb));
            BOA_HIP_TRY(hipMemcpyAsync(dev_logits_out + (size_t)t0 * d.num_classes * pv, net->mirror_sum,
                                       (size_t)nb * d.num_classes * pv * sizeof(float), hipMemcpyDeviceToDevice, net->ctx->stream));
            net->ctx->prof_break = true;
            continue;
        }
        BOA_TRY(net_forward_stack(net, dev_volume, V, zero, host_origins + (size_t)t0 * 3, nb));
        for (int i = 0; i < nb; ++i)
            BOA_TRY(net_head(net, i, d.patch, 0, dev_logits_out + (size_t)(t0 + i) * d.num_classes * pv, nullptr, nullptr, nullptr,
                             nullptr, nullptr));
    }
    return BOA_OK;
}

// the sliding-window entry points' padded volume PV must hold a patch and the volume V at offset `off`, along every axis
int check_padded(const boa_net* net, const int V[3], const int PV[3], const int off[3], const char* who) {
    for (int a = 0; a < 3; ++a)
        BOA_REQUIRE(PV[a] >= net->d.patch[a] && off[a] >= 0 && off[a] + V[a] <= PV[a],
                    "%s: padded dim %d (%d) must cover patch (%d) and volume (%d at %d)", who, a, PV[a], net->d.patch[a], V[a], off[a]);
    return BOA_OK;
}

extern "C" int boa_net_predict_sliding_window(boa_net* net, const float* dev_volume, const int V[3], const int PV[3],
                                              const int* vol_off, const int* host_origins, int n_tiles,
                                              const uint16_t* dev_gauss, uint16_t* dev_acc, uint16_t* dev_n) {
    BOA_REQUIRE(net && dev_volume && V && PV && host_origins && dev_acc && dev_n,
                "boa_net_predict_sliding_window: NULL argument");
    BOA_TRY(net_bind_arena(net));
    const boa_net_desc& d = net->d;
    const int zero[3] = {0, 0, 0};
    const int* off = vol_off ? vol_off : zero;
    BOA_TRY(check_padded(net, V, PV, off, "sliding window"));
    const size_t pv = (size_t)d.patch[0] * d.patch[1] * d.patch[2];
    for (int t0 = 0; t0 < n_tiles; t0 += net->maxN) {
        int nb = std::min(net->maxN, n_tiles - t0);
        if (net->mirror_mask) {  // mirrored mean of the fp32 logits first, then the reference's accumulate step on it
            BOA_TRY(net_mirrored_logits(net, dev_volume, V, off, host_origins + (size_t)t0 * 3, nb));
            for (int i = 0; i < nb; ++i)
                BOA_TRY(boa_accumulate_tile(net->ctx, net->mirror_sum + (size_t)i * d.num_classes * pv, dev_gauss, dev_acc, dev_n,
                                            d.num_classes, d.patch, PV, host_origins + (size_t)(t0 + i) * 3));
            continue;
        }
        BOA_TRY(net_forward_stack(net, dev_volume, V, off, host_origins + (size_t)t0 * 3, nb));
        for (int i = 0; i < nb; ++i) {  // canonical order: one launch per tile, serialised on the stream
            const int* st = host_origins + (size_t)(t0 + i) * 3;
            BOA_TRY(net_head(net, i, d.patch, 0, nullptr, dev_gauss, dev_acc, dev_n, PV, st));
        }
    }
    return BOA_OK;
}
