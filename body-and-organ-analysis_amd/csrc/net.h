// The network driver's shared types and the pieces of net.hip that the stash-based sliding windows (net_stash.hip) and the test
// seams (net_debug.hip) call.  Internal to the library.
#pragma once
#include <vector>

#include "conv.h"
#include "tile_grid.h"   // (align256)

// The network's arithmetic; the values are boa_net_create's `precision`.  F16: fp16 storage + f16 MFMA (production); F32Ref: the
// fp32 reference mode (net_f32.hip); Split: split precision (fp32 storage, hi / lo fp16 operands on the matrix cores: k_conv_ws<X3>,
// net_x3.hip).  Only the functions that answer the mode's questions look at it: in_granule, act_layout, conv_weight_piece /
// convt_weight_piece, head_kernel and the forward's launch steps (net_forward_stack, conv_step, convt_step and their kernel reports),
// besides boa_net_create's choice of the first conv's input buffer.
enum class NetMode : int { F16 = 0, F32Ref = 1, Split = 2 };

// Record format of a layer's activation buffer of C channels.  fp16 chunk planes [N][C/16][voxel][16] and split-precision octet
// planes [N][C/8][voxel][8] (fp32) both hold 32-byte records in planes that span all voxels of a tile; fp32_ref holds channels-last
// records [N][voxel][C] (fp32) of 4 C bytes in one plane.
struct ActLayout {
    int C;
    int esz;       // bytes per channel value
    bool planar;   // 32-byte records in C * esz / 32 planes, else channels-last
    size_t rec() const { return planar ? 32 : (size_t)C * esz; }
    size_t bytes(size_t vox) const { return vox * C * esz; }              // one tile of `vox` voxels
    size_t tile(size_t i, size_t vox) const { return i * bytes(vox); }    // byte offset of tile i
    // byte offset, inside every record plane, that skips a tile's first n axis-0 planes of `plane` voxels
    size_t skip(int n, size_t plane) const { return (size_t)n * plane * rec(); }
    // the plane stride (voxels) the scatter-form heads take; 0 = channels-last
    size_t plane_stride(size_t vox) const { return planar ? vox : 0; }
    // copies the first dp axis-0 planes of a tile (vox voxels, `plane` per axis-0 plane) to dst, in the same format with dp * plane
    // voxels per record plane
    hipError_t copy_head(unsigned char* dst, const void* tile, int dp, size_t plane, size_t vox, hipStream_t s) const {
        const size_t n = (size_t)dp * plane * rec();
        const int planes = planar ? C * esz / 32 : 1;
        hipError_t e = hipSuccess;
        for (int k = 0; k < planes && e == hipSuccess; ++k)
            e = hipMemcpyAsync(dst + k * n, (const unsigned char*)tile + k * vox * rec(), n, hipMemcpyDeviceToDevice, s);
        return e;
    }
    // fp32 NCDHW of one tile through the (scale, shift) table ss (nullptr: raw) and LeakyReLU
    int to_nchw(boa_ctx* c, const void* tile, const float* ss, float slope, size_t vox, float* out) const {
        if (!planar) return launch_ndhwc32_to_nchw_f32(c, (const float*)tile, ss, slope, C, vox, out);
        if (esz == 4) return launch_octet_to_nchw_f32(c, (const float*)tile, ss, slope, C, vox, out);
        return launch_ndhwc_to_nchw_f32(c, (const __half*)tile, ss, slope, 1, C, vox, out);
    }
};

inline ActLayout act_layout(NetMode m, int C) { return {C, m == NetMode::F16 ? 2 : 4, m != NetMode::F32Ref}; }

struct ConvLayer {
    ConvGeom g{};
    ConvTile t{};
    int Cin0 = 0, Cin1 = 0;  // channels of the two concatenated sources (Cin1 = 0: single source)
    bool first = false;      // stage-0 conv-0: fp32 VALU kernel reading the volume
    __half* wpk = nullptr;   // MFMA layers
    float* wfirst = nullptr; // first layer [Cin][taps][Cout]
    float* w32 = nullptr;    // fp32 mode: [taps][Cin][Cout]
    float wscale = 1.f;      // split-precision mode: power-of-two scale of the packed weights (per weight set)
    float *bias = nullptr, *gamma = nullptr, *beta = nullptr;
    void* act = nullptr;     // raw conv output in the mode's ActLayout
    float* partials = nullptr;
    float* ss = nullptr;
    unsigned* ss16 = nullptr;
    int nblk = 0;
    size_t w_elems = 0;  // fp32 elements of W in the blob
};

struct UpLayer {
    int Cin = 0, Cout = 0;
    int s[3] = {1, 1, 1};
    int din[3] = {0, 0, 0};
    __half* wpk = nullptr;
    float* w32 = nullptr;    // fp32 mode: [taps][Cin][Cout]
    float* bias = nullptr;
    void* act = nullptr;     // output in the mode's ActLayout
    float wscale = 1.f;      // split-precision mode
    float fold = 1.f;        // split-precision mode: power of two folded into the stored output (act = fold * convT output)
};

// The tile shapes of a network are chosen for a REFERENCE tile batch, not for the batch of a call or the net's max_batch: the shape
// decides how the InstanceNorm partial sums are grouped, and results must not depend on how many tiles share a launch.
// 16 = the product's default tile batch (with 8, the value of rounds 1-2, the 8^3 layers got half-size tiles -- 2 x 10 workgroups
// per sample -- which at the batches actually run (16, 25) only doubled the weight streaming: 116 -> 82, 200 -> 134, 111 -> 73 us
// per 25 tiles for the three 8^3 convs).
constexpr int TILE_REF_BATCH = 16;

struct boa_net {
    boa_ctx* ctx = nullptr;
    boa_net_desc d{};
    int maxN = 1;
    NetMode mode = NetMode::F16;
    int mirror_mask = 0;       // test-time mirroring axes (bit a = array axis a), predict_from_raw_data.py:541-557
    float* mirror_tmp = nullptr;  // [maxN][C][P] fp32 logits of one mirror variant
    float* mirror_sum = nullptr;  // [maxN][C][P] running sum / mean
    float* tiles32 = nullptr;  // fp32 mode: gathered input tiles [N][P][Cin]
    std::vector<std::vector<ConvLayer>> enc;  // [stage][conv]
    std::vector<UpLayer> up;                  // decoder order (deepest first)
    std::vector<std::vector<ConvLayer>> dec;  // [d][conv]
    float *head_w = nullptr, *head_b = nullptr;
    int* dev_origins = nullptr;
    float* first_padded = nullptr;  // zero-padded fp32 gather buffer of the first conv
    std::vector<void*> allocs;
    // Activation buffers (one per layer, ~1 GB per tile at 128^3: 25 GB at tile batch 25) live in ONE arena per context that all
    // of its networks share: the networks of a context run one after the other on its stream and every forward overwrites a
    // layer's buffer before reading it, so seven resident networks need the largest network's activations once, not seven times
    // (175 GB -> 25 GB at the bench's batch; what persists across forwards -- statistics partials, (scale, shift) tables, weight
    // arenas, the gather head's stash -- stays outside).  A layer records its offset; pointers are (re)bound whenever the arena
    // has been re-allocated for a larger network (boa_ctx::act_gen).
    struct ActSlot {
        void** where;
        size_t offset;
    };
    std::vector<ActSlot> act_slots;
    size_t act_need = 0;
    unsigned long long act_gen_seen = 0;
    int dims[BOA_MAX_STAGES][3];
    // packed weight sets (one device arena each), cached per host blob: switching folds is a pointer swap, not a re-pack
    struct WeightSet {
        const float* key;
        size_t n;
        unsigned long long sample_hash;  // FNV-1a over ~4096 evenly spaced floats: guards against a recycled host address
        unsigned char* arena;
        std::vector<float> scales;       // split-precision mode: weight scale of every conv / transposed conv (+ the output fold of a
                                         // transposed conv), blob order
    };
    std::vector<WeightSet> wsets;
};

// net.hip (documented at the definitions)
int net_bind_arena(boa_net* net);
int net_forward_stack(boa_net* net, const float* volume, const int V[3], const int vol_off[3], const int* host_origins, int N, int flip_mask = 0);
int head_kernel(const boa_net* net);
int scatter_head(const boa_net* net, const void* act, const float* ss, const int P[3], size_t plane_stride, const float* w, const float* b,
                 float* logits_out, const uint16_t* gauss, uint16_t* acc, uint16_t* nacc, const int PV[3], const int start[3]);
int net_head(boa_net* net, int i, const int P[3], int plane_skip, float* logits_out, const uint16_t* gauss, uint16_t* acc, uint16_t* nacc,
             const int PV[3], const int start[3]);
int check_padded(const boa_net* net, const int V[3], const int PV[3], const int off[3], const char* who);
void conv_kernel_info(const boa_net* net, const ConvLayer& L, int info[3]);
void convt_kernel_info(const boa_net* net, const UpLayer& U, int info[3]);
