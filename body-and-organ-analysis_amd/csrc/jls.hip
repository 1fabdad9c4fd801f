// JPEG-LS decode of a DICOM series on the device (transfer syntaxes 1.2.840.10008.1.2.4.80 / .81, ITU-T T.87).  The context
// model adapts over the whole scan, so a scan is one serial chain; the frames of a series are independent.  k_jls_wave gives every
// frame one wave: the chain runs on wave-uniform values (every lane holds the same bit stream state, context record and
// neighbours, read to the scalar side), and the lanes share what is not the chain: per row, before the chain, the part of every
// sample's context that the row above decides (jls_pre_word: 81 Q1 + 9 Q2, zero exactly where a run may start, with Rb), the run
// fills, and the row's coalesced store.  Row buffers, the pre words and the 367 context records live in LDS.  k_jls_serial is the
// plain loop, one lane per frame, rows and contexts in global memory: the reference the tests compare with, and the path of rows
// wider than BOA_JLS_WAVE_MAX_COLS.  The rules themselves are jls_codes.h, shared with the host program that runs them sanitized.
#include <vector>

#include "common.h"
#include "jls_codes.h"

static_assert(JLS_ST_TRUNCATED == BOA_JLS_TRUNCATED && JLS_ST_INVALID == BOA_JLS_INVALID && JLS_ST_OK == BOA_JLS_OK, "status codes");

namespace {

constexpr int WAVE = 64;

struct JlsFrame {
    unsigned long long off;      // of the scan in the data buffer, a multiple of 4
    unsigned len;
    int maxval, near_, t1, t2, t3, reset, pad;
};

__device__ inline JlsParams params_of(const JlsFrame& f) { return jls_derive(f.maxval, f.near_, f.t1, f.t2, f.t3, f.reset); }

// the row policy of the one-wave kernel: everything in LDS, values read by every lane alike and moved to the scalar side
struct JlsWaveRow {
    const uint32_t* pre;
    const uint16_t* prev;
    uint16_t* cur;
    int lane, cols;
    int next_x;                  // the pre word of the sample behind the last one looked at is already on its way
    uint32_t next_w;
    __device__ int above(int x) const { return jls_uni<true>((int)prev[x]); }
    __device__ uint32_t look(int x, int, int* Rb) {
        const uint32_t raw = x == next_x ? next_w : pre[x];
        next_x = x + 1;
        next_w = pre[x + 1 < cols ? x + 1 : x];
        const uint32_t w = (uint32_t)jls_uni<true>((int)raw);
        *Rb = (int)(w & 0xFFFFu);
        return w;
    }
    // (no lane branches on its own: every lane stores the sample; a lane behind a fill's end stores its last sample once more)
    __device__ void put(int x, int v) { cur[x] = (uint16_t)v; }
    __device__ void fill(int x0, int x1, int v) {
        for (int base = x0; base < x1; base += WAVE) cur[min(base + lane, x1 - 1)] = (uint16_t)v;
    }
};

// One wave per frame.  LDS: cols pre words, two rows of cols samples (dynamic), the context records (static).
__global__ __launch_bounds__(WAVE) void k_jls_wave(const uint8_t* __restrict__ data, const JlsFrame* __restrict__ frames, int rows,
                                                   int cols, uint16_t* __restrict__ out, int* __restrict__ status) {
    extern __shared__ uint32_t lds[];
    __shared__ JlsCtx ctx[JLS_CONTEXTS];
    const int lane = threadIdx.x, f = blockIdx.x;
    uint32_t* pre = lds;
    uint16_t* prev = (uint16_t*)(lds + cols);
    uint16_t* cur = prev + ((cols + 1) & ~1);
    const JlsFrame fr = frames[f];
    const JlsParams p = params_of(fr);
    // (loops of one trip count for all lanes, the index clamped: see jls_codes.h on branches)
    for (int i = 0; i < JLS_CONTEXTS; i += WAVE) ctx[min(i + lane, JLS_CONTEXTS - 1)] = jls_ctx_init(p);
    for (int base = 0; base < cols; base += WAVE) prev[min(base + lane, cols - 1)] = 0;
    __syncthreads();
    JlsBits b = jls_bits_open<true>((const uint32_t*)(data + fr.off), fr.len);
    uint16_t* o = out + (size_t)f * rows * cols;
    int runindex = 0, corner = 0, bad = 0;
    for (int r = 0; r < rows; ++r) {
        const int Ra0 = jls_uni<true>((int)prev[0]);
        for (int base = 0; base < cols; base += WAVE) {
            const int x = min(base + lane, cols - 1);
            const int Rb = prev[x], Rc = x ? (int)prev[x - 1] : corner, Rd = x + 1 < cols ? (int)prev[x + 1] : Rb;
            pre[x] = jls_pre_word(Rb, Rc, Rd, p);
        }
        __syncthreads();
        JlsWaveRow row{pre, prev, cur, lane, cols, -1, 0u};
        bad = jls_uni<true>(jls_row<true>(b, p, ctx, row, cols, Ra0, corner, &runindex));
        corner = Ra0;
        __syncthreads();
        if (bad) break;                                                // (uniform over the wave)
        for (int base = 0; base < cols; base += WAVE) {
            const int x = min(base + lane, cols - 1);
            o[(size_t)r * cols + x] = cur[x];
        }
        uint16_t* t = prev;
        prev = cur;
        cur = t;
    }
    if (lane == 0) status[f] = jls_status(b, bad);
}

// the plain loop, one lane per frame; ws: JLS_CONTEXTS records per frame
__global__ void k_jls_serial(const uint8_t* __restrict__ data, const JlsFrame* __restrict__ frames, int n_frames, int rows, int cols,
                             uint16_t* __restrict__ out, JlsCtx* __restrict__ ws, int* __restrict__ status) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames) return;
    const JlsFrame fr = frames[f];
    status[f] = jls_decode_plain((const uint32_t*)(data + fr.off), fr.len, params_of(fr), rows, cols, out + (size_t)f * rows * cols,
                                 ws + (size_t)f * JLS_CONTEXTS);
}

}  // namespace

extern "C" int boa_jls_decode(boa_ctx* c, const uint8_t* dev_data, size_t data_bytes, int n_frames, const int* frames, int rows,
                              int cols, uint16_t* dev_out, int* host_status, int serial) {
    BOA_REQUIRE(c && dev_data && frames && dev_out && host_status, "boa_jls_decode: NULL argument");
    BOA_REQUIRE(n_frames > 0, "boa_jls_decode: empty batch");
    BOA_REQUIRE(rows >= 1 && rows <= 65535 && cols >= 1 && cols <= 65535, "boa_jls_decode: frame size %d x %d", rows, cols);
    BOA_REQUIRE(((uintptr_t)dev_data & 3u) == 0, "boa_jls_decode: the data buffer is not 4-byte aligned");
    // every range the kernels follow is checked here, on the host, before anything reaches the device
    std::vector<JlsFrame> tab((size_t)n_frames);
    double in_bytes = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int* F = frames + (size_t)f * BOA_JLS_FRAME_WORDS;
        const unsigned long long off = ((unsigned long long)(unsigned)F[BOA_JLS_F_OFF_HI] << 32) | (unsigned)F[BOA_JLS_F_OFF_LO];
        const long long len = F[BOA_JLS_F_LEN];
        BOA_REQUIRE(len >= 0 && off <= data_bytes && (unsigned long long)((len + 3) & ~3ll) <= data_bytes - off,
                    "boa_jls_decode: frame %d: bytes [%llu, +%lld) and their padding outside the %zu-byte buffer", f, off, len, data_bytes);
        BOA_REQUIRE((off & 3u) == 0, "boa_jls_decode: frame %d: offset %llu is not a multiple of 4", f, off);
        BOA_REQUIRE(jls_params_valid(F[BOA_JLS_F_MAXVAL], F[BOA_JLS_F_NEAR], F[BOA_JLS_F_T1], F[BOA_JLS_F_T2], F[BOA_JLS_F_T3],
                                     F[BOA_JLS_F_RESET]),
                    "boa_jls_decode: frame %d: coding parameters MAXVAL %d NEAR %d T1 %d T2 %d T3 %d RESET %d out of range", f,
                    F[BOA_JLS_F_MAXVAL], F[BOA_JLS_F_NEAR], F[BOA_JLS_F_T1], F[BOA_JLS_F_T2], F[BOA_JLS_F_T3], F[BOA_JLS_F_RESET]);
        tab[f] = JlsFrame{off, (unsigned)len, F[BOA_JLS_F_MAXVAL], F[BOA_JLS_F_NEAR], F[BOA_JLS_F_T1], F[BOA_JLS_F_T2],
                          F[BOA_JLS_F_T3], F[BOA_JLS_F_RESET], 0};
        in_bytes += (double)len;
    }
    const bool plain = serial || cols > BOA_JLS_WAVE_MAX_COLS;
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t stb = up((size_t)n_frames * 4), ftb = up((size_t)n_frames * sizeof(JlsFrame));
    const size_t wsb = plain ? up((size_t)n_frames * JLS_CONTEXTS * sizeof(JlsCtx)) : 0;
    unsigned char* blk = nullptr;
    BOA_TRY(boa_malloc(c, stb + ftb + wsb, (void**)&blk));
    int* d_status = (int*)blk;
    JlsFrame* d_frames = (JlsFrame*)(blk + stb);
    JlsCtx* d_ws = (JlsCtx*)(blk + stb + ftb);
    hipError_t e = hipMemsetAsync(d_status, 0, (size_t)n_frames * 4, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_frames, tab.data(), (size_t)n_frames * sizeof(JlsFrame), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        c->prof_break = true;
        KernelTimer t(c, BOA_K_OTHER, 0, in_bytes + (double)n_frames * rows * cols * 2);
        if (plain) {
            hipLaunchKernelGGL(k_jls_serial, dim3((unsigned)((n_frames + WAVE - 1) / WAVE)), dim3(WAVE), 0, c->stream, dev_data, d_frames,
                               n_frames, rows, cols, dev_out, d_ws, d_status);
        } else {
            const size_t lds = (size_t)cols * 4 + (size_t)2 * ((cols + 1) & ~1) * 2;
            hipLaunchKernelGGL(k_jls_wave, dim3((unsigned)n_frames), dim3(WAVE), lds, c->stream, dev_data, d_frames, rows, cols, dev_out,
                               d_status);
        }
        t.stop();
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host_status, d_status, (size_t)n_frames * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    boa_free(c, blk);
    BOA_HIP_TRY(e);
    return BOA_OK;
}
