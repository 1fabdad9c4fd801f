// Inflate of .nii.gz inputs (boa_inflate_streams): raw deflate streams (RFC 1951) decoded in parallel by speculating on block
// starts, in the manner of pugz and rapidgzip.  A stream (one gzip member's body, empty history) is cut into chunks of chunk_bytes
// of compressed input.
//   k_inflate_find     one workgroup per chunk, one lane per bit offset: the first offset of the chunk that passes the block-start
//                      test (a dynamic, non-final header that inf_dynamic_header accepts); a chunk without one drops out
//   k_inflate_count    one wave per live chunk, lane 0 decoding: from its start to the first block end at or beyond the next live
//                      chunk's start; counts output bytes.  The host walks the chain (inf_walk), restarts the chunk behind a false
//                      candidate at its predecessor's end and launches the flagged chunks again, INF_ROUNDS times at most
//   k_inflate_store    the same decode into 16-bit symbols: a literal, or 0x8000 | k = byte k of the 32 KiB in front of the chunk
//   k_inflate_windows  one workgroup per stream, chunk after chunk: the last 32 KiB of every chunk as bytes
//   k_inflate_resolve  one workgroup per chunk: symbols -> bytes against the predecessor's window, the chunk's CRC-32
//   k_inflate_crc      one thread per stream: the chunks' CRCs combined
// The entry compares size and CRC-32 with each member's trailer.  Malformed input never faults: the entry validates every offset
// before anything is copied, the decoder's loops consume input or are bounded by a table, a read past the stream's end returns
// zero bits and ends the chunk with a status, writes are bounded by the counted length, and errors are a status per stream.
#include <algorithm>

#include "common.h"
#include "crc32_dev.h"
#include "inflate_codes.h"

static_assert(INF_OK == BOA_INF_OK && INF_TRUNCATED == BOA_INF_TRUNCATED && INF_INVALID == BOA_INF_INVALID && INF_FAR == BOA_INF_FAR &&
                  INF_OVERRUN == BOA_INF_OVERRUN && INF_SIZE == BOA_INF_SIZE && INF_CRC == BOA_INF_CRC && INF_REPAIR == BOA_INF_REPAIR &&
                  INF_TRAILING == BOA_INF_TRAILING,
              "status codes of inflate_codes.h and boa_hip.h");

namespace {

__device__ __forceinline__ unsigned long long min_u64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

constexpr int INF_FIND_NT = 256;
constexpr int INF_WAVES = 4;                   // chunks per workgroup of the decode passes
constexpr int INF_WIN_NT = 1024;
constexpr int INF_RES_NT = 256;
constexpr int INF_ROUNDS = 8;                  // repair rounds before the caller is sent to the host path
constexpr size_t INF_MAX_SRC = (size_t)1 << 40;
constexpr size_t INF_MIN_CHUNK = 64, INF_MAX_CHUNK = (size_t)1 << 30;
constexpr size_t INF_MAX_CHUNKS = (size_t)1 << 24;

// grid = chunks.  The first chunk of a stream starts at bit 0; every other one takes the first accepted offset in [nominal, search_end).
__global__ __launch_bounds__(INF_FIND_NT) void k_inflate_find(const unsigned char* __restrict__ src, InfChunk* __restrict__ chunks) {
    __shared__ unsigned long long s_min;
    InfChunk& c = chunks[blockIdx.x];
    const int t = threadIdx.x;
    const unsigned long long lo = c.nominal, hi = c.search_end;
    if (lo == 0) {
        if (t == 0) {
            c.start = 0;
            c.flags = INF_F_LIVE | INF_F_REDO;
        }
        return;
    }
    if (t == 0) s_min = INF_NO_STOP;
    __syncthreads();
    const unsigned char* s = src + c.src_off;
    const unsigned long long len = c.src_len;
    for (unsigned long long base = lo; base < hi; base += INF_FIND_NT) {
        const unsigned long long bit = base + t;
        if (bit < hi && inf_block_start(s, len, bit)) atomicMin(&s_min, bit);
        __syncthreads();
        if (s_min != INF_NO_STOP) break;                        // (uniform: every thread reads it behind the barrier)
        __syncthreads();
    }
    if (t == 0) {
        const unsigned long long m = s_min;
        c.start = m;
        c.flags = m != INF_NO_STOP ? (INF_F_LIVE | INF_F_REDO | INF_F_CAND) : 0u;
    }
}

// One wave per chunk, lane 0 decodes; the block's tables in LDS.  STORE: into the symbol buffer (every live chunk), else counting
// (the chunks with INF_F_REDO).
template <bool STORE>
__global__ __launch_bounds__(64 * INF_WAVES) void k_inflate_decode(const unsigned char* __restrict__ src, InfChunk* __restrict__ chunks,
                                                                  unsigned nchunks, unsigned short* __restrict__ sym) {
    __shared__ InfTables s_tab[INF_WAVES];
    const unsigned wave = threadIdx.x >> 6, g = blockIdx.x * INF_WAVES + wave;
    if ((threadIdx.x & 63) != 0 || g >= nchunks) return;
    InfChunk& c = chunks[g];
    if (!(c.flags & INF_F_LIVE) || (!STORE && !(c.flags & INF_F_REDO))) return;
    uint64_t end = 0;
    int final = 0, st;
    if constexpr (STORE) {
        InfStore sink{sym + c.out_off, c.nbytes};
        st = inf_decode_chunk(src + c.src_off, c.src_len, c.start, c.stop, &s_tab[wave], sink, &end, &final);
        if (st == INF_OK && (sink.n != c.nbytes || end != c.end)) st = INF_OVERRUN;      // both passes must agree
        c.status = (unsigned)st;
    } else {
        InfCount sink;
        st = inf_decode_chunk(src + c.src_off, c.src_len, c.start, c.stop, &s_tab[wave], sink, &end, &final);
        c.end = end;
        c.nbytes = sink.n;
        c.status = (unsigned)st;
        c.final = (unsigned)final;
    }
}

// grid = streams; `live` = the live chunks in order, those of stream m at [first[m], first[m + 1]).  win[j] = the 32 KiB that end
// with chunk j's last byte (zero where that is before the stream's first byte).
__global__ __launch_bounds__(INF_WIN_NT) void k_inflate_windows(const InfChunk* __restrict__ live, const unsigned* __restrict__ first,
                                                                const unsigned short* __restrict__ sym, unsigned char* __restrict__ win) {
    const unsigned lo = first[blockIdx.x], hi = first[blockIdx.x + 1];
    const int t = threadIdx.x;
    for (unsigned j = lo; j + 1 < hi; ++j) {                   // (nothing reads the last chunk's window)
        const unsigned long long n = live[j].nbytes;
        const unsigned short* s = sym + live[j].out_off;
        const unsigned char* prev = j > lo ? win + (size_t)(j - 1) * INF_WINDOW : nullptr;
        unsigned char* w = win + (size_t)j * INF_WINDOW;
        for (int k = t; k < INF_WINDOW; k += INF_WIN_NT) {
            unsigned v = 0;
            if (n + (unsigned)k >= INF_WINDOW) {               // inside the chunk
                const unsigned sv = s[n + (unsigned)k - INF_WINDOW];
                v = (sv & 0x8000u) ? (prev ? prev[sv & 0x7fffu] : 0u) : sv;
            } else if (prev)
                v = prev[(unsigned)k + (unsigned)n];           // (k + n < 32768)
            w[k] = (unsigned char)v;
        }
        __threadfence_block();
        __syncthreads();
    }
}

// grid = live chunks.  Bytes of the chunk into dst, a marker that points before the stream's first byte = INF_FAR; then the CRC-32
// of the chunk: 256 contiguous pieces, combined by one thread.
__global__ __launch_bounds__(INF_RES_NT) void k_inflate_resolve(InfChunk* __restrict__ live, const unsigned* __restrict__ is_first,
                                                                const unsigned short* __restrict__ sym, const unsigned char* __restrict__ win,
                                                                const unsigned* __restrict__ pw, unsigned char* __restrict__ dst) {
    __shared__ unsigned s_tab[256];
    __shared__ unsigned s_crc[INF_RES_NT];
    __shared__ unsigned s_bad;
    const unsigned j = blockIdx.x;
    const int t = threadIdx.x;
    InfChunk& c = live[j];
    const unsigned long long n = c.nbytes, rel = c.rel_off;
    const unsigned short* s = sym + c.out_off;
    unsigned char* d = dst + c.out_off;
    const unsigned char* prev = is_first[j] ? nullptr : win + (size_t)(j - 1) * INF_WINDOW;
    s_tab[t] = crc32_table_entry((unsigned)t);
    if (t == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    for (unsigned long long i = t; i < n; i += INF_RES_NT) {
        unsigned v = s[i];
        if (v & 0x8000u) {
            const unsigned k = v & 0x7fffu;
            if (!prev || rel + k < INF_WINDOW) {
                bad = true;
                v = 0;
            } else
                v = prev[k];
        }
        d[i] = (unsigned char)v;
    }
    if (bad) s_bad = 1;
    __threadfence_block();
    __syncthreads();
    const unsigned long long piece = (n + INF_RES_NT - 1) / INF_RES_NT;
    const unsigned long long lo = min_u64(n, piece * (unsigned long long)t), hi = min_u64(n, lo + piece);
    s_crc[t] = crc32_update(s_tab, 0xffffffffu, d, lo, hi) ^ 0xffffffffu;
    __syncthreads();
    if (t == 0) {
        unsigned crc = 0;
        const unsigned xfull = dfl_crc_xpow(pw, piece);
        for (int k = 0; k < INF_RES_NT; ++k) {
            const unsigned long long klo = min_u64(n, piece * (unsigned long long)k), khi = min_u64(n, klo + piece);
            if (khi == klo) break;
            crc = dfl_gf2_mul(khi - klo == piece ? xfull : dfl_crc_xpow(pw, khi - klo), crc) ^ s_crc[k];
        }
        c.crc = crc;
        if (s_bad) c.status = INF_FAR;
    }
}

// one thread per stream: crc32(A || B) over its live chunks in order
__global__ void k_inflate_crc(const InfChunk* __restrict__ live, const unsigned* __restrict__ first, unsigned nstreams,
                              const unsigned* __restrict__ pw, unsigned* __restrict__ stream_crc) {
    const unsigned m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nstreams) return;
    unsigned c = 0;
    for (unsigned j = first[m]; j < first[m + 1]; ++j) c = dfl_crc_combine(pw, c, live[j].crc, live[j].nbytes);
    stream_crc[m] = c;
}

struct Stage {                                 // device events around the passes, when the caller asks for their times
    boa_ctx* c;
    float* ms;
    hipEvent_t ev[2] = {};
    bool on = false;
    Stage(boa_ctx* ctx, float* out) : c(ctx), ms(out) {
        on = ms && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    }
    ~Stage() {
        for (auto e : ev)
            if (e) hipEventDestroy(e);
    }
    void begin() {
        if (on) hipEventRecord(ev[0], c->stream);
    }
    void end(int slot) {                       // the stream has been synchronised or will be before the times are read
        if (!on) return;
        hipEventRecord(ev[1], c->stream);
        hipEventSynchronize(ev[1]);
        float v = 0;
        if (hipEventElapsedTime(&v, ev[0], ev[1]) == hipSuccess) ms[slot] += v;
    }
};

struct DevBlock {                              // a boa_malloc block that leaves with the scope
    boa_ctx* c;
    void* p = nullptr;
    explicit DevBlock(boa_ctx* ctx) : c(ctx) {}
    ~DevBlock() {
        if (p) boa_free(c, p);
    }
};

}  // namespace

extern "C" size_t boa_inflate_default_chunk(void) { return 65536; }

extern "C" int boa_inflate_streams(boa_ctx* c, const uint8_t* dev_src, size_t src_bytes, int n_streams, const uint64_t* stream_off,
                                   const uint64_t* stream_len, const uint64_t* stream_size, const uint32_t* stream_crc32,
                                   size_t chunk_bytes, uint8_t* dev_out, size_t out_capacity, int* host_status, uint64_t* host_info,
                                   float* host_ms) {
    BOA_REQUIRE(c && stream_off && stream_len && stream_size && stream_crc32 && host_status && host_info,
                "boa_inflate_streams: NULL argument");
    BOA_REQUIRE(n_streams >= 1 && n_streams <= (1 << 22), "boa_inflate_streams: %d streams", n_streams);
    BOA_REQUIRE(dev_src && src_bytes >= 1 && src_bytes <= INF_MAX_SRC, "boa_inflate_streams: %zu source bytes", src_bytes);
    BOA_REQUIRE(chunk_bytes >= INF_MIN_CHUNK && chunk_bytes <= INF_MAX_CHUNK, "boa_inflate_streams: chunk_bytes %zu outside [64, 2^30]",
                chunk_bytes);
    const unsigned ns = (unsigned)n_streams;
    size_t total_out = 0, nchunks = 0;
    std::vector<unsigned> first(ns + 1);
    for (unsigned m = 0; m < ns; ++m) {
        BOA_REQUIRE(stream_len[m] >= 1 && stream_off[m] <= src_bytes && stream_len[m] <= src_bytes - stream_off[m],
                    "boa_inflate_streams: stream %u at %llu + %llu outside the %zu source bytes", m, (unsigned long long)stream_off[m],
                    (unsigned long long)stream_len[m], src_bytes);
        BOA_REQUIRE(stream_size[m] <= INF_MAX_SRC && total_out + stream_size[m] <= out_capacity,
                    "boa_inflate_streams: stream %u of %llu bytes passes out_capacity %zu", m, (unsigned long long)stream_size[m], out_capacity);
        total_out += stream_size[m];
        first[m] = (unsigned)nchunks;
        nchunks += (stream_len[m] + chunk_bytes - 1) / chunk_bytes;
        BOA_REQUIRE(nchunks <= INF_MAX_CHUNKS, "boa_inflate_streams: more than 2^24 chunks (chunk_bytes %zu)", chunk_bytes);
    }
    first[ns] = (unsigned)nchunks;
    BOA_REQUIRE(dev_out || total_out == 0, "boa_inflate_streams: NULL output");
    for (int k = 0; k < BOA_INF_INFO_WORDS; ++k) host_info[k] = 0;
    if (host_ms)
        for (int k = 0; k < BOA_INF_MS_WORDS; ++k) host_ms[k] = 0;

    std::vector<InfChunk> ch(nchunks);
    for (unsigned m = 0; m < ns; ++m)
        for (unsigned g = first[m]; g < first[m + 1]; ++g) {
            InfChunk& k = ch[g];
            k = InfChunk{};
            k.src_off = stream_off[m];
            k.src_len = stream_len[m];
            k.nominal = 8ull * (g - first[m]) * chunk_bytes;
            k.search_end = std::min<uint64_t>(k.nominal + 8ull * chunk_bytes, 8ull * stream_len[m]);
            k.stream = m;
        }
    const size_t table_b = nchunks * sizeof(InfChunk);
    DevBlock tab(c), work(c);
    BOA_TRY(boa_malloc(c, table_b + sizeof(DflCrcPow), &tab.p));
    InfChunk* d_ch = (InfChunk*)tab.p;
    unsigned* d_pw = (unsigned*)((unsigned char*)tab.p + table_b);
    BOA_HIP_TRY(hipMemcpyAsync(d_ch, ch.data(), table_b, hipMemcpyHostToDevice, c->stream));
    BOA_HIP_TRY(hipMemcpyAsync(d_pw, crc_pow().x, sizeof(DflCrcPow), hipMemcpyHostToDevice, c->stream));
    c->prof_break = true;
    Stage stage(c, host_ms);

    // ---- find ----
    stage.begin();
    hipLaunchKernelGGL(k_inflate_find, dim3((unsigned)nchunks), dim3(INF_FIND_NT), 0, c->stream, dev_src, d_ch);
    stage.end(BOA_INF_MS_FIND);
    BOA_HIP_TRY(hipGetLastError());
    BOA_HIP_TRY(hipMemcpyAsync(ch.data(), d_ch, table_b, hipMemcpyDeviceToHost, c->stream));
    BOA_HIP_TRY(hipStreamSynchronize(c->stream));
    for (unsigned m = 0; m < ns; ++m) {
        uint64_t stop = INF_NO_STOP;
        for (unsigned g = first[m + 1]; g-- > first[m];)
            if (ch[g].flags & INF_F_LIVE) {
                ch[g].stop = stop;
                stop = ch[g].start;
                if (ch[g].flags & INF_F_CAND) ++host_info[BOA_INF_I_CANDIDATES];
            }
    }
    host_info[BOA_INF_I_CHUNKS] = nchunks;

    // ---- count, walk, repair ----
    std::vector<int> status(ns, INF_OK);
    const unsigned dec_grid = (unsigned)((nchunks + INF_WAVES - 1) / INF_WAVES);
    for (int round = 0;; ++round) {
        BOA_HIP_TRY(hipMemcpyAsync(d_ch, ch.data(), table_b, hipMemcpyHostToDevice, c->stream));
        stage.begin();
        hipLaunchKernelGGL(k_inflate_decode<false>, dim3(dec_grid), dim3(64 * INF_WAVES), 0, c->stream, dev_src, d_ch, (unsigned)nchunks,
                           (unsigned short*)nullptr);
        stage.end(BOA_INF_MS_COUNT);
        BOA_HIP_TRY(hipGetLastError());
        BOA_HIP_TRY(hipMemcpyAsync(ch.data(), d_ch, table_b, hipMemcpyDeviceToHost, c->stream));
        BOA_HIP_TRY(hipStreamSynchronize(c->stream));
        for (auto& k : ch) k.flags &= ~INF_F_REDO;
        unsigned redo = 0;
        for (unsigned m = 0; m < ns; ++m) {
            if (status[m] != INF_OK) continue;
            const InfWalk w = inf_walk(ch.data(), first[m], first[m + 1] - first[m]);
            status[m] = w.status;
            host_info[BOA_INF_I_REJECTED] += w.rejected;
            if (w.status == INF_OK) redo += w.redo;
        }
        if (!redo) break;
        host_info[BOA_INF_I_ROUNDS] = (uint64_t)round + 1;
        if (round + 1 > INF_ROUNDS) {
            for (unsigned m = 0; m < ns; ++m)
                if (status[m] == INF_OK) status[m] = INF_REPAIR;      // (a stream without a flagged chunk is complete, but the call is not)
            break;
        }
    }

    // ---- offsets; the sizes against the trailers ----
    std::vector<InfChunk> live;
    std::vector<unsigned> lfirst(ns + 1), is_first;
    bool all_ok = true;
    {
        uint64_t out_off = 0;
        for (unsigned m = 0; m < ns; ++m) {
            lfirst[m] = (unsigned)live.size();
            uint64_t rel = 0;
            if (status[m] == INF_OK) {
                for (unsigned g = first[m]; g < first[m + 1]; ++g)
                    if (ch[g].flags & INF_F_LIVE) {
                        if (ch[g].nbytes > stream_size[m] - rel) {      // (no sum passes the checked size)
                            status[m] = INF_SIZE;
                            break;
                        }
                        ch[g].rel_off = rel;
                        ch[g].out_off = out_off + rel;
                        is_first.push_back(rel == 0 && live.size() == lfirst[m] ? 1u : 0u);
                        live.push_back(ch[g]);
                        rel += ch[g].nbytes;
                    }
                if (status[m] == INF_OK && rel != stream_size[m]) status[m] = INF_SIZE;
            }
            all_ok = all_ok && status[m] == INF_OK;
            out_off += stream_size[m];
        }
        lfirst[ns] = (unsigned)live.size();
    }
    host_info[BOA_INF_I_LIVE] = live.size();
    if (!all_ok) {                                                     // the caller takes its host path: nothing else is launched
        for (unsigned m = 0; m < ns; ++m) host_status[m] = status[m];
        return BOA_OK;
    }

    // ---- workspace: 2 B per output byte, a window per live chunk, the tables; checked before the launches ----
    const size_t nlive = live.size();
    const size_t sym_b = (total_out * 2 + 15) & ~(size_t)15, win_b = nlive * (size_t)INF_WINDOW, live_b = nlive * sizeof(InfChunk);
    const size_t idx_b = ((ns + 1 + nlive + ns) * 4 + 15) & ~(size_t)15;
    BOA_REQUIRE(total_out <= INF_MAX_SRC && sym_b / 2 >= total_out, "boa_inflate_streams: %zu output bytes", total_out);
    BOA_TRY(boa_malloc(c, sym_b + win_b + live_b + idx_b, &work.p));
    unsigned short* d_sym = (unsigned short*)work.p;
    unsigned char* d_win = (unsigned char*)work.p + sym_b;
    InfChunk* d_live = (InfChunk*)((unsigned char*)work.p + sym_b + win_b);
    unsigned* d_first = (unsigned*)((unsigned char*)work.p + sym_b + win_b + live_b);
    unsigned* d_isfirst = d_first + ns + 1;
    unsigned* d_scrc = d_isfirst + nlive;
    BOA_HIP_TRY(hipMemcpyAsync(d_live, live.data(), live_b, hipMemcpyHostToDevice, c->stream));
    BOA_HIP_TRY(hipMemcpyAsync(d_first, lfirst.data(), (ns + 1) * 4, hipMemcpyHostToDevice, c->stream));
    BOA_HIP_TRY(hipMemcpyAsync(d_isfirst, is_first.data(), nlive * 4, hipMemcpyHostToDevice, c->stream));
    stage.begin();
    hipLaunchKernelGGL(k_inflate_decode<true>, dim3((unsigned)((nlive + INF_WAVES - 1) / INF_WAVES)), dim3(64 * INF_WAVES), 0, c->stream,
                       dev_src, d_live, (unsigned)nlive, d_sym);
    stage.end(BOA_INF_MS_STORE);
    stage.begin();
    hipLaunchKernelGGL(k_inflate_windows, dim3(ns), dim3(INF_WIN_NT), 0, c->stream, d_live, d_first, d_sym, d_win);
    stage.end(BOA_INF_MS_WINDOWS);
    stage.begin();
    hipLaunchKernelGGL(k_inflate_resolve, dim3((unsigned)nlive), dim3(INF_RES_NT), 0, c->stream, d_live, d_isfirst, d_sym, d_win, d_pw, dev_out);
    hipLaunchKernelGGL(k_inflate_crc, dim3((ns + 63) / 64), dim3(64), 0, c->stream, d_live, d_first, ns, d_pw, d_scrc);
    stage.end(BOA_INF_MS_RESOLVE);
    BOA_HIP_TRY(hipGetLastError());
    std::vector<unsigned> scrc(ns);
    BOA_HIP_TRY(hipMemcpyAsync(live.data(), d_live, live_b, hipMemcpyDeviceToHost, c->stream));
    BOA_HIP_TRY(hipMemcpyAsync(scrc.data(), d_scrc, ns * 4, hipMemcpyDeviceToHost, c->stream));
    BOA_HIP_TRY(hipStreamSynchronize(c->stream));
    for (unsigned m = 0; m < ns; ++m) {
        for (unsigned j = lfirst[m]; j < lfirst[m + 1] && status[m] == INF_OK; ++j) status[m] = (int)live[j].status;
        if (status[m] == INF_OK && scrc[m] != stream_crc32[m]) status[m] = INF_CRC;
        host_status[m] = status[m];
    }
    return BOA_OK;
}
