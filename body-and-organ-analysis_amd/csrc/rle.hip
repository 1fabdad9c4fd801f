// RLE Lossless decode of a DICOM series on the device (transfer syntax 1.2.840.10008.1.2.5, PS3.5 Annex G): every frame is one
// PackBits stream per byte plane of its samples, most significant plane first.  A stream is a chain of control bytes, sequential
// by nature; but a control advances the read position by at most 129 bytes, so a chunk of a stream can be entered at 129 offsets
// only.  k_rle_chunk_map answers all 129 for every chunk in parallel, k_rle_chain strings the answers together (one lane per
// stream, one table lookup per chunk), k_rle_expand decodes every chunk from its now known entry, k_rle_interleave puts the byte
// planes together.  Nothing is speculated and nothing is repeated; every loop is bounded by the chunk size (rle_codes.h).
// k_rle_serial is the plain loop, one lane per stream: the reference the tests compare with.
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "rle_codes.h"

namespace {

constexpr int NT = 256;                          // lanes of a chunk's workgroup

// workspace of one group of frames: 1 GiB, or BOA_RLE_WS_MB MiB (read at every call; small values let a test reach the grouping)
size_t ws_cap() {
    const char* v = getenv("BOA_RLE_WS_MB");
    const long mb = v ? atol(v) : 0;
    return mb > 0 ? (size_t)mb << 20 : size_t(1) << 30;
}

struct RleSeg {
    unsigned long long lo;       // first byte in the data buffer
    unsigned len;
    unsigned chunk_first;        // in the group's chunk arrays
    unsigned n_chunks;
    int frame;                   // in the batch
    int slot;                    // plane slot in the group's plane buffer: 2 x (frame in group) + plane
    int pad;
};

// One workgroup per chunk: the node of every position (one control step), rle_rounds(cb) rounds of pointer doubling over two LDS
// buffers, then the 129 table words.  The rounds do not depend on the bytes.
__global__ __launch_bounds__(NT) void k_rle_chunk_map(const uint8_t* __restrict__ data, const RleSeg* __restrict__ segs,
                                                      const unsigned* __restrict__ chunk_seg, unsigned cb, unsigned* __restrict__ table) {
    extern __shared__ unsigned lds[];
    const unsigned n = rle_nodes(cb), tid = threadIdx.x, chunk = blockIdx.x;
    unsigned* a = lds;
    unsigned* b = lds + n;
    const RleSeg s = segs[chunk_seg[chunk]];
    const unsigned start = (chunk - s.chunk_first) * cb, rest = s.len - start, len = min(cb, rest);
    const uint8_t* src = data + s.lo + start;
    for (unsigned i = tid; i < n; i += NT) a[i] = rle_node(src, rest, len, n - 1u, i);
    __syncthreads();
    for (int r = rle_rounds(cb); r > 0; --r) {
        rle_double_round(a, b, n, tid, NT);
        __syncthreads();
        unsigned* t = a;
        a = b;
        b = t;
    }
    if (tid < RLE_ENTRIES) table[(size_t)chunk * RLE_ENTRIES + tid] = rle_table_word(a[tid], len, n - 1u);
}

// One lane per segment: the chain of its chunks from entry 0; a short total is the frame's status.
__global__ void k_rle_chain(const RleSeg* __restrict__ segs, int n_segs, const unsigned* __restrict__ table, unsigned npix,
                            unsigned* __restrict__ entry, unsigned* __restrict__ base, int* __restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_segs) return;
    const RleSeg s = segs[i];
    const unsigned long long total = rle_chain(table + (size_t)s.chunk_first * RLE_ENTRIES, s.n_chunks, npix, entry + s.chunk_first,
                                               base + s.chunk_first);
    if (total < npix) atomicCAS(status + s.frame, 0, BOA_RLE_TRUNCATED);
}

// One workgroup per live chunk.  The chunk's bytes (and the up to 128 operand bytes behind it) go to LDS; the positions on the
// chain from the chunk's entry are marked with their output offsets by the same doubling rounds; the marked positions whose
// control produces bytes are compacted into the run list; then lane l writes output bytes l, l + NT, ..: consecutive lanes,
// consecutive bytes, each found by a binary search of the run list.  The output is clipped at npix.
__global__ __launch_bounds__(NT) void k_rle_expand(const uint8_t* __restrict__ data, const RleSeg* __restrict__ segs,
                                                   const unsigned* __restrict__ chunk_seg, unsigned cb, const unsigned* __restrict__ entry,
                                                   const unsigned* __restrict__ base, unsigned npix, size_t plane_stride,
                                                   uint8_t* __restrict__ planes) {
    extern __shared__ unsigned lds[];
    __shared__ unsigned scan[NT];
    const unsigned n = rle_nodes(cb), tid = threadIdx.x, chunk = blockIdx.x;
    const unsigned e = entry[chunk];
    if (e == RLE_NOT_LIVE) return;                                   // (uniform over the workgroup)
    unsigned* a = lds;
    unsigned* b = lds + n;
    unsigned* mark = lds + 2 * n;
    uint8_t* bytes = (uint8_t*)(lds + 3 * n);                        // cb + 128
    const RleSeg s = segs[chunk_seg[chunk]];
    const unsigned start = (chunk - s.chunk_first) * cb, rest = s.len - start, len = min(cb, rest);
    const unsigned avail = min(cb + RLE_MAX_STEP - 1u, rest);
    const uint8_t* src = data + s.lo + start;
    for (unsigned i = tid; i < avail; i += NT) bytes[i] = src[i];
    __syncthreads();
    for (unsigned i = tid; i < n; i += NT) {
        a[i] = rle_node(bytes, rest, len, n - 1u, i);
        mark[i] = i == e ? 0u : RLE_NOT_LIVE;
    }
    __syncthreads();
    for (int r = rle_rounds(cb); r > 0; --r) {
        rle_mark_round(a, mark, n, tid, NT);
        rle_double_round(a, b, n, tid, NT);
        __syncthreads();
        unsigned* t = a;
        a = b;
        b = t;
    }
    const unsigned produced = rle_count(a[e]);
    // the run list (in b, free now): lane t looks at positions [t per, (t + 1) per)
    const unsigned per = cb / NT, p0 = tid * per;
    unsigned mine = 0;
    for (unsigned p = p0; p < p0 + per; ++p) mine += rle_run_at(bytes, rest, len, n - 1u, mark, p) != RLE_NOT_LIVE;
    scan[tid] = mine;
    __syncthreads();
    for (unsigned d = 1; d < NT; d <<= 1) {
        const unsigned v = tid >= d ? scan[tid - d] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const unsigned n_runs = scan[NT - 1];
    unsigned at = scan[tid] - mine;
    unsigned* runs = b;
    for (unsigned p = p0; p < p0 + per; ++p) {
        const unsigned w = rle_run_at(bytes, rest, len, n - 1u, mark, p);
        if (w != RLE_NOT_LIVE) runs[at++] = w;
    }
    __syncthreads();
    const unsigned o0 = base[chunk];
    const unsigned n_out = n_runs ? min(produced, npix - o0) : 0u;
    uint8_t* out = planes + (size_t)s.slot * plane_stride + o0;
    for (unsigned o = tid; o < n_out; o += NT) out[o] = rle_run_byte(bytes, rle_find_run(runs, n_runs, o), o);
}

// out[f][i] = plane 0 (the most significant byte) << 8 | plane 1; a frame of one plane is widened
__global__ void k_rle_interleave(const uint8_t* __restrict__ planes, size_t plane_stride, const int* __restrict__ frame_planes,
                                 int f0, unsigned npix, uint16_t* __restrict__ out) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = blockIdx.y;                                        // frame in the group
    if (i >= npix) return;
    const uint8_t* p = planes + (size_t)(2 * g) * plane_stride;
    const unsigned hi = p[i];
    out[(size_t)(f0 + g) * npix + i] = (uint16_t)(frame_planes[f0 + g] == 2 ? (hi << 8) | p[plane_stride + i] : hi);
}

// the plain loop, one lane per segment
__global__ void k_rle_serial(const uint8_t* __restrict__ data, const RleSeg* __restrict__ segs, int n_segs, unsigned npix,
                             size_t plane_stride, uint8_t* __restrict__ planes, int* __restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_segs) return;
    const RleSeg s = segs[i];
    if (rle_decode_serial(data + s.lo, s.len, planes + (size_t)s.slot * plane_stride, npix) < npix)
        atomicCAS(status + s.frame, 0, BOA_RLE_TRUNCATED);
}

}  // namespace

extern "C" int boa_rle_decode(boa_ctx* c, const uint8_t* dev_data, size_t data_bytes, int n_frames, const int* frames, int rows,
                              int cols, int chunk_bytes, uint16_t* dev_out, int* host_status, int serial) {
    BOA_REQUIRE(c && dev_data && frames && dev_out && host_status, "boa_rle_decode: NULL argument");
    BOA_REQUIRE(n_frames > 0, "boa_rle_decode: empty batch");
    BOA_REQUIRE(rows >= 1 && rows <= 65535 && cols >= 1 && cols <= 65535, "boa_rle_decode: frame size %d x %d", rows, cols);
    BOA_REQUIRE(chunk_bytes >= (int)RLE_CHUNK_MIN && chunk_bytes <= (int)RLE_CHUNK_MAX && (chunk_bytes & (chunk_bytes - 1)) == 0,
                "boa_rle_decode: chunk_bytes %d (a power of two in %u .. %u)", chunk_bytes, RLE_CHUNK_MIN, RLE_CHUNK_MAX);
    const unsigned cb = (unsigned)chunk_bytes, npix = (unsigned)rows * (unsigned)cols;
    const size_t plane_stride = ((size_t)npix + 15) & ~size_t(15);
    // every offset the kernels follow is checked here, on the host, before anything reaches the device
    std::vector<RleSeg> segs;
    std::vector<unsigned> chunk_seg;
    std::vector<int> frame_planes(n_frames);
    struct Group { int f0, nf; size_t s0, ns, c0, nc; };
    std::vector<Group> groups;
    Group g{0, 0, 0, 0, 0, 0};
    const size_t cap = ws_cap();
    auto ws_of = [&](size_t nf, size_t nc) { return nf * 2 * plane_stride + nc * (RLE_ENTRIES + 2) * 4; };
    for (int f = 0; f < n_frames; ++f) {
        const int* F = frames + (size_t)f * BOA_RLE_FRAME_WORDS;
        const unsigned long long off = ((unsigned long long)(unsigned)F[BOA_RLE_F_OFF_HI] << 32) | (unsigned)F[BOA_RLE_F_OFF_LO];
        const long long len = F[BOA_RLE_F_LEN];
        const int ns = F[BOA_RLE_F_N_SEG];
        BOA_REQUIRE(len >= 0 && off <= data_bytes && (unsigned long long)len <= data_bytes - off,
                    "boa_rle_decode: frame %d: bytes [%llu, +%lld) outside the %zu-byte buffer", f, off, len, data_bytes);
        BOA_REQUIRE(ns == 1 || ns == 2, "boa_rle_decode: frame %d: %d segments (1 or 2)", f, ns);
        size_t nc = 0;
        for (int k = 0; k < ns; ++k) {
            const long long lo = F[BOA_RLE_F_SEG + 2 * k], hi = F[BOA_RLE_F_SEG + 2 * k + 1];
            BOA_REQUIRE(lo >= 0 && lo <= hi && hi <= len,
                        "boa_rle_decode: frame %d segment %d: bytes [%lld, %lld) outside its %lld-byte frame", f, k, lo, hi, len);
            nc += (size_t)((hi - lo + cb - 1) / cb);
        }
        if (g.nf > 0 && (ws_of(g.nf + 1, g.nc + nc) > cap || g.nf == 65535)) {      // (65535: the interleave grid's y extent)
            groups.push_back(g);
            g = Group{f, 0, segs.size(), 0, chunk_seg.size(), 0};
        }
        for (int k = 0; k < ns; ++k) {
            const unsigned lo = (unsigned)F[BOA_RLE_F_SEG + 2 * k], hi = (unsigned)F[BOA_RLE_F_SEG + 2 * k + 1];
            RleSeg s{off + lo, hi - lo, (unsigned)g.nc, (hi - lo + cb - 1) / cb, f, 2 * g.nf + k, 0};
            for (unsigned j = 0; j < s.n_chunks; ++j) chunk_seg.push_back((unsigned)g.ns);
            g.nc += s.n_chunks;
            ++g.ns;
            segs.push_back(s);
        }
        frame_planes[f] = ns;
        ++g.nf;
    }
    groups.push_back(g);
    size_t max_nf = 0, max_ns = 0, max_nc = 0;
    for (const Group& k : groups) {
        max_nf = std::max(max_nf, (size_t)k.nf);
        max_ns = std::max(max_ns, k.ns);
        max_nc = std::max(max_nc, k.nc);
    }
    BOA_REQUIRE(max_nc < (size_t(1) << 31), "boa_rle_decode: %zu chunks in one group of frames", max_nc);

    // one block: status and planes-per-frame of the batch; segments, chunk -> segment, planes, table, entry, base of a group
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t stb = up((size_t)n_frames * 4), fpb = stb, sgb = up(max_ns * sizeof(RleSeg)), csb = up(max_nc * 4);
    const size_t plb = up(max_nf * 2 * plane_stride), tbb = up(max_nc * RLE_ENTRIES * 4), enb = csb;
    unsigned char* blk = nullptr;
    BOA_TRY(boa_malloc(c, stb + fpb + sgb + csb + plb + tbb + 2 * enb, (void**)&blk));
    int* d_status = (int*)blk;
    int* d_frame_planes = (int*)(blk + stb);
    RleSeg* d_segs = (RleSeg*)(blk + stb + fpb);
    unsigned* d_chunk_seg = (unsigned*)(blk + stb + fpb + sgb);
    uint8_t* d_planes = blk + stb + fpb + sgb + csb;
    unsigned* d_table = (unsigned*)(d_planes + plb);
    unsigned* d_entry = (unsigned*)(d_planes + plb + tbb);
    unsigned* d_base = (unsigned*)(d_planes + plb + tbb + enb);
    const size_t lds_map = (size_t)2 * rle_nodes(cb) * 4, lds_expand = (size_t)3 * rle_nodes(cb) * 4 + cb + 128;
    hipError_t e = hipMemsetAsync(d_status, 0, (size_t)n_frames * 4, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_frame_planes, frame_planes.data(), (size_t)n_frames * 4, hipMemcpyHostToDevice, c->stream);
    for (const Group& k : groups) {
        if (e != hipSuccess) break;
        e = hipMemcpyAsync(d_segs, segs.data() + k.s0, k.ns * sizeof(RleSeg), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && k.nc && !serial)
            e = hipMemcpyAsync(d_chunk_seg, chunk_seg.data() + k.c0, k.nc * 4, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) break;
        c->prof_break = true;
        // bytes: the input twice and the table written and read by the chain (one word per chunk); the planes written and read
        KernelTimer t(c, BOA_K_OTHER, 0, 2.0 * (double)k.nc * cb + (double)k.nc * (RLE_ENTRIES + 5) * 4 + (double)k.nf * npix * 6);
        const int seg_grid = (int)((k.ns + 63) / 64);
        if (serial) {
            hipLaunchKernelGGL(k_rle_serial, dim3(seg_grid), dim3(64), 0, c->stream, dev_data, d_segs, (int)k.ns, npix, plane_stride,
                               d_planes, d_status);
        } else {
            if (k.nc)
                hipLaunchKernelGGL(k_rle_chunk_map, dim3((unsigned)k.nc), dim3(NT), lds_map, c->stream, dev_data, d_segs, d_chunk_seg, cb,
                                   d_table);
            hipLaunchKernelGGL(k_rle_chain, dim3(seg_grid), dim3(64), 0, c->stream, d_segs, (int)k.ns, d_table, npix, d_entry, d_base,
                               d_status);
            if (k.nc)
                hipLaunchKernelGGL(k_rle_expand, dim3((unsigned)k.nc), dim3(NT), lds_expand, c->stream, dev_data, d_segs, d_chunk_seg, cb,
                                   d_entry, d_base, npix, plane_stride, d_planes);
        }
        hipLaunchKernelGGL(k_rle_interleave, dim3((npix + 255) / 256, (unsigned)k.nf), dim3(256), 0, c->stream, d_planes, plane_stride,
                           d_frame_planes, k.f0, npix, dev_out);
        t.stop();
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host_status, d_status, (size_t)n_frames * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    boa_free(c, blk);
    BOA_HIP_TRY(e);
    return BOA_OK;
}
