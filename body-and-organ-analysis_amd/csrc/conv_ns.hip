// k_conv_ns: wave-specialised persistent implicit-GEMM 3x3x3 conv whose consumer waves split the COUT axis (gfx950).
//
// k_conv_ws (conv_ws.hip) gives each of its four consumer waves its own voxels and ONE 32-cout chunk per staged halo: a layer
// with Cout = 128 ... 320 stages every input halo Cout / 32 times and streams the chunk's weights through LDS for every tile.
// That is the right trade for the full-resolution 32-channel layers and the wrong one for the stride-2 and deep layers
// (profiles/r02_per_layer.txt: 150-400 TFLOP/s, producer / L2 bound).  Here
//   * the block's output tile is 4 x-planes of 4 x 8 voxels (M-tile = one plane = 32 voxels) and all four consumer waves work
//     on the SAME voxels with DIFFERENT cout chunks (cout group = 4 chunks = 128 couts per staged halo);
//   * a wave's weight (A) fragments are therefore private to it: they go straight from global / L2 into registers (scalar
//     base + lane offset, a ring of three (dy, dz) tap groups, prefetched two groups = 24 MFMAs ahead, across chunk and tile
//     boundaries) -- no weight staging, no LDS space, no LDS reads for weights;
//   * the input (B) fragments come from the LDS halo with reuse along x: per (dy, dz) group the wave reads the S * 3 + 3 input
//     planes once and feeds 12 MFMAs (plane j serves the outputs r with 2 r + dx = j), 0.75 KiB of LDS reads per MFMA;
//   * producers (waves 4-7), tile sequence / virtual workgroups / run tables, deferred InstanceNorm in the staging, bias as the
//     first MFMA's C operand, register-transpose epilogue and batch-invariant statistics are k_conv_ws's (conv_ws_dev.h).
// tools/consumer_ns.hip is the isolated consumer loop (1.4-1.6 PFLOP/s with random operands, weights up to 5 MB from L2).
// Instantiated for 3x3x3 kernels with stride 2 on all axes; everything else stays on k_conv_ws.
#include <stdlib.h>

#include "conv.h"

#include "conv_ws_dev.h"

// ---- LDS halo layout ("SW") -----------------------------------------------------------------------------
// A consumer lane's voxel of M-tile plane x is (y, z) = (2 ly + dy, 2 lz + dz): in the linear [x][y][z] halo the 32 lanes of a k-half
// sit 32 bytes apart along z and 2 * 17 * 16 = 544 bytes apart along y, i.e. on EVEN 16-byte slots only and on the same slots (mod 256
// bytes) in three of the four ly rows -- ds_read_b128 is serviced in four fixed 16-lane groups ({0-3, 12-15, 20-27}, ...: hardware
// guide, LDS table), and every group met 3-way bank conflicts: the fragment reads of the stride-2 layers cost three LDS cycles where
// one would do, on an LDS that the 0.75 - 0.83 KiB of reads per MFMA already fills (round-5 trace: 2 800 cycles per chunk of 54 MFMAs).
// The stride-2 halo is therefore stored DE-INTERLEAVED by the parity of y and z:
//   slot(x, y, z) = (x * 9 + yp(y)) * 24 + zp(z),   yp(y) = (y & 1) * 5 + (y >> 1),   zp(z) = (z & 1) * 10 + (z >> 1)
// (9 x 9 x 17 halo: 5 even + 4 odd rows, 9 even + 8 odd columns).  A tap's 32 voxels are then (ly, lz) -> const + ly * 24 + lz:
// 8 contiguous slots per row, rows 24 slots = 384 bytes apart (= 128 mod 256), so each of the four lane groups covers the 16 slots
// of a 256-byte bank row exactly once; the tap offsets stay compile-time immediates.  The producers' stores (8-lane groups = 4
// consecutive voxels x 2 k-half planes, 128-byte bank rows) stay conflict-free with the odd columns at slot 10 (= 2 mod 8) and the
// planes' 64-byte skew.  Lanes past the halo store into one dummy slot behind the plane.
#define NS_SW_ROW 24
#define NS_SW_YODD 5
#define NS_SW_ZODD 10
__host__ __device__ constexpr int ns_sw_yp(int y) { return (y & 1) * NS_SW_YODD + (y >> 1); }
__host__ __device__ constexpr int ns_sw_zp(int z) { return (z & 1) * NS_SW_ZODD + (z >> 1); }
__host__ __device__ constexpr int ns_sw_slots() { return 9 * 9 * NS_SW_ROW; }            // slots of one k-half plane (+ 8 of padding: the dummy slot)
__host__ __device__ constexpr int ns_sw_plane_bytes() { return (ns_sw_slots() + 8) * 16 + 64; }   // = 64 mod 128: the k-half planes' stores interleave

// The block tile is 4 x 4 x 8 output voxels at stride 2 (conv_ns_tile): a 9 x 9 x 17 halo, NS_ITEMS rounds of WS_PROD / 2 voxels
#define NS_HV (9 * 9 * 17)
#define NS_ITEMS ((NS_HV + WS_PROD / 2 - 1) / (WS_PROD / 2))
static_assert(NS_ITEMS <= WS_MAXV, "k_conv_ns: halo items per producer lane");

// prod_setup_desc / prod_setup (conv_ws_dev.h) for the NS_ITEMS items of this halo: the input voxel indices of the tile's items; returns
// the mask of the items inside the input tensor.  (Own copy: a ProdItems stays partly in scratch -- hipcc merges the classes' stores of
// its last members into one store to a selected address -- and a scratch load among the halo loads is waited for with a vmcnt(0).)
__device__ __forceinline__ unsigned ns_setup_desc(const ConvArgs& p, const TileDesc& d, const ProdConst& k, int (&gi)[NS_ITEMS]) {
    const int cls = (d.flags >> 4) & 3;
    const int base = d.ibase;
    unsigned okm;
    if (cls == 0) {
        okm = k.in_halo;
#pragma unroll
        for (int j = 0; j < NS_ITEMS; ++j) gi[j] = base + k.rel[j];
    } else if (cls == 1) {
        unsigned out = 0;
#pragma unroll
        for (int f = 0; f < 6; ++f) out |= (d.flags >> (8 + f)) & 1 ? k.face[f] : 0u;
        okm = k.in_halo & ~out;
#pragma unroll
        for (int j = 0; j < NS_ITEMS; ++j) gi[j] = ((okm >> j) & 1u) ? base + k.rel[j] : 0;
    } else {   // the halo sticks out further (a volume smaller than a tile): per-item range checks as in prod_setup
        const int ix0 = d.tc.ox0 * p.s0 - p.p0, iy0 = d.tc.oy0 * p.s1 - p.p1, iz0 = d.tc.oz0 * p.s2 - p.p2;
        okm = 0;
#pragma unroll
        for (int j = 0; j < NS_ITEMS; ++j) {
            const unsigned ix = (unsigned)(ix0 + (k.hc[j] & 1023)), iy = (unsigned)(iy0 + ((k.hc[j] >> 10) & 1023)),
                           iz = (unsigned)(iz0 + (k.hc[j] >> 20));
            const unsigned ok = (unsigned)(ix < (unsigned)p.Di) & (unsigned)(iy < (unsigned)p.Hi) & (unsigned)(iz < (unsigned)p.Wi) &
                                ((k.in_halo >> j) & 1u);
            gi[j] = ok ? base + k.rel[j] : 0;
            okm |= ok << j;
        }
    }
    return okm;
}

// A producer lane's registers.  d: its octet of its halo voxels, ONE set: an item of the chunk being committed until it is stored, then
// the same item of the chunk after it.  s0 / s1, ok, live, has_ss: the (scale, shift) words (4 channel pairs x {scales, shifts}), the
// masks (bit j: voxel j is inside the input tensor / belongs to the halo) and the transform flag of the chunk whose loads are in
// flight; ns_roll_sw copies them when that chunk's commit begins.  (u32x4_t: a loop-carried uint4 is four scalars to hipcc, see touch128.)
struct NsRegs {
    u32x4_t d[NS_ITEMS];
    u32x4_t s0, s1;
    unsigned ok, live;
    int has_ss;
};

// item j of prod_commit / prod_commit_x3 (conv_ws_dev.h) with a per-item LDS offset instead of the linear voxel index
template <bool X3, bool SS, bool EDGE>
__device__ __forceinline__ void ns_commit_item_sw(const ConvArgs& p, const u32x4_t& d, const unsigned (&w)[8], bool ok, unsigned char* d0, int off,
                                                  int plane, unsigned slope2) {
    if constexpr (X3) {
        float y[4] = {__uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z), __uint_as_float(d.w)};
        if (SS) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float f = __builtin_fmaf(y[i], __uint_as_float(w[2 * i]), __uint_as_float(w[2 * i + 1]));
                y[i] = f > 0.f ? f : f * p.slope;
            }
        }
        uint2 hi, lo;
        x3_split4(y, hi, lo);
        if (EDGE && !ok) hi = lo = make_uint2(0, 0);
        *(uint2*)(d0 + off) = hi;
        *(uint2*)(d0 + plane + off) = lo;
    } else {
        uint4 o = make_uint4(d.x, d.y, d.z, d.w);
        if (SS) o = norm_act8_pk(o, w, slope2);
        if (EDGE && !ok) o = make_uint4(0, 0, 0, 0);
        *(uint4*)(d0 + off) = o;
    }
}

// One producer interval, rolling: item j of the chunk in rg.d is normalised and stored, and the register it leaves takes item j of
// the following chunk (ISSUE; its source `nbase`, its voxel indices `gi`) -- the loads of a chunk go out while the one before it is
// committed, with one register set and one chunk's bytes in flight.  The waits are hipcc's: loads return in order, behind item j are
// NS_ITEMS - 1 - j items of its chunk, the two (scale, shift) loads and j items of the next chunk, and the compiled loop waits with
// s_waitcnt vmcnt(10) in front of every item (profiles/r12_ns_rolling_isa_waits.txt; 12 would do).
template <bool X3, bool SS, bool EDGE, bool ISSUE>
__device__ __forceinline__ void ns_roll_items_sw(const ConvArgs& p, NsRegs& rg, const unsigned (&w_in)[8], unsigned ok, unsigned char* d0,
                                                 const int (&off)[WS_MAXV], int plane, unsigned slope2, const unsigned char* nbase,
                                                 const int (&gi)[NS_ITEMS], int q, int dbg) {
    // The copies differ in their marker, and the (scale, shift) words pass through it: hipcc otherwise merges the copies back into one
    // path with per-item masks, or hoists the transform of ALL items in front of the branch that picks the copy -- behind a vmcnt(0).
    unsigned w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = w_in[i];
#define NS_ROLL_MARK(text) \
    asm volatile(text : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(slope2))
    if (EDGE)
        NS_ROLL_MARK("; roll sw: edge tile");
    else
        NS_ROLL_MARK("; roll sw: interior tile");
#undef NS_ROLL_MARK
#pragma unroll
    for (int j = 0; j < NS_ITEMS; ++j) {
        if (!(dbg & 32)) ns_commit_item_sw<X3, SS, EDGE>(p, rg.d[j], w, (ok >> j) & 1u, d0, off[j], plane, slope2);
        // (the load stays behind the store of the item whose register it takes: scheduled ahead of it, it gets a register of its own)
        __builtin_amdgcn_sched_barrier(0);
        if (ISSUE && !(dbg & 128)) rg.d[j] = prod_load_item<u32x4_t>(nbase, gi[j], q);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the head of an issue: the chunk's masks and its (scale, shift) loads, in front of its items
__device__ __forceinline__ void ns_issue_head(const ChunkSrc& src, unsigned ok, unsigned live, int q, NsRegs& rg) {
    rg.ok = ok;
    rg.live = live;
    rg.has_ss = src.ss != nullptr;
    if (src.ss) prod_load_ss(src.ss, q, rg.s0, rg.s1);
    __builtin_amdgcn_sched_barrier(0);   // (the items behind them, in every chunk: the waits of the interval loop count on one order)
}

// The chunk in `rg` (issued one interval ago) is committed; ISSUE: the chunk after it (source `src`, items `gi`, `iok`) takes its place
template <bool X3, bool ISSUE>
__device__ __forceinline__ void ns_roll_sw(const ConvArgs& p, NsRegs& rg, unsigned char* dst_in, const int (&off)[WS_MAXV], int q, int plane,
                                           const ChunkSrc& src, const int (&gi)[NS_ITEMS], unsigned iok, unsigned live, int dbg) {
    // this chunk's words and masks leave their registers HERE (the "+v"), in front of the loads that replace them.  hipcc waits with
    // vmcnt(0) for the copy (it counts the path on which none of the four ifs below is taken): what was issued one interval ago has
    // landed before the first item is committed, as it had before the loop rolled; the rolling overlaps the commit with the ISSUE of
    // the next chunk, which the trace of the old loop showed to cost as much as the commit (profiles/NOTES_r12.md).
    unsigned w[8] = {rg.s0.x, rg.s0.y, rg.s0.z, rg.s0.w, rg.s1.x, rg.s1.y, rg.s1.z, rg.s1.w};
    asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]));
    const unsigned ok = rg.ok;
    const bool has_ss = rg.has_ss != 0;
    // padding voxels must read as zero AFTER the transform; the four (transform, edge) combinations are separate straight-line
    // copies (see prod_commit), chosen per chunk
    const bool edge = __builtin_amdgcn_ballot_w64(rg.ok != rg.live) != 0;
    int form = __builtin_amdgcn_readfirstlane((has_ss ? 2 : 0) | (edge ? 1 : 0));
    if (ISSUE) ns_issue_head(src, iok, live, q, rg);
    union {
        unsigned u;
        h2_t v;
    } sl2;
    sl2.v = h2_t{(_Float16)p.slope, (_Float16)p.slope};
    // fp16: lane q & 1 owns k-half plane q & 1 of its voxels; split precision: hi -> plane 0, lo -> plane 1, lane q & 1 the 8-byte half
    unsigned char* d0 = X3 ? dst_in + (q & 1) * 8 : dst_in + (q & 1) * plane;
    // Four ifs in a row, not an if / else tree: hipcc chains the arms of a tree through flow blocks in which the registers one arm has
    // re-loaded stay live beside those the next arm reads -- a second register set, moved back behind a vmcnt(0) at the end of the
    // interval.  Here every arm takes the set and leaves it in place (the empty asm: or the ifs become one switch, a tree again).
    if (form == 3) ns_roll_items_sw<X3, true, true, ISSUE>(p, rg, w, ok, d0, off, plane, sl2.u, src.base, gi, q, dbg);
    asm volatile("" : "+s"(form));
    if (form == 2) ns_roll_items_sw<X3, true, false, ISSUE>(p, rg, w, ok, d0, off, plane, sl2.u, src.base, gi, q, dbg);
    asm volatile("" : "+s"(form));
    if (form == 1) ns_roll_items_sw<X3, false, true, ISSUE>(p, rg, w, ok, d0, off, plane, sl2.u, src.base, gi, q, dbg);
    asm volatile("" : "+s"(form));
    if (form == 0) ns_roll_items_sw<X3, false, false, ISSUE>(p, rg, w, ok, d0, off, plane, sl2.u, src.base, gi, q, dbg);
}

// One 16-channel chunk: acc[r] += sum over the 27 taps.  b0p: LDS address of this lane's voxel in plane 0 of the wave's
// M-tiles, this lane's k-half plane (halo extents are compile-time: every fragment read has an immediate offset); wb: the
// packed weights (wave-uniform base); vcur / vnext: this lane's byte offset of (chunk, tap 0) of this and of the following
// chunk for the wave's cout chunk (always valid: the last chunk of the last tile prefetches a dummy); gs: bytes per tap.
// The accumulators enter a tile's first chunk holding the bias.
// X3 (split-precision mode, see k_conv_ws): the chunk is 8 fp32 channels as hi / lo fp16 planes, the weight fragments come in
// hi / lo pairs (lo = `lo_off` bytes behind hi in the packed array: the part stride Cout * 16) and every (plane, dx) pair is two MFMAs.
// NR: slots of the weight ring (3 or 9: a divisor of the 9 groups, so the slot of a group does not depend on the chunk); group g + NR - 1 is
// fetched while group g is consumed.  NR = 9 for the RM = 2 instantiation: its groups are 6 MFMAs (192 cycles) long, two groups ahead
// was less than an L2 round trip (BOA_WS_TRACE: 3 900 / 2 850 cycles per chunk of 54 MFMAs).
template <int S, int RM, bool X3, int NR>
__device__ __forceinline__ void consume_chunk_x(const unsigned char* b0p, f32x16 (&acc)[RM], f16x8 (&a)[NR][3], f16x8 (&al)[X3 ? NR : 1][3],
                                                const WS_GLOBAL unsigned char* wb, unsigned vcur, unsigned vnext, unsigned gs, unsigned lo_off) {
    constexpr int NB = S * (RM - 1) + 3;
    constexpr int MM = X3 ? 2 : 1;
    f16x8 b[NB];
    auto fetch_a = [&](unsigned vchunk, int g, int slot) {  // group g = dy * 3 + dz: taps g + 9 dx
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            unsigned vo = __umul24((unsigned)(g + 9 * dx), gs) + vchunk;
            asm volatile("" : "+v"(vo));  // keep the 32 -> 64 bit extension in this block: scalar-base load form
            a[slot][dx] = *(const WS_GLOBAL f16x8*)(wb + vo);
            if constexpr (X3) {
                unsigned vl = vo + lo_off;
                asm volatile("" : "+v"(vl));
                al[slot][dx] = *(const WS_GLOBAL f16x8*)(wb + vl);
            }
        }
    };
#pragma unroll
    for (int jj = 0; jj < NB; ++jj) b[jj] = *(const f16x8*)(b0p + jj * 9 * NS_SW_ROW * 16);
    __builtin_amdgcn_sched_group_barrier(0x100, NB, 0);
#pragma unroll
    for (int g = 0; g < 9; ++g) {
        const int slot = g % NR;
        if (g + NR - 1 < 9)
            fetch_a(vcur, g + NR - 1, (g + NR - 1) % NR);
        else
            fetch_a(vnext, g + NR - 1 - 9, (g + NR - 1) % NR);
        __builtin_amdgcn_sched_group_barrier(0x020, 3 * MM, 0);
#pragma unroll
        for (int jj = 0; jj < NB; ++jj) {
            int cnt = 0;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int rr = jj - dx;
                if (rr < 0 || rr % S != 0 || rr / S >= RM) continue;
                const int r = rr / S;
                acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[slot][dx], b[jj], acc[r], 0, 0, 0);
                if constexpr (X3) acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[slot][dx], b[jj], acc[r], 0, 0, 0);
                ++cnt;
            }
            if (cnt == 1)
                __builtin_amdgcn_sched_group_barrier(0x008, 1 * MM, 0);
            else if (cnt == 2)
                __builtin_amdgcn_sched_group_barrier(0x008, 2 * MM, 0);
            else if (cnt == 3)
                __builtin_amdgcn_sched_group_barrier(0x008, 3 * MM, 0);
            if (g + 1 < 9) {
                const int gn = g + 1, dy = gn / 3, dz = gn % 3;
                b[jj] = *(const f16x8*)(b0p + ((jj * 9 + ns_sw_yp(dy)) * NS_SW_ROW + ns_sw_zp(dz)) * 16);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
        }
    }
}

// S: conv stride (all axes, 2: the SW halo layout); WN: consumer waves along the cout axis (cout group = WN chunks), 4 / WN wave rows
// along x; RM: M-tiles (x-planes of 4 x 8 output voxels) per wave.  Block tile = (4 / WN) * RM planes.
template <int S, int WN, int RM, bool X3>
__global__ __launch_bounds__(WS_THREADS) void k_conv_ns(ConvArgs p, int dbg_arg, const int* __restrict__ desc, int desc_row) {
    static_assert(S == 2, "k_conv_ns: the halo layout is the stride-2 one");
#ifdef WS_WITH_TRACE
    const int dbg = dbg_arg;
#else
    constexpr int dbg = 0;   // (ablation switches: traced build only, see k_conv_ws)
    (void)dbg_arg;
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool producer = wave >= 4;
    const int l31 = lane & 31;
    const int kh = lane >> 5;
    const int HV = p.h0 * p.h1 * p.h2;
    const int plane = ns_sw_plane_bytes();
    const int ncc = (p.C0 + p.C1) / 16;
    const int buf_bytes = 2 * plane;  // LDS: [halo buf 0][halo buf 1], each two k-octet planes
    unsigned char* bufs = smem;

    // this workgroup's row of the launch's descriptor table (k_ws_build_desc, conv_sched.hip): entry 0 = its tile count, entry 1 + k =
    // its k-th tile; each role reads one 32-byte descriptor per tile with scalar loads instead of walking the run tables
    const int* __restrict__ drow = desc + (size_t)blockIdx.x * desc_row * 8;
    const int my_tiles = drow[0];
    const int my_chunks = my_tiles * ncc;
    for (int i = tid; i < p.Cout; i += WS_THREADS) ((float*)(smem + 2 * buf_bytes))[i] = p.bias[i];  // (ordered by the first barrier)
    const int tr_blk = WS_TRACING ? (int)p.trace[WS_TRACE_SLOTS - 5] : -1;   // (debug) the traced block: BOA_WS_TRACE=<block>

    if (producer) {
        // ---- producer waves: as in k_conv_ws without the weight staging (chunk g + 1 committed while the consumers work on
        // chunk g, its global loads issued one barrier interval earlier)
        const int q = tid - 256;
        ProdConst pc = prod_const(p, q, HV);
        // SW layout: this lane's LDS byte offset of its halo voxels (kernel constants, like pc.rel)
        int ldso[WS_MAXV];
#pragma unroll
        for (int j = 0; j < WS_MAXV; ++j) {
            const int v = (q >> 1) + (WS_PROD / 2) * j;
            const int hz = v % 17, t = v / 17;
            const int hy = t % 9, hx = t / 9;
            ldso[j] = (v < HV ? (hx * 9 + ns_sw_yp(hy)) * NS_SW_ROW + ns_sw_zp(hz) : ns_sw_slots()) * 16;
        }
        TileDesc pd;   // the tile whose chunks are being issued
        pd.flags = pd.vo = pd.ibase = 0;
        TileCoord& ptc = pd.tc;
        int pk = 0;
        ptc.n = ptc.cy = ptc.ox0 = ptc.oy0 = ptc.oz0 = ptc.sp = 0;
        int gi[NS_ITEMS];   // input voxel indices of the items of the tile being issued, and the mask of those inside the input tensor
        unsigned iok = 0;
#pragma unroll
        for (int j = 0; j < NS_ITEMS; ++j) gi[j] = 0;
        // Rolling commit / issue (ns_roll_items_sw): the loads of chunk g + 2 go out item by item while chunk g + 1 is committed, each
        // into the register its item has just left.  "Commit all, then issue all" spent 2 200 cycles of a 4 700-cycle interval on the
        // commit and 1 900 on the issue of 11 loads per lane (trace of an interior workgroup, 32 -> 64 @128^3, batch 25: the memory pipe
        // takes the loads at the rate it serves them) with the memory pipe idle during the first and the LDS idle during the second.
        // A/B on one box (tools/ab_layers.sh, batch 25 / 8): 32 -> 64 @128^3 -19 / -18 %, 64 -> 128 @64^3 -8 / -11 %, 128 -> 256 @32^3
        // -12 / -7 %, 256 -> 320 @16^3 -20 / -12 %.  The second register set the RM = 4 instantiations had (loads of chunk g + 2 at the
        // head of the interval: twice the bytes in flight, +16 % on the 32 -> 64 layer) lost to this loop on every layer and is gone.
        NsRegs rg;
#pragma unroll
        for (int j = 0; j < NS_ITEMS; ++j) rg.d[j] = u32x4_t{0, 0, 0, 0};
        rg.s0 = rg.s1 = u32x4_t{0, 0, 0, 0};
        rg.ok = rg.live = 0;
        rg.has_ss = 0;
        int pcc = 0;
        int ptr_n = 0;
        // debug timeline of producer wave 4 of the traced block (second half of the trace buffer): 1 barrier passed, 8 next tile set up,
        // 2 chunk committed and the next one issued.  (The stamp is a global store: while it is pending hipcc waits with vmcnt(0) for every
        // item, so the traced build's producers run item by item at the memory latency -- its timeline shows the roles, not the rates.)
#define NS_PSTAMP(code)                                                                                                          \
    do {                                                                                                                         \
        if (WS_TRACING && (int)blockIdx.x == tr_blk && wave == 4 && lane == 0 && ptr_n < WS_TRACE_SLOTS / 2 - 8) {                                  \
            p.trace[WS_TRACE_SLOTS / 2 + ptr_n] = ((unsigned long long)(code) << 56) | (__builtin_readcyclecounter() & 0x00ffffffffffffffull); \
            ++ptr_n;                                                                                                             \
        }                                                                                                                        \
    } while (0)
        const bool live = !(dbg & 2);
        if (live && my_chunks > 0) {   // chunk 0: all of it
            pd = load_desc(drow, 0);
            iok = ns_setup_desc(p, pd, pc, gi);
            const ChunkSrc src = prod_chunk_src(p, ptc.n, 0, dbg);
            ns_issue_head(src, iok, pc.in_halo, q, rg);
#pragma unroll
            for (int j = 0; j < NS_ITEMS; ++j)
                if (!(dbg & 128)) rg.d[j] = prod_load_item<u32x4_t>(src.base, gi[j], q);
            if (++pcc == ncc) pcc = 0;
        }
        // interval g: chunk g + 1 is committed while the consumers work on chunk g, and chunk g + 2 is issued; behind the workgroup's
        // last chunk nothing is issued
        for (int g = -1; live && g + 2 < my_chunks; ++g) {
            NS_PSTAMP(1);
            if (pcc == 0) {   // descriptor + halo addresses of the next tile, before its first chunk is issued
                pd = load_desc(drow, ++pk);
                // (the general halo class unpacks pc.hc and pc.in_halo per item: hipcc hoists the ~50 unpacked words out of
                //  the interval loop and spills them unless they vary with it)
#pragma unroll
                for (int j = 0; j < WS_MAXV; ++j) asm volatile("" : "+v"(pc.hc[j]));
                asm volatile("" : "+v"(pc.in_halo));
                iok = ns_setup_desc(p, pd, pc, gi);
                NS_PSTAMP(8);
            }
            const ChunkSrc src = prod_chunk_src(p, ptc.n, pcc, dbg);
            if (++pcc == ncc) pcc = 0;
            ns_roll_sw<X3, true>(p, rg, bufs + ((g + 1) & 1) * buf_bytes, ldso, q, plane, src, gi, iok, pc.in_halo, dbg);
            NS_PSTAMP(2);
            __syncthreads();
        }
        if (live && my_chunks > 0) {
            NS_PSTAMP(1);
            ChunkSrc none;
            none.base = nullptr;
            none.ss = nullptr;
            ns_roll_sw<X3, false>(p, rg, bufs + ((my_chunks - 1) & 1) * buf_bytes, ldso, q, plane, none, gi, iok, pc.in_halo, dbg);
            NS_PSTAMP(2);
            __syncthreads();
        }
        if (!live)   // (ablation without the producers: the barriers alone)
            for (int g = -1; g + 1 < my_chunks; ++g) __syncthreads();
        __syncthreads();   // the consumers' last chunk
        return;
    }

    // ---- consumer waves --------------------------------------------------------------------------------
    if (!(dbg & 1024)) __builtin_amdgcn_s_setprio(3);
    int tr_n = 0;
    // debug timeline (BOA_WS_TRACE): consumer wave 0 of block 0; codes 1 tile start, 2 before the first chunk, 3 chunk done, 4 barrier passed
#define NS_STAMP(code)                                                                                                   \
    do {                                                                                                                 \
        if (WS_TRACING && (int)blockIdx.x == tr_blk && wave == 0 && lane == 0 && tr_n < WS_TRACE_SLOTS / 2) {                              \
            p.trace[tr_n] = ((unsigned long long)(code) << 56) | (__builtin_readcyclecounter() & 0x00ffffffffffffffull); \
            ++tr_n;                                                                                                      \
        }                                                                                                                \
    } while (0)
    const int cw = wave & 3;
    const int wn = cw % WN, wm = cw / WN;
    const int ly = l31 >> 3, lz = l31 & 7;
    const int nchunks_out = p.Cout / 32;
    // this lane's voxel in plane 0 of the wave's M-tiles, its k-half plane
    const int hoff = (((2 * (wm * RM)) * 9 + ly) * NS_SW_ROW + lz) * 16 + kh * plane;
    const int srel0 = ly * p.Wo + lz;
    const size_t out_vox = (size_t)p.Do * p.Ho * p.Wo;
    const int nslots = p.nslots;
    int slot = 0;
    // InstanceNorm partial sums in the D-fragment layout (see k_conv_ws)
    float st_s[16], st_q[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) st_s[i] = st_q[i] = 0.f;
    int st_n = -1, st_ch = 0;
    auto flush_stats = [&]() {
        if (st_n < 0) return;
#define NS_HALVE(M, HALF)                                                                                \
    {                                                                                                    \
        const bool up = (l31 & (M)) != 0;                                                                \
        _Pragma("unroll") for (int i = 0; i < (HALF); ++i) {                                             \
            const float ks = up ? st_s[i + (HALF)] : st_s[i], gs_ = up ? st_s[i] : st_s[i + (HALF)];     \
            const float kq = up ? st_q[i + (HALF)] : st_q[i], gq_ = up ? st_q[i] : st_q[i + (HALF)];     \
            st_s[i] = ks + __shfl_xor(gs_, (M));                                                         \
            st_q[i] = kq + __shfl_xor(gq_, (M));                                                         \
        }                                                                                                \
    }
        NS_HALVE(1, 8)
        NS_HALVE(2, 4)
        NS_HALVE(4, 2)
        NS_HALVE(8, 1)
#undef NS_HALVE
        st_s[0] += __shfl_xor(st_s[0], 16);
        st_q[0] += __shfl_xor(st_q[0], 16);
        if (l31 < 16) {
            const int i = ((l31 & 1) << 3) | ((l31 & 2) << 1) | ((l31 & 4) >> 1) | ((l31 & 8) >> 3);
            const int row = st_ch * 32 + 8 * (i >> 2) + 4 * kh + (i & 3);
            float* pp = p.partials + (((size_t)st_n * p.Cout + row) * 2) * nslots + slot;
            pp[0] = st_s[0];
            pp[nslots] = st_q[0];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) st_s[i] = st_q[i] = 0.f;
    };

    f32x16 acc[RM];
    auto epilogue = [&](const TileCoord& tc, int ch, int dfl, int dvo) {
        st_n = tc.n;  // (the caller flushed when the sample / cout chunk / run changed)
        st_ch = ch;
        const int cout0 = ch * 32;
        const bool full = (dfl & WS_DF_FULL) != 0;   // (block tile = 4 x 4 x 8 = b x w of conv_ns_tile: make_desc's test)
        const size_t ovox = (size_t)(unsigned)dvo;
        const size_t obase = ((size_t)tc.n * p.Cout + cout0) * out_vox + ovox * 16;
        const unsigned olane = ((unsigned)kh * (unsigned)out_vox + (unsigned)srel0) * 32u;
#pragma unroll
        for (int r = 0; r < RM; ++r) {
            const int mx = wm * RM + r;  // wave-uniform plane within the block tile
            const int mrel = mx * p.Ho * p.Wo;
            bool ok = true;
            if (!full) ok = tc.ox0 + mx < p.Do && tc.oy0 + ly < p.Ho && tc.oz0 + lz < p.Wo;
            const float dm = ok ? 1.f : 0.f;
            float v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = X3 ? acc[r][i] * p.winv : acc[r][i];
            // packed fp32 (v_pk_add_f32 / v_pk_fma_f32: two entries per instruction; same operations and order per entry)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                f2_t vm = f2_t{v[2 * i], v[2 * i + 1]};
                if (!full) vm = vm * f2_t{dm, dm};
                f2_t s2 = f2_t{st_s[2 * i], st_s[2 * i + 1]}, q2 = f2_t{st_q[2 * i], st_q[2 * i + 1]};
                s2 = s2 + vm;
                q2 = __builtin_elementwise_fma(vm, vm, q2);
                st_s[2 * i] = s2.x; st_s[2 * i + 1] = s2.y;
                st_q[2 * i] = q2.x; st_q[2 * i + 1] = q2.y;
            }
            if constexpr (X3) {   // fp32 octet planes (k_conv_ws<X3>'s store)
                if (ok && !(dbg & 4)) {
                    const size_t doff = ((size_t)tc.n * p.Cout + cout0) * out_vox * 4 + (ovox + (size_t)mrel) * 32;
                    const unsigned dlo = __builtin_amdgcn_readfirstlane((unsigned)doff), dhi = __builtin_amdgcn_readfirstlane((unsigned)(doff >> 32));
                    WS_GLOBAL unsigned char* dst = sgpr_ptr((const unsigned char*)p.out + (((size_t)dhi << 32) | dlo));
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        unsigned ol = ((unsigned)srel0 * 32u + (unsigned)kh * 16u) + (unsigned)gq * ((unsigned)out_vox * 32u);
                        asm volatile("" : "+v"(ol));
                        __builtin_nontemporal_store(f32x4_t{v[gq * 4 + 0], v[gq * 4 + 1], v[gq * 4 + 2], v[gq * 4 + 3]}, (WS_GLOBAL f32x4_t*)(dst + ol));
                    }
                }
                continue;
            }
            __builtin_amdgcn_sched_barrier(0);
            unsigned w[8];
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                float lo4[4], hi4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[pr * 4 + e]), __float_as_uint(v[(pr + 2) * 4 + e]), false, false);
                    lo4[e] = __uint_as_float(sw[0]);
                    hi4[e] = __uint_as_float(sw[1]);
                }
                w[pr * 4 + 0] = cvt_pk_h2(lo4[0], lo4[1]);
                w[pr * 4 + 1] = cvt_pk_h2(lo4[2], lo4[3]);
                w[pr * 4 + 2] = cvt_pk_h2(hi4[0], hi4[1]);
                w[pr * 4 + 3] = cvt_pk_h2(hi4[2], hi4[3]);
            }
            if (ok && !(dbg & 4)) {
                WS_GLOBAL unsigned char* dst = sgpr_ptr(p.out + (obase + (size_t)mrel * 16));
                unsigned ol = olane;
                asm volatile("" : "+v"(ol));
                // non-temporal stores: the layer's output is not read again before the launch ends, so it need not displace halo lines from
                // the XCD's L2 (A/B on one box with tools/build_alt.sh, layers repeated at the power cap: 1 780 -> 1 767, 957 -> 946,
                // 823 -> 817 us; bench step 1 820 -> 1 806 ms; the HBM-bound first conv measured 0 ... -10 % with them and keeps plain stores)
                __builtin_nontemporal_store(u32x4_t{w[0], w[1], w[2], w[3]}, (WS_GLOBAL u32x4_t*)(dst + ol));
                __builtin_nontemporal_store(u32x4_t{w[4], w[5], w[6], w[7]}, (WS_GLOBAL u32x4_t*)(dst + ol + 16));
            }
        }
    };

    // weights: wpk [(cc * 27 + tap) * 2 + kh][Cout][8 halves]; a wave's fragment of (cc, tap, cout chunk ch): lane (kh, l31)
    // reads 16 bytes at ((cc * 27 + tap) * 2 * Cout + kh * Cout + ch * 32 + l31) * 16
    const unsigned gs = 32u * (unsigned)p.Cout;  // bytes per tap
    const unsigned voff = X3 ? (unsigned)l31 * 16u : ((unsigned)kh * (unsigned)p.Cout + (unsigned)l31) * 16u;   // (X3: both k-halves read the same hi / lo fragments)
    const unsigned lo_off = (unsigned)p.Cout * 16u;
    auto woff = [&](int cc, int ch) -> unsigned { return voff + (unsigned)cc * 27u * gs + (unsigned)ch * 512u; };
    constexpr int NR = (RM == 2 && !X3) ? 9 : 3;
    f16x8 a[NR][3];
    f16x8 al[X3 ? NR : 1][3];
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                a[i][j][e] = (_Float16)0.f;
                if (X3 || i == 0) al[X3 ? i : 0][j][e] = (_Float16)0.f;
            }
    auto prime = [&](unsigned vchunk) {  // groups 0 .. NR - 2 of a chunk into their ring slots
        const WS_GLOBAL unsigned char* wb = sgpr_ptr(p.wpk);
#pragma unroll
        for (int g = 0; g < NR - 1; ++g)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                unsigned vo = __umul24((unsigned)(g + 9 * dx), gs) + vchunk;
                asm volatile("" : "+v"(vo));
                a[g][dx] = *(const WS_GLOBAL f16x8*)(wb + vo);
                if constexpr (X3) {
                    unsigned vl = vo + lo_off;
                    asm volatile("" : "+v"(vl));
                    al[g][dx] = *(const WS_GLOBAL f16x8*)(wb + vl);
                }
            }
    };

    TileDesc cd;
    cd.flags = cd.vo = cd.ibase = 0;
    cd.tc.n = cd.tc.cy = cd.tc.ox0 = cd.tc.oy0 = cd.tc.oz0 = cd.tc.sp = 0;
    bool ring_valid = false;
    TileCoord done_tc = cd.tc;
    int done_ch = 0, done_fl = 0, done_vo = 0;
    bool done_active = false;
    __syncthreads();  // chunk 0 and the bias table staged
    for (int k = 0; k < my_tiles + 1; ++k) {
        const bool more = k < my_tiles;
        bool new_run = true;
        NS_STAMP(1);
        if (more) {
            cd = load_desc(drow, k);
            new_run = (cd.flags & WS_DF_NEWRUN) != 0;
        }
        const bool have_next = k + 1 < my_tiles;
        const TileCoord& tc = cd.tc;
        const int ch = tc.cy * WN + wn;
        if (k > 0 && done_active && !(dbg & 8)) epilogue(done_tc, done_ch, done_fl, done_vo);  // deferred: the previous tile's
        // ONE flush site: the accumulated partial sums go to their slot when the next tile belongs to another virtual
        // workgroup, sample or cout chunk, and at the end
        if (k > 0 && (!more || new_run || tc.n != st_n || ch != st_ch)) {
            flush_stats();
            st_n = -1;
        }
        if (!more) break;
        if (new_run) slot = (int)((unsigned)cd.flags >> 16) * 4 + cw;
        const bool active = ch < nchunks_out;
        // the chunk the ring is prefetched for after this tile: the next tile's (clamped to a valid chunk when this wave idles there)
        // (the cout group of the tile after this one: the weight ring is prefetched across tile boundaries)
        int ch_next = have_next ? drow[(size_t)(k + 2) * 8 + 1] * WN + wn : ch;
        const bool next_active = have_next && ch_next < nchunks_out;
        if (ch_next >= nchunks_out) ch_next = nchunks_out - 1;
        if (active) {
            // the accumulators start at the bias: this lane's 16 biases of the cout chunk in the D-fragment layout (entry 4 gq + e
            // <-> cout 8 gq + 4 kh + e) from the LDS copy (no bias add in the epilogue, no bias registers across the tile)
            const float* lb = (const float*)(smem + 2 * buf_bytes) + ch * 32 + 4 * kh;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const f32x4_t bv = *(const f32x4_t*)(lb + 8 * gq);
#pragma unroll
                for (int r = 0; r < RM; ++r) {
                    acc[r][gq * 4 + 0] = X3 ? bv[0] * p.wscale : bv[0]; acc[r][gq * 4 + 1] = X3 ? bv[1] * p.wscale : bv[1];
                    acc[r][gq * 4 + 2] = X3 ? bv[2] * p.wscale : bv[2]; acc[r][gq * 4 + 3] = X3 ? bv[3] * p.wscale : bv[3];
                }
            }
            if (!ring_valid) prime(woff(0, ch));
        }
        NS_STAMP(2);
        for (int cc = 0; cc < ncc; ++cc) {
            const int g = k * ncc + cc;
            if (active) {
                const unsigned char* cur = bufs + (g & 1) * buf_bytes;
                int ho = hoff;
                asm volatile("" : "+v"(ho));
                const WS_GLOBAL unsigned char* wb = sgpr_ptr(p.wpk);
                const unsigned vcur = woff(cc, ch);
                const unsigned vnext = cc + 1 < ncc ? woff(cc + 1, ch) : woff(0, ch_next);
                consume_chunk_x<S, RM, X3, NR>(cur + ho, acc, a, al, wb, vcur, vnext, gs, lo_off);
            }
            NS_STAMP(3);
            __syncthreads();
            NS_STAMP(4);
        }
        ring_valid = active && next_active;
        done_tc.n = __builtin_amdgcn_readfirstlane(tc.n);
        done_tc.cy = __builtin_amdgcn_readfirstlane(tc.cy);
        done_tc.sp = __builtin_amdgcn_readfirstlane(tc.sp);
        done_tc.ox0 = __builtin_amdgcn_readfirstlane(tc.ox0);
        done_tc.oy0 = __builtin_amdgcn_readfirstlane(tc.oy0);
        done_tc.oz0 = __builtin_amdgcn_readfirstlane(tc.oz0);
        done_ch = __builtin_amdgcn_readfirstlane(ch);
        done_fl = __builtin_amdgcn_readfirstlane(cd.flags);
        done_vo = __builtin_amdgcn_readfirstlane(cd.vo);
        done_active = active;
    }
}

// ---- host side ---------------------------------------------------------------------------------------
// The layers k_conv_ns takes (a function of the layer geometry only): 3x3x3 kernels with stride 2 on all axes, at least two cout
// chunks and an output of at least 8^3 voxels -- measured per layer against k_conv_ws on the `total` geometry (8 tiles): 32 -> 64
// @128^3, 64 -> 128 @64^3 453 -> 194 us, 128 -> 256 @32^3 224 -> 96 us, 256 -> 320 @16^3 114 -> 81 us.  The stride-1 layers with
// Cout >= 128 run at par with k_conv_ws (the epilogue of four M-tiles per 128-voxel tile costs what the fourfold halo reuse
// gains) and the 8^3 / 4^3 layers are latency-bound either way.
bool conv_ns_applicable(const ConvGeom& g) {
    const bool k333 = g.k[0] == 3 && g.k[1] == 3 && g.k[2] == 3;
    const bool s2 = g.s[0] == 2 && g.s[1] == 2 && g.s[2] == 2;
    if (!k333 || g.Cout % 32 != 0) return false;
    return s2 && g.Cout >= 64 && g.Do >= 8 && g.Ho >= 8 && g.Wo >= 8;
}

// consumer waves along the cout axis: four when the layer has four or more cout chunks, else two (Cout = 64 / 96)
static int ns_wn(int Cout) { return Cout >= 128 ? 4 : 2; }
int conv_ns_wn(int Cout) { return ns_wn(Cout); }

void conv_ns_tile(const ConvGeom& g, ConvTile* t) {
    t->variant = 2;
    t->xs = 0;   // (its own LDS layouts; ConvArgs::xs = h1 * h2 for the shared producer constants)
    t->R = 4;
    t->w[0] = 1; t->w[1] = 4; t->w[2] = 8;
    t->b[0] = 4; t->b[1] = 1; t->b[2] = 1;
    const int ext[3] = {4, 4, 8};
    const int dims[3] = {g.Do, g.Ho, g.Wo};
    for (int d = 0; d < 3; ++d) {
        t->h[d] = (ext[d] - 1) * g.s[d] + 3;
        t->tiles[d] = (dims[d] + ext[d] - 1) / ext[d];
    }
    // two halo buffers (the de-interleaved layout, see NS_SW_ROW) + the bias table
    t->lds_bytes = 4 * (size_t)ns_sw_plane_bytes() + (size_t)g.Cout * sizeof(float);
}

int conv_ns_ncy(int Cout) { return (Cout / 32 + ns_wn(Cout) - 1) / ns_wn(Cout); }

template <int S, int WN, int RM, bool X3 = false>
static void launch_ns(boa_ctx* ctx, const ConvArgs& a, const ConvTile& t, const ConvSched& s) {
    static bool once = (hipFuncSetAttribute((const void*)k_conv_ns<S, WN, RM, X3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), true);
    (void)once;
    hipLaunchKernelGGL((k_conv_ns<S, WN, RM, X3>), dim3(s.grid), dim3(WS_THREADS), t.lds_bytes, ctx->stream, a, s.dbg, s.desc, s.desc_row);
}

int launch_conv_ns(boa_ctx* ctx, const ConvArgs& a_in, const ConvTile& t, double flops, double bytes, bool x3) {
    ConvArgs a = a_in;
    a.ncy = conv_ns_ncy(a.Cout);
    a.cy_fast = 0;
    const int total = t.tiles[0] * t.tiles[1] * t.tiles[2] * a.ncy;  // tiles of one sample
    BOA_REQUIRE(t.h[0] == 9 && t.h[1] == 9 && t.h[2] == 17 && a.h0 * a.h1 * a.h2 == NS_HV && a.xs == a.h1 * a.h2,
                "conv_ns: the producers are unrolled for the 9 x 9 x 17 halo");
    BOA_REQUIRE(a.s0 == 2, "conv_ns: instantiated for stride 2 only");
    ConvSched s;
    BOA_TRY(conv_sched_prepare(ctx, a, total, "conv_ns", &s));
    KernelTimer tm(ctx, BOA_K_CONV_MFMA, flops, bytes);
    ctx->counters[x3 ? BOA_CNT_CONV_X3 : BOA_CNT_CONV_WS]++;
    if (x3) {
        if (ns_wn(a.Cout) == 2)
            launch_ns<2, 2, 2, true>(ctx, a, t, s);
        else
            launch_ns<2, 4, 4, true>(ctx, a, t, s);
    } else if (ns_wn(a.Cout) == 2)
        launch_ns<2, 2, 2>(ctx, a, t, s);
    else
        launch_ns<2, 4, 4>(ctx, a, t, s);
    tm.stop();
    conv_sched_trace_dump(ctx, a, s, total, 0);
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}
