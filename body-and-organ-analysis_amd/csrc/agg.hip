// HBM-bound voxel aggregations of the BOA body-composition / measurement path (integer arithmetic, but for the float64 HU instantiations):
// tissue subclassification + slice-wise counts and HU sums (int16 and float64 HU), per-label HU histograms, label/HU masks.
#include <string.h>

#include <algorithm>

#include "common.h"

// ------------------------------------------------------------------------------------------------------
// BCA/tissue/subclassification.py:38-53 with the rules of BCA/tissue/definition.py:22-30 applied in enum order
// (later rules overwrite): MUSCLE(-29..150 in MUSCLE=2), BONE(-1000..3000 in BONE=5), SAT/VAT/IMAT/PAT/EAT
// (-190..-30 in SUBCUTANEOUS=1 / ABDOMINAL=3 / MUSCLE=2 / MEDIASTINUM=9 / PERICARDIUM=7).
// H: the type the bounds are compared in -- int for int16 HU; double for float64 HU, where the rules compare the float value itself
// (`image >= lo` and `image <= hi`: -29.5 is neither muscle nor adipose tissue, -190.0 is adipose).  The bounds are exact in both.
template <typename H>
__device__ __forceinline__ int tissue_of(H hu, int region) {
    const bool adip = hu >= -190 && hu <= -30;
    int t = 0;
    if (region == 2 && hu >= -29 && hu <= 150) t = 1;
    if (region == 5 && hu >= -1000 && hu <= 3000) t = 2;
    if (adip) {
        if (region == 1) t = 3;
        if (region == 3) t = 4;
        if (region == 2) t = 5;
        if (region == 9) t = 6;
        if (region == 7) t = 7;
    }
    return t;
}

// What the tissue pass needs to know about the CT's value type T (int16 HU, or float64 HU: agg_f64.hip has the other float statistics).
// Per-slice counts are exact in both; the per-slice HU sums are int64, or fp64 (wave and block reduction, then one fp64 atomic per
// block and counter).  The vector form reads VEC voxels per thread: 16-byte loads of the HU values, one `bytes` load per byte array.
template <typename T>
struct TissueTraits;
template <>
struct TissueTraits<short> {
    static constexpr int VEC = 8;
    typedef int hu_t;         // tissue_of's compared type
    typedef int acc_t;        // per-thread sum
    typedef long long sum_t;  // block and slice sum
    typedef uint2 bytes;
    // workgroups per slice: 16 (each thread reduces >= 64 voxels before the wave / block reduction and its 14 global atomics; 64
    // workgroups per slice measured 0.43 ms per 512^3 volume, 8 ... 32: 0.35 ms)
    static constexpr int MAX_GX = 16;
    static __device__ __forceinline__ void load(short* dst, const short* src) { *(uint4*)dst = *(const uint4*)src; }
    // src + o if src is there, else the registers `alt` (a select here, a branch in the double form: each is the form its kernel was
    // measured with, and the compiler allocates registers differently for the other)
    static __device__ __forceinline__ void load_or(short* dst, const short* src, size_t o, const short* alt) {
        *(uint4*)dst = src ? *(const uint4*)(src + o) : *(const uint4*)alt;
    }
    static __device__ __forceinline__ void add(sum_t* p, sum_t v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }
};
template <>
struct TissueTraits<double> {
    static constexpr int VEC = 4;
    typedef double hu_t;
    typedef double acc_t;
    typedef double sum_t;
    typedef unsigned int bytes;
    static constexpr int MAX_GX = 32;
    static __device__ __forceinline__ void load(double* dst, const double* src) {
        *(double2*)dst = *(const double2*)src;
        *(double2*)(dst + 2) = *(const double2*)(src + 2);
    }
    static __device__ __forceinline__ void load_or(double* dst, const double* src, size_t o, const double* alt) {
        if (src) {
            load(dst, src + o);
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) dst[j] = alt[j];
        }
    }
    static __device__ __forceinline__ void add(sum_t* p, sum_t v) { atomicAdd(p, v); }
};

// VEC: TissueTraits<T>::VEC, or 1 (slices or arrays that the vector loads cannot take)
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_tissue_aggregate(const T* __restrict__ ct, const T* __restrict__ ct_rules,
                                                          const unsigned char* __restrict__ regions,
                                                          const unsigned char* __restrict__ parts,
                                                          unsigned char* __restrict__ tissues, int slice_vox,
                                                          unsigned int* __restrict__ counts,
                                                          typename TissueTraits<T>::sum_t* __restrict__ sums) {
    typedef TissueTraits<T> Tr;
    typedef typename Tr::acc_t acc_t;
    typedef typename Tr::sum_t sum_t;
    typedef typename Tr::bytes bytes;
    __shared__ unsigned int s_cnt[16];
    __shared__ sum_t s_sum[16];
    const int z = blockIdx.y;
    if (threadIdx.x < 16) {
        s_cnt[threadIdx.x] = 0;
        s_sum[threadIdx.x] = 0;
    }
    __syncthreads();
    int cnt[2][8];
    acc_t sum[2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            cnt[a][t] = 0;
            sum[a][t] = 0;
        }
    const size_t base = (size_t)z * slice_vox;
    const int nvec = slice_vox / VEC;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nvec; i += gridDim.x * 256) {
        T hu[VEC] __attribute__((aligned(16)));
        T hr[VEC] __attribute__((aligned(16)));
        unsigned char rg[VEC] __attribute__((aligned(sizeof(bytes))));
        unsigned char pt[VEC] __attribute__((aligned(sizeof(bytes))));
        unsigned char ts[VEC] __attribute__((aligned(sizeof(bytes))));
        const size_t o = base + (size_t)i * VEC;
        if (VEC > 1) {
            Tr::load(hu, ct + o);
            Tr::load_or(hr, ct_rules, o, hu);
            *(bytes*)rg = *(const bytes*)(regions + o);
            if (parts) *(bytes*)pt = *(const bytes*)(parts + o);
        } else {
            hu[0] = ct[o];
            hr[0] = ct_rules ? ct_rules[o] : hu[0];
            rg[0] = regions[o];
            if (parts) pt[0] = parts[o];
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int t = tissue_of<typename Tr::hu_t>(hr[j], rg[j]);
            ts[j] = (unsigned char)t;
            const bool torso = parts && pt[j] == 1;
#pragma unroll
            for (int k = 1; k < 8; ++k) {
                const bool m = (t == k);
                cnt[0][k] += m ? 1 : 0;
                sum[0][k] += m ? (acc_t)hu[j] : (acc_t)0;
                cnt[1][k] += (m && torso) ? 1 : 0;
                sum[1][k] += (m && torso) ? (acc_t)hu[j] : (acc_t)0;
            }
        }
        if (tissues) {
            if (VEC > 1)
                *(bytes*)(tissues + o) = *(const bytes*)ts;
            else
                tissues[o] = ts[0];
        }
    }
    // wave reduce, then one LDS atomic per wave and counter, then one global atomic per block and counter
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            int c = cnt[a][k];
            sum_t s = sum[a][k];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                c += __shfl_xor(c, m);
                s += __shfl_xor(s, m);
            }
            if ((threadIdx.x & 63) == 0 && c) {
                atomicAdd(&s_cnt[a * 8 + k], (unsigned int)c);
                Tr::add(&s_sum[a * 8 + k], s);
            }
        }
    __syncthreads();
    if (threadIdx.x < 16 && s_cnt[threadIdx.x]) {
        atomicAdd(&counts[(size_t)z * 16 + threadIdx.x], s_cnt[threadIdx.x]);
        Tr::add(&sums[(size_t)z * 16 + threadIdx.x], s_sum[threadIdx.x]);
    }
}

template <typename T>
static int tissue_aggregate(boa_ctx* c, const char* what, const T* dev_ct, const T* dev_ct_rules, const uint8_t* dev_regions,
                            const uint8_t* dev_parts, uint8_t* dev_tissues_out, int Z, int Y, int X, uint32_t* dev_counts,
                            typename TissueTraits<T>::sum_t* dev_hu_sums) {
    typedef TissueTraits<T> Tr;
    constexpr int VEC = Tr::VEC;   // also the alignment of the vector form's byte arrays
    static_assert(VEC == sizeof(typename Tr::bytes), "the byte arrays are loaded VEC bytes at a time: their alignment test below is % VEC");
    BOA_REQUIRE(c && dev_ct && dev_regions && dev_counts && dev_hu_sums, "%s: NULL argument", what);
    BOA_REQUIRE(Z > 0 && Y > 0 && X > 0 && (long long)Y * X < (1ll << 30), "%s: bad dims", what);
    BOA_HIP_TRY(hipMemsetAsync(dev_counts, 0, (size_t)Z * 16 * sizeof(uint32_t), c->stream));
    BOA_HIP_TRY(hipMemsetAsync(dev_hu_sums, 0, (size_t)Z * 16 * sizeof(typename Tr::sum_t), c->stream));   // (all-zero bytes are +0.0)
    const int sv = Y * X;
    // (NULL optional arrays pass; ct_rules is read with the same 16-byte loads as ct)
    const bool vec = (sv % VEC == 0) && (((uintptr_t)dev_ct) % 16 == 0) && (((uintptr_t)dev_ct_rules) % 16 == 0) &&
                     (((uintptr_t)dev_regions) % VEC == 0) && (((uintptr_t)dev_parts) % VEC == 0) && (((uintptr_t)dev_tissues_out) % VEC == 0);
    const int nvec = vec ? sv / VEC : sv;
    const int gx = std::min(ceil_div(nvec, 256), Tr::MAX_GX);
    const double vox = (double)Z * sv;
    KernelTimer t(c, BOA_K_AGG, 0,
                  vox * (1.0 + sizeof(T) + (dev_ct_rules ? (double)sizeof(T) : 0.0) + (dev_parts ? 1 : 0) + (dev_tissues_out ? 1 : 0)));
    if (vec)
        hipLaunchKernelGGL((k_tissue_aggregate<T, VEC>), dim3(gx, Z), dim3(256), 0, c->stream, dev_ct, dev_ct_rules, dev_regions, dev_parts,
                           dev_tissues_out, sv, dev_counts, dev_hu_sums);
    else
        hipLaunchKernelGGL((k_tissue_aggregate<T, 1>), dim3(gx, Z), dim3(256), 0, c->stream, dev_ct, dev_ct_rules, dev_regions, dev_parts,
                           dev_tissues_out, sv, dev_counts, dev_hu_sums);
    t.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}

extern "C" int boa_tissue_aggregate(boa_ctx* c, const int16_t* dev_ct, const int16_t* dev_ct_rules,
                                    const uint8_t* dev_regions, const uint8_t* dev_parts, uint8_t* dev_tissues_out, int Z, int Y, int X,
                                    uint32_t* dev_counts, int64_t* dev_hu_sums) {
    return tissue_aggregate<short>(c, "boa_tissue_aggregate", dev_ct, dev_ct_rules, dev_regions, dev_parts, dev_tissues_out, Z, Y, X, dev_counts,
                                   (long long*)dev_hu_sums);
}

extern "C" int boa_tissue_aggregate_f64(boa_ctx* c, const double* dev_ct, const double* dev_ct_rules, const uint8_t* dev_regions,
                                        const uint8_t* dev_parts, uint8_t* dev_tissues_out, int Z, int Y, int X, uint32_t* dev_counts,
                                        double* dev_hu_sums) {
    return tissue_aggregate<double>(c, "boa_tissue_aggregate_f64", dev_ct, dev_ct_rules, dev_regions, dev_parts, dev_tissues_out, Z, Y, X,
                                    dev_counts, dev_hu_sums);
}

// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_slice_presence(const unsigned char* __restrict__ labels, int slice_vox,
                                                        unsigned char* __restrict__ present) {
    __shared__ unsigned int flags[256];
    const int z = blockIdx.y;
    flags[threadIdx.x] = 0;
    __syncthreads();
    const unsigned char* p = labels + (size_t)z * slice_vox;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < slice_vox; i += gridDim.x * 256) flags[p[i]] = 1;
    __syncthreads();
    if (flags[threadIdx.x]) present[(size_t)z * 256 + threadIdx.x] = 1;
}

extern "C" int boa_slice_label_presence(boa_ctx* c, const uint8_t* dev_labels, int Z, int Y, int X,
                                        uint8_t* dev_present) {
    BOA_REQUIRE(c && dev_labels && dev_present && Z > 0 && Y > 0 && X > 0, "boa_slice_label_presence: bad argument");
    BOA_HIP_TRY(hipMemsetAsync(dev_present, 0, (size_t)Z * 256, c->stream));
    const int sv = Y * X;
    int gx = std::min(ceil_div(sv, 256 * 8), 32);
    KernelTimer t(c, BOA_K_AGG, 0, (double)Z * sv);
    hipLaunchKernelGGL(k_slice_presence, dim3(gx, Z), dim3(256), 0, c->stream, dev_labels, sv, dev_present);
    t.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}

// ------------------------------------------------------------------------------------------------------
// tissue projections: the reductions behind the report's coronal / sagittal tissue heat maps
// (BCA/report/plots/heatmaps.py:29-101): per selected tissue `tissue_mask.sum(axis=1)` and `.sum(axis=2)` of the (z,y,x)
// tissue volume, and `((regions > 0) & (regions < 255)).any(axis)` for the body silhouette -- 2 B per voxel in one pass
// (7 tissues x 2 axes = 14 full-volume numpy passes in the reference).  One block per z slice; a thread owns its x
// columns (coronal counts need no atomics), the sagittal row counts are wave ballots + one LDS add per wave and tissue.
struct ProjArgs {
    const unsigned char* tissues;
    const unsigned char* regions;
    int Y, X, T;
    unsigned int* cor;       // [T][Z][X]
    unsigned int* sag;       // [T][Z][Y]
    unsigned char* mcor;     // [Z][X]
    unsigned char* msag;     // [Z][Y]
    int Z;
    unsigned char lut[256];  // tissue value -> index in [0, T) or 255
};

__global__ __launch_bounds__(256) void k_tissue_projections(ProjArgs a) {
    extern __shared__ unsigned int sm[];
    unsigned int* s_cor = sm;                               // [T][X]
    unsigned int* s_sag = sm + (size_t)a.T * a.X;           // [T][Y]
    unsigned int* s_mc = s_sag + (size_t)a.T * a.Y;         // [X]
    unsigned int* s_ms = s_mc + a.X;                        // [Y]
    const int z = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int tot = a.T * (a.X + a.Y) + a.X + a.Y;
    for (int i = tid; i < tot; i += 256) sm[i] = 0;
    __syncthreads();
    const size_t base = (size_t)z * a.Y * a.X;
    const int xr = (a.X + 255) / 256 * 256;  // whole waves so that the ballots see every lane
    for (int y = 0; y < a.Y; ++y) {
        const unsigned char* trow = a.tissues + base + (size_t)y * a.X;
        const unsigned char* rrow = a.regions + base + (size_t)y * a.X;
        for (int x = tid; x < xr; x += 256) {
            int idx = 255;
            bool body = false;
            if (x < a.X) {
                idx = a.lut[trow[x]];
                const unsigned char r = rrow[x];
                body = r > 0 && r < 255;
                if (idx < a.T) s_cor[idx * a.X + x] += 1;   // this thread is the only writer of column x
                if (body) s_mc[x] = 1;
            }
            for (int t = 0; t < a.T; ++t) {
                const unsigned long long m = __builtin_amdgcn_ballot_w64(idx == t);
                if (m && lane == 0) atomicAdd(&s_sag[t * a.Y + y], (unsigned)__builtin_popcountll(m));
            }
            if (__builtin_amdgcn_ballot_w64(body) && lane == 0) s_ms[y] = 1;
        }
    }
    __syncthreads();
    for (int i = tid; i < a.T * a.X; i += 256) a.cor[((size_t)(i / a.X) * a.Z + z) * a.X + i % a.X] = s_cor[i];
    for (int i = tid; i < a.T * a.Y; i += 256) a.sag[((size_t)(i / a.Y) * a.Z + z) * a.Y + i % a.Y] = s_sag[i];
    for (int i = tid; i < a.X; i += 256) a.mcor[(size_t)z * a.X + i] = (unsigned char)s_mc[i];
    for (int i = tid; i < a.Y; i += 256) a.msag[(size_t)z * a.Y + i] = (unsigned char)s_ms[i];
}

extern "C" int boa_tissue_projections(boa_ctx* c, const uint8_t* dev_tissues, const uint8_t* dev_regions, int Z, int Y, int X,
                                      const uint8_t* host_values, int n_values, uint32_t* dev_coronal, uint32_t* dev_sagittal,
                                      uint8_t* dev_mask_coronal, uint8_t* dev_mask_sagittal) {
    BOA_REQUIRE(c && dev_tissues && dev_regions && host_values && dev_coronal && dev_sagittal && dev_mask_coronal &&
                    dev_mask_sagittal && Z > 0 && Y > 0 && X > 0,
                "boa_tissue_projections: bad argument");
    BOA_REQUIRE(n_values >= 1 && n_values <= 16, "boa_tissue_projections: %d tissue values (1..16)", n_values);
    const size_t lds = ((size_t)n_values * (X + Y) + X + Y) * 4;
    BOA_REQUIRE(lds <= 160 * 1024, "boa_tissue_projections: slice %dx%d with %d tissues needs %zu bytes of LDS", Y, X, n_values, lds);
    ProjArgs a;
    a.tissues = dev_tissues; a.regions = dev_regions; a.Y = Y; a.X = X; a.T = n_values; a.Z = Z;
    a.cor = dev_coronal; a.sag = dev_sagittal; a.mcor = dev_mask_coronal; a.msag = dev_mask_sagittal;
    for (int i = 0; i < 256; ++i) a.lut[i] = 255;
    for (int t = 0; t < n_values; ++t) a.lut[host_values[t]] = (unsigned char)t;
    static bool once = (hipFuncSetAttribute((const void*)k_tissue_projections, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), true);
    (void)once;
    KernelTimer t(c, BOA_K_AGG, 0, 2.0 * Z * Y * X);
    hipLaunchKernelGGL(k_tissue_projections, dim3(Z), dim3(256), lds, c->stream, a);
    t.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}

// ------------------------------------------------------------------------------------------------------
// per-label HU histogram (label 0 = background is never measured by the reference and is skipped)
// Per-label HU histogram with a workgroup-private HASH TABLE in LDS.  Per-voxel global atomics are hopeless here: a CT's
// histogram is concentrated (a label's voxels fall into ~100 neighbouring HU bins, a handful of cache lines), and
// device-scope atomics from the 8 XCDs on the same lines are serialised on the memory side (57 ms per pass at 512^3,
// however the voxels are batched).  Each workgroup counts its voxels into an open-addressing table keyed by
// (label, bin) -- HIST_TAB entries of {key, count} in LDS, linear probing, claimed with an LDS compare-and-swap -- whatever
// the mix of labels (compact organs or the salt-and-pepper output of a random-weight net), and adds the table to the
// global one when it fills up and at the end: one global atomic per DISTINCT key of ~10^5 voxels instead of one per
// voxel.  A wave whose 1 024 voxels all carry the same key (air around the patient) issues one LDS atomic, or none when
// the key is "not measured".
// Table size: 2^LOG2 entries of {key, count}.  LOG2 = 14 (128 KiB) leaves ONE workgroup (4 waves) per CU -- the voxel loads of an
// iteration are then a chain of exposed HBM round trips; LOG2 = 12 (32 KiB) lets four workgroups share a CU and still holds the
// distinct (label, HU) keys of a contiguous voxel range of compact organs between flushes; LOG2 = 13 (two workgroups) is the default.
#define HIST_EMPTY 0xFFFFFFFFu

// HT: threads per workgroup.  What bounds the pass on compact organs is the FLUSH: every workgroup sends each distinct (label, HU) key of
// its voxel range to the global table with one device-scope atomic, and those serialise in the fabric (the reason for the LDS tables in the
// first place) -- 2 048 workgroups of 256 threads re-send the same ~1 000 keys 2 048 times.  1 024-thread workgroups cover 4x the voxels
// per table at the same waves per CU: a quarter of the workgroups, a little more than a quarter of the atomics.
template <int LOG2, int HT>
__global__ __launch_bounds__(HT) void k_label_hist(const short* __restrict__ ct, const unsigned char* __restrict__ labels,
                                                    const unsigned char* __restrict__ mask, size_t n_all, size_t head, int hu_min,
                                                    int nbins, unsigned int* __restrict__ hist, size_t groups_per_block) {
    constexpr int HIST_TAB = 1 << LOG2;
    constexpr int HIST_FLUSH = HIST_TAB * 2 / 3;     // distinct keys in the table that trigger a flush (load factor 2/3)
    extern __shared__ __attribute__((aligned(16))) unsigned char hist_smem[];
    unsigned int* keys = (unsigned int*)hist_smem;   // [HIST_TAB]
    unsigned int* cnts = keys + HIST_TAB;            // [HIST_TAB]
    __shared__ int nkeys;
    const int tid = threadIdx.x;
    for (int i = tid; i < HIST_TAB; i += HT) {
        keys[i] = HIST_EMPTY;
        cnts[i] = 0u;
    }
    if (tid == 0) nkeys = 0;
    __syncthreads();
    // voxels [0, head) and the last (n - head) % 16 are handled one by one (unaligned views: z-slabs of a volume)
    const unsigned char* labels0 = labels;
    const short* ct0 = ct;
    const unsigned char* mask0 = mask;
    labels += head;
    ct += head;
    if (mask) mask += head;
    const size_t n = n_all - head;
    const size_t n16 = n / 16;
    auto bin_of = [&](int hu) {
        int b = hu - hu_min;
        return b < 0 ? 0 : (b >= nbins ? nbins - 1 : b);
    };
    auto count = [&](unsigned key, unsigned c) {  // key = label << 16 | bin  (nbins <= 65536)
        unsigned h = (key * 2654435761u) >> (32 - LOG2);
#pragma unroll 1
        for (int probe = 0; probe < 16; ++probe, h = (h + 1) & (HIST_TAB - 1)) {
            unsigned k = keys[h];
            if (k == HIST_EMPTY) {
                k = atomicCAS(&keys[h], HIST_EMPTY, key);
                if (k == HIST_EMPTY) {
                    atomicAdd(&nkeys, 1);
                    k = key;
                }
            }
            if (k == key) {
                atomicAdd(&cnts[h], c);
                return;
            }
        }
        atomicAdd(&hist[(size_t)(key >> 16) * nbins + (key & 0xFFFFu)], c);   // a long probe chain: straight to the global table
    };
    auto flush = [&]() {  // whole workgroup
        for (int i = tid; i < HIST_TAB; i += HT) {
            const unsigned k = keys[i];
            if (k != HIST_EMPTY) {
                atomicAdd(&hist[(size_t)(k >> 16) * nbins + (k & 0xFFFFu)], cnts[i]);
                keys[i] = HIST_EMPTY;
                cnts[i] = 0u;
            }
        }
        __syncthreads();
        if (tid == 0) nkeys = 0;
        __syncthreads();
    };
    const size_t g_begin = (size_t)blockIdx.x * groups_per_block * HT;   // groups of 16 voxels, HT per iteration
    // the next iteration's 64 bytes per lane are fetched BEFORE this iteration's table work (round 6): with 32 - 128 KiB of LDS per
    // workgroup only 1 - 4 workgroups fit a CU, and a loop of load -> wait -> LDS work -> barrier left HBM idle most of the time
    union LabV {
        uint4 u;
        unsigned char b[16];
    };
    union HuV {
        uint4 u[2];
        short h[16];
    };
    LabV nlb, nmb;
    HuV nhb;
    nlb.u = nmb.u = nhb.u[0] = nhb.u[1] = make_uint4(0, 0, 0, 0);
    auto fetch = [&](size_t it) {
        const size_t g = g_begin + it * HT + tid;
        if (it < groups_per_block && g < n16) {
            nlb.u = *(const uint4*)(labels + g * 16);
            nhb.u[0] = *(const uint4*)(ct + g * 16);
            nhb.u[1] = *(const uint4*)(ct + g * 16 + 8);
            if (mask) nmb.u = *(const uint4*)(mask + g * 16);
        }
    };
    fetch(0);
    for (size_t it = 0; it < groups_per_block; ++it) {
        const size_t g = g_begin + it * HT + tid;
        const bool live = g < n16;
        unsigned key[16];   // 0 = not measured (label 0 / masked out)
        const LabV lb = nlb, mb = nmb;
        const HuV hb = nhb;
        fetch(it + 1);
        if (live) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const unsigned l = (mask && !mb.b[i]) ? 0u : lb.b[i];
                key[i] = l ? ((l << 16) | (unsigned)bin_of(hb.h[i])) : 0u;   // label >= 1: never 0
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) key[i] = 0u;
        }
        // whole wave on one key: one atomic (or none)
        bool uni = true;
#pragma unroll
        for (int i = 1; i < 16; ++i) uni = uni && key[i] == key[0];
        const unsigned k0 = __builtin_amdgcn_readfirstlane(key[0]);
        const bool same = live ? (uni && key[0] == k0) : true;
        if (__builtin_amdgcn_ballot_w64(!same) == 0) {
            const unsigned c = 16u * (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(live));
            if (k0 != 0u && (tid & 63) == 0 && c) count(k0, c);
        } else if (live) {
            // Round 6: the 16 voxels of a lane are looked up TOGETHER.  In the steady state a key already sits in its home slot (a slot
            // keeps its key until the next flush, and flushes are behind the workgroup barrier): 16 independent ds_read_b32 of the home
            // slots, then one return-less ds_add_u32 per hit -- throughput instead of 16 dependent LDS round trips with a probe loop
            // each.  Misses (first occurrence of a key, displaced keys) take the probing insert.  Runs of equal keys are merged first
            // (CT noise makes them rare inside an organ, but label 0 / masked voxels form long runs of key 0, which cost nothing).
            unsigned hh[16], kk[16], cc[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                hh[i] = (key[i] * 2654435761u) >> (32 - LOG2);
                cc[i] = 1u;
            }
#pragma unroll
            for (int i = 15; i > 0; --i) {   // fold a voxel into its left neighbour when the keys agree (counts flow to the run's first voxel)
                const bool eq = key[i] == key[i - 1];
                cc[i - 1] += eq ? cc[i] : 0u;
                cc[i] = eq ? 0u : cc[i];
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) kk[i] = keys[hh[i]];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (key[i] != 0u && cc[i] != 0u) {
                    if (kk[i] == key[i])
                        atomicAdd(&cnts[hh[i]], cc[i]);
                    else
                        count(key[i], cc[i]);
                }
            }
        }
        // The flush decision must be the same in all 16 waves: flush() holds barriers and empties slots.  The first barrier ends
        // this iteration's inserts, so every thread latches the same nkeys; the second keeps the next iteration's inserts (which
        // increment nkeys) behind the last of those reads.  Without it a wave that read nkeys <= HIST_FLUSH could insert a new key
        // before a slower wave's read, which then saw nkeys > HIST_FLUSH and flushed alone.
        __syncthreads();
        const bool full = nkeys > HIST_FLUSH;
        __syncthreads();
        if (full) flush();
    }
    // tail (n % 16 voxels) and head, one by one straight into the global table
    if (blockIdx.x == 0) {
        if (tid < (int)(n - n16 * 16)) {
            const size_t i = n16 * 16 + tid;
            const int l = (mask && !mask[i]) ? 0 : labels[i];
            if (l) atomicAdd(&hist[(size_t)l * nbins + bin_of(ct[i])], 1u);
        }
        if (tid < (int)head) {
            const int l = (mask0 && !mask0[tid]) ? 0 : labels0[tid];
            if (l) atomicAdd(&hist[(size_t)l * nbins + bin_of(ct0[tid])], 1u);
        }
    }
    __syncthreads();
    flush();
}

__global__ __launch_bounds__(256) void k_label_hist_scalar(const short* __restrict__ ct, const unsigned char* __restrict__ labels,
                                                           const unsigned char* __restrict__ mask, size_t n, int hu_min, int nbins,
                                                           unsigned int* __restrict__ hist) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i < n; i += stride) {
        const int l = labels[i];
        if (l == 0 || (mask && !mask[i])) continue;
        int b = (int)ct[i] - hu_min;
        b = b < 0 ? 0 : (b >= nbins ? nbins - 1 : b);
        atomicAdd(&hist[(size_t)l * nbins + b], 1u);
    }
}

extern "C" int boa_label_hu_histogram(boa_ctx* c, const int16_t* dev_ct, const uint8_t* dev_labels,
                                      const uint8_t* dev_mask, size_t n, int hu_min, int nbins, uint32_t* dev_hist) {
    BOA_REQUIRE(c && dev_ct && dev_labels && dev_hist && nbins > 0 && nbins <= 65536, "boa_label_hu_histogram: bad argument");
    BOA_HIP_TRY(hipMemsetAsync(dev_hist, 0, (size_t)256 * nbins * sizeof(uint32_t), c->stream));
    if (n == 0) return BOA_OK;
    // 16-byte vector loads need the three arrays aligned at the same voxel: skip `head` voxels (views into a volume start
    // anywhere); arrays that cannot be aligned together are processed one voxel at a time
    size_t head = (size_t)((16 - ((uintptr_t)dev_labels & 15)) & 15);
    if (head > n) head = n;
    const bool together = (((uintptr_t)dev_ct + 2 * head) & 15) == 0 && (!dev_mask || (((uintptr_t)dev_mask + head) & 15) == 0);
    // contiguous voxel ranges per workgroup (few labels each): ~4 workgroups per CU, at least one 4 096-voxel iteration
    // table size / workgroups per CU, kernel time in us (round 5, 512^3):   structured phantom | bench labels (noise-like)
    //   2^14, 4:  845 | 947      2^13, 8:  679 | 1 124      2^12, 8:  571 | 1 905      2^12, 16:  650 | 2 056
    // compact organs want occupancy, salt-and-pepper labels a table that merges more duplicates before it spills: 2^13 is the default
    // round 6 (profiles/r06_hist_sweep.txt; kernel us on the structured phantom | on salt-and-pepper labels, 512^3):
    //   2^13 x 256 threads x 8 per CU (round 5)  638 | 2 937      2^13 x 1 024 x 2   486 | 2 600      2^12 x 1 024 x 2   547 | 2 650
    //   2^14 x 1 024 x 1  420 | 2 106  <- kept: ONE 1 024-thread workgroup per CU with the largest table = the fewest flush atomics
    constexpr int LOG2 = 14, HT = 1024;   // (the 128 KiB table leaves room for one workgroup per CU)
    const size_t iters = ((n - head) / 16 + HT - 1) / HT;
    const size_t gpb = std::max<size_t>(1, (iters + (size_t)c->cu_count - 1) / (size_t)c->cu_count);
    const int grid = (int)std::max<size_t>(1, (iters + gpb - 1) / gpb);
    KernelTimer t(c, BOA_K_AGG, 0, (double)n * (3.0 + (dev_mask ? 1 : 0)));
    if (together) {
        static bool once = (hipFuncSetAttribute((const void*)k_label_hist<LOG2, HT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024), true);
        (void)once;
        hipLaunchKernelGGL((k_label_hist<LOG2, HT>), dim3(grid), dim3(HT), (size_t)8 << LOG2, c->stream, dev_ct, dev_labels, dev_mask, n, head,
                           hu_min, nbins, dev_hist, gpb);
    } else {
        hipLaunchKernelGGL(k_label_hist_scalar, dim3((unsigned)std::min<size_t>((n + 255) / 256, (size_t)c->cu_count * 32)), dim3(256), 0,
                           c->stream, dev_ct, dev_labels, dev_mask, n, hu_min, nbins, dev_hist);
    }
    t.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}

// ------------------------------------------------------------------------------------------------------
struct Lut256 {
    unsigned char v[256];
};

// T: the CT's value type, B: the type the window is compared in (int16 HU as int; float64 HU as double, i.e. numpy's `ct >= lo` /
// `ct < lo` on the float value itself, no rounding to integer HU)
template <typename T, typename B>
__global__ __launch_bounds__(256) void k_label_hu_mask(const T* __restrict__ ct, const unsigned char* __restrict__ labels,
                                                       Lut256 lut, int mode, B lo, B hi, size_t n,
                                                       unsigned char* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i < n; i += stride) {
        bool m = lut.v[labels[i]] != 0;
        if (mode != 0) {
            const B hu = ct[i];
            const bool inside = hu >= lo && hu <= hi;
            m = m && (mode == 1 ? inside : !inside);
        }
        out[i] = m ? 1 : 0;
    }
}

template <typename T, typename B>
static int label_hu_mask(boa_ctx* c, const char* what, const T* dev_ct, const uint8_t* dev_labels, const uint8_t* host_lut, int mode, B hu_lo,
                         B hu_hi, size_t n, uint8_t* dev_mask_out) {
    BOA_REQUIRE(c && dev_labels && host_lut && dev_mask_out && (mode == 0 || dev_ct), "%s: bad argument", what);
    BOA_REQUIRE(mode >= 0 && mode <= 2, "%s: mode %d", what, mode);
    if (n == 0) return BOA_OK;
    Lut256 lut;
    memcpy(lut.v, host_lut, 256);
    int grid = (int)std::min<size_t>((n + 255) / 256, (size_t)c->cu_count * 32);
    KernelTimer t(c, BOA_K_AGG, 0, (double)n * (2.0 + sizeof(T)));
    hipLaunchKernelGGL((k_label_hu_mask<T, B>), dim3(grid), dim3(256), 0, c->stream, dev_ct, dev_labels, lut, mode, hu_lo, hu_hi,
                       n, dev_mask_out);
    t.stop();
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}

extern "C" int boa_label_hu_mask(boa_ctx* c, const int16_t* dev_ct, const uint8_t* dev_labels, const uint8_t* host_lut,
                                 int mode, int hu_lo, int hu_hi, size_t n, uint8_t* dev_mask_out) {
    return label_hu_mask<short, int>(c, "boa_label_hu_mask", dev_ct, dev_labels, host_lut, mode, hu_lo, hu_hi, n, dev_mask_out);
}

extern "C" int boa_label_hu_mask_f64(boa_ctx* c, const double* dev_ct, const uint8_t* dev_labels, const uint8_t* host_lut,
                                     int mode, double hu_lo, double hu_hi, size_t n, uint8_t* dev_mask_out) {
    return label_hu_mask<double, double>(c, "boa_label_hu_mask_f64", dev_ct, dev_labels, host_lut, mode, hu_lo, hu_hi, n, dev_mask_out);
}

__global__ __launch_bounds__(256) void k_label_select(const unsigned char* __restrict__ labels, size_t n, int mode,
                                                      int a, int b, int cc, unsigned char* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i < n; i += stride) {
        const int l = labels[i];
        bool m;
        if (mode == 0)
            m = l == a;
        else if (mode == 1)
            m = l > 0;
        else
            m = (l == a) || (l == b) || (l == cc);
        out[i] = m ? 1 : 0;
    }
}

extern "C" int boa_label_select(boa_ctx* c, const uint8_t* dev_labels, size_t n, int mode, const int vals[3],
                                uint8_t* dev_mask_out) {
    BOA_REQUIRE(c && dev_labels && dev_mask_out && mode >= 0 && mode <= 2, "boa_label_select: bad argument");
    BOA_REQUIRE(mode == 1 || vals, "boa_label_select: vals is NULL");
    if (n == 0) return BOA_OK;
    int grid = (int)std::min<size_t>((n + 255) / 256, (size_t)c->cu_count * 32);
    hipLaunchKernelGGL(k_label_select, dim3(grid), dim3(256), 0, c->stream, dev_labels, n, mode, vals ? vals[0] : 0,
                       vals ? vals[1] : 0, vals ? vals[2] : 0, dev_mask_out);
    BOA_HIP_TRY(hipGetLastError());
    return BOA_OK;
}
