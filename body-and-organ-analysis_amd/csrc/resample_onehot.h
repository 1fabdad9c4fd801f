// nnU-Net's one-hot label resampling (TS/resample_nnunet.py:11-33 `resize_segmentation`, order 1; per slice with nearest along
// the coarse axis in the separate-z form, :119-205) at ONE output voxel.  Plain C++: k_onehot_tables / k_resample_onehot
// (resample_onehot.hip) call these functions, tools/onehot_host.cpp calls them on the host under the sanitizers.
//
// The reference turns every label c into a 0/1 mask, resizes the mask with order 1 in fp64 and writes c wherever the result is
// >= 0.5, labels ascending, later ones overwriting.  An output voxel has at most 2 x 2 x 2 source taps, so at most 8 labels can
// have a non-zero resized mask there; for each of them the resized value is the sum, in tap order, of the tap weights
// 1.0 * w_a * w_b * w_c of the taps that hold it (the others add +0.0).  The result is the LARGEST label whose sum is >= 0.5,
// 0 when there is none.  The sums are formed on the same fp64 values in the same order as scipy forms them: exact ties at 0.5
// (every output voxel of an integer zoom factor) decide as they do there.
//
// Axis numbering here is the MEMORY order of the volume, [d0][d1][d2] with d2 fastest -- (x, y, z) on the model grid.  The
// reference resamples the transposed array [z, x, y] (TS/resampling.py:105-125), so its first axis is memory axis 2: taps are
// visited with axis 2 outermost, then 0, then 1, and the weight product is (w2 * w0) * w1.
#pragma once
#include <math.h>
#include <stdint.h>

#if !defined(BOA_HD)
#if defined(__HIPCC__)
#define BOA_HD __host__ __device__ __forceinline__
#else
#define BOA_HD inline
#endif
#endif

// one output index of one axis: the two source indices (clamped to the image) and their fp64 weights
struct OnehotTap {
    int i0, i1;
    double w0, w1;
};

BOA_HD int onehot_clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// Output index k of an axis of n_in -> n_out voxels.
//   active:  cc = (k + 0.5) * (n_in / n_out) - 0.5, fl = floor(cc), x = cc - fl; taps fl, fl + 1 clamped, weights (1 - x, x)
//            (scipy.ndimage.zoom(order=1, mode="nearest", grid_mode=True): the coordinate is NOT clamped, the indices are)
//   the separate-z axis: one source slice, floor(cc + 0.5) clamped (map_coordinates(order=0, mode="nearest")), the identity when
//            the extent does not change; weights (1.0, 0.0) -- multiplying by 1.0 and adding 0.0 are exact, so the 8-tap sum
//            below is bit for bit the 4-tap sum of the slice
// `zf` is onehot_zoom_factor(n_in, n_out): one IEEE division per axis, made once.
BOA_HD double onehot_zoom_factor(int n_in, int n_out) { return (double)n_in / (double)n_out; }

BOA_HD OnehotTap onehot_axis_tap(int k, double zf, int n_in, int n_out, bool active) {
    OnehotTap t;
    const double cc = ((double)k + 0.5) * zf - 0.5;
    if (active) {
        const double fl = floor(cc);
        const double x = cc - fl;
        t.i0 = onehot_clampi((int)fl, n_in);
        t.i1 = onehot_clampi((int)fl + 1, n_in);
        t.w0 = 1.0 - x;
        t.w1 = x;
    } else {
        t.i0 = t.i1 = n_in == n_out ? k : onehot_clampi((int)floor(cc + 0.5), n_in);
        t.w0 = 1.0;
        t.w1 = 0.0;
    }
    return t;
}

// The 8 tap weights in the reference's visiting order (memory axis 2 outermost, then 0, then 1): w[4 * r + 2 * p + q] belongs to
// the tap (axis 0: p, axis 1: q, axis 2: r).
BOA_HD void onehot_weights(const OnehotTap& t0, const OnehotTap& t1, const OnehotTap& t2, double w[8]) {
    for (int r = 0; r < 2; ++r)
        for (int p = 0; p < 2; ++p)
            for (int q = 0; q < 2; ++q) w[4 * r + 2 * p + q] = 1.0 * (r ? t2.w1 : t2.w0) * (p ? t0.w1 : t0.w0) * (q ? t1.w1 : t1.w0);
}

// The label of the voxel from its 8 tap labels and weights (same order).  One round per DISTINCT label (the label of the lowest
// tap not yet accounted for): its sum runs over all 8 taps in order, adding the weight where the label matches and +0.0 elsewhere,
// as the resize of its mask does.  A boundary voxel of two structures costs two rounds, white noise eight.  (No early exit on a
// sum above 0.5: the 8 weights add up to 1 only up to rounding, so a second label may still reach 0.5.)
BOA_HD uint8_t onehot_decide(const uint8_t l[8], const double w[8]) {
    uint64_t packed = 0;
    for (int u = 0; u < 8; ++u) packed |= (uint64_t)l[u] << (8 * u);
    unsigned rem = 0xffu, best = 0;
    while (rem) {
        const unsigned c = (unsigned)(packed >> (8 * __builtin_ctz(rem))) & 0xffu;
        unsigned m = 0;
        for (int u = 0; u < 8; ++u) m |= (unsigned)(l[u] == c) << u;
        if (c > best) {             // (background, and a label below one that already won, cannot change the result: no sum)
            double s = 0.0;
            for (int u = 0; u < 8; ++u) s += (m >> u & 1u) ? w[u] : 0.0;
            if (s >= 0.5) best = c;
        }
        rem &= ~m;
    }
    return (uint8_t)best;
}

// The four source rows (along axis 2) an output row (o0, o1) reads: row[2 * p + q] is the row of taps (axis 0: p, axis 1: q).
BOA_HD void onehot_rows(const uint8_t* in, int I1, int I2, const OnehotTap& t0, const OnehotTap& t1, const uint8_t* row[4]) {
    for (int p = 0; p < 2; ++p)
        for (int q = 0; q < 2; ++q)
            row[2 * p + q] = in + ((size_t)(p ? t0.i1 : t0.i0) * (size_t)I1 + (size_t)(q ? t1.i1 : t1.i0)) * (size_t)I2;
}

// One output voxel from its four source rows and the three axis entries.
BOA_HD uint8_t onehot_voxel(const uint8_t* const row[4], const OnehotTap& t0, const OnehotTap& t1, const OnehotTap& t2) {
    uint8_t l[8];
    double w[8];
    for (int pq = 0; pq < 4; ++pq) {
        l[pq] = row[pq][t2.i0];
        l[4 + pq] = row[pq][t2.i1];
    }
    bool same = true;
    for (int t = 1; t < 8; ++t) same = same && l[t] == l[0];
    if (same) return l[0];          // one label: its mask is 1 at every tap, the sum of the 8 weights is 1 up to a few ulp
    onehot_weights(t0, t1, t2, w);
    return onehot_decide(l, w);
}
