// resampling_fn_probabilities (order 1, order_z 0) of the fp16 logits at ONE output voxel: the device functions shared by
// k_resize_logits_argmax (resample.hip) and the class-probability pass (prob.hip), so that both see the same fp16-rounded values.
#pragma once
#include "common.h"

// nearest source index along the slice axis: scipy map_coordinates(order=0, mode="nearest") at scale * (o + 0.5) - 0.5
__device__ __forceinline__ int nearest_src(int o, double scale, int n_in) {
    const double cc = scale * ((double)o + 0.5) - 0.5;
    return min(max((int)floor(cc + 0.5), 0), n_in - 1);
}

// double -> half with ONE rounding (numpy's npy_double_to_half): to float with round-to-odd, then RTNE to half
__device__ __forceinline__ unsigned short d2h_rn(double d) {
    float f = __double2float_rz(d);
    if ((double)f != d) f = __uint_as_float(__float_as_uint(f) | 1u);
    return f2us(f);
}

// the box of the logits grid that is resampled, and the grid it is resampled to
struct LogitsResizeGeom {
    const unsigned short* logits;  // fp16 [C][L0][L1][L2]
    int C, L[3], off[3], I[3], O[3];  // full grid, crop origin, crop dims (= resampled shape), output dims
    int act[3];
    double zf[3];
};

// the (up to) 2 x 2 x 2 taps of output voxel o
struct LogitsTaps {
    double w[3][2];
    int i0[3], i1[3], nt[3];
};

__device__ __forceinline__ void logits_taps(const LogitsResizeGeom& a, const int o[3], LogitsTaps& t) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (a.act[d]) {
            const double cc = ((double)o[d] + 0.5) * a.zf[d] - 0.5;  // not clamped: the tap INDICES are (mode "nearest")
            const double fl = floor(cc);
            const double x = cc - fl;
            t.w[d][0] = 1.0 - x;
            t.w[d][1] = x;
            t.i0[d] = min(max((int)fl, 0), a.I[d] - 1);
            t.i1[d] = min(max((int)fl + 1, 0), a.I[d] - 1);
            t.nt[d] = 2;
        } else {
            t.i0[d] = t.i1[d] = a.I[d] == a.O[d] ? o[d] : nearest_src(o[d], a.zf[d], a.I[d]);
            t.nt[d] = 1;
        }
    }
}

// class c at the taps: fp64 sum in tap order, ONE rounding to fp16 (`reshaped_final` has the logits' dtype: float16)
__device__ __forceinline__ unsigned short logits_resampled(const LogitsResizeGeom& a, const LogitsTaps& t, int c) {
    const size_t lv = (size_t)a.L[0] * a.L[1] * a.L[2];
    const unsigned short* base = a.logits + (size_t)c * lv;
    double s = 0.0;
    for (int p = 0; p < t.nt[0]; ++p)
        for (int q = 0; q < t.nt[1]; ++q)
            for (int r = 0; r < t.nt[2]; ++r) {
                const int x = (p ? t.i1[0] : t.i0[0]) + a.off[0], y = (q ? t.i1[1] : t.i0[1]) + a.off[1], z = (r ? t.i1[2] : t.i0[2]) + a.off[2];
                double cf = (double)us2f(base[((size_t)x * a.L[1] + y) * a.L[2] + z]);
                if (a.act[0]) cf *= t.w[0][p];
                if (a.act[1]) cf *= t.w[1][q];
                if (a.act[2]) cf *= t.w[2][r];
                s += cf;
            }
    return d2h_rn(s);
}

// host side: fills the geometry; false when a box leaves its grid or an extent is not positive
static inline bool logits_resize_geom(LogitsResizeGeom* a, const uint16_t* dev_logits, int C, const int grid_dims[3], const int* crop_off,
                                      const int* crop_dims, const int out_dims[3], int slice_axis, int* bad_axis) {
    a->logits = dev_logits;
    a->C = C;
    for (int d = 0; d < 3; ++d) {
        a->L[d] = grid_dims[d];
        a->off[d] = crop_off ? crop_off[d] : 0;
        a->I[d] = crop_dims ? crop_dims[d] : grid_dims[d];
        a->O[d] = out_dims[d];
        // (a->I <= a->L - a->off: no sum that could overflow)
        if (!(a->L[d] >= 1 && a->off[d] >= 0 && a->I[d] >= 1 && a->off[d] <= a->L[d] && a->I[d] <= a->L[d] - a->off[d] && a->O[d] >= 1)) {
            *bad_axis = d;
            return false;
        }
        a->act[d] = d != slice_axis;
        a->zf[d] = (double)a->I[d] / (double)a->O[d];
    }
    return true;
}
