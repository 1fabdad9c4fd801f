// higher_order_resampling: nnU-Net's one-hot label resampling (TS/resample_nnunet.py `resize_segmentation`, order 1) of a uint8
// label volume in ONE pass, whatever the number of classes.  The arithmetic of one voxel is resample_onehot.h; this file holds
// the per-axis tables and the volume pass.
//
//   k_onehot_tables     one OnehotTap (two clamped source indices, two fp64 weights) per output index of the two SLOW axes, built
//                       once per call.  The lanes of a wave share an output row almost always, so their table reads are one
//                       broadcast line each.
//   k_resample_onehot   every lane owns ONEHOT_RUN = 4 consecutive bytes of the (linear) output, so a wave stores 256 contiguous
//                       bytes with one aligned dword store per lane whatever the row length.  The entry of the FAST axis is computed
//                       per voxel from the zoom factor (six fp64 operations): a table of it would be read with a stride of 4
//                       entries per lane, 96 bytes, every lane its own cache line.  The 8 taps come from global memory: four
//                       source rows per output row, the source is a few tens of MB read by neighbouring lanes and stays in the
//                       caches.  The pass is bound by the VALU work of the label rounds (onehot_decide), not by its stores
//                       (DESIGN 4.18).
#include "common.h"
#include "resample_onehot.h"

#define ONEHOT_RUN 4

__global__ __launch_bounds__(256) void k_onehot_tables(OnehotTap* __restrict__ tab, int I0, int I1, int O0, int O1, double zf0,
                                                       double zf1, int sep_axis) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < O0)
        tab[i] = onehot_axis_tap(i, zf0, I0, O0, sep_axis != 0);
    else if (i < O0 + O1)
        tab[i] = onehot_axis_tap(i - O0, zf1, I1, O1, sep_axis != 1);
}

__global__ __launch_bounds__(256) void k_resample_onehot(const unsigned char* __restrict__ in, int I1, int I2,
                                                         const OnehotTap* __restrict__ tab, int O0, int O1, int O2, double zf2,
                                                         int act2, size_t n, unsigned char* __restrict__ out) {
    const size_t first = ((size_t)blockIdx.x * 256 + threadIdx.x) * ONEHOT_RUN;
    if (first >= n) return;
    int o0, o1, o2;
    idx3(first, O1, O2, o0, o1, o2);
    const OnehotTap* tab1 = tab + O0;
    OnehotTap t0 = tab[o0], t1 = tab1[o1];
    const unsigned char* row[4];
    onehot_rows(in, I1, I2, t0, t1, row);
    const int m = n - first < ONEHOT_RUN ? (int)(n - first) : ONEHOT_RUN;
    unsigned v = 0;
    for (int j = 0; j < m; ++j) {
        v |= (unsigned)onehot_voxel(row, t0, t1, onehot_axis_tap(o2, zf2, I2, O2, act2 != 0)) << (8 * j);
        if (++o2 == O2 && j + 1 < m) {   // the run goes on in the next row (there is one: first + j + 1 < n, so o0 stays below O0)
            o2 = 0;
            if (++o1 == O1) {
                o1 = 0;
                ++o0;
            }
            t0 = tab[o0];
            t1 = tab1[o1];
            onehot_rows(in, I1, I2, t0, t1, row);
        }
    }
    if (m == ONEHOT_RUN && (((uintptr_t)out) & 3) == 0)
        *(unsigned*)(out + first) = v;
    else
        for (int j = 0; j < m; ++j) out[first + j] = (unsigned char)(v >> (8 * j));
}

extern "C" int boa_resample_onehot_u8(boa_ctx* c, const uint8_t* dev_in, const int in_dims[3], uint8_t* dev_out,
                                      const int out_dims[3], int sep_axis) {
    BOA_REQUIRE(c && dev_in && dev_out && in_dims && out_dims, "boa_resample_onehot_u8: NULL argument");
    BOA_REQUIRE(sep_axis >= -1 && sep_axis <= 2, "boa_resample_onehot_u8: sep_axis %d", sep_axis);
    for (int a = 0; a < 3; ++a)
        BOA_REQUIRE(in_dims[a] >= 1 && out_dims[a] >= 1, "boa_resample_onehot_u8: bad dims on axis %d", a);
    BOA_REQUIRE(dev_in != dev_out, "boa_resample_onehot_u8: in place");
    const size_t on = (size_t)out_dims[0] * out_dims[1] * out_dims[2];
    if (in_dims[0] == out_dims[0] && in_dims[1] == out_dims[1] && in_dims[2] == out_dims[2]) {   // "no resampling necessary"
        BOA_HIP_TRY(hipMemcpyAsync(dev_out, dev_in, on, hipMemcpyDeviceToDevice, c->stream));
        return BOA_OK;
    }
    const size_t nt = (size_t)out_dims[0] + out_dims[1];
    BOA_REQUIRE(nt <= 0x7fffffffull, "boa_resample_onehot_u8: output extents too large");
    OnehotTap* tab = nullptr;
    BOA_TRY(boa_malloc(c, nt * sizeof(OnehotTap), (void**)&tab));
    const size_t runs = (on + ONEHOT_RUN - 1) / ONEHOT_RUN;
    KernelTimer t(c, BOA_K_RESAMPLE, 0, (double)on * 2.0);
    hipLaunchKernelGGL(k_onehot_tables, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream, tab, in_dims[0], in_dims[1],
                       out_dims[0], out_dims[1], onehot_zoom_factor(in_dims[0], out_dims[0]),
                       onehot_zoom_factor(in_dims[1], out_dims[1]), sep_axis);
    hipLaunchKernelGGL(k_resample_onehot, dim3((unsigned)((runs + 255) / 256)), dim3(256), 0, c->stream, dev_in, in_dims[1],
                       in_dims[2], tab, out_dims[0], out_dims[1], out_dims[2], onehot_zoom_factor(in_dims[2], out_dims[2]),
                       (int)(sep_axis != 2), on, dev_out);
    t.stop();
    hipError_t e = hipGetLastError();
    int rc = boa_free(c, tab);  // back to the context's pool: the next user is ordered behind this pass on the stream
    BOA_HIP_TRY(e);
    return rc;
}
