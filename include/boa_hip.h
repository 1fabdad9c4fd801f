/*
 * boa_hip.h -- C ABI of libboa_hip.so: the MI355X (gfx950) engine for the BOA hot path.
 *
 * The reference (UMEssen/Body-and-Organ-Analysis v1.0.1) is 100 % Python and has NO FFI / plugin interface
 * for this path: the boundary it exposes is the Python function surface of
 * body_organ_analysis/compute/ and of the vendored nnU-Net / TotalSegmentator / body_composition_analysis
 * packages.  This header is therefore the binding a maintainer would add underneath those functions (ctypes
 * stubs are shown in INTEGRATION.md).  Every entry point cites the reference code it replaces
 * (paths relative to the reference root; NN = body_organ_analysis/_external/nnunetv2,
 * TS = .../totalsegmentator, BCA = .../body_composition_analysis, BOA = body_organ_analysis).
 *
 * Conventions
 *   - plain C: pointers, sizes, ints; no torch / C++ types.  All functions return 0 on success, a negative
 *     BOA_E* code otherwise; boa_last_error() returns a thread-local message for the last failure.
 *   - "dev" pointers are HIP device pointers (from boa_malloc, or any hipMalloc / torch data_ptr() in the
 *     same process); "host" pointers are caller-owned and only borrowed for the duration of the call.
 *   - volumes use the nnU-Net array order [X][Y][Z] with Z contiguous (NN/imageio/nibabel_reader_writer.py:51-56)
 *     for the inference path and SimpleITK order [z][y][x] with x contiguous for the measurement path
 *     (BOA/compute/measurements.py:257-258); both are "3 dims, last contiguous" for the kernels.
 *   - all launches go to the context's stream; calls are asynchronous unless documented otherwise.
 *   - fp16 values are IEEE binary16 bit patterns carried as uint16_t.
 */
#ifndef BOA_HIP_H
#define BOA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BOA_OK 0
#define BOA_EINVAL (-1)   /* bad argument / unsupported geometry  (reference: ValueError / AssertionError) */
#define BOA_EHIP (-2)     /* HIP runtime error                     (reference: RuntimeError)              */
#define BOA_ENOMEM (-3)   /* device allocation failed              (reference: OOM -> CPU retry, predict_from_raw_data.py:663-672) */
#define BOA_EINF (-4)     /* inf in normalised logits              (reference: RuntimeError, predict_from_raw_data.py:622-625)     */

typedef struct boa_ctx boa_ctx;
typedef struct boa_net boa_net;

/* ------------------------------------------------------------------ context / memory / timing ------- */
const char* boa_last_error(void);
int boa_version(void);
/* One context per GPU (one process per GPU).  stream == NULL -> the context creates its own stream,
 * otherwise it borrows the given hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
int boa_init(int device, void* stream, boa_ctx** out);
void boa_destroy(boa_ctx* ctx);
int boa_device_info(boa_ctx* ctx, char* name, int name_len, int* cu_count, size_t* total_mem, size_t* free_mem);
/* Device memory for the caller's buffers (what `torch.empty(..., device="cuda")` / the caching allocator behind it is to the
 * reference).  Stream-ordered caching allocator: boa_free parks the block without synchronising the device, boa_malloc hands
 * a parked block of about the requested size out again; every use of a block must therefore be enqueued on the context's
 * stream (all boa_* calls are).  At most $BOA_POOL_GB (default 48; 0 = no caching) stays parked; boa_trim releases all of it.
 * Pointers that did not come from boa_malloc may be passed to boa_free (synchronise + hipFree). */
int boa_malloc(boa_ctx* ctx, size_t bytes, void** dev_out);
int boa_free(boa_ctx* ctx, void* dev);
int boa_trim(boa_ctx* ctx);
/* Several contexts may live on one GPU (each with its own stream and pool: boa_hip/lanes.py runs `total` and the BCA nets on two),
 * each driven by one host thread at a time; the pool itself is mutex-protected.  A host thread other than the one that called
 * boa_init makes the context's GPU its current device with this call before it drives the context (torch does the same per
 * thread with torch.cuda.set_device). */
int boa_bind_thread(boa_ctx* ctx);
/* Diagnostics (not on the data path): the rate a pure v_mfma_f32_32x32x16_f16 loop sustains on this GPU -- no memory, no LDS,
 * one wave per SIMD with 4 independent accumulator chains -- with near-constant operands (random_operands = 0) or operands whose
 * bits differ per lane and element (1).  The part is power-limited under matrix load: the second figure (1.5-1.7 PFLOP/s measured,
 * against 2.3-2.5 for the first and 2.5 on the data sheet) is the ceiling a conv on real activations can be priced against. */
int boa_mfma_peak(boa_ctx* ctx, int random_operands, int iters, double* tflops_out);
int boa_memset(boa_ctx* ctx, void* dev, int value, size_t bytes);
int boa_h2d(boa_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);   /* synchronous */
int boa_d2h(boa_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);   /* synchronous */
/* Page-locked host memory for the volumes that cross PCIe (what `tensor.pin_memory()` is to the reference): boa_h2d / boa_d2h
 * from / to such a buffer run at link speed instead of through the runtime's pageable staging copies.  boa_host_free accepts
 * ctx == NULL (the buffer may outlive the context that allocated it). */
int boa_host_alloc(boa_ctx* ctx, size_t bytes, void** host_out);
int boa_host_free(boa_ctx* ctx, void* host);
int boa_sync(boa_ctx* ctx);
/* HIP-event timing on the context stream: ms between the two marks (boa_timer_stop synchronises). */
int boa_timer_start(boa_ctx* ctx, int slot);
int boa_timer_stop(boa_ctx* ctx, int slot, float* ms_out);
/* Per-kernel-class accumulated time, measured with HIP events around every launch of that class while
 * profiling is enabled (bench.py uses this for `roofline.achieved`).  Classes: see BOA_K_*. */
#define BOA_K_CONV_MFMA 0
#define BOA_K_CONV_FIRST 1
#define BOA_K_CONVT 2
#define BOA_K_NORM_FINALIZE 3
#define BOA_K_HEAD_ACCUM 4
#define BOA_K_ARGMAX 5
#define BOA_K_OTHER 6      /* memset, CTNormalization */
#define BOA_K_AGG 7        /* tissue map / slice tables / label histograms / masks (agg.hip, agg_f64.hip); erosion (morph.hip, ccl_bits.hip) */
#define BOA_K_MORPH 8      /* connected components (ccl_bytes.hip, ccl_bits.hip), contour fill, median (morph.hip) */
#define BOA_K_RESAMPLE 9   /* cubic / nearest resampling (resample.hip) */
#define BOA_K_COPY 10      /* boa_copy3 index remaps (reorientation, transposes, crops) */
#define BOA_K_COUNT 11
int boa_prof_enable(boa_ctx* ctx, int on);
int boa_prof_reset(boa_ctx* ctx);
int boa_prof_get(boa_ctx* ctx, int kclass, double* total_ms, long long* launches, double* flops, double* bytes);
/* Which kernel VARIANT ran (always on, independent of profiling): number of launches since the context was created or the
 * counter was last reset.  The parity tests assert with these that the kernel they check is the one the product path and
 * bench.py launch (e.g. the MFMA head, not its fp32 VALU fallback).  Returns the count, < 0 on a bad argument. */
#define BOA_CNT_HEAD_MFMA 0       /* k_head_mfma (accumulate or logits mode)                           */
#define BOA_CNT_HEAD_VALU 1       /* k_head<F0, VPT> fallback (unaligned z origin / P2 % 32 / F0 = 64) */
#define BOA_CNT_CONV_WS 2         /* k_conv_ws (wave-specialised persistent conv)                     */
#define BOA_CNT_CONV_SIMPLE 3     /* k_conv_mfma (fallback for kernel shapes k_conv_ws lacks)          */
#define BOA_CNT_FIRST_MFMA 4      /* k_conv_first_mfma                                                 */
#define BOA_CNT_FIRST_VALU 5      /* k_conv_first<K> fallback                                          */
#define BOA_CNT_F32 6             /* any kernel of the fp32 reference network mode (precision = 1)     */
#define BOA_CNT_CONV_X3 7         /* k_conv_ws<..., X3>: split-precision conv (precision = 2)          */
#define BOA_CNT_X3 8              /* the other kernels of the split-precision mode (first conv, transposed conv, head) */
#define BOA_CNT_HEAD_GATHER 9     /* k_gather_head* (fused head over all covering tiles; raw partial sums in the tile-sharded path) */
#define BOA_CNT_COPY_T 10         /* k_copy3_t (LDS-tiled transposing form of boa_copy3; k_copy3 otherwise)             */
#define BOA_CNT_BBOX_VEC 11       /* k_nonzero_bbox with its 16-byte vector loop (per-element loop otherwise)          */
#define BOA_CNT_FINALIZE_VEC8 12 /* k_finalize_labels<8> (16-byte accesses; k_finalize_labels<1> otherwise)               */
#define BOA_CNT_COUNT 13
long long boa_debug_counter(boa_ctx* ctx, int which, int reset);

/* ------------------------------------------------------------------ sliding-window arithmetic seams -- */
/* CTNormalization.run (NN/preprocessing/normalization/default_normalization_schemes.py:53-67):
 * out = ((float)clip(in, lo, hi) - mean) / max(std, 1e-8) in fp32.  in_dtype: 0 = int16, 1 = float32, 2 = int32
 * (the dtype TS/nnunet.py:472-474 resamples to; the nibabel reader casts it to float32). */
int boa_ct_normalize(boa_ctx* ctx, const void* dev_in, int in_dtype, float* dev_out, size_t n,
                     float mean, float std, float lo, float hi);

/* One iteration of the tile loop, NN/inference/predict_from_raw_data.py:611-614, given the tile's logits:
 *   pred *= gauss (fp32*fp16->fp32); acc[:, sl] += pred (fp16 RTNE); n[sl] += gauss (fp16 RTNE).
 * pred:  dev fp32 [C][P0][P1][P2]; gauss: dev fp16 [P0][P1][P2] or NULL (use_gaussian=False: weight 1);
 * acc:   dev fp16 [C][V0][V1][V2]; n: dev fp16 [V0][V1][V2]; start: tile origin in the volume. */
int boa_accumulate_tile(boa_ctx* ctx, const float* dev_pred, const uint16_t* dev_gauss, uint16_t* dev_acc,
                        uint16_t* dev_n, int C, const int P[3], const int V[3], const int start[3]);

/* torch.div(logits, n, out=logits) + inf check (predict_from_raw_data.py:620-625), fold accumulation
 * (`prediction += ...`, :494-500), `/= n_folds`, numpy argmax(0) on fp16 with first-max / NaN-is-max semantics
 * (NN/utilities/label_handling/label_handling.py:175-178) and the TotalSegmentator part->global remap
 * `seg_combined[seg == jdx] = class_map_inv[name]` (TS/nnunet.py:553-556), fused in one pass over the volume.
 *
 *   acc, n      dev fp16 accumulators of THIS fold/model (acc is overwritten with acc/n when write_logits != 0)
 *   fold_sum    dev fp16 [C][V] running fold sum, or NULL.  When non-NULL: fold_mode 0 = store (first fold),
 *               1 = add (fp16 + fp16 -> fp16), and when n_folds_final > 0 the sum is divided by n_folds_final
 *               (fp16) before the argmax; the argmax is skipped when n_folds_final == 0 (more folds to come).
 *   lut         host uint8[256] mapping local argmax index -> output label (NULL = identity)
 *   merge       0: labels_out[v] = lut[argmax];  1: labels_out[v] = lut[argmax] only where argmax != 0
 *               (later parts overwrite earlier ones, background never overwrites)
 *   crop_off/crop_dims: revert pad_nd_image (predict_from_raw_data.py:657,679): labels_out is
 *               [crop_dims] and voxel (i,j,k) comes from padded voxel (i+off0, j+off1, k+off2); NULL = no crop.
 *   inf_flag    dev int32, set to 1 if any normalised logit is +-inf (caller raises, BOA_EINF semantics).
 */
int boa_finalize_labels(boa_ctx* ctx, uint16_t* dev_acc, const uint16_t* dev_n, int C, const int V[3],
                        uint16_t* dev_fold_sum, int fold_mode, int n_folds_final, int write_logits,
                        const uint8_t* host_lut, int merge, uint8_t* dev_labels_out,
                        const int* crop_off, const int* crop_dims, int* dev_inf_flag);
/* boa_finalize_labels restricted to planes [plane_lo, plane_hi) of axis 0 of the padded grid (the planes a rank owns in
 * the tile-sharded mode); acc / n / fold_sum keep the full-grid layout. */
int boa_finalize_labels_planes(boa_ctx* ctx, uint16_t* dev_acc, const uint16_t* dev_n, int C, const int V[3],
                               uint16_t* dev_fold_sum, int fold_mode, int n_folds_final, int write_logits,
                               const uint8_t* host_lut, int merge, uint8_t* dev_labels_out, const int* crop_off,
                               const int* crop_dims, int* dev_inf_flag, int plane_lo, int plane_hi);

/* ------------------------------------------------------------------ network (PlainConvUNet) ---------- */
/* Geometry of dynamic_network_architectures PlainConvUNet as the reference instantiates it from plans.json
 * (NN/utilities/plans_handling/plans_handler.py:59-92; NN/utilities/get_network_from_plans.py:34-38):
 * encoder stages of n_conv x [Conv3d(k, stride on first conv, pad (k-1)/2, bias) -> InstanceNorm3d(eps 1e-5,
 * affine) -> LeakyReLU(0.01)], decoder stages of ConvTranspose3d(k = s = stride, bias) -> cat(up, skip) ->
 * n_conv blocks, final 1x1x1 Conv3d head (deep supervision off, predict_from_raw_data.py:110). */
#define BOA_MAX_STAGES 8
typedef struct {
    int n_stages;
    int in_channels;
    int num_classes;
    int features[BOA_MAX_STAGES];
    int kernel[BOA_MAX_STAGES][3];
    int stride[BOA_MAX_STAGES][3];
    int n_conv_enc[BOA_MAX_STAGES];
    int n_conv_dec[BOA_MAX_STAGES]; /* n_stages - 1 entries, decoder order (deepest first) */
    int patch[3];
    float norm_eps;
    float lrelu_slope;
} boa_net_desc;

/* weights: host fp32 blob, tensors concatenated in this order, PyTorch memory layout:
 *   for each encoder stage s, conv i:  W[Cout][Cin][k0][k1][k2], b[Cout], gamma[Cout], beta[Cout]
 *   for each decoder stage d (deepest first): Wt[Cin][Cout][s0][s1][s2], bt[Cout], then for conv i: W, b, gamma, beta
 *   head: W[num_classes][features[0]], b[num_classes]
 * (state-dict keys encoder.stages.S.0.convs.I.{conv,norm}.*, decoder.transpconvs.D.*, decoder.stages.D.convs.I.*,
 *  decoder.seg_layers.<last>.*).
 * precision: 0 = fp16 weights / activations on the f16 matrix cores with fp32 accumulation (production; what the reference's
 * CUDA path computes under autocast, predict_from_raw_data.py:648); 1 = fp32 "exact" mode: fp32 weights, activations and
 * accumulation (v_mfma_f32_32x32x2_f32) = what the reference's CPU path computes; a correctness mode, ~30x slower. */
int boa_net_create(boa_ctx* ctx, const boa_net_desc* desc, const float* host_weights, size_t n_floats,
                   int max_batch, int precision, boa_net** out);
void boa_net_destroy(boa_net* net);
size_t boa_net_weight_count(const boa_net_desc* desc); /* expected n_floats, 0 on invalid desc */
/* swap weights (next fold), NN/inference/predict_from_raw_data.py:486-489 `load_state_dict(params)` */
int boa_net_load_weights(boa_net* net, const float* host_weights, size_t n_floats);

/* Test-time mirroring, `_internal_maybe_mirror_and_predict` (predict_from_raw_data.py:541-557): with axes_mask != 0 (bit a =
 * array axis a of the allowed mirroring axes) every tile's logits become the fp32 mean over the plain forward and the
 * forwards of all non-empty axis combinations of the flipped tile, flipped back -- (2^axes) x the network cost.  BOA runs
 * every model with tta=False (TS/python_api.py:753); the switch exists because nnUNetPredictor(use_mirroring=True) does. */
int boa_net_set_mirroring(boa_net* net, int axes_mask);

/* network(x) for a batch of tiles gathered from a resident volume
 * (replaces `self.network(workon)` predict_from_raw_data.py:543 + producer thread :568-571):
 *   volume   dev fp32 [Cin][V0][V1][V2] (already normalised); tile voxels outside the volume read as 0
 *            (pad_nd_image) -- origins may be negative / overhang for volumes smaller than the patch.
 *   origins  host int[n_tiles][3]
 *   logits   dev fp32 [n_tiles][num_classes][P0][P1][P2]  (PyTorch NCDHW)  */
int boa_net_forward(boa_net* net, const float* dev_volume, const int V[3], const int* host_origins,
                    int n_tiles, float* dev_logits_out);

/* Whole `_internal_predict_sliding_window_return_logits` loop (predict_from_raw_data.py:560-631) for one
 * fold: for every tile in the given (canonical x->y->z) order: forward, head, *gauss, fp16 accumulate.
 * acc/n must be zeroed by the caller (boa_memset).  vol_off: position of the real volume inside the padded
 * accumulator grid (pad_nd_image `below`), NULL = {0,0,0}.  Tiles are processed in batches of <= max_batch
 * through the conv stack; accumulation is applied strictly in the given order.
 *   PV  padded accumulator dims (>= patch), V real volume dims. */
int boa_net_predict_sliding_window(boa_net* net, const float* dev_volume, const int V[3], const int PV[3],
                                   const int* vol_off, const int* host_origins, int n_tiles,
                                   const uint16_t* dev_gauss, uint16_t* dev_acc, uint16_t* dev_n);

/* Fused form of the same loop for the label-only path (csrc/head_gather.hip): the conv stack leaves the last decoder activation
 * of EVERY tile in a stash, then one pass over the volume walks, per voxel, the covering tiles in ascending tile index (the
 * reference's `+=` order, predict_from_raw_data.py:611-614) with the running fp16 sums in registers and goes on to the
 * normalisation, fold sum / mean (:483-500), argmax, label remap and crop of boa_finalize_labels -- the accumulator planes never
 * exist.  Same arithmetic and rounding sequence as boa_net_predict_sliding_window + boa_finalize_labels (labels bit-identical;
 * tests/test_gpu_gather_head.py).  One call per fold (after boa_net_load_weights), fold_index ascending:
 *   dev_fold        fp16 [C][PV] scratch, n_folds > 1 only (the fold sum lives there between the calls)
 *   dev_labels_out  written by the LAST fold's call (merge / lut / crop_off / crop_dims as in boa_finalize_labels)
 *   dev_inf_flag    set non-zero if a normalised logit is +-inf (:622-625)
 * boa_net_labels_supported: 1 when the network / tile layout qualifies (production precision, no mirroring, 32 features at
 * full resolution, <= 31 classes, patch z extent a multiple of 32, tile origins = the cartesian grid of compute_steps_for_sliding_window in canonical order).
 * Returns BOA_ENOMEM when the stash (n_tiles x patch voxels x 64 B) does not fit: the caller falls back to the loop above. */
int boa_net_labels_supported(boa_net* net, const int* host_origins, int n_tiles);
int boa_net_predict_labels_fold(boa_net* net, const float* dev_volume, const int V[3], const int PV[3], const int* vol_off,
                                const int* host_origins, int n_tiles, const uint16_t* dev_gauss, uint16_t* dev_fold,
                                int fold_index, int n_folds, const uint8_t* host_lut, int merge, uint8_t* dev_labels_out,
                                const int* crop_off, const int* crop_dims, int* dev_inf_flag);

/* ---- one volume on several GPUs (SURVEY 8e "tile partitioning"): each rank owns a block of tile rows along axis 0 ----
 * Same loop as boa_net_predict_sliding_window over THIS rank's tiles, except that for tile i the first
 * host_defer_planes[i] planes (axis 0) are not accumulated: their head input is kept in *stash_out.  The caller places
 * the lower rank's partial sums for those planes into acc / n (they were received over RCCL/xGMI) and then calls
 * boa_net_apply_deferred, which adds the stashed planes in the original tile order -- per voxel the fp16 `+=` sequence
 * is the reference's (predict_from_raw_data.py:611-614), so the result is bit-identical to the single-GPU loop.
 * The stash remembers the head weights of the fold that produced it (it may be applied after the network switched folds).
 * acc / n must be zero on entry in the planes this rank's tiles cover: when the network and tile grid qualify
 * (boa_net_labels_supported) the non-deferred planes are WRITTEN by one gather-head launch (raw partial sums, all covering
 * tiles of this rank in ascending order) and boa_net_apply_deferred is one more launch of that kernel over the deferred
 * planes, started from the planes' contents; otherwise both run the per-tile scatter head.  With host_defer_planes all
 * zero this is the single-GPU accumulate loop in its gather form (the resampled label path uses it that way). */
typedef struct boa_stash boa_stash;
int boa_net_predict_sliding_window_deferred(boa_net* net, const float* dev_volume, const int V[3], const int PV[3],
                                            const int* vol_off, const int* host_origins, int n_tiles,
                                            const uint16_t* dev_gauss, uint16_t* dev_acc, uint16_t* dev_n,
                                            const int* host_defer_planes, boa_stash** stash_out);
int boa_net_apply_deferred(boa_net* net, const boa_stash* stash, const uint16_t* dev_gauss, uint16_t* dev_acc,
                           uint16_t* dev_n, const int PV[3]);
void boa_stash_destroy(boa_stash* stash);

/* Debug / unit-test seam: run ONE conv block on device tensors in PyTorch layout.
 *   in  dev fp32 [N][Cin][D][H][W], w/b/gamma/beta host fp32; out dev fp32 [N][Cout][Do][Ho][Wo] =
 *   LeakyReLU(InstanceNorm(Conv3d(in))) when with_norm_act != 0, else the raw convolution (+bias).
 * impl: 0 = MFMA implicit-GEMM kernel, 1 = naive direct kernel (on-device cross-check). */
int boa_conv_block_test(boa_ctx* ctx, const float* dev_in, int N, int Cin, const int dims[3],
                        const float* host_w, const float* host_b, const float* host_gamma, const float* host_beta,
                        int Cout, const int kernel[3], const int stride[3], int with_norm_act, int impl,
                        float* dev_out); /* impl must be 0 */
/* Debug seam for the per-layer error report (fp16 production mode against the fp32 exact mode, tools/layer_error.py): the
 * activation a layer left behind for `tile` of the LAST batch that went through the conv stack, as fp32 [C][D][H][W] with the
 * layer's InstanceNorm + LeakyReLU applied (i.e. what the next layer consumes; transposed convs have no norm: raw output).
 * kind 0 = encoder conv (stage, conv), 1 = transposed conv (stage = decoder index, deepest first), 2 = decoder conv.
 * dev_out == NULL only returns channels / dims. */
int boa_net_debug_activation(boa_net* net, int kind, int stage, int conv, int tile, float* dev_out, int* channels_out,
                             int dims_out[3]);
/* Per-layer test seam (tests/test_gpu_layer_parity.py): what one layer stored for `tile` of the LAST batch through the conv stack,
 * with the same (kind, stage, conv) addressing as boa_net_debug_activation.
 *   dev_raw   (may be NULL) dev fp32 [C][D][H][W]: the layer's RAW stored output (pre-norm conv output + bias; fp16 storage widened
 *             exactly, fp32 / octet storage as it is)
 *   host_ss   (may be NULL) host fp32 [C][2]: the (scale, shift) the consumers apply, lrelu(raw * scale + shift); (1, 0) for a
 *             transposed conv, whose output is consumed raw
 *   host_ss16 (may be NULL; fp16-mode convs only) host uint16 [C/2][4]: the packed words the fp16 consumers read,
 *             {scale(c), scale(c + 1), shift(c), shift(c + 1)} as fp16 bits per channel pair
 *   host_info (may be NULL) int[3]: {BOA_LK_* kernel that ran, R of k_conv_ws / k_conv_ns / k_conv_mfma or MT of k_convt_x3,
 *             convs: 1 if k_conv_ws ran its row-reuse form (split precision: the tap-paired loop); transposed convs: log2 of the
 *             power of two the split-precision mode folds into the stored output (dev_raw has it taken out again)}
 * kind 3 = the head (stage, conv ignored): reports channels / dims / host_info[0] only; dev_raw, host_ss, host_ss16 must be NULL. */
#define BOA_LK_FIRST_VALU 1   /* k_conv_first (fp32 VALU)       */
#define BOA_LK_FIRST_MFMA 2   /* k_conv_first_mfma              */
#define BOA_LK_CONV_WS 3      /* k_conv_ws                      */
#define BOA_LK_CONV_NS 4      /* k_conv_ns                      */
#define BOA_LK_CONV_MFMA 5    /* k_conv_mfma fallback           */
#define BOA_LK_CONV_F32 6     /* fp32 mode conv (net_f32.hip)   */
#define BOA_LK_CONVT_X3 7     /* k_convt_x3                     */
#define BOA_LK_CONVT_MFMA 8   /* k_convt_mfma                   */
#define BOA_LK_CONVT_RW 9     /* k_convt_mfma_rw                */
#define BOA_LK_CONVT_DEEP 10  /* k_convt_deep                   */
#define BOA_LK_CONVT_F32 11   /* fp32 mode transposed conv      */
#define BOA_LK_HEAD_X3 12     /* k_head_x3                      */
#define BOA_LK_HEAD_F32 13    /* k_head_f32 (fp32 / octet input) */
#define BOA_LK_HEAD_MFMA 14   /* launch_head: k_head_mfma or its VALU fallback (boa_debug_counter tells which) */
int boa_net_debug_layer(boa_net* net, int kind, int stage, int conv, int tile, float* dev_raw, float* host_ss, uint16_t* host_ss16,
                        int* channels_out, int dims_out[3], int* host_info);

/* Unit-test seam: the fused 1x1x1 head + Gaussian-weighted fp16 accumulation of ONE tile, launched exactly as the tile
 * loop of boa_net_predict_sliding_window launches it (same kernel selection: the MFMA head when F0 == 32, C <= 31,
 * P[2] % 32 == 0 and the z origin / extent are 8-voxel aligned, else the fp32 VALU head; boa_debug_counter tells which).
 *   act  dev fp16 [F0/16][P0][P1][P2][16] (the engine's chunk-planar activation layout): the last decoder conv's raw output;
 *        ss dev fp32 [F0][2] its InstanceNorm (scale, shift)
 *   w    dev fp32 [C][F0], b dev fp32 [C]
 *   logits_out != NULL: write the tile's fp32 logits [C][P0][P1][P2] (what `self.network(x)` returns, :543);
 *   logits_out == NULL: `pred *= gauss; acc[sl] += pred; n[sl] += gauss` (:611-614) on acc [C][PV] / n [PV] at `start`.
 * The two modes run the same instruction sequence up to the logit, so accumulating tiles and comparing with the oracle's
 * accumulate step applied to the logits-mode output checks the production accumulate arithmetic bit for bit. */
int boa_head_tile(boa_ctx* ctx, const uint16_t* dev_act, const float* dev_ss, int F0, const int P[3], int C,
                  const float* dev_w, const float* dev_b, float slope, float* dev_logits_out, const uint16_t* dev_gauss,
                  uint16_t* dev_acc, uint16_t* dev_n, const int PV[3], const int start[3]);
/* The same seam for the fp32-input heads.  kind = BOA_LK_HEAD_X3 (k_head_x3: act = octet planes [4][stride voxels][8], F0 == 32, at most
 * 32 classes) or BOA_LK_HEAD_F32 (k_head_f32: stride == 0: channels-last records [voxel][F0]; else octet planes [F0/8][stride voxels][8]).
 * The remaining arguments are boa_head_tile's; the call forwards to the launcher the network driver uses and does nothing else. */
int boa_head_tile_f32(boa_ctx* ctx, int kind, const float* dev_act_f32, size_t stride, const float* dev_ss, int F0, const int P[3], int C,
                      const float* dev_w, const float* dev_b, float slope, float* dev_logits_out, const uint16_t* dev_gauss,
                      uint16_t* dev_acc, uint16_t* dev_n, const int PV[3], const int start[3]);
int boa_convtranspose_test(boa_ctx* ctx, const float* dev_in, int N, int Cin, const int dims[3],
                           const float* host_w, const float* host_b, int Cout, const int stride[3], float* dev_out);

/* Host-only plan query (no GPU touched, no context): everything that selects code for one conv / transposed conv of a network, from
 * the functions the network set-up and the launchers call.  mode: 0 = fp16, 2 = split precision.  plan_override (may be NULL):
 * {variant, R, w[3], b[3]} instead of the planner's choice, completed and checked as the planner's candidates are (BOA_EINVAL where
 * the planner would skip it).  plan_out: int[BOA_PLAN_WORDS]
 *   conv : 0 variant (0 k_conv_mfma, 1 k_conv_ws, 2 k_conv_ns), 1 R, 2-4 w, 5-7 b, 8-10 h, 11 xs, 12-14 tiles, 15 lds_bytes, 16 row reuse,
 *          17 resident weights, 18 cy_fast, 19 vw, 20 nslots, 21 cout waves of k_conv_ns, 22 cout groups per spatial tile, 23 nblk (the
 *          statistics slots per (n, cout): the partials table holds [N][Cout][2][nblk] floats), 24-26 output dims, 27 BOA_LK_*, 28 split
 *   convT: 0 convt_mfma_form (-1: split precision), 1 MT of k_convt_x3, 2 BOA_LK_*, 3 stride of the last axis, 4 Cin / 16, 5-7 output dims */
#define BOA_PLAN_WORDS 32
int boa_conv_plan(int Cin0, int Cin1, const int dims[3], int Cout, const int kernel[3], const int stride[3], int cu_count, int mode,
                  const int* plan_override, int* plan_out);
int boa_convt_plan(int Cin, const int dims[3], int Cout, const int stride[3], int cu_count, int mode, int norm_src, int* plan_out);
/* Unit-test seams: ONE layer launched as the network launches it (production packers, launch_conv_mfma / launch_conv_x3 +
 * launch_norm_finalize, launch_convt_mfma / launch_convt_x3), with the plan of boa_conv_plan for the context's CU count.
 *   sources   dev fp32 [N][C][D][H][W], converted to the mode's layout (fp16 chunk planes / fp32 octet planes); per source the
 *             producer's tables or NULL (raw source): dev_ss fp32 [N][C][2], and for the fp16 mode dev_ss16 [N][C/2][2] packed words
 *   dev_raw   the kernel's own output buffer in the mode's layout: fp16 [N][Cout/16][vox][16] / fp32 [N][Cout/8][vox][8]
 *   dev_ss [N][Cout][2], dev_ss16 [N][Cout] words (fp16 mode, else NULL), dev_partials [N][Cout][2][nblk] floats, ZEROED by the caller
 *   host_plan (may be NULL) int[BOA_PLAN_WORDS]: the plan that ran
 * boa_convt_layer_test, fp16 mode: dev_ss without dev_ss16 runs k_convt_mfma's fp32-table transform (the network always passes both) */
int boa_conv_layer_test(boa_ctx* ctx, int mode, int N, const int dims[3], const float* dev_src0, int C0, const float* dev_ss0,
                        const uint32_t* dev_ss16_0, const float* dev_src1, int C1, const float* dev_ss1, const uint32_t* dev_ss16_1,
                        const float* host_w, const float* host_b, const float* host_gamma, const float* host_beta, int Cout,
                        const int kernel[3], const int stride[3], const int* plan_override, void* dev_raw, float* dev_ss,
                        uint32_t* dev_ss16, float* dev_partials, int* host_plan);
int boa_convt_layer_test(boa_ctx* ctx, int mode, int N, const int dims[3], const float* dev_src, int Cin, const float* dev_ss,
                         const uint32_t* dev_ss16, const float* host_w, const float* host_b, int Cout, const int stride[3], void* dev_raw,
                         int* host_plan);

/* ------------------------------------------------------------------ body-composition / HU aggregation - */
/* subclassify_tissues (BCA/tissue/subclassification.py:38-53, rules BCA/tissue/definition.py:6-30) fused with
 * the slice-wise voxel counts of Builder.prepare (BCA/report/builder.py:403-444) and the per-slice HU sums that
 * `np.mean(image[tissue_mask])` (builder.py:284-305) needs.
 *   ct int16 [Z][Y][X], regions uint8, parts uint8 (may be NULL -> no torso counts), tissues_out uint8 (may be NULL)
 *   ct_rules (may be NULL = ct): the HU the derivation rules look at -- the 3x3 in-plane median-filtered CT when
 *           median_filtering is on (subclassification.py:21-36); HU sums always come from `ct` (builder.py gets the
 *           unfiltered image)
 *   counts  dev uint32 [Z][2][8]   (index 0 unused; [0] = all voxels, [1] = body_parts == TORSO(1))
 *   hu_sums dev int64  [Z][2][8]
 * counts/hu_sums are overwritten. */
int boa_tissue_aggregate(boa_ctx* ctx, const int16_t* dev_ct, const int16_t* dev_ct_rules, const uint8_t* dev_regions,
                         const uint8_t* dev_parts,
                         uint8_t* dev_tissues_out, int Z, int Y, int X, uint32_t* dev_counts, int64_t* dev_hu_sums);

/* Per-slice presence of each label value (np.where(mask.any(axis=(1,2))) in builder.py:56-100,170-199 and
 * BCA/commands.py:24-45): present[z][label] = 1 if any voxel of slice z has that label. dev uint8 [Z][256]. */
int boa_slice_label_presence(boa_ctx* ctx, const uint8_t* dev_labels, int Z, int Y, int X, uint8_t* dev_present);

/* The reductions behind the report's coronal / sagittal tissue heat maps (BCA/report/plots/heatmaps.py:29-101), one pass
 * over the (z,y,x) uint8 volumes: for each tissue value v_t (host_values, 1..16 of them)
 *   coronal[t][z][x]  = #{y : tissues[z,y,x] == v_t}     (`tissue_mask.sum(axis=1)`)
 *   sagittal[t][z][y] = #{x : tissues[z,y,x] == v_t}     (`tissue_mask.sum(axis=2)`)
 * and the body silhouettes `((regions > 0) & (regions < 255)).any(axis)`: mask_coronal[z][x], mask_sagittal[z][y] (0/1).
 * Colour mapping / resizing / contour drawing of the report stay on the host (out of scope). */
int boa_tissue_projections(boa_ctx* ctx, const uint8_t* dev_tissues, const uint8_t* dev_regions, int Z, int Y, int X,
                           const uint8_t* host_values, int n_values, uint32_t* dev_coronal, uint32_t* dev_sagittal,
                           uint8_t* dev_mask_coronal, uint8_t* dev_mask_sagittal);

/* One pass replacing the ~125 full-volume passes of metrics_for_each_region (BOA/compute/measurements.py:74-123,
 * 203-241): histogram of HU per label.  hist dev uint32 [256][nbins], bin = clamp(hu - hu_min, 0, nbins-1);
 * mask (optional dev uint8, same shape): only voxels with mask != 0 are counted (eroded / fat-window masks).
 * hist is overwritten.  Exact order statistics (median, percentiles), mean, std, min, max follow on the host
 * from integer counts. */
int boa_label_hu_histogram(boa_ctx* ctx, const int16_t* dev_ct, const uint8_t* dev_labels, const uint8_t* dev_mask,
                           size_t n_voxels, int hu_min, int nbins, uint32_t* dev_hist);

/* mask_out = (lut[labels] != 0) && (hu_lo <= ct <= hu_hi  [in_range] | ct < hu_lo || ct > hu_hi [!in_range]);
 * get_region_minus_fat / compute_lung_measurement fat masks (BOA/compute/measurements.py:29-39,126-148).
 * lut: host uint8[256]; mode 0 = label only, 1 = inside [lo,hi], 2 = outside [lo,hi]. */
int boa_label_hu_mask(boa_ctx* ctx, const int16_t* dev_ct, const uint8_t* dev_labels, const uint8_t* host_lut,
                      int mode, int hu_lo, int hu_hi, size_t n_voxels, uint8_t* dev_mask_out);

/* get_basic_statistics (TS/statistics.py:76-141: `seg == k`, touches_border, `data.sum()`, np.average per structure, 117 times over
 * the volume) as one pass over a contiguous uint8 label volume [d0][d1][d2] (d2 fastest) and the CT on the same grid (ct_dtype 1 int16,
 * 2 int32: the model-grid image needs no conversion copy).  dev_out, BOA_LABEL_STATS_WORDS 64-bit words, is overwritten:
 *   [0, 256)    uint64 count of every label value (0 included)
 *   [256, 512)  int64  sum of the CT values under it
 *   [512, 768)  uint64 non-zero if a voxel of the label has `i < border || i >= dim - border` on any axis -- numpy's `mask[:3]` /
 *               `mask[-3:]` of touches_border (TS/statistics.py:76-88), also for dims shorter than 2 * border and than border
 *   [768], [769] int64 min and max of the CT (INT64_MAX, INT64_MIN for an empty volume)
 * Integer arithmetic throughout: independent of the order of arrival, bitwise reproducible.  Both arrays must be 16-byte aligned.
 * Does not synchronise. */
#define BOA_LABEL_STATS_WORDS 770
int boa_label_basic_stats(boa_ctx* ctx, const void* dev_ct, int ct_dtype, const uint8_t* dev_labels, const int dims[3], int border,
                          uint64_t* dev_out);
/* out[i] = host_lut[labels[i]]; `img_data *= np.isin(img_data, subset labels)` of roi_subset (TS/nnunet.py:707-709) is the table with
 * lut[v] = v for the subset and 0 elsewhere.  In place (out == labels) is allowed. */
int boa_label_apply_lut(boa_ctx* ctx, const uint8_t* dev_labels, size_t n, const uint8_t host_lut[256], uint8_t* dev_out);

/* ---- the same measurements on CT values held as float64 (`get_fdata()` of a float-valued, scaled or out-of-int16-range CT;
 * the reference computes on whatever array its reader hands over: BOA/compute/measurements.py:257-258, BCA/report/builder.py).
 *
 * boa_group_stats_f64: what `np.mean / std / min / max / median / percentile(hu_region, 25 | 75)` of metrics_for_region
 * (BOA/compute/measurements.py:95-112) need, for up to 255 voxel groups at once.  host_lut[256] maps a label value to its group
 * (0xFF: not measured); label unions are LUT entries with the same group, a 0/1 mask with lut[1] = 0 is the masked form.
 *   host_count[n_groups]                               voxels per group (exact)
 *   host_stats[n_groups][BOA_GROUP_STATS_F64_COLS]     min, max, sum, m2, then the order statistics (0-based ranks in the sorted
 *       group) floor((count-1)/4), ceil((count-1)/4), floor((count-1)/2), ceil((count-1)/2), floor(3(count-1)/4), ceil(3(count-1)/4)
 *   m2 = sum((x - sum / count)^2), taken in a second pass about the fp64 mean as np.std does.
 * min, max and the order statistics are exact (radix select on the 64 bits of the values, eight passes of 9 B per voxel; no
 * sort, no download of the volume); sum and m2 are fp64 sums whose last bits depend on the order of the atomic adds.  Values
 * must be finite (the host checks before it uploads).  Rows of empty groups are zero.  Synchronous. */
#define BOA_GROUP_STATS_F64_COLS 10
int boa_group_stats_f64(boa_ctx* ctx, const double* dev_ct, const uint8_t* dev_labels, size_t n_voxels, const uint8_t* host_lut,
                        int n_groups, uint64_t* host_count, double* host_stats);
/* boa_label_hu_mask on float64 HU: the window is compared on the float value itself (`ct >= lo`, `ct < lo`: no rounding). */
int boa_label_hu_mask_f64(boa_ctx* ctx, const double* dev_ct, const uint8_t* dev_labels, const uint8_t* host_lut,
                          int mode, double hu_lo, double hu_hi, size_t n_voxels, uint8_t* dev_mask_out);
/* boa_tissue_aggregate on float64 HU: the derivation rules compare the float value (-29.5 is neither muscle nor adipose tissue),
 * counts and the tissue map are exact, hu_sums is dev double [Z][2][8]. */
int boa_tissue_aggregate_f64(boa_ctx* ctx, const double* dev_ct, const double* dev_ct_rules, const uint8_t* dev_regions,
                             const uint8_t* dev_parts, uint8_t* dev_tissues_out, int Z, int Y, int X, uint32_t* dev_counts,
                             double* dev_hu_sums);

/* erode_region (BOA/compute/measurements.py:61-71): binary erosion with a k^3 ones footprint whose anchor is
 * the centre of the end-padded (k+1)^3 footprint for even k; voxels outside the volume count as set.
 * Separable min filter, three passes. tmp: dev uint8 scratch of the same size. */
int boa_binary_erode(boa_ctx* ctx, const uint8_t* dev_mask, uint8_t* dev_out, uint8_t* dev_tmp, int Z, int Y, int X,
                     int kernel_value);

/* Connected components, 26-connectivity (skimage.measure.label default for 3-D inputs,
 * BCA/body_regions/postprocess.py:9; remove_small_objects(connectivity=3), BCA/body_parts/postprocess.py:43-48)
 * of `mask != 0` by atomic union-find on the device.
 *   roots dev int32 [n]: linear index of the component's first voxel in raster order (= the order in which
 *         skimage numbers components), -1 for background;
 *   sizes dev uint32 [n]: component size stored at the root's index, 0 elsewhere;
 *   host_n_components (optional): number of components. */
int boa_ccl26(boa_ctx* ctx, const uint8_t* dev_mask, int Z, int Y, int X, int32_t* dev_roots, uint32_t* dev_sizes,
              int* host_n_components);
/* _filter_largest_unique_segment (BCA/body_regions/postprocess.py:8-15): every component except the largest
 * (ties: the one numbered first, i.e. smallest root) gets seg = fill_value (255). No-op for <= 1 component. */
int boa_ccl_filter_largest(boa_ctx* ctx, const int32_t* dev_roots, const uint32_t* dev_sizes, size_t n,
                           uint8_t* dev_seg, int fill_value);
/* remove_small_objects(mask, max_size): clear mask where the component has <= max_size voxels. */
int boa_ccl_remove_small(boa_ctx* ctx, const int32_t* dev_roots, const uint32_t* dev_sizes, size_t n,
                         uint32_t max_size, uint8_t* dev_mask_inout);
/* ---- z-slab sharded connected components: per-component tables for the host-side merge over slab interfaces ----
 * boa_ccl_list_components: the (root index, size) pairs of boa_ccl26's result, in no particular order; *host_count is the
 *   true number (may exceed max_out: call again with larger arrays).  Synchronous.
 * boa_scatter_u32: dst[idx[i]] = val[i] (the merged sizes of the components that cross an interface go back into `sizes`,
 *   so that boa_ccl_remove_small decides on the global size).  Synchronous.
 * boa_ccl_fill_unmarked: seg = fill_value on every component whose sizes[root] != mark (_filter_largest_unique_segment when
 *   the largest component was determined globally: its local pieces carry `mark`). */
int boa_ccl_list_components(boa_ctx* ctx, const uint32_t* dev_sizes, size_t n, int max_out, int32_t* host_roots,
                            uint32_t* host_sizes, int* host_count);
int boa_scatter_u32(boa_ctx* ctx, uint32_t* dev_dst, const int32_t* host_idx, const uint32_t* host_val, int m);
int boa_ccl_fill_unmarked(boa_ctx* ctx, const int32_t* dev_roots, const uint32_t* dev_sizes, size_t n, uint32_t mark,
                          uint8_t* dev_seg, int fill_value);
/* Blobs of a label volume, 6-connectivity (scipy.ndimage.label's default structure, as TS/postprocessing.py:13-98 calls it on
 * `data == idx`, label by label): a component is a maximal face-connected set of voxels with the same non-zero value, so ONE
 * labelling of the uint8 volume [D0][D1][D2] (D2 fastest) serves every label (csrc/ccl_labels.hip).
 *   roots dev int32 [n]: linear index of the component's first voxel in raster order (= the order in which scipy numbers the
 *         components of a label), -1 on background;
 *   sizes dev uint32 [n]: component size stored at the root's index, 0 elsewhere;
 *   host_n_components (optional): number of components of all labels; without it the call does not synchronise.
 * D0, D1 <= 65535 and D0 * D1 * D2 < 2^31. */
int boa_label_blobs6(boa_ctx* ctx, const uint8_t* dev_labels, int D0, int D1, int D2, int32_t* dev_roots, uint32_t* dev_sizes,
                     int* host_n_components);
/* The blob filters on boa_label_blobs6's result, in place on the volume that was labelled, per label value v by host_mode[v]:
 *   0  leave label v alone;
 *   1  size interval (remove_small_blobs): clear the components with size <= lo or size > hi;
 *   2  keep largest (keep_largest_blob): clear every component of label v but the largest (tie: the smallest root, which is
 *      np.argmax's first).
 * host_mode[0] is ignored.  Voxels that an earlier call cleared stay cleared; the sizes of the remaining components still hold, so
 * several calls may follow one labelling.  lo, hi do not matter without a mode 1. */
int boa_label_blobs_filter(boa_ctx* ctx, const int32_t* dev_roots, const uint32_t* dev_sizes, size_t n, const uint8_t host_mode[256],
                           uint32_t lo, uint32_t hi, uint8_t* dev_labels_inout);
/* mask_out = (labels == value) [mode 0] | (lut-free) labels > 0 [mode 1] | labels in {a,b,c} [mode 2, vals[3]] */
int boa_label_select(boa_ctx* ctx, const uint8_t* dev_labels, size_t n, int mode, const int vals[3],
                     uint8_t* dev_mask_out);

/* remove_small_labeled_objects, slice-wise contour fill (BCA/body_parts/postprocess.py:31-39: per (y,x) slice
 * cv2.findContours(RETR_EXTERNAL) + drawContours(FILLED)): out = mask != 0 OR background pixel that is not 4-connected
 * to the slice border through background.  scratch_i32: dev int32 [n]; scratch_u8: dev uint8 [n]; out must not alias. */
int boa_fill_holes_2d(boa_ctx* ctx, const uint8_t* dev_mask, int Z, int Y, int X, int32_t* dev_scratch_i32,
                      uint8_t* dev_scratch_u8, uint8_t* dev_out);
/* remove_outside_of_mask (TS/postprocessing.py:101-131, `heartchambers_highres`): scipy.ndimage.binary_dilation(mask,
 * iterations) with the default 6-neighbour cross and border_value 0; the caller then clears the labels where the result is
 * 0 (boa_mask_assign with invert = 1).  iterations >= 1; tmp: dev uint8 scratch of the same size; no aliasing. */
int boa_binary_dilate_cross(boa_ctx* ctx, const uint8_t* dev_mask, uint8_t* dev_out, uint8_t* dev_tmp, int Z, int Y, int X,
                            int iterations);
/* `out[filled] = label` (BCA/body_parts/postprocess.py:50): out[i] = value where (mask[i] != 0) != invert. */
int boa_mask_assign(boa_ctx* ctx, const uint8_t* dev_mask, size_t n, int invert, int value, uint8_t* dev_out);
/* ---- bit-mask morphology (csrc/ccl_bits.hip, round 5): the same filters on BIT-PACKED masks, batched over independent masks ----
 * A mask is [Z][Y][W] uint32 words, W = ceil(X / 32), bit i of word w <-> x = 32 w + i (bits beyond X are 0); a batch of M masks is
 * M consecutive masks (boa_bits_words words each).  Replaces, for the BCA post-processing (BCA/body_parts/postprocess.py:7-52,
 * BCA/body_regions/postprocess.py:8-40), the per-label chains of boa_label_select / boa_fill_holes_2d / boa_ccl26 /
 * boa_ccl_remove_small / boa_mask_assign: the per-label passes of remove_small_labeled_objects all read the ORIGINAL mask
 * (`label_mask = mask == label`) and are independent until `out[filled] = label`.  Components are 26-connected; a component's size and
 * first voxel (raster order: the tie-break of the largest-component filter) are those of boa_ccl26.
 *   boa_bits_words          words per mask
 *   boa_bits_select         mask m = { voxel : host_lut[label] bit m } for m < n_masks <= 8, one pass over the uint8 label volume
 *                           (`mask == label`, `seg > 0`, `seg in {a, b, c}` are all such look-ups)
 *   boa_bits_unpack         one mask -> uint8 0 / 1 volume (tests, interop with the byte-mask kernels)
 *   boa_bits_fill_holes_2d  per (mask, z slice): cv2.findContours(RETR_EXTERNAL) + drawContours(FILLED) = foreground + background not
 *                           4-connected to the slice border; in and out may not alias; boa_bits_fill_supported(Y, X) == 0: the slice
 *                           does not fit the LDS flood (use boa_fill_holes_2d on bytes)
 *   boa_bits_remove_small   remove_small_objects(max_size, connectivity = 3) in place on every mask; invert != 0: on the complements
 *                           (np.invert / remove_small_objects / np.invert: small holes are filled)
 *   boa_bits_filter_largest _filter_largest_unique_segment on ONE mask: seg = fill_value outside its largest component
 *   boa_bits_assign_labels  out[v] = host_labels[m] for the largest m whose mask holds v (`out[filled] = label`, ascending); voxels in no
 *                           mask of the batch keep their value: zero `out` first, apply batches of <= 8 labels in ascending order
 *   boa_bits_erode_u8       uint8 mask -> uint8 0 / 1 mask eroded by the box of offsets [lo, hi] per axis (outside the volume counts as
 *                           set): what boa_binary_erode runs (pack, three separable passes on bits, unpack) */
size_t boa_bits_words(int Z, int Y, int X);
int boa_bits_erode_u8(boa_ctx* ctx, const uint8_t* dev_mask, uint8_t* dev_out, int Z, int Y, int X, int lo, int hi);
int boa_bits_select(boa_ctx* ctx, const uint8_t* dev_seg, int Z, int Y, int X, const uint8_t host_lut[256], int n_masks, uint32_t* dev_bits);
int boa_bits_unpack(boa_ctx* ctx, const uint32_t* dev_bits, int Z, int Y, int X, uint8_t* dev_out);
int boa_bits_fill_supported(int Y, int X);
int boa_bits_fill_holes_2d(boa_ctx* ctx, const uint32_t* dev_in, int Z, int Y, int X, int n_masks, uint32_t* dev_out);
int boa_bits_remove_small(boa_ctx* ctx, uint32_t* dev_bits, int Z, int Y, int X, int n_masks, uint32_t max_size, int invert);
int boa_bits_filter_largest(boa_ctx* ctx, const uint32_t* dev_bits, int Z, int Y, int X, uint8_t* dev_seg, int fill_value);
int boa_bits_assign_labels(boa_ctx* ctx, const uint32_t* dev_bits, int Z, int Y, int X, int n_masks, const uint8_t* host_labels, uint8_t* dev_out);
/* the part -> combined merge `seg_combined[seg == jdx] = class_map_inv[name]` (TS/nnunet.py:553-556) on label volumes that
 * already carry global labels: out[i] = part[i] where part[i] != 0 (tile-sharded mode merges after the label exchange). */
int boa_label_overlay(boa_ctx* ctx, const uint8_t* dev_part, size_t n, uint8_t* dev_out);
/* subclassify_tissues(median_filtering=True) (BCA/tissue/subclassification.py:21-36): scipy.ndimage.median_filter
 * with size 3 on two axes and 1 on `flat_axis` (0 = z, 1 = y, 2 = x of the [Z][Y][X] array), mode="reflect". */
int boa_median3_inplane(boa_ctx* ctx, const int16_t* dev_in, int Z, int Y, int X, int flat_axis, int16_t* dev_out);
/* the same selection on float64 values (exact: the result is one of the nine inputs) */
int boa_median3_inplane_f64(boa_ctx* ctx, const double* dev_in, int Z, int Y, int X, int flat_axis, double* dev_out);

/* ------------------------------------------------------------------ index remaps around a task ------- */
/* Strided 3-D gather copy with dtype conversion: the device form of as_closest_canonical / undo_canonical
 * (TS/alignment.py:8-46: axis permutation + flips), crop_to_bbox / undo_crop (TS/cropping.py:41-49,126-132), the
 * (x,y,z) <-> (z,y,x) view change between nibabel and nnU-Net arrays (NN/imageio/nibabel_reader_writer.py:51-56),
 * crop_to_nonzero / insert_crop_into_image, and the z-splits of TS/nnunet.py:495-505,583-586.
 *   out[out_off + sum_k o_k * out_step[k]] = (out type) in[in_off + sum_k o_k * in_step[k]]   for o in [0, dims)
 * Offsets / steps are in elements (steps may be negative).  dtype codes: 0 uint8, 1 int16, 2 int32, 3 float32,
 * 4 float64; float -> integer conversion truncates (numpy astype). */
int boa_copy3(boa_ctx* ctx, const void* dev_in, int in_dtype, long long in_off, const long long in_step[3],
              const int dims[3], void* dev_out, int out_dtype, long long out_off, const long long out_step[3]);
/* Bounding box of data != 0 (crop_to_nonzero, NN/preprocessing/cropping/cropping.py:6-29; binary_fill_holes cannot
 * change it): host_bbox = {lo0, hi0, lo1, hi1, lo2, hi2} with hi exclusive; [0, dim) when all zero.
 * dtype: 0 uint8, 1 int16, 2 int32, 3 float32.  Synchronous. */
int boa_nonzero_bbox(boa_ctx* ctx, const void* dev_in, int dtype, const int dims[3], int host_bbox[6]);

/* ------------------------------------------------------------------ resampling (TS/resampling.py) --- */
/* change_spacing / resample_img order 3 (TS/resampling.py:24-56,129-222): scipy.ndimage.zoom(data, zoom, order=3,
 * mode="nearest") restated in fp64 (edge pad 12, cubic B-spline prefilter with 'reflect' initialisation, 64-tap
 * interpolation, coordinate = out * (n_in - 1) / (n_out - 1)); only the shapes determine the sampling grid.
 * in_dtype: 0 int16, 1 float32, 2 float64, 3 int32; out_dtype: 0 int32 (`.astype(np.int32)` truncation), 1 float64.
 * Every fp64 operation in scipy's order with scipy's constants: bit-identical to scipy 1.15.3 on the golden vectors
 * (tests/golden/g5_resample.npz) including the int32 truncation.  Synchronous (frees its fp64 scratch of (X+24)(Y+24)(Z+24) doubles). */
int boa_resample_cubic(boa_ctx* ctx, const void* dev_in, int in_dtype, const int in_dims[3], void* dev_out, int out_dtype,
                       const int out_dims[3]);
/* order 0 (labels back to the original grid, TS/nnunet.py:685-687): index floor(out * (n_in-1)/(n_out-1) + 0.5). */
int boa_resample_nearest_u8(boa_ctx* ctx, const uint8_t* dev_in, const int in_dims[3], uint8_t* dev_out,
                            const int out_dims[3]);
/* higher_order_resampling (labels back to the original grid with nnunet_resample=True, TS/nnunet.py:670-683 ->
 * TS/resample_nnunet.py:11-33,119-205): nnU-Net's one-hot resampling of a label volume in one pass.  The reference resizes the
 * 0/1 mask of every label with order 1 (skimage.transform.resize(mode="edge", anti_aliasing=False), restated as for
 * boa_resize_skimage_f32: scipy.ndimage.zoom(grid_mode=True, mode="nearest"), fp64) and writes the label where the result is
 * >= 0.5, labels ascending, later ones overwriting.  Here every output voxel gathers its (at most) 8 taps, sums per distinct
 * label the fp64 tap weights 1.0 * w * w * w in scipy's tap order and keeps the LARGEST label whose sum is >= 0.5, else 0 -- the
 * same fp64 values, so exact ties at 0.5 (integer zoom factors) decide as in the reference.  Bit-identical to the per-label loop
 * (tests/onehot_reference.py) for any number of labels.
 *   dev_in / dev_out  uint8 [d0][d1][d2], d2 fastest: (x, y, z) of the model-grid / input-grid image.  The reference works on the
 *                     transposed array [z, x, y] (TS/resampling.py:105-125); the taps are visited in ITS axis order (d2 outermost,
 *                     then d0, then d1).  in_dims / out_dims and sep_axis number the axes in memory order.
 *   sep_axis          -1: one 3-D resize.  0..2 ("separate z"): every slice along that axis is resized in 2-D (4 taps) and the
 *                     axis itself is sampled nearest, floor(cc + 0.5) clamped (map_coordinates order 0); the identity when its
 *                     extent does not change.
 * in_dims == out_dims copies ("no resampling necessary").  dev_in and dev_out must not alias.  Asynchronous on the context's
 * stream (its table of d0 + d1 output entries comes from and goes back to the context's pool). */
int boa_resample_onehot_u8(boa_ctx* ctx, const uint8_t* dev_in, const int in_dims[3], uint8_t* dev_out, const int out_dims[3],
                           int sep_axis);


/* ------------------------------------------------------------------ nnU-Net's own resampling to / from the plans' spacing --- */
/* resampling_fn_data (NN/preprocessing/preprocessors/default_preprocessor.py:82-93 -> NN/preprocessing/resampling/
 * default_resampling.py:113-196, is_seg False, order 3, order_z 0): skimage.transform.resize(mode="edge",
 * anti_aliasing=False, clip=True) restated from its published algorithm (scipy.ndimage.zoom(grid_mode=True,
 * mode="nearest") + clip to the input's range; skimage itself is absent from the build image: unpinned) in fp64, result
 * cast to float32.  slice_axis = -1: one 3-D resize; 0..2 ("separate z", anisotropic spacing): every slice along that axis
 * is resized in 2-D (clip range per slice) and the axis itself is sampled nearest (map_coordinates order 0) when its
 * extent changes.  in / out: dev fp32 [d0][d1][d2].  Synchronous (frees its fp64 scratch). */
int boa_resize_skimage_f32(boa_ctx* ctx, const float* dev_in, const int in_dims[3], float* dev_out, const int out_dims[3],
                           int order, int slice_axis);
/* resampling_fn_probabilities + argmax (NN/inference/export_prediction.py:25-47): the (fold-mean) fp16 logits
 * [C][grid_dims], of which the box crop_off / crop_dims is the network's output for the resampled image (pad_nd_image
 * reverted), are resampled with order 1 to out_dims (slice_axis as above), rounded to fp16 (the reference's result array
 * has the logits' dtype) and reduced with numpy's argmax semantics; lut / merge as boa_finalize_labels.  The [C][out_dims]
 * tensor is never materialised.  (skimage's clip is a no-op for order 1 up to one fp64 rounding and is not applied.) */
int boa_resize_logits_argmax(boa_ctx* ctx, const uint16_t* dev_logits, int C, const int grid_dims[3], const int* crop_off,
                             const int* crop_dims, const int out_dims[3], int slice_axis, const uint8_t* host_lut, int merge,
                             uint8_t* dev_labels_out);

/* convert_predicted_logits_to_segmentation_with_correct_shape(..., return_probabilities=True)
 * (NN/inference/export_prediction.py:14-71) in one pass: the (fold-mean) fp16 logits [C][grid_dims] -- as boa_finalize_labels
 * (write_logits = 1) or its fold mean leave them -- become fp32 class probabilities and, optionally, the labels taken from them.
 *   crop_off / crop_dims   the network's output for the image (pad_nd_image reverted); NULL = the whole grid
 *   out_dims, slice_axis   resampling_fn_probabilities (:25-33) of that box to out_dims: order 1, fp16-rounded, the arithmetic of
 *                          boa_resize_logits_argmax; NULL or equal to the box: the logits are taken as they are
 *   apply_inference_nonlin (NN/utilities/label_handling/label_handling.py:128-141): logits.float(), softmax over the classes in fp32:
 *                          m = max, e_c = expf(x_c - m), s = sum in ascending class order, p_c = e_c / s (csrc/softmax_codes.h);
 *                          |p - p64| <= (C + 110) 2^-24 p64 where p64 > 2^-100, else <= 2^-99
 *   labels                 convert_probabilities_to_segmentation (:144-183): the first class whose p equals the maximum p (the argmax
 *                          of the probabilities, not of the logits), through host_lut (uint8[256], NULL = identity)
 *   bbox_lo / full_dims    revert_cropping_on_probabilities (:197-220): the box goes to bbox_lo of the pre-crop grid full_dims;
 *                          outside it p_0 = 1, p_c = 0 for c > 0 and the label is lut[0]
 *   perm                   transpose_backward on the spatial axes (export_prediction.py:56-58, numpy's transpose): output axis i is
 *                          axis perm[i] of the pre-crop grid.  The identity (every shipped plan) without resampling is the fast
 *                          path: one coalesced read per class plane, full-line stores; any other perm, and the resampled form, take a
 *                          plain kernel of one thread per output voxel.
 *   dev_prob               fp32 [C][full_dims permuted]; dev_labels: uint8 [full_dims permuted] or NULL
 * A NaN logit gives NaN probabilities at that voxel and label lut[0]; +-65504, subnormals and equal columns are ordinary inputs (the
 * caller has raised on inf).  BOA_EINVAL before anything is launched: C outside 1..255, a box that leaves its grid, perm not a
 * permutation, slice_axis outside -1..2, an extent below 1 or a class plane of 2^31 voxels or more.  Asynchronous on the context's
 * stream. */
int boa_logits_to_probabilities(boa_ctx* ctx, const uint16_t* dev_logits, int C, const int grid_dims[3], const int* crop_off,
                                const int* crop_dims, const int* out_dims, int slice_axis, const int bbox_lo[3],
                                const int full_dims[3], const int perm[3], float* dev_prob, const uint8_t* host_lut,
                                uint8_t* dev_labels);

/* ------------------------------------------------------------------ several GPUs on one volume (RCCL) -- */
/* The tile-sharded sliding window (boa_hip/tile_shard.py): ranks own blocks of tile rows of the sliding window
 * (NN/inference/predict_from_raw_data.py:523-558 orders the tiles axis 0 outermost; :611-614 adds them one after the other into
 * fp16 buffers) and exchange the partial sums of the planes where two blocks overlap.  The reference has no counterpart (one
 * device per process); these entry points carry its accumulate loop across devices.  RCCL is resolved at run time (dlopen;
 * $BOA_RCCL_LIB overrides the search), collectives run on a communication stream of the boa_comm that is ordered against the
 * context's compute stream by events: boa_comm_* calls queue work and return, boa_comm_wait makes LATER compute work wait for
 * what has been queued (no host synchronisation anywhere).
 *   boa_comm_unique_id : ncclGetUniqueId on one rank; the 128 bytes reach the other ranks out of band (launcher / store)
 *   boa_comm_create    : ncclCommInitRank (collective over all ranks)
 *   boa_comm_shift_slab: planes [send_lo, send_hi) of the C class planes of `acc` + of `nacc` (fp16 [.][PV0][PV1][PV2]: one
 *                        contiguous run per class, sent in place) -> rank dst; planes [recv_lo, recv_hi) <- rank src, written in
 *                        place (recv_stage NULL: the exact hand-over, the receiver has not added anything there yet) or into
 *                        recv_stage [(C + 1)][planes][PV1 PV2] for boa_add_f16_planes (the pairwise fp16 sum).  dst / src < 0: none
 *   boa_comm_exchange  : generic grouped send / recv of byte ranges (pieces matched in order)
 *   boa_comm_planes_to_owner: plane ranges of the C class planes of fp16 logits [C][PV0][PV1][PV2] to / from SEVERAL peers, in place:
 *                        message i of the send list = planes [send_lo[i], send_hi[i]) of every class -> rank send_peer[i], likewise the
 *                        receive list (disjoint from what this rank keeps).  The reduce-scatter of plane-disjoint fold logits
 *                        (predict_from_raw_data.py:494-500 adds the folds; every rank only finalises its own plane share): each plane
 *                        travels once, to the rank that finalises it -- half the per-link bytes of the all-reduce.  Classes go out in
 *                        sub-groups whose size depends on $BOA_COMM_GROUP and the world size only, so all ranks walk the same groups
 *   boa_comm_all_reduce: in-place sum over all ranks; dtype 0 uint8, 1 fp16, 2 int32, 3 fp32 (label volumes with disjoint
 *                        supports: TS/nnunet.py:553-556 merges the parts afterwards; inf flags; plane-disjoint logits) */
typedef struct boa_comm boa_comm;
int boa_comm_available(void);
const char* boa_comm_library(void);
int boa_comm_unique_id(unsigned char id_out[128]);
int boa_comm_create(boa_ctx* ctx, int world, int rank, const unsigned char id[128], boa_comm** out);
void boa_comm_destroy(boa_comm* comm);
int boa_comm_wait(boa_comm* comm);
int boa_comm_exchange(boa_comm* comm, int dst, const void* const* send_ptrs, const size_t* send_bytes, int n_send, int src,
                      void* const* recv_ptrs, const size_t* recv_bytes, int n_recv);
int boa_comm_shift_slab(boa_comm* comm, int dst, int send_lo, int send_hi, int src, int recv_lo, int recv_hi, uint16_t* dev_acc,
                        uint16_t* dev_n, int C, const int PV[3], uint16_t* recv_stage);
int boa_comm_all_reduce(boa_comm* comm, void* dev, size_t count, int dtype);
int boa_comm_planes_to_owner(boa_comm* comm, uint16_t* dev_logits, int C, const int PV[3], int n_send, const int* send_peer,
                             const int* send_lo, const int* send_hi, int n_recv, const int* recv_peer, const int* recv_lo,
                             const int* recv_hi);
int boa_comm_stats(boa_comm* comm, long long* calls, long long* bytes);
/* acc[k][lo:hi] = half(float(acc[k][lo:hi]) + float(stage[k])), k = 0 .. C (C = the n plane): the owner's side of the pairwise
 * fp16 sum of a slab ("allreduce" exchange mode) */
int boa_add_f16_planes(boa_ctx* ctx, uint16_t* dev_acc, uint16_t* dev_n, const uint16_t* dev_stage, int C, const int PV[3], int lo, int hi);

/* ------------------------------------------------------------------ JPEG Lossless decode (jpeg_ll.hip) --- */
/* DICOM transfer syntaxes 1.2.840.10008.1.2.4.57 / .70 = ITU T.81 Process 14, one component.  The host parses the markers,
 * removes the byte stuffing and the RSTn markers (boa_hip/jpeg_lossless.py) and passes, all as HOST arrays:
 *   frames  int32 [n_frames][BOA_LJ_FRAME_WORDS]: fields BOA_LJ_F_* (byte offset of the frame's un-stuffed entropy-coded data
 *           in dev_data: 4-aligned, its bytes padded to a multiple of 4 inside the buffer; restart rows 0 = no restart interval);
 *           every frame of a batch has the same rows x cols;
 *   segs    int32 [n_segs][4]: one per restart interval of each frame, in frame order: start byte, end byte (relative to the
 *           frame), first row (= k x restart rows), index of its first subsequence;
 *   subs    int32 [n_subs][2]: the split of every segment for the parallel decode: start byte (relative to the frame; the first
 *           one = the segment's start, then strictly increasing below its end), segment index;
 *   tables  uint32 [n_tables][BOA_LJ_TABLE_WORDS]: a DHT table expanded for lookup: words 0-255 = 512 uint16 entries
 *           (len << 8 | SSSS) indexed by the next 9 stream bits, 0 where the code is longer; words 256-273 = maxcode[l]
 *           (int32, -1 when no code has l bits), 274-291 = valoff[l] (huffval index of code c of length l = valoff[l] + c),
 *           292-355 = huffval bytes (little-endian packed).
 * Decodes the whole batch in one launch (serial = 0: one workgroup per frame, parallel entropy decode; serial = 1: one lane
 * per frame, the sequential T.81 decoder) into dev_out uint16 [n_frames][rows][cols] (sample << Pt, modulo 2^16) and returns
 * the per-frame status (BOA_LJ_OK / _TRUNCATED / _INVALID_CODE / _TRAILING_GARBAGE) in host_status.  Every offset is
 * validated on the host first (BOA_EINVAL); malformed streams are reported per frame, never by a fault.  Synchronous. */
#define BOA_LJ_FRAME_WORDS 16
#define BOA_LJ_F_OFF_LO 0
#define BOA_LJ_F_OFF_HI 1
#define BOA_LJ_F_LEN 2
#define BOA_LJ_F_ROWS 3
#define BOA_LJ_F_COLS 4
#define BOA_LJ_F_P 5
#define BOA_LJ_F_PT 6
#define BOA_LJ_F_PRED 7
#define BOA_LJ_F_RESTART_ROWS 8
#define BOA_LJ_F_TABLE 9
#define BOA_LJ_F_SEG_FIRST 10
#define BOA_LJ_F_N_SEG 11
#define BOA_LJ_F_SUB_FIRST 12
#define BOA_LJ_F_N_SUB 13
#define BOA_LJ_TABLE_WORDS 384
#define BOA_LJ_OK 0
#define BOA_LJ_TRUNCATED 1
#define BOA_LJ_INVALID_CODE 2
#define BOA_LJ_TRAILING_GARBAGE 3
int boa_ljpeg_decode(boa_ctx* ctx, const uint8_t* dev_data, size_t data_bytes, int n_frames, const int* frames, int n_segs,
                     const int* segs, int n_subs, const int* subs, int n_tables, const uint32_t* tables, uint16_t* dev_out,
                     int* host_status, int serial);

/* ------------------------------------------------------------------ DCT JPEG decode (jpeg_dct.hip) --- */
/* DICOM transfer syntaxes 1.2.840.10008.1.2.4.50 / .51 = ITU T.81 sequential DCT (baseline Process 1, extended Process 2 / 4),
 * Huffman, one component, P = 8 or 12, decoded to the pixels libjpeg gives by default (JDCT_ISLOW).  The host parses the markers,
 * removes the byte stuffing and the RSTn markers (boa_hip/jpeg_dct.py) and passes, all as HOST arrays:
 *   frames  int32 [n_frames][BOA_JD_FRAME_WORDS]: fields BOA_JD_F_* (byte offset of the frame's un-stuffed entropy-coded data
 *           in dev_data: 4-aligned, its bytes padded to a multiple of 4 inside the buffer; restart interval in blocks, 0 = none;
 *           indices of its DC and AC tables in `tables` and of its quantisation table in `qtables`); every frame is rows x cols,
 *           = ceil(rows / 8) x ceil(cols / 8) blocks in raster order (one MCU is one 8 x 8 block);
 *   segs    int32 [n_segs][4]: one per restart interval of each frame, in frame order: start byte, end byte (relative to the
 *           frame), first block (= k x restart interval), index of its first subsequence;
 *   subs    int32 [n_subs][2]: the split of every segment for the parallel decode, as for boa_ljpeg_decode;
 *   tables  uint32 [n_tables][BOA_LJ_TABLE_WORDS]: DHT tables of either class expanded as for boa_ljpeg_decode (a value is the
 *           DC table's SSSS or the AC table's RRRRSSSS byte);
 *   qtables uint16 [n_qtables][64]: quantisation tables in natural (row-major) order.
 * Decodes the batch (serial = 0: one workgroup per frame, parallel entropy decode; serial = 1: one lane per frame, the loop of
 * T.81 F.2.2), then dequantises and inverse-transforms every block, into dev_out uint16 [n_frames][rows][cols], and returns the
 * per-frame status (BOA_JD_OK / _TRUNCATED / _INVALID_CODE / _RUN_PAST_BLOCK / _BAD_SSSS / _TRAILING) in host_status; the
 * blocks of a failed frame that were not reached decode as zero coefficients.  The coefficient workspace (2 B per padded sample)
 * is capped at 1 GiB (BOA_JDCT_WS_KB KiB where that variable is set): longer series decode in chunks of frames inside the call.
 * Every offset is validated on the host first (BOA_EINVAL); malformed streams are reported per frame, never by a fault.
 * Synchronous. */
#define BOA_JD_FRAME_WORDS 16
#define BOA_JD_F_OFF_LO 0
#define BOA_JD_F_OFF_HI 1
#define BOA_JD_F_LEN 2
#define BOA_JD_F_P 3
#define BOA_JD_F_RESTART 4
#define BOA_JD_F_DC_TABLE 5
#define BOA_JD_F_AC_TABLE 6
#define BOA_JD_F_QTABLE 7
#define BOA_JD_F_SEG_FIRST 8
#define BOA_JD_F_N_SEG 9
#define BOA_JD_F_SUB_FIRST 10
#define BOA_JD_F_N_SUB 11
#define BOA_JD_OK 0
#define BOA_JD_TRUNCATED 1
#define BOA_JD_INVALID_CODE 2
#define BOA_JD_RUN_PAST_BLOCK 3
#define BOA_JD_BAD_SSSS 4
#define BOA_JD_TRAILING 5
int boa_jdct_decode(boa_ctx* ctx, const uint8_t* dev_data, size_t data_bytes, int n_frames, const int* frames, int rows, int cols,
                    int n_segs, const int* segs, int n_subs, const int* subs, int n_tables, const uint32_t* tables, int n_qtables,
                    const uint16_t* qtables, uint16_t* dev_out, int* host_status, int serial);

/* ------------------------------------------------------------------ JPEG 2000 decode (j2k.hip) --- */
/* DICOM transfer syntaxes 1.2.840.10008.1.2.4.90 / .91 holding a reversible (5/3) or an irreversible (9/7, scalar quantisation)
 * stream, ITU T.800, one component, one tile, code-block style 0.  The host parses the codestream and runs tier-2 (boa_hip/jpeg2000.py) and passes, as HOST arrays:
 *   frames  int32 [n_frames][BOA_J2K_FRAME_WORDS]: fields BOA_J2K_F_* (sample offset of the frame's output in dev_out: frames
 *           packed in order, each rows x cols; decomposition levels; precision P 1..16; signed 0 / 1; its range of blocks:
 *           blocks grouped by frame, in frame order; the wavelet transform, BOA_J2K_T_97 or BOA_J2K_T_53: the value of the COD
 *           field); frames of a batch may differ in size, levels, precision and transform;
 *   blocks  int32 [n_blocks][BOA_J2K_BLOCK_WORDS]: fields BOA_J2K_B_* (frame; orientation 0 LL, 1 HL, 2 LH, 3 HH; x0, y0, w, h:
 *           the block's place in the frame's coefficient plane, Mallat layout, w x h at most 4096; magnitude bit-planes
 *           Mb - zero bit-planes; coding passes, the first a cleanup pass on the most significant plane; byte offset and length
 *           of its data in dev_data, the contributions of all layers concatenated; in a 9/7 frame BOA_J2K_B_STEP, the float32 bits of
 *           half the subband's quantisation step, 0.5f * (1 + mu_b / 2048) 2^(P - eps_b), finite and positive).
 * Runs tier-1 of every block in one launch per chunk of frames (chunks keep the workspace below 1 GiB), then the inverse 5/3
 * or the inverse 9/7 (dequantisation, transform and rounding in OpenJPEG's float32 arithmetic, csrc/j2k_dwt97.h: the pixels
 * are OpenJPEG's) with the DC level shift, into dev_out uint16 (the sample clamped to its P-bit range, modulo 2^16), and returns the per-frame
 * status (BOA_J2K_OK / _INVALID: a block with more passes than its bit-planes allow, or beyond 30 bit-planes) in host_status.
 * A block with fewer than 3 x bit-planes - 2 passes (a stream truncated by its layers; none is valid too) is reconstructed as
 * OpenJPEG does: a significant coefficient coded down to plane b >= 1 gets 2^(b - 1) added to its magnitude (the midpoint).
 * Every field is validated on the host first (BOA_EINVAL); malformed streams are reported per frame, never by a fault.
 * Synchronous. */
#define BOA_J2K_FRAME_WORDS 12
#define BOA_J2K_F_OUT_LO 0
#define BOA_J2K_F_OUT_HI 1
#define BOA_J2K_F_ROWS 2
#define BOA_J2K_F_COLS 3
#define BOA_J2K_F_LEVELS 4
#define BOA_J2K_F_P 5
#define BOA_J2K_F_SIGNED 6
#define BOA_J2K_F_BLOCK_FIRST 7
#define BOA_J2K_F_N_BLOCKS 8
#define BOA_J2K_F_TRANSFORM 9
#define BOA_J2K_T_97 0
#define BOA_J2K_T_53 1
#define BOA_J2K_BLOCK_WORDS 12
#define BOA_J2K_B_FRAME 0
#define BOA_J2K_B_ORIENT 1
#define BOA_J2K_B_X0 2
#define BOA_J2K_B_Y0 3
#define BOA_J2K_B_W 4
#define BOA_J2K_B_H 5
#define BOA_J2K_B_NUMBPS 6
#define BOA_J2K_B_PASSES 7
#define BOA_J2K_B_OFF_LO 8
#define BOA_J2K_B_OFF_HI 9
#define BOA_J2K_B_LEN 10
#define BOA_J2K_B_STEP 11
#define BOA_J2K_OK 0
#define BOA_J2K_INVALID 1
int boa_j2k_decode(boa_ctx* ctx, const uint8_t* dev_data, size_t data_bytes, int n_frames, const int* frames, int n_blocks,
                   const int* blocks, uint16_t* dev_out, int* host_status);

/* ------------------------------------------------------------------ RLE Lossless decode (rle.hip) --- */
/* DICOM transfer syntax 1.2.840.10008.1.2.5 = PS3.5 Annex G: every byte plane of a frame's samples is one PackBits stream (a
 * segment), the most significant plane first.  The host reads the 64-byte RLE header of every frame (boa_hip/rle_lossless.py) and
 * passes, as a HOST array:
 *   frames  int32 [n_frames][BOA_RLE_FRAME_WORDS]: fields BOA_RLE_F_* (byte offset and length of the frame in dev_data, no
 *           alignment asked; 1 or 2 segments = 8- or 16-bit samples; per segment its first byte and the byte behind its last,
 *           relative to the frame); every frame of a batch has rows x cols samples, frames of 1 and of 2 segments may be mixed.
 * Decoding rule, per segment: control byte c < 128 copies the next c + 1 bytes, c > 128 repeats the next byte 257 - c times,
 * c == 128 does nothing; the decode stops when rows x cols bytes are produced (a run that crosses that count is clipped, whatever
 * follows is ignored) or at the first control whose operand bytes are not all inside the segment (it produces nothing); fewer
 * bytes than rows x cols = BOA_RLE_TRUNCATED for the frame, whose samples are then unspecified.  Runs may cross row ends.
 * serial = 0: every segment is cut into chunks of chunk_bytes (a power of two in 256 .. 4096); the chunks are mapped, chained and
 * expanded in parallel (rle.hip); serial = 1: one lane per segment, the plain loop.  Both write byte planes that one more kernel
 * interleaves into dev_out uint16 [n_frames][rows][cols] (plane 0 = the high byte; a frame of one segment is widened).  Batches
 * whose workspace (two planes per frame, 129 + 2 words per chunk) would pass 1 GiB (or BOA_RLE_WS_MB MiB, where that
 * environment variable holds a positive number) are decoded in groups of frames within the call.  Every offset is validated on the host first (BOA_EINVAL); malformed streams are reported per frame in host_status,
 * never by a fault.  Synchronous. */
#define BOA_RLE_FRAME_WORDS 8
#define BOA_RLE_F_OFF_LO 0
#define BOA_RLE_F_OFF_HI 1
#define BOA_RLE_F_LEN 2
#define BOA_RLE_F_N_SEG 3
#define BOA_RLE_F_SEG 4          /* then [segment][first byte, end byte] */
#define BOA_RLE_OK 0
#define BOA_RLE_TRUNCATED 1
int boa_rle_decode(boa_ctx* ctx, const uint8_t* dev_data, size_t data_bytes, int n_frames, const int* frames, int rows, int cols,
                   int chunk_bytes, uint16_t* dev_out, int* host_status, int serial);

/* ------------------------------------------------------------------ JPEG-LS decode (jls.hip) --- */
/* DICOM transfer syntaxes 1.2.840.10008.1.2.4.80 / .81 = ITU-T T.87, one component, no interleaving, no restart interval, no
 * mapping table.  The host reads the markers of every frame (boa_hip/jpeg_ls.py) and passes, as a HOST array:
 *   frames  int32 [n_frames][BOA_JLS_FRAME_WORDS]: fields BOA_JLS_F_* (byte offset, a multiple of 4, and length of the frame's
 *           scan in dev_data, whose bytes up to the next multiple of 4 behind the scan must lie inside dev_data; the coding
 *           parameters MAXVAL, NEAR, T1, T2, T3, RESET with the defaults resolved, in the ranges of T.87 C.2.4.1.1); every frame
 *           of a batch has rows x cols samples, the parameters may differ from frame to frame.
 * Decoding rule: the scan is read most significant bit first; after a 0xFF byte the next byte carries 7 bits, and a byte >= 0x80
 * there is a marker that ends the stream; behind the end zero bits are read.  Samples are decoded in raster order as T.87 Annex A
 * lays down (the first row sees zeros above it; Ra at a row's start is Rb, Rc there is the row above's starting Ra, Rd at a
 * row's end is Rb; RUNindex persists over the rows; a run that reaches the row's end has no interruption sample).  A Golomb code
 * with more zeros than its limit allows, a mapped error above RANGE or a run that passes the row's end end the frame with
 * BOA_JLS_INVALID; a frame whose decoding took a bit from behind the stream's end is BOA_JLS_TRUNCATED instead (also where it
 * met an invalid code there).  The samples of a failed frame are unspecified; bytes behind the last sample's code are ignored.
 * serial = 0: one wave per frame (k_jls_wave: the chain on wave-uniform values, the other lanes on what the row above decides,
 * the run fills and the stores; rows up to BOA_JLS_WAVE_MAX_COLS samples, wider frames take the other path); serial = 1: one
 * lane per frame, the plain loop (k_jls_serial).  dev_out: uint16 [n_frames][rows][cols].  Every range is validated on the host
 * first (BOA_EINVAL); malformed scans are reported per frame in host_status, never by a fault.  Synchronous. */
#define BOA_JLS_FRAME_WORDS 16
#define BOA_JLS_F_OFF_LO 0
#define BOA_JLS_F_OFF_HI 1
#define BOA_JLS_F_LEN 2
#define BOA_JLS_F_MAXVAL 3
#define BOA_JLS_F_NEAR 4
#define BOA_JLS_F_T1 5
#define BOA_JLS_F_T2 6
#define BOA_JLS_F_T3 7
#define BOA_JLS_F_RESET 8
#define BOA_JLS_WAVE_MAX_COLS 4096
#define BOA_JLS_OK 0
#define BOA_JLS_TRUNCATED 1
#define BOA_JLS_INVALID 2
int boa_jls_decode(boa_ctx* ctx, const uint8_t* dev_data, size_t data_bytes, int n_frames, const int* frames, int rows, int cols,
                   uint16_t* dev_out, int* host_status, int serial);

/* ------------------------------------------------------------------ deflate encoder for label volumes (deflate.hip) --- */
/* The data body of a .nii.gz label volume as raw deflate streams (RFC 1951), one per gzip member (RFC 1952), encoded on the
 * device.  dev_src: n payload bytes in file order.  The payload is cut into members of member_bytes (1 .. 2^30; the last may be
 * shorter; n == 0 is one member whose body is the empty final fixed block, 03 00), every member into deflate blocks of 16 KiB of
 * input.  Each block is parsed greedily against two candidates per position, distance 1 (a run) and distance row_bytes (the
 * voxel one x-row back; row_bytes outside 1 .. 32768 = no row candidate), matches of 3 .. 258 bytes that neither reach before
 * the member's first byte nor past the block's last, and written with the fixed Huffman codes (BTYPE = 01), or as a stored block
 * (BTYPE = 00) where that is not larger.  Non-final blocks are byte-aligned by an empty stored block; the last block of a member
 * has BFINAL = 1 and is padded to a byte, so every member inflates on its own.
 * Output: the bodies packed back to back in dev_out, member m at [host_offsets[m], host_offsets[m + 1]) (n_members + 1 entries,
 * n_members = max(1, ceil(n / member_bytes))), and host_crc32[m] = the CRC-32 (RFC 1952 section 8) of member m's payload,
 * computed on the device.  out_capacity must be at least boa_deflate_bound(n, member_bytes) (every block stored: n + 5 bytes per
 * block; 0 for sizes boa_deflate_members rejects), else BOA_EINVAL before anything is launched.  Deterministic.  Synchronous. */
size_t boa_deflate_bound(size_t n, size_t member_bytes);
int boa_deflate_members(boa_ctx* ctx, const uint8_t* dev_src, size_t n, size_t member_bytes, int row_bytes, uint8_t* dev_out,
                        size_t out_capacity, size_t* host_offsets, uint32_t* host_crc32);
/* The same with two more choices; boa_deflate_members is this call with near_bytes = 1, flags = 0.
 * near_bytes (1 .. 16): the short candidate distance, the item size of the voxels (a tie between the candidates goes to it).
 * flags = BOA_DEFLATE_DYNAMIC: every block is also sized as a dynamic-Huffman block (BTYPE = 10) over the same tokens: the
 * literal/length and distance symbols are counted, each alphabet gets the code lengths of least cost within 15 bits (7 bits for
 * the code-length code of the header: package-merge, so the cost is the optimum also where the Huffman tree would be deeper), the
 * lengths are run-length coded by zlib's greedy rule (zero runs of 11 .. 138 -> 18, of 3 .. 10 -> 17, a non-zero length once and
 * its repeats in groups of 3 .. 6 -> 16, the rest literally; one sequence over both alphabets), HLIT / HDIST / HCLEN end at the last
 * used symbol; a block without a match has HDIST = 1 with a zero length, one with a single distance symbol a 1-bit code.  The
 * block is written in that form only where it is smaller than both the fixed and the stored form, so boa_deflate_bound holds.
 * near_bytes outside 1 .. 16, near_bytes other than 1 without BOA_DEFLATE_DYNAMIC (the fixed-code kernel is the one it was, with
 * distance 1) or an unknown flag bit: BOA_EINVAL before anything is launched. */
#define BOA_DEFLATE_DYNAMIC 1
int boa_deflate_members2(boa_ctx* ctx, const uint8_t* dev_src, size_t n, size_t member_bytes, int row_bytes, int near_bytes, int flags,
                         uint8_t* dev_out, size_t out_capacity, size_t* host_offsets, uint32_t* host_crc32);

/* ---- per-structure mask files of a label volume (label_masks.hip, deflate.hip) ----
 * One binary mask file per structure is the payload (labels == k) ? 1 : 0 for every k, cut into the same members.  A structure fills
 * a small part of the volume, so most (label, member) pairs are all zero: the presence pass finds the others, and only those are
 * encoded, straight from the label volume -- the mask bytes exist in LDS only.
 *
 * boa_label_member_presence: host_bits = n_members rows of 8 words, n_members = max(1, ceil(n / member_bytes)) as above; bit k of row m
 * (word k / 32, bit k % 32) = label k occurs in bytes [m member_bytes, (m + 1) member_bytes) of dev_labels.  member_bytes 1 .. 2^30,
 * any alignment of dev_labels; n == 0 gives one all-zero row.  One pass, deterministic, synchronous. */
int boa_label_member_presence(boa_ctx* ctx, const uint8_t* dev_labels, size_t n, size_t member_bytes, uint32_t* host_bits);
/* boa_deflate_label_pairs: pair p = (host_pair_label[p], host_pair_member[p]) yields the raw deflate body and the CRC-32 of the payload
 * (dev_labels[i] == label) ? 1 : 0 over that member: body p at [host_offsets[p], host_offsets[p + 1]) of dev_out (n_pairs + 1 entries),
 * byte for byte what boa_deflate_members2(mask, n, member_bytes, row_bytes, 1, flags, ..) yields for the member on the materialised
 * mask.  Any pair may be listed, in any order, present or not, more than once.  The launch covers the blocks of the listed pairs
 * only.  BOA_EINVAL before anything is launched: out_capacity below the sum over the pairs of (member length + 5 bytes per 16 KiB
 * block of it; at least one block: boa_deflate_bound(member length, member length), 5 for the empty payload), a member index at or
 * beyond n_members, an unknown flag bit, n_pairs < 0.  n_pairs == 0 returns BOA_OK with host_offsets[0] = 0 and launches nothing.
 * Deterministic.  Synchronous. */
int boa_deflate_label_pairs(boa_ctx* ctx, const uint8_t* dev_labels, size_t n, size_t member_bytes, int row_bytes, int flags,
                            const uint8_t* host_pair_label, const uint32_t* host_pair_member, int n_pairs, uint8_t* dev_out,
                            size_t out_capacity, size_t* host_offsets, uint32_t* host_crc32);

/* ------------------------------------------------------------------ inflate of .nii.gz inputs (inflate.hip) --- */
/* Raw deflate streams (RFC 1951) decoded on the device, each checked against its gzip trailer (RFC 1952).  A stream is one member's
 * body: stream_off[m] / stream_len[m] = its place in dev_src (src_bytes), an empty history, stream_size[m] = its payload bytes (the
 * trailer's ISIZE, taken as the whole size) and stream_crc32[m] = the trailer's CRC-32; all HOST arrays of n_streams entries.  The
 * payloads are written back to back into dev_out (out_capacity >= the sum of stream_size).  A file with a member index is many
 * streams, a foreign single-member file is one.
 * Every stream is cut into chunks of chunk_bytes (64 .. 2^30; boa_inflate_default_chunk() = 64 KiB) of compressed input.  Chunk 0
 * starts at bit 0; every other chunk looks for the first bit offset of its range that passes the block-start test (BFINAL = 0,
 * BTYPE = 2, HLIT / HDIST <= 29, a complete code-length code, the lengths decode as one sequence without a leading repeat or an
 * overrun, symbol 256 has a length, both codes complete or incomplete as zlib's inflate_table accepts), and drops out without one.
 * Each live chunk decodes up to the first block end at or beyond the next live chunk's start, counting bytes; the chain is accepted
 * where every end is the next start.  A chunk behind a false candidate is restarted at its predecessor's end, a bounded number of
 * rounds.  The chunks are then decoded into 16-bit symbols (a literal, or a reference into the unknown 32 KiB in front of the
 * chunk), the windows are resolved chunk after chunk, and the symbols become bytes with a CRC-32 per chunk, combined per stream.
 * host_status[m]: BOA_INF_OK, or why the stream was not decoded; with any status other than OK the content of dev_out is undefined
 * and the caller inflates on the host.  host_info[BOA_INF_INFO_WORDS]: BOA_INF_I_*.  host_ms (may be NULL): BOA_INF_MS_WORDS floats,
 * the device-event times of the passes in ms.  Every offset is validated first (BOA_EINVAL), malformed streams are reported per
 * stream, never by a fault: lengths 286 / 287 and distances 30 / 31, a stored block whose LEN is not ~NLEN, a read past the
 * stream's end (zero bits, BOA_INF_TRUNCATED), a distance before the stream's first byte (BOA_INF_FAR).  Synchronous. */
#define BOA_INF_OK 0
#define BOA_INF_TRUNCATED 1
#define BOA_INF_INVALID 2
#define BOA_INF_FAR 3
#define BOA_INF_OVERRUN 4
#define BOA_INF_SIZE 5
#define BOA_INF_CRC 6
#define BOA_INF_REPAIR 7
#define BOA_INF_TRAILING 8
#define BOA_INF_INFO_WORDS 8
#define BOA_INF_I_CHUNKS 0       /* chunks of all streams */
#define BOA_INF_I_CANDIDATES 1   /* block starts the find pass accepted */
#define BOA_INF_I_REJECTED 2     /* candidates the chain check dropped */
#define BOA_INF_I_ROUNDS 3       /* repair rounds */
#define BOA_INF_I_LIVE 4         /* chunks that decoded in the end */
#define BOA_INF_MS_WORDS 8
#define BOA_INF_MS_FIND 0
#define BOA_INF_MS_COUNT 1
#define BOA_INF_MS_STORE 2
#define BOA_INF_MS_WINDOWS 3
#define BOA_INF_MS_RESOLVE 4
size_t boa_inflate_default_chunk(void);
int boa_inflate_streams(boa_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, int n_streams, const uint64_t* stream_off,
                        const uint64_t* stream_len, const uint64_t* stream_size, const uint32_t* stream_crc32, size_t chunk_bytes,
                        uint8_t* dev_out, size_t out_capacity, int* host_status, uint64_t* host_info, float* host_ms);

#ifdef __cplusplus
}
#endif
#endif /* BOA_HIP_H */
