/*
 * dafne_amd.h -- C ABI of libdafne_amd.so, the MI355X (gfx950) replacement for the
 * native pieces of braun-steven/DAFNe's inference path.
 *
 * Conventions (all entry points):
 *   - plain C types only; every pointer named d_* is a DEVICE pointer owned by
 *     the caller; `stream` is a hipStream_t passed as void* (NULL = default stream)
 *   - the library never allocates device memory and never synchronises the
 *     device: work is enqueued on `stream`; scratch comes from the caller through
 *     (d_ws, ws_bytes), sized by the matching *_workspace_bytes() query
 *   - return value: 0 = OK, non-zero = error (DAFNE_E_*); the message is
 *     available from dafne_last_error() (thread-local); nothing throws across
 *     the boundary
 *   - re-entrant: no mutable global state; one call <-> one stream
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   poly_nms.poly_gpu_nms(dets[M,9] f32, thresh, device_id)   dafne/modeling/nms/nms.py:6,91
 *       (external CUDA ext, DOTA_devkit poly_nms_gpu)         -> dafne_poly_nms_hip / _batched
 *   batched_nms_poly's offset arithmetic                      dafne/modeling/nms/nms.py:74-90
 *                                                             -> dafne_select_over_all_levels_hip
 *   select_over_all_levels' kthvalue cap                      dafne/modeling/dafne/dafne_outputs.py:907-925
 *                                                             -> dafne_select_over_all_levels_hip
 *   polyiou.iou_poly (SWIG C++)                               tools/prepare_dota/polyiou.cpp:112
 *                                                             -> dafne_poly_iou_pairs_hip
 *   forward_for_single_feature_map (+ sort_quadrilateral)     dafne/modeling/dafne/dafne_outputs.py:792-905,
 *                                                             dafne/utils/sort_corners.py:26-92
 *                                                             -> dafne_decode_levels_hip
 *   torch conv2d / GroupNorm / max_pool2d / interpolate       dafne/modeling/dafne/dafne.py:209-229,318-344,
 *   (cuDNN through torch) in backbone and head                dafne/modeling/backbone/fpn.py:26-37
 *                                                             -> dafne_conv2d_nhwc_bf16_hip and friends
 */
#ifndef DAFNE_AMD_H
#define DAFNE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAFNE_OK 0
#define DAFNE_E_INVALID 1   /* bad argument (null pointer, negative size, ...) */
#define DAFNE_E_WORKSPACE 2 /* workspace too small */
#define DAFNE_E_HIP 3       /* a HIP runtime call / kernel launch failed */
#define DAFNE_E_UNSUPPORTED 4

/* Library / ABI version: major*10000 + minor*100 + patch. */
int dafne_abi_version(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char* dafne_last_error(void);

/* ---------------------------------------------------------------- polygon IoU */
/*
 * fp64 IoU of n quadrilateral pairs, bit-identical to the reference's
 * polyiou.cpp arithmetic.  d_p, d_q: [n,8] float64 (x0,y0,..,x3,y3); d_out: [n].
 */
int dafne_poly_iou_pairs_hip(const double* d_p, const double* d_q, int64_t n,
                             double* d_out, void* stream);

/* --------------------------------------------------------------- rotated NMS */
/*
 * Tile ResultMerge NMS (dafne/utils/ResultMerge_multi_process.py:61-121 py_cpu_nms_poly_fast, called from
 * nmsbynamedict :160-176 for every original image of a Task1_<class>.txt file; tools/prepare_dota has the
 * same file).  Rows are FLOAT64 [x1..y4, score] exactly as mergesingle builds them ((tile poly + offset) /
 * rate, :217-228); order = argsort(score, stable)[::-1]; row j is dropped iff a kept earlier row i has
 * iou_poly(i, j) > thresh (polyiou.cpp, fp64) AND, when strict_hbb != 0, their axis-aligned hulls pass the
 * reference's `hbb_ovr > 0` test (:80-98).  strict_hbb == 0 gives py_cpu_nms_poly (:24-58).
 * d_dets9 [n_images][m_cap][9] doubles, d_counts [n_images] or NULL (= m_cap rows each); d_keep
 * [n_images][m_cap] original row indices in descending-score order, d_num_keep [n_images].
 */
size_t dafne_poly_nms_f64_workspace_bytes(int n_images, int m_cap);
int dafne_poly_nms_f64_batched_hip(const double* d_dets9, const int32_t* d_counts, int n_images, int m_cap,
                                   double thresh, int strict_hbb, int64_t* d_keep, int32_t* d_num_keep,
                                   void* d_ws, size_t ws_bytes, int flags, void* stream);

/*
 * Horizontal-box NMS of the tile merge for DOTA Task2 (dafne/utils/ResultMerge_multi_process.py:124-155 py_cpu_nms, the NMS
 * mergebyrec :238-248 hands to mergebase; tools/prepare_dota/ResultMerge.py has the same file).  Rows are FLOAT64
 * [x1, y1, x2, y2, score]; area = (x2 - x1 + 1) * (y2 - y1 + 1); for a kept row i and a later row j
 * w = max(0, min(x2_i, x2_j) - max(x1_i, x1_j) + 1), h likewise, inter = w * h, ovr = inter / (area_i + area_j - inter),
 * fp64 in that operation order; j survives iff ovr <= thresh (a NaN suppresses, as np.where(ovr <= thresh) leaves it out).
 * order = argsort(score, stable)[::-1], as dafne_poly_nms_f64_batched_hip.
 * d_dets5 [n_images][m_cap][5] doubles, d_counts [n_images] or NULL (= m_cap rows each); d_keep [n_images][m_cap] original
 * row indices in descending-score order, d_num_keep [n_images].  m_cap <= 65536.
 */
size_t dafne_hbb_nms_f64_workspace_bytes(int n_images, int m_cap);
int dafne_hbb_nms_f64_batched_hip(const double* d_dets5, const int32_t* d_counts, int n_images, int m_cap, double thresh,
                                  int64_t* d_keep, int32_t* d_num_keep, void* d_ws, size_t ws_bytes, void* stream);

/*
 * Greedy polygon NMS, the replacement for poly_nms.poly_gpu_nms (nms.py:91).
 *   d_dets9   [M,9] float32, C-contiguous: 8 corner coordinates + score
 *   thresh    a box is suppressed iff IoU(kept, box) > thresh (fp64 compare)
 *   d_keep    [M] int64 out: indices into d_dets9 of the kept rows, in
 *             descending-score order (equal scores: larger index first, i.e.
 *             np.argsort(kind="stable")[::-1])
 *   d_num_keep  [1] int32 out
 * IoU: fp64 triangle-fan clip of polyiou.cpp on the float32 inputs.
 */
size_t dafne_poly_nms_workspace_bytes(int n_images, int m_cap);
/*
 * `flags` (every NMS entry point takes it, per call; the library holds no mutable global state, so concurrent callers
 * on other threads / streams are unaffected): 0 = default.  DAFNE_NMS_EXACT_ONLY is the parity switch.  The in-model
 * NMS decides `iou_poly > thresh` (polyiou.cpp:112-133 in fp64) and takes three analytic shortcuts on the way, each with
 * a proven margin: a guarded hull-separation pre-filter, an IoU upper bound for convex pairs, and
 * a one-lane geometric clip for pairs far from the threshold.  With DAFNE_NMS_EXACT_ONLY all three are off for THIS
 * call (every pair of every live tile runs the reference-order clip; same results, slower): what tests/test_gpu_nms.py
 * uses to show the shortcuts change nothing.  Unknown bits -> DAFNE_E_INVALID.
 *
 * dafne_poly_nms_stats_offset: byte offset inside the NMS workspace of uint32 stats[n_images][4], valid after a
 * call has completed: pairs decided by (0) the fast path as "suppress", (1) the fast path as "keep", (2) the
 * reference-order path, (3) the reference-order path of tiles that overflowed the pair lists.  f64_rows: 1 for the
 * dafne_poly_nms_f64_* workspace layout.
 */
#define DAFNE_NMS_EXACT_ONLY 1
size_t dafne_poly_nms_stats_offset(int n_images, int m_cap, int f64_rows);
int dafne_poly_nms_hip(const float* d_dets9, int M, double thresh, int64_t* d_keep,
                       int32_t* d_num_keep, void* d_ws, size_t ws_bytes, int flags, void* stream);
/*
 * Batched form: n_images independent problems in one set of launches.
 *   d_dets9   [n_images, m_cap, 9]; d_counts [n_images] int32 DEVICE (rows used
 *             per image, <= m_cap; read on the device, no host sync)
 *   post_topk > 0: after NMS keep only rows whose score >= the post_topk-th
 *             best kept score (dafne_outputs.py:916-923; ties may exceed it)
 *   d_keep    [n_images, m_cap] int64; d_num_keep [n_images] int32
 */
int dafne_poly_nms_batched_hip(const float* d_dets9, const int32_t* d_counts, int n_images,
                               int m_cap, double thresh, int post_topk, int64_t* d_keep,
                               int32_t* d_num_keep, void* d_ws, size_t ws_bytes, int flags, void* stream);
/*
 * ml_nms + the post-NMS cap for a batch (nms.py:10-92, dafne_outputs.py:907-925):
 * class 5 -> 4, offset = float(class) * (max(boxes) - min(boxes) + 1) in fp32 per
 * image, NMS at nms_thresh, then the post_topk cap.
 *   d_boxes8 [n_images, m_cap, 8] f32 (16-byte aligned), d_scores [n_images, m_cap] f32,
 *   d_classes [n_images, m_cap] int32, d_counts [n_images] int32 (device).
 */
int dafne_select_over_all_levels_hip(const float* d_boxes8, const float* d_scores,
                                     const int32_t* d_classes, const int32_t* d_counts,
                                     int n_images, int m_cap, double nms_thresh, int post_topk,
                                     int64_t* d_keep, int32_t* d_num_keep, void* d_ws,
                                     size_t ws_bytes, int flags, void* stream);

/* ------------------------------------------------------ decode / top-k / sort */
typedef struct dafne_level_desc {
    const float* d_logits;  /* [N, H, W, C]  (NHWC == the reference's permuted view) */
    const float* d_delta;   /* [N, H, W, 8]  corners_pred output                      */
    const float* d_center;  /* [N, H, W, 2]  center_pred output                       */
    const float* d_ctrness; /* [N, H, W]     ctrness logits                           */
    /* pixel strides in floats (>= C, 8, 2, 1): lets several predictions share one
     * NHWC buffer, e.g. corners_pred+ctrness written by one fused conv          */
    int32_t logits_ps, delta_ps, center_ps, ctrness_ps;
    int32_t H, W, stride;   /* feature size and FPN stride                            */
    float scale;            /* the level's learnable Scale (dafne.py:405-411)         */
} dafne_level_desc;

typedef struct dafne_decode_params {
    int32_t n_images, n_levels, n_classes;
    int32_t pre_nms_topk;     /* PRE_NMS_TOPK_TEST per level            */
    float pre_nms_thresh;     /* INFERENCE_TH_TEST, strict >            */
    int32_t thresh_with_ctr;  /* THRESH_WITH_CTR                        */
    int32_t sort_corners;     /* SORT_CORNERS                           */
    int32_t m_cap;            /* rows per image in the outputs (>= n_levels*pre_nms_topk) */
    int32_t flags;            /* 0 (released head) or DAFNE_DECODE_* bits below; unknown bits are rejected */
} dafne_decode_params;

/* Heads without a center regression (CORNER_PREDICTION direct / offset / iterative, dafne.py:372-422): corners =
 * delta*scale*stride + location; d_center may be NULL. */
#define DAFNE_DECODE_NO_CENTER 1
/* CENTERNESS none (dafne.py:474-480, dafne_outputs.py:810-830): score = sigmoid(cls), no square root, centerness
 * reported as 1.0, thresh_with_ctr ignored; d_ctrness may be NULL. */
#define DAFNE_DECODE_NO_CTRNESS 2

/*
 * forward_for_single_feature_map for every level and image
 * (dafne_outputs.py:771-772,792-905): sigmoid, sqrt(cls*ctr), threshold, per
 * level top-k, corner decode ((center.repeat+delta)*scale*stride + location;
 * delta*scale*stride + location with DAFNE_DECODE_NO_CENTER),
 * optional canonical corner order, hull box.  Outputs are per image, levels
 * concatenated in order, candidates within a level in (location, class) order:
 *   d_corners [N, m_cap, 8], d_scores [N, m_cap], d_ctr [N, m_cap],
 *   d_classes [N, m_cap] int32, d_locs [N, m_cap, 2], d_levels [N, m_cap] int32,
 *   d_hbox [N, m_cap, 4], d_counts [N] int32.
 */
size_t dafne_decode_workspace_bytes(const dafne_decode_params* prm, const dafne_level_desc* levels);
int dafne_decode_levels_hip(const dafne_decode_params* prm, const dafne_level_desc* levels,
                            float* d_corners, float* d_scores, float* d_ctr, int32_t* d_classes,
                            float* d_locs, int32_t* d_levels, float* d_hbox, int32_t* d_counts,
                            void* d_ws, size_t ws_bytes, void* stream);
/* sort_quadrilateral on [n,8] float32 (sort_corners.py:26-92). */
int dafne_sort_quadrilateral_hip(const float* d_in, float* d_out, int64_t n, void* stream);
/*
 * Gather the kept rows and apply detector_postprocess + OneStageDetector._postprocess
 * (one_stage_detector.py:79-98): hull boxes scaled by out/net-input size, clipped,
 * empty ones dropped; corners and locations scaled by out/orig.  d_sizes:
 * [N,6] float32 = (net_h, net_w, out_h, out_w, orig_h, orig_w) per image.
 * do_postprocess: 0 = plain gather; 1 = d2 detector_postprocess only (hull boxes;
 * what forward(do_postprocess=False) still does); 2 = also rescale corners/locations.
 * Output rows [N, k_cap, DAFNE_DET_ROW] float32 = corners8, score, centerness,
 * class, level, hbox4, loc2 (class/level stored as float); d_out_counts [N].
 * Rows beyond k_cap are dropped and still counted (caller checks count <= k_cap).
 */
#define DAFNE_DET_ROW 18
int dafne_gather_detections_hip(const float* d_corners, const float* d_scores, const float* d_ctr,
                                const int32_t* d_classes, const float* d_locs,
                                const int32_t* d_levels, const float* d_hbox,
                                const int64_t* d_keep, const int32_t* d_num_keep,
                                const float* d_sizes, int do_postprocess, int n_images, int m_cap,
                                int k_cap, float* d_out, int32_t* d_out_counts, void* stream);

/* ------------------------------------------------------------- dense engine */
/*
 * Activations: NHWC bf16 with a zero halo of 1 pixel: [N, H+2, W+2, C]; producers
 * write the interior only, so the halo stays zero and a 3x3 tap never needs a
 * bounds check.  Weights: bf16 [Cout_pad][Cin/64][KH][KW][64] (k = slab, kh, kw, cin%64), rows
 * beyond Cout zero; Cout_pad = dafne_conv2d_cout_pad(Cout).  Bias: fp32 [Cout_pad]
 * (FrozenBN folded into weight scale + bias).
 */
#define DAFNE_CONV_RELU 1u         /* ReLU in the epilogue                              */
#define DAFNE_CONV_RESIDUAL 2u     /* += d_res (same shape as the output) before ReLU   */
#define DAFNE_CONV_UPSAMPLE_ADD 4u /* += nearest-2x upsample of d_res [N,H/2+2,W/2+2,C] */
#define DAFNE_CONV_OUT_F32 8u      /* fp32 un-haloed NHWC output [N,Hout,Wout,Cout]     */
#define DAFNE_CONV_GN_STATS 16u    /* emit per-(M tile, group of 8 ch) sum and sum-sq   */
#define DAFNE_CONV_GN_INPUT 32u    /* GroupNorm + ReLU of the INPUT applied on load (3x3 patch / slab kernels) */
#define DAFNE_CONV_GN_FINALIZE 64u /* with GN_STATS, 3x3 patch-kernel layers with Cout == 256 (kernel id 6): the last tile
                                    * of every image finalises mean / rstd into d_gn_stats_out -- same values, bit for bit, as
                                    * dafne_groupnorm_finalize_hip on d_gn_partial, without the extra launch */
#define DAFNE_CONV_EXCLUSIVE 128u  /* scheduling hint, results unchanged: nothing else runs on the GPU next to this launch (one
                                    * stream, whole batch).  Small launches (<= one 128 x 128 tile per CU) then take the whole
                                    * LDS of their CU for a 4-stage operand ring (K loop without a drain per step); launches of
                                    * plans that share the GPU with other streams keep the small footprint */

#define DAFNE_CONV_FRAG16 256u     /* dafne_conv3x3_c256_hip / _pair_hip only: d_wfrag is in the 16x16x32 fragment order (below) and the
                                    * launch runs on v_mfma_f32_16x16x32_bf16 (cheaper per flop on this package); fp32 sums in another
                                    * order than the 32x32x16 form: <= 1 bf16 ulp apart on an output, run-to-run identical */
#define DAFNE_CONV_RELU_INPUT 512u  /* dafne_conv2d_wr_hip only: ReLU of the INPUT applied on load (per bf16: a set sign bit gives 0, anything
                                    * else is unchanged -- dafne_relu_copy_bf16_hip's definition); bit-identical to that launch
                                    * followed by the plain call */

typedef struct dafne_conv_seg {
    const void* d_in;   /* bf16 [N, Hin+2, Win+2, Cin]; stem: [N, Hin, Win, 4] pre-padded */
    void* d_out;        /* bf16 [N, Hout+2, Wout+2, Cout] or fp32 [N,Hout,Wout,Cout]      */
    const void* d_res;  /* residual / coarser map for UPSAMPLE_ADD, or NULL               */
    int32_t Hin, Win, Hout, Wout;
} dafne_conv_seg;

typedef struct dafne_conv_params {
    int32_t n_images, n_segs;   /* segments share weights (the FPN levels of the head) */
    int32_t Cin, Cout, KH, KW, stride, pad;
    uint32_t flags;
    const void* d_weight;
    const float* d_bias;        /* or NULL */
    float* d_gn_partial;        /* GN_STATS: [num_tiles][Cout/8][2] fp32 */
    /* GN_INPUT: the input maps are the RAW output of the previous tower convolution; GroupNorm(Cin/8
     * groups) + ReLU is applied on load from these statistics (dafne_groupnorm_finalize_hip) */
    const float* d_in_gn_stats; /* [n_segs][n_images][Cin/8][2] mean, rstd */
    const float* d_in_gn_gamma; /* [Cin] */
    const float* d_in_gn_beta;  /* [Cin] */
    /* GN_FINALIZE: */
    float* d_gn_stats_out;      /* [n_segs][n_images][Cout/8][2] mean, rstd of the OUTPUT maps */
    int32_t* d_gn_counters;     /* [n_segs][n_images] int32, zero before the first launch (the kernel resets them) */
    float gn_eps;
} dafne_conv_params;

/*
 * 1x1 (pad 0) and 3x3 (pad 1) convolutions, stride 1 or 2, Cin % 64 == 0; plus the
 * ResNet stem as (Cin=4, 7x7, stride 2) on the image layout that
 * dafne_preprocess_image_hip writes (K = 7 rows x 8 cols x 4 ch, zero weights in
 * the padding taps; weight rows are 256 bf16).
 * Limits per segment (DAFNE_E_UNSUPPORTED beyond them): 2^20 output pixels per image; 2^32 - 1
 * bytes of haloed input over all images, n_images * (Hin+2) * (Win+2) * Cin * 2 (the kernels use
 * 32-bit byte offsets that include the image index), and as many bytes of residual on the
 * streaming 1x1 kernel: split a larger batch.
 */
int dafne_conv2d_nhwc_bf16_hip(const dafne_conv_params* prm, const dafne_conv_seg* segs, void* stream);
/*
 * 3x3 / stride 1 / pad 1 layers with 256 input channels (the DAFNe head towers, dafne.py:318-348, and the FPN output
 * convolutions [d2 FPN recalled]) on the resident-patch kernel (conv3x3_rp_kernel): 4 x 32 pixel tiles x 256 output
 * channels, the whole (4+2) x (32+2) x 256-channel input patch resident in LDS, weights streamed L2 -> registers.
 * Same parameter block, flags (RELU, GN_STATS, GN_INPUT, GN_FINALIZE), statistics layout and result definition as
 * dafne_conv2d_nhwc_bf16_hip (same K order, same epilogue expressions: outputs are bit-identical to that call; the
 * GroupNorm partial sums are grouped by THIS kernel's tiles, so d_gn_partial needs dafne_conv3x3_c256_num_tiles rows and
 * a finalised mean / rstd may differ from the other kernel's in the last bit).  prm->d_weight is ignored; d_wfrag: bf16
 * [Cout/256][8 waves][144 k16 steps][64 lanes][8] = rows nt*256 + wave*32 + (lane & 31), K columns 16*step +
 * 8*(lane >> 5) .. +8 of the packed weight [Cout][Cin/64][KH][KW][64]  (engine.pack_conv3x3_frag).
 * With DAFNE_CONV_FRAG16 in prm->flags (round 6): d_wfrag: bf16 [Cout/256][8 waves][144 fragments][64 lanes][8], fragment 2m + cb =
 * rows nt*256 + wave*32 + 16*cb + (lane & 15), K columns 32*m + 8*(lane >> 4) .. +8  (engine.pack_conv3x3_frag16); the launch runs the
 * 16x16x32 form of the kernel: the same tiles, statistics layout and definition, fp32 sums of an output in another order (<= 1 bf16
 * ulp from the 32x32x16 form; not bit-identical to dafne_conv2d_nhwc_bf16_hip).
 * The kernel is persistent (one workgroup per CU walks the tiles) and never predicates a store: rows of out-of-image
 * tile pixels go to d_scratch (>= dafne_conv3x3_c256_scratch_bytes(); holds nothing afterwards; may be shared by calls).
 * Shapes: Cin == 256, Cout % 256 == 0, Cout <= 1024, bias, bf16 output, no residual / top-down add; else
 * DAFNE_E_UNSUPPORTED (dafne_conv3x3_c256_ok: 1 / 0).
 */
int dafne_conv3x3_c256_ok(const dafne_conv_params* prm, const dafne_conv_seg* segs);
int dafne_conv3x3_c256_num_tiles(const dafne_conv_params* prm, const dafne_conv_seg* segs);
int dafne_conv3x3_c256_tiles_per_image(const dafne_conv_params* prm, const dafne_conv_seg* segs, int32_t* out);
/* Two layers of identical shape and flags (cls_tower.i and center_tower.i of the DAFNe head, dafne.py:318-348: independent
 * chains) in ONE launch of the persistent kernel: twice the tiles per launch (2784 instead of 1392 at batch 8: 10.9 rounds on
 * 256 CUs instead of 5.4 -- the last-round loss halves) and half the launch boundaries.  Each layer keeps its own tensors,
 * weights, bias and GroupNorm state; results are those of two dafne_conv3x3_c256_hip calls. */
int dafne_conv3x3_c256_pair_hip(const dafne_conv_params* prm_a, const dafne_conv_seg* segs_a, const void* d_wfrag_a,
                                const dafne_conv_params* prm_b, const dafne_conv_seg* segs_b, const void* d_wfrag_b,
                                void* d_scratch, size_t scratch_bytes, void* stream);
size_t dafne_conv3x3_c256_scratch_bytes(void);
int dafne_conv3x3_c256_hip(const dafne_conv_params* prm, const dafne_conv_seg* segs, const void* d_wfrag, void* d_scratch,
                           size_t scratch_bytes, void* stream);
/*
 * Small-M layers -- res5 (1x1 / 3x3 / stride-2 projections on 32 x 32 maps), the FPN laterals, the P4 / P5 outputs and
 * LastLevelP6P7's stride-2 convolutions (backbone/fpn.py:16-37,58-91; d2 ResNet / FPN [recalled]) -- on conv_wr_kernel
 * (conv_wr.hip): 128-pixel x 256-channel tiles over the flat (image, row, column) pixel order, weights streamed L2 ->
 * registers, pixel operand staged by DMA, and a DETERMINISTIC split-K: dafne_conv2d_wr_splits() workgroups share a tile,
 * each writes its fp32 partial (128 KB) to d_workspace, the last arriver sums them in slice order and runs the epilogue.
 * Same parameter block and result definition as dafne_conv2d_nhwc_bf16_hip for one segment with flags RELU / RESIDUAL /
 * UPSAMPLE_ADD / RELU_INPUT (EXCLUSIVE is accepted and ignored: the slice count depends on the shape and the CU count only); 1x1 pad 0 or 3x3 pad 1, stride 1 / 2,
 * Cin % 64 == 0, Cout % 256 == 0, bias required; else DAFNE_E_UNSUPPORTED (dafne_conv2d_wr_ok: 1 / 0).  One slice: K order
 * and epilogue expressions are dafne_conv2d_nhwc_bf16_hip's -> bit-identical output.  Several slices: the fp32 sum is
 * grouped by slices (fp32 rounding apart from the unsplit sum; run-to-run identical).  prm->d_weight is ignored;
 * d_wfrag: bf16 [Cout/256][8 waves][K/16 steps][64 lanes][8] = rows nt*256 + wave*32 + (lane & 31), K columns 16*step +
 * 8*(lane >> 5) .. +8 of the packed weight [Cout][Cin/64][KH][KW][64]  (engine.pack_conv_frag).
 * d_workspace: >= dafne_conv2d_wr_workspace_bytes() (0 for one slice: may be NULL); its first 64 KB are arrival tickets
 * and MUST BE ZERO before the first call (the kernel leaves them zero); calls on ONE stream may share it.
 */
int dafne_conv2d_wr_ok(const dafne_conv_params* prm, const dafne_conv_seg* segs);
int dafne_conv2d_wr_splits(const dafne_conv_params* prm, const dafne_conv_seg* segs);
size_t dafne_conv2d_wr_workspace_bytes(const dafne_conv_params* prm, const dafne_conv_seg* segs);
int dafne_conv2d_wr_hip(const dafne_conv_params* prm, const dafne_conv_seg* segs, const void* d_wfrag, void* d_workspace,
                        size_t workspace_bytes, void* stream);
/*
 * dafne_pred_wgrad_hip (ABI 154, conv_pred_wgrad.hip): the weight and bias gradient of one of the head's prediction
 * convolutions (cls_logits, corners_pred + ctrness, center_pred; dafne.py:318-344) -- 3x3 / stride 1 / pad 1, Cin == 256,
 * 1 <= Cout <= 16 -- summed over every segment, image and pixel:
 *     d_dw[co, ci, kh, kw] = sum g[s][n, y, x, co] * X[s][n, y + kh - 1, x + kw - 1, ci]        d_db[co] = sum g[s][n, y, x, co]
 * prm / segs: the forward call's own description of its input (dafne_conv2d_nhwc_bf16_hip; flags OUT_F32, GN_INPUT and
 * EXCLUSIVE are accepted, anything else is DAFNE_E_INVALID; d_weight, d_bias and the segments' d_out are not read and may
 * be NULL).  X is the bf16 number the forward kernel multiplies: the stored haloed map, or with GN_INPUT GroupNorm + ReLU of
 * it in dafne_groupnorm_relu_nhwc_bf16_hip's expression, rounded to bf16, and zero outside the image (the halo stays zero
 * after the normalisation).  d_gout [n_segs] (a HOST array of device pointers): fp32 [N, Hout, Wout, gout_ps] per segment,
 * channels 0 .. Cout-1 of every pixel are read (gout_ps >= Cout: a view of the leading channels of a wider buffer works,
 * the gap is never read).  d_dw: fp32 [Cout, 256, 3, 3] (OIHW, the state-dict layout); d_db: fp32 [Cout]; every element of
 * both is written, no memset needed.
 * Arithmetic: v_mfma_f32_16x16x32_bf16 over the pixels with g as a hi + lo bf16 pair (|g - hi - lo| <= 2^-16 |g|) and
 * fp32 accumulation per workgroup: |error| <= (2^-16 + n 2^-24) sum |g x| over the n summed pixels.  No atomics: each
 * workgroup writes its partial to d_ws once, a second kernel adds the partials in workgroup order in fp64 -- equal bits from
 * run to run.  d_ws: dafne_pred_wgrad_workspace_bytes(prm, segs) bytes (0: refused parameters, or no device).
 * Refusals, before any launch: NULL pointers, gout_ps < Cout, n_segs outside 1..5 -> DAFNE_E_INVALID; Cin != 256, Cout
 * outside 1..16, not 3x3 / stride 1 / pad 1, a segment above 2^20 pixels per image or 2^32 - 1 bytes of haloed input (the
 * forward call's 32-bit offset limits) -> DAFNE_E_UNSUPPORTED; a small workspace -> DAFNE_E_WORKSPACE.
 */
size_t dafne_pred_wgrad_workspace_bytes(const dafne_conv_params* prm, const dafne_conv_seg* segs);
int dafne_pred_wgrad_hip(const dafne_conv_params* prm, const dafne_conv_seg* segs, const float* const* d_gout, int gout_ps,
                         float* d_dw, float* d_db, void* d_ws, size_t ws_bytes, void* stream);
/*
 * dafne_pred_dgrad_gn_hip (ABI 155, conv_pred_dgrad.hip): the DATA gradient of one of the head's prediction convolutions, carried
 * back through the ReLU and the GroupNorm the forward applies on load, to the raw output of the tower's last convolution.
 * prm / segs: the forward call's own description of its input, as for dafne_pred_wgrad_hip, and GN_INPUT is REQUIRED (raw maps
 * x, d_in_gn_stats (mean, rstd), d_in_gn_gamma, d_in_gn_beta).  d_weight: the packed bf16 weight the forward multiplied,
 * [Cout_pad][256/64][3][3][64] (rows beyond Cout are not read).  d_gout / gout_ps: as for dafne_pred_wgrad_hip.  With groups of 8
 * channels and m = 8 H W per (segment, image, group):
 *     xhat = (x - mean) rstd;  a = the bf16 number the forward multiplied (dafne_groupnorm_relu_nhwc_bf16_hip's expression)
 *     ga[y, x, ci] = sum g[y - kh + 1, x - kw + 1, co] * W[co, ci, kh, kw]  (taps outside the image: 0);   gz = ga [a > 0]
 *     d_dgamma[c] = sum gz xhat;  d_dbeta[c] = sum gz;  gxhat = gz gamma[c];  s1 = sum_group gxhat;  s2 = sum_group gxhat xhat
 *     d_gx[s][n, y, x, c] = rstd (gxhat - s1 / m - xhat s2 / m);   d_dbias[c] = sum d_gx
 * (the forward's bf16 roundings are straight-through, the stored statistics are taken as the statistics of x).  d_gx [n_segs] (a
 * HOST array of device pointers): fp32 dense [N, Hout, Wout, 256], no halo; d_dgamma, d_dbeta, d_dbias: fp32 [256] -- GroupNorm
 * weight / bias and the bias of the convolution that wrote x.  Every element of all outputs is written.
 * Arithmetic: v_mfma_f32_16x16x32_bf16 with exact bf16 weights and g as a hi + lo bf16 pair, fp32 accumulation; two passes over
 * the pixels (the second recomputes ga); no atomics: per-tile and per-workgroup partials in d_ws, added in a fixed order in fp64
 * -- equal bits from run to run.  d_ws: dafne_pred_dgrad_gn_workspace_bytes(prm, segs) bytes (0: refused parameters, or no device)
 * = 4 * (768 * workgroups + 64 * tiles + 64 * n_segs * n_images), tiles of 4 x 32 pixels, workgroups = min(tiles, 2 * CUs).
 * Refusals, before any launch: NULL pointers, gout_ps < Cout, n_segs outside 1..5, GN_INPUT missing or without statistics,
 * unknown flags -> DAFNE_E_INVALID; Cin != 256, Cout outside 1..16, not 3x3 / stride 1 / pad 1, the forward call's 32-bit offset
 * limits -> DAFNE_E_UNSUPPORTED; a small workspace -> DAFNE_E_WORKSPACE.
 */
size_t dafne_pred_dgrad_gn_workspace_bytes(const dafne_conv_params* prm, const dafne_conv_seg* segs);
int dafne_pred_dgrad_gn_hip(const dafne_conv_params* prm, const dafne_conv_seg* segs, const void* d_weight,
                            const float* const* d_gout, int gout_ps, float* const* d_gx, float* d_dgamma, float* d_dbeta,
                            float* d_dbias, void* d_ws, size_t ws_bytes, void* stream);
/*
 * dafne_tower_wgrad_hip (ABI 156, conv_tower_wgrad.hip): the weight gradient of one 256 -> 256 tower convolution of the head
 * (cls_tower / corners_tower .0 .3 .6 .9) -- 3x3 / stride 1 / pad 1 -- summed over every segment, image and pixel:
 *     d_dw[co, ci, kh, kw] = sum g[s][n, y, x, co] * X[s][n, y + kh - 1, x + kw - 1, ci]
 * prm / segs: the forward call's own description of its input, with Cin == Cout == 256 (flags GN_STATS, GN_INPUT, GN_FINALIZE,
 * EXCLUSIVE and FRAG16 are accepted, anything else is DAFNE_E_INVALID; d_weight, d_bias, the output-side GroupNorm pointers and
 * the segments' d_out are not read and may be NULL).  X: as for dafne_pred_wgrad_hip -- the stored haloed map, or with GN_INPUT
 * GroupNorm + ReLU of it rounded to bf16, zero outside the image.  d_gout [n_segs] (a HOST array of device pointers): fp32 dense
 * [N, Hout, Wout, 256] per segment.  d_dw: fp32 [256, 256, 3, 3] (OIHW); every element is written.  There is no bias gradient:
 * it is d_dbias of the data-gradient call of the layer behind (dafne_tower_dgrad_gn_hip, dafne_pred_dgrad_gn_hip).
 * Arithmetic: as dafne_pred_wgrad_hip (g as a hi + lo bf16 pair, fp32 accumulation per workgroup):
 * |error| <= (2^-16 + n 2^-24) sum |g x| over the n summed pixels.  A workgroup owns a block of 64 output x 64 input channels
 * of d_dw and a share of the tiles of 4 x 32 pixels: an input patch is staged (and normalised) once per 64 output channels.  No
 * atomics: the launch is 16 blocks x P pixel splits, P = min(tiles, CUs / 16); split p writes slab p of d_ws, a second kernel adds
 * the slabs in order in fp64 -- equal bits from run to run.  d_ws: dafne_tower_wgrad_workspace_bytes(prm, segs) = P * 256 * 2304 * 4
 * bytes (0: refused parameters, or no device).
 * Refusals, before any launch: NULL pointers, n_segs outside 1..5, GN_INPUT without statistics, unknown flags ->
 * DAFNE_E_INVALID; not 256 -> 256, not 3x3 / stride 1 / pad 1, a segment above 2^20 pixels per image or 2^32 - 1 bytes of haloed
 * input -> DAFNE_E_UNSUPPORTED; a small workspace -> DAFNE_E_WORKSPACE.
 */
size_t dafne_tower_wgrad_workspace_bytes(const dafne_conv_params* prm, const dafne_conv_seg* segs);
int dafne_tower_wgrad_hip(const dafne_conv_params* prm, const dafne_conv_seg* segs, const float* const* d_gout, float* d_dw,
                          void* d_ws, size_t ws_bytes, void* stream);
/*
 * dafne_tower_dgrad_gn_hip (ABI 156, conv_tower_dgrad.hip): the DATA gradient of one 256 -> 256 tower convolution of the head
 * (.3 .6 .9), carried back through the ReLU and the GroupNorm the forward applies on load, to the raw output of the tower
 * convolution before it.  The formulas and the meaning of every argument are dafne_pred_dgrad_gn_hip's with Cout = 256: prm /
 * segs (GN_INPUT REQUIRED; flags as for dafne_tower_wgrad_hip), d_weight: the packed bf16 weight the forward multiplied,
 * [256][256/64][3][3][64]; d_gout: fp32 dense [N, Hout, Wout, 256] per segment; d_gx: fp32 dense [N, Hout, Wout, 256] per
 * segment; d_dgamma, d_dbeta, d_dbias: fp32 [256].  d_gout, d_gx and d_ws are aligned to 16 bytes.  Every element of all outputs
 * is written.
 * Arithmetic: v_mfma_f32_16x16x32_bf16 with exact bf16 weights and g as a hi + lo bf16 pair, fp32 accumulation over K = 2304.
 * The weight is transposed into d_ws ([4 chunks of 64 co][9 taps][256 ci][64 co]) and streams through LDS; pass 1 stores gz =
 * ga [a > 0] in d_gx, pass 2 is elementwise and in place.  No atomics: per-tile and per-workgroup partials in d_ws, added in a
 * fixed order in fp64 -- equal bits from run to run.  d_ws: dafne_tower_dgrad_gn_workspace_bytes(prm, segs) bytes (0: refused
 * parameters, or no device) = 1 179 648 + 4 * (512 * G1 + 64 * tiles + 64 * n_segs * n_images + 256 * G2), tiles of 4 x 32 pixels,
 * G1 = min(tiles, CUs), G2 = min(ceil(pixels / 4), 8 * CUs).
 * Refusals, before any launch: NULL or misaligned pointers, n_segs outside 1..5, GN_INPUT missing or without statistics, unknown
 * flags -> DAFNE_E_INVALID; not 256 -> 256, not 3x3 / stride 1 / pad 1, the forward call's 32-bit offset limits ->
 * DAFNE_E_UNSUPPORTED; a small workspace -> DAFNE_E_WORKSPACE.
 */
size_t dafne_tower_dgrad_gn_workspace_bytes(const dafne_conv_params* prm, const dafne_conv_seg* segs);
int dafne_tower_dgrad_gn_hip(const dafne_conv_params* prm, const dafne_conv_seg* segs, const void* d_weight,
                             const float* const* d_gout, float* const* d_gx, float* d_dgamma, float* d_dbeta, float* d_dbias,
                             void* d_ws, size_t ws_bytes, void* stream);
/*
 * fp8-weight twin (BASELINE config 5: "fp8 weights, CDNA4 fp8 MFMA conv path"; SURVEY 8(b) item 5
 * dafne_conv2d_nhwc_{bf16,fp8w}_hip).  The reference has no fp8 path: this entry DEFINES it.
 *   d_weight   OCP e4m3 bytes [Cout][Cin/64][KH][KW][64] (same K order as the bf16 layout, 1 byte per element)
 *   d_oscale   fp32 [Cout]: weight dequantisation scale of the output channel divided by in_qscale
 *   in_qscale  > 0: activations (bf16 in HBM, after the optional GN_INPUT GroupNorm + ReLU, in fp32) are multiplied
 *              by it, clamped to +-448 and rounded to e4m3 (round to nearest even) while they are loaded
 * out = epilogue(oscale[c] * sum_k e4m3(w)[c][k] * e4m3(x)[k] + bias[c]) with fp32 accumulation on
 * v_mfma_f32_32x32x64_f8f6f4; flags / GroupNorm statistics / output layout as dafne_conv2d_nhwc_bf16_hip.
 * Shapes: 3x3, stride 1, pad 1, Cin % 64 == 0, Cout % 256 == 0, bias, bf16 output, no residual / top-down add
 * (the head towers and FPN output convolutions: the layers the bf16 patch kernel takes); anything else returns
 * DAFNE_E_UNSUPPORTED -- the other layers of a config-5 model run dafne_conv2d_nhwc_bf16_hip on weights that the
 * host dequantised exactly (power-of-two scales).  Tile geometry (d_gn_partial rows) = the bf16 call's when that
 * call's kernel id is 6.
 */
int dafne_conv2d_nhwc_fp8w_hip(const dafne_conv_params* prm, const dafne_conv_seg* segs, const float* d_oscale,
                               float in_qscale, void* stream);
/* M tiles of the fp8w call (rows of d_gn_partial) and per image of every segment: the fp8 kernel always uses the 3x3 patch
 * kernel's 8 x 32 pixel tiles, whatever kernel the bf16 call of the same layer would pick; -1 / error code when the layer is
 * not one the fp8 kernel takes */
int dafne_conv2d_fp8w_num_tiles(const dafne_conv_params* prm, const dafne_conv_seg* segs);
int dafne_conv2d_fp8w_tiles_per_image(const dafne_conv_params* prm, const dafne_conv_seg* segs, int32_t* out);
int dafne_conv2d_cout_pad(int Cout);
/* output pixels per M tile the call would use (geometry of d_gn_partial rows), -1 on error */
int dafne_conv2d_tile_pixels(const dafne_conv_params* prm, const dafne_conv_seg* segs);
/* number of M tiles the call above launches (= rows of d_gn_partial), -1 on error */
int dafne_conv2d_num_tiles(const dafne_conv_params* prm, const dafne_conv_seg* segs);
/* which kernel the call dispatches to (profiling / bench attribution), -1 on error:
 * 0 conv_igemm_kernel<1,4,1,2> (32 cout x 256 px)   1 conv_igemm_kernel<1,4,2,2> (64 x 256)
 * 2 conv_igemm_kernel<2,2,2,2> (128 x 128)           3 conv_igemm_kernel<4,2,2,4> (256 x 256, 8 waves)
 * 4 conv_stream_kernel (persistent, 1x1, Cin 512)    5 conv_ws_kernel (persistent, weights in registers, 1x1, Cin <= 256)
 * 6 conv3x3_patch_kernel (3x3 s1, 256 cout x 8x32 px tiles, input patch staged once per 64-channel slab)
 * 7 conv3x3_slab_kernel (3x3 s1, Cout <= 32, fp32 output: whole 64-channel slabs of both operands in LDS)
 * 8 conv3x3_pred16_kernel (the same layers with Cin = 256 and Cout <= 16: persistent, all weights resident in LDS) */
int dafne_conv2d_kernel_id(const dafne_conv_params* prm, const dafne_conv_seg* segs);
/* M tiles per image of every segment (out[n_segs]): where a segment's rows sit in d_gn_partial */
int dafne_conv2d_tiles_per_image(const dafne_conv_params* prm, const dafne_conv_seg* segs, int32_t* out);

/*
 * OneStageDetector.preprocess_image (one_stage_detector.py:100-107) + ImageList
 * padding: (x - mean)/std on uint8 BGR images [N,3,H,W] (layout_hwc=0) or [N,H,W,3]
 * (=1), zero-padded to Hn x Wn (multiples of 32), written as bf16
 * [N, Hn+6, Wn+6, 4] (3-pixel zero border for the 7x7 stem, 4th channel 0).
 * d_valid_hw: optional int32 [N,2] true sizes (pixels beyond are padding).
 * mean3/std3 are HOST pointers (3 floats each).
 */
int dafne_preprocess_image_hip(const uint8_t* d_img, int layout_hwc, int n_images, int H, int W,
                               const int32_t* d_valid_hw, const float* mean3, const float* std3,
                               int Hn, int Wn, void* d_out, void* stream);
/*
 * detectron2 ResizeShortestEdge / ResizeTransform.apply_image on uint8 images = PIL.Image.resize(BILINEAR)
 * [recalled; dafne/modeling/tta.py:71-99 builds its views with it], bit-exact to Pillow's 8-bit resampler
 * (two separable passes, 22-bit fixed-point coefficients, uint8 intermediate), plus the horizontal / vertical
 * flip of a TTA view folded into the store.  d_in: [C,H,W] (layout_hwc = 0) or [H,W,C] (= 1) uint8;
 * d_out: [C,new_h,new_w] uint8; d_ws: dafne_resize_workspace_bytes(C, H, new_w) bytes.
 */
size_t dafne_resize_workspace_bytes(int C, int H, int new_w);
int dafne_resize_bilinear_u8_hip(const uint8_t* d_in, int layout_hwc, int C, int H, int W, int new_h, int new_w,
                                 int hflip, int vflip, uint8_t* d_out, void* d_ws, size_t ws_bytes, void* stream);
/*
 * conv2 of the res2 bottlenecks [detectron2 BottleneckBlock, recalled; the ResNet of backbone/fpn.py:58-91]: 3x3 / stride 1 /
 * pad 1, 64 -> 64 channels, + bias (FrozenBN folded), optional ReLU.  d_in / d_out: bf16 NHWC [N,H+2,W+2,64] with a zero
 * 1-pixel halo (interior of d_out written); d_weight: bf16 [64, 576], k = (kh, kw, channel) -- the layout
 * dafne_conv2d_nhwc_bf16_hip takes for this layer (engine.pack_conv).  Persistent workgroups with all weights in registers
 * and the input patch of an 8 x 32 output tile staged once in LDS.  Bit-identical to dafne_conv2d_nhwc_bf16_hip.
 */
int dafne_conv3x3_c64_hip(const void* d_in, const void* d_weight, const float* d_bias, int n_images, int H, int W, int relu,
                          void* d_out, void* stream);
/*
 * Tail of one res4 bottleneck + head of the next in one kernel [detectron2 BottleneckBlock, recalled; the ResNet of
 * backbone/fpn.py:58-91]:  d_out = relu(conv3(d_in) + bias3 + d_res)  (1x1, 256 -> 1024, identity shortcut) and
 * d_next = relu(conv1'(d_out) + bias1)  (1x1, 1024 -> 256, the NEXT block's first convolution, stride 1).
 * All tensors bf16 NHWC with a 1-pixel halo: d_in / d_next [N,H+2,W+2,256], d_res / d_out [N,H+2,W+2,1024] (interior
 * written).  d_wfrag: both weight matrices fragment-major, bf16 [8][8][16][64][8] = [phase][wave][k16 step]
 * [lane][8]: phase 2c = conv3 rows c*256 + wave*32 + (lane & 31), K columns 16*step + 8*(lane >> 5) .. +8;
 * phase 2c+1 = conv1' rows wave*32 + (lane & 31), K columns c*256 + 16*step + 8*(lane >> 5) .. +8  (engine.pack_b2b).
 * Bit-identical to dafne_conv2d_nhwc_bf16_hip(conv3, RELU|RESIDUAL) followed by (conv1', RELU); d_out is written
 * once and not read back.
 */
int dafne_bottleneck_tail_head_hip(const void* d_in, const void* d_res, const void* d_wfrag, const float* d_bias3,
                                   const float* d_bias1, int n_images, int H, int W, void* d_out, void* d_next,
                                   void* stream);
/*
 * The whole body of a res4 bottleneck + the head of the next in one kernel (same reference block; conv_bneck.hip):
 *   T = relu(conv2(d_in) + bias2)  (3x3, 256 -> 256, pad 1; d_in = the block's conv1 output),
 *   d_out = relu(conv3(T) + bias3 + d_res)  (1x1, 256 -> 1024),  d_next = relu(conv1'(d_out) + bias1)  (1x1, 1024 -> 256).
 * T never reaches HBM.  Tensors as for dafne_bottleneck_tail_head_hip (bf16 NHWC, 1-pixel halo, interior written); any
 * H, W (4 x 32 pixel tiles -- 2 x 32 where a launch would leave seven eighths of the CUs without a tile; stores of out-of-image
 * tile pixels are masked; d_scratch needs dafne_bottleneck_body_scratch_bytes() bytes and holds nothing afterwards).
 * d_wfrag (ABI 140): conv2 fragment-major, bf16 [8 waves][144 k16 steps][64 lanes][8] (row wave*32 + perm[lane & 31]; K columns
 * 16*step + 8*(lane >> 5) .. +8 of dafne_conv2d_nhwc_bf16_hip's packed weight: 64-channel slab, kh, kw, channel), followed by
 * [8 GEMMs][8 waves][16 k16 steps][64 lanes][8]: GEMM 2c = conv3 rows c*256 + wave*32 + perm[lane & 31] over K = 256, GEMM 2c+1 =
 * conv1' rows wave*32 + perm[lane & 31] over K-chunk c.  perm[8g + 4h + i] = 16 (g >> 1) + 8h + 4 (g & 1) + i  (g = 0..3, h = 0..1,
 * i = 0..3): the rows of every 32-block in the order that makes a lane's 16 accumulator registers two runs of 8 consecutive
 * channels (engine.pack_bneck; NOT dafne_bottleneck_tail_head_hip's layout any more).  Bit-identical to
 * dafne_conv2d_nhwc_bf16_hip(conv2, RELU) followed by dafne_bottleneck_tail_head_hip.  d_next == NULL (the stage's last block: no
 * next conv1): only d_out is produced (d_bias1 may be NULL; the conv1' section of d_wfrag is still read: pack zeros),
 * bit-identical to dafne_conv2d_nhwc_bf16_hip(conv2, RELU) followed by (conv3, RELU|RESIDUAL).
 */
size_t dafne_bottleneck_body_scratch_bytes(void);
int dafne_bottleneck_body_hip(const void* d_in, const void* d_res, const void* d_wfrag, const float* d_bias2,
                              const float* d_bias3, const float* d_bias1, int n_images, int H, int W, void* d_out,
                              void* d_next, void* d_scratch, size_t scratch_bytes, void* stream);
/*
 * The same kernel with v_mfma_f32_16x16x32_bf16 at its three GEMM sites (ABI 150; the towers' DAFNE_CONV_FRAG16 for res4: half the
 * accumulator traffic per flop).  Same arguments, sizes, tile choice and scratch; d_wfrag in engine.pack_bneck16's order: the same
 * sections and byte counts as above with 1-KiB fragments of 16 rows x 32 k -- fragment 2m + cb of a wave = rows wave*32 +
 * perm16[16 cb + (lane & 15)], K columns 32m + 8*(lane >> 4) .. +8 (conv2: 144 fragments per wave, k32 group m = the k16 steps 2m,
 * 2m + 1 of one slab and tap; each GEMM of conv3 / conv1': 16 fragments per wave), perm16[16 cb + 4a + i] = 8a + 4 cb + i  (cb = 0..1,
 * a = 0..3, i = 0..3): a lane's 4 + 4 accumulator registers of a 16-pixel fragment are one run of 8 consecutive channels.  Every
 * output is the same products summed in another order: at most 1 bf16 ulp from dafne_bottleneck_body_hip on an output whose sum
 * does not cancel, NOT bit-identical to it; identical from run to run, at any batch size and tile height.  A model runs ONE of the
 * two entries for all its res4 blocks (engine: EngineOptions.rp_mfma16).
 */
int dafne_bottleneck_body16_hip(const void* d_in, const void* d_res, const void* d_wfrag, const float* d_bias2,
                                const float* d_bias3, const float* d_bias1, int n_images, int H, int W, void* d_out,
                                void* d_next, void* d_scratch, size_t scratch_bytes, void* stream);
/*
 * The same pair for the narrow stage res2 (same reference block):  d_out = relu(conv3(d_in) + bias3 + d_res)  (1x1,
 * 64 -> 256; d_res = the block's shortcut: the identity input or the projection's output) and
 * d_next = relu(conv1'(d_out) + bias1)  (1x1, 256 -> 64).  d_in / d_next [N,H+2,W+2,64], d_res / d_out [N,H+2,W+2,256],
 * bf16 NHWC with a 1-pixel halo (interior written).  d_wfrag: bf16, conv3 fragment-major [8 waves][4 k16 steps][64 lanes][8]
 * (rows wave*32 + (lane & 31), K columns 16*step + 8*(lane >> 5) .. +8) followed by conv1' [2 halves][16 steps][64 lanes][8]
 * (rows half*32 + (lane & 31), same K columns)  (engine.pack_b2b_narrow).  A streaming kernel: persistent workgroups,
 * both weight matrices in registers, 160 KB of HBM traffic per 128 pixels instead of 224 KB.  Bit-identical to
 * dafne_conv2d_nhwc_bf16_hip(conv3, RELU|RESIDUAL) followed by (conv1', RELU).
 */
int dafne_bottleneck_tail_head_narrow_hip(const void* d_in, const void* d_res, const void* d_wfrag, const float* d_bias3,
                                          const float* d_bias1, int n_images, int H, int W, void* d_out, void* d_next,
                                          void* stream);
/*
 * The tail + head pair for res3:  d_out = relu(conv3(d_in) + bias3 + d_res)  (1x1, 128 -> 512) and
 * d_next = relu(conv1'(d_out) + bias1)  (1x1, 512 -> 128).  d_in / d_next [N,H+2,W+2,128], d_res / d_out [N,H+2,W+2,512].
 * d_wfrag: bf16 [16 quarter blocks][4 channel quarters][4 k16 steps][64 lanes][8] in the order the kernel consumes them:
 * for each 256-channel chunk c of d_out: conv3 rows c*256 + rp*128 + quarter*32 + (lane & 31) over K columns
 * 16*(4*sh + step) + 8*(lane >> 5) .. +8 for (rp, sh) = (0,0) (0,1) (1,0) (1,1), then conv1' rows quarter*32 + (lane & 31)
 * over K columns c*256 + rp*128 + 16*(4*sh + step) + 8*(lane >> 5) .. +8 in the same (rp, sh) order  (engine.pack_b2b_mid).
 * Persistent workgroups; waves 0-3 issue every HBM access, waves 4-7 the weight stream (separate vmcnt queues).
 * Bit-identical to dafne_conv2d_nhwc_bf16_hip(conv3, RELU|RESIDUAL) followed by (conv1', RELU).
 */
int dafne_bottleneck_tail_head_mid_hip(const void* d_in, const void* d_res, const void* d_wfrag, const float* d_bias3,
                                       const float* d_bias1, int n_images, int H, int W, void* d_out, void* d_next,
                                       void* stream);
/*
 * Block 0 of res2, whose shortcut is a projection (1x1, 64 -> 256, no ReLU) of the block's input d_x0 [N,H+2,W+2,64]:
 *   shortcut = bf16(proj(d_x0) + bias_sc);  d_out = relu(conv3(d_in) + bias3 + shortcut);  d_next = relu(conv1'(d_out) + bias1).
 * The 256-channel shortcut map is never written or read (112 KB of HBM traffic per 128 pixels instead of 304 KB for the
 * three launches).  d_wfrag: the layout above followed by the projection's weights [8 waves][4 steps][64 lanes][8]
 * (engine.pack_b2b_narrow(w3, w1, wsc)).  Bit-identical to dafne_conv2d_nhwc_bf16_hip(proj), (conv3, RELU|RESIDUAL), (conv1', RELU).
 */
int dafne_bottleneck_proj_tail_head_narrow_hip(const void* d_in, const void* d_x0, const void* d_wfrag, const float* d_bias3,
                                               const float* d_bias_sc, const float* d_bias1, int n_images, int H, int W,
                                               void* d_out, void* d_next, void* stream);
/*
 * A WHOLE res2 bottleneck body, optionally with the head of the next block, in one kernel (same reference block;
 * conv_blk_narrow.hip):  T = relu(conv2(d_in) + bias2)  (3x3, 64 -> 64, pad 1; d_in = the block's conv1 output),
 * d_out = relu(conv3(T) + bias3 + X)  (1x1, 64 -> 256) and, when d_next is given, d_next = relu(conv1'(d_out) + bias1)
 * (1x1, 256 -> 64).  X = d_res [N,H+2,W+2,256] (identity shortcut) or, when d_bias_sc is given (block 0), the projection
 * shortcut conv_sc(d_res) + bias_sc of the block's 64-channel input d_res [N,H+2,W+2,64], rounded to bf16 as the separate
 * launch stores it.  T never reaches HBM (per block at batch 8: 67 MB written + read).  d_wfrag (engine.pack_blk_narrow):
 * conv2 fragment-major [2 channel halves][36 k16 steps][64 lanes][8] (rows half*32 + (lane & 31), K columns 16*step +
 * 8*(lane >> 5) .. +8 of dafne_conv2d_nhwc_bf16_hip's packed weight: kh, kw, channel), conv3 [2 halves of 128][4 quarters]
 * [4 steps][64][8], conv1' [2 halves][16 steps][64][8] (zeros without d_next), the projection in conv3's layout (zeros
 * without d_bias_sc).  4 x 32 pixel tiles, any H, W: rows of out-of-image tile pixels are written to d_scratch
 * (>= dafne_bottleneck_block_narrow_scratch_bytes(); holds nothing afterwards).  Bit-identical to
 * dafne_conv2d_nhwc_bf16_hip(conv2, RELU) followed by dafne_bottleneck_[proj_]tail_head_narrow_hip (or by
 * dafne_conv2d_nhwc_bf16_hip(conv3, RELU|RESIDUAL) without d_next).
 */
size_t dafne_bottleneck_block_narrow_scratch_bytes(void);
int dafne_bottleneck_block_narrow_hip(const void* d_in, const void* d_res, const void* d_wfrag, const float* d_bias2,
                                      const float* d_bias3, const float* d_bias_sc, const float* d_bias1, int n_images, int H, int W,
                                      void* d_out, void* d_next, void* d_scratch, size_t scratch_bytes, void* stream);
/*
 * The LAST res2 bottleneck body at the pixels res3 reads (same reference block with STRIDE_IN_1X1: res3.0.conv1 and
 * res3.0.shortcut are 1x1 stride 2 pad 0; conv_blk_narrow_s2.hip).  With Ho = (H+1)/2, Wo = (W+1)/2, for i < Ho, j < Wo:
 *   T(i,j) = relu(conv2(d_in)(2i,2j) + bias2)   (3x3, 64 -> 64, pad 1, evaluated at the even pixels = stride 2),
 *   d_out(i,j) = relu(conv3(T)(i,j) + bias3 + d_res(2i,2j))   (1x1, 64 -> 256, identity shortcut).
 * d_in [N,H+2,W+2,64], d_res [N,H+2,W+2,256], d_out the COMPACT map [N,Ho+2,Wo+2,256] (interior written, halo untouched).
 * d_wfrag: dafne_bottleneck_block_narrow_hip's (engine.pack_blk_narrow(w2, w3)); only the conv2 and conv3 sections are read.
 * 2 x 32 output-pixel tiles, any H, W: rows of out-of-image tile pixels are written to d_scratch
 * (>= dafne_bottleneck_block_narrow_s2_scratch_bytes(); holds nothing afterwards).  d_out(i,j) is bit-identical to pixel
 * (2i,2j) of dafne_bottleneck_block_narrow_hip's d_out (d_bias_sc == NULL, d_next == NULL).
 */
size_t dafne_bottleneck_block_narrow_s2_scratch_bytes(void);
int dafne_bottleneck_block_narrow_s2_hip(const void* d_in, const void* d_res, const void* d_wfrag, const float* d_bias2,
                                         const float* d_bias3, int n_images, int H, int W, void* d_out, void* d_scratch,
                                         size_t scratch_bytes, void* stream);
/*
 * A WHOLE res3 bottleneck body, optionally with the head of the next block, in one kernel (same reference block;
 * conv_blk_mid.hip):  T = relu(conv2(d_in) + bias2)  (3x3, 128 -> 128, pad 1; d_in = the block's conv1 output),
 * d_out = relu(conv3(T) + bias3 + d_res)  (1x1, 128 -> 512; d_res = the block's shortcut: identity input or projection
 * output) and, when d_next is given, d_next = relu(conv1'(d_out) + bias1)  (1x1, 512 -> 128).  d_in / d_next
 * [N,H+2,W+2,128], d_res / d_out [N,H+2,W+2,512].  T never reaches HBM and every weight byte is fetched once per 128 pixels
 * (dafne_bottleneck_tail_head_mid_hip: once per 64).  d_wfrag (engine.pack_blk_mid): conv2 fragment-major [4 channel
 * groups][72 k16 steps][64 lanes][8] (rows group*32 + (lane & 31), K columns 16*step + 8*(lane >> 5) .. +8 of
 * dafne_conv2d_nhwc_bf16_hip's packed weight: 64-channel slab, kh, kw, channel), conv3 [2 halves of 256][8 groups][8 steps]
 * [64][8], conv1' [4 groups][32 steps][64][8] (zeros without d_next: the section is still read).  4 x 32 pixel tiles, any
 * H, W: rows of out-of-image tile pixels are written to d_scratch (>= dafne_bottleneck_block_mid_scratch_bytes(); holds
 * nothing afterwards).  Bit-identical to dafne_conv2d_nhwc_bf16_hip(conv2, RELU) followed by
 * dafne_bottleneck_tail_head_mid_hip (or by dafne_conv2d_nhwc_bf16_hip(conv3, RELU|RESIDUAL) without d_next).
 */
size_t dafne_bottleneck_block_mid_scratch_bytes(void);
int dafne_bottleneck_block_mid_hip(const void* d_in, const void* d_res, const void* d_wfrag, const float* d_bias2,
                                   const float* d_bias3, const float* d_bias1, int n_images, int H, int W, void* d_out,
                                   void* d_next, void* d_scratch, size_t scratch_bytes, void* stream);
/*
 * detectron2 BasicStem in one kernel [recalled; the backbone of backbone/fpn.py:58-91]: conv 7x7 / s2 / p3
 * (FrozenBN folded into d_weight / d_bias) + ReLU + max-pool 3x3 / s2 / p1.  d_in: the layout
 * dafne_preprocess_image_hip writes, bf16 [N, H+6, W+6, 4]; d_weight: bf16 [64, 256] with k = (kh 0..7, kw 0..7,
 * c 0..3), zero where kh = 7, kw = 7 or c = 3 (the stem weight of dafne_conv2d_nhwc_bf16_hip); d_out: bf16
 * [N, H/4+2, W/4+2, 64] (interior written, halo untouched).  H, W multiples of 4.  Bit-identical to the stem
 * through dafne_conv2d_nhwc_bf16_hip followed by dafne_maxpool3x3s2_nhwc_bf16_hip; the half-resolution map
 * never reaches HBM.
 */
int dafne_stem_pool_hip(const void* d_in, const void* d_weight, const float* d_bias, int n_images, int H, int W,
                        void* d_out, void* stream);
/*
 * The same, plus the first convolution of res2.0 (detectron2 BottleneckBlock.conv1 [recalled]: 1x1, 64 -> 64, FrozenBN folded,
 * + ReLU) computed on the pooled tile while it is in LDS: d_w1 bf16 [64, 64] (cout, cin: the weight of
 * dafne_conv2d_nhwc_bf16_hip), d_b1 fp32 [64], d_out1 bf16 [N, H/4+2, W/4+2, 64] (interior written).  d_out as above.
 * Bit-identical to dafne_stem_pool_hip followed by dafne_conv2d_nhwc_bf16_hip(1x1, RELU) on d_out.
 */
int dafne_stem_pool_conv1_hip(const void* d_in, const void* d_weight, const float* d_bias, const void* d_w1, const float* d_b1,
                              int n_images, int H, int W, void* d_out, void* d_out1, void* stream);
/* 3x3 stride-2 pad-1 max pool of a post-ReLU map: [N,Hin+2,Win+2,C] -> [N,Hin/2+2,Win/2+2,C] */
int dafne_maxpool3x3s2_nhwc_bf16_hip(const void* d_in, void* d_out, int n_images, int Hin, int Win,
                                     int C, void* stream);

typedef struct dafne_gn_seg {
    void* d_x;                      /* bf16 [N, H+2, W+2, C], normalised in place */
    int32_t H, W;
    int32_t tile0, tiles_per_img;   /* where this segment's tiles sit in d_partial */
} dafne_gn_seg;
/*
 * Statistics half of the call below: tile partials -> mean / rstd in d_stats, no normalisation pass.
 * For layers whose consumer applies GroupNorm + ReLU on load (DAFNE_CONV_GN_INPUT).  d_x of the segments
 * is not touched.
 */
int dafne_groupnorm_finalize_hip(const dafne_gn_seg* segs, int n_segs, int n_images, int C,
                                 const float* d_partial, float* d_stats, float eps, void* stream);
/*
 * GroupNorm(C/8 groups, eps) + ReLU (dafne.py:330-344) from the conv's tile
 * partials: fixed-order reduction -> mean/rstd per (segment, image, group) in
 * d_stats [n_segs][N][C/8][2], then y = relu((x-mean)*rstd*gamma+beta) in place.
 */
int dafne_groupnorm_relu_nhwc_bf16_hip(const dafne_gn_seg* segs, int n_segs, int n_images, int C,
                                       const float* d_partial, float* d_stats, const float* d_gamma,
                                       const float* d_beta, float eps, void* stream);
/* out = relu(in) on n_elems bf16 values (n_elems % 8 == 0); halo zeros stay zero. */
int dafne_relu_copy_bf16_hip(const void* d_in, void* d_out, int64_t n_elems, void* stream);

/* ------------------------------------------------ iterative corner chain */
typedef struct dafne_chain_seg {
    const float* d_t;   /* [N, H, W, t_ps] fp32: channels 2k, 2k+1 = c{k}_pred's corners-tower part + bias (k = 0..3) */
    float* d_out;       /* [N, H, W, 8] fp32: [c0|c1|c2|c3]; must not alias d_t (halo pixels of d_t are re-read) */
    int32_t H, W;
} dafne_chain_seg;
/*
 * CORNER_PREDICTION iterative (dafne.py:381-387) after its tower parts: c0 = T[0:2], c_k = T[2k:2k+2] +
 * conv3x3(cat(c0..c_{k-1}); W_k) with zero padding at the map border, k = 1..3, in fp32, one launch for every
 * segment (level) and image.  d_w: the 216 chain weights, c1_pred.weight[:, C:], c2_pred.weight[:, C:],
 * c3_pred.weight[:, C:] (OIHW fp32, 36 + 72 + 108 floats).  n_segs <= 8, t_ps >= 8.
 */
int dafne_corner_chain_hip(const dafne_chain_seg* segs, int n_segs, int n_images, int t_ps, const float* d_w,
                           void* stream);

/* ------------------------------------------------------ whole-scene inference */
/*
 * The DOTA split in one launch (tools/prepare_dota SplitOnlyImage_multi_process.SplitSingle at rate 1,
 * saveimagepatches(padding=True)): tile t is the patch x patch crop of its scene at (left, up), pixels past the
 * scene edge 0.  `tiles` is a HOST array of n_tiles descriptors (checked on the host, copied into d_ws on `stream`);
 * d_scene: uint8 BGR [H,W,3] (layout_hwc = 1) or [3,H,W] (= 0), 0 <= left < w, 0 <= up < h.  d_out_hwc: [n_tiles,
 * patch, patch, 3] uint8, 8-byte aligned (detect_packed(layout_hwc=True) takes it).  patch % 8 != 0 ->
 * DAFNE_E_UNSUPPORTED.  d_ws: dafne_scene_tiles_workspace_bytes(n_tiles) bytes.
 */
typedef struct dafne_scene_tile {
    const uint8_t* d_scene;
    int32_t h, w, layout_hwc, left, up, reserved;
} dafne_scene_tile;
size_t dafne_scene_tiles_workspace_bytes(int n_tiles);
int dafne_scene_tiles_u8_hip(const dafne_scene_tile* tiles, int n_tiles, int patch, uint8_t* d_out_hwc, void* d_ws,
                             size_t ws_bytes, void* stream);
/*
 * Tile detections -> the f64 rows of the tile merge (ResultMerge_multi_process.mergebypoly after
 * _generate_task_1_files' text round trip), one bucket per (scene, class): bucket s * n_classes + c.
 *   d_rows [n_tiles, k_cap, DAFNE_DET_ROW] f32 + d_counts [n_tiles] (detect_packed's output); d_tile_info [n_tiles, 3]
 *   int32 (left, up, scene index < n_scenes); skip_mask: bit c set = class c is left out (DOTA-1.5 container-crane);
 *   score_mode 1: score^2 / centerness in fp32 (task1_scores, CENTERNESS != none and not CENTERNESS_USE_IN_SCORE).
 * Row: x_k = (rint(double(v_k) * 100) / 100 + left | up) / 1.0, score = rint(double(s) * 1e4) / 1e4, i.e.
 * float("%.2f" % v) / float("%.4f" % s) shifted as poly2origpoly does.  Order in a bucket: tile order, then the
 * tile's row order (a stable compaction; no atomic decides a position).
 *   d_bucket_counts [n_scenes * n_classes] int32: the bucket's TRUE row count (always written)
 *   d_dets [n_buckets, m_cap, 9] f64, d_src [n_buckets, m_cap] int32 (tile * k_cap + row): rows at positions < m_cap.
 * m_cap = 0 computes the counts only (d_dets / d_src may be NULL): the caller sizes m_cap from them.  n_classes <= 64.
 * d_ws: dafne_scene_merge_workspace_bytes(n_tiles, n_classes) bytes.
 */
size_t dafne_scene_merge_workspace_bytes(int n_tiles, int n_classes);
int dafne_scene_merge_rows_hip(const float* d_rows, const int32_t* d_counts, int n_tiles, int k_cap, const int32_t* d_tile_info,
                               int n_scenes, int n_classes, uint64_t skip_mask, int score_mode, int m_cap, double* d_dets,
                               int32_t* d_bucket_counts, int32_t* d_src, void* d_ws, size_t ws_bytes, void* stream);

/*
 * The same tile detections as the rows of the Task2 merge (ResultMerge_multi_process.py:238-248 mergebyrec): arguments, bucket
 * order, skip mask, score mode, d_bucket_counts, d_src and the two-call protocol of dafne_scene_merge_rows_hip (same
 * workspace size).  d_dets5 [n_buckets, m_cap, 5] f64: xmin, ymin, xmax, ymax, score with xmin = the minimum of the Task1
 * row's four x values (rint(double(v) * 100) / 100 + left), ymin / xmax / ymax likewise -- dafne/utils/dota_utils.py:109-127
 * (dots4ToRec4, parse_dota_rec) -- and the Task1 row's score.
 */
int dafne_scene_merge_hbb_rows_hip(const float* d_rows, const int32_t* d_counts, int n_tiles, int k_cap, const int32_t* d_tile_info,
                                   int n_scenes, int n_classes, uint64_t skip_mask, int score_mode, int m_cap, double* d_dets5,
                                   int32_t* d_bucket_counts, int32_t* d_src, void* d_ws, size_t ws_bytes, void* stream);

/*
 * TTA views cut straight from the scenes (DotaDatasetMapperTTA, dafne/modeling/tta.py:71-99: per TEST.AUG size, plain /
 * hflip / vflip).  View v = Pillow's BILINEAR resize of the win_h x win_w window of its source at (left, up) to
 * out_h x out_w, then the flips; window pixels past the source read as 0 (the split's padding=True).  Bit for bit
 * dafne_resize_bilinear_u8_hip of the zero-padded crop (dafne_scene_tiles_u8_hip) with the same flips, including out ==
 * window (flips only) and upscales.  Two kinds of source: a scene with the window set to a tile, or an already resized
 * tile with the window set to the whole image.
 *   views: HOST array of n_views descriptors (checked on the host, copied into d_ws on `stream`); d_src uint8 BGR
 *   [h,w,3] (layout_hwc = 1) or [3,h,w] (= 0), left, up >= 0, hflip / vflip 0 or 1.
 *   d_out: [n_views, 3, out_h, out_w] uint8 CHW (detect_packed's batch).
 * A downscale beyond dafne_resize_bilinear_u8_hip's tap limit, or more than 8 distinct window widths (or heights) in one
 * call -> DAFNE_E_UNSUPPORTED.  d_ws: dafne_scene_views_workspace_bytes(views, n_views, out_h, out_w) bytes (the
 * descriptors and the coefficient tables, computed once per call and axis); 0 = unsupported arguments.
 */
typedef struct dafne_view_src {
    const uint8_t* d_src;
    int32_t h, w, layout_hwc;
    int32_t left, up, win_h, win_w;
    int32_t hflip, vflip, reserved;
} dafne_view_src;
size_t dafne_scene_views_workspace_bytes(const dafne_view_src* views, int n_views, int out_h, int out_w);
int dafne_scene_views_u8_hip(const dafne_view_src* views, int n_views, int out_h, int out_w, uint8_t* d_out, void* d_ws,
                             size_t ws_bytes, void* stream);
/*
 * Tiles of a RESAMPLED scene, cut straight from the original scene (multi-scale whole-scene inference, scene.detect_scenes(
 * scales=...)): tile t is the patch x patch crop at (left, up) of PIL.Image.resize(scene, (new_w, new_h), filter) -- Pillow's
 * two-pass 8-bit resampler on the WHOLE scene, so the taps clip at the scene's border and not at the tile's -- and 0 past
 * new_h / new_w, bit for bit.  filter: DAFNE_FILTER_BILINEAR (triangle, support 1) or DAFNE_FILTER_BICUBIC (a = -0.5, support
 * 2).  The resampled scene is never written: a workgroup resamples the source rows its output rows need into LDS.
 *   tiles: HOST array of n_tiles descriptors (checked on the host, copied into d_ws on `stream`); d_scene uint8 [h,w,3]
 *   (layout_hwc = 1) or [3,h,w] (= 0); new_h, new_w >= 1; 0 <= left < new_w, 0 <= up < new_h.
 *   d_out_hwc: [n_tiles, patch, patch, 3] uint8, 4-byte aligned (what dafne_scene_tiles_u8_hip writes).
 * patch % 4 != 0, or a downscale whose filter needs more than 64 taps (bilinear above 31x, bicubic above 15x) ->
 * DAFNE_E_UNSUPPORTED.  Any number of distinct (size, new size, filter) axes per call.  d_ws:
 * dafne_scene_scaled_tiles_workspace_bytes(tiles, n_tiles) bytes (descriptors + one coefficient table per distinct axis); 0 =
 * invalid descriptors.
 */
#define DAFNE_FILTER_BILINEAR 0
#define DAFNE_FILTER_BICUBIC 1
typedef struct dafne_scaled_tile {
    const uint8_t* d_scene;
    int32_t h, w, layout_hwc;
    int32_t new_h, new_w;
    int32_t left, up;
    int32_t filter;
} dafne_scaled_tile;
size_t dafne_scene_scaled_tiles_workspace_bytes(const dafne_scaled_tile* tiles, int n_tiles);
int dafne_scene_scaled_tiles_u8_hip(const dafne_scaled_tile* tiles, int n_tiles, int patch, uint8_t* d_out_hwc, void* d_ws,
                                    size_t ws_bytes, void* stream);
/*
 * dafne_scene_merge_rows_hip / dafne_scene_merge_hbb_rows_hip for tiles of resampled scenes: d_tile_scale [n_tiles] f64
 * (device), the rate of each tile's split; x_k = (rint(double(v_k) * 100) / 100 + left | up) / scale in fp64, which is
 * poly2origpoly's float(poly + x) / float(rate) (ResultMerge_multi_process.py), so the rows are in ORIGINAL scene coordinates;
 * the Task2 row is dots4ToRec4 of those values (min / max after the division).  left / up of d_tile_info are in the resampled
 * scene's coordinates.  NULL = every scale 1.0: the unscaled entries, bit for bit.  Everything else as the unscaled entries.
 */
int dafne_scene_merge_rows_scaled_hip(const float* d_rows, const int32_t* d_counts, int n_tiles, int k_cap,
                                      const int32_t* d_tile_info, const double* d_tile_scale, int n_scenes, int n_classes,
                                      uint64_t skip_mask, int score_mode, int m_cap, double* d_dets, int32_t* d_bucket_counts,
                                      int32_t* d_src, void* d_ws, size_t ws_bytes, void* stream);
int dafne_scene_merge_hbb_rows_scaled_hip(const float* d_rows, const int32_t* d_counts, int n_tiles, int k_cap,
                                          const int32_t* d_tile_info, const double* d_tile_scale, int n_scenes, int n_classes,
                                          uint64_t skip_mask, int score_mode, int m_cap, double* d_dets5,
                                          int32_t* d_bucket_counts, int32_t* d_src, void* d_ws, size_t ws_bytes, void* stream);
/*
 * The merge input of OneStageRCNNWithTTA (dafne/modeling/tta.py:237-262) for n_images images on the device: every view's
 * packed rows (detect_packed(do_postprocess=False): d_rows [k_cap, DAFNE_DET_ROW] f32 + *d_count, device pointers per
 * view, so the chunks of several detector calls need no concatenation) back through the inverse of the view's transforms:
 * x' = ((flip_x ? width - x : x) * rx1) * rx2, y' likewise with flip_y / height / ry1 / ry2, float32 in that order (rx1:
 * view -> loader image, rx2: loader image -> original image, float32 of the double ratio; 1 where there is none).
 * Output: the Candidates layout of dafne_decode_levels_hip, [n_images, m_cap] rows: corners (8), scores, ctr, classes,
 * locs (2), levels copied from the row, hbox = min / max of the mapped corners; d_counts [n_images] = the image's rows.
 * Order: per image the views in slot order (slot = position in the mapper's view order), each view's rows in their own
 * order; a view's offset is the prefix of the earlier slots' counts (no atomic decides a position).  (image, slot) pairs
 * must be unique; views per image x k_cap <= m_cap <= 65536 (the rotated NMS's limit).
 * d_overflow [n_images] int32: 1 where a view's count is above k_cap (its rows are truncated: the caller must raise).
 * views: HOST array (copied into d_ws on `stream`); d_ws: dafne_tta_candidates_workspace_bytes(n_views, n_images) bytes.
 */
typedef struct dafne_tta_view {
    const float* d_rows;
    const int32_t* d_count;
    int32_t tile, slot;
    int32_t flip_x, flip_y;
    float width, height;
    float rx1, ry1, rx2, ry2;
} dafne_tta_view;
size_t dafne_tta_candidates_workspace_bytes(int n_views, int n_images);
int dafne_tta_candidates_hip(const dafne_tta_view* views, int n_views, int n_images, int k_cap, int m_cap, float* d_corners,
                             float* d_scores, float* d_ctr, int32_t* d_classes, float* d_locs, int32_t* d_levels,
                             float* d_hbox, int32_t* d_counts, int32_t* d_overflow, void* d_ws, size_t ws_bytes, void* stream);

/*
 * Scoring whole-scene detections against the scenes' labels: dafne/evaluation/voc_eval.py:132-205 for fixed inputs, without
 * the text files.  Buckets are (scene, class): bucket s * n_classes + c.  Ground truth d_gt [n_gt, 8] f64 is sorted
 * bucket-major (file order inside a bucket), bucket b = rows d_gt_offsets[b] .. d_gt_offsets[b + 1] (n_buckets + 1 int32).
 *
 * dafne_scene_match_hip: for detection d (d_dets [n, 8] f64, d_bucket [n] int32; a bucket outside [0, n_buckets) has no
 * ground truth) the candidates are its bucket's boxes whose axis-aligned hulls pass inters / uni > 0 with the +1 convention
 * on widths, heights and both areas (voc_eval.py:150-178, fp64, that operation order); ov = iou_poly(ground truth,
 * detection), bit for bit polyiou.cpp.  d_ovmax[d] = max over the candidates, d_jmax[d] = the lowest index INSIDE THE
 * BUCKET among the maxima (np.argmax); no candidates: -inf and -1.  A candidate pair that does not touch gives 0.
 *
 * dafne_scene_mark_hip: the greedy marking as a rank minimum.  d_rank [n] int32: the detection's position in the order
 * voc_eval walks (descending score), distinct among the detections of one class.  With ovmax > thresh: matched box
 * difficult (d_difficult [n_gt] uint8) -> tp = fp = 0; else tp = 1 for the smallest rank matched to that box and fp = 1 for
 * the others; ovmax <= thresh -> fp = 1.  d_tp, d_fp [n] uint8.  d_ws: dafne_scene_mark_workspace_bytes(n_gt) bytes (one
 * int32 per box, an integer atomicMin: its result does not depend on the order of arrival).
 * n = 0 launches nothing; n_gt = 0 and empty buckets are valid.
 */
int dafne_scene_match_hip(const double* d_dets, const int32_t* d_bucket, int n, const double* d_gt, const int32_t* d_gt_offsets,
                          int n_buckets, int n_gt, double* d_ovmax, int32_t* d_jmax, void* stream);
/*
 * dafne_scene_match_hbb_hip: the Task2 (horizontal box) form of dafne_scene_match_hip.  d_dets [n, 4] and d_gt [n_gt, 4] f64
 * are xmin, ymin, xmax, ymax (dota_utils.py:109-127 dots4ToRec4 of the oriented boxes); ov against EVERY box of the bucket is
 * inters / uni of dafne/evaluation/voc_eval.py:158-173 applied to the two rectangles (+1 on widths, heights and both areas,
 * fp64, that operation order).  d_ovmax[d] = the maximum over the bucket (zeros included), d_jmax[d] = the lowest index inside
 * the bucket among the maxima; an empty bucket or one outside [0, n_buckets): -inf and -1.  Marking: dafne_scene_mark_hip.
 */
int dafne_scene_match_hbb_hip(const double* d_dets, const int32_t* d_bucket, int n, const double* d_gt, const int32_t* d_gt_offsets,
                              int n_buckets, int n_gt, double* d_ovmax, int32_t* d_jmax, void* stream);
size_t dafne_scene_mark_workspace_bytes(int n_gt);
int dafne_scene_mark_hip(const int32_t* d_rank, const double* d_ovmax, const int32_t* d_jmax, const int32_t* d_bucket, int n,
                         const int32_t* d_gt_offsets, int n_buckets, const uint8_t* d_difficult, int n_gt, double thresh,
                         uint8_t* d_tp, uint8_t* d_fp, void* d_ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------- target assignment, loss values and the losses' gradients */
/*
 * dafne_assign_targets_hip: compute_targets_for_locations plus _get_ground_truth's stride division
 * (dafne/modeling/dafne/dafne_outputs.py:252-503) for a batch.  Ground truth: the boxes of all images packed one after the
 * other, d_gt_corners [n_gt, 8], d_gt_hbox [n_gt, 4] (x1, y1, x2, y2), d_gt_area [n_gt] f32, d_gt_class [n_gt] int32, and
 * d_gt_offsets [n_images + 1] int32 ascending from 0 (image i owns rows offsets[i] .. offsets[i + 1]; read on the device and
 * clamped to [0, n_gt]).  Locations are regenerated as compute_locations (dafne.py:37-44) makes them from H, W, stride.
 * size_lo / size_hi: the level's size of interest (:183-190); radius: float(stride * POS_RADIUS).
 * Outputs, LEVEL first, then image, then location (the order of the reference's losses(), :527): position
 * p = n_images * (locations of the levels before l) + image * H_l * W_l + location;
 *   d_label [P] int32 (n_classes = background), d_target_ind [P] int32 (row into the packed boxes, -1 for an image without
 *   boxes), d_reg_corners [P, 8], d_reg_ltrb [P, 4], d_reg_abcd [P, 4] f32 (those of box 0 of the image at background).
 * fp32 in the reference's operation order: integers equal and floats bit-equal to torch on the CPU for finite inputs.
 */
#define DAFNE_TGT_CENTER_SAMPLE 1
#define DAFNE_TGT_CENTER_SAMPLE_ONLY 2
#define DAFNE_TGT_COMBINE_CENTER_SAMPLE 4
#define DAFNE_TGT_IN_BOX_CHECK 8
#define DAFNE_TGT_LEVEL_SIZE_FILTERING 16
#define DAFNE_TGT_FPN_STRIDE_NORM 32
#define DAFNE_TGT_ALL_FLAGS 63
typedef struct dafne_target_params {
    int32_t n_images, n_levels, n_classes, flags;      /* n_levels <= 8 */
    int32_t H[8], W[8], stride[8];
    float size_lo[8], size_hi[8], radius[8];
} dafne_target_params;
int dafne_assign_targets_hip(const dafne_target_params* prm, const float* d_gt_corners, const float* d_gt_hbox,
                             const float* d_gt_area, const int32_t* d_gt_class, const int32_t* d_gt_offsets, int n_gt,
                             int32_t* d_label, int32_t* d_target_ind, float* d_reg_corners, float* d_reg_ltrb,
                             float* d_reg_abcd, void* stream);

/*
 * dafne_losses_hip: dafne_losses (dafne_outputs.py:620-731) with ModulatedEightPointLoss / SmoothL1Loss
 * (dafne/modeling/losses/smooth_l1.py) and the sigmoid focal loss  p = sigmoid(x), ce = BCEWithLogits(x, t),
 * p_t = p t + (1 - p)(1 - t), loss = ce (1 - p_t)^gamma (alpha t + (1 - alpha)(1 - t)), summed.  World size 1.
 * levels: the head's raw outputs as dafne_decode_levels_hip takes them (corner regression = (center.repeat(4) + delta) *
 * scale, or delta * scale without d_center, center regression = center * scale, all fp32 as DAFNeHead.forward forms them);
 * with DAFNE_LOSS_COOKED d_delta is the finished corner regression and d_center the finished center regression.
 * d_label / d_reg_*: dafne_assign_targets_hip's outputs for the same levels and n_images.
 * Every term is evaluated in fp64 from these fp32 values -- that is the engine's definition of the loss; the reference's
 * fp32 result is one rounding of the same formulas.  The centerness target's ratio (min / max)(min / max) is the fp32 value the
 * reference forms, raised to float(1 / ctr_alpha) in fp64.  Partial sums per workgroup in d_ws, added in index order by a
 * last workgroup: no floating-point atomics, equal bits from run to run.
 * d_out6 [6] f64: loss/cls, loss/corners, loss/center, loss/ctr (each times its lambda; 0 for a term the configuration
 * lacks), num_pos, loss_denorm.  d_ctr_targets [P] f32 or NULL: the centerness target at positives, 0 elsewhere.
 */
#define DAFNE_LOSS_LOGSPACE 1
#define DAFNE_LOSS_MODULATION 2
#define DAFNE_LOSS_SORT_CORNERS 4
#define DAFNE_LOSS_HAS_CENTER_REG 8
#define DAFNE_LOSS_COOKED 16
#define DAFNE_LOSS_CTR_PLAIN 32
#define DAFNE_LOSS_CTR_ORIENTED 64
#define DAFNE_LOSS_ALL_FLAGS 127
typedef struct dafne_loss_params {
    int32_t n_images, n_levels, n_classes, flags;
    double alpha, gamma;        /* focal loss (LOSS_ALPHA, LOSS_GAMMA) */
    double beta;                /* LOSS_SMOOTH_L1_BETA */
    double ctr_alpha;           /* CENTERNESS_ALPHA */
    double lambda_cls, lambda_corners, lambda_center, lambda_ctr;
} dafne_loss_params;
size_t dafne_losses_workspace_bytes(const dafne_loss_params* prm, const dafne_level_desc* levels);
int dafne_losses_hip(const dafne_loss_params* prm, const dafne_level_desc* levels, const int32_t* d_label,
                     const float* d_reg_corners, const float* d_reg_ltrb, const float* d_reg_abcd, double* d_out6,
                     float* d_ctr_targets, void* d_ws, size_t ws_bytes, void* stream);

/*
 * dafne_losses_backward_hip: the derivative of dafne_losses_hip's four terms (dafne_outputs.py:620-731, smooth_l1.py) with
 * respect to the inputs that feed them, for the DAFNE_LOSS_COOKED form only (without it: DAFNE_E_UNSUPPORTED): logits <-
 * loss/cls, corner regression <- loss/corners, center regression <- loss/center, centerness logits <- loss/ctr.  The
 * conventions are those of the reference's autograd: the centerness target is a constant; the modulated minimum sends its
 * gradient to the first of equal shifts (none, [1,2,3,0], [3,0,1,2]); sort_quadrilateral sends none to the output slots it
 * leaves at zero (a quadrilateral without an l * r < 0 candidate: only the leftmost corner receives one); the smooth L1 has
 * sign(0) = 0 and the linear branch from |x - y| == beta on.  Every term in fp64 from the fp32 inputs, times its lambda and its
 * upstream factor d_grad_out4 [4] f64 (cls, corners, center, ctr; read on the device), rounded once to fp32.
 * prm, levels, d_label, d_reg_*: as given to dafne_losses_hip.  d_fwd_ws / fwd_ws_bytes: that call's workspace, unchanged
 * since -- its partial sums are added again in the forward's order, so num_pos, the centerness sum and the "sum > 0" decision
 * are the forward's own, with no host read between the two calls.
 * grads [n_levels]: where the gradients go, in the layout of the inputs (NHWC per level) with their own pixel strides.  Every
 * element of every tensor given is written (zeros at non-positives for the three regression / centerness tensors): no memset,
 * no atomics, one writer per element, equal bits from run to run.  A pointer that is NULL in every level leaves that gradient
 * out; d_center / d_ctrness must be NULL when the configuration lacks the term.
 * d_ws: dafne_losses_backward_workspace_bytes(prm, levels) bytes (0: bad parameters / level table).
 */
typedef struct dafne_level_grad {
    float* d_logits;   /* [N, H, W, C] */
    float* d_delta;    /* [N, H, W, 8] */
    float* d_center;   /* [N, H, W, 2] */
    float* d_ctrness;  /* [N, H, W]    */
    int32_t logits_ps, delta_ps, center_ps, ctrness_ps;      /* pixel strides in floats (>= C, 8, 2, 1) */
} dafne_level_grad;
size_t dafne_losses_backward_workspace_bytes(const dafne_loss_params* prm, const dafne_level_desc* levels);
int dafne_losses_backward_hip(const dafne_loss_params* prm, const dafne_level_desc* levels, const int32_t* d_label,
                              const float* d_reg_corners, const float* d_reg_ltrb, const float* d_reg_abcd, const void* d_fwd_ws,
                              size_t fwd_ws_bytes, const double* d_grad_out4, const dafne_level_grad* grads, void* d_ws,
                              size_t ws_bytes, void* stream);

/*
 * dafne_head_uncook_backward_hip (ABI 154): dafne_losses_backward_hip differentiates with respect to the FINISHED regressions
 * (DAFNE_LOSS_COOKED); this call carries those gradients back through DAFNeHead.forward's last step (dafne.py:394-411) to the
 * raw outputs of the prediction convolutions and to the per-level scales:
 *     center-to-corner  reg = (center.repeat(4) + delta) * s, center_reg = center * s        direct / offset  reg = delta * s
 *     d_g_delta [.., 0..7] = s g_reg;  d_g_delta [.., 8] = g_ctrness (with d_g_ctrness: the fused [delta8|ctrness] layout)
 *     d_g_center = s (sum over the four corners of g_reg + g_center_reg)
 *     d_g_scale [l] = sum g_reg (center.repeat(4) + delta) + sum g_center_reg center      (fp64, one number per level)
 * Per level: NHWC fp32 tensors of [n_images, H, W] pixels with their own pixel strides (floats).  d_center, d_g_center_reg and
 * d_g_center are all given (center-to-corner) or all NULL, d_g_ctrness is given or NULL, the same way in every level.  Every
 * value is formed in fp64 from the fp32 inputs and rounded once; d_g_scale is reduced in a fixed order without atomics (equal
 * bits from run to run): |error| <= n 2^-53 sum |terms|.  d_ws: dafne_head_uncook_backward_workspace_bytes() bytes (0:
 * refused).  NULL / inconsistent pointers, a pixel stride below the channels read, n_levels outside 1..8 -> DAFNE_E_INVALID;
 * 2^31 pixels in a level -> DAFNE_E_UNSUPPORTED.  The iterative head's corner chain has no backward.
 */
typedef struct dafne_uncook_level {
    const float* d_g_reg;         /* [N, H, W, 8] gradient of the finished corner regression */
    const float* d_g_center_reg;  /* [N, H, W, 2] gradient of the finished center regression, or NULL */
    const float* d_g_ctrness;     /* [N, H, W]    gradient of the centerness logits, or NULL */
    const float* d_delta;         /* [N, H, W, 8] raw corners_pred output */
    const float* d_center;        /* [N, H, W, 2] raw center_pred output, or NULL */
    float* d_g_delta;             /* [N, H, W, 8 or 9] out */
    float* d_g_center;            /* [N, H, W, 2] out, or NULL */
    int32_t g_reg_ps, g_center_reg_ps, g_ctrness_ps, delta_ps, center_ps, g_delta_ps, g_center_ps;
    int32_t H, W;
    float scale;
} dafne_uncook_level;
size_t dafne_head_uncook_backward_workspace_bytes(const dafne_uncook_level* levels, int n_levels, int n_images);
int dafne_head_uncook_backward_hip(const dafne_uncook_level* levels, int n_levels, int n_images, double* d_g_scale, void* d_ws,
                                   size_t ws_bytes, void* stream);

/*
 * Scene labels -> the ground truth of every tile of a split scene (ImgSplit_multi_process.splitbase.savepatches at rate 1
 * for convex quadrilaterals, then the training filter of DOTA2COCO.py / dafne/data/datasets/dota.py); the operation order
 * is written down in csrc/scene_labels_kernels.h.
 * dafne_scene_split_labels_hip: one thread per (tile, object of its scene) pair.  d_tiles5 [T, 5] int32 = scene, left, up,
 * right, down (right = min(left + patch, w - 1), down = min(up + patch, h - 1): SplitSingle's rectangle); d_pair_off
 * [T + 1] int32: pair p of tile t is object d_obj_off[scene] + (p - d_pair_off[t]); d_obj_off [S + 1]; d_boxes [G, 8] f64 and
 * d_difficult [G] int32 in label-file order per scene.  d_records [P, 12] int32: outcome (0 none, 1 inside, 2 cut to 4
 * vertices, 3 cut to 5, 4 dropped with < 4, 5 dropped with > 5, 6 non-convex object), the 8 tile coordinates, difficult
 * (2: the part left is <= thresh of the object), kept (passes difficult != 2, area > min_area, max side >= min_side, no
 * coinciding corners), 0.  n_pairs above INT32_MAX is refused.
 * dafne_scene_pack_tile_gt_hip: ordered compaction per tile (count, exclusive scan over tiles, write; no atomics).  Set (a),
 * the written rows: d_all_offsets [T + 1], d_all_corners [n, 8] int32, class, difficult, src (row of d_boxes).  Set (b), the
 * kept rows as dafne_assign_targets_hip reads them: d_kept_offsets [T + 1], corners f32 [n, 8] = (float)(coordinate * ratio)
 * (the product in f64), sort_quadrilateral applied when `sort`, hull box, area (shoelace in f64, rounded), class, src.  The
 * row arrays must hold n_pairs rows.  d_stats9: the 7 outcome counts, written rows, kept rows.
 */
int dafne_scene_split_labels_hip(const int32_t* d_tiles5, const int32_t* d_pair_off, int n_tiles, const int32_t* d_obj_off,
                                 int n_scenes, const double* d_boxes, const int32_t* d_difficult, int n_objects, int patch,
                                 double thresh, double min_area, double min_side, int32_t* d_records, int64_t n_pairs,
                                 void* stream);
size_t dafne_scene_pack_tile_gt_workspace_bytes(int n_tiles);
int dafne_scene_pack_tile_gt_hip(const int32_t* d_records, const int32_t* d_pair_off, const int32_t* d_tiles5, int n_tiles,
                                 const int32_t* d_obj_off, const int32_t* d_class, double ratio_x, double ratio_y, int sort,
                                 int32_t* d_all_offsets, int32_t* d_all_corners, int32_t* d_all_class, int32_t* d_all_difficult,
                                 int32_t* d_all_src, int32_t* d_kept_offsets, float* d_kept_corners, float* d_kept_hbox,
                                 float* d_kept_area, int32_t* d_kept_class, int32_t* d_kept_src, int32_t* d_stats9, void* d_ws,
                                 size_t ws_bytes, void* stream);

/*
 * Training views (tools/plain_train_net.py:229-256 build_train_loader: hflip, vflip, resize, quarter turns; then
 * DAFNeDatasetMapper's ground truth), cut straight from scenes or tiles.  A view is the win_h x win_w window of its source at
 * (left, up) (0 past the source, as dafne_view_src), flipped, THEN resized with Pillow's BILINEAR filter to new_h x new_w,
 * then turned by rot quarter turns counter-clockwise: np.rot90(resize(flip(window)), rot), the exact permutation.
 *   dafne_train_views_u8_hip: views is a HOST array (checked on the host, copied into d_ws on `stream`).  d_out
 *   [n_views, 3, cap_h, cap_w] uint8, 4-byte aligned, cap_w % 4 == 0: view v fills [:oh, :ow] of its slab, (oh, ow) = (new_h,
 *   new_w) for an even rot and (new_w, new_h) for an odd one, and every other byte of the slab is written 0 by the same launch.
 *   d_valid_hw [n_views, 2] int32 receives (oh, ow).  cap_w % 4 != 0, a misaligned output, a view that does not fit its slab
 *   or a downscale beyond dafne_resize_bilinear_u8_hip's tap limit -> DAFNE_E_UNSUPPORTED.  Any number of distinct (window,
 *   new size) axes per call.  d_ws: dafne_train_views_workspace_bytes(views, n_views) bytes; 0 = invalid descriptors.
 *   dafne_train_gt_hip: the ground truth of the same views (d_src of the descriptors is not read).  Object g of view v,
 *   d_offsets_in[v] <= g < d_offsets_in[v + 1] (device int32 [n_views + 1]; G bounds the rows of every array), has the fp32
 *   corners d_corners_in[g] at window scale.  In fp64, one operation at a time: x = win_w - x if hflip; y = win_h - y if vflip;
 *   x = x * (new_w / win_w), y = y * (new_h / win_h); rot 1: (x, y) = (y, new_w - x), rot 2: (new_w - x, new_h - y), rot 3:
 *   (new_h - y, x).  area = (float)(0.5 * |sum x_i y_(i-1) - sum y_i x_(i-1)|), the sums in index order from 0.0 (PolygonMasks.area
 *   before the cast); the corners are rounded to fp32 once, hbox = min / max of the fp32 corners, then sort_quadrilateral is
 *   applied when `sort`; a row is kept when hbox width > 1e-5f and height > 1e-5f (fp32; filter_empty_instances by box).  Kept rows
 *   are packed per view in input order (count, exclusive scan over the views, ordered write; no atomics): d_corners [G, 8],
 *   d_hbox [G, 4], d_area [G] f32, d_classes [G] int32, d_offsets_out [n_views + 1] int32, d_src [G] int32 (the input row of
 *   every kept row) -- the arrays dafne_assign_targets_hip reads.  d_ws: dafne_train_gt_workspace_bytes(n_views, G) bytes.
 */
typedef struct dafne_train_view {
    const uint8_t* d_src;
    int32_t h, w, layout_hwc;
    int32_t left, up, win_h, win_w;
    int32_t hflip, vflip;
    int32_t new_h, new_w, rot;
} dafne_train_view;
size_t dafne_train_views_workspace_bytes(const dafne_train_view* views, int n_views);
int dafne_train_views_u8_hip(const dafne_train_view* views, int n_views, int cap_h, int cap_w, uint8_t* d_out, int32_t* d_valid_hw,
                             void* d_ws, size_t ws_bytes, void* stream);
size_t dafne_train_gt_workspace_bytes(int n_views, int G);
int dafne_train_gt_hip(const dafne_train_view* views, int n_views, const float* d_corners_in, const int32_t* d_classes_in,
                       const int32_t* d_offsets_in, int G, int sort, float* d_corners, float* d_hbox, float* d_area,
                       int32_t* d_classes, int32_t* d_offsets_out, int32_t* d_src, void* d_ws, size_t ws_bytes, void* stream);

/*
 * SGD step on the device, packed compute copies written in place (csrc/solver_kernels.h; DESIGN row F14).  One launch updates every
 * tensor of a table.  Per element, in fp32 (torch.optim.SGD with momentum, dampening 0, no Nesterov, bit for bit):
 *     g'  = weight_decay == 0 ? g : fmaf(weight_decay, p, g)
 *     buf = first_step ? g' : (momentum * buf) + g'          two roundings, not fused
 *     p   = fmaf(-lr_t, buf, p)                              lr_t = (float)(lr * lr_factor), the product in double
 *     g   = 0                                                when zero_grad
 * d_p / d_g / d_buf hold n fp32 each (d_buf is not read on the first step).  `form` says which compute copy follows the new p:
 *   DAFNE_SGD_NONE  none.
 *   DAFNE_SGD_F32   d_copy[i] = p[i], or p[i] + d_addend[i] (fp32, one rounding) when d_addend is given: a convolution bias at
 *                   its row offset inside pack_conv's [Cout_pad] bias (the caller passes the offset pointer; padding rows are
 *                   not touched), a GroupNorm affine, a level scale into the buffer the host reads back.
 *   DAFNE_SGD_CONV  p is an OIHW weight [Cout, Cin, KH, KW], Cin % 64 == 0, KH * KW <= 9.  Rounded to bf16 (nearest even on
 *                   the bits as tensor.to(bfloat16): subnormals kept, NaN -> 0x7FC0) it goes to rows row0 .. row0 + Cout of the
 *                   packed matrix d_plain [rows, K] bf16, K = Cin * KH * KW, column (c / 64) * 64 * KH * KW + (kh * KW + kw) * 64 +
 *                   c % 64 (engine.pack_conv), and to every fragment-major form given (rows % 256 == 0 then), all in 16-byte
 *                   groups g = 8 columns 8 * kg .. + 8 of row r:
 *                     d_frag, d_wr [rows/256][8 waves][K/16][2][32 rows][8]: group ((((r >> 5) * (K/16) + kg / 2) * 2 + kg % 2) * 32 +
 *                       r % 32)  (engine.pack_conv3x3_frag / pack_conv_frag);
 *                     d_frag16 [rows/256][8 waves][K/32][2][4][16 rows][8]: group (((((r >> 5) * (K/32) + kg / 4) * 2 + (r >> 4) % 2) *
 *                       4 + kg % 4) * 16 + r % 16)  (engine.pack_conv3x3_frag16).
 *                   Two tensors may share one packed matrix at different row0 (corners_pred rows 0..7, ctrness row 8).  All
 *                   pointers of a CONV tensor are 16-byte aligned.
 * The table: dafne_sgd_table_build writes into HOST memory the image the kernel reads -- the n_tensors descriptors, then one
 * 16-byte entry per chunk (16 rows x one 64-channel slab of a CONV tensor; 1024 elements otherwise; dafne_sgd_num_chunks of
 * them, the launch's workgroups) -- dafne_sgd_table_bytes bytes.  The caller uploads it once, 16-byte aligned, and again only
 * when a descriptor changes.  dafne_sgd_step_hip takes the same HOST descriptors (checked at every call) and the device image.
 * A descriptor the kernel cannot serve -- a NULL d_p / d_g / d_buf / d_copy / d_plain, n <= 0 or not Cout * Cin * KH * KW, an
 * unknown form, rows outside the packed matrix, a misaligned pointer (DAFNE_E_INVALID), Cin % 64 != 0, more than 9 taps, a
 * fragment form on a matrix that is no multiple of 256 rows (DAFNE_E_UNSUPPORTED) -- makes every call here fail (num_chunks:
 * -1, table_bytes: 0) with the message set; nothing is launched and no buffer changes.  Vector stores only, every output
 * element has one writer: equal bits from run to run.
 */
#define DAFNE_SGD_NONE 0
#define DAFNE_SGD_F32 1
#define DAFNE_SGD_CONV 2
typedef struct dafne_sgd_tensor {
    float* d_p;                   /* master parameter, n fp32 */
    float* d_g;                   /* gradient */
    float* d_buf;                 /* momentum buffer */
    int64_t n;
    double lr_factor;             /* lr_t = (float)(lr * lr_factor) */
    float weight_decay;
    int32_t form;                 /* DAFNE_SGD_* */
    float* d_copy;                /* F32: the fp32 compute copy */
    const float* d_addend;        /* F32: optional, copy = p + addend */
    void* d_plain;                /* CONV: packed bf16 matrix [rows, K] (row 0) */
    void* d_frag;                 /* CONV: optional fragment-major forms of the WHOLE matrix */
    void* d_frag16;
    void* d_wr;
    int32_t Cout, Cin, KH, KW;
    int32_t row0, rows;           /* first row of this tensor in the packed matrix; rows of that matrix (Cout_pad) */
    int32_t reserved[2];
} dafne_sgd_tensor;
int dafne_sgd_num_chunks(const dafne_sgd_tensor* tensors, int n_tensors);
size_t dafne_sgd_table_bytes(const dafne_sgd_tensor* tensors, int n_tensors);
int dafne_sgd_table_build(const dafne_sgd_tensor* tensors, int n_tensors, void* h_table, size_t table_bytes);
int dafne_sgd_step_hip(const dafne_sgd_tensor* tensors, int n_tensors, const void* d_table, size_t table_bytes, double lr,
                       double momentum, int first_step, int zero_grad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DAFNE_AMD_H */
