// Target assignment, loss values and the losses' gradients with respect to the head outputs, of DAFNeOutputs, for gfx950.
//
//   assign_kernel    compute_targets_for_locations + _get_ground_truth's stride division
//                    (dafne/modeling/dafne/dafne_outputs.py:252-503): one thread per (image, location), the image's
//                    boxes staged through LDS in chunks of kChunk, a running (min area, first index) carried across
//                    the chunks (= the reference's min(dim=1) over its dense [K, G] matrix: the first index wins a
//                    tie, index 0 wins when every entry is INF).  Locations are regenerated (dafne.py:37-44).
//                    fp32, every operation singly and in the reference's order: the unit is compiled with
//                    -ffp-contract=off; sqrtf and the division operator are the correctly rounded forms (hipcc's default
//                    -fhip-fp32-correctly-rounded-divide-sqrt; this toolchain's __fsqrt_rn is the native approximation).
//   loss_kernel      dafne_losses (:620-731) with ModulatedEightPointLoss / SmoothL1Loss
//                    (dafne/modeling/losses/smooth_l1.py) and the sigmoid focal loss, every term in fp64 from the fp32
//                    inputs; per-workgroup partial sums (a fixed LDS tree) go to the workspace
//   loss_final       one workgroup adds the partial sums in index order and takes the data-dependent branches
//                    (max(num_pos, 1), max(sum ctr, 1e-6), "weights only if their sum is > 0", num_pos == 0)
//   loss_grad        the derivative of those values with respect to the COOKED inputs (described where it is defined)
// No floating-point atomics anywhere: two runs give equal bits.
//
// Output order of both kernels (and of the reference's losses(), :527): level first, then image, then location --
// position p = n_images * (locations of the levels before l) + image * H_l * W_l + location.
//
// This text is compiled as part of decode.hip (its last #include): one matrix-free translation unit with -ffp-contract=off
// -fno-slp-vectorize, under the static packed-fp32 rule that unit is held to (tests/test_packed_fp32.py).
#pragma once
#include "common.h"
#include "sort_quad.h"

namespace {
namespace targets {

constexpr int kMaxLv = 8;
constexpr int kChunk = 64;      // boxes per LDS chunk (16 words each: corners 8, hbox 4, area, 3 unused)
constexpr int kThreads = 256;
constexpr float kInf = 100000000.0f;   // INF of dafne_outputs.py:19, exact in fp32
constexpr int kSums = 8;        // focal, corners weighted / plain, center weighted / plain, centerness BCE, sum of centerness, positives

struct AssignDev {
    int n_images, n_levels, n_classes, flags, K, n_gt;
    int W[kMaxLv], stride[kMaxLv], koff[kMaxLv + 1];
    float lo[kMaxLv], hi[kMaxLv], rad[kMaxLv];
    const float* corners;
    const float* hbox;
    const float* area;
    const int* cls;
    const int* offsets;
    int* label;
    int* tind;
    float* tc;
    float* tl;
    float* ta;
};

// 1/2 * |cross(a - loc, b - loc)|  (area_triangle, :101-106)
__device__ __forceinline__ float tri_area(float ax, float ay, float bx, float by, float x, float y) {
    const float x0 = ax - x, x1 = ay - y, y0 = bx - x, y1 = by - y;
    return 0.5f * fabsf(x0 * y1 - x1 * y0);
}

// dist_point_to_line (:53-64) from (x0, y0) to the line through (x1, y1), (x2, y2)
__device__ __forceinline__ float point_line(float x1, float y1, float x2, float y2, float x0, float y0) {
    const float dy = y2 - y1, dx = x2 - x1;
    const float nom = fabsf(((dy * x0 - dx * y0) + x2 * y1) - y2 * x1);
    const float den = sqrtf(dy * dy + dx * dx);
    return nom / den;
}

__global__ void __launch_bounds__(kThreads) assign_kernel(AssignDev P) {
    __shared__ float s_box[kChunk][16];
    const int img = blockIdx.y;
    const int tid = threadIdx.x;
    const int k_raw = blockIdx.x * kThreads + tid;
    const bool live = k_raw < P.K;
    const int k = live ? k_raw : P.K - 1;
    int l = 0;
#pragma unroll
    for (int j = 1; j < kMaxLv; j++)
        if (j < P.n_levels && k >= P.koff[j]) l = j;
    const int loc = k - P.koff[l];
    const int Kl = P.koff[l + 1] - P.koff[l];
    const int st = P.stride[l];
    const float x = (float)((loc % P.W[l]) * st) + (float)(st / 2);
    const float y = (float)((loc / P.W[l]) * st) + (float)(st / 2);
    const size_t p = (size_t)P.n_images * P.koff[l] + (size_t)img * Kl + loc;

    int g0 = P.offsets[img], g1 = P.offsets[img + 1];
    g0 = min(max(g0, 0), P.n_gt);
    g1 = min(max(g1, g0), P.n_gt);
    const int G = g1 - g0;
    if (G == 0) {     // :375-381 (uniform over the block: no barrier is skipped by a part of it)
        if (live) {
            P.label[p] = P.n_classes;
            P.tind[p] = -1;
#pragma unroll
            for (int q = 0; q < 8; q++) P.tc[p * 8 + q] = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; q++) { P.tl[p * 4 + q] = 0.0f; P.ta[p * 4 + q] = 0.0f; }
        }
        return;
    }
    const bool center_sample = P.flags & DAFNE_TGT_CENTER_SAMPLE;
    const bool cs_only = P.flags & DAFNE_TGT_CENTER_SAMPLE_ONLY;
    const bool combine = P.flags & DAFNE_TGT_COMBINE_CENTER_SAMPLE;
    const bool box_check = P.flags & DAFNE_TGT_IN_BOX_CHECK;
    const bool size_filter = P.flags & DAFNE_TGT_LEVEL_SIZE_FILTERING;
    // get_sample_region's early return (:322): center_x[..., 0].sum() == 0, K copies of the first box's center -- zero exactly
    // when that center is zero -- gives an all-false mask for the whole image
    const bool cs_none = (P.hbox[(size_t)g0 * 4 + 0] + P.hbox[(size_t)g0 * 4 + 2]) * 0.5f == 0.0f;
    const float rad = P.rad[l], lo = P.lo[l], hi = P.hi[l];

    float best = 0.0f;
    int bi = 0;
    for (int c0 = 0; c0 < G; c0 += kChunk) {
        const int nb = min(kChunk, G - c0);
        __syncthreads();
        for (int e = tid; e < nb * 16; e += kThreads) {
            const int b = e >> 4, f = e & 15;
            const size_t g = (size_t)(g0 + c0 + b);
            float v = 0.0f;
            if (f < 8) v = P.corners[g * 8 + f];
            else if (f < 12) v = P.hbox[g * 4 + (f - 8)];
            else if (f == 12) v = P.area[g];
            s_box[b][f] = v;
        }
        __syncthreads();
        if (!live) continue;
        for (int b = 0; b < nb; b++) {
            const float* B = s_box[b];
            const float b0 = B[8], b1 = B[9], b2 = B[10], b3 = B[11];
            const float lt = x - b0, tp = y - b1, rt = b2 - x, bt = b3 - y;       // :387-390
            bool in_cs;
            if (center_sample) {       // get_sample_region (:297-352), no bitmasks
                if (cs_none) {
                    in_cs = false;
                } else {
                    const float cx = (b0 + b2) * 0.5f, cy = (b1 + b3) * 0.5f;
                    const float xmin = cx - rad, ymin = cy - rad, xmax = cx + rad, ymax = cy + rad;
                    const float q0 = xmin > b0 ? xmin : b0;
                    const float q1 = ymin > b1 ? ymin : b1;
                    const float q2 = xmax > b2 ? b2 : xmax;
                    const float q3 = ymax > b3 ? b3 : ymax;
                    in_cs = (x - q0 > 0.0f) && (q2 - x > 0.0f) && (y - q1 > 0.0f) && (q3 - y > 0.0f);
                }
            } else {
                in_cs = lt > 0.0f && tp > 0.0f && rt > 0.0f && bt > 0.0f;          // :434
            }
            bool in_box = in_cs;
            if (!cs_only) {            // is_in_quadrilateral (:109-119)
                const float sum = ((tri_area(B[0], B[1], B[2], B[3], x, y) + tri_area(B[2], B[3], B[4], B[5], x, y)) +
                                   tri_area(B[4], B[5], B[6], B[7], x, y)) + tri_area(B[6], B[7], B[0], B[1], x, y);
                const bool in_q = !(sum > (B[12] + 1e-3f));
                in_box = combine ? (in_cs && in_q) : in_q;
            }
            float mx = lt;             // :460-464
            mx = tp > mx ? tp : mx;
            mx = rt > mx ? rt : mx;
            mx = bt > mx ? bt : mx;
            const bool cared = mx >= lo && mx <= hi;
            float a = B[12];
            if (box_check && !in_box) a = kInf;
            if (size_filter && !cared) a = kInf;
            const int gi = c0 + b;
            if (gi == 0 || a < best) { best = a; bi = gi; }
        }
    }
    if (!live) return;
    const size_t g = (size_t)(g0 + bi);
    float c[8], h[4];
#pragma unroll
    for (int q = 0; q < 8; q++) c[q] = P.corners[g * 8 + q];
#pragma unroll
    for (int q = 0; q < 4; q++) h[q] = P.hbox[g * 4 + q];
    float tc[8], tl[4], ta[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        tc[2 * q] = c[2 * q] - x;
        tc[2 * q + 1] = c[2 * q + 1] - y;
        const int n = (q + 1) & 3;
        ta[q] = point_line(c[2 * q], c[2 * q + 1], c[2 * n], c[2 * n + 1], x, y);
    }
    tl[0] = x - h[0]; tl[1] = y - h[1]; tl[2] = h[2] - x; tl[3] = h[3] - y;
    if (P.flags & DAFNE_TGT_FPN_STRIDE_NORM) {      // :289-293
        const float s = (float)st;
#pragma unroll
        for (int q = 0; q < 8; q++) tc[q] = tc[q] / s;
#pragma unroll
        for (int q = 0; q < 4; q++) { tl[q] = tl[q] / s; ta[q] = ta[q] / s; }
    }
    P.label[p] = best == kInf ? P.n_classes : P.cls[g];      // :488-489
    P.tind[p] = g0 + bi;                                     // :485 (num_targets = boxes of the images before)
#pragma unroll
    for (int q = 0; q < 8; q++) P.tc[p * 8 + q] = tc[q];
#pragma unroll
    for (int q = 0; q < 4; q++) { P.tl[p * 4 + q] = tl[q]; P.ta[p * 4 + q] = ta[q]; }
}

// ------------------------------------------------------------------------------------------------ losses
struct LossLv {
    const float* logits;
    const float* delta;
    const float* center;
    const float* ctr;
    int lps, dps, cps, tps;
    float scale;
};

struct LossDev {
    LossLv lv[kMaxLv];
    int n_levels, C, P, flags;
    int poff[kMaxLv + 1];     // first position of each level
    double alpha, gamma, beta, ctr_expo;
    const int* label;
    const float* tc;
    const float* tl;
    const float* ta;
    double* partial;          // [blocks][kSums]
    float* ctr_out;           // [P] or NULL
};

__device__ __forceinline__ int level_of(const LossDev& D, int p) {
    int l = 0;
#pragma unroll
    for (int j = 1; j < kMaxLv; j++)
        if (j < D.n_levels && p >= D.poff[j]) l = j;
    return l;
}

// BCEWithLogits(x, t) = max(x, 0) - x t + log(1 + exp(-|x|))
__device__ __forceinline__ double bce_logits(double x, double t) {
    return (fmax(x, 0.0) - x * t) + log1p(exp(-fabs(x)));
}

// fvcore's smooth_l1_loss on n = |input - target|, then the optional log1p (smooth_l1.py:23-28, 49-67, 88-91)
__device__ __forceinline__ double sl1(double n, double beta, bool logspace) {
    double v = n;
    if (!(beta < 1e-5)) v = n < beta ? 0.5 * n * n / beta : n - 0.5 * beta;
    return logspace ? log1p(v) : v;
}

// centerness target of a positive (compute_ctrness_targets, :79-93): the ratio in fp32 as the reference forms it, the power in
// fp64, NaN -> 0; 1 without centerness
__device__ __forceinline__ double ctr_target(const LossDev& D, int p) {
    if (!(D.flags & (DAFNE_LOSS_CTR_PLAIN | DAFNE_LOSS_CTR_ORIENTED))) return 1.0;
    const float* src = (D.flags & DAFNE_LOSS_CTR_PLAIN) ? D.tl : D.ta;
    const float s0 = src[(size_t)p * 4 + 0], s1 = src[(size_t)p * 4 + 1], s2 = src[(size_t)p * 4 + 2], s3 = src[(size_t)p * 4 + 3];
    const float lrmin = s2 < s0 ? s2 : s0, lrmax = s2 > s0 ? s2 : s0;
    const float tbmin = s3 < s1 ? s3 : s1, tbmax = s3 > s1 ? s3 : s1;
    const float r = (lrmin / lrmax) * (tbmin / tbmax);
    const double cw = pow((double)r, D.ctr_expo);
    return cw != cw ? 0.0 : cw;
}

__global__ void __launch_bounds__(kThreads) loss_kernel(LossDev D) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * kThreads;
    const int npos = min(kThreads, D.P - p0);
    double acc[kSums];
#pragma unroll
    for (int q = 0; q < kSums; q++) acc[q] = 0.0;

    // sigmoid focal loss over every (position, class) of this block's positions
    for (int e = tid; e < npos * D.C; e += kThreads) {
        const int q = e / D.C, c = e - q * D.C;
        const int p = p0 + q;
        const int l = level_of(D, p);
        const size_t rem = (size_t)(p - D.poff[l]);
        const double x = (double)D.lv[l].logits[rem * D.lv[l].lps + c];
        const double t = D.label[p] == c ? 1.0 : 0.0;
        const double pr = 1.0 / (1.0 + exp(-x));
        const double ce = bce_logits(x, t);
        const double pt = pr * t + (1.0 - pr) * (1.0 - t);
        double v = ce * pow(1.0 - pt, D.gamma);
        if (D.alpha >= 0.0) v = (D.alpha * t + (1.0 - D.alpha) * (1.0 - t)) * v;
        acc[0] += v;
    }

    // regression / centerness terms: one thread per position, positives only
    const int p = p0 + tid;
    float ctr_f = 0.0f;
    if (tid < npos && D.label[p] != D.C) {
        const int l = level_of(D, p);
        const LossLv& L = D.lv[l];
        const size_t rem = (size_t)(p - D.poff[l]);
        const bool cooked = D.flags & DAFNE_LOSS_COOKED;
        const bool logspace = D.flags & DAFNE_LOSS_LOGSPACE;
        float q[8];
        if (cooked) {
#pragma unroll
            for (int k = 0; k < 8; k++) q[k] = L.delta[rem * L.dps + k];
        } else if (L.center) {        // (center.repeat(4) + delta) * scale, fp32 as DAFNeHead.forward computes it (dafne.py:405-411)
#pragma unroll
            for (int k = 0; k < 8; k++) q[k] = (L.center[rem * L.cps + (k & 1)] + L.delta[rem * L.dps + k]) * L.scale;
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) q[k] = L.delta[rem * L.dps + k] * L.scale;
        }
        if (D.flags & DAFNE_LOSS_SORT_CORNERS) dafne::sort_quad(q);
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) t[k] = D.tc[(size_t)p * 8 + k];
        const double cw = ctr_target(D, p);
        ctr_f = (float)cw;
        // corners (ModulatedEightPointLoss / SmoothL1Loss)
        double l0 = 0.0, l1 = 0.0, l2 = 0.0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double tk = (double)t[k];
            l0 += sl1(fabs((double)q[k] - tk), D.beta, logspace);
            l1 += sl1(fabs((double)q[(k + 2) & 7] - tk), D.beta, logspace);     // input[:, [1, 2, 3, 0]]
            l2 += sl1(fabs((double)q[(k + 6) & 7] - tk), D.beta, logspace);     // input[:, [3, 0, 1, 2]]
        }
        double lc = l0;
        if (D.flags & DAFNE_LOSS_MODULATION) {
            lc = l1 < lc ? l1 : lc;
            lc = l2 < lc ? l2 : lc;
        }
        acc[1] = lc * cw;
        acc[2] = lc;
        if (D.flags & DAFNE_LOSS_HAS_CENTER_REG) {
            const double tx = ((((double)t[0] + (double)t[2]) + (double)t[4]) + (double)t[6]) / 4.0;
            const double ty = ((((double)t[1] + (double)t[3]) + (double)t[5]) + (double)t[7]) / 4.0;
            float cx, cy;
            if (cooked) { cx = L.center[rem * L.cps]; cy = L.center[rem * L.cps + 1]; }
            else { cx = L.center[rem * L.cps] * L.scale; cy = L.center[rem * L.cps + 1] * L.scale; }
            const double le = sl1(fabs((double)cx - tx), D.beta, logspace) + sl1(fabs((double)cy - ty), D.beta, logspace);
            acc[3] = le * cw;
            acc[4] = le;
        }
        if (L.ctr) acc[5] = bce_logits((double)L.ctr[rem * L.tps], cw);
        acc[6] = cw;
        acc[7] = 1.0;
    }
    if (D.ctr_out && tid < npos) D.ctr_out[p] = ctr_f;

    // fixed-order tree per quantity
#pragma unroll
    for (int q = 0; q < kSums; q++) {
        __syncthreads();
        red[tid] = acc[q];
        __syncthreads();
        for (int s = kThreads / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (tid == 0) D.partial[(size_t)blockIdx.x * kSums + q] = red[0];
    }
}

struct FinalDev {
    const double* partial;
    int blocks, has_center, has_ctr;
    double lam_cls, lam_corners, lam_center, lam_ctr;
    double* out;     // [6]
};

__global__ void __launch_bounds__(64) loss_final_kernel(FinalDev F) {
    __shared__ double s[kSums];
    const int tid = threadIdx.x;
    if (tid < kSums) {
        double a = 0.0;
        for (int b = 0; b < F.blocks; b++) a += F.partial[(size_t)b * kSums + tid];
        s[tid] = a;
    }
    __syncthreads();
    if (tid != 0) return;
    const double num_pos = s[7];
    const double num_pos_avg = num_pos > 1.0 ? num_pos : 1.0;          // :630
    const double denorm = s[6] > 1e-6 ? s[6] : 1e-6;                   // :665
    const bool weighted = s[6] > 0.0;                                  // smooth_l1.py:31,105
    double corners = 0.0, center = 0.0, ctr = 0.0;
    if (num_pos > 0.0) {                                               // :668-709
        corners = (weighted ? s[1] : s[2]) / denorm;
        if (F.has_center) center = (weighted ? s[3] : s[4]) / denorm;
        if (F.has_ctr) ctr = s[5] / num_pos_avg;
    }
    F.out[0] = s[0] / num_pos_avg * F.lam_cls;
    F.out[1] = corners * F.lam_corners;
    F.out[2] = center * F.lam_center;
    F.out[3] = ctr * F.lam_ctr;
    F.out[4] = num_pos;
    F.out[5] = denorm;
}

int levels_ok(int n_images, int n_levels, const int* H, const int* W, long long* K_out) {
    if (n_images <= 0 || n_levels <= 0 || n_levels > kMaxLv) return 0;
    long long K = 0;
    for (int l = 0; l < n_levels; l++) {
        if (H[l] <= 0 || W[l] <= 0) return 0;
        K += (long long)H[l] * W[l];
    }
    *K_out = K;
    return 1;
}


int assign_targets(const dafne_target_params* prm, const float* d_gt_corners, const float* d_gt_hbox,
                             const float* d_gt_area, const int32_t* d_gt_class, const int32_t* d_gt_offsets, int n_gt,
                             int32_t* d_label, int32_t* d_target_ind, float* d_reg_corners, float* d_reg_ltrb,
                             float* d_reg_abcd, void* stream) {
    if (!prm || !d_gt_offsets || !d_label || !d_target_ind || !d_reg_corners || !d_reg_ltrb || !d_reg_abcd || n_gt < 0)
        return dafne::fail(DAFNE_E_INVALID, "assign_targets: bad args");
    if (n_gt > 0 && (!d_gt_corners || !d_gt_hbox || !d_gt_area || !d_gt_class))
        return dafne::fail(DAFNE_E_INVALID, "assign_targets: %d boxes but a null box array", n_gt);
    if (prm->flags & ~DAFNE_TGT_ALL_FLAGS) return dafne::fail(DAFNE_E_INVALID, "assign_targets: unknown flags 0x%x", prm->flags);
    long long K = 0;
    if (!levels_ok(prm->n_images, prm->n_levels, prm->H, prm->W, &K) || prm->n_classes <= 0)
        return dafne::fail(DAFNE_E_INVALID, "assign_targets: bad level table");
    if (K * prm->n_images * 8 >= (1ll << 31)) return dafne::fail(DAFNE_E_UNSUPPORTED, "assign_targets: more than 2^31 outputs");
    AssignDev P;
    P.n_images = prm->n_images; P.n_levels = prm->n_levels; P.n_classes = prm->n_classes; P.flags = prm->flags;
    P.K = (int)K; P.n_gt = n_gt;
    int off = 0;
    for (int l = 0; l < kMaxLv; l++) {
        const bool on = l < prm->n_levels;
        if (on && prm->stride[l] <= 0) return dafne::fail(DAFNE_E_INVALID, "assign_targets: stride %d", prm->stride[l]);
        P.W[l] = on ? prm->W[l] : 1; P.stride[l] = on ? prm->stride[l] : 1;
        P.lo[l] = on ? prm->size_lo[l] : 0.0f; P.hi[l] = on ? prm->size_hi[l] : 0.0f; P.rad[l] = on ? prm->radius[l] : 0.0f;
        P.koff[l] = off;
        if (on) off += prm->H[l] * prm->W[l];
    }
    P.koff[kMaxLv] = off;
    for (int l = prm->n_levels; l < kMaxLv; l++) P.koff[l] = off;
    P.corners = d_gt_corners; P.hbox = d_gt_hbox; P.area = d_gt_area; P.cls = d_gt_class; P.offsets = d_gt_offsets;
    P.label = d_label; P.tind = d_target_ind; P.tc = d_reg_corners; P.tl = d_reg_ltrb; P.ta = d_reg_abcd;
    hipLaunchKernelGGL(assign_kernel, dim3((unsigned)((K + kThreads - 1) / kThreads), (unsigned)prm->n_images), dim3(kThreads), 0,
                       (hipStream_t)stream, P);
    return dafne::check_launch("assign_targets");
}

int loss_blocks(const dafne_loss_params* prm, const dafne_level_desc* levels, long long* P_out) {
    if (!prm || !levels) return 0;
    int H[kMaxLv], W[kMaxLv];
    if (prm->n_levels <= 0 || prm->n_levels > kMaxLv) return 0;
    for (int l = 0; l < prm->n_levels; l++) { H[l] = levels[l].H; W[l] = levels[l].W; }
    long long K = 0;
    if (!levels_ok(prm->n_images, prm->n_levels, H, W, &K)) return 0;
    const long long P = K * prm->n_images;
    if (prm->n_classes <= 0 || P * 8 >= (1ll << 31) || (long long)kThreads * prm->n_classes >= (1ll << 31)) return 0;
    *P_out = P;
    return (int)((P + kThreads - 1) / kThreads);
}

size_t losses_workspace_bytes(const dafne_loss_params* prm, const dafne_level_desc* levels) {
    long long P = 0;
    const int nb = loss_blocks(prm, levels, &P);
    return nb ? dafne::align_up((size_t)nb * kSums * sizeof(double), 256) : 0;
}

// The level table and the scalars of LossDev, with the checks of every level: shared by losses and losses_backward.
int fill_loss_dev(const char* who, const dafne_loss_params* prm, const dafne_level_desc* levels, const int32_t* d_label,
                  const float* d_reg_corners, const float* d_reg_ltrb, const float* d_reg_abcd, long long Pn, LossDev& D) {
    const bool has_center = prm->flags & DAFNE_LOSS_HAS_CENTER_REG;
    const bool has_ctr = prm->flags & (DAFNE_LOSS_CTR_PLAIN | DAFNE_LOSS_CTR_ORIENTED);
    D.n_levels = prm->n_levels; D.C = prm->n_classes; D.P = (int)Pn; D.flags = prm->flags;
    int off = 0;
    for (int l = 0; l < kMaxLv; l++) {
        D.poff[l] = off;
        if (l < prm->n_levels) {
            const dafne_level_desc& s = levels[l];
            if (!s.d_logits || !s.d_delta || (has_center && !s.d_center) || (has_ctr && !s.d_ctrness))
                return dafne::fail(DAFNE_E_INVALID, "%s: level %d lacks an input the configuration reads", who, l);
            if (s.logits_ps < prm->n_classes || s.delta_ps < 8 || (s.d_center && s.center_ps < 2) || (s.d_ctrness && s.ctrness_ps < 1))
                return dafne::fail(DAFNE_E_INVALID, "%s: level %d pixel stride too small", who, l);
            D.lv[l] = LossLv{s.d_logits, s.d_delta, s.d_center, has_ctr ? s.d_ctrness : nullptr, s.logits_ps, s.delta_ps, s.center_ps,
                             s.ctrness_ps, s.scale};
            off += prm->n_images * s.H * s.W;
        } else {
            D.lv[l] = LossLv{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0.0f};
        }
    }
    D.poff[kMaxLv] = off;
    D.alpha = prm->alpha; D.gamma = prm->gamma; D.beta = prm->beta;
    D.ctr_expo = (double)(float)(1.0 / prm->ctr_alpha);      // torch raises an fp32 tensor to the fp32 value of 1 / alpha
    D.label = d_label; D.tc = d_reg_corners; D.tl = d_reg_ltrb; D.ta = d_reg_abcd;
    D.partial = nullptr; D.ctr_out = nullptr;
    return 0;
}

int losses(const dafne_loss_params* prm, const dafne_level_desc* levels, const int32_t* d_label,
                     const float* d_reg_corners, const float* d_reg_ltrb, const float* d_reg_abcd, double* d_out6,
                     float* d_ctr_targets, void* d_ws, size_t ws_bytes, void* stream) {
    long long Pn = 0;
    const int nb = loss_blocks(prm, levels, &Pn);
    if (!nb) return dafne::fail(DAFNE_E_INVALID, "losses: bad params / level table");
    if (!d_label || !d_reg_corners || !d_reg_ltrb || !d_reg_abcd || !d_out6) return dafne::fail(DAFNE_E_INVALID, "losses: null pointer");
    if (prm->flags & ~DAFNE_LOSS_ALL_FLAGS) return dafne::fail(DAFNE_E_INVALID, "losses: unknown flags 0x%x", prm->flags);
    if ((prm->flags & DAFNE_LOSS_CTR_PLAIN) && (prm->flags & DAFNE_LOSS_CTR_ORIENTED))
        return dafne::fail(DAFNE_E_INVALID, "losses: both centerness modes");
    if (!d_ws || ws_bytes < losses_workspace_bytes(prm, levels)) return dafne::fail(DAFNE_E_WORKSPACE, "losses: workspace too small");
    if (!(prm->ctr_alpha > 0.0)) return dafne::fail(DAFNE_E_INVALID, "losses: CENTERNESS_ALPHA %g", prm->ctr_alpha);
    const bool has_center = prm->flags & DAFNE_LOSS_HAS_CENTER_REG;
    const bool has_ctr = prm->flags & (DAFNE_LOSS_CTR_PLAIN | DAFNE_LOSS_CTR_ORIENTED);
    LossDev D;
    if (int rc = fill_loss_dev("losses", prm, levels, d_label, d_reg_corners, d_reg_ltrb, d_reg_abcd, Pn, D)) return rc;
    D.partial = static_cast<double*>(d_ws); D.ctr_out = d_ctr_targets;
    hipLaunchKernelGGL(loss_kernel, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, D);
    if (int rc = dafne::check_launch("losses")) return rc;
    FinalDev F{D.partial, nb, has_center ? 1 : 0, has_ctr ? 1 : 0, prm->lambda_cls, prm->lambda_corners, prm->lambda_center,
               prm->lambda_ctr, d_out6};
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, F);
    return dafne::check_launch("losses (final)");
}

// ------------------------------------------------------------------------------------------------ loss gradients
// The derivative of what loss_kernel / loss_final_kernel compute, with the conventions of the reference's autograd
// (dafne_outputs.py:620-731, smooth_l1.py): the minimum of the modulated loss sends its gradient to the FIRST of the equal
// shifts, sort_quadrilateral's selection sends none to the slots it leaves at zero, the centerness target is a constant.
//   loss_grad_state_kernel   re-adds the forward's partial sums of the centerness targets and of the positives in the
//                            forward's order (loss_final_kernel's loop), so that num_pos, the sum and "sum > 0" are the
//                            forward's own; two doubles in the workspace, no host read
//   loss_grad_kernel         one workgroup per kThreads positions as loss_kernel: the logits gradient flat over (position,
//                            class), the regression / centerness gradients one thread per position, zeros at non-positives.
// Every element has one writer and is written: no memset, no atomics, equal bits from run to run.
struct GradLv {
    float* logits;
    float* delta;
    float* center;
    float* ctr;
    int lps, dps, cps, tps;
};

struct GradDev {
    LossDev D;
    GradLv g[kMaxLv];
    const double* state;      // [2]: num_pos, sum of the centerness targets
    const double* grad_out;   // [4]: upstream factors of cls, corners, center, ctr
    double lam_cls, lam_corners, lam_center, lam_ctr;
};

__global__ void __launch_bounds__(64) loss_grad_state_kernel(const double* partial, int blocks, double* state) {
    const int tid = threadIdx.x;
    if (tid >= 2) return;
    const int q = tid == 0 ? 7 : 6;
    double a = 0.0;
    for (int b = 0; b < blocks; b++) a += partial[(size_t)b * kSums + q];
    state[tid] = a;
}

// d/dd of sl1(|d|): sign(d) * (n / beta below beta, 1 from beta on), divided by 1 + v in log space; sign(0) = 0
__device__ __forceinline__ double sl1_grad(double d, double beta, bool logspace) {
    const double n = fabs(d);
    const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    double v = n, dv = 1.0;
    if (!(beta < 1e-5)) {
        if (n < beta) { v = 0.5 * n * n / beta; dv = n / beta; }
        else v = n - 0.5 * beta;
    }
    if (logspace) dv = dv / (1.0 + v);
    return sg * dv;
}

__global__ void __launch_bounds__(kThreads) loss_grad_kernel(GradDev G) {
    const LossDev& D = G.D;
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * kThreads;
    const int npos = min(kThreads, D.P - p0);
    const double num_pos = G.state[0], csum = G.state[1];
    const double num_pos_avg = num_pos > 1.0 ? num_pos : 1.0;
    const double denorm = csum > 1e-6 ? csum : 1e-6;
    const bool weighted = csum > 0.0;

    if (G.g[0].logits) {
        const double f_cls = G.lam_cls * G.grad_out[0];
        for (int e = tid; e < npos * D.C; e += kThreads) {
            const int q = e / D.C, c = e - q * D.C;
            const int p = p0 + q;
            const int l = level_of(D, p);
            const size_t rem = (size_t)(p - D.poff[l]);
            const double x = (double)D.lv[l].logits[rem * D.lv[l].lps + c];
            const double t = D.label[p] == c ? 1.0 : 0.0;
            const double pr = 1.0 / (1.0 + exp(-x));
            const double pt = pr * t + (1.0 - pr) * (1.0 - t);
            const double om = 1.0 - pt;
            double g = pow(om, D.gamma) * (pr - t);
            if (D.gamma != 0.0) {
                const double ce = bce_logits(x, t);
                g = g - D.gamma * pow(om, D.gamma - 1.0) * ce * ((2.0 * t - 1.0) * pr * (1.0 - pr));
            }
            if (D.alpha >= 0.0) g = (D.alpha * t + (1.0 - D.alpha) * (1.0 - t)) * g;
            G.g[l].logits[rem * G.g[l].lps + c] = (float)(g / num_pos_avg * f_cls);
        }
    }

    if (tid >= npos) return;
    const int p = p0 + tid;
    const int l = level_of(D, p);
    const LossLv& L = D.lv[l];
    const GradLv& O = G.g[l];
    const size_t rem = (size_t)(p - D.poff[l]);
    float gq[8], gc0 = 0.0f, gc1 = 0.0f, gt = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++) gq[k] = 0.0f;
    if (D.label[p] != D.C && num_pos > 0.0) {
        const bool logspace = D.flags & DAFNE_LOSS_LOGSPACE;
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) t[k] = D.tc[(size_t)p * 8 + k];
        const double cw = ctr_target(D, p);
        const double w = (weighted ? cw : 1.0) / denorm;
        if (O.delta) {
            float q[8];
#pragma unroll
            for (int k = 0; k < 8; k++) q[k] = L.delta[rem * L.dps + k];
            int src[4] = {0, 1, 2, 3};
            if (D.flags & DAFNE_LOSS_SORT_CORNERS) dafne::sort_quad_src(q, src);
            int sh = 0;
            if (D.flags & DAFNE_LOSS_MODULATION) {      // loss_kernel's three sums and its choice
                double l0 = 0.0, l1 = 0.0, l2 = 0.0;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const double tk = (double)t[k];
                    l0 += sl1(fabs((double)q[k] - tk), D.beta, logspace);
                    l1 += sl1(fabs((double)q[(k + 2) & 7] - tk), D.beta, logspace);
                    l2 += sl1(fabs((double)q[(k + 6) & 7] - tk), D.beta, logspace);
                }
                double lc = l0;
                if (l1 < lc) { lc = l1; sh = 1; }
                if (l2 < lc) { lc = l2; sh = 2; }
            }
            const double f = w * (G.lam_corners * G.grad_out[1]);
            float gk[8];      // by target component k
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const float qs = sh == 0 ? q[k] : (sh == 1 ? q[(k + 2) & 7] : q[(k + 6) & 7]);
                gk[k] = (float)(sl1_grad((double)qs - (double)t[k], D.beta, logspace) * f);
            }
            float gs[8];      // by sorted slot j = (k + shift) & 7
#pragma unroll
            for (int j = 0; j < 8; j++) gs[j] = sh == 0 ? gk[j] : (sh == 1 ? gk[(j + 6) & 7] : gk[(j + 2) & 7]);
#pragma unroll
            for (int c = 0; c < 4; c++) {               // back through the sort: slot j came from corner src[j]
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (src[j] == c) { gq[2 * c] = gs[2 * j]; gq[2 * c + 1] = gs[2 * j + 1]; }
            }
        }
        if (O.center) {
            const double tx = ((((double)t[0] + (double)t[2]) + (double)t[4]) + (double)t[6]) / 4.0;
            const double ty = ((((double)t[1] + (double)t[3]) + (double)t[5]) + (double)t[7]) / 4.0;
            const double f = w * (G.lam_center * G.grad_out[2]);
            gc0 = (float)(sl1_grad((double)L.center[rem * L.cps] - tx, D.beta, logspace) * f);
            gc1 = (float)(sl1_grad((double)L.center[rem * L.cps + 1] - ty, D.beta, logspace) * f);
        }
        if (O.ctr) {
            const double x = (double)L.ctr[rem * L.tps];
            gt = (float)((1.0 / (1.0 + exp(-x)) - cw) / num_pos_avg * (G.lam_ctr * G.grad_out[3]));
        }
    }
    if (O.delta) {
#pragma unroll
        for (int k = 0; k < 8; k++) O.delta[rem * O.dps + k] = gq[k];
    }
    if (O.center) { O.center[rem * O.cps] = gc0; O.center[rem * O.cps + 1] = gc1; }
    if (O.ctr) O.ctr[rem * O.tps] = gt;
}

size_t losses_backward_workspace_bytes(const dafne_loss_params* prm, const dafne_level_desc* levels) {
    long long P = 0;
    return loss_blocks(prm, levels, &P) ? 256 : 0;
}

int losses_backward(const dafne_loss_params* prm, const dafne_level_desc* levels, const int32_t* d_label,
                    const float* d_reg_corners, const float* d_reg_ltrb, const float* d_reg_abcd, const void* d_fwd_ws,
                    size_t fwd_ws_bytes, const double* d_grad_out4, const dafne_level_grad* grads, void* d_ws, size_t ws_bytes,
                    void* stream) {
    long long Pn = 0;
    const int nb = loss_blocks(prm, levels, &Pn);
    if (!nb) return dafne::fail(DAFNE_E_INVALID, "losses_backward: bad params / level table");
    if (!d_label || !d_reg_corners || !d_reg_ltrb || !d_reg_abcd || !d_grad_out4 || !grads)
        return dafne::fail(DAFNE_E_INVALID, "losses_backward: null pointer");
    if (prm->flags & ~DAFNE_LOSS_ALL_FLAGS) return dafne::fail(DAFNE_E_INVALID, "losses_backward: unknown flags 0x%x", prm->flags);
    if ((prm->flags & DAFNE_LOSS_CTR_PLAIN) && (prm->flags & DAFNE_LOSS_CTR_ORIENTED))
        return dafne::fail(DAFNE_E_INVALID, "losses_backward: both centerness modes");
    if (!(prm->flags & DAFNE_LOSS_COOKED))
        return dafne::fail(DAFNE_E_UNSUPPORTED, "losses_backward: only the DAFNE_LOSS_COOKED form has a backward (the raw head "
                                                "outputs' Scale and center + delta chain is not differentiated)");
    if (!d_fwd_ws || fwd_ws_bytes < losses_workspace_bytes(prm, levels))
        return dafne::fail(DAFNE_E_WORKSPACE, "losses_backward: the forward's workspace is missing or too small");
    if (!d_ws || ws_bytes < losses_backward_workspace_bytes(prm, levels))
        return dafne::fail(DAFNE_E_WORKSPACE, "losses_backward: workspace too small");
    if (!(prm->ctr_alpha > 0.0)) return dafne::fail(DAFNE_E_INVALID, "losses_backward: CENTERNESS_ALPHA %g", prm->ctr_alpha);
    const bool has_center = prm->flags & DAFNE_LOSS_HAS_CENTER_REG;
    const bool has_ctr = prm->flags & (DAFNE_LOSS_CTR_PLAIN | DAFNE_LOSS_CTR_ORIENTED);
    GradDev G;
    if (int rc = fill_loss_dev("losses_backward", prm, levels, d_label, d_reg_corners, d_reg_ltrb, d_reg_abcd, Pn, G.D)) return rc;
    for (int l = 0; l < kMaxLv; l++) {
        if (l >= prm->n_levels) {
            G.g[l] = GradLv{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0};
            continue;
        }
        const dafne_level_grad& g = grads[l];
        if ((g.d_center && !has_center) || (g.d_ctrness && !has_ctr))
            return dafne::fail(DAFNE_E_INVALID, "losses_backward: level %d has a gradient for a term the configuration lacks", l);
        if (!g.d_logits != !grads[0].d_logits || !g.d_delta != !grads[0].d_delta || !g.d_center != !grads[0].d_center ||
            !g.d_ctrness != !grads[0].d_ctrness)
            return dafne::fail(DAFNE_E_INVALID, "losses_backward: level %d leaves out another set of gradients than level 0", l);
        if ((g.d_logits && g.logits_ps < prm->n_classes) || (g.d_delta && g.delta_ps < 8) || (g.d_center && g.center_ps < 2) ||
            (g.d_ctrness && g.ctrness_ps < 1))
            return dafne::fail(DAFNE_E_INVALID, "losses_backward: level %d gradient pixel stride too small", l);
        G.g[l] = GradLv{g.d_logits, g.d_delta, g.d_center, g.d_ctrness, g.logits_ps, g.delta_ps, g.center_ps, g.ctrness_ps};
    }
    double* state = static_cast<double*>(d_ws);
    G.state = state; G.grad_out = d_grad_out4;
    G.lam_cls = prm->lambda_cls; G.lam_corners = prm->lambda_corners; G.lam_center = prm->lambda_center; G.lam_ctr = prm->lambda_ctr;
    hipLaunchKernelGGL(loss_grad_state_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, static_cast<const double*>(d_fwd_ws), nb,
                       state);
    if (int rc = dafne::check_launch("losses_backward (state)")) return rc;
    hipLaunchKernelGGL(loss_grad_kernel, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, G);
    return dafne::check_launch("losses_backward");
}

}  // namespace targets
}  // namespace

extern "C" {

size_t dafne_losses_backward_workspace_bytes(const dafne_loss_params* prm, const dafne_level_desc* levels) {
    return targets::losses_backward_workspace_bytes(prm, levels);
}

int dafne_losses_backward_hip(const dafne_loss_params* prm, const dafne_level_desc* levels, const int32_t* d_label,
                              const float* d_reg_corners, const float* d_reg_ltrb, const float* d_reg_abcd, const void* d_fwd_ws,
                              size_t fwd_ws_bytes, const double* d_grad_out4, const dafne_level_grad* grads, void* d_ws,
                              size_t ws_bytes, void* stream) {
    return targets::losses_backward(prm, levels, d_label, d_reg_corners, d_reg_ltrb, d_reg_abcd, d_fwd_ws, fwd_ws_bytes, d_grad_out4,
                                    grads, d_ws, ws_bytes, stream);
}

int dafne_assign_targets_hip(const dafne_target_params* prm, const float* d_gt_corners, const float* d_gt_hbox,
                             const float* d_gt_area, const int32_t* d_gt_class, const int32_t* d_gt_offsets, int n_gt,
                             int32_t* d_label, int32_t* d_target_ind, float* d_reg_corners, float* d_reg_ltrb,
                             float* d_reg_abcd, void* stream) {
    return targets::assign_targets(prm, d_gt_corners, d_gt_hbox, d_gt_area, d_gt_class, d_gt_offsets, n_gt, d_label, d_target_ind,
                                   d_reg_corners, d_reg_ltrb, d_reg_abcd, stream);
}

size_t dafne_losses_workspace_bytes(const dafne_loss_params* prm, const dafne_level_desc* levels) {
    return targets::losses_workspace_bytes(prm, levels);
}

int dafne_losses_hip(const dafne_loss_params* prm, const dafne_level_desc* levels, const int32_t* d_label,
                     const float* d_reg_corners, const float* d_reg_ltrb, const float* d_reg_abcd, double* d_out6,
                     float* d_ctr_targets, void* d_ws, size_t ws_bytes, void* stream) {
    return targets::losses(prm, levels, d_label, d_reg_corners, d_reg_ltrb, d_reg_abcd, d_out6, d_ctr_targets, d_ws, ws_bytes,
                           stream);
}

}  // extern "C"
