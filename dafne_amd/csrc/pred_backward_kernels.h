// Back through the finished regressions of DAFNeHead.forward (dafne.py:394-411) -- included at the end of decode.hip
// (-ffp-contract=off, no packed fp32), next to targets_kernels.h whose loss backward differentiates with respect to them:
//
//     center-to-corner   reg = (center.repeat(4) + delta) * s_l      center_reg = center * s_l
//     direct / offset    reg = delta * s_l
//
//   g_delta  = s g_reg                                                     (straight into channels 0..7 of the fused
//                                                                           [delta8|ctrness] gradient; channel 8 = g_ctrness)
//   g_center = s (sum over the four corners of g_reg + g_center_reg)
//   g_scale  = sum g_reg (center.repeat(4) + delta) + sum g_center_reg center      one fp64 number per level
//
// Every value is formed in fp64 from the fp32 inputs and rounded once.  g_scale: one thread per pixel, the 256 terms of a
// workgroup are added by a fixed tree, the workgroups' partials of a level by a second kernel in a fixed order: no atomics,
// equal bits from run to run.
#pragma once

namespace {
namespace uncook {

constexpr int kMaxLv = 8;
constexpr int kThreads = 256;

struct Lv {
    const float* g_reg; const float* g_creg; const float* g_ctr; const float* delta; const float* center;
    float* g_delta; float* g_center;
    int g_reg_ps, g_creg_ps, g_ctr_ps, delta_ps, center_ps, g_delta_ps, g_center_ps;
    int npx, block0;
    float scale;
};

struct Dev {
    Lv lv[kMaxLv];
    int n_levels;
    double* partial;    // [blocks]
};

__global__ void __launch_bounds__(kThreads) uncook_kernel(Dev D) {
    __shared__ double red[kThreads];
    int l = 0;
#pragma unroll
    for (int k = 1; k < kMaxLv; k++)
        if (k < D.n_levels && (int)blockIdx.x >= D.lv[k].block0) l = k;
    const Lv& L = D.lv[l];
    const int px = ((int)blockIdx.x - L.block0) * kThreads + (int)threadIdx.x;
    double term = 0.0;
    if (px < L.npx) {
        const size_t p = (size_t)px;
        const double s = (double)L.scale;
        double g[8], sx = 0.0, sy = 0.0;
#pragma unroll
        for (int k = 0; k < 8; k++) g[k] = (double)L.g_reg[p * L.g_reg_ps + k];
        double cx = 0.0, cy = 0.0;
        if (L.center) {
            cx = (double)L.center[p * L.center_ps];
            cy = (double)L.center[p * L.center_ps + 1];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double d = (double)L.delta[p * L.delta_ps + k];
            term += g[k] * (((k & 1) ? cy : cx) + d);
            if (k & 1) sy += g[k];
            else sx += g[k];
            L.g_delta[p * L.g_delta_ps + k] = (float)(g[k] * s);
        }
        if (L.g_ctr) L.g_delta[p * L.g_delta_ps + 8] = L.g_ctr[p * L.g_ctr_ps];
        if (L.center) {
            const double gx = (double)L.g_creg[p * L.g_creg_ps], gy = (double)L.g_creg[p * L.g_creg_ps + 1];
            term += gx * cx + gy * cy;
            L.g_center[p * L.g_center_ps] = (float)(s * (sx + gx));
            L.g_center[p * L.g_center_ps + 1] = (float)(s * (sy + gy));
        }
    }
    red[threadIdx.x] = term;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) D.partial[blockIdx.x] = red[0];
}

// one workgroup of 64 lanes per level: lane j adds partials j, j + 64, ... in order, lane 0 adds the 64 lane sums in order
__global__ void __launch_bounds__(64) uncook_scale_kernel(Dev D, int total_blocks, double* g_scale) {
    __shared__ double red[64];
    const int l = (int)blockIdx.x;
    const int b0 = D.lv[l].block0, b1 = l + 1 < D.n_levels ? D.lv[l + 1].block0 : total_blocks;
    double s = 0.0;
    for (int b = b0 + (int)threadIdx.x; b < b1; b += 64) s += D.partial[b];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < 64; k++) t += red[k];
        g_scale[l] = t;
    }
}

// -> DAFNE_OK with D filled and *nb = the number of workgroups, or the refusal
int build(const dafne_uncook_level* levels, int n_levels, int n_images, Dev& D, int* nb) {
    *nb = 0;
    if (!levels || n_levels < 1 || n_levels > kMaxLv || n_images < 1)
        return dafne::fail(DAFNE_E_INVALID, "head_uncook_backward: bad level table / image count");
    long long blocks = 0;
    for (int l = 0; l < n_levels; l++) {
        const dafne_uncook_level& s = levels[l];
        const bool c2c = levels[0].d_center != nullptr, ctr = levels[0].d_g_ctrness != nullptr;
        if (!s.d_g_reg || !s.d_delta || !s.d_g_delta || s.H < 1 || s.W < 1 || (s.d_center != nullptr) != c2c ||
            (s.d_g_ctrness != nullptr) != ctr || (c2c && (!s.d_g_center_reg || !s.d_g_center)) || (!c2c && (s.d_g_center_reg || s.d_g_center)))
            return dafne::fail(DAFNE_E_INVALID, "head_uncook_backward: level %d: null or inconsistent pointers", l);
        if (s.g_reg_ps < 8 || s.delta_ps < 8 || s.g_delta_ps < (ctr ? 9 : 8) || (c2c && (s.center_ps < 2 || s.g_center_reg_ps < 2 || s.g_center_ps < 2)) ||
            (ctr && s.g_ctrness_ps < 1))
            return dafne::fail(DAFNE_E_INVALID, "head_uncook_backward: level %d: pixel stride too small", l);
        const long long npx = (long long)n_images * s.H * s.W;
        if (npx > 0x7fffffffll - kThreads) return dafne::fail(DAFNE_E_UNSUPPORTED, "head_uncook_backward: level %d has %lld pixels", l, npx);
        Lv& o = D.lv[l];
        o.g_reg = s.d_g_reg; o.g_creg = s.d_g_center_reg; o.g_ctr = s.d_g_ctrness; o.delta = s.d_delta; o.center = s.d_center;
        o.g_delta = s.d_g_delta; o.g_center = s.d_g_center;
        o.g_reg_ps = s.g_reg_ps; o.g_creg_ps = s.g_center_reg_ps; o.g_ctr_ps = s.g_ctrness_ps; o.delta_ps = s.delta_ps;
        o.center_ps = s.center_ps; o.g_delta_ps = s.g_delta_ps; o.g_center_ps = s.g_center_ps;
        o.npx = (int)npx; o.block0 = (int)blocks; o.scale = s.scale;
        blocks += (npx + kThreads - 1) / kThreads;
        if (blocks > 0x7fffffffll) return dafne::fail(DAFNE_E_UNSUPPORTED, "head_uncook_backward: too many pixels");
    }
    D.n_levels = n_levels;
    D.partial = nullptr;
    *nb = (int)blocks;
    return DAFNE_OK;
}

}  // namespace uncook
}  // namespace

extern "C" {

size_t dafne_head_uncook_backward_workspace_bytes(const dafne_uncook_level* levels, int n_levels, int n_images) {
    uncook::Dev D;
    int nb = 0;
    if (uncook::build(levels, n_levels, n_images, D, &nb)) return 0;
    return (size_t)nb * sizeof(double);
}

int dafne_head_uncook_backward_hip(const dafne_uncook_level* levels, int n_levels, int n_images, double* d_g_scale, void* d_ws,
                                   size_t ws_bytes, void* stream) {
    uncook::Dev D;
    int nb = 0;
    if (int rc = uncook::build(levels, n_levels, n_images, D, &nb)) return rc;
    if (!d_g_scale || !d_ws) return dafne::fail(DAFNE_E_INVALID, "head_uncook_backward: null pointer");
    if (ws_bytes < (size_t)nb * sizeof(double)) return dafne::fail(DAFNE_E_WORKSPACE, "head_uncook_backward: workspace %zu < %zu", ws_bytes, (size_t)nb * sizeof(double));
    D.partial = static_cast<double*>(d_ws);
    hipLaunchKernelGGL(uncook::uncook_kernel, dim3((unsigned)nb), dim3(uncook::kThreads), 0, (hipStream_t)stream, D);
    if (int rc = dafne::check_launch("head_uncook_backward")) return rc;
    hipLaunchKernelGGL(uncook::uncook_scale_kernel, dim3((unsigned)n_levels), dim3(64), 0, (hipStream_t)stream, D, nb, d_g_scale);
    return dafne::check_launch("head_uncook_backward (scales)");
}

}  // extern "C"
