// The ground truth of a batch of training views, for gfx950 (dafne_train_gt_hip): the coordinate side of the reference's
// augmentation list (tools/plain_train_net.py:229-256: hflip, vflip, resize, RandomRotation by quarter turns) and what
// DAFNeDatasetMapper (dafne/data/datasets/dafne_dataset_mapper.py:13-47) makes of the transformed polygons.
//
//   transform_kernel one thread per object.  The view of object g is the last v with offsets_in[v] <= g.  In fp64, every
//                    operation singly and in this order (the unit is compiled with -ffp-contract=off):
//                      1. x = win_w - x if hflip            2. y = win_h - y if vflip
//                      3. x = x * (new_w / win_w), y = y * (new_h / win_h)      (the ratio first: ResizeTransform.apply_coords)
//                      4. W, H = new_w, new_h; rot 1: (x, y) = (y, W - x); rot 2: (W - x, H - y); rot 3: (H - y, x)
//                         (np.rot90's permutation for coordinates whose pixel centres sit at i + 0.5)
//                      5. area = 0.5 |s1 - s2|, s1 = sum_i x_i y_(i-1), s2 = sum_i y_i x_(i-1) added in index order from 0.0
//                         (detectron2's polygon_area), rounded to fp32
//                      6. corners rounded to fp32 once; hbox = min / max of the fp32 corners; then sort_quad when `sort`
//                      7. kept: hbox width > 1e-5f and height > 1e-5f, both in fp32 (Boxes.nonempty)
//   count_kernel     one wavefront per view: kept rows (lane sums, xor-shuffle reduction)
//   scan_kernel      one wavefront: exclusive scan of the per-view counts -> offsets_out [n_views + 1]
//   write_kernel     one wavefront per view: a kept row's position = its view's offset + kept rows before it in the view
//                    (ballot + popcount).  Ordered, no atomics: equal bits from run to run.
//
// This text is compiled as part of decode.hip (its last #include), like targets_kernels.h: one matrix-free translation unit
// with -ffp-contract=off -fno-slp-vectorize under the static packed-fp32 rule (tests/test_packed_fp32.py).
#pragma once
#include "common.h"
#include "sort_quad.h"

namespace {
namespace train_views {

constexpr int kRecF = 13;        // 8 corners, 4 hbox, area

struct ViewGt {
    int32_t win_h, win_w, hflip, vflip, new_h, new_w, rot, reserved;
};

struct GtArgs {
    const ViewGt* views;
    const float* corners_in;     // [G, 8]
    const int32_t* offsets_in;   // [n_views + 1]
    float* recf;                 // [G, 13]
    int32_t* kept;               // [G]
    int n_views, G, sort;
};

__global__ void __launch_bounds__(256) transform_kernel(GtArgs a) {
    const long long gg = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gg >= a.G) return;
    const int g = (int)gg;
    if (g >= a.offsets_in[a.n_views]) return;
    int lo = 0, hi = a.n_views;          // the last view with offsets_in[v] <= g (empty views own no row)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (a.offsets_in[mid] <= g) lo = mid; else hi = mid;
    }
    const ViewGt v = a.views[lo];
    const double ww = (double)v.win_w, wh = (double)v.win_h, W = (double)v.new_w, H = (double)v.new_h;
    const double rx = W / ww, ry = H / wh;
    double x[4], y[4];
    for (int i = 0; i < 4; i++) {
        double px = (double)a.corners_in[(size_t)g * 8 + 2 * i], py = (double)a.corners_in[(size_t)g * 8 + 2 * i + 1];
        if (v.hflip) px = ww - px;
        if (v.vflip) py = wh - py;
        px = px * rx;
        py = py * ry;
        double qx = px, qy = py;
        if (v.rot == 1) { qx = py; qy = W - px; }
        if (v.rot == 2) { qx = W - px; qy = H - py; }
        if (v.rot == 3) { qx = H - py; qy = px; }
        x[i] = qx;
        y[i] = qy;
    }
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < 4; i++) {
        const int k = (i + 3) & 3;
        s1 = s1 + x[i] * y[k];
        s2 = s2 + y[i] * x[k];
    }
    float q[8];
    for (int i = 0; i < 4; i++) {
        q[2 * i] = (float)x[i];
        q[2 * i + 1] = (float)y[i];
    }
    // the box before the sort: the reference filters first, and sort_quadrilateral leaves zeros where it finds no diagonal
    // (collinear corners), which would widen the box of exactly the rows the filter is there to drop
    const float x1 = fminf(fminf(q[0], q[2]), fminf(q[4], q[6])), y1 = fminf(fminf(q[1], q[3]), fminf(q[5], q[7]));
    const float x2 = fmaxf(fmaxf(q[0], q[2]), fmaxf(q[4], q[6])), y2 = fmaxf(fmaxf(q[1], q[3]), fmaxf(q[5], q[7]));
    if (a.sort) dafne::sort_quad(q);
    float* r = a.recf + (size_t)g * kRecF;
    for (int i = 0; i < 8; i++) r[i] = q[i];
    r[8] = x1; r[9] = y1; r[10] = x2; r[11] = y2;
    r[12] = (float)(0.5 * fabs(s1 - s2));
    a.kept[g] = ((x2 - x1) > 1e-5f && (y2 - y1) > 1e-5f) ? 1 : 0;
}

__device__ inline int wave_sum(int v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// grid = n_views blocks of 64 threads (one wavefront)
__global__ void __launch_bounds__(64) count_kernel(const int32_t* kept, const int32_t* offsets_in, int G, int32_t* counts) {
    const int v = blockIdx.x, lane = threadIdx.x;
    const int p0 = offsets_in[v], n = min(offsets_in[v + 1], G) - p0;
    int c = 0;
    for (int j = lane; j < n; j += 64) c += kept[p0 + j];
    c = wave_sum(c);
    if (lane == 0) counts[v] = c;
}

// one block of 64 threads
__global__ void __launch_bounds__(64) scan_kernel(const int32_t* counts, int n_views, int32_t* offsets_out) {
    const int lane = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < n_views; base += 64) {
        const int t = base + lane;
        const bool ok = t < n_views;
        const int c = ok ? counts[t] : 0;
        int s = c;
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(s, d, 64);
            if (lane >= d) s += u;
        }
        if (ok) offsets_out[t] = carry + s - c;
        carry += __shfl(s, 63, 64);
    }
    if (lane == 0) offsets_out[n_views] = carry;
}

struct PackArgs {
    const float* recf;
    const int32_t* kept;
    const int32_t* offsets_in;
    const int32_t* classes_in;
    const int32_t* offsets_out;
    float *corners, *hbox, *area;
    int32_t *classes, *src;
    int G;
};

// grid = n_views blocks of 64 threads (one wavefront)
__global__ void __launch_bounds__(64) write_kernel(PackArgs a) {
    const int v = blockIdx.x, lane = threadIdx.x;
    const int p0 = a.offsets_in[v], n = min(a.offsets_in[v + 1], a.G) - p0;
    int base = a.offsets_out[v];
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int j0 = 0; j0 < n; j0 += 64) {      // n is the same in every lane: all of them reach the ballot
        const int j = j0 + lane;
        const int g = p0 + (j < n ? j : 0);
        const bool kept = j < n && a.kept[g] != 0;
        const unsigned long long mk = __ballot(kept);
        if (kept) {
            const size_t o = (size_t)base + __popcll(mk & below);
            const float* r = a.recf + (size_t)g * kRecF;
            for (int i = 0; i < 8; i++) a.corners[o * 8 + i] = r[i];
            for (int i = 0; i < 4; i++) a.hbox[o * 4 + i] = r[8 + i];
            a.area[o] = r[12];
            a.classes[o] = a.classes_in[g];
            a.src[o] = g;
        }
        base += __popcll(mk);
    }
}

size_t views_bytes(int n_views) { return dafne::align_up(sizeof(ViewGt) * (size_t)n_views, 256); }
size_t counts_bytes(int n_views) { return dafne::align_up(sizeof(int32_t) * (size_t)n_views, 256); }
size_t recf_bytes(int G) { return dafne::align_up(sizeof(float) * kRecF * (size_t)(G > 0 ? G : 1), 256); }
size_t kept_bytes(int G) { return dafne::align_up(sizeof(int32_t) * (size_t)(G > 0 ? G : 1), 256); }

}  // namespace train_views
}  // namespace

extern "C" {

size_t dafne_train_gt_workspace_bytes(int n_views, int G) {
    using namespace train_views;
    if (n_views < 1 || G < 0) return 0;
    return views_bytes(n_views) + counts_bytes(n_views) + recf_bytes(G) + kept_bytes(G);
}

int dafne_train_gt_hip(const dafne_train_view* views, int n_views, const float* d_corners_in, const int32_t* d_classes_in,
                       const int32_t* d_offsets_in, int G, int sort, float* d_corners, float* d_hbox, float* d_area,
                       int32_t* d_classes, int32_t* d_offsets_out, int32_t* d_src, void* d_ws, size_t ws_bytes, void* stream) {
    using namespace train_views;
    if (!views || n_views < 1 || G < 0) return dafne::fail(DAFNE_E_INVALID, "train_gt: bad args (n_views %d, G %d)", n_views, G);
    if (!d_offsets_in || !d_offsets_out || !d_ws || (G > 0 && (!d_corners_in || !d_classes_in || !d_corners || !d_hbox || !d_area ||
                                                               !d_classes || !d_src)))
        return dafne::fail(DAFNE_E_INVALID, "train_gt: null pointer");
    for (int v = 0; v < n_views; v++) {
        const dafne_train_view& s = views[v];
        if (s.win_h < 1 || s.win_w < 1 || (s.hflip != 0 && s.hflip != 1) || (s.vflip != 0 && s.vflip != 1) || s.new_h < 1 ||
            s.new_w < 1 || s.rot < 0 || s.rot > 3)
            return dafne::fail(DAFNE_E_INVALID, "train_gt: view %d: window %dx%d flips %d/%d -> %dx%d rot %d", v, s.win_h, s.win_w,
                               s.hflip, s.vflip, s.new_h, s.new_w, s.rot);
    }
    const size_t need = dafne_train_gt_workspace_bytes(n_views, G);
    if (ws_bytes < need) return dafne::fail(DAFNE_E_WORKSPACE, "train_gt: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    ViewGt* hv = new ViewGt[n_views];
    for (int v = 0; v < n_views; v++) {
        const dafne_train_view& s = views[v];
        hv[v].win_h = s.win_h; hv[v].win_w = s.win_w; hv[v].hflip = s.hflip; hv[v].vflip = s.vflip;
        hv[v].new_h = s.new_h; hv[v].new_w = s.new_w; hv[v].rot = s.rot; hv[v].reserved = 0;
    }
    const hipError_t ce = hipMemcpyAsync(d_ws, hv, sizeof(ViewGt) * (size_t)n_views, hipMemcpyHostToDevice, st);
    delete[] hv;
    if (ce != hipSuccess) return dafne::fail(DAFNE_E_HIP, "train_gt: hipMemcpyAsync: %s", hipGetErrorString(ce));
    uint8_t* p = static_cast<uint8_t*>(d_ws);
    const ViewGt* d_views = reinterpret_cast<const ViewGt*>(p);
    int32_t* counts = reinterpret_cast<int32_t*>(p + views_bytes(n_views));
    float* recf = reinterpret_cast<float*>(p + views_bytes(n_views) + counts_bytes(n_views));
    int32_t* kept = reinterpret_cast<int32_t*>(p + views_bytes(n_views) + counts_bytes(n_views) + recf_bytes(G));
    if (G > 0) {
        GtArgs a;
        a.views = d_views; a.corners_in = d_corners_in; a.offsets_in = d_offsets_in; a.recf = recf; a.kept = kept;
        a.n_views = n_views; a.G = G; a.sort = sort;
        hipLaunchKernelGGL(transform_kernel, dim3((unsigned)(((size_t)G + 255) / 256)), dim3(256), 0, st, a);
        if (int rc = dafne::check_launch("train_views::transform_kernel")) return rc;
    }
    hipLaunchKernelGGL(count_kernel, dim3(n_views), dim3(64), 0, st, kept, d_offsets_in, G, counts);
    if (int rc = dafne::check_launch("train_views::count_kernel")) return rc;
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(64), 0, st, counts, n_views, d_offsets_out);
    if (int rc = dafne::check_launch("train_views::scan_kernel")) return rc;
    PackArgs w;
    w.recf = recf; w.kept = kept; w.offsets_in = d_offsets_in; w.classes_in = d_classes_in; w.offsets_out = d_offsets_out;
    w.corners = d_corners; w.hbox = d_hbox; w.area = d_area; w.classes = d_classes; w.src = d_src; w.G = G;
    hipLaunchKernelGGL(write_kernel, dim3(n_views), dim3(64), 0, st, w);
    return dafne::check_launch("train_views::write_kernel");
}

}  // extern "C"
