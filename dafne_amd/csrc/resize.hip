// ResizeShortestEdge's pixel resampling on the GPU, bit-exact to Pillow's 8-bit bilinear resize.
//
// Reference path: DotaDatasetMapperTTA (dafne/modeling/tta.py:71-99) -> detectron2 ResizeShortestEdge ->
// ResizeTransform.apply_image, which for uint8 images is `PIL.Image.resize((w, h), BILINEAR)` [detectron2
// v0.5, recalled; Pillow is a third-party dependency, its published algorithm is restated here:
// libImaging/Resample.c -- precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal/Vertical_8bpc].
//   * separable, horizontal pass first into a uint8 intermediate, then the vertical pass;
//   * per output index: center = (i + 0.5) * scale, support = max(scale, 1), taps [int(center - support + .5),
//     int(center + support + .5)) clipped to the image, triangle weights normalised in double precision, then
//     fixed point: k = (int)(+-0.5 + w * 2^22); pixel = clip8((2^21 + sum pix * k) >> 22).
// The coefficients are recomputed per thread in fp64 (this file is built with -ffp-contract=off: same IEEE
// operations as the C code).  Horizontal / vertical flips of the TTA views are folded into the store index.
#include "common.h"

#include <string.h>

namespace {

constexpr int kPrec = 22;      // PRECISION_BITS = 32 - 8 - 2
constexpr int kMaxTaps = 64;   // downscale factors up to ~31x

struct Taps {
    int xmin, n;
    int k[kMaxTaps];
};

constexpr int kBilinear = 0, kBicubic = 1;      // dafne_scaled_tile.filter

// Pillow's filter functions (Resample.c bilinear_filter / bicubic_filter with a = -0.5), a >= 0
template <int F>
__device__ __forceinline__ double filter_weight(double a) {
    if (F == kBilinear) return a < 1.0 ? 1.0 - a : 0.0;
    if (a < 1.0) return ((-0.5 + 2.0) * a - (-0.5 + 3.0)) * a * a + 1;
    if (a < 2.0) return (((a - 5) * a + 8) * a - 4) * -0.5;
    return 0.0;
}

// coefficients of output index i for an axis of in_size -> out_size samples; F: the filter (support 1 / 2)
template <int F>
__device__ __forceinline__ void taps_for(int i, int in_size, int out_size, Taps& t) {
    const double scale = (double)(float)in_size / out_size;      // box = (0, in_size) as floats
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (F == kBilinear ? 1.0 : 2.0) * filterscale;
    const double center = 0.0 + (i + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > kMaxTaps) xmax = kMaxTaps;       // excluded on the host
    double w[kMaxTaps];
    double ww = 0.0;
    for (int x = 0; x < xmax; x++) {
        double a = (x + xmin - center + 0.5) * ss;
        if (a < 0.0) a = -a;
        const double v = filter_weight<F>(a);
        w[x] = v;
        ww += v;
    }
    for (int x = 0; x < xmax; x++) {
        double v = w[x];
        if (ww != 0.0) v /= ww;
        t.k[x] = v < 0 ? (int)(-0.5 + v * (double)(1 << kPrec)) : (int)(0.5 + v * (double)(1 << kPrec));
    }
    t.xmin = xmin;
    t.n = xmax;
}

__device__ __forceinline__ void taps_for(int i, int in_size, int out_size, Taps& t) { taps_for<kBilinear>(i, in_size, out_size, t); }

__device__ __forceinline__ unsigned char clip8(int v) {
    v >>= kPrec;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// horizontal pass: in [C,H,W] (or [H,W,C]) -> tmp [C,H,new_w]
__global__ void __launch_bounds__(256) resize_h_kernel(const unsigned char* __restrict__ in, int hwc, int C, int H, int W,
                                                       int new_w, unsigned char* __restrict__ tmp) {
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    if (xx >= new_w) return;
    Taps t;
    taps_for(xx, W, new_w, t);
    for (int y = blockIdx.y; y < H; y += gridDim.y)
        for (int c = 0; c < C; c++) {
            int acc = 1 << (kPrec - 1);
            for (int x = 0; x < t.n; x++) {
                const int px = hwc ? in[((size_t)y * W + x + t.xmin) * C + c] : in[((size_t)c * H + y) * W + x + t.xmin];
                acc += px * t.k[x];
            }
            tmp[((size_t)c * H + y) * new_w + xx] = clip8(acc);
        }
}

// vertical pass + flips: tmp [C,H,new_w] -> out [C,new_h,new_w]
__global__ void __launch_bounds__(256) resize_v_kernel(const unsigned char* __restrict__ tmp, int C, int H, int new_h, int new_w,
                                                       int hflip, int vflip, unsigned char* __restrict__ out) {
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    const int yy = blockIdx.y;
    if (xx >= new_w || yy >= new_h) return;
    Taps t;
    taps_for(yy, H, new_h, t);
    const int oy = vflip ? new_h - 1 - yy : yy, ox = hflip ? new_w - 1 - xx : xx;
    for (int c = 0; c < C; c++) {
        int acc = 1 << (kPrec - 1);
        for (int y = 0; y < t.n; y++) acc += (int)tmp[((size_t)c * H + y + t.xmin) * new_w + xx] * t.k[y];
        out[((size_t)c * new_h + oy) * new_w + ox] = clip8(acc);
    }
}

}  // namespace

extern "C" {

size_t dafne_resize_workspace_bytes(int C, int H, int new_w) {
    if (C < 1 || H < 1 || new_w < 1) return 0;
    return dafne::align_up((size_t)C * H * new_w, 256);
}

int dafne_resize_bilinear_u8_hip(const uint8_t* d_in, int layout_hwc, int C, int H, int W, int new_h, int new_w,
                                 int hflip, int vflip, uint8_t* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    if (!d_in || !d_out || !d_ws || C < 1 || H < 1 || W < 1 || new_h < 1 || new_w < 1)
        return dafne::fail(DAFNE_E_INVALID, "resize: bad args");
    if (ws_bytes < dafne_resize_workspace_bytes(C, H, new_w))
        return dafne::fail(DAFNE_E_WORKSPACE, "resize: workspace %zu < %zu", ws_bytes, dafne_resize_workspace_bytes(C, H, new_w));
    // tap count of the widest filter: 2 * ceil(support) + 1
    const double sx = (double)W / new_w, sy = (double)H / new_h;
    if ((sx > 1 ? sx : 1) * 2 + 2 > kMaxTaps || (sy > 1 ? sy : 1) * 2 + 2 > kMaxTaps)
        return dafne::fail(DAFNE_E_UNSUPPORTED, "resize: downscale factor above %d", kMaxTaps / 2 - 1);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* tmp = (unsigned char*)d_ws;
    const int gy = H < 1024 ? H : 1024;
    hipLaunchKernelGGL(resize_h_kernel, dim3((new_w + 255) / 256, gy), dim3(256), 0, st, d_in, layout_hwc, C, H, W, new_w, tmp);
    int rc = dafne::check_launch("resize_h");
    if (rc) return rc;
    hipLaunchKernelGGL(resize_v_kernel, dim3((new_w + 255) / 256, new_h), dim3(256), 0, st, tmp, C, H, new_h, new_w, hflip, vflip,
                       d_out);
    return dafne::check_launch("resize_v");
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- whole-scene tile gather
// The DOTA split (tools/prepare_dota SplitOnlyImage_multi_process.SplitSingle, saveimagepatches(padding=True)) as one launch
// over every tile of every scene of a call: tile t is the patch x patch crop of its scene at (left, up), zero past the edge.
namespace {

constexpr int kPix = 8;        // pixels per thread of the tile gather: 24 output bytes, three 8-byte stores

// 4-byte-aligned word that holds byte p; every word read holds at least one byte of the source row, so no read leaves
// the allocation's last word
__device__ __forceinline__ uint32_t word_at(const uint8_t* base, size_t p) {
    return *reinterpret_cast<const uint32_t*>(base + (p & ~(size_t)3));
}

// n bytes (n % 4 == 0, n <= 24) starting at the unaligned byte offset p, as n / 4 little-endian words
template <int N>
__device__ __forceinline__ void load_unaligned(const uint8_t* base, size_t p, uint32_t (&out)[N]) {
    const int sh = (int)(p & 3) * 8;
    uint32_t w[N + 1];
#pragma unroll
    for (int k = 0; k < N; k++) w[k] = word_at(base, p + 4 * k);
    w[N] = sh ? word_at(base, p + 4 * N) : 0u;       // only when the span crosses one more word
#pragma unroll
    for (int k = 0; k < N; k++) out[k] = sh ? (uint32_t)((((uint64_t)w[k + 1]) << 32 | w[k]) >> sh) : w[k];
}

// One thread = 8 consecutive output pixels of one tile row.  Interior: aligned word loads + shifts, three 8-byte
// stores.  Edge (any of the 8 pixels past the scene): byte loads under a mask, zeros outside.
__global__ void __launch_bounds__(256) scene_tiles_kernel(const dafne_scene_tile* __restrict__ tiles, int n_tiles, int patch,
                                                          uint8_t* __restrict__ out) {
    const int per_row = patch / kPix;
    const size_t per_tile = (size_t)patch * per_row;
    const size_t total = per_tile * n_tiles;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i / per_tile);
        const size_t r = i - (size_t)t * per_tile;
        const int y = (int)(r / per_row);
        const int x0 = (int)(r - (size_t)y * per_row) * kPix;
        const dafne_scene_tile d = tiles[t];
        const int sy = d.up + y, sx = d.left + x0;
        uint32_t o[6];
        if (sy < d.h && sx + kPix <= d.w) {
            if (d.layout_hwc) {
                load_unaligned<6>(d.d_scene, ((size_t)sy * d.w + sx) * 3, o);
            } else {
                const size_t plane = (size_t)d.h * d.w;
                const size_t p = (size_t)sy * d.w + sx;
                uint32_t c[3][2];
                load_unaligned<2>(d.d_scene, p, c[0]);
                load_unaligned<2>(d.d_scene + plane, p, c[1]);
                load_unaligned<2>(d.d_scene + 2 * plane, p, c[2]);
                uint8_t b[24];
#pragma unroll
                for (int k = 0; k < kPix; k++)
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) b[3 * k + ch] = (uint8_t)(c[ch][k >> 2] >> (8 * (k & 3)));
#pragma unroll
                for (int k = 0; k < 6; k++)
                    o[k] = (uint32_t)b[4 * k] | (uint32_t)b[4 * k + 1] << 8 | (uint32_t)b[4 * k + 2] << 16 |
                           (uint32_t)b[4 * k + 3] << 24;
            }
        } else {
            uint8_t b[24];
            const size_t plane = (size_t)d.h * d.w;
#pragma unroll
            for (int k = 0; k < kPix; k++) {
                const bool in = sy < d.h && sx + k < d.w;
                const size_t p = in ? (size_t)sy * d.w + sx + k : 0;
#pragma unroll
                for (int ch = 0; ch < 3; ch++)
                    b[3 * k + ch] = in ? (d.layout_hwc ? d.d_scene[p * 3 + ch] : d.d_scene[ch * plane + p]) : (uint8_t)0;
            }
#pragma unroll
            for (int k = 0; k < 6; k++)
                o[k] = (uint32_t)b[4 * k] | (uint32_t)b[4 * k + 1] << 8 | (uint32_t)b[4 * k + 2] << 16 | (uint32_t)b[4 * k + 3] << 24;
        }
        // byte offset ((t * patch + y) * patch + x0) * 3 is a multiple of 24: 8-byte aligned
        uint2* dst = reinterpret_cast<uint2*>(out + (((size_t)t * patch + y) * patch + x0) * 3);
        dst[0] = make_uint2(o[0], o[1]);
        dst[1] = make_uint2(o[2], o[3]);
        dst[2] = make_uint2(o[4], o[5]);
    }
}

}  // namespace

extern "C" {

size_t dafne_scene_tiles_workspace_bytes(int n_tiles) {
    if (n_tiles < 1) return 0;
    return dafne::align_up(sizeof(dafne_scene_tile) * (size_t)n_tiles, 256);
}

int dafne_scene_tiles_u8_hip(const dafne_scene_tile* tiles, int n_tiles, int patch, uint8_t* d_out_hwc, void* d_ws,
                             size_t ws_bytes, void* stream) {
    if (!tiles || !d_out_hwc || !d_ws || n_tiles < 1 || patch < kPix)
        return dafne::fail(DAFNE_E_INVALID, "scene_tiles: bad args (n_tiles %d, patch %d)", n_tiles, patch);
    if (patch % kPix) return dafne::fail(DAFNE_E_UNSUPPORTED, "scene_tiles: patch %d is not a multiple of %d", patch, kPix);
    if (ws_bytes < dafne_scene_tiles_workspace_bytes(n_tiles))
        return dafne::fail(DAFNE_E_WORKSPACE, "scene_tiles: workspace %zu < %zu", ws_bytes, dafne_scene_tiles_workspace_bytes(n_tiles));
    for (int t = 0; t < n_tiles; t++) {
        const dafne_scene_tile& d = tiles[t];
        if (!d.d_scene || d.h < 1 || d.w < 1 || (d.layout_hwc != 0 && d.layout_hwc != 1) || d.left < 0 || d.up < 0 ||
            d.left >= d.w || d.up >= d.h)
            return dafne::fail(DAFNE_E_INVALID, "scene_tiles: tile %d: scene %dx%d layout %d origin (%d, %d)", t, d.h, d.w,
                               d.layout_hwc, d.left, d.up);
    }
    hipStream_t st = (hipStream_t)stream;
    DAFNE_HIP_TRY(hipMemcpyAsync(d_ws, tiles, sizeof(dafne_scene_tile) * (size_t)n_tiles, hipMemcpyHostToDevice, st));
    const size_t total = (size_t)n_tiles * patch * (patch / kPix);
    const size_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(scene_tiles_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st,
                       (const dafne_scene_tile*)d_ws, n_tiles, patch, d_out_hwc);
    return dafne::check_launch("scene_tiles");
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------- scene TTA views
// DotaDatasetMapperTTA's views (dafne/modeling/tta.py:71-99: per TEST.AUG size, plain / hflip / vflip) cut straight out of
// the scenes: view v is the Pillow-exact bilinear resize of a zero-padded window of its source, then the flips, i.e. bit for
// bit resize_u8(gather_tiles(...)[v] as CHW, out_h, out_w, hflip, vflip) (taps_for and clip8 above, the same integer sums).
// The coefficients are computed once per launch and axis (views_taps_kernel, taps_for's fp64 operations) into the
// workspace.  views_kernel: a workgroup owns kViewBX resampled columns x `by` resampled rows of one view; it runs the
// horizontal pass into LDS for the source rows those rows' vertical taps touch, and then the vertical pass from LDS, so the
// uint8 intermediate never leaves the chip.  The host picks `by` so that the LDS rows fit kViewLdsBudget.
namespace {

constexpr int kViewBX = 64;                 // resampled columns per workgroup
constexpr int kViewLdsBudget = 48 * 1024;   // LDS per workgroup: three workgroups per CU (160 KiB)
constexpr int kViewMaxAxes = 8;             // distinct window widths (and heights) per launch
constexpr int kTapStride = 2 + kMaxTaps;    // per output index: xmin, n, k[kMaxTaps]

struct ViewDev {
    dafne_view_src s;
    int tx, ty;                             // coefficient table of the x / y axis
};

struct AxisDev {
    int in_size, out_size;
    int filter, reserved;                   // kBilinear / kBicubic
    size_t off;                             // int offset of the table in the coefficient area
};

__global__ void __launch_bounds__(256) views_taps_kernel(const AxisDev* __restrict__ axes, int n_axes,
                                                         int* __restrict__ coef) {
    const int a = blockIdx.y;
    if (a >= n_axes) return;
    const AxisDev ax = axes[a];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ax.out_size) return;
    Taps t;
    if (ax.filter == kBicubic)
        taps_for<kBicubic>(i, ax.in_size, ax.out_size, t);
    else
        taps_for<kBilinear>(i, ax.in_size, ax.out_size, t);
    int* c = coef + ax.off + (size_t)i * kTapStride;
    c[0] = t.xmin;
    c[1] = t.n;
    for (int x = 0; x < t.n; x++) c[2 + x] = t.k[x];
}

// window pixel (r, x), channel ch of the view's source; 0 outside the source (the split's zero padding)
__device__ __forceinline__ int window_px(const dafne_view_src& s, int r, int x, int ch) {
    const long long sy = (long long)s.up + r, sx = (long long)s.left + x;
    if (sy >= s.h || sx >= s.w) return 0;
    return s.layout_hwc ? s.d_src[((size_t)sy * s.w + sx) * 3 + ch] : s.d_src[((size_t)ch * s.h + sy) * s.w + sx];
}

__global__ void __launch_bounds__(256) views_kernel(const ViewDev* __restrict__ views, int n_views, const AxisDev* __restrict__ axes,
                                                    const int* __restrict__ coef, int out_h, int out_w, int by, int rows_cap,
                                                    uint8_t* __restrict__ out) {
    extern __shared__ uint8_t tmp[];         // [3][rows_cap][kViewBX]
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kViewBX, y0 = blockIdx.y * by;
    const int nx = min(kViewBX, out_w - x0), ny = min(by, out_h - y0);
    for (int v = blockIdx.z; v < n_views; v += gridDim.z) {
        const ViewDev vd = views[v];
        const dafne_view_src& s = vd.s;
        const int* cx = coef + axes[vd.tx].off;
        const int* cy = coef + axes[vd.ty].off;
        // source rows of the block's vertical taps: xmin is non-decreasing in the output index, and so is xmin + n
        const int ylo = cy[(size_t)y0 * kTapStride];
        const int* clast = cy + (size_t)(y0 + ny - 1) * kTapStride;
        const int nrows = min(clast[0] + clast[1] - ylo, rows_cap);
        // horizontal pass: rows [ylo, ylo + nrows) x the block's columns -> LDS
        for (int e = tid; e < nrows * kViewBX; e += blockDim.x) {
            const int r = e / kViewBX, c = e - r * kViewBX;
            if (c >= nx) continue;
            const int* t = cx + (size_t)(x0 + c) * kTapStride;
            const int xmin = t[0], n = t[1];
            int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
            for (int x = 0; x < n; x++) {
                const int k = t[2 + x];
                a0 += window_px(s, ylo + r, xmin + x, 0) * k;
                a1 += window_px(s, ylo + r, xmin + x, 1) * k;
                a2 += window_px(s, ylo + r, xmin + x, 2) * k;
            }
            tmp[(0 * rows_cap + r) * kViewBX + c] = clip8(a0);
            tmp[(1 * rows_cap + r) * kViewBX + c] = clip8(a1);
            tmp[(2 * rows_cap + r) * kViewBX + c] = clip8(a2);
        }
        __syncthreads();
        // vertical pass + flips folded into the store index
        for (int e = tid; e < ny * kViewBX; e += blockDim.x) {
            const int yl = e / kViewBX, c = e - yl * kViewBX;
            if (c >= nx) continue;
            const int yy = y0 + yl, xx = x0 + c;
            const int* t = cy + (size_t)yy * kTapStride;
            const int r0 = t[0] - ylo, n = t[1];
            int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
            for (int y = 0; y < n; y++) {
                const int k = t[2 + y];
                const int r = r0 + y < rows_cap ? r0 + y : rows_cap - 1;     // (never clamps: rows_cap bounds the span)
                a0 += (int)tmp[(0 * rows_cap + r) * kViewBX + c] * k;
                a1 += (int)tmp[(1 * rows_cap + r) * kViewBX + c] * k;
                a2 += (int)tmp[(2 * rows_cap + r) * kViewBX + c] * k;
            }
            const int oy = s.vflip ? out_h - 1 - yy : yy, ox = s.hflip ? out_w - 1 - xx : xx;
            const size_t plane = (size_t)out_h * out_w;
            uint8_t* o = out + (size_t)v * 3 * plane + (size_t)oy * out_w + ox;
            o[0] = clip8(a0);
            o[plane] = clip8(a1);
            o[2 * plane] = clip8(a2);
        }
        __syncthreads();
    }
}

// the distinct window widths / heights of a launch -> axis tables; false when there are more than kViewMaxAxes of either
bool view_axes(const dafne_view_src* views, int n_views, int out_h, int out_w, AxisDev* axes, int* n_axes, int* tx, int* ty) {
    int na = 0;
    for (int pass = 0; pass < 2; pass++) {
        const int first = na;
        for (int v = 0; v < n_views; v++) {
            const int in = pass ? views[v].win_h : views[v].win_w;
            int a = first;
            while (a < na && axes[a].in_size != in) a++;
            if (a == na) {
                if (na - first >= kViewMaxAxes) return false;
                axes[na].in_size = in;
                axes[na].out_size = pass ? out_h : out_w;
                axes[na].filter = kBilinear;
                na++;
            }
            (pass ? ty : tx)[v] = a;
        }
    }
    size_t off = 0;
    for (int a = 0; a < na; a++) {
        axes[a].off = off;
        off += (size_t)axes[a].out_size * kTapStride;
    }
    *n_axes = na;
    return true;
}

// rows of the LDS intermediate a workgroup of `by` resampled rows needs, for the largest vertical scale of the launch:
// the span ylo .. xmin + n of rows y0 .. y0 + by - 1 is at most (by - 1) * scale + 2 * support + 1 (taps_for's rounding)
int view_rows_cap(double scale, int by, int in_max, double filter_support = 1.0) {
    const double support = filter_support * (scale < 1.0 ? 1.0 : scale);
    int r = (int)((by - 1) * scale + 2.0 * support + 1.0) + 2;
    return r < in_max ? r : in_max;
}

size_t views_header_bytes(int n_views) {
    return dafne::align_up(sizeof(ViewDev) * (size_t)n_views, 256) + dafne::align_up(sizeof(AxisDev) * 2 * kViewMaxAxes, 256);
}

}  // namespace

extern "C" {

size_t dafne_scene_views_workspace_bytes(const dafne_view_src* views, int n_views, int out_h, int out_w) {
    if (!views || n_views < 1 || out_h < 1 || out_w < 1) return 0;
    AxisDev axes[2 * kViewMaxAxes];
    int na = 0;
    int* tx = new int[n_views];
    int* ty = new int[n_views];
    const bool ok = view_axes(views, n_views, out_h, out_w, axes, &na, tx, ty);
    delete[] tx;
    delete[] ty;
    if (!ok) return 0;
    size_t coef = 0;
    for (int a = 0; a < na; a++) coef += (size_t)axes[a].out_size * kTapStride;
    return views_header_bytes(n_views) + dafne::align_up(coef * sizeof(int), 256);
}

int dafne_scene_views_u8_hip(const dafne_view_src* views, int n_views, int out_h, int out_w, uint8_t* d_out, void* d_ws,
                             size_t ws_bytes, void* stream) {
    if (!views || !d_out || !d_ws || n_views < 1 || out_h < 1 || out_w < 1)
        return dafne::fail(DAFNE_E_INVALID, "scene_views: bad args (n_views %d, out %dx%d)", n_views, out_h, out_w);
    double sy_max = 0.0;
    int in_h_max = 1;
    for (int v = 0; v < n_views; v++) {
        const dafne_view_src& s = views[v];
        if (!s.d_src || s.h < 1 || s.w < 1 || (s.layout_hwc != 0 && s.layout_hwc != 1) || s.left < 0 || s.up < 0 ||
            s.win_h < 1 || s.win_w < 1 || (s.hflip != 0 && s.hflip != 1) || (s.vflip != 0 && s.vflip != 1))
            return dafne::fail(DAFNE_E_INVALID, "scene_views: view %d: source %dx%d layout %d window (%d, %d) %dx%d flips %d/%d", v,
                               s.h, s.w, s.layout_hwc, s.left, s.up, s.win_h, s.win_w, s.hflip, s.vflip);
        // the limit of dafne_resize_bilinear_u8_hip: tap count of the widest filter, 2 * ceil(support) + 1
        const double sx = (double)s.win_w / out_w, sy = (double)s.win_h / out_h;
        if ((sx > 1 ? sx : 1) * 2 + 2 > kMaxTaps || (sy > 1 ? sy : 1) * 2 + 2 > kMaxTaps)
            return dafne::fail(DAFNE_E_UNSUPPORTED, "scene_views: view %d: downscale factor above %d", v, kMaxTaps / 2 - 1);
        if (sy > sy_max) sy_max = sy;
        if (s.win_h > in_h_max) in_h_max = s.win_h;
    }
    const size_t need = dafne_scene_views_workspace_bytes(views, n_views, out_h, out_w);
    if (need == 0) return dafne::fail(DAFNE_E_UNSUPPORTED, "scene_views: more than %d window widths or heights in one launch", kViewMaxAxes);
    if (ws_bytes < need) return dafne::fail(DAFNE_E_WORKSPACE, "scene_views: workspace %zu < %zu", ws_bytes, need);
    // header: views + axis tables, one copy
    const size_t hdr = views_header_bytes(n_views);
    const size_t vbytes = dafne::align_up(sizeof(ViewDev) * (size_t)n_views, 256);
    uint8_t* blob = new uint8_t[hdr]();
    ViewDev* vd = reinterpret_cast<ViewDev*>(blob);
    AxisDev* axes = reinterpret_cast<AxisDev*>(blob + vbytes);
    int na = 0;
    int* tx = new int[n_views];
    int* ty = new int[n_views];
    view_axes(views, n_views, out_h, out_w, axes, &na, tx, ty);
    for (int v = 0; v < n_views; v++) {
        vd[v].s = views[v];
        vd[v].tx = tx[v];
        vd[v].ty = ty[v];
    }
    delete[] tx;
    delete[] ty;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t ce = hipMemcpyAsync(d_ws, blob, hdr, hipMemcpyHostToDevice, st);
    delete[] blob;
    if (ce != hipSuccess) return dafne::fail(DAFNE_E_HIP, "scene_views: hipMemcpyAsync: %s", hipGetErrorString(ce));
    const ViewDev* d_views = (const ViewDev*)d_ws;
    const AxisDev* d_axes = (const AxisDev*)((uint8_t*)d_ws + vbytes);
    int* d_coef = (int*)((uint8_t*)d_ws + hdr);
    const int omax = out_h > out_w ? out_h : out_w;
    hipLaunchKernelGGL(views_taps_kernel, dim3((omax + 255) / 256, na), dim3(256), 0, st, d_axes, na, d_coef);
    int rc = dafne::check_launch("scene_views_taps");
    if (rc) return rc;
    // rows per workgroup: the most that keep the LDS intermediate within the budget
    int by = 32, rows_cap = view_rows_cap(sy_max, by, in_h_max);
    while (by > 1 && 3 * kViewBX * rows_cap > kViewLdsBudget) {
        by /= 2;
        rows_cap = view_rows_cap(sy_max, by, in_h_max);
    }
    const unsigned gz = (unsigned)(n_views < 65535 ? n_views : 65535);
    hipLaunchKernelGGL(views_kernel, dim3((out_w + kViewBX - 1) / kViewBX, (out_h + by - 1) / by, gz), dim3(256),
                       (size_t)3 * kViewBX * rows_cap, st, d_views, n_views, d_axes, d_coef, out_h, out_w, by, rows_cap, d_out);
    return dafne::check_launch("scene_views");
}

}  // extern "C"

// ------------------------------------------------------------------------------------- tiles of a resampled scene
// The split of a scene resampled to new_h x new_w (multi-scale whole-scene inference): tile t is the patch x patch crop at
// (left, up) of Pillow's resize of the WHOLE scene with its filter (the taps clip at the scene's border, not at the tile's),
// zero past new_h / new_w -- cut straight from the original scene.  views_kernel's structure: one coefficient table per distinct
// (in size, out size, filter) axis of the call (views_taps_kernel), a workgroup owns kViewBX columns x `by` rows of one tile,
// runs the horizontal pass into LDS for the source rows its vertical taps touch (clip8 after it, as Pillow's uint8 intermediate:
// bicubic coefficients are negative), then the vertical pass from LDS into an LDS copy of its output rows, which leaves as
// 4-byte words.  The resampled scene itself never exists in memory.
namespace {

constexpr int kTileStore = 4;               // bytes per store: patch * 3 and kViewBX * 3 are multiples of it

struct ScaledDev {
    dafne_scaled_tile s;
    int tx, ty;                             // coefficient table of the x / y axis
};

__global__ void __launch_bounds__(256) scaled_tiles_kernel(const ScaledDev* __restrict__ tiles, int n_tiles,
                                                           const AxisDev* __restrict__ axes, const int* __restrict__ coef, int patch,
                                                           int by, int rows_cap, uint8_t* __restrict__ out) {
    extern __shared__ uint8_t tmp[];         // [3][rows_cap][kViewBX], then the output rows [by][kViewBX * 3]
    uint8_t* obuf = tmp + (size_t)3 * rows_cap * kViewBX;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kViewBX, y0 = blockIdx.y * by;
    const int bw = min(kViewBX, patch - x0), bh = min(by, patch - y0);       // the block's share of the tile
    for (int v = blockIdx.z; v < n_tiles; v += gridDim.z) {
        const ScaledDev td = tiles[v];
        const dafne_scaled_tile& s = td.s;
        const int X0 = s.left + x0, Y0 = s.up + y0;                          // resampled coordinates of the block
        const int nx = max(0, min(bw, s.new_w - X0)), ny = max(0, min(bh, s.new_h - Y0));
        const bool any = nx > 0 && ny > 0;                                   // (block-uniform)
        const int* cx = coef + axes[td.tx].off;
        const int* cy = coef + axes[td.ty].off;
        int ylo = 0;
        if (any) {
            // source rows of the block's vertical taps: xmin is non-decreasing in the output index, and so is xmin + n
            ylo = cy[(size_t)Y0 * kTapStride];
            const int* clast = cy + (size_t)(Y0 + ny - 1) * kTapStride;
            const int nrows = min(clast[0] + clast[1] - ylo, rows_cap);
            const size_t plane = (size_t)s.h * s.w;
            for (int e = tid; e < nrows * kViewBX; e += blockDim.x) {
                const int r = e / kViewBX, c = e - r * kViewBX;
                if (c >= nx) continue;
                const int* t = cx + (size_t)(X0 + c) * kTapStride;
                const int xmin = t[0], n = t[1];
                const size_t p = (size_t)(ylo + r) * s.w + xmin;             // taps stay inside the scene: no bounds test
                int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
                if (s.layout_hwc) {
                    const uint8_t* src = s.d_scene + p * 3;
                    for (int x = 0; x < n; x++) {
                        const int k = t[2 + x];
                        a0 += (int)src[3 * x] * k;
                        a1 += (int)src[3 * x + 1] * k;
                        a2 += (int)src[3 * x + 2] * k;
                    }
                } else {
                    const uint8_t* src = s.d_scene + p;
                    for (int x = 0; x < n; x++) {
                        const int k = t[2 + x];
                        a0 += (int)src[x] * k;
                        a1 += (int)src[plane + x] * k;
                        a2 += (int)src[2 * plane + x] * k;
                    }
                }
                tmp[(0 * rows_cap + r) * kViewBX + c] = clip8(a0);
                tmp[(1 * rows_cap + r) * kViewBX + c] = clip8(a1);
                tmp[(2 * rows_cap + r) * kViewBX + c] = clip8(a2);
            }
        }
        __syncthreads();
        // vertical pass into the output rows; zero past the resampled scene
        for (int e = tid; e < bh * kViewBX; e += blockDim.x) {
            const int yl = e / kViewBX, c = e - yl * kViewBX;
            if (c >= bw) continue;
            uint8_t b0 = 0, b1 = 0, b2 = 0;
            if (c < nx && yl < ny) {
                const int* t = cy + (size_t)(Y0 + yl) * kTapStride;
                const int r0 = t[0] - ylo, n = t[1];
                int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
                for (int y = 0; y < n; y++) {
                    const int k = t[2 + y];
                    const int r = r0 + y < rows_cap ? r0 + y : rows_cap - 1;     // (never clamps: rows_cap bounds the span)
                    a0 += (int)tmp[(0 * rows_cap + r) * kViewBX + c] * k;
                    a1 += (int)tmp[(1 * rows_cap + r) * kViewBX + c] * k;
                    a2 += (int)tmp[(2 * rows_cap + r) * kViewBX + c] * k;
                }
                b0 = clip8(a0);
                b1 = clip8(a1);
                b2 = clip8(a2);
            }
            uint8_t* o = obuf + (yl * kViewBX + c) * 3;
            o[0] = b0;
            o[1] = b1;
            o[2] = b2;
        }
        __syncthreads();
        // the block's bw * 3 bytes of every row: byte offset ((v * patch + y) * patch + x0) * 3 is a multiple of 4
        const int wpr = bw * 3 / kTileStore;
        for (int e = tid; e < bh * wpr; e += blockDim.x) {
            const int yl = e / wpr, q = e - yl * wpr;
            uint32_t* dst = reinterpret_cast<uint32_t*>(out + (((size_t)v * patch + y0 + yl) * patch + x0) * 3);
            dst[q] = reinterpret_cast<const uint32_t*>(obuf + yl * kViewBX * 3)[q];
        }
        __syncthreads();
    }
}

struct ScaledPlan {
    AxisDev* axes;          // 2 * n_tiles at most
    int* tx;
    int* ty;
    int n_axes;
    size_t coef_ints;
};

// the distinct (in size, out size, filter) axes of a call; tx / ty: per tile its tables.  The caller owns the arrays.
void scaled_axes(const dafne_scaled_tile* tiles, int n_tiles, ScaledPlan& p) {
    int na = 0;
    for (int v = 0; v < n_tiles; v++)
        for (int pass = 0; pass < 2; pass++) {
            const int in = pass ? tiles[v].h : tiles[v].w, o = pass ? tiles[v].new_h : tiles[v].new_w, f = tiles[v].filter;
            int a = 0;
            // consecutive tiles share their scene and scale: look at the latest tables first
            for (a = na - 1; a >= 0; a--)
                if (p.axes[a].in_size == in && p.axes[a].out_size == o && p.axes[a].filter == f) break;
            if (a < 0) {
                a = na++;
                p.axes[a].in_size = in;
                p.axes[a].out_size = o;
                p.axes[a].filter = f;
                p.axes[a].reserved = 0;
            }
            (pass ? p.ty : p.tx)[v] = a;
        }
    size_t off = 0;
    for (int a = 0; a < na; a++) {
        p.axes[a].off = off;
        off += (size_t)p.axes[a].out_size * kTapStride;
    }
    p.n_axes = na;
    p.coef_ints = off;
}

bool scaled_tile_ok(const dafne_scaled_tile& d) {
    return d.d_scene && d.h >= 1 && d.w >= 1 && (d.layout_hwc == 0 || d.layout_hwc == 1) && d.new_h >= 1 && d.new_w >= 1 &&
           d.left >= 0 && d.up >= 0 && d.left < d.new_w && d.up < d.new_h && (d.filter == kBilinear || d.filter == kBicubic);
}

size_t scaled_tiles_bytes(int n_tiles) { return dafne::align_up(sizeof(ScaledDev) * (size_t)n_tiles, 256); }
size_t scaled_axes_bytes(int n_axes) { return dafne::align_up(sizeof(AxisDev) * (size_t)n_axes, 256); }

}  // namespace

extern "C" {

size_t dafne_scene_scaled_tiles_workspace_bytes(const dafne_scaled_tile* tiles, int n_tiles) {
    if (!tiles || n_tiles < 1) return 0;
    for (int v = 0; v < n_tiles; v++)
        if (!scaled_tile_ok(tiles[v])) return 0;
    ScaledPlan p;
    p.axes = new AxisDev[2 * (size_t)n_tiles];
    p.tx = new int[n_tiles];
    p.ty = new int[n_tiles];
    scaled_axes(tiles, n_tiles, p);
    delete[] p.axes;
    delete[] p.tx;
    delete[] p.ty;
    return scaled_tiles_bytes(n_tiles) + scaled_axes_bytes(p.n_axes) + dafne::align_up(p.coef_ints * sizeof(int), 256);
}

int dafne_scene_scaled_tiles_u8_hip(const dafne_scaled_tile* tiles, int n_tiles, int patch, uint8_t* d_out_hwc, void* d_ws,
                                    size_t ws_bytes, void* stream) {
    if (!tiles || !d_out_hwc || !d_ws || n_tiles < 1 || patch < kTileStore)
        return dafne::fail(DAFNE_E_INVALID, "scene_scaled_tiles: bad args (n_tiles %d, patch %d)", n_tiles, patch);
    if (patch % kTileStore)
        return dafne::fail(DAFNE_E_UNSUPPORTED, "scene_scaled_tiles: patch %d is not a multiple of %d", patch, kTileStore);
    int omax = 1;
    for (int v = 0; v < n_tiles; v++) {
        const dafne_scaled_tile& d = tiles[v];
        if (!scaled_tile_ok(d))
            return dafne::fail(DAFNE_E_INVALID, "scene_scaled_tiles: tile %d: scene %dx%d layout %d -> %dx%d origin (%d, %d) filter %d", v,
                               d.h, d.w, d.layout_hwc, d.new_h, d.new_w, d.left, d.up, d.filter);
        // tap count of the widest filter: 2 * ceil(support) + 1, support = (1 | 2) * max(scale, 1)
        const double fs = d.filter == kBicubic ? 2.0 : 1.0;
        const double sx = (double)d.w / d.new_w, sy = (double)d.h / d.new_h;
        if (fs * (sx > 1 ? sx : 1) * 2 + 2 > kMaxTaps || fs * (sy > 1 ? sy : 1) * 2 + 2 > kMaxTaps)
            return dafne::fail(DAFNE_E_UNSUPPORTED, "scene_scaled_tiles: tile %d: %s downscale factor above %d", v,
                               d.filter == kBicubic ? "bicubic" : "bilinear", (int)((kMaxTaps / 2 - 1) / fs));
        if (d.new_h > omax) omax = d.new_h;
        if (d.new_w > omax) omax = d.new_w;
    }
    const size_t need = dafne_scene_scaled_tiles_workspace_bytes(tiles, n_tiles);
    if (ws_bytes < need) return dafne::fail(DAFNE_E_WORKSPACE, "scene_scaled_tiles: workspace %zu < %zu", ws_bytes, need);
    ScaledPlan p;
    p.axes = new AxisDev[2 * (size_t)n_tiles];
    p.tx = new int[n_tiles];
    p.ty = new int[n_tiles];
    scaled_axes(tiles, n_tiles, p);
    // header: tiles + axis tables, one copy
    const size_t tbytes = scaled_tiles_bytes(n_tiles), hdr = tbytes + scaled_axes_bytes(p.n_axes);
    uint8_t* blob = new uint8_t[hdr]();
    ScaledDev* td = reinterpret_cast<ScaledDev*>(blob);
    for (int v = 0; v < n_tiles; v++) {
        td[v].s = tiles[v];
        td[v].tx = p.tx[v];
        td[v].ty = p.ty[v];
    }
    memcpy(blob + tbytes, p.axes, sizeof(AxisDev) * (size_t)p.n_axes);
    const int na = p.n_axes;
    delete[] p.axes;
    delete[] p.tx;
    delete[] p.ty;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t ce = hipMemcpyAsync(d_ws, blob, hdr, hipMemcpyHostToDevice, st);
    delete[] blob;
    if (ce != hipSuccess) return dafne::fail(DAFNE_E_HIP, "scene_scaled_tiles: hipMemcpyAsync: %s", hipGetErrorString(ce));
    const ScaledDev* d_tiles = (const ScaledDev*)d_ws;
    const AxisDev* d_axes = (const AxisDev*)((uint8_t*)d_ws + tbytes);
    int* d_coef = (int*)((uint8_t*)d_ws + hdr);
    for (int a0 = 0; a0 < na; a0 += 65535) {
        const int n = na - a0 < 65535 ? na - a0 : 65535;
        hipLaunchKernelGGL(views_taps_kernel, dim3((omax + 255) / 256, n), dim3(256), 0, st, d_axes + a0, n, d_coef);
        const int rc = dafne::check_launch("scene_scaled_tiles_taps");
        if (rc) return rc;
    }
    // rows per workgroup: the most that keep the LDS intermediate and the output rows within the budget
    int by = 32 < patch ? 32 : patch, rows_cap = 0;
    for (;;) {
        rows_cap = 1;
        for (int v = 0; v < n_tiles; v++) {
            const dafne_scaled_tile& d = tiles[v];
            const int r = view_rows_cap((double)d.h / d.new_h, by, d.h, d.filter == kBicubic ? 2.0 : 1.0);
            if (r > rows_cap) rows_cap = r;
        }
        if (by == 1 || 3 * kViewBX * (rows_cap + by) <= kViewLdsBudget) break;
        by /= 2;
    }
    const size_t lds = (size_t)3 * kViewBX * (rows_cap + by);
    if (lds > 64 * 1024) return dafne::fail(DAFNE_E_UNSUPPORTED, "scene_scaled_tiles: %d source rows per output row", rows_cap);
    const unsigned gz = (unsigned)(n_tiles < 65535 ? n_tiles : 65535);
    hipLaunchKernelGGL(scaled_tiles_kernel, dim3((patch + kViewBX - 1) / kViewBX, (patch + by - 1) / by, gz), dim3(256), lds, st,
                       d_tiles, n_tiles, d_axes, d_coef, patch, by, rows_cap, d_out_hwc);
    return dafne::check_launch("scene_scaled_tiles");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------- training views
// The batch the reference trains on (tools/plain_train_net.py:229-256: hflip, vflip, resize, quarter turns), cut straight
// from scenes or tiles: view v = np.rot90(Pillow's BILINEAR resize of the FLIPPED zero-padded window, rot) in the top left
// corner of its cap_h x cap_w slab, 0 in the rest of the slab (ImageList's padding), all written by one launch.
// A workgroup owns a T x T tile of the OUTPUT.  Its pre-rotation rectangle R (T x T of the resized image, possibly hanging
// over it) follows from rot; it runs the horizontal pass for the flipped-window rows the rectangle's vertical taps touch into
// LDS, then the vertical pass, whose result it writes into an LDS copy of the output tile at the ROTATED position (byte
// writes; the copy's pitch is T + 4 bytes = an odd number of words, so the 32 lanes of a half wave that walk down a column
// of the copy on the odd rotations hit 32 different banks).  The tile leaves as 4-byte words in the output's row order for
// every rot; bytes outside the view are written 0 by the same stores.  One writer per output byte, no atomics.
namespace {

struct TrainDev {
    dafne_train_view s;
    int tx, ty;                             // coefficient table of the x / y axis
};

// flipped-window pixel (r, x), channel ch: the flips come BEFORE the resize (the reference's augmentation order)
__device__ __forceinline__ int train_px(const dafne_train_view& s, int r, int x, int ch) {
    const int wr = s.vflip ? s.win_h - 1 - r : r, wx = s.hflip ? s.win_w - 1 - x : x;
    const long long sy = (long long)s.up + wr, sx = (long long)s.left + wx;
    if (sy >= s.h || sx >= s.w) return 0;
    return s.layout_hwc ? s.d_src[((size_t)sy * s.w + sx) * 3 + ch] : s.d_src[((size_t)ch * s.h + sy) * s.w + sx];
}

__global__ void __launch_bounds__(256) train_views_kernel(const TrainDev* __restrict__ views, int n_views,
                                                          const AxisDev* __restrict__ axes, const int* __restrict__ coef, int cap_h,
                                                          int cap_w, int T, int rows_cap, uint8_t* __restrict__ out,
                                                          int32_t* __restrict__ valid_hw) {
    extern __shared__ uint8_t tmp[];         // [3][rows_cap][T], then the output tile [3][T][T + 4]
    const int pitch = T + 4;
    uint8_t* obuf = tmp + (size_t)3 * rows_cap * T;
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * T, oy0 = blockIdx.y * T;
    const int tw = min(T, cap_w - ox0), th = min(T, cap_h - oy0);           // the block's share of the slab (tw % 4 == 0)
    for (int v = blockIdx.z; v < n_views; v += gridDim.z) {
        const TrainDev vd = views[v];
        const dafne_train_view& s = vd.s;
        const int H = s.new_h, W = s.new_w, rot = s.rot;
        if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
            valid_hw[2 * v] = (rot & 1) ? W : H;
            valid_hw[2 * v + 1] = (rot & 1) ? H : W;
        }
        // the tile's rectangle of the resized image: rows ry0 + [0, T), columns rx0 + [0, T)
        //   rot 1: out[i][j] = R[j][W - 1 - i]   rot 2: R[H - 1 - i][W - 1 - j]   rot 3: R[H - 1 - j][i]      (np.rot90)
        const int ry0 = rot == 0 ? oy0 : rot == 1 ? ox0 : rot == 2 ? H - oy0 - T : H - ox0 - T;
        const int rx0 = rot == 0 ? ox0 : rot == 1 ? W - oy0 - T : rot == 2 ? W - ox0 - T : oy0;
        const int ya = max(0, -ry0), yb = min(T, H - ry0), xa = max(0, -rx0), xb = min(T, W - rx0);
        const bool any = ya < yb && xa < xb;                                 // (block-uniform)
        const int* cx = coef + axes[vd.tx].off;
        const int* cy = coef + axes[vd.ty].off;
        int flo = 0;
        if (any) {
            // flipped-window rows of the rectangle's vertical taps: xmin is non-decreasing in the output index, and so is xmin + n
            flo = cy[(size_t)(ry0 + ya) * kTapStride];
            const int* clast = cy + (size_t)(ry0 + yb - 1) * kTapStride;
            const int nrows = min(clast[0] + clast[1] - flo, rows_cap);
            for (int e = tid; e < nrows * T; e += blockDim.x) {
                const int r = e / T, c = e - r * T;
                if (c < xa || c >= xb) continue;
                const int* t = cx + (size_t)(rx0 + c) * kTapStride;
                const int xmin = t[0], n = t[1];
                int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
                for (int x = 0; x < n; x++) {
                    const int k = t[2 + x];
                    a0 += train_px(s, flo + r, xmin + x, 0) * k;
                    a1 += train_px(s, flo + r, xmin + x, 1) * k;
                    a2 += train_px(s, flo + r, xmin + x, 2) * k;
                }
                tmp[(0 * rows_cap + r) * T + c] = clip8(a0);
                tmp[(1 * rows_cap + r) * T + c] = clip8(a1);
                tmp[(2 * rows_cap + r) * T + c] = clip8(a2);
            }
        }
        __syncthreads();
        // vertical pass over the rectangle, written at the rotated place of the output tile; 0 outside the view
        for (int e = tid; e < T * T; e += blockDim.x) {
            const int yl = e / T, c = e - yl * T;
            uint8_t b0 = 0, b1 = 0, b2 = 0;
            if (any && yl >= ya && yl < yb && c >= xa && c < xb) {
                const int* t = cy + (size_t)(ry0 + yl) * kTapStride;
                const int r0 = t[0] - flo, n = t[1];
                int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
                for (int y = 0; y < n; y++) {
                    const int k = t[2 + y];
                    const int r = r0 + y < rows_cap ? r0 + y : rows_cap - 1;     // (never clamps: rows_cap bounds the span)
                    a0 += (int)tmp[(0 * rows_cap + r) * T + c] * k;
                    a1 += (int)tmp[(1 * rows_cap + r) * T + c] * k;
                    a2 += (int)tmp[(2 * rows_cap + r) * T + c] * k;
                }
                b0 = clip8(a0);
                b1 = clip8(a1);
                b2 = clip8(a2);
            }
            const int oyl = rot == 0 ? yl : rot == 1 ? T - 1 - c : rot == 2 ? T - 1 - yl : c;
            const int oxl = rot == 0 ? c : rot == 1 ? yl : rot == 2 ? T - 1 - c : T - 1 - yl;
            uint8_t* o = obuf + oyl * pitch + oxl;
            o[0] = b0;
            o[(size_t)T * pitch] = b1;
            o[(size_t)2 * T * pitch] = b2;
        }
        __syncthreads();
        // the tile's rows as words: byte offset ((v * 3 + ch) * cap_h + y) * cap_w + ox0 is a multiple of 4
        const int wpr = tw / 4;
        for (int e = tid; e < 3 * th * wpr; e += blockDim.x) {
            const int ch = e / (th * wpr), rem = e - ch * th * wpr;
            const int yl = rem / wpr, q = rem - yl * wpr;
            uint32_t* dst = reinterpret_cast<uint32_t*>(out + (((size_t)v * 3 + ch) * cap_h + oy0 + yl) * cap_w + ox0);
            dst[q] = reinterpret_cast<const uint32_t*>(obuf + ((size_t)ch * T + yl) * pitch)[q];
        }
        __syncthreads();
    }
}

struct TrainPlan {
    AxisDev* axes;          // 2 * n_views at most
    int* tx;
    int* ty;
    int n_axes;
    size_t coef_ints;
};

// the distinct (window size, new size) axes of a call; tx / ty: per view its tables.  The caller owns the arrays.
void train_axes(const dafne_train_view* views, int n_views, TrainPlan& p) {
    int na = 0;
    for (int v = 0; v < n_views; v++)
        for (int pass = 0; pass < 2; pass++) {
            const int in = pass ? views[v].win_h : views[v].win_w, o = pass ? views[v].new_h : views[v].new_w;
            int a = 0;
            for (a = na - 1; a >= 0; a--)
                if (p.axes[a].in_size == in && p.axes[a].out_size == o) break;
            if (a < 0) {
                a = na++;
                p.axes[a].in_size = in;
                p.axes[a].out_size = o;
                p.axes[a].filter = kBilinear;
                p.axes[a].reserved = 0;
            }
            (pass ? p.ty : p.tx)[v] = a;
        }
    size_t off = 0;
    for (int a = 0; a < na; a++) {
        p.axes[a].off = off;
        off += (size_t)p.axes[a].out_size * kTapStride;
    }
    p.n_axes = na;
    p.coef_ints = off;
}

bool train_view_ok(const dafne_train_view& s) {
    return s.d_src && s.h >= 1 && s.w >= 1 && (s.layout_hwc == 0 || s.layout_hwc == 1) && s.left >= 0 && s.up >= 0 && s.win_h >= 1 &&
           s.win_w >= 1 && (s.hflip == 0 || s.hflip == 1) && (s.vflip == 0 || s.vflip == 1) && s.new_h >= 1 && s.new_w >= 1 &&
           s.rot >= 0 && s.rot <= 3;
}

size_t train_views_bytes(int n_views) { return dafne::align_up(sizeof(TrainDev) * (size_t)n_views, 256); }

}  // namespace

extern "C" {

size_t dafne_train_views_workspace_bytes(const dafne_train_view* views, int n_views) {
    if (!views || n_views < 1) return 0;
    for (int v = 0; v < n_views; v++)
        if (!train_view_ok(views[v])) return 0;
    TrainPlan p;
    p.axes = new AxisDev[2 * (size_t)n_views];
    p.tx = new int[n_views];
    p.ty = new int[n_views];
    train_axes(views, n_views, p);
    delete[] p.axes;
    delete[] p.tx;
    delete[] p.ty;
    return train_views_bytes(n_views) + scaled_axes_bytes(p.n_axes) + dafne::align_up(p.coef_ints * sizeof(int), 256);
}

int dafne_train_views_u8_hip(const dafne_train_view* views, int n_views, int cap_h, int cap_w, uint8_t* d_out, int32_t* d_valid_hw,
                             void* d_ws, size_t ws_bytes, void* stream) {
    if (!views || !d_out || !d_valid_hw || !d_ws || n_views < 1 || cap_h < 1 || cap_w < 1)
        return dafne::fail(DAFNE_E_INVALID, "train_views: bad args (n_views %d, cap %dx%d)", n_views, cap_h, cap_w);
    if (cap_w % 4 || ((uintptr_t)d_out & 3))
        return dafne::fail(DAFNE_E_UNSUPPORTED, "train_views: cap_w %d is not a multiple of 4, or the output is not 4-byte aligned", cap_w);
    double sy_max = 0.0;
    int in_h_max = 1, omax = 1;
    for (int v = 0; v < n_views; v++) {
        const dafne_train_view& s = views[v];
        if (!train_view_ok(s))
            return dafne::fail(DAFNE_E_INVALID, "train_views: view %d: source %dx%d layout %d window (%d, %d) %dx%d flips %d/%d -> %dx%d rot %d",
                               v, s.h, s.w, s.layout_hwc, s.left, s.up, s.win_h, s.win_w, s.hflip, s.vflip, s.new_h, s.new_w, s.rot);
        const int oh = (s.rot & 1) ? s.new_w : s.new_h, ow = (s.rot & 1) ? s.new_h : s.new_w;
        if (oh > cap_h || ow > cap_w)
            return dafne::fail(DAFNE_E_UNSUPPORTED, "train_views: view %d: %dx%d does not fit the %dx%d slab", v, oh, ow, cap_h, cap_w);
        // the limit of dafne_resize_bilinear_u8_hip: tap count of the widest filter, 2 * ceil(support) + 1
        const double sx = (double)s.win_w / s.new_w, sy = (double)s.win_h / s.new_h;
        if ((sx > 1 ? sx : 1) * 2 + 2 > kMaxTaps || (sy > 1 ? sy : 1) * 2 + 2 > kMaxTaps)
            return dafne::fail(DAFNE_E_UNSUPPORTED, "train_views: view %d: downscale factor above %d", v, kMaxTaps / 2 - 1);
        if (sy > sy_max) sy_max = sy;
        if (s.win_h > in_h_max) in_h_max = s.win_h;
        if (s.new_h > omax) omax = s.new_h;
        if (s.new_w > omax) omax = s.new_w;
    }
    const size_t need = dafne_train_views_workspace_bytes(views, n_views);
    if (ws_bytes < need) return dafne::fail(DAFNE_E_WORKSPACE, "train_views: workspace %zu < %zu", ws_bytes, need);
    TrainPlan p;
    p.axes = new AxisDev[2 * (size_t)n_views];
    p.tx = new int[n_views];
    p.ty = new int[n_views];
    train_axes(views, n_views, p);
    // header: views + axis tables, one copy
    const size_t vbytes = train_views_bytes(n_views), hdr = vbytes + scaled_axes_bytes(p.n_axes);
    uint8_t* blob = new uint8_t[hdr]();
    TrainDev* vd = reinterpret_cast<TrainDev*>(blob);
    for (int v = 0; v < n_views; v++) {
        vd[v].s = views[v];
        vd[v].tx = p.tx[v];
        vd[v].ty = p.ty[v];
    }
    memcpy(blob + vbytes, p.axes, sizeof(AxisDev) * (size_t)p.n_axes);
    const int na = p.n_axes;
    delete[] p.axes;
    delete[] p.tx;
    delete[] p.ty;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t ce = hipMemcpyAsync(d_ws, blob, hdr, hipMemcpyHostToDevice, st);
    delete[] blob;
    if (ce != hipSuccess) return dafne::fail(DAFNE_E_HIP, "train_views: hipMemcpyAsync: %s", hipGetErrorString(ce));
    const TrainDev* d_views = (const TrainDev*)d_ws;
    const AxisDev* d_axes = (const AxisDev*)((uint8_t*)d_ws + vbytes);
    int* d_coef = (int*)((uint8_t*)d_ws + hdr);
    for (int a0 = 0; a0 < na; a0 += 65535) {
        const int n = na - a0 < 65535 ? na - a0 : 65535;
        hipLaunchKernelGGL(views_taps_kernel, dim3((omax + 255) / 256, n), dim3(256), 0, st, d_axes + a0, n, d_coef);
        const int rc = dafne::check_launch("train_views_taps");
        if (rc) return rc;
    }
    // the tile edge: the largest of 64 .. 4 whose LDS intermediate and output tile stay within the budget
    int T = 64, rows_cap = view_rows_cap(sy_max, T, in_h_max);
    while (T > 4 && 3 * T * (rows_cap + T + 4) > kViewLdsBudget) {
        T /= 2;
        rows_cap = view_rows_cap(sy_max, T, in_h_max);
    }
    const size_t lds = (size_t)3 * T * (rows_cap + T + 4);
    if (lds > 64 * 1024) return dafne::fail(DAFNE_E_UNSUPPORTED, "train_views: %d source rows per output tile", rows_cap);
    const unsigned gz = (unsigned)(n_views < 65535 ? n_views : 65535);
    hipLaunchKernelGGL(train_views_kernel, dim3((cap_w + T - 1) / T, (cap_h + T - 1) / T, gz), dim3(256), lds, st, d_views, n_views,
                       d_axes, d_coef, cap_h, cap_w, T, rows_cap, d_out, d_valid_hw);
    return dafne::check_launch("train_views");
}

}  // extern "C"
