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

namespace {

constexpr int kPrec = 22;      // PRECISION_BITS = 32 - 8 - 2
constexpr int kMaxTaps = 64;   // downscale factors up to ~31x

struct Taps {
    int xmin, n;
    int k[kMaxTaps];
};

// coefficients of output index i for an axis of in_size -> out_size samples
__device__ __forceinline__ void taps_for(int i, int in_size, int out_size, Taps& t) {
    const double scale = (double)(float)in_size / out_size;      // box = (0, in_size) as floats
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
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
        const double v = a < 1.0 ? 1.0 - a : 0.0;
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
