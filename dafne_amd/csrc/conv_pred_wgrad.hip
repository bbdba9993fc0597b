// Weight and bias gradient of the head's prediction convolutions (cls_logits, corners_pred + ctrness, center_pred; dafne.py:318-344):
// 3x3 / stride 1 / pad 1, 256 input channels, <= 16 output channels, summed over every pixel of up to five levels (gfx950).
//
//     dW[co, ci, kh, kw] = sum over (level, image, y, x) of g[y, x, co] * X[y + kh - 1, x + kw - 1, ci]        db[co] = sum of g
//
// X is the bf16 number conv3x3_pred16_kernel multiplies: the stored haloed map, or (GN_INPUT) GroupNorm + ReLU of it in the
// expression of gn_apply_kernel, rounded to bf16, and ZERO outside the image (the halo is not relu(beta)).
//
// The product is a GEMM whose K runs over PIXELS: [16 output channels] x [pixels] . [pixels] x [9 taps x 256 channels].
//   * a workgroup (4 waves) walks tiles of 4 x 32 output pixels over all levels and keeps its whole 16 x 2304 fp32 partial in
//     accumulators: wave w owns input channels 64w .. 64w + 63, 9 taps x 4 blocks of 16 channels = 36 tiles of 16 x 16;
//   * a wave stages ITS 64 channels of the tile's 6 x 34 input patch (128 B per pixel: one cache line) in its own LDS region,
//     normalising on the way (GN_INPUT); nothing is shared between waves, so the tile loop has no workgroup barrier and the four
//     waves of a CU overlap each other's loads and matrix work;
//   * v_mfma_f32_16x16x32_bf16 with K = the 32 pixels of a tile row: the B operand (8 consecutive pixels of one channel per lane)
//     comes out of the pixel-major LDS image through ds_read_b64_tr_b16, shifted by (kh, kw) pixels per tap; the A operand is g,
//     fp32, fed as a hi + lo bf16 pair (two MFMAs per fragment: |g - hi - lo| <= 2^-16 |g|), straight from global memory;
//   * db rides along as a 37th tile against a fragment of ones;
//   * no atomics: every workgroup writes its partial once to the workspace, pred_wgrad_reduce_kernel adds the partials in
//     workgroup order in fp64 and writes every element of dW (OIHW) and db.  Which tiles a workgroup walks is a function of the
//     shapes and the CU count only, so the bits are equal from run to run.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int kMaxSegs = 5;                         // what dafne_conv2d_nhwc_bf16_hip takes
constexpr int kCin = 256, kMaxCout = 16;
constexpr int kTH = 4, kTW = 32;                    // tile of output pixels: one k32 step per row
constexpr int kPC = kTW + 2;                        // patch columns
constexpr int kPR = (kTH + 2) * kPC;                // 204 patch pixels
constexpr int kWaveLds = kPR * 128;                 // 26 112 B: [patch pixel][64 channels] bf16, 16-byte chunks XOR-swizzled by column
constexpr int kNW = 4, kNT = 256;
constexpr int kSmem = kNW * kWaveLds;               // 104 448 B: one workgroup per CU
constexpr int kPieces = (kPR + 7) / 8;              // 26 passes of 8 pixels x 8 chunks per wave
constexpr int kRow = kCin * 9;                      // 2304 elements of dW per output channel
constexpr int kPart = kMaxCout * kRow + kMaxCout;   // floats of one workgroup's partial: dW rows, then db
static_assert(kPieces % 2 == 0, "two load batches");
static_assert(kSmem <= 160 * 1024, "LDS budget");

struct WgSeg {
    const char* in;      // bf16 [N, H+2, W+2, 256]
    const float* g;      // fp32 [N, H, W, ps]
    int H, W, tiles_x, tiles_per_img, tile0;
};

struct WgDev {
    WgSeg seg[kMaxSegs];
    int n_segs, N, Cout, ps, mtiles;
    const float* stats;  // [n_segs][N][32][2] mean, rstd (GN_INPUT)
    const float* gamma;  // [256]
    const float* beta;   // [256]
    float* ws;           // [workgroups][kPart]
};

__device__ __forceinline__ unsigned short bf16_bits(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }

template <bool GNIN>
__global__ void __launch_bounds__(kNT) pred_wgrad_kernel(WgDev P) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* wl = lds + wave * kWaveLds;
    const int q = lane & 7, prow = lane >> 3;       // staging: 16-byte chunk (8 channels), pixel of a pass
    const int fcol = lane & 15, kg = lane >> 4;     // fragment column / row, 8-pixel K group
    const int tq = fcol >> 2, tp = fcol & 3;        // transposed read: this lane addresses pixel tq, channels 4tp .. 4tp + 3 of its block

    float gam[8], bet[8];
    if (GNIN) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            gam[k] = P.gamma[wave * 64 + q * 8 + k];
            bet[k] = P.beta[wave * 64 + q * 8 + k];
        }
    }
    bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; j++) ones[j] = (__bf16)1.0f;

    f32x4 acc[36], accb;
#pragma unroll
    for (int i = 0; i < 36; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    accb = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int t = (int)blockIdx.x; t < P.mtiles; t += (int)gridDim.x) {
        int si = 0;
#pragma unroll
        for (int k = 1; k < kMaxSegs; k++)
            if (k < P.n_segs && t >= P.seg[k].tile0) si = k;
        const WgSeg& S = P.seg[si];
        const int H = S.H, W = S.W, Hp = H + 2, Wp = W + 2;
        const int tloc = t - S.tile0;
        const int img = tloc / S.tiles_per_img;
        const int tt = tloc - img * S.tiles_per_img;
        const int ty = tt / S.tiles_x;
        const int Y0 = ty * kTH, X0 = (tt - ty * S.tiles_x) * kTW;

        // ---- g of the tile: lane = (output channel fcol, pixels 8kg .. 8kg + 7) of each of the four rows; pixels beyond the map,
        // channels beyond Cout and the gap of a strided buffer are never read (clamped address, value replaced by zero)
        float gv[kTH][8];
        {
            const int cc = fcol < P.Cout ? fcol : P.Cout - 1;
#pragma unroll
            for (int ry = 0; ry < kTH; ry++) {
                const int y = Y0 + ry, yy = y < H ? y : H - 1;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int x = X0 + 8 * kg + j, xx = x < W ? x : W - 1;
                    const float v = S.g[((size_t)(img * H + yy) * W + xx) * P.ps + cc];
                    gv[ry][j] = (y < H && x < W && fcol < P.Cout) ? v : 0.f;
                }
            }
        }
        float mean = 0.f, rstd = 0.f;
        if (GNIN) {
            const float* st = P.stats + ((size_t)si * P.N + img) * (kCin / 8) * 2 + (wave * 8 + q) * 2;
            mean = st[0];
            rstd = st[1];
        }
        // ---- this wave's 64 channels of the patch: global -> (GroupNorm + ReLU) -> LDS.  Patch pixel (py, px) is haloed pixel
        // (Y0 + py, X0 + px); what lies beyond the haloed map (and, GN_INPUT, everything outside the image) is written as zero
        const char* src = S.in + wave * 128 + q * 16;
#pragma unroll
        for (int b = 0; b < 2; b++) {
            u32x4 raw[kPieces / 2];
            unsigned keep[kPieces / 2];
#pragma unroll
            for (int i = 0; i < kPieces / 2; i++) {
                int r = (b * (kPieces / 2) + i) * 8 + prow;
                r = r < kPR ? r : kPR - 1;
                const int py = r / kPC, px = r - py * kPC;
                int gy = Y0 + py, gx = X0 + px;
                const bool ok = GNIN ? (gy >= 1 && gy <= H && gx >= 1 && gx <= W) : (gy < Hp && gx < Wp);
                gy = gy < Hp ? gy : Hp - 1;
                gx = gx < Wp ? gx : Wp - 1;
                keep[i] = ok ? 0xffffffffu : 0u;
                const unsigned off = ((unsigned)(img * Hp + gy) * (unsigned)Wp + (unsigned)gx) * (unsigned)(kCin * 2);
                raw[i] = *(const u32x4*)(src + (size_t)off);
            }
#pragma unroll
            for (int i = 0; i < kPieces / 2; i++) {
                const int r = (b * (kPieces / 2) + i) * 8 + prow;
                unsigned w[4] = {raw[i].x, raw[i].y, raw[i].z, raw[i].w};
                if (GNIN) {
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        // the expression of gn_apply_kernel: (x - mean) * rstd, one fused multiply-add with gamma and beta, bf16, ReLU
                        const float x0 = __uint_as_float(w[j] << 16), x1 = __uint_as_float(w[j] & 0xffff0000u);
                        const float y0 = __builtin_fmaf((x0 - mean) * rstd, gam[2 * j], bet[2 * j]);
                        const float y1 = __builtin_fmaf((x1 - mean) * rstd, gam[2 * j + 1], bet[2 * j + 1]);
                        unsigned lo = bf16_bits(y0), hi = bf16_bits(y1);
                        lo = (lo & 0x8000u) ? 0u : lo;
                        hi = (hi & 0x8000u) ? 0u : hi;
                        w[j] = lo | (hi << 16);
                    }
                }
                const u32x4 o = {w[0] & keep[i], w[1] & keep[i], w[2] & keep[i], w[3] & keep[i]};
                const int py = r / kPC, px = r - py * kPC;
                if (r < kPR) *(u32x4*)(wl + r * 128 + ((q ^ ((px >> 1) & 7)) << 4)) = o;
            }
        }
        // the wave's own writes, read back by other lanes of the same wave: LDS serves a wave in order
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();

        // ---- one k32 step per tile row
#pragma unroll
        for (int ry = 0; ry < kTH; ry++) {
            bf16x8 ahi, alo;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const __bf16 h = (__bf16)gv[ry][j];
                ahi[j] = h;
                alo[j] = (__bf16)(gv[ry][j] - (float)h);
            }
            accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, ones, accb, 0, 0, 0);
            accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, ones, accb, 0, 0, 0);
#pragma unroll
            for (int kh = 0; kh < 3; kh++)
#pragma unroll
                for (int kw = 0; kw < 3; kw++) {
                    // element e of read h is patch pixel (ry + kh, 8kg + 4h + e + kw): k = 8kg + 4h + e, the pixel of g's element
                    const int c0 = 8 * kg + tq + kw, c1 = c0 + 4;
                    const int r0 = (ry + kh) * kPC + c0, r1 = r0 + 4;
#pragma unroll
                    for (int cb = 0; cb < 4; cb++) {
                        const int chunk = cb * 2 + (tp >> 1);
                        const s16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (lds_s16x4*)(wl + r0 * 128 + ((chunk ^ ((c0 >> 1) & 7)) << 4) + (tp & 1) * 8));
                        const s16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (lds_s16x4*)(wl + r1 * 128 + ((chunk ^ ((c1 >> 1) & 7)) << 4) + (tp & 1) * 8));
                        const bf16x8 bf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
                        f32x4& a = acc[(kh * 3 + kw) * 4 + cb];
                        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, bf, a, 0, 0, 0);
                        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, bf, a, 0, 0, 0);
                    }
                }
        }
        // the next tile's writes wait for these reads: one wave, in order
        __builtin_amdgcn_wave_barrier();
    }

    // ---- the partial: accumulator register k of lane (kg, fcol) is (output channel 4kg + k, input channel 64 wave + 16 cb + fcol)
    float* part = P.ws + (size_t)blockIdx.x * kPart;
#pragma unroll
    for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int cb = 0; cb < 4; cb++)
#pragma unroll
            for (int k = 0; k < 4; k++)
                part[(4 * kg + k) * kRow + (wave * 64 + cb * 16 + fcol) * 9 + tap] = acc[tap * 4 + cb][k];
    if (wave == 0 && fcol == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) part[kMaxCout * kRow + 4 * kg + k] = accb[k];
    }
}

// dW[e] / db[co] = the partials of all workgroups added in workgroup order, in fp64; one thread per element
__global__ void __launch_bounds__(256) pred_wgrad_reduce_kernel(const float* __restrict__ ws, int nparts, int Cout, float* __restrict__ dW,
                                                                float* __restrict__ db) {
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int nw = Cout * kRow;
    if (e >= nw + Cout) return;
    const float* p = ws + (e < nw ? e : kMaxCout * kRow + (e - nw));
    double s = 0.0;
    for (int k = 0; k < nparts; k++) s += (double)p[(size_t)k * kPart];
    if (e < nw) dW[e] = (float)s;
    else db[e - nw] = (float)s;
}

// -> DAFNE_OK with D filled (pointers of the gradients excepted), or the refusal
int wg_build(WgDev& D, const dafne_conv_params* p, const dafne_conv_seg* segs, int ps) {
    if (!p || !segs) return dafne::fail(DAFNE_E_INVALID, "pred_wgrad: null params");
    if (p->n_segs < 1 || p->n_segs > kMaxSegs || p->n_images < 1)
        return dafne::fail(DAFNE_E_INVALID, "pred_wgrad: %d segments / %d images (1..%d segments)", p->n_segs, p->n_images, kMaxSegs);
    if (p->flags & ~(DAFNE_CONV_OUT_F32 | DAFNE_CONV_GN_INPUT | DAFNE_CONV_EXCLUSIVE))
        return dafne::fail(DAFNE_E_INVALID, "pred_wgrad: flags 0x%x (a prediction call has OUT_F32, GN_INPUT, EXCLUSIVE)", p->flags);
    if (p->Cin != kCin) return dafne::fail(DAFNE_E_UNSUPPORTED, "pred_wgrad: Cin %d, not 256", p->Cin);
    if (p->Cout < 1 || p->Cout > kMaxCout) return dafne::fail(DAFNE_E_UNSUPPORTED, "pred_wgrad: Cout %d outside 1..16", p->Cout);
    if (p->KH != 3 || p->KW != 3 || p->stride != 1 || p->pad != 1) return dafne::fail(DAFNE_E_UNSUPPORTED, "pred_wgrad: only 3x3 / stride 1 / pad 1");
    if (ps < p->Cout) return dafne::fail(DAFNE_E_INVALID, "pred_wgrad: pixel stride %d below Cout %d", ps, p->Cout);
    if ((p->flags & DAFNE_CONV_GN_INPUT) && (!p->d_in_gn_stats || !p->d_in_gn_gamma || !p->d_in_gn_beta))
        return dafne::fail(DAFNE_E_INVALID, "pred_wgrad: GN_INPUT without statistics / affine pointers");
    long long t = 0;
    for (int s = 0; s < p->n_segs; s++) {
        const dafne_conv_seg& g = segs[s];
        if (!g.d_in || g.Hout < 1 || g.Wout < 1 || g.Hin != g.Hout || g.Win != g.Wout) return dafne::fail(DAFNE_E_INVALID, "pred_wgrad: segment %d", s);
        // the limits of the forward call: 2^20 pixels per image, the haloed map of all images below 2^32 bytes
        if ((long long)g.Hout * g.Wout > (1 << 20) || g.Wout > (1 << 12))
            return dafne::fail(DAFNE_E_UNSUPPORTED, "pred_wgrad: segment %d output %dx%d above 2^20 pixels per image", s, g.Hout, g.Wout);
        const long long in_bytes = (long long)p->n_images * (g.Hin + 2) * (g.Win + 2) * kCin * 2;
        if (in_bytes > 0xffffffffll)
            return dafne::fail(DAFNE_E_UNSUPPORTED, "pred_wgrad: segment %d input of %lld bytes (%d images of %dx%dx%d) is beyond 32-bit offsets: "
                                                    "split the batch", s, in_bytes, p->n_images, g.Hin, g.Win, kCin);
        WgSeg& o = D.seg[s];
        o.in = (const char*)g.d_in;
        o.g = nullptr;
        o.H = g.Hout; o.W = g.Wout;
        o.tiles_x = (g.Wout + kTW - 1) / kTW;
        o.tiles_per_img = o.tiles_x * ((g.Hout + kTH - 1) / kTH);
        o.tile0 = (int)t;
        t += (long long)o.tiles_per_img * p->n_images;
        if (t > 0x7fffffffll) return dafne::fail(DAFNE_E_UNSUPPORTED, "pred_wgrad: too many tiles");
    }
    D.n_segs = p->n_segs; D.N = p->n_images; D.Cout = p->Cout; D.ps = ps; D.mtiles = (int)t;
    D.stats = p->d_in_gn_stats; D.gamma = p->d_in_gn_gamma; D.beta = p->d_in_gn_beta;
    D.ws = nullptr;
    return DAFNE_OK;
}

// workgroups of a launch: one per CU, never more than tiles
int wg_grid(const WgDev& D, int* grid) {
    int cus = 0;
    if (int rc = dafne::device_cus(&cus)) return rc;
    *grid = D.mtiles < cus ? D.mtiles : cus;
    return DAFNE_OK;
}

}  // namespace

extern "C" {

size_t dafne_pred_wgrad_workspace_bytes(const dafne_conv_params* prm, const dafne_conv_seg* segs) {
    WgDev D;
    if (wg_build(D, prm, segs, prm ? prm->Cout : 0)) return 0;
    int grid = 0;
    if (wg_grid(D, &grid)) return 0;
    return (size_t)grid * kPart * sizeof(float);
}

int dafne_pred_wgrad_hip(const dafne_conv_params* prm, const dafne_conv_seg* segs, const float* const* d_gout, int gout_ps, float* d_dw,
                         float* d_db, void* d_ws, size_t ws_bytes, void* stream) {
    WgDev D;
    if (int rc = wg_build(D, prm, segs, gout_ps)) return rc;
    if (!d_gout || !d_dw || !d_db || !d_ws) return dafne::fail(DAFNE_E_INVALID, "pred_wgrad: null argument");
    for (int s = 0; s < D.n_segs; s++) {
        if (!d_gout[s]) return dafne::fail(DAFNE_E_INVALID, "pred_wgrad: null gradient of segment %d", s);
        D.seg[s].g = d_gout[s];
    }
    int grid = 0;
    if (int rc = wg_grid(D, &grid)) return rc;
    const size_t need = (size_t)grid * kPart * sizeof(float);
    if (ws_bytes < need) return dafne::fail(DAFNE_E_WORKSPACE, "pred_wgrad: workspace %zu < %zu", ws_bytes, need);
    D.ws = (float*)d_ws;
    hipStream_t st = (hipStream_t)stream;
    DAFNE_MAX_LDS_ONCE(kSmem, (const void*)pred_wgrad_kernel<false>, (const void*)pred_wgrad_kernel<true>);
    if (prm->flags & DAFNE_CONV_GN_INPUT) hipLaunchKernelGGL(pred_wgrad_kernel<true>, dim3(grid), dim3(kNT), kSmem, st, D);
    else hipLaunchKernelGGL(pred_wgrad_kernel<false>, dim3(grid), dim3(kNT), kSmem, st, D);
    if (int rc = dafne::check_launch("pred_wgrad")) return rc;
    const int total = D.Cout * kRow + D.Cout;
    hipLaunchKernelGGL(pred_wgrad_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, st, (const float*)D.ws, grid, D.Cout, d_dw, d_db);
    return dafne::check_launch("pred_wgrad_reduce");
}

}  // extern "C"
