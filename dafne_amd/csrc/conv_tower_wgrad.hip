// Weight gradient of one tower convolution of the head (cls_tower / corners_tower .0 .3 .6 .9; dafne.py:350-372): 3x3 / stride 1 /
// pad 1, 256 -> 256 channels, summed over every pixel of up to five levels (gfx950).
//
//     dW[co, ci, kh, kw] = sum over (level, image, y, x) of g[y, x, co] * X[y + kh - 1, x + kw - 1, ci]
//
// X is the bf16 number the forward multiplied, exactly as in conv_pred_wgrad.hip: the stored haloed map, or (GN_INPUT) GroupNorm +
// ReLU of it in the expression of gn_apply_kernel, rounded to bf16, and ZERO outside the image (the halo is not relu(beta)).  There
// is no bias gradient here: it comes out of the data-gradient call of the layer behind (conv_tower_dgrad.hip, conv_pred_dgrad.hip).
//
// The product is a GEMM whose K runs over PIXELS: [256 output channels] x [pixels] . [pixels] x [9 taps x 256 channels], and its
// result, 256 x 2304 fp32 (2.4 MB), is what has to be split:
//   * CHOICE of the accumulator split.  A wave keeps 16 output channels x 9 taps x 32 input channels = 18 tiles of 16 x 16 = 72
//     accumulator registers per lane.  conv_pred_wgrad.hip's split (64 input channels, 144 registers) needs a lone wave per SIMD
//     (512 registers): compiled for two waves it spills over 200 registers, and alone it has nothing to run its staging under.
//     With 72 accumulators, g (32) and a staging batch (16) a wave has room in 256 registers, so the workgroup is EIGHT waves, two
//     per SIMD (4 groups of 16 output channels x 2 halves of 32 input channels), all on the SAME 64 input channels: it owns
//     block (64 co, 64 ci) of dW, all nine taps, in 8 x 64 x 72 of the CU's 4 x 64 x 512 registers and 26 KB of its 160 KB of LDS;
//   * so a patch is staged and normalised ONCE per 64 output channels: the workgroup's 512 threads bring the 64 input channels of
//     the tile's 6 x 34 input patch (128 B per pixel: one cache line) into ONE LDS image of 26 112 B, normalising on the way
//     (GN_INPUT), and the eight waves read it.  Sixteen launches of pred_wgrad_kernel over 16-channel slices of g stage every patch
//     sixteen times; this kernel four times;
//   * the launch is 16 blocks x P pixel splits: workgroup (block, p) walks tiles p, p + P, ... of 4 x 32 output pixels over all
//     levels.  P = CUs / 16 (one workgroup per CU), never more than tiles;
//   * v_mfma_f32_16x16x32_bf16 with K = the 32 pixels of a tile row: the B operand (8 consecutive pixels of one channel per lane)
//     comes out of the pixel-major LDS image through ds_read_b64_tr_b16, shifted by (kh, kw) pixels per tap; the A operand is g,
//     fp32, fed as a hi + lo bf16 pair (two MFMAs per fragment: |g - hi - lo| <= 2^-16 |g|), straight from global memory;
//   * no atomics: workgroup (block, p) writes its block of partial slab p once, tower_wgrad_reduce_kernel adds the P slabs in order
//     in fp64 and writes every element of dW (OIHW).  Which tiles a workgroup walks is a function of the shapes and the CU count
//     only, so the bits are equal from run to run.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int kMaxSegs = 5;                         // what dafne_conv2d_nhwc_bf16_hip takes
constexpr int kC = 256;                             // Cin = Cout
constexpr int kTH = 4, kTW = 32;                    // tile of output pixels: one k32 step per row
constexpr int kPC = kTW + 2;                        // patch columns
constexpr int kPR = (kTH + 2) * kPC;                // 204 patch pixels
constexpr int kLds = kPR * 128;                     // 26 112 B: [patch pixel][64 channels] bf16, 16-byte chunks XOR-swizzled by column
constexpr int kNT = 512;
constexpr int kBlk = 64;                            // a workgroup's block of dW: 64 output x 64 input channels
constexpr int kBlocks = (kC / kBlk) * (kC / kBlk);  // 16
constexpr int kPasses = (kPR + 63) / 64;            // 4 passes of 64 pixels x 8 chunks per workgroup
constexpr int kRow = kC * 9;                        // 2304 elements of dW per output channel
constexpr int kSlab = kC * kRow;                    // floats of one pixel split's partial: all of dW
constexpr int kAllowed = DAFNE_CONV_GN_STATS | DAFNE_CONV_GN_INPUT | DAFNE_CONV_GN_FINALIZE | DAFNE_CONV_EXCLUSIVE | DAFNE_CONV_FRAG16;

struct TwSeg {
    const char* in;      // bf16 [N, H+2, W+2, 256]
    const float* g;      // fp32 [N, H, W, 256]
    int H, W, tiles_x, tiles_per_img, tile0;
};

struct TwDev {
    TwSeg seg[kMaxSegs];
    int n_segs, N, mtiles, splits;
    const float* stats;  // [n_segs][N][32][2] mean, rstd (GN_INPUT)
    const float* gamma;  // [256]
    const float* beta;   // [256]
    float* ws;           // [splits][kSlab]
};

__device__ __forceinline__ unsigned short bf16_bits(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }

template <bool GNIN>
__global__ void __launch_bounds__(kNT) tower_wgrad_kernel(TwDev P) {
    __shared__ __attribute__((aligned(16))) char lds[kLds];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int blk = (int)blockIdx.x % kBlocks, split = (int)blockIdx.x / kBlocks;
    const int cob = blk >> 2, cib = blk & 3;        // the block: output channels 64 cob .., input channels 64 cib ..
    const int q = tid & 7, prow = tid >> 3;         // staging: 16-byte chunk (8 channels), pixel of a pass
    const int fcol = lane & 15, kg = lane >> 4;     // fragment column / row, 8-pixel K group
    const int tq = fcol >> 2, tp = fcol & 3;        // transposed read: this lane addresses pixel tq, channels 4tp .. 4tp + 3 of its block
    const int wco = wave & 3, wci = wave >> 2;      // the wave's 16 output channels and 32 input channels of the block
    const int co = cob * kBlk + wco * 16 + fcol;    // the output channel whose g this lane feeds

    float gam[8], bet[8];
    if (GNIN) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            gam[k] = P.gamma[cib * kBlk + q * 8 + k];
            bet[k] = P.beta[cib * kBlk + q * 8 + k];
        }
    }

    f32x4 acc[18];
#pragma unroll
    for (int i = 0; i < 18; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int t = split; t < P.mtiles; t += P.splits) {
        int si = 0;
#pragma unroll
        for (int k = 1; k < kMaxSegs; k++)
            if (k < P.n_segs && t >= P.seg[k].tile0) si = k;
        const TwSeg& S = P.seg[si];
        const int H = S.H, W = S.W, Hp = H + 2, Wp = W + 2;
        const int tloc = t - S.tile0;
        const int img = tloc / S.tiles_per_img;
        const int tt = tloc - img * S.tiles_per_img;
        const int ty = tt / S.tiles_x;
        const int Y0 = ty * kTH, X0 = (tt - ty * S.tiles_x) * kTW;

        // ---- g of the tile: lane = (output channel co, pixels 8kg .. 8kg + 7) of each of the four rows; pixels beyond the map are
        // never read (clamped address, value replaced by zero)
        float gv[kTH][8];
#pragma unroll
        for (int ry = 0; ry < kTH; ry++) {
            const int y = Y0 + ry, yy = y < H ? y : H - 1;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int x = X0 + 8 * kg + j, xx = x < W ? x : W - 1;
                const float v = S.g[((size_t)(img * H + yy) * W + xx) * kC + co];
                gv[ry][j] = (y < H && x < W) ? v : 0.f;
            }
        }
        float mean = 0.f, rstd = 0.f;
        if (GNIN) {
            const float* st = P.stats + ((size_t)si * P.N + img) * (kC / 8) * 2 + (cib * 8 + q) * 2;
            mean = st[0];
            rstd = st[1];
        }
        // ---- the block's 64 input channels of the patch: global -> (GroupNorm + ReLU) -> LDS.  Patch pixel (py, px) is haloed pixel
        // (Y0 + py, X0 + px); what lies beyond the haloed map (and, GN_INPUT, everything outside the image) is written as zero
        const char* src = S.in + cib * 128 + q * 16;
        u32x4 raw[kPasses];
        unsigned keep[kPasses];
#pragma unroll
        for (int i = 0; i < kPasses; i++) {
            int r = i * 64 + prow;
            r = r < kPR ? r : kPR - 1;
            const int py = r / kPC, px = r - py * kPC;
            int gy = Y0 + py, gx = X0 + px;
            const bool ok = GNIN ? (gy >= 1 && gy <= H && gx >= 1 && gx <= W) : (gy < Hp && gx < Wp);
            gy = gy < Hp ? gy : Hp - 1;
            gx = gx < Wp ? gx : Wp - 1;
            keep[i] = ok ? 0xffffffffu : 0u;
            const unsigned off = ((unsigned)(img * Hp + gy) * (unsigned)Wp + (unsigned)gx) * (unsigned)(kC * 2);
            raw[i] = *(const u32x4*)(src + (size_t)off);
        }
#pragma unroll
        for (int i = 0; i < kPasses; i++) {
            const int r = i * 64 + prow;
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
            if (r < kPR) *(u32x4*)(lds + r * 128 + ((q ^ ((px >> 1) & 7)) << 4)) = o;
        }
        __syncthreads();

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
#pragma unroll
            for (int kh = 0; kh < 3; kh++)
#pragma unroll
                for (int kw = 0; kw < 3; kw++) {
                    // element e of read h is patch pixel (ry + kh, 8kg + 4h + e + kw): k = 8kg + 4h + e, the pixel of g's element
                    const int c0 = 8 * kg + tq + kw, c1 = c0 + 4;
                    const int r0 = (ry + kh) * kPC + c0, r1 = r0 + 4;
#pragma unroll
                    for (int cb = 0; cb < 2; cb++) {
                        const int chunk = (wci * 2 + cb) * 2 + (tp >> 1);
                        const s16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (lds_s16x4*)(lds + r0 * 128 + ((chunk ^ ((c0 >> 1) & 7)) << 4) + (tp & 1) * 8));
                        const s16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (lds_s16x4*)(lds + r1 * 128 + ((chunk ^ ((c1 >> 1) & 7)) << 4) + (tp & 1) * 8));
                        const bf16x8 bf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
                        f32x4& a = acc[(kh * 3 + kw) * 2 + cb];
                        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, bf, a, 0, 0, 0);
                        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, bf, a, 0, 0, 0);
                    }
                }
        }
        // the next tile's writes wait for these reads
        __syncthreads();
    }

    // ---- the partial: accumulator register k of lane (kg, fcol) is (output channel 64 cob + 16 wco + 4kg + k, input channel
    // 64 cib + 32 wci + 16 cb + fcol).  A split beyond the tiles (never launched: splits <= tiles) would write zeros
    float* part = P.ws + (size_t)split * kSlab;
#pragma unroll
    for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int cb = 0; cb < 2; cb++)
#pragma unroll
            for (int k = 0; k < 4; k++)
                part[(cob * kBlk + wco * 16 + 4 * kg + k) * kRow + (cib * kBlk + wci * 32 + cb * 16 + fcol) * 9 + tap] = acc[tap * 2 + cb][k];
}

// dW[e] = the partial slabs added in split order, in fp64; one thread per element
__global__ void __launch_bounds__(256) tower_wgrad_reduce_kernel(const float* __restrict__ ws, int nparts, float* __restrict__ dW) {
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= kSlab) return;
    double s = 0.0;
    for (int k = 0; k < nparts; k++) s += (double)ws[(size_t)k * kSlab + e];
    dW[e] = (float)s;
}

// -> DAFNE_OK with D filled (pointers of the gradients and the split count excepted), or the refusal
int tw_build(TwDev& D, const dafne_conv_params* p, const dafne_conv_seg* segs) {
    if (!p || !segs) return dafne::fail(DAFNE_E_INVALID, "tower_wgrad: null params");
    if (p->n_segs < 1 || p->n_segs > kMaxSegs || p->n_images < 1)
        return dafne::fail(DAFNE_E_INVALID, "tower_wgrad: %d segments / %d images (1..%d segments)", p->n_segs, p->n_images, kMaxSegs);
    if (p->flags & ~(unsigned)kAllowed)
        return dafne::fail(DAFNE_E_INVALID, "tower_wgrad: flags 0x%x (a tower call has GN_STATS, GN_INPUT, GN_FINALIZE, EXCLUSIVE, FRAG16)", p->flags);
    if (p->Cin != kC || p->Cout != kC) return dafne::fail(DAFNE_E_UNSUPPORTED, "tower_wgrad: %d -> %d channels, not 256 -> 256", p->Cin, p->Cout);
    if (p->KH != 3 || p->KW != 3 || p->stride != 1 || p->pad != 1) return dafne::fail(DAFNE_E_UNSUPPORTED, "tower_wgrad: only 3x3 / stride 1 / pad 1");
    if ((p->flags & DAFNE_CONV_GN_INPUT) && (!p->d_in_gn_stats || !p->d_in_gn_gamma || !p->d_in_gn_beta))
        return dafne::fail(DAFNE_E_INVALID, "tower_wgrad: GN_INPUT without statistics / affine pointers");
    long long t = 0;
    for (int s = 0; s < p->n_segs; s++) {
        const dafne_conv_seg& g = segs[s];
        if (!g.d_in || g.Hout < 1 || g.Wout < 1 || g.Hin != g.Hout || g.Win != g.Wout) return dafne::fail(DAFNE_E_INVALID, "tower_wgrad: segment %d", s);
        // the limits of the forward call: 2^20 pixels per image, the haloed map of all images below 2^32 bytes
        if ((long long)g.Hout * g.Wout > (1 << 20) || g.Wout > (1 << 12))
            return dafne::fail(DAFNE_E_UNSUPPORTED, "tower_wgrad: segment %d output %dx%d above 2^20 pixels per image", s, g.Hout, g.Wout);
        const long long in_bytes = (long long)p->n_images * (g.Hin + 2) * (g.Win + 2) * kC * 2;
        if (in_bytes > 0xffffffffll)
            return dafne::fail(DAFNE_E_UNSUPPORTED, "tower_wgrad: segment %d input of %lld bytes (%d images of %dx%dx%d) is beyond 32-bit offsets: "
                                                    "split the batch", s, in_bytes, p->n_images, g.Hin, g.Win, kC);
        TwSeg& o = D.seg[s];
        o.in = (const char*)g.d_in;
        o.g = nullptr;
        o.H = g.Hout; o.W = g.Wout;
        o.tiles_x = (g.Wout + kTW - 1) / kTW;
        o.tiles_per_img = o.tiles_x * ((g.Hout + kTH - 1) / kTH);
        o.tile0 = (int)t;
        t += (long long)o.tiles_per_img * p->n_images;
        if (t > 0x7fffffffll) return dafne::fail(DAFNE_E_UNSUPPORTED, "tower_wgrad: too many tiles");
    }
    D.n_segs = p->n_segs; D.N = p->n_images; D.mtiles = (int)t; D.splits = 0;
    D.stats = p->d_in_gn_stats; D.gamma = p->d_in_gn_gamma; D.beta = p->d_in_gn_beta;
    D.ws = nullptr;
    return DAFNE_OK;
}

// pixel splits of a launch: 16 blocks x splits = one workgroup (two waves per SIMD) per CU, never more splits than tiles
int tw_splits(const TwDev& D, int* splits) {
    int cus = 0;
    if (int rc = dafne::device_cus(&cus)) return rc;
    int s = cus / kBlocks;
    s = s < 1 ? 1 : s;
    *splits = D.mtiles < s ? D.mtiles : s;
    return DAFNE_OK;
}

}  // namespace

extern "C" {

size_t dafne_tower_wgrad_workspace_bytes(const dafne_conv_params* prm, const dafne_conv_seg* segs) {
    TwDev D;
    if (tw_build(D, prm, segs)) return 0;
    int splits = 0;
    if (tw_splits(D, &splits)) return 0;
    return (size_t)splits * kSlab * sizeof(float);
}

int dafne_tower_wgrad_hip(const dafne_conv_params* prm, const dafne_conv_seg* segs, const float* const* d_gout, float* d_dw, void* d_ws,
                          size_t ws_bytes, void* stream) {
    TwDev D;
    if (int rc = tw_build(D, prm, segs)) return rc;
    if (!d_gout || !d_dw || !d_ws) return dafne::fail(DAFNE_E_INVALID, "tower_wgrad: null argument");
    for (int s = 0; s < D.n_segs; s++) {
        if (!d_gout[s]) return dafne::fail(DAFNE_E_INVALID, "tower_wgrad: null gradient of segment %d", s);
        D.seg[s].g = d_gout[s];
    }
    int splits = 0;
    if (int rc = tw_splits(D, &splits)) return rc;
    const size_t need = (size_t)splits * kSlab * sizeof(float);
    if (ws_bytes < need) return dafne::fail(DAFNE_E_WORKSPACE, "tower_wgrad: workspace %zu < %zu", ws_bytes, need);
    D.splits = splits;
    D.ws = (float*)d_ws;
    hipStream_t st = (hipStream_t)stream;
    if (prm->flags & DAFNE_CONV_GN_INPUT) hipLaunchKernelGGL(tower_wgrad_kernel<true>, dim3(kBlocks * splits), dim3(kNT), 0, st, D);
    else hipLaunchKernelGGL(tower_wgrad_kernel<false>, dim3(kBlocks * splits), dim3(kNT), 0, st, D);
    if (int rc = dafne::check_launch("tower_wgrad")) return rc;
    hipLaunchKernelGGL(tower_wgrad_reduce_kernel, dim3(kSlab / 256), dim3(256), 0, st, (const float*)D.ws, splits, d_dw);
    return dafne::check_launch("tower_wgrad_reduce");
}

}  // extern "C"
