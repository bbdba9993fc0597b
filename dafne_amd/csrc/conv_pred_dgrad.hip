// Data gradient of the head's prediction convolutions (cls_logits, corners_pred + ctrness, center_pred; dafne.py:318-344) carried
// back through the ReLU and the GroupNorm the forward applies on load (GN_INPUT), down to the RAW output of the tower's last
// convolution (gfx950).  Per prediction call, over up to five levels:
//
//     xhat = (x - mean) rstd                a = bf16(relu(fma(xhat, gamma, beta)))   (gn_apply_kernel's expression; 0 outside the image)
//     ga[y, x, ci] = sum over (co, kh, kw) of g[y - kh + 1, x - kw + 1, co] * Wb[co, ci, kh, kw]          (taps outside the image: 0)
//     gz = ga [a > 0]       dgamma[c] = sum gz xhat       dbeta[c] = sum gz
//     gxhat = gz gamma[c]   s1 = sum over the group of gxhat    s2 = sum over the group of gxhat xhat     (group: 8 channels x H x W = m)
//     gx = rstd (gxhat - s1 / m - xhat s2 / m)                  dbias[c] = sum gx
//
// The product is a GEMM  [256 input channels] x [K = 9 taps x 16 output channels, padded to 160] . [K] x [pixels]:
//   * v_mfma_f32_16x16x32_bf16 with the WEIGHTS as the A operand (exact bf16, 20 fragments per wave held in registers for the whole
//     launch: wave w owns input channels 64w .. 64w + 63) and g as the B operand, fp32 fed as a hi + lo bf16 pair (two MFMAs per
//     fragment: |g - hi - lo| <= 2^-16 |g|).  The result has the pixel on the lane and four consecutive channels in the registers:
//     x is read as 8 bytes and gx written as 16 bytes per lane, and a lane's four channels lie in one GroupNorm group;
//   * a workgroup (4 waves) walks tiles of 4 x 32 pixels over all levels; the tile's g with its one-pixel ring (6 x 34 pixels x 16
//     channels, zero outside the image and beyond Cout) is split into the hi and lo bf16 halves ONCE, while it is staged in LDS, and
//     shared by the four waves: a B fragment is one 16-byte LDS read, no conversion in the K loop;
//   * the raw map of a block of 16 pixels is loaded one block ahead, under the matrix work of the block before it;
//   * gx needs the group sums of the whole map, so the pixels are passed over twice.  CHOICE: the second pass RECOMPUTES ga.
//     Bytes per pixel: pass 1 reads 64 (g) + 512 (x); pass 2 reads 64 + 512 and writes 1024 (gx): 2176 B.  Storing gz in pass 1 and
//     reading it back would move 576 + 1024 (gz out), then 1024 (gz in) + 512 (x, for xhat) + 1024 (gx): 4160 B.  The recomputation
//     costs a second round of 320 MFMAs per 128-pixel tile and wave, which stays below the time of the bytes it saves
//     (measured times of both passes: profiles/NOTES_head_tail.md);
//   * no atomics: pass 1 writes s1 / s2 per TILE and dgamma / dbeta per WORKGROUP to the workspace, pred_dgrad_sums_kernel adds them
//     in a fixed order in fp64; pass 2 reads s1 / m, s2 / m from there and writes dbias per workgroup, reduced the same
//     way.  Which tiles a workgroup walks depends on the shapes and the CU count only: equal bits from run to run.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

constexpr int kMaxSegs = 5;                         // what dafne_conv2d_nhwc_bf16_hip takes
constexpr int kCin = 256, kMaxCout = 16, kGroups = kCin / 8;
constexpr int kTH = 4, kTW = 32;                    // tile of pixels: 8 blocks of 16 pixels (the N of an MFMA)
constexpr int kPC = kTW + 2;                        // ring columns
constexpr int kPR = (kTH + 2) * kPC;                // 204 ring pixels
constexpr int kGS = 40;                             // bf16 per staged pixel: 16 hi, 16 lo, 8 of padding (16-byte alignment, spreads the banks)
constexpr int kNT = 256;
constexpr int kWRow = kCin * 9;                     // packed weight row: [256/64 slabs][3][3][64]
constexpr int kPart = 3 * kCin;                     // floats of a workgroup's partial: dgamma, dbeta, dbias
constexpr int kTileSums = 2 * kGroups;              // floats of a tile's partial: (s1, s2) per group

struct DgSeg {
    const char* in;      // bf16 [N, H+2, W+2, 256], raw
    const float* g;      // fp32 [N, H, W, ps]
    float* gx;           // fp32 [N, H, W, 256]
    int H, W, tiles_x, tiles_per_img, tile0;
};

struct DgDev {
    DgSeg seg[kMaxSegs];
    int n_segs, N, Cout, ps, mtiles;
    const float* stats;          // [n_segs][N][32][2] mean, rstd
    const float* gamma;          // [256]
    const float* beta;           // [256]
    const unsigned short* w;     // bf16 [Cout_pad][4][3][3][64]
    float* part;                 // [workgroups][kPart]
    float* tsum;                 // [mtiles][kTileSums]
    float* gsum;                 // [n_segs][N][32][2]: s1 / m, s2 / m
};

// PASS 1: group sums per tile, dgamma / dbeta per workgroup.  PASS 2: gx, dbias per workgroup.
template <int PASS>
__global__ void __launch_bounds__(kNT, 2) pred_dgrad_kernel(DgDev P) {
    __shared__ __attribute__((aligned(16))) unsigned short gl[kPR * kGS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fcol = lane & 15, kg = lane >> 4;     // fragment row (A) / column (B), 8-element K group
    const int half = kg >> 1;                       // the tap of a k32 step this lane feeds: 2s + half; output channels 8 (kg & 1) ..
    const int c0 = wave * 64 + 4 * kg;              // + 16 cb + k: the channel of accumulator register k of block cb

    // ---- the weights of the whole launch: fragment (s, cb) = rows (input channels) 64 wave + 16 cb + fcol, K = (tap 2s + half,
    // output channels 8 (kg & 1) + j); tap 9 and the rows beyond Cout are zero
    bf16x8 wf[5][4];
#pragma unroll
    for (int s = 0; s < 5; s++) {
        const int tap = 2 * s + half, tapc = tap < 9 ? tap : 8;
#pragma unroll
        for (int cb = 0; cb < 4; cb++) {
            s16x8 v;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int co = 8 * (kg & 1) + j, coc = co < P.Cout ? co : P.Cout - 1;
                const unsigned short b = P.w[coc * kWRow + wave * 576 + tapc * 64 + cb * 16 + fcol];
                v[j] = (tap < 9 && co < P.Cout) ? (short)b : (short)0;
            }
            wf[s][cb] = __builtin_bit_cast(bf16x8, v);
        }
    }
    // ring offset of the pixel a k32 step reads: output pixel (ry, cx) of the tile and tap (kh, kw) -> ring pixel (ry - kh + 2, cx - kw + 2)
    int toff[5];
#pragma unroll
    for (int s = 0; s < 5; s++) {
        const int tap = 2 * s + half, tapc = tap < 9 ? tap : 8;
        const int kh = tapc / 3, kw = tapc - 3 * kh;
        toff[s] = ((2 - kh) * kPC + (2 - kw)) * kGS + 8 * (kg & 1);
    }
    // gamma and beta live in LDS (the registers go to the weights): [256] + [256]
    __shared__ __attribute__((aligned(16))) float gb[2 * kCin];
    gb[tid] = P.gamma[tid];
    gb[kCin + tid] = P.beta[tid];
    // per-workgroup sums: PASS 1 (dgamma, dbeta), PASS 2 (dbias, in wa)
    float wa[4][4], wb[4][4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
        for (int k = 0; k < 4; k++) wa[cb][k] = wb[cb][k] = 0.f;

    for (int t = (int)blockIdx.x; t < P.mtiles; t += (int)gridDim.x) {
        int si = 0;
#pragma unroll
        for (int k = 1; k < kMaxSegs; k++)
            if (k < P.n_segs && t >= P.seg[k].tile0) si = k;
        const DgSeg& S = P.seg[si];
        const int H = S.H, W = S.W, Wp = W + 2;
        const int tloc = t - S.tile0;
        const int img = tloc / S.tiles_per_img;
        const int tt = tloc - img * S.tiles_per_img;
        const int ty = tt / S.tiles_x;
        const int Y0 = ty * kTH, X0 = (tt - ty * S.tiles_x) * kTW;

        // ---- g of the tile and its ring -> LDS; pixels outside the image and channels beyond Cout are zero, the gap of a strided
        // buffer is never read (clamped address, value replaced)
        // (the loads of a batch first: two memory latencies per tile, not one per element)
        constexpr int kIt = (kPR * 16 + kNT - 1) / kNT, kBatch = (kIt + 1) / 2;
#pragma unroll
        for (int b = 0; b < kIt; b += kBatch) {
            float sv[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; k++) {
                const int i = tid + (b + k) * kNT;
                const int pix = (i >> 4) < kPR ? (i >> 4) : kPR - 1, co = i & 15;
                const int py = pix / kPC, px = pix - py * kPC;
                const int y = Y0 + py - 1, x = X0 + px - 1;
                const bool ok = y >= 0 && y < H && x >= 0 && x < W && co < P.Cout;
                const int yy = y < 0 ? 0 : (y < H ? y : H - 1), xx = x < 0 ? 0 : (x < W ? x : W - 1), cc = co < P.Cout ? co : P.Cout - 1;
                const float v = S.g[((size_t)(img * H + yy) * W + xx) * P.ps + cc];
                sv[k] = ok ? v : 0.f;
            }
#pragma unroll
            for (int k = 0; k < kBatch; k++) {
                const int i = tid + (b + k) * kNT;
                if (i < kPR * 16) {
                    const __bf16 h = (__bf16)sv[k];
                    gl[(i >> 4) * kGS + (i & 15)] = __builtin_bit_cast(unsigned short, h);
                    gl[(i >> 4) * kGS + 16 + (i & 15)] = __builtin_bit_cast(unsigned short, (__bf16)(sv[k] - (float)h));
                }
            }
        }
        __syncthreads();

        float mean[4], rstd[4], s1[4], s2[4];
        {
            const size_t sg = ((size_t)si * P.N + img) * kGroups + wave * 8 + half;
#pragma unroll
            for (int cb = 0; cb < 4; cb++) {
                mean[cb] = P.stats[(sg + 2 * cb) * 2];
                rstd[cb] = P.stats[(sg + 2 * cb) * 2 + 1];
                if (PASS == 2) {
                    s1[cb] = P.gsum[(sg + 2 * cb) * 2];
                    s2[cb] = P.gsum[(sg + 2 * cb) * 2 + 1];
                } else {
                    s1[cb] = s2[cb] = 0.f;
                }
            }
        }

        // the raw map of this lane's pixel of block pb: four channels of each of the four blocks (clamped address beyond the image)
        auto load_x = [&](int pb, u32x2* r) {
            const int y = Y0 + (pb >> 1), x = X0 + (pb & 1) * 16 + fcol;
            const int yy = y < H ? y : H - 1, xx = x < W ? x : W - 1;
            const char* xp = S.in + ((size_t)(img * (H + 2) + yy + 1) * Wp + xx + 1) * (kCin * 2) + c0 * 2;
#pragma unroll
            for (int cb = 0; cb < 4; cb++) r[cb] = *(const u32x2*)(xp + cb * 32);
        };
        u32x2 xr[4], xn[4];
        load_x(0, xr);
#pragma unroll 1
        for (int pb = 0; pb < 2 * kTH; pb++) {
            const int ry = pb >> 1, cx = (pb & 1) * 16 + fcol;
            const int y = Y0 + ry, x = X0 + cx;
            const bool valid = y < H && x < W;
            const int yy = y < H ? y : H - 1, xx = x < W ? x : W - 1;
            // one block ahead: its latency runs under this block's matrix work
            load_x(pb + 1 < 2 * kTH ? pb + 1 : pb, xn);

            f32x4 acc[4];
#pragma unroll
            for (int cb = 0; cb < 4; cb++) acc[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const unsigned short* gp = gl + (ry * kPC + cx) * kGS;
#pragma unroll
            for (int s = 0; s < 5; s++) {
                s16x8 fh = *(const s16x8*)(gp + toff[s]), fl = *(const s16x8*)(gp + toff[s] + 16);
                if (s == 4 && half) {                       // step 4 holds tap 8 and the padding tap
                    fh = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
                    fl = fh;
                }
                const bf16x8 bhi = __builtin_bit_cast(bf16x8, fh), blo = __builtin_bit_cast(bf16x8, fl);
#pragma unroll
                for (int cb = 0; cb < 4; cb++) {
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][cb], bhi, acc[cb], 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][cb], blo, acc[cb], 0, 0, 0);
                }
            }

            // ---- accumulator register k of block cb: (channel c0 + 16 cb + k, this lane's pixel)
            float* op = PASS == 2 ? S.gx + ((size_t)(img * H + yy) * W + xx) * kCin + c0 : nullptr;
#pragma unroll
            for (int cb = 0; cb < 4; cb++) {
                f32x4 o;
                const f32x4 gam = *(const f32x4*)(gb + c0 + 16 * cb), bet = *(const f32x4*)(gb + kCin + c0 + 16 * cb);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const unsigned u = k < 2 ? xr[cb].x : xr[cb].y;
                    const float xf = __uint_as_float((k & 1) ? (u & 0xffff0000u) : (u << 16));
                    // the expression of gn_apply_kernel: (x - mean) * rstd, one fused multiply-add with gamma and beta, bf16, ReLU
                    const float xh = (xf - mean[cb]) * rstd[cb];
                    const float a = (float)(__bf16)__builtin_fmaf(xh, gam[k], bet[k]);
                    const float gz = (valid && a > 0.f) ? acc[cb][k] : 0.f;
                    const float gxh = gz * gam[k];
                    if (PASS == 1) {
                        wa[cb][k] = __builtin_fmaf(gz, xh, wa[cb][k]);
                        wb[cb][k] += gz;
                        s1[cb] += gxh;
                        s2[cb] = __builtin_fmaf(gxh, xh, s2[cb]);
                    } else {
                        const float v = rstd[cb] * (gxh - s1[cb] - xh * s2[cb]);
                        o[k] = v;
                        wa[cb][k] += valid ? v : 0.f;
                    }
                }
                if (PASS == 2 && valid) *(f32x4*)(op + 16 * cb) = o;
            }
#pragma unroll
            for (int cb = 0; cb < 4; cb++) xr[cb] = xn[cb];
        }

        if (PASS == 1) {
            // the tile's group sums: the 32 lanes with this lane's `half` hold group wave * 8 + 2 cb + half
#pragma unroll
            for (int cb = 0; cb < 4; cb++) {
#pragma unroll
                for (int d = 1; d <= 16; d <<= 1) {
                    s1[cb] += __shfl_xor(s1[cb], d);
                    s2[cb] += __shfl_xor(s2[cb], d);
                }
                if ((lane & 31) == 0) {
                    float* o = P.tsum + (size_t)t * kTileSums + (wave * 8 + 2 * cb + half) * 2;
                    o[0] = s1[cb];
                    o[1] = s2[cb];
                }
            }
        }
        // the next tile's staging waits for these reads
        __syncthreads();
    }

    // ---- the workgroup's partial: sums over the 16 pixels lanes of a channel
    float* part = P.part + (size_t)blockIdx.x * kPart;
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float a = wa[cb][k], b = wb[cb][k];
#pragma unroll
            for (int d = 1; d <= 8; d <<= 1) {
                a += __shfl_xor(a, d);
                if (PASS == 1) b += __shfl_xor(b, d);
            }
            if (fcol == 0) {
                const int c = c0 + 16 * cb + k;
                if (PASS == 1) {
                    part[c] = a;
                    part[kCin + c] = b;
                } else {
                    part[2 * kCin + c] = a;
                }
            }
        }
}

// The reductions: one wave per element; lane j adds partials j, j + 64, ... in that order in fp64, then the 64 sums meet in a
// butterfly (lane distances 32, 16, .. 1: every lane ends with the same sum) -- a fixed tree: equal bits from run to run
__device__ __forceinline__ double ordered_sum64(const float* p, size_t stride, int n, int j) {
    double s = 0.0;
    for (int k = j; k < n; k += 64) s += (double)p[(size_t)k * stride];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

// after pass 1: gsum[(segment, image, group)] = (s1 / m, s2 / m) from the tiles of the image; dgamma / dbeta from the workgroups' partials
__global__ void __launch_bounds__(256) pred_dgrad_sums_kernel(DgDev P, int nparts, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int e = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), j = (int)threadIdx.x & 63;
    const int ng = P.n_segs * P.N * kTileSums;
    if (e < ng) {
        const int r = e % kTileSums, sidx = e / kTileSums;
        const int si = sidx / P.N, img = sidx - si * P.N;
        const DgSeg& S = P.seg[si];
        const float* p = P.tsum + ((size_t)S.tile0 + (size_t)img * S.tiles_per_img) * kTileSums + r;
        const double s = ordered_sum64(p, kTileSums, S.tiles_per_img, j);
        if (j == 0) P.gsum[e] = (float)(s / (8.0 * (double)S.H * (double)S.W));
    } else {
        const int c = e - ng;
        const double s = ordered_sum64(P.part + c, kPart, nparts, j);
        if (j == 0) {
            if (c < kCin) dgamma[c] = (float)s;
            else dbeta[c - kCin] = (float)s;
        }
    }
}

// after pass 2: dbias from the workgroups' partials
__global__ void __launch_bounds__(256) pred_dgrad_bias_kernel(const float* __restrict__ part, int nparts, float* __restrict__ dbias) {
    const int c = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), j = (int)threadIdx.x & 63;
    const double s = ordered_sum64(part + 2 * kCin + c, kPart, nparts, j);
    if (j == 0) dbias[c] = (float)s;
}

// -> DAFNE_OK with D filled (pointers of the gradients, the weight and the workspace excepted), or the refusal
int dg_build(DgDev& D, const dafne_conv_params* p, const dafne_conv_seg* segs, int ps) {
    if (!p || !segs) return dafne::fail(DAFNE_E_INVALID, "pred_dgrad_gn: null params");
    if (p->n_segs < 1 || p->n_segs > kMaxSegs || p->n_images < 1)
        return dafne::fail(DAFNE_E_INVALID, "pred_dgrad_gn: %d segments / %d images (1..%d segments)", p->n_segs, p->n_images, kMaxSegs);
    if (p->flags & ~(DAFNE_CONV_OUT_F32 | DAFNE_CONV_GN_INPUT | DAFNE_CONV_EXCLUSIVE))
        return dafne::fail(DAFNE_E_INVALID, "pred_dgrad_gn: flags 0x%x (a prediction call has OUT_F32, GN_INPUT, EXCLUSIVE)", p->flags);
    if (p->Cin != kCin) return dafne::fail(DAFNE_E_UNSUPPORTED, "pred_dgrad_gn: Cin %d, not 256", p->Cin);
    if (p->Cout < 1 || p->Cout > kMaxCout) return dafne::fail(DAFNE_E_UNSUPPORTED, "pred_dgrad_gn: Cout %d outside 1..16", p->Cout);
    if (p->KH != 3 || p->KW != 3 || p->stride != 1 || p->pad != 1) return dafne::fail(DAFNE_E_UNSUPPORTED, "pred_dgrad_gn: only 3x3 / stride 1 / pad 1");
    if (ps < p->Cout) return dafne::fail(DAFNE_E_INVALID, "pred_dgrad_gn: pixel stride %d below Cout %d", ps, p->Cout);
    if (!(p->flags & DAFNE_CONV_GN_INPUT))
        return dafne::fail(DAFNE_E_INVALID, "pred_dgrad_gn: the call does not normalise on load (GN_INPUT): the raw map and its statistics are the input");
    if (!p->d_in_gn_stats || !p->d_in_gn_gamma || !p->d_in_gn_beta)
        return dafne::fail(DAFNE_E_INVALID, "pred_dgrad_gn: GN_INPUT without statistics / affine pointers");
    long long t = 0;
    for (int s = 0; s < p->n_segs; s++) {
        const dafne_conv_seg& g = segs[s];
        if (!g.d_in || g.Hout < 1 || g.Wout < 1 || g.Hin != g.Hout || g.Win != g.Wout) return dafne::fail(DAFNE_E_INVALID, "pred_dgrad_gn: segment %d", s);
        // the limits of the forward call: 2^20 pixels per image, the haloed map of all images below 2^32 bytes
        if ((long long)g.Hout * g.Wout > (1 << 20) || g.Wout > (1 << 12))
            return dafne::fail(DAFNE_E_UNSUPPORTED, "pred_dgrad_gn: segment %d output %dx%d above 2^20 pixels per image", s, g.Hout, g.Wout);
        const long long in_bytes = (long long)p->n_images * (g.Hin + 2) * (g.Win + 2) * kCin * 2;
        if (in_bytes > 0xffffffffll)
            return dafne::fail(DAFNE_E_UNSUPPORTED, "pred_dgrad_gn: segment %d input of %lld bytes (%d images of %dx%dx%d) is beyond 32-bit offsets: "
                                                    "split the batch", s, in_bytes, p->n_images, g.Hin, g.Win, kCin);
        DgSeg& o = D.seg[s];
        o.in = (const char*)g.d_in;
        o.g = nullptr;
        o.gx = nullptr;
        o.H = g.Hout; o.W = g.Wout;
        o.tiles_x = (g.Wout + kTW - 1) / kTW;
        o.tiles_per_img = o.tiles_x * ((g.Hout + kTH - 1) / kTH);
        o.tile0 = (int)t;
        t += (long long)o.tiles_per_img * p->n_images;
        if (t > 0x7fffffffll / kTileSums) return dafne::fail(DAFNE_E_UNSUPPORTED, "pred_dgrad_gn: too many tiles");
    }
    D.n_segs = p->n_segs; D.N = p->n_images; D.Cout = p->Cout; D.ps = ps; D.mtiles = (int)t;
    D.stats = p->d_in_gn_stats; D.gamma = p->d_in_gn_gamma; D.beta = p->d_in_gn_beta;
    D.w = nullptr; D.part = nullptr; D.tsum = nullptr; D.gsum = nullptr;
    return DAFNE_OK;
}

// workgroups of a launch: two per CU, never more than tiles
int dg_grid(const DgDev& D, int* grid) {
    int cus = 0;
    if (int rc = dafne::device_cus(&cus)) return rc;
    *grid = D.mtiles < 2 * cus ? D.mtiles : 2 * cus;
    return DAFNE_OK;
}

// floats of the workspace: [workgroups][kPart], [tiles][kTileSums], [n_segs][N][kTileSums]
size_t dg_floats(const DgDev& D, int grid) { return (size_t)grid * kPart + (size_t)D.mtiles * kTileSums + (size_t)D.n_segs * D.N * kTileSums; }

}  // namespace

extern "C" {

size_t dafne_pred_dgrad_gn_workspace_bytes(const dafne_conv_params* prm, const dafne_conv_seg* segs) {
    DgDev D;
    if (dg_build(D, prm, segs, prm ? prm->Cout : 0)) return 0;
    int grid = 0;
    if (dg_grid(D, &grid)) return 0;
    return dg_floats(D, grid) * sizeof(float);
}

int dafne_pred_dgrad_gn_hip(const dafne_conv_params* prm, const dafne_conv_seg* segs, const void* d_weight, const float* const* d_gout,
                            int gout_ps, float* const* d_gx, float* d_dgamma, float* d_dbeta, float* d_dbias, void* d_ws, size_t ws_bytes,
                            void* stream) {
    DgDev D;
    if (int rc = dg_build(D, prm, segs, gout_ps)) return rc;
    if (!d_weight || !d_gout || !d_gx || !d_dgamma || !d_dbeta || !d_dbias || !d_ws) return dafne::fail(DAFNE_E_INVALID, "pred_dgrad_gn: null argument");
    for (int s = 0; s < D.n_segs; s++) {
        if (!d_gout[s] || !d_gx[s]) return dafne::fail(DAFNE_E_INVALID, "pred_dgrad_gn: null gradient of segment %d", s);
        D.seg[s].g = d_gout[s];
        D.seg[s].gx = d_gx[s];
    }
    int grid = 0;
    if (int rc = dg_grid(D, &grid)) return rc;
    const size_t need = dg_floats(D, grid) * sizeof(float);
    if (ws_bytes < need) return dafne::fail(DAFNE_E_WORKSPACE, "pred_dgrad_gn: workspace %zu < %zu", ws_bytes, need);
    D.w = (const unsigned short*)d_weight;
    D.part = (float*)d_ws;
    D.tsum = D.part + (size_t)grid * kPart;
    D.gsum = D.tsum + (size_t)D.mtiles * kTileSums;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pred_dgrad_kernel<1>, dim3(grid), dim3(kNT), 0, st, D);
    if (int rc = dafne::check_launch("pred_dgrad_gn pass 1")) return rc;
    const int total = D.n_segs * D.N * kTileSums + 2 * kCin;
    hipLaunchKernelGGL(pred_dgrad_sums_kernel, dim3(total / 4), dim3(256), 0, st, D, grid, d_dgamma, d_dbeta);
    if (int rc = dafne::check_launch("pred_dgrad_gn sums")) return rc;
    hipLaunchKernelGGL(pred_dgrad_kernel<2>, dim3(grid), dim3(kNT), 0, st, D);
    if (int rc = dafne::check_launch("pred_dgrad_gn pass 2")) return rc;
    hipLaunchKernelGGL(pred_dgrad_bias_kernel, dim3(kCin / 4), dim3(256), 0, st, (const float*)D.part, grid, d_dbias);
    return dafne::check_launch("pred_dgrad_gn bias");
}

}  // extern "C"
