// Data gradient of one tower convolution of the head (cls_tower / corners_tower .3 .6 .9; dafne.py:350-372) carried back through the
// ReLU and the GroupNorm the forward applies on load (GN_INPUT), down to the RAW output of the tower convolution before it
// (gfx950).  3x3 / stride 1 / pad 1, 256 -> 256 channels, over up to five levels.  The arithmetic is conv_pred_dgrad.hip's:
//
//     xhat = (x - mean) rstd                a = bf16(relu(fma(xhat, gamma, beta)))   (gn_apply_kernel's expression; 0 outside the image)
//     ga[y, x, ci] = sum over (co, kh, kw) of g[y - kh + 1, x - kw + 1, co] * Wb[co, ci, kh, kw]          (taps outside the image: 0)
//     gz = ga [a > 0]       dgamma[c] = sum gz xhat       dbeta[c] = sum gz
//     gxhat = gz gamma[c]   s1 = sum over the group of gxhat    s2 = sum over the group of gxhat xhat     (group: 8 channels x H x W = m)
//     gx = rstd (gxhat - s1 / m - xhat s2 / m)                  dbias[c] = sum gx
//
// The product is a GEMM  [256 input channels] x [K = 9 taps x 256 output channels = 2304] . [K] x [pixels]:
//   * v_mfma_f32_16x16x32_bf16 with the WEIGHTS as the A operand (exact bf16) and g as the B operand, fp32 fed as a hi + lo bf16
//     pair (two MFMAs per fragment: |g - hi - lo| <= 2^-16 |g|).  The result has the pixel on the lane and four consecutive
//     channels in the registers, and a lane's four channels lie in one GroupNorm group;
//   * a workgroup (4 waves) walks tiles of 4 x 32 pixels over all levels; wave w owns input channels 64w .. 64w + 63 of all 128
//     pixels: 8 pixel blocks x 4 channel blocks of 16 x 16 = 128 accumulator registers, alive over the whole K loop;
//   * K is walked as 4 chunks of 64 output channels x 9 taps.  Per chunk, the tile's g with its one-pixel ring (6 x 34 pixels x 64
//     channels, zero outside the image) is split into the hi and lo bf16 halves ONCE while it is staged in LDS (272 B per pixel:
//     128 hi, 128 lo, 16 of padding that spreads the banks), shared by the four waves and by the nine taps;
//   * the weights (1.2 MB) do not fit in registers: slice (chunk, tap) = [256 input channels][64 output channels] bf16, 32 KB,
//     streams through a double buffer in LDS (rows of 144 B: 128 + 16 of padding).  The slice behind the one being multiplied is
//     requested from global memory before the matrix work and written to the other buffer after it: one barrier per slice.  That
//     layout, [chunk][tap][ci][co in chunk], is the transpose of engine.pack_conv's [co][ci / 64][tap][ci % 64]; tower_dgrad_
//     transpose_kernel builds it in the workspace from the packed bf16 weight the forward multiplied;
//   * LDS: 55 488 (g ring) + 2 x 36 864 (weights) = 129 216 B, one workgroup per CU;
//   * gx needs the group sums of the whole map, so the pixels are passed over twice.  CHOICE: pass 1 STORES gz (fp32, in the gx
//     buffer itself); recomputing ga in the second pass, what conv_pred_dgrad.hip does at K = 160, would cost 2.4 MFLOP per pixel
//     here against 2 KB.  Pass 2 (tower_dgrad_apply_kernel) is elementwise and in place: gz and x in, gx out, dbias partials;
//   * no atomics: pass 1 writes s1 / s2 per TILE and dgamma / dbeta per WORKGROUP to the workspace, tower_dgrad_sums_kernel adds them
//     in a fixed order in fp64; pass 2 reads s1 / m, s2 / m from there and writes dbias per workgroup, reduced the same
//     way.  Which tiles / pixels a workgroup walks depends on the shapes and the CU count only: equal bits from run to run.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int kMaxSegs = 5;                         // what dafne_conv2d_nhwc_bf16_hip takes
constexpr int kC = 256, kGroups = kC / 8;           // Cin = Cout
constexpr int kTH = 4, kTW = 32;                    // tile of pixels: 8 blocks of 16 pixels (the N of an MFMA)
constexpr int kPB = 2 * kTH;                        // pixel blocks of a tile
constexpr int kPC = kTW + 2;                        // ring columns
constexpr int kPR = (kTH + 2) * kPC;                // 204 ring pixels
constexpr int kCh = 64, kChunks = kC / kCh;         // output channels per K chunk
constexpr int kGS = 272;                            // bytes per staged ring pixel: 64 hi, 64 lo bf16, 16 of padding
constexpr int kWS = 144;                            // bytes per staged weight row: 64 bf16, 16 of padding
constexpr int kRing = kPR * kGS;                    // 55 488 B
constexpr int kWBuf = kC * kWS;                     // 36 864 B
constexpr int kSmem = kRing + 2 * kWBuf;            // 129 216 B
constexpr int kSlices = kChunks * 9;                // 36 weight slices of 32 KB
constexpr int kSliceElems = kC * kCh;               // bf16 elements of a slice
constexpr int kNT = 256;
constexpr int kWRow = kC * 9;                       // packed weight row: [256/64 slabs][3][3][64]
constexpr int kPart = 2 * kC;                       // floats of a pass-1 workgroup's partial: dgamma, dbeta
constexpr int kTileSums = 2 * kGroups;              // floats of a tile's partial: (s1, s2) per group
constexpr int kApplyPx = 4;                         // pixels a pass-2 workgroup takes per step (64 lanes x 4 channels each)
constexpr int kAllowed = DAFNE_CONV_GN_STATS | DAFNE_CONV_GN_INPUT | DAFNE_CONV_GN_FINALIZE | DAFNE_CONV_EXCLUSIVE | DAFNE_CONV_FRAG16;
static_assert(kSmem <= 160 * 1024, "LDS budget");

struct TdSeg {
    const char* in;      // bf16 [N, H+2, W+2, 256], raw
    const float* g;      // fp32 [N, H, W, 256]
    float* gx;           // fp32 [N, H, W, 256]: gz after pass 1, gx after pass 2
    int H, W, tiles_x, tiles_per_img, tile0;
};

struct TdDev {
    TdSeg seg[kMaxSegs];
    int n_segs, N, mtiles;
    const float* stats;          // [n_segs][N][32][2] mean, rstd
    const float* gamma;          // [256]
    const float* beta;           // [256]
    const unsigned short* w;     // bf16 [256][4][3][3][64]: engine.pack_conv
    unsigned short* wt;          // bf16 [4 chunks][9 taps][256 ci][64 co]
    float* part;                 // [pass-1 workgroups][kPart]
    float* tsum;                 // [mtiles][kTileSums]
    float* gsum;                 // [n_segs][N][32][2]: s1 / m, s2 / m
    float* part2;                // [pass-2 workgroups][256]: dbias
};

// wt[chunk][tap][ci][col] = w[co = 64 chunk + col][ci / 64][tap][ci % 64]; one thread per element
__global__ void __launch_bounds__(256) tower_dgrad_transpose_kernel(const unsigned short* __restrict__ w, unsigned short* __restrict__ wt) {
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= kSlices * kSliceElems) return;
    const int col = e & (kCh - 1), ci = (e >> 6) & (kC - 1), st = e >> 14;
    const int chunk = st / 9, tap = st - 9 * chunk;
    wt[e] = w[(chunk * kCh + col) * kWRow + (ci >> 6) * 576 + tap * 64 + (ci & 63)];
}

// PASS 1: gz into the gx buffer, group sums per tile, dgamma / dbeta per workgroup
__global__ void __launch_bounds__(kNT) tower_dgrad_kernel(TdDev P) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* ring = lds;
    char* wbuf = lds + kRing;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fcol = lane & 15, kg = lane >> 4;     // fragment row (A) / column (B), 8-element K group
    const int half = kg >> 1;                       // the GroupNorm group of this lane's channels of block cb: 8 wave + 2 cb + half
    const int c0 = wave * 64 + 4 * kg;              // + 16 cb + k: the channel of accumulator register k of block cb

    // per-workgroup sums over the tiles: dgamma, dbeta
    float wa[4][4], wb[4][4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
        for (int k = 0; k < 4; k++) wa[cb][k] = wb[cb][k] = 0.f;

    // weight slice sl: global -> registers (8 chunks of 16 B per thread, consecutive threads consecutive chunks) -> LDS buffer
    auto slice_load = [&](int sl, u32x4* r) {
        const u32x4* src = (const u32x4*)(P.wt + (size_t)sl * kSliceElems);
#pragma unroll
        for (int k = 0; k < 8; k++) r[k] = src[tid + k * kNT];
    };
    auto slice_store = [&](int buf, const u32x4* r) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int i = tid + k * kNT;
            *(u32x4*)(wbuf + buf * kWBuf + (i >> 3) * kWS + (i & 7) * 16) = r[k];
        }
    };

    for (int t = (int)blockIdx.x; t < P.mtiles; t += (int)gridDim.x) {
        int si = 0;
#pragma unroll
        for (int k = 1; k < kMaxSegs; k++)
            if (k < P.n_segs && t >= P.seg[k].tile0) si = k;
        const TdSeg& S = P.seg[si];
        const int H = S.H, W = S.W, Wp = W + 2;
        const int tloc = t - S.tile0;
        const int img = tloc / S.tiles_per_img;
        const int tt = tloc - img * S.tiles_per_img;
        const int ty = tt / S.tiles_x;
        const int Y0 = ty * kTH, X0 = (tt - ty * S.tiles_x) * kTW;

        f32x4 acc[kPB][4];
#pragma unroll
        for (int pb = 0; pb < kPB; pb++)
#pragma unroll
            for (int cb = 0; cb < 4; cb++) acc[pb][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};

        // the tile before this one has been read to the end (its last slice sits in buffer 1, the ring is its last chunk's)
        __syncthreads();
        {
            u32x4 r[8];
            slice_load(0, r);
            slice_store(0, r);
        }
#pragma unroll 1
        for (int it = 0; it < kSlices; it++) {
            const int chunk = it / 9, tap = it - 9 * chunk;
            if (tap == 0) {
                // ---- chunk `chunk` of g of the tile and its ring -> LDS as hi / lo; pixels outside the image are zero (clamped
                // address, value replaced).  The chunk before it has been read by every wave: the barrier that ended slice it - 1
                constexpr int kIt = (kPR * 16 + kNT - 1) / kNT, kBatch = (kIt + 1) / 2;        // 13 float4 per thread, two batches
#pragma unroll
                for (int b = 0; b < kIt; b += kBatch) {
                    f32x4 sv[kBatch];
#pragma unroll
                    for (int k = 0; k < kBatch; k++) {
                        const int i = tid + (b + k) * kNT;
                        const int pix = (i >> 4) < kPR ? (i >> 4) : kPR - 1, c4 = i & 15;
                        const int py = pix / kPC, px = pix - py * kPC;
                        const int y = Y0 + py - 1, x = X0 + px - 1;
                        const bool ok = y >= 0 && y < H && x >= 0 && x < W;
                        const int yy = y < 0 ? 0 : (y < H ? y : H - 1), xx = x < 0 ? 0 : (x < W ? x : W - 1);
                        const f32x4 v = *(const f32x4*)(S.g + ((size_t)(img * H + yy) * W + xx) * kC + chunk * kCh + 4 * c4);
                        sv[k] = ok ? v : (f32x4){0.f, 0.f, 0.f, 0.f};
                    }
#pragma unroll
                    for (int k = 0; k < kBatch; k++) {
                        const int i = tid + (b + k) * kNT;
                        if (b + k < kIt && i < kPR * 16) {
                            unsigned short hi[4], lo[4];
#pragma unroll
                            for (int j = 0; j < 4; j++) {
                                const __bf16 h = (__bf16)sv[k][j];
                                hi[j] = __builtin_bit_cast(unsigned short, h);
                                lo[j] = __builtin_bit_cast(unsigned short, (__bf16)(sv[k][j] - (float)h));
                            }
                            char* dst = ring + (i >> 4) * kGS + (i & 15) * 8;
                            *(u32x2*)dst = (u32x2){(unsigned)hi[0] | ((unsigned)hi[1] << 16), (unsigned)hi[2] | ((unsigned)hi[3] << 16)};
                            *(u32x2*)(dst + 128) = (u32x2){(unsigned)lo[0] | ((unsigned)lo[1] << 16), (unsigned)lo[2] | ((unsigned)lo[3] << 16)};
                        }
                    }
                }
            }
            // the ring and buffer it & 1 are complete; every wave is done with buffer (it + 1) & 1 (slice it - 1)
            __syncthreads();
            u32x4 nx[8];
            if (it + 1 < kSlices) slice_load(it + 1, nx);

            // output pixel (ry, cx) of the tile and tap (kh, kw) -> ring pixel (ry - kh + 2, cx - kw + 2)
            const int kh = tap / 3, kw = tap - 3 * kh;
            const char* gp0 = ring + ((2 - kh) * kPC + (2 - kw) + fcol) * kGS + kg * 16;
            const char* wp0 = wbuf + (it & 1) * kWBuf + (wave * 64 + fcol) * kWS + kg * 16;
#pragma unroll
            for (int s = 0; s < 2; s++) {
                // A fragment (s, cb): rows (input channels) 64 wave + 16 cb + fcol, K = output channels 64 chunk + 32 s + 8 kg + j
                bf16x8 wf[4];
#pragma unroll
                for (int cb = 0; cb < 4; cb++) wf[cb] = __builtin_bit_cast(bf16x8, *(const s16x8*)(wp0 + cb * 16 * kWS + s * 64));
#pragma unroll
                for (int pb = 0; pb < kPB; pb++) {
                    const char* gp = gp0 + ((pb >> 1) * kPC + (pb & 1) * 16) * kGS + s * 64;
                    const bf16x8 bhi = __builtin_bit_cast(bf16x8, *(const s16x8*)gp);
                    const bf16x8 blo = __builtin_bit_cast(bf16x8, *(const s16x8*)(gp + 128));
#pragma unroll
                    for (int cb = 0; cb < 4; cb++) {
                        acc[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[cb], bhi, acc[pb][cb], 0, 0, 0);
                        acc[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[cb], blo, acc[pb][cb], 0, 0, 0);
                    }
                }
            }
            if (it + 1 < kSlices) slice_store((it + 1) & 1, nx);
            // a new chunk's ring is written at the top of the next slice: behind every wave's reads of this one
            if (tap == 8) __syncthreads();
        }

        // ---- accumulator register k of block (pb, cb): (channel c0 + 16 cb + k, pixel fcol of block pb)
        float mean[4], rstd[4], s1[4], s2[4];
        {
            const size_t sg = ((size_t)si * P.N + img) * kGroups + wave * 8 + half;
#pragma unroll
            for (int cb = 0; cb < 4; cb++) {
                mean[cb] = P.stats[(sg + 2 * cb) * 2];
                rstd[cb] = P.stats[(sg + 2 * cb) * 2 + 1];
                s1[cb] = s2[cb] = 0.f;
            }
        }
        f32x4 gam[4], bet[4];
#pragma unroll
        for (int cb = 0; cb < 4; cb++) {
            gam[cb] = *(const f32x4*)(P.gamma + c0 + 16 * cb);
            bet[cb] = *(const f32x4*)(P.beta + c0 + 16 * cb);
        }
#pragma unroll
        for (int pb = 0; pb < kPB; pb++) {
            const int y = Y0 + (pb >> 1), x = X0 + (pb & 1) * 16 + fcol;
            const bool valid = y < H && x < W;
            const int yy = y < H ? y : H - 1, xx = x < W ? x : W - 1;
            // the raw map of this lane's pixel: four channels of each of the four blocks (clamped address beyond the image)
            const char* xp = S.in + ((size_t)(img * (H + 2) + yy + 1) * Wp + xx + 1) * (kC * 2) + c0 * 2;
            u32x2 xr[4];
#pragma unroll
            for (int cb = 0; cb < 4; cb++) xr[cb] = *(const u32x2*)(xp + cb * 32);
            float* op = S.gx + ((size_t)(img * H + yy) * W + xx) * kC + c0;
#pragma unroll
            for (int cb = 0; cb < 4; cb++) {
                f32x4 o;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const unsigned u = k < 2 ? xr[cb].x : xr[cb].y;
                    const float xf = __uint_as_float((k & 1) ? (u & 0xffff0000u) : (u << 16));
                    // the expression of gn_apply_kernel: (x - mean) * rstd, one fused multiply-add with gamma and beta, bf16, ReLU
                    const float xh = (xf - mean[cb]) * rstd[cb];
                    const float a = (float)(__bf16)__builtin_fmaf(xh, gam[cb][k], bet[cb][k]);
                    const float gz = (valid && a > 0.f) ? acc[pb][cb][k] : 0.f;
                    const float gxh = gz * gam[cb][k];
                    o[k] = gz;
                    wa[cb][k] = __builtin_fmaf(gz, xh, wa[cb][k]);
                    wb[cb][k] += gz;
                    s1[cb] += gxh;
                    s2[cb] = __builtin_fmaf(gxh, xh, s2[cb]);
                }
                if (valid) *(f32x4*)(op + 16 * cb) = o;
            }
        }
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

    // ---- the workgroup's partial: sums over the 16 pixel lanes of a channel
    float* part = P.part + (size_t)blockIdx.x * kPart;
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float a = wa[cb][k], b = wb[cb][k];
#pragma unroll
            for (int d = 1; d <= 8; d <<= 1) {
                a += __shfl_xor(a, d);
                b += __shfl_xor(b, d);
            }
            if (fcol == 0) {
                const int c = c0 + 16 * cb + k;
                part[c] = a;
                part[kC + c] = b;
            }
        }
}

// PASS 2, elementwise and in place: gx = rstd (gz gamma - s1 / m - xhat s2 / m); dbias per workgroup.  Thread = (channels 4 cq ..
// 4 cq + 3, pixel lane pl of 4); a workgroup walks pixels 4 b + pl, 4 (b + workgroups) + pl, ... of every level in turn
__global__ void __launch_bounds__(kNT) tower_dgrad_apply_kernel(TdDev P) {
    __shared__ float red[kApplyPx][kC];
    const int tid = threadIdx.x;
    const int cq = tid & 63, pl = tid >> 6;
    const f32x4 gam = *(const f32x4*)(P.gamma + 4 * cq);
    float db[4] = {0.f, 0.f, 0.f, 0.f};
    for (int si = 0; si < P.n_segs; si++) {
        const TdSeg& S = P.seg[si];
        const int H = S.H, W = S.W, HW = H * W, npx = P.N * HW;
        for (int p = (int)blockIdx.x * kApplyPx + pl; p < npx; p += (int)gridDim.x * kApplyPx) {
            const int img = p / HW, rem = p - img * HW;
            const int y = rem / W, x = rem - y * W;
            const size_t sg = (((size_t)si * P.N + img) * kGroups + (cq >> 1)) * 2;
            const float mean = P.stats[sg], rstd = P.stats[sg + 1];
            const float s1 = P.gsum[sg], s2 = P.gsum[sg + 1];
            const u32x2 xr = *(const u32x2*)(S.in + ((size_t)(img * (H + 2) + y + 1) * (W + 2) + x + 1) * (kC * 2) + cq * 8);
            float* gp = S.gx + (size_t)p * kC + 4 * cq;
            const f32x4 gz = *(const f32x4*)gp;
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned u = k < 2 ? xr.x : xr.y;
                const float xf = __uint_as_float((k & 1) ? (u & 0xffff0000u) : (u << 16));
                const float xh = (xf - mean) * rstd;
                const float gxh = gz[k] * gam[k];
                const float v = rstd * (gxh - s1 - xh * s2);
                o[k] = v;
                db[k] += v;
            }
            *(f32x4*)gp = o;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) red[pl][4 * cq + k] = db[k];
    __syncthreads();
    P.part2[(size_t)blockIdx.x * kC + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
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
__global__ void __launch_bounds__(256) tower_dgrad_sums_kernel(TdDev P, int nparts, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int e = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), j = (int)threadIdx.x & 63;
    const int ng = P.n_segs * P.N * kTileSums;
    if (e < ng) {
        const int r = e % kTileSums, sidx = e / kTileSums;
        const int si = sidx / P.N, img = sidx - si * P.N;
        const TdSeg& S = P.seg[si];
        const float* p = P.tsum + ((size_t)S.tile0 + (size_t)img * S.tiles_per_img) * kTileSums + r;
        const double s = ordered_sum64(p, kTileSums, S.tiles_per_img, j);
        if (j == 0) P.gsum[e] = (float)(s / (8.0 * (double)S.H * (double)S.W));
    } else {
        const int c = e - ng;
        const double s = ordered_sum64(P.part + c, kPart, nparts, j);
        if (j == 0) {
            if (c < kC) dgamma[c] = (float)s;
            else dbeta[c - kC] = (float)s;
        }
    }
}

// after pass 2: dbias from the workgroups' partials
__global__ void __launch_bounds__(256) tower_dgrad_bias_kernel(const float* __restrict__ part2, int nparts, float* __restrict__ dbias) {
    const int c = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), j = (int)threadIdx.x & 63;
    const double s = ordered_sum64(part2 + c, kC, nparts, j);
    if (j == 0) dbias[c] = (float)s;
}

// -> DAFNE_OK with D filled (pointers of the gradients, the weight and the workspace excepted), or the refusal
int td_build(TdDev& D, const dafne_conv_params* p, const dafne_conv_seg* segs, long long* pixels) {
    if (!p || !segs) return dafne::fail(DAFNE_E_INVALID, "tower_dgrad_gn: null params");
    if (p->n_segs < 1 || p->n_segs > kMaxSegs || p->n_images < 1)
        return dafne::fail(DAFNE_E_INVALID, "tower_dgrad_gn: %d segments / %d images (1..%d segments)", p->n_segs, p->n_images, kMaxSegs);
    if (p->flags & ~(unsigned)kAllowed)
        return dafne::fail(DAFNE_E_INVALID, "tower_dgrad_gn: flags 0x%x (a tower call has GN_STATS, GN_INPUT, GN_FINALIZE, EXCLUSIVE, FRAG16)", p->flags);
    if (p->Cin != kC || p->Cout != kC) return dafne::fail(DAFNE_E_UNSUPPORTED, "tower_dgrad_gn: %d -> %d channels, not 256 -> 256", p->Cin, p->Cout);
    if (p->KH != 3 || p->KW != 3 || p->stride != 1 || p->pad != 1) return dafne::fail(DAFNE_E_UNSUPPORTED, "tower_dgrad_gn: only 3x3 / stride 1 / pad 1");
    if (!(p->flags & DAFNE_CONV_GN_INPUT))
        return dafne::fail(DAFNE_E_INVALID, "tower_dgrad_gn: the call does not normalise on load (GN_INPUT): the raw map and its statistics are the input");
    if (!p->d_in_gn_stats || !p->d_in_gn_gamma || !p->d_in_gn_beta)
        return dafne::fail(DAFNE_E_INVALID, "tower_dgrad_gn: GN_INPUT without statistics / affine pointers");
    long long t = 0, px = 0;
    for (int s = 0; s < p->n_segs; s++) {
        const dafne_conv_seg& g = segs[s];
        if (!g.d_in || g.Hout < 1 || g.Wout < 1 || g.Hin != g.Hout || g.Win != g.Wout) return dafne::fail(DAFNE_E_INVALID, "tower_dgrad_gn: segment %d", s);
        // the limits of the forward call: 2^20 pixels per image, the haloed map of all images below 2^32 bytes
        if ((long long)g.Hout * g.Wout > (1 << 20) || g.Wout > (1 << 12))
            return dafne::fail(DAFNE_E_UNSUPPORTED, "tower_dgrad_gn: segment %d output %dx%d above 2^20 pixels per image", s, g.Hout, g.Wout);
        const long long in_bytes = (long long)p->n_images * (g.Hin + 2) * (g.Win + 2) * kC * 2;
        if (in_bytes > 0xffffffffll)
            return dafne::fail(DAFNE_E_UNSUPPORTED, "tower_dgrad_gn: segment %d input of %lld bytes (%d images of %dx%dx%d) is beyond 32-bit offsets: "
                                                    "split the batch", s, in_bytes, p->n_images, g.Hin, g.Win, kC);
        TdSeg& o = D.seg[s];
        o.in = (const char*)g.d_in;
        o.g = nullptr;
        o.gx = nullptr;
        o.H = g.Hout; o.W = g.Wout;
        o.tiles_x = (g.Wout + kTW - 1) / kTW;
        o.tiles_per_img = o.tiles_x * ((g.Hout + kTH - 1) / kTH);
        o.tile0 = (int)t;
        t += (long long)o.tiles_per_img * p->n_images;
        px += (long long)p->n_images * g.Hout * g.Wout;
        if (t > 0x7fffffffll / kTileSums) return dafne::fail(DAFNE_E_UNSUPPORTED, "tower_dgrad_gn: too many tiles");
    }
    D.n_segs = p->n_segs; D.N = p->n_images; D.mtiles = (int)t;
    D.stats = p->d_in_gn_stats; D.gamma = p->d_in_gn_gamma; D.beta = p->d_in_gn_beta;
    D.w = nullptr; D.wt = nullptr; D.part = nullptr; D.tsum = nullptr; D.gsum = nullptr; D.part2 = nullptr;
    *pixels = px;
    return DAFNE_OK;
}

// workgroups of pass 1: one per CU (the LDS of one), never more than tiles; of pass 2: eight per CU, never more than steps
int td_grids(const TdDev& D, long long pixels, int* grid1, int* grid2) {
    int cus = 0;
    if (int rc = dafne::device_cus(&cus)) return rc;
    *grid1 = D.mtiles < cus ? D.mtiles : cus;
    const long long steps = (pixels + kApplyPx - 1) / kApplyPx;
    *grid2 = (int)(steps < 8ll * cus ? steps : 8ll * cus);
    return DAFNE_OK;
}

// floats of the workspace: the transposed weight (bf16, two per float), [grid1][kPart], [tiles][kTileSums], [n_segs][N][kTileSums], [grid2][256]
constexpr size_t kWtFloats = (size_t)kSlices * kSliceElems / 2;
size_t td_floats(const TdDev& D, int grid1, int grid2) {
    return kWtFloats + (size_t)grid1 * kPart + (size_t)D.mtiles * kTileSums + (size_t)D.n_segs * D.N * kTileSums + (size_t)grid2 * kC;
}

}  // namespace

extern "C" {

size_t dafne_tower_dgrad_gn_workspace_bytes(const dafne_conv_params* prm, const dafne_conv_seg* segs) {
    TdDev D;
    long long px = 0;
    if (td_build(D, prm, segs, &px)) return 0;
    int g1 = 0, g2 = 0;
    if (td_grids(D, px, &g1, &g2)) return 0;
    return td_floats(D, g1, g2) * sizeof(float);
}

int dafne_tower_dgrad_gn_hip(const dafne_conv_params* prm, const dafne_conv_seg* segs, const void* d_weight, const float* const* d_gout,
                             float* const* d_gx, float* d_dgamma, float* d_dbeta, float* d_dbias, void* d_ws, size_t ws_bytes, void* stream) {
    TdDev D;
    long long px = 0;
    if (int rc = td_build(D, prm, segs, &px)) return rc;
    if (!d_weight || !d_gout || !d_gx || !d_dgamma || !d_dbeta || !d_dbias || !d_ws) return dafne::fail(DAFNE_E_INVALID, "tower_dgrad_gn: null argument");
    if ((size_t)d_ws & 15) return dafne::fail(DAFNE_E_INVALID, "tower_dgrad_gn: workspace not aligned to 16 bytes");
    for (int s = 0; s < D.n_segs; s++) {
        if (!d_gout[s] || !d_gx[s]) return dafne::fail(DAFNE_E_INVALID, "tower_dgrad_gn: null gradient of segment %d", s);
        if (((size_t)d_gout[s] | (size_t)d_gx[s]) & 15)
            return dafne::fail(DAFNE_E_INVALID, "tower_dgrad_gn: gradient of segment %d not aligned to 16 bytes", s);
        D.seg[s].g = d_gout[s];
        D.seg[s].gx = d_gx[s];
    }
    int g1 = 0, g2 = 0;
    if (int rc = td_grids(D, px, &g1, &g2)) return rc;
    const size_t need = td_floats(D, g1, g2) * sizeof(float);
    if (ws_bytes < need) return dafne::fail(DAFNE_E_WORKSPACE, "tower_dgrad_gn: workspace %zu < %zu", ws_bytes, need);
    D.w = (const unsigned short*)d_weight;
    D.wt = (unsigned short*)d_ws;
    D.part = (float*)d_ws + kWtFloats;
    D.tsum = D.part + (size_t)g1 * kPart;
    D.gsum = D.tsum + (size_t)D.mtiles * kTileSums;
    D.part2 = D.gsum + (size_t)D.n_segs * D.N * kTileSums;
    hipStream_t st = (hipStream_t)stream;
    DAFNE_MAX_LDS_ONCE(kSmem, (const void*)tower_dgrad_kernel);
    hipLaunchKernelGGL(tower_dgrad_transpose_kernel, dim3(kSlices * kSliceElems / 256), dim3(256), 0, st, D.w, D.wt);
    if (int rc = dafne::check_launch("tower_dgrad_gn transpose")) return rc;
    hipLaunchKernelGGL(tower_dgrad_kernel, dim3(g1), dim3(kNT), kSmem, st, D);
    if (int rc = dafne::check_launch("tower_dgrad_gn pass 1")) return rc;
    const int total = D.n_segs * D.N * kTileSums + 2 * kC;
    hipLaunchKernelGGL(tower_dgrad_sums_kernel, dim3(total / 4), dim3(256), 0, st, D, g1, d_dgamma, d_dbeta);
    if (int rc = dafne::check_launch("tower_dgrad_gn sums")) return rc;
    hipLaunchKernelGGL(tower_dgrad_apply_kernel, dim3(g2), dim3(kNT), 0, st, D);
    if (int rc = dafne::check_launch("tower_dgrad_gn pass 2")) return rc;
    hipLaunchKernelGGL(tower_dgrad_bias_kernel, dim3(kC / 4), dim3(256), 0, st, (const float*)D.part2, g2, d_dbias);
    return dafne::check_launch("tower_dgrad_gn bias");
}

}  // extern "C"
