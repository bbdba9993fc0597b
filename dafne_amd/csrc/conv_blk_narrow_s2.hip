// The LAST res2 bottleneck body evaluated only where res3 reads it (gfx950).  ResNet-50/101 put a stage's stride in the first
// 1x1 of its block 0 (STRIDE_IN_1X1): res3.0.conv1 and res3.0.shortcut are 1x1, stride 2, pad 0 and touch only the pixels
// (2i, 2j) of the res2 output, and nothing else reads that map (the FPN starts at res3).  So for i < Ho = (H+1)/2, j < Wo = (W+1)/2
//
//     T(i,j) = relu(conv2(U)(2i,2j) + bias2)              3x3, 64 -> 64, pad 1, at the even pixels only (= stride 2)
//     Y(i,j) = relu(conv3(T)(i,j) + bias3 + X(2i,2j))     1x1, 64 -> 256, identity shortcut
//
// and Y is the COMPACT map [N, Ho+2, Wo+2, 256] that the two res3.0 layers then read with stride 1.  Against
// conv_blk_narrow_kernel<false,false> on the full map: a quarter of the X rows read, of the Y rows written and of the 3x3 / 1x1
// work; every pixel of U is still a tap of some even output pixel.
//
// Structure: conv_blk_narrow.hip's (persistent workgroups, one per CU, 8 waves; conv2's weights resident in LDS in fragment
// order, conv3's in registers; loads of tile k+1 issued during tile k and awaited at its top with a COUNTED vmcnt that never
// waits for a store) on tiles of 2 x 32 OUTPUT pixels:
//   * the (2*2+1) x (2*32+1) x 64-channel input patch (325 px, 41 DMA pieces of 8 px x 128 B) goes to LDS with the 16-byte
//     chunk XOR keyed on the patch column q, ((q >> 1) & 7): lane `frow` reads column 2*frow + kw, so eight consecutive lanes
//     hit eight different chunk slots at every tap; single-buffered, re-requested the moment phase A is done with it;
//   * phase A (waves 0-3: 32 channels x one tile row each) = 36 k16 steps of (A fragment from LDS, B fragment from the patch,
//     one MFMA), exactly the sibling's K order (tap-major, k16 ascending);
//   * 64 pixels x 256 channels of Y fit the sibling's 32-KB buffer at once: the shortcut rows (even pixels only, 512
//     contiguous bytes each) are parked there, every wave runs conv3 for two 32-channel groups x one 32-pixel fragment and
//     applies (acc + bias3) + X -> ReLU -> bf16 in place, then the rows go to HBM -- no halves, three barriers fewer per tile;
//   * LDS: weights 72 + patch 41 + T 8 + Y 32 + constants 4 = 157 KB;
//   * ragged tiles: loads are clamped into the tensor, rows of out-of-image pixels are STORED to a dump area (never
//     predicated: the vmcnt bookkeeping needs an exact instruction count).
// An MFMA output element does not depend on which other pixels share its fragment, and the K orders and epilogue expressions
// are the sibling's: Y(i,j) is bit-identical to pixel (2i,2j) of what dafne_bottleneck_block_narrow_hip writes.
#include <stdlib.h>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((address_space(1))) void gvoid;
typedef __attribute__((address_space(3))) void lvoid;

constexpr int kTH = 2, kTW = 32, kPx = kTH * kTW;    // output pixels of a tile
constexpr int kPC = 2 * kTW + 1, kPR = 2 * kTH + 1;  // input patch: 5 x 65 pixels
constexpr int kPPieces = (kPR * kPC + 7) / 8;        // 41 DMA pieces of 8 px x 128 B
constexpr int kPPerWave = (kPPieces + 7) / 8;        // 6 per wave (the tail re-requests the last piece)
constexpr int kPatch = kPPieces * 1024;              // 41 984 B
constexpr int kSlab = kPx * 128;                     // [64 px][64 ch]: 8 KB
constexpr int kCM = 64, kCB = 256;
constexpr int kStepsA = 36;                          // 9 taps x 4 k16 steps
constexpr int kW2Bytes = 2 * kStepsA * 1024;         // conv2 weights, fragment-major: 72 KB
constexpr int kOffW2 = 0;
constexpr int kOffPatch = kOffW2 + kW2Bytes;
constexpr int kOffT = kOffPatch + kPatch;            // T tile
constexpr int kOffY = kOffT + kSlab;                 // Y: 4 slabs of 64 channels
constexpr int kOffBias = kOffY + 4 * kSlab;          // fp32 [64 conv2 | 256 conv3]
constexpr int kSmemTotal = kOffBias + 4096;
static_assert((kCM + kCB) * 4 <= 4096 && kSmemTotal <= 160 * 1024, "LDS budget");
constexpr int kNW = 8, kNT = 512;
constexpr int kDumpBytes = kPx * kCB * 2;            // one Y row per tile pixel: 32 KB
constexpr int kWfA3 = kW2Bytes;                      // d_wfrag (engine.pack_blk_narrow): conv3 [2 halves][4 quarters][4 steps][64][8]

struct BlkS2Dev {
    const char* in;      // bf16 [N, H+2, W+2, 64]    U
    const char* res;     // bf16 [N, H+2, W+2, 256]   X
    const char* wf;
    const float* b2;     // [64]
    const float* b3;     // [256]
    char* out;           // bf16 [N, Ho+2, Wo+2, 256] Y
    char* dump;          // >= kDumpBytes
    int N, H, W, Ho, Wo, tiles_x, tiles_per_img, tiles;
    unsigned max_pix;    // N * (H+2) * (W+2) - 1
};

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    f32x2 v = {a, b};
    bf16x2 r = __builtin_convertvector(v, bf16x2);
    return __builtin_bit_cast(unsigned, r);
}

// Vector-memory program order of a lane in tile k (after the top wait):
//   patch(k+1): 6 DMA pieces | 4 X(k+1) row loads | 4 Y row stores
// At the top of tile k+1 everything up to the last LOAD must have landed; younger than it are only the 4 stores: vmcnt(4).
// The wait never waits for a store of its own tile.
__global__ void __launch_bounds__(512, 2) conv_blk_narrow_s2_kernel(BlkS2Dev P) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, half = lane >> 5;
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
    const int Wp = P.W + 2, Wop = P.Wo + 2;
    const int G = gridDim.x;
    const int my_tiles = (P.tiles - (int)blockIdx.x + G - 1) / G;

    struct TileXY { int img, row0, col0; };             // row0, col0: OUTPUT coordinates
    auto tile_xy = [&](int t) {
        TileXY r;
        r.img = t / P.tiles_per_img;
        const int rem = t - r.img * P.tiles_per_img;
        const int ty = rem / P.tiles_x;
        r.row0 = ty * kTH;
        r.col0 = (rem - ty * P.tiles_x) * kTW;
        return r;
    };
    // tile pixel px = r * 32 + c  <->  output pixel (row0 + r, col0 + c)  <->  input pixel (2 (row0 + r), 2 (col0 + c))
    auto x_index = [&](const TileXY& T, int px) {           // haloed INPUT pixel index of the shortcut row, clamped into the image (loads)
        int r = T.row0 + (px >> 5), c = T.col0 + (px & 31);
        r = r < P.Ho ? r : P.Ho - 1;
        c = c < P.Wo ? c : P.Wo - 1;
        return (unsigned)((T.img * (P.H + 2) + 2 * r + 1) * Wp + 2 * c + 1);
    };
    auto y_index = [&](const TileXY& T, int px) {           // haloed OUTPUT pixel index (valid pixels only)
        return (unsigned)((T.img * (P.Ho + 2) + T.row0 + (px >> 5) + 1) * Wop + T.col0 + (px & 31) + 1);
    };
    auto pix_valid = [&](const TileXY& T, int px) { return T.row0 + (px >> 5) < P.Ho && T.col0 + (px & 31) < P.Wo; };

    // ---- resident operands: conv2 weights -> LDS (72 pieces of 1 KB, 9 per wave), conv3 weights -> registers, biases -> LDS
#pragma unroll
    for (int i = 0; i < 9; i++)
        __builtin_amdgcn_global_load_lds((gvoid*)(P.wf + (size_t)(wave * 9 + i) * 1024 + lane * 16), (lvoid*)(lds + kOffW2 + (wave * 9 + i) * 1024), 16, 0, 0);
    const int cq = wave & 3, pf = wave >> 2;                  // conv3: 32-channel quarter of both 128-channel halves, pixel fragment (tile row)
    const int ct = wave & 1, pt = (wave >> 1) & 1;            // phase A (waves 0-3): 32-channel half, tile row
    bf16x8 a3[8];
    {
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const char* w3 = P.wf + kWfA3 + (size_t)((h * 4 + cq) * 4 + s) * 1024 + lane * 16;
                asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(a3[h * 4 + s]) : "v"(w3) : "memory");
            }
        float* lb = (float*)(lds + kOffBias);
        if (tid < kCM) lb[tid] = P.b2[tid];
        if (tid < kCB) lb[kCM + tid] = P.b3[tid];
    }

    // ---- per-tile loads
    auto issue_patch = [&](const TileXY& T) {
        // piece pc = 8 consecutive patch pixels (pp = p * 65 + q <-> haloed input pixel (2 row0 + p, 2 col0 + q)); wave w moves
        // pieces w, w + 8, .. w + 40, clamped to the last one: every wave issues the same number of DMAs
#pragma unroll
        for (int ii = 0; ii < kPPerWave; ii++) {
            int pc = wave + kNW * ii;
            pc = pc < kPPieces ? pc : kPPieces - 1;
            int ln = lane;
            asm volatile("" : "+v"(ln));                       // addresses recomputed per tile (held across the loop they spill)
            const int pp = pc * 8 + (ln >> 3);
            const int p = (pp * 1009) >> 16;                   // pp / 65 for pp < 384
            const int q = pp - p * kPC;
            unsigned g = (unsigned)((T.img * (P.H + 2) + 2 * T.row0 + p) * Wp + 2 * T.col0 + q);
            g = g < P.max_pix ? g : P.max_pix;                 // ragged tiles (and the last piece's tail) reach past the image
            __builtin_amdgcn_global_load_lds((gvoid*)(P.in + (size_t)g * (kCM * 2) + (unsigned)(((ln & 7) ^ ((q >> 1) & 7)) * 16)),
                                             (lvoid*)(lds + kOffPatch + pc * 1024), 16, 0, 0);
        }
    };
    // shortcut rows: pass i of 4, 32 threads read one even pixel's 512 B
    u32x4 rr[4];
#pragma unroll
    for (int i = 0; i < 4; i++) rr[i] = u32x4{0u, 0u, 0u, 0u};
    auto issue_x = [&](const TileXY& T) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int idx = tid + kNT * i;
            asm volatile("" : "+v"(idx));
            const char* src = P.res + (size_t)x_index(T, idx >> 5) * (kCB * 2) + (idx & 31) * 16;
            // "+v": the destination stays the register that carries rr[] around the tile loop
            asm volatile("global_load_dwordx4 %0, %1, off nt" : "+v"(rr[i]) : "v"(src) : "memory");
        }
    };

    unsigned bs[4];                          // B fragment of k16 step s inside a [64 px][128 B] slab, pixel fragment 0
#pragma unroll
    for (int s = 0; s < 4; s++) bs[s] = (unsigned)(frow * 128 + (((2 * s + half) ^ ((frow >> 1) & 7)) * 16));
    auto barrier = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    const float* lbias = (const float*)(lds + kOffBias);

    if (my_tiles > 0) {
        const TileXY T0 = tile_xy((int)blockIdx.x);
        issue_patch(T0);
        issue_x(T0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < 8; s++) asm volatile("" : "+v"(a3[s]));

    for (int kk = 0; kk < my_tiles; kk++) {
        const int t = (int)blockIdx.x + kk * G;
        const TileXY T = tile_xy(t);
        const TileXY Tn = tile_xy(kk + 1 < my_tiles ? t + G : t);      // the last tile re-requests itself: fixed instruction count
        // ---- 1. this tile's loads have landed (only the previous tile's 4 row stores are younger)
        if (kk > 0) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        // ---- 2. shortcut rows -> the Y buffer (free since the previous tile's last barrier): [slab][px][64 ch], 16-byte chunk ^ ((px >> 1) & 7)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            asm volatile("" : "+v"(rr[i]));
            const int idx = tid + kNT * i;
            const int px = idx >> 5, j = idx & 31;
            const unsigned ad = lds_base + (unsigned)(kOffY + (j >> 3) * kSlab + px * 128 + (((j & 7) ^ ((px >> 1) & 7)) * 16));
            asm volatile("ds_write_b128 %0, %1" ::"v"(ad), "v"(rr[i]) : "memory");
        }
        barrier();       // patch k (+ weights on the first tile) visible; every wave is done with the previous tile's LDS
        // ---- 3. phase A (waves 0-3): T (32 channels ct x tile row pt) = conv2 at the even pixels of the patch, weights from LDS
        if (wave < 4) {
            f32x16 acc;
#pragma unroll
            for (int k = 0; k < 16; k++) acc[k] = 0.f;
            int fr = frow;
            asm volatile("" : "+v"(fr));
            const char* wa = lds + kOffW2 + ct * kStepsA * 1024 + lane * 16;
#pragma unroll
            for (int kh = 0; kh < 3; kh++)
#pragma unroll
                for (int kw = 0; kw < 3; kw++) {
                    const int q = kw + 2 * fr;                          // patch column of this lane's B row
                    const char* pb = lds + kOffPatch + ((2 * pt + kh) * kPC + q) * 128;
                    const int sw = (q >> 1) & 7;
                    bf16x8 af[4], bf[4];
#pragma unroll
                    for (int s = 0; s < 4; s++) {
                        af[s] = *(const bf16x8*)(wa + ((kh * 3 + kw) * 4 + s) * 1024);
                        bf[s] = *(const bf16x8*)(pb + (((2 * s + half) ^ sw) * 16));
                    }
#pragma unroll
                    for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s], bf[s], acc, 0, 0, 0);
                }
            // (acc + bias2) -> ReLU -> bf16 -> T tile
            const int px = pt * 32 + frow;
            const unsigned tb = lds_base + (unsigned)(kOffT + px * 128 + 8 * half);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const float* bp = lbias + ct * 32 + 8 * g + 4 * half;
                const float v0 = fmaxf(acc[4 * g] + bp[0], 0.f), v1 = fmaxf(acc[4 * g + 1] + bp[1], 0.f);
                const float v2 = fmaxf(acc[4 * g + 2] + bp[2], 0.f), v3 = fmaxf(acc[4 * g + 3] + bp[3], 0.f);
                u32x2 pk;
                pk.x = pack_bf16(v0, v1);
                pk.y = pack_bf16(v2, v3);
                const unsigned ad = tb + (unsigned)((((ct * 4 + g) ^ ((px >> 1) & 7))) * 16);
                asm volatile("ds_write_b64 %0, %1" ::"v"(ad), "v"(pk) : "memory");
            }
        }
        barrier();       // T complete; every wave is done with the patch
        // ---- 4. next tile's loads (the patch buffer is free; rr[] was parked in step 2)
        issue_patch(Tn);
        issue_x(Tn);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            // ---- 5. conv3: Y (32 channels cq of half h x pixel fragment pf) = W3 . T
            f32x16 acc1;
#pragma unroll
            for (int k = 0; k < 16; k++) acc1[k] = 0.f;
            bf16x8 bfr[4];
#pragma unroll
            for (int s = 0; s < 4; s++) bfr[s] = *(const bf16x8*)(lds + kOffT + pf * 4096 + bs[s]);
#pragma unroll
            for (int s = 0; s < 4; s++) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3[h * 4 + s], bfr[s], acc1, 0, 0, 0);
            // ---- 6. (acc + bias3) + X -> ReLU -> bf16, in place in the Y buffer (each lane reads and writes only its own elements)
            {
                typedef __attribute__((ext_vector_type(4))) float f32x4;
                typedef __attribute__((ext_vector_type(2))) float f32x2;
                const unsigned ebase = lds_base + (unsigned)(kOffY + (2 * h + (cq >> 1)) * kSlab + pf * 4096 + frow * 128 + 8 * half);
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const unsigned ead = ebase + (unsigned)(((((cq & 1) * 4 + g) ^ ((frow >> 1) & 7))) * 16);
                    const f32x4 bv = *(const f32x4*)(lbias + kCM + h * 128 + cq * 32 + 8 * g + 4 * half);
                    u32x2 r;
                    asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r) : "v"(ead) : "memory");
                    const f32x2 blo = {bv[0], bv[1]}, bhi = {bv[2], bv[3]};
                    const f32x2 rlo = {__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u)};
                    const f32x2 rhi = {__uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u)};
                    const f32x2 alo = {acc1[4 * g], acc1[4 * g + 1]}, ahi = {acc1[4 * g + 2], acc1[4 * g + 3]};
                    const f32x2 vlo = alo + blo + rlo, vhi = ahi + bhi + rhi;          // (acc + bias) + residual
                    r.x = pack_bf16(fmaxf(vlo[0], 0.f), fmaxf(vlo[1], 0.f));
                    r.y = pack_bf16(fmaxf(vhi[0], 0.f), fmaxf(vhi[1], 0.f));
                    asm volatile("ds_write_b64 %1, %0" ::"v"(r), "v"(ead) : "memory");
                }
            }
        }
        barrier();       // Y is complete
        // ---- 7. Y rows -> HBM: pass i of 4, 32 threads write one pixel's 512 B (exactly 4 stores per lane)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int idx = tid + kNT * i;
            asm volatile("" : "+v"(idx));
            const int px = idx >> 5, j = idx & 31;
            const u32x4 v = *(const u32x4*)(lds + kOffY + (j >> 3) * kSlab + px * 128 + (((j & 7) ^ ((px >> 1) & 7)) * 16));
            char* a = P.out + (size_t)y_index(T, px) * (kCB * 2);
            char* d = P.dump + (size_t)px * (kCB * 2);
            a = pix_valid(T, px) ? a : d;
            __builtin_nontemporal_store(v, (u32x4*)(a + j * 16));
        }
        // a slow wave's LDS reads for the row stores against a fast wave parking the next tile's rows in the same buffer
        barrier();
        __builtin_amdgcn_sched_barrier(0);
    }
    // the last tile re-requested its own patch: nothing may still be on its way into this workgroup's LDS when it is released
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

extern "C" {

size_t dafne_bottleneck_block_narrow_s2_scratch_bytes(void) { return (size_t)kDumpBytes; }

int dafne_bottleneck_block_narrow_s2_hip(const void* d_in, const void* d_res, const void* d_wfrag, const float* d_bias2,
                                         const float* d_bias3, int n_images, int H, int W, void* d_out, void* d_scratch,
                                         size_t scratch_bytes, void* stream) {
    if (!d_in || !d_res || !d_wfrag || !d_bias2 || !d_bias3 || !d_out || !d_scratch)
        return dafne::fail(DAFNE_E_INVALID, "bottleneck_block_narrow_s2: null argument");
    if (n_images < 1 || H < 1 || W < 1 || (long long)H * W > (1 << 20)) return dafne::fail(DAFNE_E_INVALID, "bottleneck_block_narrow_s2: bad size");
    if (scratch_bytes < (size_t)kDumpBytes) return dafne::fail(DAFNE_E_WORKSPACE, "bottleneck_block_narrow_s2: scratch %zu < %d", scratch_bytes, kDumpBytes);
    BlkS2Dev D;
    D.in = (const char*)d_in; D.res = (const char*)d_res; D.wf = (const char*)d_wfrag;
    D.b2 = d_bias2; D.b3 = d_bias3;
    D.out = (char*)d_out; D.dump = (char*)d_scratch;
    D.N = n_images; D.H = H; D.W = W;
    D.Ho = (H + 1) / 2; D.Wo = (W + 1) / 2;
    D.tiles_x = (D.Wo + kTW - 1) / kTW;
    D.tiles_per_img = D.tiles_x * ((D.Ho + kTH - 1) / kTH);
    const long long tiles = (long long)D.tiles_per_img * n_images;
    const long long pix = (long long)n_images * (H + 2) * (W + 2);
    if (tiles > (1ll << 24) || pix * (kCB * 2) > 0xffffffffll) return dafne::fail(DAFNE_E_UNSUPPORTED, "bottleneck_block_narrow_s2: too large");
    D.tiles = (int)tiles;
    D.max_pix = (unsigned)(pix - 1);
    DAFNE_MAX_LDS_ONCE(kSmemTotal, (const void*)conv_blk_narrow_s2_kernel);
    int n_cu = 0;
    if (int rc = dafne::device_cus(&n_cu)) return rc;
    const int grid = D.tiles < n_cu ? D.tiles : n_cu;
    hipLaunchKernelGGL(conv_blk_narrow_s2_kernel, dim3(grid), dim3(kNT), kSmemTotal, (hipStream_t)stream, D);
    return dafne::check_launch("conv_blk_narrow_s2");
}

}  // extern "C"
